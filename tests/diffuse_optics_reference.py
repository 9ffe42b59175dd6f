"""Extended-precision CPU reference of the diffuse rows along a direction in the haze optics
(sr_diffuse_optics_jacobian_rows_dev, engine.diffuse_optics_jacobian), in numpy.longdouble, with the yardstick of its
error and the case set of tests/test_diffuse_optics_host.py and tests/test_gpu_diffuse_optics.py.  A helper module: no
fixture, no pytest setting, nothing that needs a GPU.  It builds on tests/diffuse_source_reference.py and
tests/diffuse_jacobian_reference.py (imported, not edited).

The definition (the build's own; the reference tree has no counterpart).  Parameter p moves ssa_g by
dssa[p][g], asym_g by dasym[p][g] and the surface albedo by dalb[p].  The per-gas coefficients as built move by

    f = max(asym, 0)^2        df  = 2 max(asym, 0) dasym          (0 for asym <= 0)
    cs = ssa (1 - f)          dcs = dssa (1 - f) - ssa df
    ca = 1 - ssa              dca = -dssa
    cg = ssa (asym - f)       dcg = dssa (asym - f) + ssa (dasym - df)

and per layer and point, t_g = V[g][l] A[g][l][j]:  dsp = sum dcs t_g, dal = sum dca t_g, dsg = sum dcg t_g,
dD = D dlnbeam[p][l][j]; at the boundary dRb_0 = dalb[p], dUb_0 = Ub_0 dlnbeam[p][N][j] + dalb[p] max(mu0, 0) sun beam[N].
dJ is the tangent of J of the function as built, with the three rules of diffuse_jacobian_reference (the floor of co,
g = 0 where sp == 0, an empty layer); jac[ray][p][j] = sum_l Q[ray][l][j] dJ[p][l][j].

reference      the analytic tangent in long double: the definition's four sums differentiated (sigma, sigma_f, sigma_g,
               alpha), the closed forms' tangent on every layer (diffuse_jacobian_reference.layer_tangent), the adding
               recurrences with dRb and dUb seeded at the boundary.
plain64        the kernel's formulas term by term in fp64: the coefficients' tangents made first (the host plan's
               statements), the sums gas by gas on t_g, the closed forms' tangent inside a parameter's layer range (the
               layers where a gas with a non-zero coefficient tangent has a column) and dE+- = E+- dlnbeam outside it.
fd_reference   central differences of diffuse_source_reference's long-double adding form in ssa + h dssa, asym + h dasym,
               albedo + h dalb and beam exp(h dlnbeam), at diffuse_jacobian_reference's steps with two Richardson levels.

The yardstick is diffuse_jacobian_reference's, eps = 2^-53:

    b = eps (n_gas + C n_layers + 16) S,   S = sum over source layers l' (and the boundary row l' = N, which holds the
                                               albedo's direction) of |the tangent along that layer's direction alone|

with C = C_OPTICS.  Measured on the host (tests/test_diffuse_optics_host.py prints the figures): see C_OPTICS below.
"""
import numpy as np

import diffuse_jacobian_reference as DJ
import diffuse_source_reference as R

LD, EPS53 = R.LD, R.EPS53
# The layer constant of the yardstick for optics directions: twice diffuse_jacobian_reference.C_LAYER = 64, for these
# directions only.  With 64, plain64 reaches 0.75 b at the one-layer panel column (1, 3, 63, 2, 8), parameter 1: a direction
# in asym of one of three gases under a moving beam, where the asym part and the beam part of the ONE source layer have
# opposite signs (S sees their sum), and the constant 16 carries half of the bound; then 0.60 at random column 169 (an
# albedo direction, the beam held fixed); every other column stays below 0.45.  Measured against the long-double reference,
# never against the kernel.
C_OPTICS = 2 * DJ.C_LAYER
PANEL = DJ.PANEL


def bound(S, n_gas, n_layers):
    return LD(EPS53) * (n_gas + C_OPTICS * n_layers + 16) * np.asarray(S, LD)


def coefficient_tangents(ssa, asym, dssa, dasym, ft):
    """(dcs, dca, dcg) [n_par, n_gas]: the tangents of ssa (1 - f), 1 - ssa, ssa (asym - f), statement by statement as the
    host plan makes them, in ft."""
    ssa, asym, dssa, dasym = (np.asarray(x, ft) for x in (ssa, asym, dssa, dasym))
    pos = asym > 0
    f = np.where(pos, asym * asym, ft(0))
    df = np.where(pos[None, :], ft(2) * asym[None, :] * dasym, ft(0))
    return dssa * (1 - f)[None, :] - ssa[None, :] * df, -dssa, dssa * (asym - f)[None, :] + ssa[None, :] * (dasym - df)


def masks(c):
    """[n_par, 2]: per parameter the layer range lo .. hi - 1 that holds every layer in which a gas with a non-zero
    coefficient tangent has a column (0, 0: none), as the entry makes it."""
    dcs, dca, dcg = coefficient_tangents(c["ssa"], c["asym"], c["dssa"], c["dasym"], np.float64)
    moved = (dcs != 0) | (dca != 0) | (dcg != 0)                       # [n_par, n_gas]
    V = np.asarray(c["V"])
    out = np.zeros((moved.shape[0], 2), np.int64)
    for p in range(moved.shape[0]):
        hit = np.nonzero(np.any((V != 0) & moved[p][:, None], axis=0))[0]
        if hit.size:
            out[p] = hit[0], hit[-1] + 1
    return out


def _sums_kernel(c):
    """(dsp, dal, dsg) [n_par, N, n_pts] as the kernel forms them, fp64: coefficient tangents first, gases ascending."""
    A, V = np.asarray(c["A"], np.float64), np.asarray(c["V"], np.float64)
    dcs, dca, dcg = coefficient_tangents(c["ssa"], c["asym"], c["dssa"], c["dasym"], np.float64)
    z = np.zeros((dcs.shape[0],) + A.shape[1:])
    dsp, dal, dsg = z.copy(), z.copy(), z.copy()
    for g in range(A.shape[0]):
        t = (V[g][:, None] * A[g])[None]
        dsp = dsp + dcs[:, g, None, None] * t
        dal = dal + dca[:, g, None, None] * t
        dsg = dsg + dcg[:, g, None, None] * t
    return dsp, dal, dsg


def _sums_definition(c):
    """The same three rows from the definition's four sums differentiated, long double."""
    A, V, ssa, asym, dssa, dasym = (np.asarray(c[k], LD) for k in ("A", "V", "ssa", "asym", "dssa", "dasym"))
    pos = asym > 0
    f = np.where(pos, asym * asym, LD(0))
    df = np.where(pos[None, :], 2 * asym[None, :] * dasym, LD(0))
    z = np.zeros((dssa.shape[0],) + A.shape[1:], LD)
    dsig, dal, dsf, dsgm = z.copy(), z.copy(), z.copy(), z.copy()
    for g in range(A.shape[0]):
        t = (V[g][:, None] * A[g])[None]
        dsig = dsig + dssa[:, g, None, None] * t
        dal = dal - dssa[:, g, None, None] * t
        dsf = dsf + (dssa[:, g] * f[g] + ssa[g] * df[:, g])[:, None, None] * t
        dsgm = dsgm + (dssa[:, g] * asym[g] + ssa[g] * dasym[:, g])[:, None, None] * t
    return dsig - dsf, dal, dsgm - dsf


def _tangent(sp, al, sg, dsp, dal, dsg, beam, sun, dlnb, dalb, mu0, albedo, ft, mask=None, split=False):
    """diffuse_jacobian_reference._tangent with the boundary's own direction: dRb_0 = dalb, dUb_0 = Ub_0 dlnb[N] + dalb
    max(mu0, 0) sun beam[N] (split: both in the boundary row l' = N).  The adding step and the downward sweep are its
    statements unchanged -- they already take a non-zero dRb from below."""
    N, n_pts = sp.shape
    n_par = dsp.shape[0]
    K = N + 1 if split else 1
    beam, sun, dlnb, dalb = np.asarray(beam, ft), np.asarray(sun, ft), np.asarray(dlnb, ft), np.asarray(dalb, ft)
    albedo_, mu0_ = ft(albedo), ft(mu0)

    def embed(x, l):
        if not split:
            return x[:, None, :]
        z = np.zeros((n_par, K, n_pts), ft)
        z[:, l, :] = x
        return z

    Rb = np.full((n_pts,), albedo_, ft)
    Cb = np.full((n_pts,), 1 - albedo_, ft)
    lit = max(mu0_, ft(0)) * (sun * beam[N])
    Ub = albedo_ * lit
    dRb = embed(dalb[:, None] * np.ones((1, n_pts), ft), N)
    dUb = embed(Ub[None, :] * dlnb[:, N, :] + dalb[:, None] * lit[None, :], N)
    keep = []
    for l in range(N):
        D = sun * beam[l]
        o = R.layer_operators(sp[l], al[l], sg[l], D, mu0, ft)
        dlb = dlnb[:, l, :]
        t = DJ.layer_tangent(sp[l][None], al[l][None], sg[l][None], D[None], mu0, dsp[:, l], dal[:, l], dsg[:, l], D[None] * dlb, ft)
        if mask is not None:
            inside = ((l >= mask[:, 0]) & (l < mask[:, 1]))[:, None]
            zero = np.zeros((n_par, n_pts), ft)
            t = {key: np.where(inside, t[key], {"Ep": o["Ep"][None] * dlb, "Em": o["Em"][None] * dlb}.get(key, zero)) for key in t}
        t = {key: embed(val, l) for key, val in t.items()}
        live = o["live"]
        q = np.where(live, 1 / np.where(live, Cb + Rb * o["oneR"], ft(1)), ft(1))
        tq, cn, wv = o["T"] * q, o["Em"] + o["R"] * Ub, Ub + Rb * o["Em"]
        cn2 = o["oneR"] * Cb + Rb * o["absb"] * (o["oneR"] + o["T"])
        z = np.where(live, (Cb + Rb * o["absb"]) * q, ft(0))
        dq = np.where(live, (q * q) * (dRb * o["R"] + Rb * t["R"]), ft(0))
        bA, mA = t["T"] + tq * (dRb * o["R"] + Rb * t["R"]), np.abs(t["T"]) + tq * (np.abs(dRb) * o["R"] + Rb * np.abs(t["R"]))
        bB, mB = (tq * o["R"] * dRb - t["R"] * z) - t["absb"], (tq * o["R"] * np.abs(dRb) + np.abs(t["R"]) * z) + np.abs(t["absb"])
        dtq = q * np.where(mA <= mB, bA, bB)
        keep.append((tq, cn * q, Rb, Ub, dtq, (t["Em"] + (t["R"] * Ub + o["R"] * dUb)) * q + cn * dq, dRb, dUb))
        dwv = dUb + (dRb * o["Em"] + Rb * t["Em"])
        dUb, dRb = (t["Ep"] + (o["T"] * dwv * q + wv * dtq),
                    o["T"] * Rb * dtq + ((t["R"] * z - o["T"] * Rb * q * t["absb"]) + o["T"] * o["T"] * q * dRb))
        Ub, Cb, Rb = o["Ep"] + o["T"] * wv * q, cn2 * q, o["R"] + o["T"] * o["T"] * Rb * q
    if ft is np.float64:        # the kernel's constant
        kJ = np.float64(1.7320508075688772) / (8.0 * 3.141592653589793)
    else:
        kJ = np.sqrt(LD(3)) / (8 * (4 * np.arctan(LD(1))))
    fm = np.zeros((n_pts,), ft)
    dfp, dfm = dUb, np.zeros((n_par, K, n_pts), ft)
    dJ = np.zeros((n_par, K, N, n_pts), ft)
    for l in range(N - 1, -1, -1):
        tq, cq, rb, ub, dtq, dcq, drb, dub = keep[l]
        fm_l = tq * fm + cq
        dfm_l = (dtq * fm + tq * dfm) + dcq
        dfp_l = dub + (drb * fm_l + rb * dfm_l)
        dJ[:, :, l, :] = kJ * ((dfp_l + dfm_l) + (dfp + dfm))
        dfp, dfm, fm = dfp_l, dfm_l, fm_l
    return dJ if split else dJ[:, 0]


def _filled(c):
    """The case with every direction present: a None is zeros."""
    n_gas, N, n_pts = c["A"].shape
    n_par = next(np.asarray(c[k]).shape[0] for k in ("dssa", "dasym", "dalb") if c.get(k) is not None)
    out = dict(c)
    for k, shape in (("dssa", (n_par, n_gas)), ("dasym", (n_par, n_gas)), ("dalb", (n_par,)), ("dlnbeam", (n_par, N + 1, n_pts))):
        if out.get(k) is None:
            out[k] = np.zeros(shape)
    return out


def reference(c, yardstick=False):
    """dict(dJ [n_par, N, n_pts], jac [n_rays, n_par, n_pts]) of a case (dict: the forward case plus dssa, dasym, dalb,
    dlnbeam, Q; any of them may be None), in long double; yardstick=True: also S_dJ and S_jac."""
    c = _filled(c)
    sp, al, sg = R.optics_definition(c["A"], c["V"], c["ssa"], c["asym"], LD)
    a = (sp, al, sg) + _sums_definition(c) + (c["beam"], c["sun"], c["dlnbeam"], c["dalb"], c["mu0"], c["albedo"], LD)
    dJ = _tangent(*a)
    out = dict(dJ=dJ)
    Q = c.get("Q")
    if Q is not None:
        out["jac"] = DJ.contract(Q, dJ, LD)
    if yardstick:
        parts = _tangent(*a, split=True)                # [n_par, N + 1, N, n_pts]
        out["S_dJ"] = np.sum(np.abs(parts), axis=1)
        if Q is not None:
            out["S_jac"] = np.sum(np.abs(np.einsum("rlj,pklj->rpkj", np.asarray(Q, LD), parts)), axis=2)
    return out


def plain64(c):
    """The kernel's formulas term by term in fp64: dict(dJ, jac)."""
    c = _filled(c)
    sp, al, sg = R.optics_kernel(c["A"], c["V"], c["ssa"], c["asym"])
    dJ = _tangent(sp, al, sg, *_sums_kernel(c), c["beam"], c["sun"], c["dlnbeam"], c["dalb"], c["mu0"], c["albedo"], np.float64,
                  mask=masks(c))
    out = dict(dJ=dJ)
    if c.get("Q") is not None:
        out["jac"] = DJ.contract(c["Q"], dJ, np.float64)
    return out


def fd_reference(c, p=0):
    """(dJ [N, n_pts] of parameter p by central differences and two Richardson levels, |r1b - r1a|), long double: only
    diffuse_source_reference's adding form is evaluated, at ssa + h dssa, asym + h dasym, albedo + h dalb and
    beam exp(h dlnbeam).  The steps, the levels and the self-consistency are diffuse_jacobian_reference.fd_reference's."""
    c = _filled(c)
    ssa, asym, beam = (np.asarray(c[k], LD) for k in ("ssa", "asym", "beam"))
    dssa, dasym, dalb, dlnb = (np.asarray(c[k], LD)[p] for k in ("dssa", "dasym", "dalb", "dlnbeam"))

    def J(h):
        h = LD(h)
        sp, al, sg = R.optics_definition(c["A"], c["V"], ssa + h * dssa, asym + h * dasym, LD)
        return R._adding(sp, al, sg, beam * np.exp(h * dlnb), c["sun"], c["mu0"], LD(c["albedo"]) + h * dalb, LD)[1]

    D = [(J(h) - J(-h)) / (2 * LD(h)) for h in DJ.FD_STEPS]
    r1a, r1b = (4 * D[1] - D[0]) / 3, (4 * D[2] - D[1]) / 3
    return (16 * r1b - r1a) / 15, np.abs(r1b - r1a)


def directions(rng, c, n_par, n_rays):
    """The case c with dssa, dasym [n_par, n_gas], dalb [n_par], dlnbeam [n_par, N + 1, n_pts] and Q [n_rays, N, n_pts]
    (None for n_rays = 0), mixed over the three kinds: parameter p moves ssa of a random gas (p % 3 == 0), asym of a
    random gas (1) or the albedo alone (2: an empty layer range); from the fourth parameter on, every third moves all three
    at once on every gas.  Either sign, sizes 0.2 .. 1.  dlnbeam is random in [-1, 1]; parameter 2, an albedo direction,
    holds the beam fixed.

    What the yardstick's S does not see, as in diffuse_jacobian_reference: parts that cancel inside ONE source layer.  So an
    ssa direction gives dlnbeam its own sign on every row (more scattering, more J: one sign with a brighter beam), and an
    albedo direction gives the boundary row its sign (both stand in that row).  A direction in asym ALONE with the beam held
    fixed is not among them: it moves light between the two streams, dJ changes sign with height, and where it does S = |dJ|
    itself is 0 pointwise while every arithmetic's error stays that of the addends (measured on such columns: plain64 within
    1e-15 of the column's largest |dJ|, at 1e13 b) -- no constant covers a zero of S.  Asym directions here come with a
    moving beam, whose rows carry S; the pure one is pinned by differences and exact cases in the tests."""
    n_gas, N, n_pts = c["A"].shape
    dssa, dasym, dalb = np.zeros((n_par, n_gas)), np.zeros((n_par, n_gas)), np.zeros(n_par)
    size = lambda *s: rng.uniform(0.2, 1.0, s) * rng.choice([-1.0, 1.0], s)
    dlnbeam = rng.uniform(-1.0, 1.0, (n_par, N + 1, n_pts))
    for p in range(n_par):
        g = int(rng.integers(n_gas))
        if p >= 3 and p % 3 == 0:
            dssa[p], dasym[p], dalb[p] = size(n_gas), size(n_gas), size()
        elif p % 3 == 0:
            dssa[p, g] = size()
            dlnbeam[p] = np.abs(dlnbeam[p]) * np.sign(dssa[p, g])
        elif p % 3 == 1:
            dasym[p, g] = size()
        else:
            dalb[p] = size()
            dlnbeam[p, N] = np.abs(dlnbeam[p, N]) * np.sign(dalb[p])
    if n_par >= 3:
        dlnbeam[2] = 0.0
    Q = rng.uniform(0.1, 1.0, (n_rays, N, n_pts)) if n_rays else None
    return dict(c, dssa=dssa, dasym=dasym, dalb=dalb, dlnbeam=dlnbeam, Q=Q)


def panel_case(n_layers, n_gas, n_pts, n_par, n_rays):
    """One case of the GPU bound panel: the forward op's panel case with optics directions."""
    rng = np.random.default_rng([20261023, n_layers, n_gas, n_pts, n_par, n_rays])
    return directions(rng, R.panel_case(n_layers, n_gas, n_pts), n_par, n_rays)


def pure_asym_case(n_layers, n_gas, n_pts, n_par, n_rays):
    """The panel case with pure asym directions: every parameter moves asym alone (of one gas, or from the fourth on of every
    gas), the beam held fixed -- what S cannot bound pointwise (directions' docstring)."""
    rng = np.random.default_rng([20261023, 5, n_layers, n_gas, n_pts, n_par, n_rays])
    c = directions(rng, R.panel_case(n_layers, n_gas, n_pts), n_par, n_rays)
    dasym = np.zeros((n_par, n_gas))
    for p in range(n_par):
        if p >= 3:
            dasym[p] = rng.uniform(0.2, 1.0, n_gas) * rng.choice([-1.0, 1.0], n_gas)
        else:
            dasym[p, int(rng.integers(n_gas))] = rng.uniform(0.2, 1.0) * rng.choice([-1.0, 1.0])
    return dict(c, dssa=None, dasym=dasym, dalb=None, dlnbeam=None)


def column_bound(ref, Q, n_gas, n_layers):
    """dict(dJ, jac) from reference(c, yardstick=True): the yardstick b with, per (parameter, point), the LARGEST S over the
    layers of the column in place of the pointwise S (for jac times sum_l Q[ray, l]).  For a direction whose dJ changes
    sign with height: S -- the sum over the source layers of |that layer's own tangent| -- has a zero wherever every source
    layer's tangent crosses zero at the same height, and the crossing moves with the rounding of the layers around it, so
    what an arithmetic can hold there is the column's scale, not the point's.  C_OPTICS as for every optics direction."""
    top = np.max(np.asarray(ref["S_dJ"], LD), axis=1, keepdims=True)                 # [n_par, 1, n_pts]
    fac = LD(EPS53) * (n_gas + C_OPTICS * n_layers + 16)
    out = dict(dJ=fac * np.broadcast_to(top, np.asarray(ref["dJ"]).shape))
    if Q is not None:
        out["jac"] = fac * np.asarray(Q, LD).sum(axis=1)[:, None, :] * top[None, :, 0, :]
    return out


def random_columns(n=300, seed=17):
    """The 300 random columns of the host test: N from 1 to 80, two points, one to five parameters, two rays."""
    rng = np.random.default_rng([20261023, seed])
    for i in range(n):
        n_layers = int(rng.choice([1, 2, 3, 5, 12, 17, 40, 80])) if i % 3 else int(rng.integers(1, 81))
        yield directions(rng, R.column_case(rng, n_layers, int(rng.integers(1, 9)), 2), int(rng.integers(1, 6)), 2)


def fd_columns(n=40, seed=19):
    """The columns of the difference check: N <= 17, n_gas <= 3, values away from the kinks so that the differences are
    clean -- ssa in [0.05, 0.95], |asym| in [0.05, 0.9] with asym >= -0.4, albedo in [0.05, 0.95] -- one parameter that
    moves all three quantities and ln beam."""
    rng = np.random.default_rng([20261023, seed])
    for i in range(n):
        n_gas = int(rng.integers(1, 4))
        c = R.column_case(rng, int(rng.integers(1, 18)), n_gas, 2)
        asym = rng.uniform(0.05, 0.9, n_gas) * rng.choice([-1.0, 1.0], n_gas)
        c = dict(c, ssa=rng.uniform(0.05, 0.95, n_gas), asym=np.maximum(asym, -0.4), albedo=float(rng.uniform(0.05, 0.95)))
        c = directions(rng, c, 4, 0)
        yield dict(c, dssa=c["dssa"][3:], dasym=c["dasym"][3:], dalb=c["dalb"][3:], dlnbeam=np.ascontiguousarray(c["dlnbeam"][3:]))
