"""Extended-precision CPU reference of the diffuse rows in the Jacobians (sr_diffuse_jacobian_rows_dev,
engine.diffuse_jacobian), in numpy.longdouble, with the yardstick of its error and the case set of
tests/test_diffuse_jacobian_host.py and tests/test_gpu_diffuse_jacobian.py.  A helper module: no fixture, no pytest
setting, nothing that needs a GPU.  It builds on tests/diffuse_source_reference.py (imported, not edited).

The definition (the build's own; the reference tree has no counterpart).  In the notation of
diffuse_source_reference a parameter x_p moves, per layer l and grid point j,

    d t_g[l] = dV[p][g][l] A[g][l][j],   d D_l = D_l dlnbeam[p][l][j],   d Ub_0 = Ub_0 dlnbeam[p][N][j]

and dJ[p][l][j] is the tangent of J_l of the function as built: co = max(al / dtau, 2^-52) has derivative 0 where the floor
holds, g = 0 where sp == 0 has derivative 0 there, a layer with dtau == 0 passes light through whatever dV says (every
operator derivative 0).  jac[ray][p][j] = sum_l Q[ray][l][j] dJ[p][l][j].

reference      the analytic tangent in long double: every quantity of the layer operators and of the two sweeps with its
               tangent beside it, the closed forms' tangent on every layer.
plain64        the kernel's formulas term by term in fp64: the per-gas coefficients made first, the closed forms' tangent
               inside a parameter's layer range and dE+- = E+- dlnbeam outside it, the layer sum ascending from 0.
fd_reference   central differences of diffuse_source_reference's long-double adding form at the steps 1e-3, 5e-4, 2.5e-4
               of V + h dV and beam exp(h dlnbeam), with two Richardson levels; returns the last level and the agreement
               of the two values of the level before (the self-consistency).  Independent of every tangent formula here.

Measured on the host (tests/test_diffuse_jacobian_host.py prints them), 40 random columns of column_case (N <= 17,
n_gas <= 3, one gas's V moved on three layers and ln beam on all), in units of the column's largest |dJ|:
|r1b - r1a| 6.6e-15 (the agreement of the two first-level values, fd_reference's docstring; the distance of the last two
levels, |r2 - r1b|, is a fifteenth of it, 4.4e-16), |reference - fd_reference| 5.6e-15 = 0.86 |r1b - r1a| (the assertion:
<= 2 |r1b - r1a|; 10 |r2 - r1b| = 0.67 |r1b - r1a| lies below r2's own rounding and is printed: 12.9).

The yardstick is the project's convention, the sum of the absolute addends, pointwise, eps = 2^-53:

    b = eps (n_gas + C_LAYER n_layers + 16) S,   S[ray, p, j] = sum_{l'} | sum_l Q[ray, l, j] dJ_l restricted to source layer l' |

the tangent run once per source layer l' (dV and dlnbeam of that layer alone) plus the boundary row (l' = N); for dJ
itself Q is the unit row.  C_LAYER = 64 was set so that plain64 stays at <= 0.5 of b over the panel and 300 random
columns.  Measured: plain64 / b <= 0.49 on the host (dJ 0.487 at random column 41: five thin lossless layers, co 7e-12,
under a beam of 3e-9 at the moved layer, where a scatterer's column moves T down and R up alike and
dJ_l = kJ (dF+_l + dF-_l + dF+_{l+1} + dF-_{l+1}) is a hundredth of its addends -- the sum of the two interfaces'
fluxes, no closed form's cancellation; then random column 110, three layers of optical depth 54, at 82 eps; every other
column needs C <= 12; jac 0.140).  The GPU test asserts <= 1 (the factor 2 for the device's exp / sqrt / division) and
measured 0.105 on the MI355X (jac 0.105, dJ 0.096, one-layer columns of the panel; 0.014 at 80 layers).

What S does not see: a direction whose parts cancel INSIDE one source layer -- a gas's column against its own shadow in
dlnbeam (J ~ V beam: d ln V = -d ln beam to four digits turned up among 300 columns), or the scattering against the
absorption of one gas -- is conditioned worse than S says by the cancellation's factor, in any arithmetic that rounds the
per-gas coefficients before it forms the sums.  `directions` therefore gives dlnbeam on a parameter's own layers the sign
of its dV, and Q >= 0 as the derivative of a radiance to an emission is (a signed Q cancels in the layer sum itself).
The sign pattern a scene makes is pinned beside that: `physical_directions` (dlnbeam the shadow of the parameter's own
column, opposite to its dV) against the yardstick BY PARTS, reference(c, yardstick="parts"), in which the dV part and the
dlnbeam part of a source layer are addends of their own, with the same C_LAYER: plain64 0.42 over the panel and 100
random columns (bound 0.5), MI355X 0.079 over five panel shapes (bound 1).
"""
import numpy as np

import diffuse_source_reference as R

LD, EPS53, CO_MIN = R.LD, R.EPS53, R.CO_MIN
C_LAYER = 64
PAR_TILE, RAY_TILE = 4, 8       # kDiffuseJacPars, kDiffuseJacRays: the panel crosses both

# the bound panel of the GPU test: (n_layers, n_gas, n_pts, n_par, n_rays), every value of the issue's five lists
PANEL = ((1, 1, 1, 1, 1), (1, 3, 63, 2, 8), (1, 8, 257, 5, 9), (1, 1, 65, 9, 1),
         (2, 1, 63, 5, 9), (2, 3, 1, 9, 8), (2, 8, 65, 1, 1), (2, 3, 257, 2, 9),
         (3, 1, 257, 2, 1), (3, 3, 65, 5, 8), (3, 8, 1, 9, 9), (3, 8, 63, 1, 8),
         (17, 1, 65, 9, 9), (17, 3, 257, 5, 8), (17, 8, 63, 2, 1), (17, 3, 1, 1, 9), (17, 8, 257, 9, 8),
         (80, 1, 63, 1, 9), (80, 3, 65, 9, 9), (80, 8, 1, 5, 1), (80, 3, 257, 2, 8), (80, 8, 65, 5, 9), (80, 1, 1, 9, 8))


def bound(S, n_gas, n_layers):
    return LD(EPS53) * (n_gas + C_LAYER * n_layers + 16) * np.asarray(S, LD)


def masks(dV, V):
    """[n_par, 2]: per parameter the layer range lo .. hi - 1 that holds every non-zero dV[p, :, l] of a layer with any
    column (0, 0: none), as the entry makes it."""
    dV = np.asarray(dV)
    filled = np.any(np.asarray(V) != 0, axis=0)
    out = np.zeros((dV.shape[0], 2), np.int64)
    for p in range(dV.shape[0]):
        hit = np.nonzero(np.any(dV[p] != 0, axis=0) & filled)[0]
        if hit.size:
            out[p] = hit[0], hit[-1] + 1
    return out


def even_functions(y, ft):
    """(e, Sh, Ch, c2, W, c2p): exp(-x) and, each times it, sinh(x) / x, cosh x, (cosh x - 1) / y, (cosh x - sinh(x) / x) / y and
    d((cosh x - 1) / y) / dy at x = sqrt(y), as the kernel's diffuse_even makes them for y < 4: power series in y (fourteen
    terms in fp64; twenty in long double, where the next is below 1e-33 of the sum)."""
    y = np.asarray(y, ft)
    e = np.exp(-np.sqrt(y))
    a, S, c2, W, c2p = np.ones_like(y), np.zeros_like(y), np.zeros_like(y), np.zeros_like(y), np.zeros_like(y)
    for n in range(14 if ft is np.float64 else 20):
        S = S + a
        c2 = c2 + a * (ft(1) / (2 * n + 2))
        W = W + a * (ft(1) / (2 * n + 3))
        c2p = c2p + a * (ft(1) / (ft(2) * (2 * n + 3) * (2 * n + 4)))
        a = a * (y * (ft(1) / ((ft(2) * n + 2) * (2 * n + 3))))
    return e, e * S, e * (1 + y * c2), e * c2, e * W, e * c2p


def layer_tangent(sp, al, sg, D, mu0, dsp, dal, dsg, dD, ft):
    """dict(R, T, Ep, Em, absb) of the tangent of layer_operators along (dsp, dal, dsg, dD), arrays that broadcast,
    in ft: the kernel's diffuse_layer_tangent, statement by statement -- the operators' even forms in k (T = 1 / Delta,
    R = gamma2 dtau (sinh(x) / x) / Delta, E+ + E- = D (omega dtau) An, E+ - E- = -sqrt3 mu0 D (omega g dtau) Bn,
    1 - R - T = d dtau An), whose tangents do not go through d sqrt(co), with co dtau = al, omega dtau = sp and
    omega g dtau = sg above the floor."""
    dtau = sp + al
    live = dtau > 0
    one = ft(1)
    sdt = np.where(live, dtau, one)
    ddtau = dsp + dal
    fl = ~(np.where(live, al, one) / sdt > ft(CO_MIN))
    om = 1 - ft(CO_MIN)
    cd, dcd = np.where(fl, ft(CO_MIN) * sdt, al), np.where(fl, ft(CO_MIN) * ddtau, dal)
    od, dod = np.where(fl, om * sdt, sp), np.where(fl, om * ddtau, dsp)
    sc = sp > 0
    ssp = np.where(sc, sp, one)
    g = np.where(sc, sg / ssp, ft(0))
    dg = np.where(sc, (dsg - g * dsp) / ssp, ft(0))
    go = np.where(fl, g * od, np.where(sc, sg, ft(0)))
    dgo = np.where(fl, dg * od + g * dod, np.where(sc, dsg, ft(0)))
    r3 = np.sqrt(ft(3))
    bd, dbd = r3 * cd, r3 * dcd
    bs, dbs = r3 * (sdt - go), r3 * (ddtau - dgo)
    y, dy = bd * bs, dbd * bs + bd * dbs
    a1, da1 = (bs + bd) / 2, (dbs + dbd) / 2
    a2, da2 = (r3 * (od - go)) / 2, (r3 * (dod - dgo)) / 2
    small = y < 4
    # y < 4: the series; tangents of the functions themselves, each times e
    ys, dys = np.where(small, y, ft(0)), np.where(small, dy, ft(0))
    e, Sh, Ch, c2, W, c2p = even_functions(ys, ft)
    rD = 1 / (Ch + a1 * Sh)
    dSh = (W * dys) / 2
    dDh = (Sh * dys) / 2 + (da1 * Sh + a1 * dSh)
    T, Rv = e * rD, a2 * Sh * rD
    tT_s = -(T * dDh * rD)
    tR_s = ((da2 * Sh + a2 * dSh) - Rv * dDh) * rD
    c2y = c2p * dys
    An_s, Bn_s = (bs * c2 + Sh) * rD, (bd * c2 + Sh) * rD
    dAn_s = (((dbs * c2 + bs * c2y) + dSh) - An_s * dDh) * rD
    dBn_s = (((dbd * c2 + bd * c2y) + dSh) - Bn_s * dDh) * rD
    # a thick layer: the tangents of the SCALED functions e f, in which dtau is left in e^-x and e^-2x alone
    yl, dyl = np.where(small, ft(4), y), np.where(small, ft(0), dy)
    x = np.sqrt(yl)
    dx = dyl / 2 / x
    e = np.exp(-x)
    e2 = e * e
    Ch, dCh = (1 + e2) / 2, -(e2 * dx)
    Sh = (1 - e2) / 2 / x
    dSh = (e2 * dx - Sh * dx) / x
    c2 = (Ch - e) / yl
    dc2 = ((dCh + e * dx) - c2 * dyl) / yl
    rD = 1 / (Ch + a1 * Sh)
    dDh = dCh + (da1 * Sh + a1 * dSh)
    T, Rv = e * rD, a2 * Sh * rD
    tT_l = -((e * dx + T * dDh) * rD)
    tR_l = ((da2 * Sh + a2 * dSh) - Rv * dDh) * rD
    An_l, Bn_l = (bs * c2 + Sh) * rD, (bd * c2 + Sh) * rD
    dAn_l = (((dbs * c2 + bs * dc2) + dSh) - An_l * dDh) * rD
    dBn_l = (((dbd * c2 + bd * dc2) + dSh) - Bn_l * dDh) * rD
    pick = lambda lo, hi: np.where(small, lo, hi)
    tT, tR, An, Bn, dAn, dBn = pick(tT_s, tT_l), pick(tR_s, tR_l), pick(An_s, An_l), pick(Bn_s, Bn_l), pick(dAn_s, dAn_l), pick(dBn_s, dBn_l)
    des = (dD * od + D * dod) * An + D * od * dAn
    c = r3 * ft(mu0)
    ded = -(c * ((dD * go + D * dgo) * Bn + D * go * dBn))
    t = dict(R=tR, T=tT, Ep=(des + ded) / 2, Em=(des - ded) / 2, absb=dbd * An + bd * dAn)
    return {key: np.where(live, val, ft(0)) for key, val in t.items()}


def _sums(A, dV, ssa, asym, ft, kernel):
    """(dsp, dal, dsg) [n_par, N, n_pts] of the directions, by the definition's sums (ft) or the kernel's coefficients."""
    A, dV = np.asarray(A, ft), np.asarray(dV, ft)
    out = []
    for p in range(dV.shape[0]):
        out.append(R.optics_kernel(A, dV[p], ssa, asym) if kernel else R.optics_definition(A, dV[p], ssa, asym, ft))
    return tuple(np.stack([o[i] for o in out]) for i in range(3))


def _tangent(sp, al, sg, dsp, dal, dsg, beam, sun, dlnb, mu0, albedo, ft, mask=None, split=False):
    """dJ of every direction, in ft.  sp, al, sg [N, n_pts]; dsp, dal, dsg [n_par, N, n_pts]; dlnb [n_par, N + 1, n_pts].
    mask [n_par, 2]: the closed forms' tangent inside a parameter's range and dE+- = E+- dlnb outside it, as the kernel
    does; None: the closed forms' tangent on every layer.  split: the direction of every source layer l' (and the
    boundary, l' = N) alone -- returns [n_par, N + 1, N, n_pts]; else [n_par, N, n_pts]."""
    N, n_pts = sp.shape
    n_par = dsp.shape[0]
    K = N + 1 if split else 1
    beam, sun, dlnb = np.asarray(beam, ft), np.asarray(sun, ft), np.asarray(dlnb, ft)
    albedo_, mu0_ = ft(albedo), ft(mu0)

    def embed(x, l):            # a layer's tangent [n_par, n_pts] as the carried shape [n_par, K, n_pts]
        if not split:
            return x[:, None, :]
        z = np.zeros((n_par, K, n_pts), ft)
        z[:, l, :] = x
        return z

    Rb = np.full((n_pts,), albedo_, ft)
    Cb = np.full((n_pts,), 1 - albedo_, ft)
    Ub = albedo_ * (max(mu0_, ft(0)) * (sun * beam[N]))
    dRb = np.zeros((n_par, K, n_pts), ft)
    dUb = embed(Ub[None, :] * dlnb[:, N, :], N)
    keep = []
    for l in range(N):
        D = sun * beam[l]
        o = R.layer_operators(sp[l], al[l], sg[l], D, mu0, ft)
        dlb = dlnb[:, l, :]
        t = layer_tangent(sp[l][None], al[l][None], sg[l][None], D[None], mu0, dsp[:, l], dal[:, l], dsg[:, l], D[None] * dlb, ft)
        if mask is not None:
            inside = ((l >= mask[:, 0]) & (l < mask[:, 1]))[:, None]
            zero = np.zeros((n_par, n_pts), ft)
            t = {key: np.where(inside, t[key], {"Ep": o["Ep"][None] * dlb, "Em": o["Em"][None] * dlb}.get(key, zero)) for key in t}
        t = {key: embed(val, l) for key, val in t.items()}
        live = o["live"]
        q = np.where(live, 1 / np.where(live, Cb + Rb * o["oneR"], ft(1)), ft(1))
        tq, cn, wv = o["T"] * q, o["Em"] + o["R"] * Ub, Ub + Rb * o["Em"]
        cn2 = o["oneR"] * Cb + Rb * o["absb"] * (o["oneR"] + o["T"])
        # Cb = 1 - Rb: dCb = -dRb is not carried.  z = 1 - T q Rb as a sum; d(T q) through d(1 - R - T) and z (see the kernel)
        z = np.where(live, (Cb + Rb * o["absb"]) * q, ft(0))
        dq = np.where(live, (q * q) * (dRb * o["R"] + Rb * t["R"]), ft(0))
        tqr = o["T"] * q
        bA, mA = t["T"] + tqr * (dRb * o["R"] + Rb * t["R"]), np.abs(t["T"]) + tqr * (np.abs(dRb) * o["R"] + Rb * np.abs(t["R"]))
        bB, mB = (tqr * o["R"] * dRb - t["R"] * z) - t["absb"], (tqr * o["R"] * np.abs(dRb) + np.abs(t["R"]) * z) + np.abs(t["absb"])
        dtq = q * np.where(mA <= mB, bA, bB)         # the form whose addends are smaller: dT under a thick layer, dabsb in a lossless one
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


def contract(Q, dJ, ft):
    """jac [n_rays, n_par, n_pts] = sum_l Q[ray, l] dJ[p, l], l ascending from 0, in ft."""
    Q, dJ = np.asarray(Q, ft), np.asarray(dJ, ft)
    out = np.zeros((Q.shape[0], dJ.shape[0], Q.shape[2]), ft)
    for l in range(Q.shape[1]):
        out = out + Q[:, None, l, :] * dJ[None, :, l, :]
    return out


def _dlnb(c, dlnbeam):
    n_par, (N, n_pts) = np.asarray(c["dV"]).shape[0], c["A"].shape[1:]
    return np.zeros((n_par, N + 1, n_pts)) if dlnbeam is None else dlnbeam


def reference(c, yardstick=False):
    """dict(dJ [n_par, N, n_pts], jac [n_rays, n_par, n_pts]) of a case (dict: the forward case plus dV, dlnbeam, Q; Q or
    dlnbeam may be None), in long double; yardstick=True: also S_dJ and S_jac, the sums of the absolute addends per source
    layer; yardstick="parts": per source layer AND part, the dV part and the dlnbeam part of a layer as addends of their
    own (physical_directions, whose two parts have opposite signs)."""
    sp, al, sg = R.optics_definition(c["A"], c["V"], c["ssa"], c["asym"], LD)
    dsp, dal, dsg = _sums(c["A"], c["dV"], c["ssa"], c["asym"], LD, False)
    a = (sp, al, sg, dsp, dal, dsg, c["beam"], c["sun"], _dlnb(c, c.get("dlnbeam")), c["mu0"], c["albedo"], LD)
    dJ = _tangent(*a)
    out = dict(dJ=dJ)
    Q = c.get("Q")
    if Q is not None:
        out["jac"] = contract(Q, dJ, LD)
    if yardstick == "parts":
        zero = np.zeros_like(dsp)
        parts = np.concatenate([_tangent(*(a[:6] + a[6:8] + (np.zeros_like(a[8]),) + a[9:]), split=True),
                                _tangent(*(a[:3] + (zero, zero, zero) + a[6:]), split=True)], axis=1)
    elif yardstick:
        parts = _tangent(*a, split=True)                # [n_par, N + 1, N, n_pts]
    if yardstick:
        out["S_dJ"] = np.sum(np.abs(parts), axis=1)
        if Q is not None:
            out["S_jac"] = np.sum(np.abs(np.einsum("rlj,pklj->rpkj", np.asarray(Q, LD), parts)), axis=2)
    return out


def plain64(c):
    """The kernel's formulas term by term in fp64: dict(dJ, jac)."""
    sp, al, sg = R.optics_kernel(c["A"], c["V"], c["ssa"], c["asym"])
    dsp, dal, dsg = _sums(c["A"], c["dV"], c["ssa"], c["asym"], np.float64, True)
    dJ = _tangent(sp, al, sg, dsp, dal, dsg, c["beam"], c["sun"], _dlnb(c, c.get("dlnbeam")), c["mu0"], c["albedo"], np.float64,
                  mask=masks(c["dV"], c["V"]))
    out = dict(dJ=dJ)
    if c.get("Q") is not None:
        out["jac"] = contract(c["Q"], dJ, np.float64)
    return out


FD_STEPS = (1e-3, 5e-4, 2.5e-4)


def fd_reference(c, p=0):
    """(dJ [N, n_pts] of parameter p by central differences and two Richardson levels, the self-consistency of the
    differences), long double.  Independent of the tangent formulas: only diffuse_source_reference's adding form is
    evaluated.  With D0, D1, D2 the differences at the three steps, the first level is r1a = (4 D1 - D0) / 3 and
    r1b = (4 D2 - D1) / 3, the second r2 = (16 r1b - r1a) / 15, which is returned.  The self-consistency is |r1b - r1a|,
    the agreement of the two values of the last level that has two: at these steps the differences are dominated by the
    rounding of the long-double forward solve (some ten eps of J over h), and r2 carries 0.9 of the rounding of
    r1b - r1a (weights 64, -20, 1 over 45 against 4, -5, 1 over 3, the noise of D_i growing as 1 / h_i).  The distance
    r2 - r1b is (r1b - r1a) / 15 by construction: ten times it is below r2's own rounding, whatever is compared with it."""
    V, dV, beam = np.asarray(c["V"], LD), np.asarray(c["dV"], LD)[p], np.asarray(c["beam"], LD)
    dlnb = np.asarray(_dlnb(c, c.get("dlnbeam")), LD)[p]

    def J(h):
        h = LD(h)
        sp, al, sg = R.optics_definition(c["A"], V + h * dV, c["ssa"], c["asym"], LD)
        return R._adding(sp, al, sg, beam * np.exp(h * dlnb), c["sun"], c["mu0"], c["albedo"], LD)[1]

    D = [(J(h) - J(-h)) / (2 * LD(h)) for h in FD_STEPS]
    r1a, r1b = (4 * D[1] - D[0]) / 3, (4 * D[2] - D[1]) / 3
    r2 = (16 * r1b - r1a) / 15
    return r2, np.abs(r1b - r1a)


def directions(rng, c, n_par, n_rays, relative=False):
    """The case c with dV [n_par, n_gas, N], dlnbeam [n_par, N + 1, n_pts] and Q [n_rays, N, n_pts] (None for n_rays = 0):
    per parameter a node triangle of one to three layers on a random gas, either sign, non-zero on non-empty layers only
    (relative: that gas's own V times the triangle, so that h is a relative step and V + h dV a valid column); from three parameters on, parameter 1
    has dV = 0 (only the beam moves) and parameter 2 dlnbeam = 0; with two, parameter 1 has dV = 0."""
    n_gas, N, n_pts = c["A"].shape
    V = c["V"]
    dV = np.zeros((n_par, n_gas, N))
    full = np.where(np.any(V > 0, axis=0))[0]
    for p in range(n_par):
        if full.size == 0 or (p == 1 and n_par >= 2):
            continue
        g, mid, width = int(rng.integers(n_gas)), int(rng.choice(full)), int(rng.integers(1, 4))
        sign = float(rng.choice([-1.0, 1.0]))
        for l, w in zip(range(mid - width // 2, mid - width // 2 + width), ((1.0,), (0.5, 0.5), (0.5, 1.0, 0.5))[width - 1]):
            if 0 <= l < N and np.any(V[:, l] > 0):
                scale = V[g, l] if relative else float(V[:, l].max())
                dV[p, g, l] = sign * w * (1.0 if relative else rng.uniform(0.2, 1.0)) * scale
    dlnbeam = rng.uniform(-1.0, 1.0, (n_par, N + 1, n_pts))
    for p, l in zip(*np.nonzero(np.any(dV != 0, axis=1))):      # a layer's own two parts with one sign: see the docstring
        dlnbeam[p, l] = np.abs(dlnbeam[p, l]) * np.sign(dV[p, :, l].sum())
    if n_par >= 3:
        dlnbeam[2] = 0.0
    Q = rng.uniform(0.1, 1.0, (n_rays, N, n_pts)) if n_rays else None
    return dict(c, dV=dV, dlnbeam=dlnbeam, Q=Q)


def physical_directions(c):
    """The case c with the dlnbeam a column parameter really has: more column, less beam -- d ln beam at a layer's middle
    is minus the parameter's optical depth above it (half of the layer's own), over max(|mu0|, 0.2); the boundary row sees
    all of it.  The two parts of a layer then have opposite signs, which the yardstick by parts is for."""
    A, dV = np.asarray(c["A"]), np.asarray(c["dV"])
    dtau = np.einsum("pgl,glj->plj", dV, A)                                      # [n_par, N, n_pts]
    above = np.cumsum(dtau[:, ::-1], axis=1)[:, ::-1]                           # layers l .. N - 1
    mid = above - 0.5 * dtau
    dlnbeam = -np.concatenate([mid, above[:, :1]], axis=1) / max(abs(c["mu0"]), 0.2)
    return dict(c, dlnbeam=np.ascontiguousarray(dlnbeam))


def panel_case(n_layers, n_gas, n_pts, n_par, n_rays):
    """One case of the GPU bound panel: the forward op's panel case with directions."""
    rng = np.random.default_rng([20261022, n_layers, n_gas, n_pts, n_par, n_rays])
    return directions(rng, R.panel_case(n_layers, n_gas, n_pts), n_par, n_rays)


def random_columns(n=300, seed=11):
    """The 300 random columns of the host test: N from 1 to 80, two points, one to five parameters, two rays."""
    rng = np.random.default_rng([20261022, seed])
    for i in range(n):
        n_layers = int(rng.choice([1, 2, 3, 5, 12, 17, 40, 80])) if i % 3 else int(rng.integers(1, 81))
        yield directions(rng, R.column_case(rng, n_layers, int(rng.integers(1, 9)), 2), int(rng.integers(1, 6)), 2)


def fd_columns(n=40, seed=13):
    """The columns of the difference check: N <= 17, n_gas <= 3, one gas's V moved on up to three layers and ln beam on
    all; no column at the floor's kink (co exactly 0 stays 0 on both sides: only the scatterer moves there)."""
    rng = np.random.default_rng([20261022, seed])
    for i in range(n):
        c = R.column_case(rng, int(rng.integers(1, 18)), int(rng.integers(1, 4)), 2)
        yield directions(rng, c, 1, 0, relative=True)
