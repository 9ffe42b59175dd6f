"""Extended-precision CPU reference of the two-stream diffuse source (sr_diffuse_source_rows_dev, engine.diffuse_source),
in numpy.longdouble, stated twice, with the yardstick of its error and the case set of tests/test_diffuse_source_host.py
and tests/test_gpu_diffuse_source.py.  A helper module: no fixture, no pytest setting, nothing that needs a GPU.

The definition (the build's own; the reference tree has no counterpart), per grid point, layers
l = 0 .. N-1 bottom to top, interfaces i = 0 .. N, t_g = V[g][l] A[g][l][j], f_g = max(asym_g, 0)^2:

    sigma = sum ssa_g t_g, alpha = sum (1 - ssa_g) t_g, sigma_f = sum ssa_g f_g t_g, sigma_g = sum ssa_g asym_g t_g
    sigma' = sigma - sigma_f, dtau' = sigma' + alpha, co = max(alpha / dtau', 2^-52), omega' = 1 - co,
    g' = (sigma_g - sigma_f) / sigma'  (0 where sigma' == 0)
    gamma1 - gamma2 = sqrt3 co, gamma1 + gamma2 = sqrt3 (1 - omega' g'), gamma3 = (1 - sqrt3 g' mu0) / 2
    S+ = omega' D gamma3, S- = omega' D (1 - gamma3), D = sun beam[l]
    dF+/dtau = gamma1 F+ - gamma2 F- - S+,   dF-/dtau = gamma2 F+ - gamma1 F- + S-        (tau downward)
    F-(top) = 0, F+(bottom) = albedo (F-(bottom) + max(mu0, 0) sun beam[N]), F+- continuous
    J_l = sqrt3 (F+_l + F-_l + F+_{l+1} + F-_{l+1}) / (8 pi),   emi[l] = ssa_G (1 - f_G) A[G][l] J_l

reference      the layer operators R, T, E+- in the closed forms that do not cancel near omega' -> 1, added bottom up and
               swept top down; 1 - R and 1 - R - T have closed forms of their own (u (1 + Gamma e^2) / den and
               m u (1 - Gamma e) / den), and 1 - Rb of the stack below is carried beside Rb, so that 1 - Rb R is a sum
               of non-negative terms -- algebraically the elimination q = 1 / (1 - Rb R) of the issue's statement.
reference_bvp  the 2N x 2N interface system in the scaled exponential basis e^{-k x}, e^{-k (dtau' - x)} with the
               particular solution (gamma1 S+ + gamma2 S-) / k^2, (gamma1 S- + gamma2 S+) / k^2, solved by Gaussian
               elimination with partial pivoting: independent of the R / T / E closed forms.  Its particular solution
               cancels as co -> 0 (condition ~ 1 / co), so it is compared where co >= 1e-3 only.
plain64        the kernel's formulas term by term in fp64 numpy (the same code path as `reference` with fp64 in
               long double's place and the kernel's per-gas coefficients ssa (1 - f), 1 - ssa, ssa (asym - f)).

The yardstick, pointwise for J, emi and the fluxes, eps = 2^-53:

    b = eps (n_gas + C_LAYER n_layers + 16) |ref|

n_gas for the three sums of a layer, C_LAYER per layer of the two sweeps, 16 for the output products and the boundary.
C_LAYER = 16 was set so that plain64 stays at <= 0.5 of b over the GPU panel and 300 random columns (N 1 .. 80, dtau 1e-8
.. 80, co down to 1e-14 and exactly 0, empty layers, beam spanning e^-30, albedo 0 .. 1, mu0 -0.3 .. 1): each layer has
some forty roundings in its operators and the two sweeps, of which about a third add up with one sign in the worst
column.  Measured: plain64 / b <= 0.26 on the host (emi 0.260, J 0.241, flux 0.236; tests/test_diffuse_source_host.py
prints it and asserts <= 0.5); the GPU test asserts <= 1 (the factor 2 for the device's exp / expm1 / sqrt / division)
and measured 0.26 on the MI355X (the worst case is a one-layer column, where the constant 16 carries the bound).
"""
import numpy as np

LD = np.longdouble
assert np.finfo(LD).eps < 2e-19, "numpy.longdouble is not an extended-precision type here: no reference, no fallback"

EPS53 = 2.0 ** -53
C_LAYER = 16
CO_MIN = 2.0 ** -52

# the bound panel of the GPU test
N_LAYERS = (1, 2, 3, 17, 80)
N_GAS = (1, 3, 8)
N_PTS = (1, 63, 65, 257)


def bound(ref, n_gas, n_layers):
    return LD(EPS53) * (n_gas + C_LAYER * n_layers + 16) * np.abs(np.asarray(ref, LD))


def ratio(got, ref, b):
    """max |got - ref| / b as fp64; where b is 0 the result must be exactly the reference's.  A NaN or Inf is an error."""
    got = np.asarray(got)
    assert np.all(np.isfinite(np.asarray(got, np.float64))), "non-finite result"
    err = np.abs(np.asarray(got, LD) - ref)
    with np.errstate(divide="ignore", invalid="ignore"):
        q = np.where(b > 0, err / np.where(b > 0, b, LD(1)), np.where(err == 0, LD(0), LD(np.inf)))
    return float(np.max(q)) if q.size else 0.0


def _f(asym, ft):
    a = np.asarray(asym, ft)
    return np.maximum(a, ft(0)) ** 2


def optics_definition(A, V, ssa, asym, ft=LD):
    """(sigma', alpha, sigma_g - sigma_f) [n_layers, n_pts] by the definition's four sums, in ft."""
    A, V, ssa, asym = (np.asarray(x, ft) for x in (A, V, ssa, asym))
    f = _f(asym, ft)
    z = np.zeros(A.shape[1:], ft)
    sig, al, sf, sg = z.copy(), z.copy(), z.copy(), z.copy()
    for g in range(A.shape[0]):
        t = V[g][:, None] * A[g]
        sig = sig + ssa[g] * t
        al = al + (1 - ssa[g]) * t
        sf = sf + ssa[g] * f[g] * t
        sg = sg + ssa[g] * asym[g] * t
    return sig - sf, al, sg - sf


def optics_kernel(A, V, ssa, asym):
    """The same three rows as the kernel forms them, fp64: per-gas coefficients made first, gases ascending."""
    A, V, ssa, asym = (np.asarray(x, np.float64) for x in (A, V, ssa, asym))
    f = _f(asym, np.float64)
    cs, ca, cg = ssa * (1.0 - f), 1.0 - ssa, ssa * (asym - f)
    z = np.zeros(A.shape[1:])
    sp, al, sg = z.copy(), z.copy(), z.copy()
    for g in range(A.shape[0]):
        t = V[g][:, None] * A[g]
        sp = sp + cs[g] * t
        al = al + ca[g] * t
        sg = sg + cg[g] * t
    return sp, al, sg


def _coefficients(sp, al, sg, ft):
    """(dtau, co, om, g, d, s) of one layer's rows; dtau == 0 gives harmless values (the caller masks them)."""
    dtau = sp + al
    live = dtau > 0
    safe = np.where(live, dtau, ft(1))
    co = np.maximum(np.where(live, al, ft(1)) / safe, ft(CO_MIN))
    om = 1 - co
    g = np.where(sp > 0, sg / np.where(sp > 0, sp, ft(1)), ft(0))
    r3 = np.sqrt(ft(3))
    return dtau, live, co, om, g, r3 * co, r3 * (1 - om * g)


def layer_operators(sp, al, sg, D, mu0, ft):
    """dict(R, T, Ep, Em, oneR, absb) of one layer, arrays over the points, in ft: the kernel's closed forms."""
    dtau, live, co, om, g, d, s = _coefficients(sp, al, sg, ft)
    r3 = np.sqrt(ft(3))
    sd, ss = np.sqrt(d), np.sqrt(s)
    k, g1 = sd * ss, (s + d) / 2
    g2 = (r3 * om * (1 - g)) / 2
    rg = 1 / (g1 + k)
    Gm, u = g2 * rg, sd * (sd + ss) * rg
    x = k * dtau
    e, m = np.exp(-x), -np.expm1(-x)
    ge = 1 + Gm * e
    rden = 1 / ((u + Gm * m) * ge)
    R = Gm * m * (1 + e) * rden
    T = e * u * (1 + Gm) * rden
    oneR = u * (1 + Gm * e * e) * rden
    absb = m * u * (1 - Gm * e) * rden
    oneT = m * (u + Gm * ge) * rden
    src = om * D
    es = src * (sd + ss) * rg * (m / sd) / ge
    ed = -(src * (r3 * g * ft(mu0))) / s * (oneT + R)
    o = dict(R=R, T=T, Ep=(es + ed) / 2, Em=(es - ed) / 2, oneR=oneR, absb=absb)
    idle = dict(R=0, T=1, Ep=0, Em=0, oneR=1, absb=0)
    o = {key: np.where(live, val, ft(idle[key])) for key, val in o.items()}
    o["live"] = live
    return o


def _adding(sp, al, sg, beam, sun, mu0, albedo, ft):
    """F [2, N + 1, n_pts] (F+, F-) and J [N, n_pts] by adding bottom up and sweeping top down, in ft."""
    N = sp.shape[0]
    beam, sun = np.asarray(beam, ft), np.asarray(sun, ft)
    albedo, mu0 = ft(albedo), ft(mu0)
    Rb = np.full(sun.shape, albedo, ft)
    Cb = np.full(sun.shape, 1 - albedo, ft)
    Ub = albedo * (max(mu0, ft(0)) * (sun * beam[N]))
    keep = []
    for l in range(N):
        o = layer_operators(sp[l], al[l], sg[l], sun * beam[l], mu0, ft)
        q = np.where(o["live"], 1 / (Cb + Rb * o["oneR"]), ft(1))     # (an empty layer: every quantity keeps its bits)
        keep.append((o["T"] * q, (o["Em"] + o["R"] * Ub) * q, Rb, Ub))
        Ub = o["Ep"] + o["T"] * (Ub + Rb * o["Em"]) * q
        Cb = (o["oneR"] * Cb + Rb * o["absb"] * (o["oneR"] + o["T"])) * q
        Rb = o["R"] + o["T"] * o["T"] * Rb * q
    F = np.zeros((2, N + 1) + sun.shape, ft)
    J = np.zeros((N,) + sun.shape, ft)
    F[0, N] = Ub
    if ft is np.float64:        # the kernel's constant
        kJ = np.float64(1.7320508075688772) / (8.0 * 3.141592653589793)
    else:                       # pi to long double's precision
        kJ = np.sqrt(LD(3)) / (8 * (4 * np.arctan(LD(1))))
    for l in range(N - 1, -1, -1):
        tq, cq, rb, ub = keep[l]
        F[1, l] = tq * F[1, l + 1] + cq
        F[0, l] = ub + rb * F[1, l]
        J[l] = kJ * ((F[0, l] + F[1, l]) + (F[0, l + 1] + F[1, l + 1]))
    return F, J


def _emi(A, ssa, asym, J, out_gas, ft):
    ssa, asym = np.asarray(ssa, ft), np.asarray(asym, ft)
    w = ssa[out_gas] * (1 - _f(asym, ft)[out_gas])
    return (w * np.asarray(A, ft)[out_gas]) * J


def reference(A, V, ssa, asym, beam, sun, mu0, albedo, out_gas=0):
    """dict(emi [N, n_pts], J [N, n_pts], flux [2, N + 1, n_pts]) in long double.  A [n_gas, N, n_pts], V [n_gas, N], ssa /
    asym [n_gas], beam [N + 1, n_pts], sun [n_pts]: fp64 inputs taken as exact."""
    sp, al, sg = optics_definition(A, V, ssa, asym, LD)
    F, J = _adding(sp, al, sg, beam, sun, mu0, albedo, LD)
    return dict(emi=_emi(A, ssa, asym, J, out_gas, LD), J=J, flux=F)


def plain64(A, V, ssa, asym, beam, sun, mu0, albedo, out_gas=0):
    """The kernel's formulas term by term in fp64: the same dict."""
    sp, al, sg = optics_kernel(A, V, ssa, asym)
    F, J = _adding(sp, al, sg, beam, sun, mu0, albedo, np.float64)
    return dict(emi=_emi(A, ssa, asym, J, out_gas, np.float64), J=J, flux=F)


def min_co(A, V, ssa, asym):
    """The smallest co of any non-empty layer and point (long double): what reference_bvp's conditioning goes by."""
    sp, al, _ = optics_definition(A, V, ssa, asym, LD)
    dtau = sp + al
    live = dtau > 0
    return float(np.min(np.where(live, al / np.where(live, dtau, LD(1)), LD(1))))


def _solve(M, rhs):
    """Gaussian elimination with partial pivoting in long double (no LAPACK in long double)."""
    M, rhs = M.copy(), rhs.copy()
    n = len(rhs)
    for c in range(n):
        p = c + int(np.argmax(np.abs(M[c:, c])))
        if p != c:
            M[[c, p]], rhs[[c, p]] = M[[p, c]], rhs[[p, c]]
        fac = M[c + 1:, c] / M[c, c]
        M[c + 1:] -= fac[:, None] * M[c][None, :]
        rhs[c + 1:] -= fac * rhs[c]
    x = np.zeros(n, LD)
    for c in range(n - 1, -1, -1):
        x[c] = (rhs[c] - M[c, c + 1:] @ x[c + 1:]) / M[c, c]
    return x


def reference_bvp(A, V, ssa, asym, beam, sun, mu0, albedo, out_gas=0):
    """The same dict from the interface system in the scaled exponential basis, point by point, in long double.  In a
    layer, x downward from its top: F+ = Gamma a e^{-k x} + b e^{-k (dtau - x)} + P+, F- = a e^{-k x} + Gamma b
    e^{-k (dtau - x)} + P-.  Empty layers are left out of the system and their interfaces copied."""
    sp, al, sg = optics_definition(A, V, ssa, asym, LD)
    N, n_pts = sp.shape
    beam, sun = np.asarray(beam, LD), np.asarray(sun, LD)
    mu0, albedo, r3 = LD(mu0), LD(albedo), np.sqrt(LD(3))
    F = np.zeros((2, N + 1, n_pts), LD)
    for j in range(n_pts):
        lay = [l for l in range(N) if sp[l, j] + al[l, j] > 0]
        n = len(lay)
        surf = albedo * max(mu0, LD(0)) * sun[j] * beam[N, j]
        if n == 0:
            F[0, :, j] = surf
            continue
        Gm, ex, Pp, Pm = (np.zeros(n, LD) for _ in range(4))
        for i, l in enumerate(lay):     # i = 0: the lowest live layer
            dtau, live, co, om, g, d, s = _coefficients(sp[l, j], al[l, j], sg[l, j], LD)
            g1, g2 = (s + d) / 2, (s - d) / 2
            k = np.sqrt(d * s)
            g3 = (1 - r3 * g * mu0) / 2
            D = sun[j] * beam[l, j]
            Sp, Sm = om * D * g3, om * D * (1 - g3)
            Gm[i], ex[i] = g2 / (g1 + k), np.exp(-k * dtau)
            Pp[i], Pm[i] = (g1 * Sp + g2 * Sm) / (k * k), (g1 * Sm + g2 * Sp) / (k * k)
        M, rhs = np.zeros((2 * n, 2 * n), LD), np.zeros(2 * n, LD)
        # unknowns (a_i, b_i) at columns 2 i, 2 i + 1.  top of layer i (x = 0): F+ = Gm a + ex b + P+, F- = a + Gm ex b + P-;
        # bottom (x = dtau): F+ = Gm ex a + b + P+, F- = ex a + Gm b + P-
        row = 0
        t = n - 1                       # F-(top of the highest live layer) = 0
        M[row, 2 * t], M[row, 2 * t + 1], rhs[row] = 1, Gm[t] * ex[t], -Pm[t]
        row += 1
        for i in range(n - 1):          # bottom of layer i + 1 = top of layer i
            up, lo = i + 1, i
            M[row, 2 * up], M[row, 2 * up + 1], M[row, 2 * lo], M[row, 2 * lo + 1] = Gm[up] * ex[up], 1, -Gm[lo], -ex[lo]
            rhs[row] = Pp[lo] - Pp[up]
            row += 1
            M[row, 2 * up], M[row, 2 * up + 1], M[row, 2 * lo], M[row, 2 * lo + 1] = ex[up], Gm[up], -1, -Gm[lo] * ex[lo]
            rhs[row] = Pm[lo] - Pm[up]
            row += 1
        # F+(bottom) = albedo (F-(bottom) + direct)
        M[row, 0], M[row, 1] = Gm[0] * ex[0] - albedo * ex[0], 1 - albedo * Gm[0]
        rhs[row] = surf + albedo * Pm[0] - Pp[0]
        x = _solve(M, rhs)
        a, b = x[0::2], x[1::2]
        top_p, top_m = Gm * a + ex * b + Pp, a + Gm * ex * b + Pm
        bot_p, bot_m = Gm * ex * a + b + Pp, ex * a + Gm * b + Pm
        # interfaces: below the lowest live layer everything equals its bottom; between live layers the lower one's top
        i = 0
        for itf in range(N + 1):
            while i < n and lay[i] < itf - 0:
                i += 1
            # i: the first live layer with index >= itf, i.e. the live layer ABOVE this interface (n: none)
            if i < n:
                F[0, itf, j], F[1, itf, j] = bot_p[i], bot_m[i]
            else:
                F[0, itf, j], F[1, itf, j] = top_p[n - 1], top_m[n - 1]
    kJ = np.sqrt(LD(3)) / (8 * (4 * np.arctan(LD(1))))
    J = kJ * ((F[0, :-1] + F[1, :-1]) + (F[0, 1:] + F[1, 1:]))
    return dict(emi=_emi(A, ssa, asym, J, out_gas, LD), J=J, flux=F)


def column_case(rng, n_layers, n_gas, n_pts, tau_lo=1e-8, tau_hi=80.0, co_lo=1e-14, conservative=0.15, empty=0.1,
                albedo=None, mu0=None):
    """dict(A, V, ssa, asym, beam, sun, mu0, albedo, out_gas) of one random case, fp64.  Gas 0 is the scatterer whose rows
    are made; per layer its optical depth is log-uniform in [tau_lo, tau_hi] / n_layers .. and the absorbers' share is
    set so that co is log-uniform in [co_lo, 1]; with probability `conservative` a case has ssa = 1 and no absorber at all
    (co exactly 0), with probability `empty` a layer is empty (every V = 0).  beam falls from 1 at the top by up to
    e^-30 to the lower boundary; albedo in [0, 1], mu0 in [-0.3, 1]."""
    cons = rng.uniform() < conservative
    ssa = np.zeros(n_gas)
    asym = np.zeros(n_gas)
    n_sca = 1 if n_gas == 1 else int(rng.integers(1, min(n_gas, 3) + 1))
    ssa[:n_sca] = 1.0 if cons else rng.uniform(0.3, 1.0, n_sca)
    if not cons and rng.uniform() < 0.5:
        ssa[0] = 1.0
    asym[:n_sca] = rng.uniform(-0.5, 0.95, n_sca)
    total = np.exp(rng.uniform(np.log(tau_lo), np.log(tau_hi)))
    share = rng.dirichlet(np.ones(n_layers)) * total                      # the scatterers' optical depth per layer
    V = np.zeros((n_gas, n_layers))
    V[:n_sca] = rng.dirichlet(np.ones(n_sca), n_layers).T * share[None, :]
    if n_gas > n_sca and not cons:
        co = np.exp(rng.uniform(np.log(co_lo), 0.0, n_layers))
        absorb = share * co / np.maximum(1.0 - co, 1e-3)
        V[n_sca:] = rng.dirichlet(np.ones(n_gas - n_sca), n_layers).T * absorb[None, :]
    V[:, rng.uniform(size=n_layers) < empty] = 0.0
    A = rng.uniform(0.5, 1.5, (n_gas, n_layers, n_pts)) * np.exp(rng.uniform(np.log(0.3), 0.0, n_pts))[None, None, :]
    depth = rng.uniform(0.0, 30.0) * np.linspace(1.0, 0.0, n_layers + 2)[1:]   # layer middles bottom .. top, then ...
    beam = np.exp(-np.concatenate([depth[1:], depth[:1]]))[:, None] * rng.uniform(0.9, 1.0, (n_layers + 1, n_pts))
    return dict(A=A, V=V, ssa=ssa, asym=asym, beam=np.ascontiguousarray(beam), sun=rng.uniform(5.0, 20.0, n_pts),
                mu0=float(rng.uniform(-0.3, 1.0)) if mu0 is None else float(mu0),
                albedo=float(rng.choice([0.0, 1.0, rng.uniform()])) if albedo is None else float(albedo), out_gas=0)


def bvp_case(rng, n_layers, n_pts=2, empty=0.0):
    """A case reference_bvp is conditioned for: a scatterer (ssa = 1) and an absorber with, per layer, dtau' log-uniform
    in about [3e-3, 5] and co in about [3e-3, 1] (the table's spread over the points moves both by up to a factor 3)."""
    asym = np.array([rng.uniform(-0.5, 0.9), 0.0])
    f = max(asym[0], 0.0) ** 2
    dtau = np.exp(rng.uniform(np.log(1e-2), np.log(5.0), n_layers))
    co = np.exp(rng.uniform(np.log(1e-2), 0.0, n_layers))
    V = np.array([dtau * (1 - co) / (1 - f), dtau * co])
    V[:, rng.uniform(size=n_layers) < empty] = 0.0
    A = rng.uniform(0.6, 1.4, (2, n_layers, n_pts))
    depth = rng.uniform(0.0, 30.0) * np.linspace(1.0, 0.0, n_layers + 2)[1:]
    beam = np.exp(-np.concatenate([depth[1:], depth[:1]]))[:, None] * rng.uniform(0.9, 1.0, (n_layers + 1, n_pts))
    return dict(A=A, V=V, ssa=np.array([1.0, 0.0]), asym=asym, beam=np.ascontiguousarray(beam), sun=rng.uniform(5.0, 20.0, n_pts),
                mu0=float(rng.uniform(-0.3, 1.0)), albedo=float(rng.choice([0.0, 1.0, rng.uniform()])), out_gas=0)


def min_dtau(A, V, ssa, asym):
    """The smallest dtau' of any non-empty layer and point."""
    sp, al, _ = optics_definition(A, V, ssa, asym, LD)
    dtau = sp + al
    return float(np.min(np.where(dtau > 0, dtau, LD(np.inf))))


def panel_case(n_layers, n_gas, n_pts, seed=0):
    """One case of the GPU bound panel."""
    return column_case(np.random.default_rng([20261021, n_layers, n_gas, n_pts, seed]), n_layers, n_gas, n_pts)


def random_columns(n=300, seed=7):
    """The 300 random columns of the host test: N from 1 to 80, one or two points each."""
    rng = np.random.default_rng([20261021, seed])
    for i in range(n):
        n_layers = int(rng.choice([1, 2, 3, 5, 12, 17, 40, 80])) if i % 3 else int(rng.integers(1, 81))
        yield column_case(rng, n_layers, int(rng.integers(1, 9)), 2)


def args(c):
    return (c["A"], c["V"], c["ssa"], c["asym"], c["beam"], c["sun"], c["mu0"], c["albedo"], c["out_gas"])


def conservation_case(n_layers, n_pts, seed=0):
    """ssa = 1, one gas, no absorber, albedo 0: F+_N + F-_0 = sum_l dtau'_l D_l.  The floor co >= 2^-52 = 2 eps takes
    2 eps of the light per scattering, and light scatters about max(tau, tau^2) times before it leaves: the column's
    optical depth stays below 2, so that the floor's share stays inside b (at tau = 20 it is 25 eps alone)."""
    rng = np.random.default_rng([20261021, 99, n_layers, n_pts, seed])
    c = column_case(rng, n_layers, 1, n_pts, tau_lo=1e-2, tau_hi=2.0 / 1.5, conservative=1.1, empty=0.0, albedo=0.0)
    return c


def absorbed_input(c):
    """sum_l dtau'_l D_l [n_pts] of a case, in long double."""
    sp, al, _ = optics_definition(c["A"], c["V"], c["ssa"], c["asym"], LD)
    return np.sum((sp + al) * np.asarray(c["sun"], LD)[None, :] * np.asarray(c["beam"], LD)[:-1], axis=0)
