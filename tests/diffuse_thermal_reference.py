"""Extended-precision CPU reference of thermal emission as a source of the two-stream diffuse field
(sr_diffuse_thermal_rows_dev, engine.diffuse_thermal_source), in numpy.longdouble, stated twice, with the yardstick of
its error and the case set of tests/test_diffuse_thermal_host.py and tests/test_gpu_diffuse_thermal.py.  A helper module:
no fixture, no pytest setting, nothing that needs a GPU.

The definition (the build's own) is that of tests/diffuse_source_reference.py -- its sums, layer
operators, boundary conditions and outputs -- with one more source.  Layer l emits isotropically, constant over the layer,
at its own temperature:

    S+ = S- = 2 pi co B_l,   B_l = 2 h c^2 nu_j^3 / (exp(c2 nu_j / T_l) - 1),   nu_j = w0 + (double)(g_lo + j) step

so that the particular solution is F+ = F- = 2 pi B_l / sqrt3 and the layer sends out E+_th = E-_th = (2 pi / sqrt3) B_l
(1 - R - T), with 1 - R - T = m u / (1 + Gamma e) (absorptance() below: no subtraction).  A layer with alpha == 0 at a
point has a thermal source of exactly 0.  A Lambertian surface of emissivity 1 - albedo at t_surface (0: none) adds (1 - albedo) (2 pi / sqrt3) B(nu, t_surface) to the upwelling at the lower
boundary.  With a sun (beam, sun, mu0) the solar sources are added to the same equations; without one they are absent.

    own_emission = 0:  emi[l] = ssa_G (1 - f_G) A[G][l] J_l
    own_emission = 1:  emi[l] = A[G][l] ((1 - ssa_G) B_l + ssa_G (1 - f_G) J_l)

reference      the adding form: diffuse_source_reference's closed-form layer operators with E_th added to E+-.
reference_bvp  the 2N x 2N interface system of diffuse_source_reference.reference_bvp with 2 pi B_l / sqrt3 added to both
               particular solutions (where alpha > 0) and the surface's emission added to its last row.
plain64        the kernel's formulas term by term in fp64 numpy: the Planck function as absorber_table_reference.planck
               states the kernel's (x~ with its exact residual), the constants the kernel's doubles.

Planck is evaluated in long double from the fp64 nu_j and T, both taken as exact.  The yardstick, pointwise for J, emi
and the fluxes, eps = 2^-53:

    b = eps (n_gas + C_LAYER n_layers + 16 + C_PLANCK + 2 x_max) |ref|,    x_max = c2 nu_j / min(T)

diffuse_source_reference's count plus the absorber-table reference's allowance for one Planck value, eps (8 + 2 x): J and
the fluxes are combinations of the B_l (and the solar sources) with non-negative weights, so the largest relative error
of a B_l carries through.  C_PLANCK = 8 is that reference's constant, unchanged.  Measured: plain64 / b <= 0.23 over the
GPU panel's cases (thermal alone and with the sun, own_emission off and on) and 300 random columns with temperatures of
70 .. 200 K per layer and nu in 500 .. 3300 cm^-1, x up to 66.5 (emi 0.151, J 0.135, flux 0.225;
tests/test_diffuse_thermal_host.py prints it and asserts <= 0.5); the GPU test asserts <= 1 and measured 0.22 on the
MI355X (a one-layer column, as for the solar source).  With 1 - R - T formed as m u (1 - Gamma e) / den the same
measurement gave 9400 (co = 3.5e-14 above a surface of albedo 1): the subtraction, not the constants -- see absorptance().
"""
import numpy as np

import absorber_table_reference as AR
import diffuse_source_reference as R

LD = R.LD
EPS53 = R.EPS53
C_PLANCK = 8

N_LAYERS, N_GAS, N_PTS = R.N_LAYERS, R.N_GAS, R.N_PTS
ratio = R.ratio


def x_max(c):
    """c2 nu_j / min(T) [n_pts] of a case (the surface's temperature counts where it emits)."""
    t = np.min(c["temps"]) if not c["t_surface"] > 0 else min(np.min(c["temps"]), c["t_surface"])
    return LD(AR.C2) * nu_of(c).astype(LD) / LD(t)


def bound(ref, n_gas, n_layers, xmax):
    return LD(EPS53) * (n_gas + R.C_LAYER * n_layers + 16 + C_PLANCK + 2 * np.asarray(xmax, LD)) * np.abs(np.asarray(ref, LD))


def nu_of(c):
    return AR.grid_nu(c["w0"], c["step"], c["g_lo"], c["A"].shape[2])


def planck_rows(nu, temps, ft):
    """B [len(temps), n_pts] in ft; fp64 as the kernel forms it."""
    return np.stack([AR.planck(nu, T, ft)[0] for T in np.atleast_1d(temps)])


def _k_thermal(ft):
    if ft is np.float64:        # the kernel's constant
        return np.float64(2.0 * 3.141592653589793 / 1.7320508075688772)
    return 2 * (4 * np.arctan(LD(1))) / np.sqrt(LD(3))


def _k_mean(ft):
    if ft is np.float64:
        return np.float64(1.7320508075688772) / (8.0 * 3.141592653589793)
    return np.sqrt(LD(3)) / (8 * (4 * np.arctan(LD(1))))


def absorptance(sp, al, sg, ft):
    """1 - R - T of one layer's rows in ft, as m u / (1 + Gamma e): diffuse_source_reference's closed form m u (1 - Gamma e)
    / den with u + Gamma m = 1 - Gamma e cancelled against den = (u + Gamma m)(1 + Gamma e).  Nothing is subtracted: as
    co -> 0 in a thin layer 1 - Gamma e itself loses sqrt(co) of its digits, which a source cannot afford (the adding's
    use of it can: there it stands beside terms of order 1).  0 for an empty layer."""
    dtau, live, co, om, g, d, s = R._coefficients(sp, al, sg, ft)
    r3 = np.sqrt(ft(3))
    sd, ss = np.sqrt(d), np.sqrt(s)
    k, g1 = sd * ss, (s + d) / 2
    g2 = (r3 * om * (1 - g)) / 2
    rg = 1 / (g1 + k)
    Gm, u = g2 * rg, sd * (sd + ss) * rg
    x = k * dtau
    e, m = np.exp(-x), -np.expm1(-x)
    return np.where(live, m * u / (1 + Gm * e), ft(0))


def _adding(sp, al, sg, B, Bs, beam, sun, mu0, albedo, ft):
    """F [2, N + 1, n_pts] and J [N, n_pts] by adding bottom up and sweeping top down, in ft.  beam None: no sun."""
    N, n_pts = sp.shape
    albedo, kth = ft(albedo), _k_thermal(ft)
    Rb, Cb = np.full(n_pts, albedo, ft), np.full(n_pts, 1 - albedo, ft)
    if beam is None:
        sun, beam, mu0 = np.zeros(n_pts, ft), np.zeros((N + 1, n_pts), ft), ft(0)
        Ub = np.zeros(n_pts, ft)
    else:
        beam, sun, mu0 = np.asarray(beam, ft), np.asarray(sun, ft), ft(mu0)
        Ub = albedo * (max(mu0, ft(0)) * (sun * beam[N]))
    if Bs is not None:
        Ub = Ub + Cb * (kth * Bs)
    keep = []
    for l in range(N):
        o = R.layer_operators(sp[l], al[l], sg[l], sun * beam[l], mu0, ft)
        eth = np.where(al[l] > 0, (kth * B[l]) * absorptance(sp[l], al[l], sg[l], ft), ft(0))       # no absorber: an exact 0
        Ep, Em = o["Ep"] + eth, o["Em"] + eth
        q = np.where(o["live"], 1 / (Cb + Rb * o["oneR"]), ft(1))
        keep.append((o["T"] * q, (Em + o["R"] * Ub) * q, Rb, Ub))
        Ub = Ep + o["T"] * (Ub + Rb * Em) * q
        Cb = (o["oneR"] * Cb + Rb * o["absb"] * (o["oneR"] + o["T"])) * q
        Rb = o["R"] + o["T"] * o["T"] * Rb * q
    F, J = np.zeros((2, N + 1, n_pts), ft), np.zeros((N, n_pts), ft)
    F[0, N] = Ub
    kJ = _k_mean(ft)
    for l in range(N - 1, -1, -1):
        tq, cq, rb, ub = keep[l]
        F[1, l] = tq * F[1, l + 1] + cq
        F[0, l] = ub + rb * F[1, l]
        J[l] = kJ * ((F[0, l] + F[1, l]) + (F[0, l + 1] + F[1, l + 1]))
    return F, J


def _emi(A, ssa, asym, J, B, out_gas, own, ft):
    ssa, asym = np.asarray(ssa, ft), np.asarray(asym, ft)
    w = ssa[out_gas] * (1 - R._f(asym, ft)[out_gas])
    sca = np.asarray(A, ft)[out_gas]
    if own:
        return sca * ((1 - ssa[out_gas]) * B + w * J)
    return (w * sca) * J


def _run(c, solar, own, ft, optics):
    sp, al, sg = optics(c["A"], c["V"], c["ssa"], c["asym"]) if ft is np.float64 else optics(c["A"], c["V"], c["ssa"], c["asym"], LD)
    nu = nu_of(c)
    B = planck_rows(nu, c["temps"], ft)
    Bs = planck_rows(nu, [c["t_surface"]], ft)[0] if c["t_surface"] > 0 else None
    beam, sun = (c["beam"], c["sun"]) if solar else (None, None)
    F, J = _adding(sp, al, sg, B, Bs, beam, sun, c["mu0"], c["albedo"], ft)
    return dict(emi=_emi(c["A"], c["ssa"], c["asym"], J, B, c["out_gas"], own, ft), J=J, flux=F, B=B)


def reference(c, solar=True, own=False):
    """dict(emi, J, flux, B) in long double of the case c (thermal_case); solar=False: thermal emission alone."""
    return _run(c, solar, own, LD, R.optics_definition)


def plain64(c, solar=True, own=False):
    """The kernel's formulas term by term in fp64: the same dict."""
    return _run(c, solar, own, np.float64, R.optics_kernel)


def reference_bvp(c, solar=True, own=False):
    """The same dict from the interface system (diffuse_source_reference.reference_bvp's unknowns, rows and basis), point
    by point, in long double: 2 pi B_l / sqrt3 added to both particular solutions where alpha > 0, the surface's emission
    added to the last row."""
    A, V, ssa, asym = c["A"], c["V"], c["ssa"], c["asym"]
    sp, al, sg = R.optics_definition(A, V, ssa, asym, LD)
    N, n_pts = sp.shape
    nu = nu_of(c)
    B = planck_rows(nu, c["temps"], LD)
    kth = _k_thermal(LD)
    Bs = planck_rows(nu, [c["t_surface"]], LD)[0] if c["t_surface"] > 0 else np.zeros(n_pts, LD)
    beam = np.asarray(c["beam"], LD) if solar else np.zeros((N + 1, n_pts), LD)
    sun = np.asarray(c["sun"], LD) if solar else np.zeros(n_pts, LD)
    mu0, albedo, r3 = LD(c["mu0"] if solar else 0.0), LD(c["albedo"]), np.sqrt(LD(3))
    F = np.zeros((2, N + 1, n_pts), LD)
    for j in range(n_pts):
        lay = [l for l in range(N) if sp[l, j] + al[l, j] > 0]
        n = len(lay)
        surf = albedo * max(mu0, LD(0)) * sun[j] * beam[N, j] + (1 - albedo) * kth * Bs[j]
        if n == 0:
            F[0, :, j] = surf
            continue
        Gm, ex, Pp, Pm = (np.zeros(n, LD) for _ in range(4))
        for i, l in enumerate(lay):     # i = 0: the lowest live layer
            dtau, live, co, om, g, d, s = R._coefficients(sp[l, j], al[l, j], sg[l, j], LD)
            g1, g2 = (s + d) / 2, (s - d) / 2
            k = np.sqrt(d * s)
            g3 = (1 - r3 * g * mu0) / 2
            D = sun[j] * beam[l, j]
            Sp, Sm = om * D * g3, om * D * (1 - g3)
            Gm[i], ex[i] = g2 / (g1 + k), np.exp(-k * dtau)
            pth = kth * B[l, j] if al[l, j] > 0 else LD(0)
            Pp[i], Pm[i] = (g1 * Sp + g2 * Sm) / (k * k) + pth, (g1 * Sm + g2 * Sp) / (k * k) + pth
        M, rhs = np.zeros((2 * n, 2 * n), LD), np.zeros(2 * n, LD)
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
        # F+(bottom) = albedo (F-(bottom) + direct) + the surface's emission
        M[row, 0], M[row, 1] = Gm[0] * ex[0] - albedo * ex[0], 1 - albedo * Gm[0]
        rhs[row] = surf + albedo * Pm[0] - Pp[0]
        x = R._solve(M, rhs)
        a, b = x[0::2], x[1::2]
        top_p, top_m = Gm * a + ex * b + Pp, a + Gm * ex * b + Pm
        bot_p, bot_m = Gm * ex * a + b + Pp, ex * a + Gm * b + Pm
        i = 0
        for itf in range(N + 1):
            while i < n and lay[i] < itf:
                i += 1
            if i < n:       # the live layer above this interface
                F[0, itf, j], F[1, itf, j] = bot_p[i], bot_m[i]
            else:
                F[0, itf, j], F[1, itf, j] = top_p[n - 1], top_m[n - 1]
    J = _k_mean(LD) * ((F[0, :-1] + F[1, :-1]) + (F[0, 1:] + F[1, 1:]))
    return dict(emi=_emi(A, ssa, asym, J, B, c["out_gas"], own, LD), J=J, flux=F, B=B)


def with_thermal(c, rng, t_lo=70.0, t_hi=200.0, nu_lo=500.0, nu_hi=3300.0):
    """A diffuse_source_reference case with the thermal call's own inputs: temperatures of t_lo .. t_hi K per layer, a grid
    of step 0.01 cm^-1 somewhere in nu_lo .. nu_hi cm^-1 with a shard offset g_lo, a surface that emits or not."""
    n_layers, n_pts = c["A"].shape[1:]
    step = (2900.0 + 0.01) - 2900.0
    g_lo = int(rng.integers(0, 5000))
    w0 = float(np.floor(rng.uniform(nu_lo, nu_hi - (g_lo + n_pts) * step)))
    t_surface = 0.0 if rng.uniform() < 0.4 else float(rng.uniform(t_lo, t_hi))
    return dict(c, temps=rng.uniform(t_lo, t_hi, n_layers), w0=w0, step=step, g_lo=g_lo, t_surface=t_surface)


def panel_case(n_layers, n_gas, n_pts, seed=0):
    """One case of the GPU bound panel: diffuse_source_reference's column with temperatures and a grid."""
    rng = np.random.default_rng([20261022, n_layers, n_gas, n_pts, seed])
    return with_thermal(R.column_case(rng, n_layers, n_gas, n_pts), rng)


def random_columns(n=300, seed=7):
    """The 300 random columns of the host test: N from 1 to 80, one or two points each."""
    rng = np.random.default_rng([20261022, seed])
    for i in range(n):
        n_layers = int(rng.choice([1, 2, 3, 5, 12, 17, 40, 80])) if i % 3 else int(rng.integers(1, 81))
        yield with_thermal(R.column_case(rng, n_layers, int(rng.integers(1, 9)), 2), rng)


def bvp_case(rng, n_layers, n_pts=2, empty=0.0):
    return with_thermal(R.bvp_case(rng, n_layers, n_pts, empty), rng)
