"""Extended-precision CPU reference of the limb radiance recursion and its Jacobians (include/spectrobot_hip.h):

    I   <- I t + E f,                      t = exp(-tau),  f = (1 - t) / tau
    J_p <- J_p t + (-I_prev t dtau_p + dE_p f + E f' dtau_p),     f' = (tau t - (1 - t)) / tau^2

written from those formulas in numpy.longdouble (x87 extended: 64-bit mantissa), with an error bound that follows the
problem's conditioning, a plain fp64 restatement that serves as the yardstick of that bound, and a panel of regimes
(thin switch, range-reduction boundaries, the subnormal edge of exp, saturated and negative optical depths) laid along
the spectral axis so that one launch visits all of them.  A helper module: no fixture, no pytest setting.

The bound.  A result's error is measured in UNITS of

    2^-53 (A + (n_gas + 1) C [+ F]) + 1e-290

A: the same recursion over absolute values -- what one rounding of every term costs;
C: the conditioning to the rounding of each segment's tau, sum_s |J(tau_s (1 + d)) - J| / d (d = 2^-30): tau is a sum
   of n_gas rounded products, and d t / t = -tau (d tau / tau) makes a saturated or cancelling path sensitive to it
   far beyond A (the plain fp64 recursion's Jacobians measure 18 units with C and ~210 without);
F: |I_obs| sum_s |dtau_p|, the resolution floor of the adjoint fold alone, which forms what enters a near-side segment as
   the observed radiance minus what the segments in front of it emit (tools/stress_fold.py hidden_floor).
The absolute floor lets results below the smallest normal double count as zero (underflow is allowed).
"""
import numpy as np

LD = np.longdouble
assert np.finfo(LD).eps < 2e-19, "numpy.longdouble is not an extended-precision type here: no reference, no fallback"

THIN = 1e-12          # the build's definition: f = 1, f' = -1/2 where !(|tau| > 1e-12) (sr_device.hpp attenuation())
D_COND = 2.0 ** -30
EPS53 = 2.0 ** -53
FLOOR = 1e-290

# K_PLAIN: max units(plain_fp64, reference) over the regime panel -- the distance of an honest fp64 implementation
# (libm exp / expm1, IEEE division, path order, tau as the fp64 sum of products) from the reference, in the bound's own
# units.  The kernels' limit is 8 x K_PLAIN computed on each test's own inputs.  Measured 2026-10-17 on
# panel_problem(41, 2, 3, 20261017): 2 gases, 41 segments, 3 parameters, 188 columns: radiances 27.4 ('all -1e-06':
# 41 amplifying segments, every one rounding I again), Jacobians 18.5 (209 with C left out of the bound).  The
# recorded constants are 1.5 x the measurement and may be at most 2 x what was measured when they were written;
# tests/test_limb_reference_host.py asserts that the live measurement does not exceed them.
K_PLAIN_RAD_MEASURED, K_PLAIN_JAC_MEASURED = 27.4, 18.5
K_PLAIN_RAD = 41.0
K_PLAIN_JAC = 25.0
KERNEL_MARGIN = 8.0   # reciprocal + Newton steps for the division, a polynomial exp of <= 1 ulp, sums over up to four
                      # gases in another order, the four composed affine maps of the split kernel

LN2 = float(np.log(2.0))
SPECIAL = ([0.0, 1e-300, 1e-18, 1e-15, 9.9e-13, 1e-12, 1.01e-12,
            1e-10, 1e-8, 1e-6, 1e-4, 1e-2,
            0.2499, 0.25, 0.5 * LN2 * (1 - 2.0 ** -50), 0.5 * LN2 * (1 + 2.0 ** -50), 1.0,
            1.5 * LN2 * (1 - 2.0 ** -50), 1.5 * LN2 * (1 + 2.0 ** -50), 7.5 * LN2,
            30.0, 300.0, 700.0, 745.2, 746.0, 800.0, 1e4, 1e6,
            -1e-13, -1e-6, -0.3, -2.0])
MIN_PATH_TAU = -20.0


# ------------------------------------------------------------------------------------------------------------------
# the functions of one segment
# ------------------------------------------------------------------------------------------------------------------
def _atten_ld(tau, thin):
    """t, f, f' in long double: Taylor series for |tau| < 0.25 (the closed form of f' cancels even in long double),
    -expm1(-tau)/tau and (tau t - (1 - t))/tau^2 above; thin: mask where f = 1, f' = -1/2 by definition (or None)."""
    tau = np.asarray(tau, LD)
    with np.errstate(all="ignore"):
        t = np.exp(-tau)
        small = np.abs(tau) < 0.25
        x = np.where(small, tau, LD(0))
        f_s = np.zeros_like(tau)
        for k in range(24, -1, -1):        # f = sum_k (-x)^k / (k+1)! in nested form: 1 - x/2 (1 - x/3 (1 - ...))
            f_s = f_s * (-x) / LD(k + 2) + LD(1)
        # f' = sum_k -(k+1) (-x)^k / (k+2)! = -1/2 + x/3 - x^2/8 + ..., term by term (the terms shrink by >= 4 k:
        # 25 of them are far below 2^-64)
        fact = LD(2)                       # (k+2)!
        pw = np.ones_like(tau)             # (-x)^k
        fp_s = -LD(1) / fact * pw
        for k in range(1, 25):
            pw = pw * (-x)
            fact = fact * LD(k + 2)
            fp_s = fp_s - LD(k + 1) * pw / fact
        big = np.where(small, LD(1), tau)
        em1 = -np.expm1(-big)
        f_b = em1 / big
        fp_b = (big * np.exp(-big) - em1) / (big * big)
        f = np.where(small, f_s, f_b)
        fp = np.where(small, fp_s, fp_b)
    if thin is not None:
        f = np.where(thin, LD(1), f)
        fp = np.where(thin, LD(-0.5), fp)
    return t, f, fp


def _sweep(tau_k, E, dtau, dE, I0, thin, solo, absolute):
    """The recursion for K variants of tau at once: tau_k [K, S, N]; E [S, N]; dtau, dE [P, S, N]; I0 [N].
    Returns I [K, N], J [K, P, N]; absolute: the recursion over absolute values (A_I, A)."""
    K, S, N = tau_k.shape
    P = dtau.shape[0]
    t, f, fp = _atten_ld(tau_k, thin)
    if absolute:
        t, f, fp, E, dtau, dE, I0 = (np.abs(v) for v in (t, f, fp, E, dtau, dE, I0))
    sgn = LD(1) if absolute else LD(-1)
    I = np.broadcast_to(np.asarray(I0, LD), (K, N)).copy()
    J = np.zeros((K, P, N), LD)
    with np.errstate(under="ignore"):
        for s in range(S):
            ts, fs, fps = t[:, s], f[:, s], fp[:, s]
            src = sgn * (I * ts)[:, None, :] * dtau[None, :, s, :]
            if not solo:
                src = src + dE[None, :, s, :] * fs[:, None, :] + (E[s] * fps)[:, None, :] * dtau[None, :, s, :]
            J = J * ts[:, None, :] + src
            I = I * ts if solo else I * ts + E[s] * fs
    return I, J


def recursion_reference(tau, E, dtau, dE, I0, solo=False, thin_rule=True, want_cond=True, thin_ulps=0):
    """The recursion in long double.  tau, E [S, N]; dtau, dE [P, S, N]; I0 [N]: fp64 arrays taken as exact (or long
    double arrays: products of fp64 coefficients and columns formed in long double, see products()).
    thin_ulps: where tau is a rounded sum of products, an fp64 implementation's tau within that many ulps of the thin
    switch lands on either side of the definition's step (5e-13 of f) by its order of operations, and both sides are
    right: the step's effect, segment by segment, is added to A and A_I there (0: tau is exact, no allowance).
    Returns a dict: I [N], J [P, N], A_I [N], A [P, N], C_I [N], C [P, N], F [P, N] (module docstring)."""
    tau, E, dtau, dE, I0 = (np.asarray(v, LD) for v in (tau, E, dtau, dE, I0))
    S, N = tau.shape
    P = dtau.shape[0]
    assert E.shape == (S, N) and dtau.shape == (P, S, N) and dE.shape == (P, S, N) and I0.shape == (N,)
    thin = ~(np.abs(tau) > LD(THIN)) if thin_rule else None
    # variant 0: the problem itself; variant 1 + s: tau of segment s scaled by (1 + d).  The thin mask stays the
    # unperturbed problem's: C measures conditioning, not the definition's step at 1e-12.
    n_var = 1 + (S if want_cond else 0)
    tau_k = np.broadcast_to(tau, (n_var, S, N)).copy()
    for s in range(n_var - 1):
        tau_k[1 + s, s] = tau[s] * (LD(1) + LD(D_COND))
    thin_k = None if thin is None else np.broadcast_to(thin, tau_k.shape)
    I_k, J_k = _sweep(tau_k, E, dtau, dE, I0, thin_k, solo, False)
    A_I, A = _sweep(tau[None], E, dtau, dE, I0, thin if thin is None else thin[None], solo, True)
    I, J = I_k[0], J_k[0]
    if want_cond:
        C_I = np.abs(I_k[1:] - I).sum(axis=0) / LD(D_COND)
        C = np.abs(J_k[1:] - J).sum(axis=0) / LD(D_COND)
    else:
        C_I, C = np.zeros_like(I), np.zeros_like(J)
    F = np.abs(I)[None, :] * np.abs(dtau).sum(axis=1)
    A_I, A = A_I[0], A[0]
    if thin_rule and thin_ulps:
        amb = np.abs(np.abs(tau) - LD(THIN)) <= LD(thin_ulps * 2.0 ** -52 * THIN)
        cols = np.flatnonzero(amb.any(axis=0))
        if cols.size:
            segs = np.flatnonzero(amb[:, cols].any(axis=1))
            thin_f = np.broadcast_to(thin[:, cols], (segs.size, S, cols.size)).copy()
            for k, s in enumerate(segs):
                thin_f[k, s] ^= amb[s, cols]
            I_f, J_f = _sweep(np.broadcast_to(tau[:, cols], thin_f.shape), E[:, cols], dtau[:, :, cols], dE[:, :, cols],
                              I0[cols], thin_f, solo, False)
            A_I, A = A_I.copy(), A.copy()
            A_I[cols] += np.abs(I_f - I[cols]).sum(axis=0) / LD(EPS53)
            A[:, cols] += np.abs(J_f - J[:, cols]).sum(axis=0) / LD(EPS53)
    return dict(I=I, J=J, A_I=A_I, A=A, C_I=C_I, C=C, F=F)


def units(got, ref, A, C, n_gas, F=None):
    """|got - ref| / (2^-53 (A + (n_gas + 1) C [+ F]) + 1e-290), as fp64; a NaN or Inf in `got` is an error."""
    got = np.asarray(got)
    if not np.all(np.isfinite(got)):
        bad = np.argwhere(~np.isfinite(got))
        raise AssertionError("non-finite result at %d places, first at index %s" % (len(bad), tuple(bad[0])))
    bound = np.asarray(A, LD) + LD(n_gas + 1) * np.asarray(C, LD)
    if F is not None:
        bound = bound + np.asarray(F, LD)
    with np.errstate(under="ignore"):
        u = np.abs(np.asarray(got, LD) - np.asarray(ref, LD)) / (LD(EPS53) * bound + LD(FLOOR))
    return np.asarray(u, np.float64)


def products(coef, col, dtype):
    """sum_g coef[g] col[g] in `dtype`: coef [G, S, N] (fp64 coefficients of each segment's row), col [G, S] (fp64
    columns).  dtype long double: the reference's exact-input form; float64: what any fp64 implementation computes."""
    coef = np.asarray(coef, dtype)
    col = np.asarray(col, dtype)
    out = coef[0] * col[0][:, None]
    for g in range(1, coef.shape[0]):
        out = out + coef[g] * col[g][:, None]
    return out


# ------------------------------------------------------------------------------------------------------------------
# the yardstick: the same recursion in plain fp64
# ------------------------------------------------------------------------------------------------------------------
_FACT = np.cumprod(np.concatenate([[1.0], np.arange(1.0, 21.0)]))     # k!
DEFECTS = ("thin_at_1e-6", "fprime_half_to_1e-4", "exp_off_1e-13", "naive_f")


def plain_fp64(tau, E, dtau, dE, I0, solo=False, defect=None):
    """The recursion in plain numpy fp64: np.exp, np.expm1, IEEE division, path order, the thin rule, f' by its series
    below |tau| = 0.25 and by the closed form above; its inputs are
    fp64 (tau as the fp64 sum of products: products(..., np.float64)).  The yardstick of the tolerance, not a test
    subject.  defect: one of DEFECTS, a seeded fault for the tests of the bound's teeth.  Returns I [N], J [P, N]."""
    tau, E, dtau, dE, I0 = (np.asarray(v, np.float64) for v in (tau, E, dtau, dE, I0))
    assert defect is None or defect in DEFECTS
    S, N = tau.shape
    I = I0.copy()
    J = np.zeros((dtau.shape[0], N))
    with np.errstate(all="ignore"):
        for s in range(S):
            x = tau[s]
            thin = ~(np.abs(x) > (1e-6 if defect == "thin_at_1e-6" else THIN))
            xs = np.where(thin, 1.0, x)
            t = np.exp(-x)
            if defect == "exp_off_1e-13":
                t = t * (1.0 + 1e-13)
            em1 = (1.0 - t) if defect in ("naive_f", "exp_off_1e-13") else -np.expm1(-x)
            f = np.where(thin, 1.0, em1 / xs)
            # f': the closed form is a difference of nearly equal numbers below ~0.25 (good to 2^-53 / tau only): an
            # honest implementation takes the series there, as the reference does
            xt = np.where(np.abs(xs) < 0.25, xs, 0.0)
            fps = np.zeros_like(xt)
            for k in range(17, -1, -1):          # f' = sum_k -(k+1) (-x)^k / (k+2)!, Horner
                fps = fps * (-xt) - (k + 1.0) / _FACT[k + 2]
            fp = np.where(thin, -0.5, np.where(np.abs(xs) < 0.25, fps, (xs * t - em1) / (xs * xs)))
            if defect == "fprime_half_to_1e-4":
                fp = np.where(np.abs(x) <= 1e-4, -0.5, fp)
            src = -(I * t)[None, :] * dtau[:, s]
            if not solo:
                src = src + dE[:, s] * f[None, :] + (E[s] * fp)[None, :] * dtau[:, s]
            J = J * t[None, :] + src
            I = I * t if solo else I * t + E[s] * f
    return I, J


# ------------------------------------------------------------------------------------------------------------------
# the regime panel
# ------------------------------------------------------------------------------------------------------------------
def regime_panel(n_seg, rng, repeat=1):
    """The columns of the spectral axis, each its own regime: tau [n_seg, N] (N = 188), names [N], source [n_seg, N]
    (an O(1) source function, zero in every seventh column), I0 [N] (0 and a positive value in turn).
    - every segment equal to one special value;
    - one special segment at the start, the middle and the end of an O(0.01 ... 0.5) path;
    - 60 log-uniform mixtures over 1e-16 ... 1e3, every third with an opaque middle of six segments at 1e2 ... 1e4.
    Negative values are placed so that the total path tau stays above -20 when every row is crossed `repeat` times."""
    cols, names = [], []
    bg = lambda: 10.0 ** rng.uniform(-2.0, np.log10(0.5), n_seg)
    for v in SPECIAL:
        c = np.full(n_seg, v)
        if v < 0 and v * n_seg * repeat < MIN_PATH_TAU + 1.0:
            keep = max(1, int((-MIN_PATH_TAU - 1.0) / (-v * repeat)))
            c = bg()
            c[:keep] = v
        cols.append(c)
        names.append("all %g" % v)
    for where, pos in (("start", 0), ("middle", n_seg // 2), ("end", n_seg - 1)):
        for v in SPECIAL:
            c = bg()
            c[pos] = v
            cols.append(c)
            names.append("%s %g" % (where, v))
    for m in range(60):
        c = 10.0 ** rng.uniform(-16.0, 3.0, n_seg)
        tag = "mix %d" % m
        if m % 3 == 2:
            w = min(6, max(1, n_seg // 2))
            a = (n_seg - w) // 2
            c[a:a + w] = 10.0 ** rng.uniform(2.0, 4.0, w)
            tag += " opaque middle"
        cols.append(c)
        names.append(tag)
    tau = np.array(cols).T.copy()
    N = tau.shape[1]
    source = rng.uniform(0.5, 2.0, (n_seg, N))
    source[:, ::7] = 0.0
    I0 = np.where(np.arange(N) % 2 == 0, 0.0, rng.uniform(0.5, 3.0, N))
    return dict(tau=tau, names=names, source=source, I0=I0)


def emission_of(tau, source):
    """E of a segment from its tau and source function: source |tau|, and source x 1e-3 where tau is exactly 0 (emission
    without absorption is legal input)."""
    return source * np.where(tau == 0.0, 1e-3, np.abs(tau))


def tile_columns(n_panel, n_pts, rng):
    """Panel column of every point of a wider (or narrower) launch: the first tile in panel order, every further tile
    by its own permutation -- an indexing error cannot return the right number from the wrong column."""
    idx = [np.arange(n_panel)]
    while sum(len(i) for i in idx) < n_pts:
        idx.append(rng.permutation(n_panel))
    return np.concatenate(idx)[:n_pts]


def worst(u, names=None, cols=None):
    """(max units, description of where) of a units array whose last axis is the spectral axis."""
    u = np.asarray(u)
    if u.size == 0:
        return 0.0, "-"
    k = np.unravel_index(int(np.argmax(u)), u.shape)
    j = int(k[-1]) if cols is None else int(cols[k[-1]])
    return float(u[k]), ("%s (col %d%s)" % (names[j], j, ", index %s" % (k[:-1],) if len(k) > 1 else "")) if names else str(k)


def panel_problem(n_seg, n_gas, n_par, seed):
    """A coefficient-and-column statement of the panel for the host tests: abs_g[s, j] = share_g tau[s, j] / u_g[s],
    emi_g likewise from the source function, columns u_g[s] of O(1e18), and n_par column parameters (parameter p moves
    the column of gas p % n_gas on a random subset of the segments).  Returns the panel plus coef_a, coef_e [G, S, N],
    col [G, S], par_gas [P], dcol [P, S]."""
    rng = np.random.default_rng(seed)
    pan = regime_panel(n_seg, rng)
    share = rng.uniform(0.2, 1.0, n_gas)
    share /= share.sum()
    col = 10.0 ** rng.uniform(17.0, 19.0, (n_gas, n_seg))
    E = emission_of(pan["tau"], pan["source"])
    pan["coef_a"] = share[:, None, None] * pan["tau"][None] / col[:, :, None]
    pan["coef_e"] = share[:, None, None] * E[None] / col[:, :, None]
    pan["col"] = col
    pan["par_gas"] = np.arange(n_par) % n_gas
    pan["dcol"] = np.array([col[p % n_gas] * rng.uniform(0.0, 1.0, n_seg) * (rng.random(n_seg) < 0.7) for p in range(n_par)])
    return pan


def forms(coef_a, coef_e, col, par_gas, dcol, dtype):
    """tau, E [S, N] and dtau, dE [P, S, N] of a coefficient-and-column statement, the products formed in `dtype`."""
    tau = products(coef_a, col, dtype)
    E = products(coef_e, col, dtype)
    dtau = np.array([np.asarray(coef_a[g], dtype) * np.asarray(dcol[p], dtype)[:, None] for p, g in enumerate(par_gas)])
    dE = np.array([np.asarray(coef_e[g], dtype) * np.asarray(dcol[p], dtype)[:, None] for p, g in enumerate(par_gas)])
    return tau, E, dtau, dE
