"""The definition of a tabulated absorber on coefficient rows (include/spectrobot_hip.h: sr_abs_table_*),
written from the formulas in numpy.longdouble (x87 extended: 64-bit mantissa), with the bound a double evaluation is held
to, per point.  The build's own definition: the reference project has no counterpart.

    nu_j   = w0 + (double)(g_lo + j) step            the double the kernel forms (unfused), taken as exact from here on
    t      = (nu_j - v0_k) / dv_k,  i = floor(t)
    s_k(j) = a_k[i] + (a_k[i+1] - a_k[i]) (t - i)     0 <= i <= n_k - 2;   a_k[n_k - 1] at t == n_k - 1;   0 outside
    abs    = c (w_lo s_lo + w_hi s_hi)               emi  = source ? abs B(nu_j, T) : 0
    dabs   = c (dw_lo s_lo + dw_hi s_hi)             demi = source ? dabs B + abs dB/dT : 0
    B      = 2 h c^2 nu^3 / (exp(x) - 1), x = c2 nu / T;    dB/dT = B (x / T) e^x / (e^x - 1)

h, c, c2 are the library's doubles (sr_constants.hpp).  The rows' plan (set2, w2, dw2) is an INPUT, as it is for the
kernel; plan() below states the host policy of engine.AbsorberTable.plan in long double.  Loops over rows and sets,
numpy over the grid points.  evaluate(..., dtype=np.float64) is the same text in double: the plain fp64 restatement that
serves as the yardstick of the bounds (tests/test_absorber_table_host.py holds it to half of each).

The bounds, eps = 2^-53:
    b_abs  = eps [ 8 c (|w_lo s_lo| + |w_hi s_hi|) + 4 c sum_k |w_k| |t_k| |a_k[i+1] - a_k[i]| ]
             (the second term: the rounding of the position t -- one subtraction, one division -- times the local slope;
              it dominates at large indices and is a property of the problem)
    b_emi  = b_abs B + eps (8 + 2 x) |emi|                          (the condition number of the exponential)
    b_dabs = b_abs with dw for w
    b_demi = b_dabs B + eps (8 + 2 x) |dabs B| + b_abs dB/dT + eps (12 + 2 x) |abs dB/dT|
             (dB/dT = B times x / T times e^x / (e^x - 1): two divisions and two products more than B, the last factor's
              condition number x / (e^x - 1) < 1 for the windows used here, x >= 2)
A point within a rounding of a set's range END is outside the bounds' reach (the definition jumps there): the test
cases put grid points exactly on an end or well between.  A helper module: no fixture, no pytest setting.
"""
import numpy as np

LD = np.longdouble
assert np.finfo(LD).eps < 2e-19, "numpy.longdouble is not an extended-precision type here: no reference, no fallback"

EPS = 2.0 ** -53
H_CGS = 6.62607015e-34 * 1.e7
C_CGS = 299792458.0 * 1.e2
K_CGS = 1.380649e-23 * 1.e7
C2 = H_CGS * C_CGS / K_CGS


def grid_nu(w0, step, g_lo, n_pts):
    """The doubles nu_j = w0 + (double)(g_lo + j) step, unfused."""
    return np.float64(w0) + (np.arange(n_pts) + int(g_lo)).astype(np.float64) * np.float64(step)


def interp_set(nu, v0, dv, values, dtype=LD):
    """s_k at the points nu, the position t, |a[i+1] - a[i]| of the interval used, and the membership mask."""
    a = np.asarray(values, dtype=np.float64).astype(dtype)
    n = a.size
    t = (nu.astype(dtype) - dtype(v0)) / dtype(dv)
    inside = (t >= 0) & (t <= n - 1)
    i = np.clip(np.floor(np.where(inside, t, 0)).astype(np.int64), 0, n - 1)
    i1 = np.minimum(i + 1, n - 1)
    s = np.where(inside, a[i] + (a[i1] - a[i]) * (t - i.astype(dtype)), dtype(0))
    slope = np.where(inside, np.abs(a[i1] - a[i]), dtype(0))
    return s, np.where(inside, t, dtype(0)), slope, inside


def _two_prod(a, b):
    """a b = p + e exactly, in double (Veltkamp splitting and Dekker's product: numpy has no fused multiply-add)."""
    def split(v):
        c = 134217729.0 * v
        hi = c - (c - v)
        return hi, v - hi
    p = a * b
    (ah, al), (bh, bl) = split(a), split(b)
    return p, ((ah * bh - p) + ah * bl + al * bh) + al * bl


def planck(nu, T, dtype=LD):
    """B, dB/dT and x = c2 nu / T at the points nu, row temperature T.  In double, exp(x) is taken as the kernel takes it:
    x~ = (c2 nu)(1 / T) with its exact residual against the unrounded quotient, exp(x) = exp(x~)(1 + dx) -- x rounded twice
    would alone spend the emission bound's eps 2 x."""
    if dtype is np.float64:
        nu, T = nu.astype(np.float64), np.float64(T)
        p, p_lo = _two_prod(np.float64(C2), nu)
        rT = 1.0 / T
        x = p * rT
        q, q_lo = _two_prod(x, T)
        dx = (((p - q) - q_lo) + p_lo) * rT
        ex = np.exp(x)
        ex = ex + ex * dx
    else:
        nu, T = nu.astype(dtype), dtype(T)
        x = dtype(C2) * nu / T
        ex = np.exp(x)
    B = dtype(2) * dtype(H_CGS) * (dtype(C_CGS) * dtype(C_CGS)) * (nu * nu * nu) / (ex - dtype(1))
    return B, B * (x / T) * (ex / (ex - dtype(1))), x


def evaluate(sets, set2, w2, dw2, temps, scale, w0, step, g_lo, n_pts, source=True, dtype=LD):
    """sets: [(T, v0, dv, values[, P])]; set2 / w2 / dw2 [n_rows][2] (dw2 None: zeros); scale None or [n_rows].
    Returns a dict of [n_rows][n_pts] arrays of `dtype`: abs, emi, dabs, demi, their bounds b_abs, b_emi, b_dabs, b_demi,
    and B, x."""
    nu = grid_nu(w0, step, g_lo, n_pts)
    n_rows = len(temps)
    set2 = np.asarray(set2).reshape(n_rows, 2)
    w2 = np.asarray(w2, dtype=np.float64).reshape(n_rows, 2)
    dw2 = np.zeros((n_rows, 2)) if dw2 is None else np.asarray(dw2, dtype=np.float64).reshape(n_rows, 2)
    cache = {}
    out = {k: np.zeros((n_rows, n_pts), dtype=dtype) for k in ("abs", "emi", "dabs", "demi", "b_abs", "b_emi", "b_dabs", "b_demi",
                                                               "B", "x")}
    eps = dtype(EPS)
    for r in range(n_rows):
        c = dtype(1) if scale is None else dtype(np.float64(scale[r]))
        terms = []
        for q in range(2):
            k = int(set2[r, q])
            if k not in cache:
                cache[k] = interp_set(nu, sets[k][1], sets[k][2], sets[k][3], dtype)
            terms.append(cache[k])
        (s_lo, t_lo, d_lo, _), (s_hi, t_hi, d_hi, _) = terms
        B, dB, x = planck(nu, temps[r], dtype)
        out["B"][r], out["x"][r] = B, x
        for name, w in (("abs", w2[r]), ("dabs", dw2[r])):
            wl, wh = dtype(w[0]), dtype(w[1])
            out[name][r] = c * (wl * s_lo + wh * s_hi)
            out["b_" + name][r] = eps * (8 * np.abs(c) * (np.abs(wl * s_lo) + np.abs(wh * s_hi)) +
                                         4 * np.abs(c) * (np.abs(wl) * np.abs(t_lo) * d_lo + np.abs(wh) * np.abs(t_hi) * d_hi))
        if source:
            a, da = out["abs"][r], out["dabs"][r]
            out["emi"][r] = a * B
            out["demi"][r] = da * B + a * dB
            out["b_emi"][r] = out["b_abs"][r] * B + eps * (8 + 2 * x) * np.abs(a * B)
            out["b_demi"][r] = (out["b_dabs"][r] * B + eps * (8 + 2 * x) * np.abs(da * B) + out["b_abs"][r] * dB +
                                eps * (12 + 2 * x) * np.abs(a * dB))
    return out


def plan(set_temp, set_press, temps, press=None):
    """The host policy (engine.AbsorberTable.plan) in long double: set2 [n][2], w2, dw2 [n][2] (LD).  With labels and
    press the group nearest in ln P (ties: the lower pressure), else all sets; linear in T inside the group, clamped
    outside (w = (1, 0), dw = 0); a row exactly at a set takes it with weight 1 and the derivative of the interval above,
    0 at the hottest set."""
    set_temp = np.asarray(set_temp, dtype=np.float64)
    temps = np.atleast_1d(np.asarray(temps, dtype=np.float64))
    n = temps.size
    use_p = set_press is not None and press is not None
    if use_p:
        set_press = np.asarray(set_press, dtype=np.float64)
        press = np.broadcast_to(np.asarray(press, dtype=np.float64), (n,))
        labels = sorted(set(set_press.tolist()))
    set2, w2, dw2 = np.zeros((n, 2), np.int32), np.zeros((n, 2), LD), np.zeros((n, 2), LD)
    for r in range(n):
        idx = np.arange(set_temp.size)
        if use_p:
            dist = [abs(np.log(LD(press[r])) - np.log(LD(p))) for p in labels]
            best = min(range(len(labels)), key=lambda g: (dist[g], labels[g]))
            idx = idx[set_press == labels[best]]
        idx = idx[np.argsort(set_temp[idx], kind="stable")]
        tk, T = set_temp[idx], temps[r]
        if T < tk[0] or T >= tk[-1]:
            k = idx[0] if T < tk[0] else idx[-1]
            set2[r], w2[r] = (k, k), (1, 0)
            continue
        k = max(q for q in range(idx.size) if tk[q] <= T)
        span = LD(tk[k + 1]) - LD(tk[k])
        hi = (LD(T) - LD(tk[k])) / span
        set2[r], w2[r], dw2[r] = (idx[k], idx[k + 1]), (1 - hi, hi), (-1 / span, 1 / span)
    return set2, w2, dw2


GRID = (2900.0, (2900.0 + 0.01) - 2900.0, 300)   # w0, step (the difference of the grid's first two doubles, which is what
                                                 # engine.grid_params reads), points: a full block of 256 and a partial one; c2 nu / T >= 13 for T <= 310 K
ROW_TEMPS = np.array([140.0, 200.0, 170.0, 230.0, 310.0])   # below the coldest set, exactly at a set, between two sets
ROW_PRESS = np.array([0.5, 1.0, 3.0, 10.0, 30.0])           # twice, above the hottest set
ROW_SCALE = np.array([1.0, 1e5, 1e9, 1e14, 1e18])
SET_TEMPS = (150.0, 200.0, 250.0, 300.0)
SET_PRESS = (1.0, 1.0, 20.0, 20.0)


def panel_sets(g_lo, seed=20261020, labels=False):
    """The four sets of the kernel's test panel for the shard starting at g_lo: one finer than the grid, one coarser, one
    covering points 100 .. 180 (its lower end bitwise grid point 100, its upper end 0.4 steps above point 180), one whose
    last knot is bitwise grid point 256, the block boundary.  Values ~1e-20 with some negative ones."""
    w0, step, n = GRID
    nu = grid_nu(w0, step, g_lo, n)
    rng = np.random.default_rng([seed, g_lo])
    axes = [(nu[0] - 0.013, step / 3.7, 1120), (nu[0] - 0.5, 0.13, 40),
            (nu[100], (nu[180] + 0.4 * step - nu[100]) / 32.0, 33), (nu[256] - 2.0, 0.015625, 129)]
    assert (nu[100] - axes[2][0]) / axes[2][1] == 0.0 and (nu[256] - axes[3][0]) / axes[3][1] == 128.0, "panel not exact"
    sets = []
    for k, (v0, dv, m) in enumerate(axes):
        s = (SET_TEMPS[k], float(v0), float(dv), 1e-20 * (rng.uniform(size=m) - 0.1))
        sets.append(s + (SET_PRESS[k],) if labels else s)
    return sets
