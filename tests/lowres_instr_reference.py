"""Extended-precision CPU reference of the instrument step's two INSTRUMENT derivatives (the comment above
sr_lowres_weights_kernel; sr_hires_to_lowres_instr_shard_dev): with the notation of tests/lowres_reference.py,

    x_i = 1e7 / g_i,   t_i = (x_i - f) / w,   band = k sum_i s_i W_i  over the window lo <= x_i <= hi,

and the window's MEMBERSHIP HELD FIXED (it is piecewise constant in f and w: between its jumps the sums below are the
exact derivatives of the value, a jump is of relative size exp(-n_sigma^2 / 2)),

    centre f -> f + delta (nm):   d band / d delta = k sum_i s_i W_i t_i / w
    width  w -> w e^eta:          d band / d eta   = k sum_i s_i W_i (t_i^2 - 1)

(W_i = u_i c_i, u_i = g_i^2 1e-7 exp(-t_i^2 / 2) / (w sqrt(2 pi)): d u / d f = u t / w; d u / d ln w = u (t^2 - 1), t^2
from the exponential and -1 from the normalisation; the interval widths c_i do not depend on the band.)

The grid, the window, the panel and the unit factors are those of tests/lowres_reference.py, imported from there; what is
fp64 data and what is long double is as there: the nm grid and the window's selection in fp64, everything after it --
t, the Gaussian, the factors t / w and t^2 - 1, the products, the sums -- in numpy.longdouble.

The unit.  A result's error is measured, as the value's, in units of

    2^-53 A + 1e-290,   A = the sum of the terms' magnitudes, each with what one rounding of t costs it.

A rounding of t, t -> t (1 + e), moves a term s W F(t) by
    s W F t^2 e                 through the exponential (d exp(-t^2 / 2) = -t^2 (dt / t) exp(-t^2 / 2): the value's term), and by
    s W (dF / dt) t e           through the factor F:  F = t / w: (t / w) e, i.e. |F| e;   F = t^2 - 1: 2 t^2 e,
so, with the 1 of the value's unit for the term's own roundings,

    A_centre = sum_i |s_i W_i| (|t_i| / w) (1 + t_i^2 + 1)  =  sum_i |s_i W_i| |t_i| (2 + t_i^2) / w
    A_width  = sum_i |s_i W_i| (|t_i^2 - 1| (1 + t_i^2) + 2 t_i^2)

The second is not |term| times a factor: where t^2 is near 1 the factor t^2 - 1 cancels, and what a rounding of t leaves
there (2 t^2 e) is counted in full.  x - f and the interval widths are differences of neighbouring fp64 values, as in the
value's unit.

plain_fp64_instr is the same three sums in plain numpy fp64, written here (never taken from a kernel): the yardstick of
the bound (K_PLAIN_INSTR) and the restatement that takes seeded defects.  A helper module: no fixture, no pytest setting.
"""
import numpy as np

import lowres_reference as R

LD = R.LD
ROWS = ("value", "d / d centre", "d / d ln width")

# K_PLAIN_INSTR: max units(plain_fp64_instr, reference) over the two derivative rows of every (spectrum, band) pair of
# the panel below -- the distance of an honest fp64 evaluation (libm exp, IEEE division, numpy's sums) from the reference
# in the bound's own units.  A kernel's limit is KERNEL_MARGIN x max(K_PLAIN_INSTR over the test's own pairs, 1), never
# taken from a kernel.  Measured 2026-10-18 on panel(2975.0, 5e-4, 8193, 33, 20261018), n_sigma 5, 'Wm2' (33 bands, 2 dense
# + 305 one-hot spectra): 4.6 units, the width's row of a one-hot spectrum under a random band (a single weight: the
# roundings of t, of t t, of the exponential's argument and libm's exp; the centre's row measures 3.8, on the signed dense spectrum).  The recorded constant
# is 1.5 x the measurement and may be at most 2 x it; tests/test_lowres_instr_reference_host.py asserts that the live
# measurement does not exceed it.
K_PLAIN_INSTR_MEASURED = 4.6
K_PLAIN_INSTR = 6.9
K_PLAIN_INSTR_PANEL = R.K_PLAIN_PANEL


def weights_instr(grid, centers, widths, n_sigma=5.0, g_lo=0, n_sh=None):
    """The three weight tables in long double, in cm-1 index order of the shard: W [3, n_bands, n_sh] (the value's, the
    centre's, the width's; zero outside a window and for a window of fewer than two points), the tables of the unit
    AW [3, n_bands, n_sh] (|W| times the conditioning factor of the docstring), count [n_bands]."""
    g, x = R._shard(grid, g_lo, n_sh)
    n = x.size
    centers, widths = np.asarray(centers, np.float64), np.asarray(widths, np.float64)
    W, AW = np.zeros((3, centers.size, n), LD), np.zeros((3, centers.size, n), LD)
    count = np.zeros(centers.size, np.int64)
    gl, xl = g.astype(LD), x.astype(LD)
    root_2pi = np.sqrt(LD(2) * np.arctan(LD(1)) * LD(4))
    for b, (f, w) in enumerate(zip(centers, widths)):
        i0, i1, _, _ = R._window(x, f, w, n_sigma)
        count[b] = i1 - i0
        if i1 - i0 < 2:
            continue
        xs, gs = xl[i0:i1], gl[i0:i1]
        t = (xs - LD(f)) / LD(w)
        with np.errstate(under="ignore"):
            u = gs * gs * R._ten(-7) * (np.exp(-t * t / LD(2)) / (LD(w) * root_2pi))
        c = np.empty(i1 - i0, LD)
        c[1:-1] = (xs[2:] - xs[:-2]) / LD(2)
        c[0] = (xs[1] - xs[0]) / LD(2)
        c[-1] = (xs[-1] - xs[-2]) / LD(2)
        with np.errstate(under="ignore"):
            wv = u * c
            t2 = t * t
            rows = (wv, wv * t / LD(w), wv * (t2 - LD(1)))
            cond = (np.abs(wv) * (LD(1) + t2), np.abs(wv) * np.abs(t) * (LD(2) + t2) / LD(w),
                    np.abs(wv) * (np.abs(t2 - LD(1)) * (LD(1) + t2) + LD(2) * t2))
        for k in range(3):
            W[k, b, n - i1:n - i0] = rows[k][::-1]
            AW[k, b, n - i1:n - i0] = cond[k][::-1]
    return W, AW, count


def band_reference_instr(grid, spec, centers, widths, n_sigma=5.0, units="Wm2", g_lo=0):
    """The value and the two instrument derivatives of the bands of spec [n_spec, n_sh] (a shard: its partial sums) in
    long double.  Returns a dict: value, A [n_spec, 3, n_bands] (rows: ROWS; long double, in `units`; the centre's row per
    nm), count [n_bands], guard [n_bands].  Row 0 is lowres_reference.band_reference's value and A."""
    spec = np.atleast_2d(np.asarray(spec, np.float64))
    n_sh = spec.shape[1]
    W, AW, count = weights_instr(grid, centers, widths, n_sigma, g_lo, n_sh)
    val, A = np.zeros((spec.shape[0], 3, W.shape[1]), LD), np.zeros((spec.shape[0], 3, W.shape[1]), LD)
    with np.errstate(under="ignore"):
        for r in range(spec.shape[0]):
            idx = np.flatnonzero(spec[r])
            s = spec[r, idx].astype(LD)
            val[r] = (W[:, :, idx] * s[None, None, :]).sum(axis=2)
            A[r] = (AW[:, :, idx] * np.abs(s)[None, None, :]).sum(axis=2)
    k = R.unit_factor(units)
    return dict(value=val * k, A=A * k, count=count, guard=R.guard(grid, centers, widths, n_sigma, g_lo, n_sh))


def units_of(got, ref):
    """|got - value| / (2^-53 A + 1e-290) of a [n_spec, 3, n_bands] result, as fp64."""
    return R.units_raw(got, ref["value"], ref["A"])


DEFECTS = ("t_sign", "t2_without_minus_one", "missing_inverse_width", "dband16_gets_dband0", "derivative_tiles_get_value_tiles")


def plain_fp64_instr(grid, spec, centers, widths, n_sigma=5.0, units="Wm2", g_lo=0, defect=None):
    """The three weight tables and their products with the spectra in plain numpy fp64, as the kernels organise them:
    [n_spec, 3, n_bands].  defect: one of DEFECTS, a seeded fault for the tests of the bound's teeth."""
    assert defect is None or defect in DEFECTS
    spec = np.atleast_2d(np.asarray(spec, np.float64))
    n = spec.shape[1]
    g, x = R._shard(grid, g_lo, n)
    centers, widths = np.asarray(centers, np.float64), np.asarray(widths, np.float64)
    W = np.zeros((3, centers.size, n))
    for b, (f, w) in enumerate(zip(centers, widths)):
        lo, hi = f - n_sigma * w, f + n_sigma * w
        sel = np.flatnonzero((x >= lo) & (x <= hi))
        if sel.size < 2:
            continue
        i0, i1 = int(sel[0]), int(sel[-1]) + 1
        xs, gs = x[i0:i1], g[i0:i1]
        t = (xs - f) / w
        with np.errstate(under="ignore"):
            u = ((gs * gs) * 1.e-7) * ((1 / (w * np.sqrt(2. * np.pi))) * np.exp(-0.5 * (t * t)))
            c = np.empty(i1 - i0)
            c[1:-1] = (xs[2:] - xs[:-2]) / 2.0
            c[0], c[-1] = (xs[1] - xs[0]) / 2.0, (xs[-1] - xs[-2]) / 2.0
            wv = u * c
            tc = -t if defect == "t_sign" else t
            fc = tc if defect == "missing_inverse_width" else tc / w
            fw = t * t if defect == "t2_without_minus_one" else t * t - 1.0
            rows = (wv, wv * fc, wv * fw)
        for k in range(3):
            W[k, b, n - i1:n - i0] = rows[k][::-1]
    if defect == "dband16_gets_dband0" and centers.size > R.TILE:
        W[1:, R.TILE] = W[1:, 0]
    if defect == "derivative_tiles_get_value_tiles":
        W[1], W[2] = W[0], W[0]
    with np.errstate(under="ignore"):
        v = np.einsum("rj,kbj->rkb", spec, W)
    v = v * 1.e-3
    if units == "ergscm2":
        v = v * 1.e3
    if units == "nWcm2":
        v = v * 1.e5
    return v


def measure_k_plain_instr(P=None):
    """(max units over the derivative rows, where) of plain_fp64_instr on a panel (default: K_PLAIN_INSTR_PANEL)."""
    P = R.panel(*K_PLAIN_INSTR_PANEL) if P is None else P
    ref = band_reference_instr(P["grid"], P["spec"], P["centers"], P["widths"], P["n_sigma"])
    u = units_of(plain_fp64_instr(P["grid"], P["spec"], P["centers"], P["widths"], P["n_sigma"]), ref)
    k, worst = 0.0, "-"
    for row in (1, 2):
        m, where = R.worst(u[:, row], P["spec_names"], P["band_names"])
        if m >= k:
            k, worst = m, "%s | %s" % (ROWS[row], where)
    return k, worst
