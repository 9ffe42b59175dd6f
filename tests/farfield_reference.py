"""Extended-precision CPU model of ONE line's far-field expansion over ONE box (sr_kernels.hip, "far field by local
(Taylor) expansions"): the region-1 rational of the reference (lineshape.f:456-478),

    w(x, ry) = (a + b x^2) / (c + x^2 (d + 4 x^2)),      x = (grid point - line centre) / dw',

its degree-n Taylor series in t = (j - box centre) / h over a box of W = 64 << level points (h = W / 2, the points at
t = +-(k - 1/2) / h), by power-series division of the quadratic by the quartic, and what the truncated series differs by
from w itself, relative to w -- the quantity sr_far_field_truncation_bound() speaks of ("of a line's own contribution").
Written from those formulas in numpy.longdouble (x87 extended: 64-bit mantissa), with a plain fp64 restatement of the same
recurrence and Horner evaluation beside it as the yardstick of rounding.  Where a box may take a line is NOT restated
here: min_distance() asks the library (engine.far_field_min_distance -> sr_far_field_min_distance, the expression the
kernels compile).  A helper module: no fixture, no pytest setting.

Geometry.  `distance`: grid points between the box centre (a half point) and the line's centre INDEX, as the kernels'
integer test sees it; `offset`: where the line's true centre sits relative to that index, in points (|offset| <= 1/2:
the index is the nearest grid point).  xstep = grid step / dw' (FastRec::xstep).
"""
import numpy as np

LD = np.longdouble
assert np.finfo(LD).eps < 2e-19, "numpy.longdouble is not an extended-precision type here: no reference, no fallback"

EPS53 = 2.0 ** -53

# The contract's panel (tests/test_farfield_reference_host.py): (xstep, ry) from a Doppler line on a fine grid, whose
# double poles at |x| = 0.71 sit hundreds of points out, to grids 20 dw' coarse and Lorentz wings (ry = 100), and the
# line's centre on its index or half a point to either side of it.
PANEL = ((0.0025, 1e-3), (0.05, 0.01), (0.05, 5.0), (0.5, 0.5), (2.0, 1e-3), (2.0, 100.0), (20.0, 1e-4))
OFFSETS = (0.0, 0.5, -0.5)
LEVELS = (0, 1, 2, 3, 4)

# K_PLAIN_FAR: max over the panel (levels x PANEL x OFFSETS, nearest admissible distance, the library's degree) of
# |series_fp64 - series_longdouble| / |w| in units of 2^-53 -- the distance of an honest fp64 implementation of the
# expansion (IEEE division, the recurrence and Horner with separate multiplies and adds) from the reference.  The GPU
# tests allow the kernels bound + 8 x K_PLAIN_FAR x 2^-53 (reciprocal + Newton steps for the division, the lane
# reduction's order, the L2L fold; the factor of tests/limb_reference.py).  Measured 2026-10-18: 9.69 (level 4,
# xstep 0.05, ry 0.01, centre on its index; nowhere on the panel below 3).
# Recorded as 14.5, the measurement x 1.5 (14.535) cut to three figures; test_k_plain_far_recorded_and_respected asserts
# that the live value stays below it.
K_PLAIN_FAR_MEASURED = 9.69
K_PLAIN_FAR = 14.5
KERNEL_MARGIN = 8.0


def region1_coef(ry, dtype=LD):
    """a, b, c, d of lineshape.f:456-459 (the reference's literals), in `dtype`."""
    ry = np.asarray(ry, dtype)
    one, two = dtype(1), dtype(2)
    ry2 = ry * ry
    a = ry * (dtype(1.1283792) + dtype(2.2567584) * ry2)
    b = dtype(2.2567584) * ry
    c = (one + two * ry2) * (one + two * ry2)
    d = dtype(-4) + dtype(8) * ry2
    return a, b, c, d


def rational(x, ry, dtype=LD):
    """w(x, ry) in `dtype` (IEEE division)."""
    a, b, c, d = region1_coef(ry, dtype)
    x = np.asarray(x, dtype)
    x2 = x * x
    return (a + b * x2) / (c + x2 * (d + dtype(4) * x2))


def series_coefficients(xc, e, ry, degree, dtype=LD):
    """f_0 .. f_degree of w(xc + e t, ry) = sum_n f_n t^n: numerator n_0 + n_1 t + n_2 t^2, denominator d_0 + ... + d_4 t^4
    (x^2 = u_0 + u_1 t + u_2 t^2), f_n = (n_n - sum_(k=1..4) d_k f_(n-k)) / d_0."""
    a, b, c, d = region1_coef(ry, dtype)
    xc, e = dtype(xc), dtype(e)
    u0, u1, u2 = xc * xc, dtype(2) * xc * e, e * e
    num = [a + b * u0, b * u1, b * u2]
    den = [c + u0 * (d + dtype(4) * u0), u1 * (d + dtype(8) * u0), u2 * d + dtype(4) * (u1 * u1 + dtype(2) * u0 * u2),
           dtype(8) * u1 * u2, dtype(4) * u2 * u2]
    f = []
    for n in range(degree + 1):
        s = num[n] if n < 3 else dtype(0)
        for k in range(1, min(4, n) + 1):
            s = s - den[k] * f[n - k]
        f.append(s / den[0])
    return f


def horner(f, t):
    t = np.asarray(t, type(f[0]))
    y = np.full(t.shape, f[-1], dtype=t.dtype)
    for c in f[-2::-1]:
        y = y * t + c
    return y


def box_points(level, dtype=LD):
    """t of the W = 64 << level points of a box: +-(k - 1/2) / h."""
    W = 64 << level
    h = dtype(W // 2)
    return (np.arange(W).astype(dtype) + dtype(0.5) - h) / h


def box_series(level, xstep, ry, distance, degree, offset=0.0, dtype=LD, t=None):
    """(series, w, t) over the box's points (or the given t) for a line whose centre index is `distance` points from the
    box centre and whose centre sits `offset` points beyond that index, seen from the box."""
    h = 32 << level
    xstep = dtype(xstep)
    xc = (dtype(distance) + dtype(offset)) * xstep
    e = dtype(h) * xstep
    t = box_points(level, dtype) if t is None else np.asarray(t, dtype)
    f = series_coefficients(xc, e, ry, degree, dtype)
    return horner(f, t), rational(xc + e * t, ry, dtype), t


def truncation(level, xstep, ry, distance, degree, offset=0.0, where=False):
    """max over the box's points of |series - w| / |w| in long double (with where=True also the t it is reached at)."""
    s, w, t = box_series(level, xstep, ry, distance, degree, offset)
    err = np.abs(s - w) / np.abs(w)
    k = int(np.argmax(err))
    return (float(err[k]), float(t[k])) if where else float(err[k])


def plain_rounding(level, xstep, ry, distance, degree, offset=0.0):
    """max |series_fp64 - series_longdouble| / |w| in units of 2^-53: what fp64 arithmetic alone costs the expansion."""
    s_ld, w, _ = box_series(level, xstep, ry, distance, degree, offset)
    s_64, _, _ = box_series(level, xstep, ry, distance, degree, offset, dtype=np.float64)
    return float(np.max(np.abs(s_64.astype(LD) - s_ld) / np.abs(w))) / EPS53


def remainder_inverse_square(r, degree):
    """(facing edge, far edge) of a wing ~ 1/x^2 at r = h / distance, relative to the line's value there:
    (D + h t)^-2 = D^-2 sum_n (n + 1) (-r t)^n, the terms n > d summed and divided by (1 + r t)^-2 at t = -1 / +1:
    (d + 2 - (d + 1) r) r^(d+1) and (d + 2 + (d + 1) r) r^(d+1)."""
    r = LD(r)
    p = r ** (degree + 1)
    return float((degree + 2 - (degree + 1) * r) * p), float((degree + 2 + (degree + 1) * r) * p)


def pole_margin(xstep):
    """The layer's pole margin in grid points as the host sets it for a line of Doppler width dw' = step / xstep
    (sr_api.hip fill_layer_stage: ceil(0.71 dw' / step) + 1)."""
    return int(np.ceil(0.71 / xstep)) + 1


def min_distance_pm(level, pm):
    """Nearest admissible distance of a level's box for a layer of pole margin pm, from the library itself."""
    from spectrobot_amd import engine
    return engine.far_field_min_distance(level, pm)


def min_distance(level, xstep):
    return min_distance_pm(level, pole_margin(xstep))
