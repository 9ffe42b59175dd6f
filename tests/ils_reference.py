"""Extended-precision CPU reference of the instrument step under a TABULATED line shape (sr_set_ils; the comment above
sr_lowres_weights_tab_kernel): with the notation of tests/lowres_reference.py,

    x_i = 1e7 / g_i,   t_i = (x_i - f) / w,   p_i = g_i^2 1e-7 c_i   (c_i: the trapezoid interval weights, half at the ends)
    window of a band:  f + t_lo w <= x_i <= f + t_hi w
    value              band   = k sum_i s_i p_i phi^(t_i) / w
    d / d centre (nm)  band_f = -k sum_i s_i p_i phi^'(t_i) / w^2
    d / d ln width     band_w = -k sum_i s_i p_i (phi^(t_i) + t_i phi^'(t_i)) / w

the window's MEMBERSHIP HELD FIXED in the two derivative rows.  phi^ is the cubic Hermite interpolant of n_tab knots phi_k
at t_lo + k h, h = (t_hi - t_lo) / (n_tab - 1): slopes m_k = (phi_(k+1) - phi_(k-1)) / (2 h) inside, (phi_1 - phi_0) / h and
(phi_(n-1) - phi_(n-2)) / h at the ends; on interval k = clamp(floor((t - t_lo) / h), 0, n_tab - 2), s = (t - t_lo) / h - k,

    phi^  = (1 + 2 s)(1 - s)^2 phi_k + s (1 - s)^2 h m_k + s^2 (3 - 2 s) phi_(k+1) + s^2 (s - 1) h m_(k+1)
    phi^' = the derivative of the same cubic,   phi^'' its second derivative (the unit needs it)

One table for all bands (phi [1, n_tab]) or one per band (phi [n_bands, n_tab]).

The grid, the panel, the unit factors and the error measure are those of tests/lowres_reference.py, imported from there.
What is fp64 DATA and what is long double: the grid, the spectrum, the centres, the widths, t_lo, t_hi and the knots are
fp64 data; the nm grid and the window's selection (lo = f + t_lo w, hi = f + t_hi w) are fp64, as there: which points
belong to a band is part of the definition.  Everything after that -- t, h, the slopes, the interval index, the cubic,
the products, the sums, the unit factors -- is numpy.longdouble.  (With t_lo = -n_sigma, t_hi = n_sigma the fp64 window
ends are bitwise those of the Gaussian's window: the panel's windows of 1, 2, 3 points, its chunk and slot edges carry
over.)

The unit.  A result's error is measured in units of 2^-53 A + 1e-290.  A sums, per term, the magnitudes of what is added
up to form it -- the FOUR Hermite contributions, not their possibly cancelling sum phi^ (a lobed table passes through
zero where its contributions do not) -- and what ONE rounding of t, t -> t (1 + e), costs the term:

    value:   s p / w   x (sum_j |c_j|                             + |t phi^'|)
    centre:  s p / w^2 x (sum_j |e_j| / h                         + |t phi^''|)
    width:   s p / w   x (sum_j |c_j| + |t| sum_j |e_j| / h       + |t| (2 |phi^'| + |t phi^''|))

with c_j the four terms of phi^ above and e_j / h the four terms of phi^' (6 s (1 - s) phi_(k+1), -6 s (1 - s) phi_k,
-(3 s - 1)(1 - s) h m_k, s (3 s - 2) h m_(k+1), over h).  The rounding terms: d phi^(t) = phi^' t e; d phi^'(t) = phi^'' t e;
d (phi^ + t phi^') = (2 phi^' + t phi^'') t e.  The interval widths and x - f are differences of neighbouring fp64 values, as
in the value's unit.  What the unit does NOT count is the rounding of t - t_lo (it costs phi^' ulp(t_lo), not phi^' t e)
and of h: an honest fp64 evaluation pays them, and K_PLAIN_ILS below measures what they come to in these units.

The guard is lowres_reference.guard's, generalised to the table's window ends (guard_ils).

plain_fp64_ils is the same three sums in plain numpy fp64, written here from the formulas above (never taken from a
kernel): the yardstick of the bound (K_PLAIN_ILS) and the restatement that takes seeded defects.  A helper module: no
fixture, no pytest setting.
"""
import numpy as np

import lowres_reference as R

LD = R.LD
ROWS = ("value", "d / d centre", "d / d ln width")

# K_PLAIN_ILS: max units(plain_fp64_ils, reference) over the three rows of every (spectrum, band) pair of the panel below
# under lobed_tables(33) (one table per band) and under its first table shared by all bands -- the distance of an honest
# fp64 evaluation from the reference in the bound's own units.  A kernel's limit is KERNEL_MARGIN x max(K_PLAIN_ILS over
# the test's own pairs, 1) (lowres_reference.limit), never taken from a kernel.  Measured 2026-10-19 on
# panel(2975.0, 5e-4, 8193, 33, 20261018) (33 bands, 2 dense + 305 one-hot spectra), 'Wm2': 554 units, the centre's row of
# the one-hot spectrum in the middle of the 3-point window under its own table.  That point has t = 8e-7: phi^' there is
# the table's small skew slope, so the unit (|phi^'| and |t phi^''|) is tiny, while t - t_lo is rounded to half an ulp of
# t_lo = -5 and (t - t_lo) / h to half an ulp of 80 -- 5e-16 in t, through phi^'' = -3.3 phi(0): the rounding the unit
# leaves out, measured.  The next largest pair measures 16.8; the dense spectra 4.2, 3.7 and 0.7 units in the three rows,
# the one-hot spectra 5.6 and 3.6 in the value's and the width's.  The recorded constant is
# 1.5 x the measurement and may be at most 2 x it; tests/test_ils_reference_host.py asserts that the live measurement does
# not exceed it.
K_PLAIN_ILS_MEASURED = 554.3
K_PLAIN_ILS = 1.5 * K_PLAIN_ILS_MEASURED
K_PLAIN_ILS_PANEL = R.K_PLAIN_PANEL

# The Gaussian as a table (n_tab = 641 on +-5, exp(-t^2 / 2) / sqrt(2 pi) as given) against the closed-form Gaussian's
# reference (lowres_instr_reference.band_reference_instr) on gaussian_check_bands(): the largest difference of a row over
# the row's largest magnitude.  The value's agreement is bounded by what is derivable -- both integrate the same function
# over the same window, the interpolation error of a C1 cubic with h = 1/64 is far below the Gaussian's own truncated
# area erfc(5 / sqrt 2) = 5.7e-7 --; the derivative rows carry the central-difference slopes' O(h^2) and converge with
# n_tab: measured 2026-10-19 (this file's __main__), asserted at 2 x the measurement.
GAUSS_TAB = (641, 5.0)
GAUSS_VALUE_FLOOR = 5.733031437583869e-07          # erfc(5 / sqrt(2))
GAUSS_ROW_MEASURED = (2.78e-5, 4.93e-6)            # centre, width at n_tab = 641 (161: 3.2e-4, 3.6e-5; 1281: 4.7e-6, 8.2e-7); the value: 9.3e-10

# The reference's derivative rows against long-double central differences of its own value:
#   |row - FD(h / 2)| <= 2 |FD(h) - FD(h / 2)| + FD_EPS max|row|
# FD_EPS: what the comparison leaves on fd_check_bands() under lobed_tables(1), measured 2026-10-19 on this CPU with the
# first term set to zero, x 2: the interpolant is C1 only, a difference that straddles a knot sees the jump of phi^''.
FD_EPS_MEASURED = 9.9e-10       # the centre's row (|row - FD(h / 2)| itself: 1.6e-7 of max|row|); the width's row: no excess at all
FD_EPS = 2.0 * FD_EPS_MEASURED


# ----------------------------------------------------------------------------------------------------------------------
# tables
# ----------------------------------------------------------------------------------------------------------------------
def normalise(t_lo, t_hi, phi):
    """phi [n_shapes, n_tab] divided by the exact integral of each interpolant (long double, rounded once)."""
    p = np.atleast_2d(np.asarray(phi, np.float64)).astype(LD)
    h = (LD(t_hi) - LD(t_lo)) / LD(p.shape[1] - 1)
    area = h * (p.sum(axis=1) - (p[:, 0] + p[:, -1]) / LD(2) + ((p[:, 1] - p[:, 0]) - (p[:, -1] - p[:, -2])) / LD(12))
    assert np.all(area > 0)
    return np.asarray(p / area[:, None], np.float64)


def lobed_tables(n_shapes, n_tab=161):
    """(t_lo, t_hi, phi [n_shapes, n_tab]): asymmetric lobed shapes on +-5 (h = 1/16 with 161 knots),
    sinc(t) (1 + a t / 5) (1 - (t / 5)^2) with a skew a that differs from table to table (0.3, then spread over
    [-0.6, 0.6]): negative side lobes, zeros inside the support, zero at both ends, normalised to unit area."""
    t = np.linspace(-5.0, 5.0, n_tab)
    skew = np.array([0.3] + [0.6 * np.cos(1.0 + 2.4 * q) for q in range(1, n_shapes)])
    phi = np.sinc(t)[None, :] * (1.0 + skew[:, None] * t[None, :] / 5.0) * (1.0 - (t[None, :] / 5.0) ** 2)
    return -5.0, 5.0, normalise(-5.0, 5.0, phi)


def skewed_table(n_tab=65):
    """(t_lo, t_hi, phi [1, n_tab]) on [-5, 3] (h = 1/8 with 65 knots: every knot an exact fp64 value):
    exp(-t^2 / 2) (1 + 0.3 tanh t), cut where it is NOT small -- phi(3) is 1.4e-2 of the peak -- so that the table's ends,
    the clamp and the window's ends show in the numbers.  Normalised."""
    t = np.linspace(-5.0, 3.0, n_tab)
    return -5.0, 3.0, normalise(-5.0, 3.0, np.exp(-0.5 * t * t) * (1.0 + 0.3 * np.tanh(t)))


def gaussian_table(n_tab=641, t_max=5.0):
    t = np.linspace(-t_max, t_max, n_tab)
    return -t_max, t_max, (np.exp(-0.5 * t * t) / np.sqrt(2.0 * np.pi))[None, :]


# ----------------------------------------------------------------------------------------------------------------------
# the reference
# ----------------------------------------------------------------------------------------------------------------------
def _window(x, f, w, t_lo, t_hi):
    """[i0, i1) of f + t_lo w <= x_i <= f + t_hi w on the fp64 values (x ascending)."""
    lo, hi = f + t_lo * w, f + t_hi * w
    sel = np.flatnonzero((x >= lo) & (x <= hi))
    if sel.size == 0:
        return 0, 0, lo, hi
    assert sel[-1] - sel[0] + 1 == sel.size
    return int(sel[0]), int(sel[-1]) + 1, lo, hi


def guard_ils(grid, centers, widths, t_lo, t_hi, g_lo=0, n_sh=None):
    """lowres_reference.guard for the window ends f + t_lo w and f + t_hi w: per band the distance of an end from the
    nearest grid point, in units of the local spacing."""
    _, x = R._shard(grid, g_lo, n_sh)
    out = np.zeros(len(centers))
    for b, (f, w) in enumerate(zip(centers, widths)):
        d = []
        for e in (f + t_lo * w, f + t_hi * w):
            k = int(np.searchsorted(x, e))
            a, c = max(k - 1, 0), min(k, x.size - 1)
            if a == c:
                a, c = (0, 1) if k == 0 else (x.size - 2, x.size - 1)
            d.append(min(abs(e - x[a]), abs(e - x[c])) / (x[c] - x[a]))
        out[b] = min(d)
    return out


def hermite(phi, t_lo, t_hi, t):
    """The interpolant of the fp64 knots phi [n_tab] at the long-double offsets t, in long double: (c [4, n], e [4, n],
    d2 [n], h) with phi^ = sum_j c_j, phi^' = sum_j e_j / h, phi^'' = d2 / h^2."""
    p = np.asarray(phi, np.float64).astype(LD)
    n = p.size
    h = (LD(t_hi) - LD(t_lo)) / LD(n - 1)
    d = np.empty(n, LD)                                   # h m_k
    d[1:-1] = (p[2:] - p[:-2]) / LD(2)
    d[0], d[-1] = p[1] - p[0], p[-1] - p[-2]
    q = (np.asarray(t, LD) - LD(t_lo)) / h
    k = np.clip(np.floor(q).astype(np.int64), 0, n - 2)
    s = q - k.astype(LD)
    r = LD(1) - s
    p0, p1, d0, d1 = p[k], p[k + 1], d[k], d[k + 1]
    c = np.stack([(LD(1) + LD(2) * s) * r * r * p0, s * r * r * d0, s * s * (LD(3) - LD(2) * s) * p1, -s * s * r * d1])
    e = np.stack([-LD(6) * s * r * p0, -(LD(3) * s - LD(1)) * r * d0, LD(6) * s * r * p1, s * (LD(3) * s - LD(2)) * d1])
    d2 = (LD(12) * s - LD(6)) * (p0 - p1) + (LD(6) * s - LD(4)) * d0 + (LD(6) * s - LD(2)) * d1
    return c, e, d2, h


def _tables(phi, n_bands):
    phi = np.atleast_2d(np.asarray(phi, np.float64))
    assert phi.shape[0] in (1, n_bands), "n_shapes is 1 or n_bands"
    return phi


def weights_ils(grid, centers, widths, t_lo, t_hi, phi, g_lo=0, n_sh=None):
    """The three weight tables in long double, in cm-1 index order of the shard: W [3, n_bands, n_sh] (zero outside a
    window and for a window of fewer than two points), the tables of the unit AW [3, n_bands, n_sh] (the docstring's
    factors), count [n_bands]."""
    g, x = R._shard(grid, g_lo, n_sh)
    n = x.size
    centers, widths = np.asarray(centers, np.float64), np.asarray(widths, np.float64)
    phi = _tables(phi, centers.size)
    W, AW = np.zeros((3, centers.size, n), LD), np.zeros((3, centers.size, n), LD)
    count = np.zeros(centers.size, np.int64)
    gl, xl = g.astype(LD), x.astype(LD)
    for b, (f, w) in enumerate(zip(centers, widths)):
        i0, i1, _, _ = _window(x, f, w, t_lo, t_hi)
        count[b] = i1 - i0
        if i1 - i0 < 2:
            continue
        xs, gs = xl[i0:i1], gl[i0:i1]
        wl = LD(w)
        t = (xs - LD(f)) / wl
        cc = np.empty(i1 - i0, LD)
        cc[1:-1] = (xs[2:] - xs[:-2]) / LD(2)
        cc[0] = (xs[1] - xs[0]) / LD(2)
        cc[-1] = (xs[-1] - xs[-2]) / LD(2)
        p = gs * gs * R._ten(-7) * cc
        with np.errstate(under="ignore"):
            c, e, d2, h = hermite(phi[b if phi.shape[0] > 1 else 0], t_lo, t_hi, t)
            f0, f1, f2 = c.sum(axis=0), e.sum(axis=0) / h, d2 / (h * h)
            mc, me, at = np.abs(c).sum(axis=0), np.abs(e).sum(axis=0) / h, np.abs(t)
            rows = (p * f0 / wl, -p * f1 / (wl * wl), -p * (f0 + t * f1) / wl)
            cond = (p / wl * (mc + at * np.abs(f1)), p / (wl * wl) * (me + at * np.abs(f2)),
                    p / wl * (mc + at * me + at * (LD(2) * np.abs(f1) + at * np.abs(f2))))
        for k in range(3):
            W[k, b, n - i1:n - i0] = rows[k][::-1]
            AW[k, b, n - i1:n - i0] = cond[k][::-1]
    return W, AW, count


def band_reference_ils(grid, spec, centers, widths, t_lo, t_hi, phi, units="Wm2", g_lo=0):
    """The value and the two instrument derivatives of the bands of spec [n_spec, n_sh] (a shard: its partial sums) in
    long double.  Returns a dict: value, A [n_spec, 3, n_bands] (rows: ROWS; long double, in `units`; the centre's row per
    nm), count [n_bands], guard [n_bands]."""
    spec = np.atleast_2d(np.asarray(spec, np.float64))
    n_sh = spec.shape[1]
    W, AW, count = weights_ils(grid, centers, widths, t_lo, t_hi, phi, g_lo, n_sh)
    val, A = np.zeros((spec.shape[0], 3, W.shape[1]), LD), np.zeros((spec.shape[0], 3, W.shape[1]), LD)
    with np.errstate(under="ignore"):
        for r in range(spec.shape[0]):
            idx = np.flatnonzero(spec[r])
            s = spec[r, idx].astype(LD)
            val[r] = (W[:, :, idx] * s[None, None, :]).sum(axis=2)
            A[r] = (AW[:, :, idx] * np.abs(s)[None, None, :]).sum(axis=2)
    k = R.unit_factor(units)
    return dict(value=val * k, A=A * k, count=count, guard=guard_ils(grid, centers, widths, t_lo, t_hi, g_lo, n_sh))


def units_of(got, ref):
    """|got - value| / (2^-53 A + 1e-290) of a [n_spec, 3, n_bands] result, as fp64."""
    return R.units_raw(got, ref["value"], ref["A"])


# ----------------------------------------------------------------------------------------------------------------------
# the yardstick, and the restatement that takes seeded defects
# ----------------------------------------------------------------------------------------------------------------------
DEFECTS = ("unclamped_last_knot", "one_sided_slopes_everywhere", "centre_row_sign", "width_row_without_t_dphi",
           "missing_inverse_width", "band_b_gets_table_0", "window_from_n_sigma")


def plain_fp64_ils(grid, spec, centers, widths, t_lo, t_hi, phi, units="Wm2", g_lo=0, defect=None, n_sigma=5.0):
    """The three weight tables and their products with the spectra in plain numpy fp64: [n_spec, 3, n_bands].  defect: one
    of DEFECTS, a seeded fault for the tests of the bound's teeth:
      unclamped_last_knot          the interval index is floor((t - t_lo) / h) as it comes; a point whose index is not an
                                   interval of the table (t = t_hi exactly: index n_tab - 1) counts as outside, 0
      one_sided_slopes_everywhere  m_k = (phi_(k+1) - phi_k) / h at every knot but the last
      centre_row_sign              +p phi^' / w^2
      width_row_without_t_dphi     -p phi^ / w
      missing_inverse_width        the centre's row -p phi^' / w
      band_b_gets_table_0          every band reads the first table
      window_from_n_sigma          the window f -+ n_sigma w of the Gaussian, whatever the table's support"""
    assert defect is None or defect in DEFECTS
    spec = np.atleast_2d(np.asarray(spec, np.float64))
    n = spec.shape[1]
    g, x = R._shard(grid, g_lo, n)
    centers, widths = np.asarray(centers, np.float64), np.asarray(widths, np.float64)
    phi = _tables(phi, centers.size)
    n_tab = phi.shape[1]
    h = (t_hi - t_lo) / (n_tab - 1)
    W = np.zeros((3, centers.size, n))
    for b, (f, w) in enumerate(zip(centers, widths)):
        tab = phi[b if phi.shape[0] > 1 and defect != "band_b_gets_table_0" else 0]
        m = np.empty(n_tab)
        m[1:-1] = (tab[2:] - tab[:-2]) / (2.0 * h)
        m[0], m[-1] = (tab[1] - tab[0]) / h, (tab[-1] - tab[-2]) / h
        if defect == "one_sided_slopes_everywhere":
            m[:-1] = (tab[1:] - tab[:-1]) / h
        lo, hi = (f - n_sigma * w, f + n_sigma * w) if defect == "window_from_n_sigma" else (f + t_lo * w, f + t_hi * w)
        sel = np.flatnonzero((x >= lo) & (x <= hi))
        if sel.size < 2:
            continue
        i0, i1 = int(sel[0]), int(sel[-1]) + 1
        xs, gs = x[i0:i1], g[i0:i1]
        t = (xs - f) / w
        q = (t - t_lo) / h
        kq = np.floor(q).astype(np.int64)
        k = np.clip(kq, 0, n_tab - 2)
        s = q - k
        r = 1.0 - s
        p0, p1, m0, m1 = tab[k], tab[k + 1], m[k], m[k + 1]
        with np.errstate(under="ignore"):
            f0 = (1.0 + 2.0 * s) * r * r * p0 + s * r * r * (h * m0) + s * s * (3.0 - 2.0 * s) * p1 + s * s * (s - 1.0) * (h * m1)
            f1 = 6.0 * s * (s - 1.0) * (p0 - p1) / h + (3.0 * s - 1.0) * (s - 1.0) * m0 + s * (3.0 * s - 2.0) * m1
            if defect == "unclamped_last_knot":
                out = (kq < 0) | (kq > n_tab - 2)
                f0, f1 = np.where(out, 0.0, f0), np.where(out, 0.0, f1)
            c = np.empty(i1 - i0)
            c[1:-1] = (xs[2:] - xs[:-2]) / 2.0
            c[0], c[-1] = (xs[1] - xs[0]) / 2.0, (xs[-1] - xs[-2]) / 2.0
            p = ((gs * gs) * 1.e-7) * c
            row_f = -p * f1 / (w if defect == "missing_inverse_width" else w * w)
            if defect == "centre_row_sign":
                row_f = -row_f
            row_w = -p * f0 / w if defect == "width_row_without_t_dphi" else -p * (f0 + t * f1) / w
            rows = (p * f0 / w, row_f, row_w)
        for kk in range(3):
            W[kk, b, n - i1:n - i0] = rows[kk][::-1]
    with np.errstate(under="ignore"):
        v = np.einsum("rj,kbj->rkb", spec, W)
    v = v * 1.e-3
    if units == "ergscm2":
        v = v * 1.e3
    if units == "nWcm2":
        v = v * 1.e5
    return v


def measure_k_plain_ils(P=None):
    """(max units over the three rows, where) of plain_fp64_ils on a panel (default: K_PLAIN_ILS_PANEL), under the 33
    per-band lobed tables and under the first of them shared by all bands."""
    P = R.panel(*K_PLAIN_ILS_PANEL) if P is None else P
    t_lo, t_hi, phi = lobed_tables(len(P["centers"]))
    k, worst = 0.0, "-"
    for tag, tab in (("per-band tables", phi), ("one shared table", phi[:1])):
        ref = band_reference_ils(P["grid"], P["spec"], P["centers"], P["widths"], t_lo, t_hi, tab)
        u = units_of(plain_fp64_ils(P["grid"], P["spec"], P["centers"], P["widths"], t_lo, t_hi, tab), ref)
        for row in range(3):
            m, where = R.worst(u[:, row], P["spec_names"], P["band_names"])
            if m >= k:
                k, worst = m, "%s | %s | %s" % (tag, ROWS[row], where)
    return k, worst


# ----------------------------------------------------------------------------------------------------------------------
# cases
# ----------------------------------------------------------------------------------------------------------------------
GRID = (2975.0, 5e-4)


def exact_cases(grid, k, t_lo, t_hi, t_knot, w=0.25):
    """Three bands of width w = 2^-2 around the nm grid value x_k of cm-1 point k (as lowres_reference.exact_end_cases):
    f = x_k - t_lo w (the window's LOWER end is bitwise x_k, t = t_lo there), f = x_k - t_hi w (the UPPER end is x_k,
    t = t_hi: the last knot) and f = x_k - t_knot w (t = t_knot, an interior knot).  t_lo w, t_hi w and t_knot w are
    multiples of 2^-5 and x_k lies in [2048, 4096): the sums are exact.  Returns centers, widths, x_k."""
    xk = 1e7 / np.asarray(grid, np.float64)[k]
    assert 2048.0 <= xk - 8.0 and xk + 8.0 < 4096.0
    return np.array([xk - t_lo * w, xk - t_hi * w, xk - t_knot * w]), np.full(3, w), xk


def gaussian_check_bands(grid):
    """Three well-resolved bands inside the grid: windows of +-5 w with >= 500 points each."""
    x = 1e7 / np.asarray(grid, np.float64)[::-1]
    span = x[-1] - x[0]
    centers = x[0] + span * np.array([0.27, 0.5, 0.71])
    widths = span * np.array([0.012, 0.02, 0.027])
    return centers, widths


def fd_check_bands(grid):
    """Bands for the finite-difference check: inside the grid, a few hundred points each, unequal widths."""
    x = 1e7 / np.asarray(grid, np.float64)[::-1]
    span = x[-1] - x[0]
    return x[0] + span * np.array([0.22, 0.41, 0.58, 0.77]), span * np.array([0.008, 0.013, 0.021, 0.017])


def rel_rows(got, ref):
    """max |got - ref| / max |ref| per row of [n_spec, 3, n_bands] arrays: [3]."""
    got, ref = np.asarray(got, LD), np.asarray(ref, LD)
    return np.array([float(np.abs(got[:, k] - ref[:, k]).max() / np.abs(ref[:, k]).max()) for k in range(3)])


def gaussian_agreement(n_tab=GAUSS_TAB[0], n_pts=8193):
    """rel_rows of the tabulated Gaussian's reference against lowres_instr_reference's, on gaussian_check_bands."""
    import lowres_instr_reference as I
    grid, _ = R.make_grid(GRID[0], GRID[1], n_pts)
    rng = np.random.default_rng([20261019, n_pts])
    spec = np.stack([rng.uniform(0.5, 1.5, n_pts), rng.choice([-1.0, 1.0], n_pts) * 10.0 ** rng.uniform(-6.0, 0.0, n_pts),
                     1.0 + 0.5 * np.sin(np.arange(n_pts) / 37.0)])
    centers, widths = gaussian_check_bands(grid)
    t_lo, t_hi, phi = gaussian_table(n_tab, GAUSS_TAB[1])
    tab = band_reference_ils(grid, spec, centers, widths, t_lo, t_hi, phi)
    clo = I.band_reference_instr(grid, spec, centers, widths, n_sigma=GAUSS_TAB[1])
    assert np.array_equal(tab["count"], clo["count"]) and tab["count"].min() >= 500
    return rel_rows(tab["value"], clo["value"])


def fd_check(n_pts=8193):
    """The reference's two derivative rows against long-double central differences of its value in f and ln w, on
    fd_check_bands under the first lobed table.  Returns per row (worst excess of |row - FD(h/2)| over 2 |FD(h) - FD(h/2)|, in
    units of max|row|; worst of |row - FD(h/2)| alone in the same units): the first is what FD_EPS has to cover."""
    grid, _ = R.make_grid(GRID[0], GRID[1], n_pts)
    rng = np.random.default_rng([20261019, n_pts, 7])
    spec = np.stack([rng.uniform(0.5, 1.5, n_pts), 1.0 + 0.5 * np.sin(np.arange(n_pts) / 37.0)])
    cen, wid = fd_check_bands(grid)
    t_lo, t_hi, phi = lobed_tables(1)
    ref = band_reference_ils(grid, spec, cen, wid, t_lo, t_hi, phi)
    assert ref["guard"].min() >= 1e-2 and ref["count"].min() >= 100
    x = 1e7 / grid[::-1]
    move = 0.2 * ref["guard"] * np.diff(x).min()           # what a window end may move, nm: no point enters or leaves
    out = []
    for row in (1, 2):
        if row == 1:
            h = 2.0 ** np.floor(np.log2(np.minimum(wid * 2.0 ** -12, move)))
            at = lambda m, hh: (cen + m * hh, wid)
            coord = lambda c, w: c.astype(LD)
        else:
            h = 2.0 ** np.floor(np.log2(np.minimum(2.0 ** -12, move / (5.0 * wid) / 2.0)))
            at = lambda m, hh: (cen, wid * np.exp(m * hh))
            coord = lambda c, w: np.log(w.astype(LD))
        fd = {}
        for name, hh in (("h", h), ("h/2", h / 2.0)):
            v = {}
            for m in (-1, 1):
                c, w = at(m, hh)
                got = band_reference_ils(grid, spec, c, w, t_lo, t_hi, phi)
                assert np.array_equal(got["count"], ref["count"])
                v[m] = (got["value"][:, 0], coord(c, w))
            fd[name] = (v[1][0] - v[-1][0]) / (v[1][1] - v[-1][1])[None, :]
        scale = np.abs(ref["value"][:, row]).max()
        miss = np.abs(ref["value"][:, row] - fd["h/2"])
        trunc = LD(2) * np.abs(fd["h"] - fd["h/2"])
        out.append((float(np.maximum(miss - trunc, 0).max() / scale), float(miss.max() / scale)))
    return out


if __name__ == "__main__":
    k, where = measure_k_plain_ils()
    print("K_PLAIN_ILS live %.4g at %s" % (k, where))
    for n_tab in (161, 321, 641, 1281):
        print("gaussian table n_tab %5d: value %.3g centre %.3g width %.3g of the row's maximum" % ((n_tab,) + tuple(gaussian_agreement(n_tab))))
    print("finite differences (excess, miss) centre, width:", fd_check())
