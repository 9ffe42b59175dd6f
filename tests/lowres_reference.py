"""Extended-precision CPU reference of the instrument step (SpectralIntensity.hires_to_lowres, spect_classes.py:1180-1191;
the comment above sr_lowres_weights_kernel): cm-1 -> nm, a Gaussian ILS over +-n_sigma widths, the trapezoid rule on the
irregular nm grid, the unit factors

    x_i = 1e7 / g_i,   t_i = (x_i - f) / w,   u_i = g_i^2 1e-7 exp(-t_i^2 / 2) / (w sqrt(2 pi))
    band = sum over the trapezoids between neighbouring selected points (lo <= x_i <= hi, lo, hi = f -+ n_sigma w)
         = sum_i s_i W_i,   W_i = u_i c_i,   c_i = (x_(i+1) - x_(i-1)) / 2 inside the window, the half interval at its ends

written from that definition in numpy.longdouble (x87 extended: 64-bit mantissa), with an error unit that follows the
sum's conditioning, the plain fp64 evaluation (oracle.hires_to_lowres) as the yardstick of the bound, a plain numpy
restatement that takes seeded defects, and a panel of bands and spectra that visits the edges of the kernels' tiling
(4096-point chunks, 64-point slots, tiles of 16 bands).  A helper module: no fixture, no pytest setting.

What is fp64 DATA and what is long double.  The grid array w0 + step arange(n) as numpy forms it, the spectrum, the
centres, the widths and n_sigma are fp64 data.  The nm grid x_i = 1e7 / g_i is taken in fp64 as the reference program
forms it, and the window is selected on those fp64 values with lo, hi = f -+ n_sigma w in fp64: which points belong to a
band is part of the definition, not of the arithmetic.  Everything after that -- t, the Gaussian, g^2 1e-7, the interval
widths, the products, the sum, the unit factors (powers of ten, not their fp64 neighbours) -- is long double.

The unit.  A result's error is measured in UNITS of

    2^-53 A + 1e-290,      A = sum_i |s_i W_i| (1 + t_i^2)

the sum of magnitudes, each term with what a rounding of t costs through the exponential (d exp(-t^2/2) = -t^2 (dt / t)
exp(-t^2/2)).  The interval widths and x - f are differences of neighbouring fp64 values (exact), so they add nothing.
The absolute floor lets results below the smallest normal double count as zero.

The guard.  Whether a grid point that lies within a rounding of lo or hi belongs to the window is decided by the fp64
comparison alone; the panel keeps every window end at least 1e-6 of the local spacing from the nearest grid point
(guard()), so that no honest fp64 evaluation of 1e7 / g and f -+ n_sigma w selects other points.  The two exact-end
cases are built outside that guard, with ends that are bitwise grid values (exact_end_cases()).
"""
import numpy as np

LD = np.longdouble
assert np.finfo(LD).eps < 2e-19, "numpy.longdouble is not an extended-precision type here: no reference, no fallback"

EPS53 = 2.0 ** -53
FLOOR = 1e-290
CHUNK = 4096     # points per block of sr_lowres_apply_kernel (kLowresChunk)
SLOT = 64        # points per partial sum of the recursion kernels' band epilogue (a wave)
TILE = 16        # bands per block of the apply kernel and per MFMA tile of the epilogue
GUARD_MIN = 1e-6
UNITS = ("Wm2", "ergscm2", "nWcm2")

# K_PLAIN: max units(oracle.hires_to_lowres, reference) over the (spectrum, band) pairs of a panel -- the distance of an
# honest fp64 implementation (libm exp, IEEE division, the trapezoids summed one after the other in grid order) from the
# reference, in the bound's own units.  A kernel's limit is KERNEL_MARGIN x max(K_PLAIN, 1), K_PLAIN taken over each
# test's own pairs (never from a kernel); the floor of 1 is one half-ulp of the sum of magnitudes: any fp64 result may
# be that far off.  Measured 2026-10-18 on panel(2975.0, 5e-4, 8193, 33, 20261018), n_sigma 5, 'Wm2' (33 bands, 2 dense
# + 305 one-hot spectra): 15.2 units, on a random band that covers the whole grid under the positive-noise spectrum
# (8193 trapezoids summed in sequence); the signed spectrum measures 2.3, one-hot spectra (a single weight) <= 4.0.  The recorded constant is 1.5 x the measurement and may be at
# most 2 x what was measured when it was written; tests/test_lowres_reference_host.py asserts that the live measurement
# does not exceed it.
K_PLAIN_MEASURED = 15.2
K_PLAIN = 23.0
K_PLAIN_PANEL = (2975.0, 5e-4, 8193, 33, 20261018)
KERNEL_MARGIN = 8.0   # a GPU exp of <= 1 ulp, sums strided over 256 threads and shuffled across a wave, the partial sums
                      # of chunks and of 64-point slots added in another order


def _ten(k):
    return LD(10) ** k if k >= 0 else LD(1) / LD(10) ** (-k)


_UNIT_POW = {"Wm2": -3, "ergscm2": 0, "nWcm2": 2}      # 'ergscm2' -> 'Wm2' 1e-3; back 1e3; -> 'nWcm2' 1e-3 x 1e5


def unit_factor(units):
    return _ten(_UNIT_POW[units])


def make_grid(w0, step, n):
    """w0 + step arange(n) as numpy forms it, step snapped to (w0 + step) - w0 so that grid[1] - grid[0] == step (what
    np.arange(w0, w1, step) does, and what engine.grid_params reads back).  Returns (grid, step)."""
    step = float((w0 + step) - w0)
    grid = w0 + step * np.arange(n)
    assert grid[1] - grid[0] == step
    return grid, step


def _shard(grid, g_lo, n_sh):
    grid = np.asarray(grid, np.float64)
    n_sh = grid.size - g_lo if n_sh is None else n_sh
    assert 0 <= g_lo and n_sh >= 1 and g_lo + n_sh <= grid.size
    g = grid[g_lo:g_lo + n_sh][::-1].copy()            # nm index i <-> cm-1 index n - 1 - i
    return g, 1e7 / g                                   # fp64, as the reference program forms it


def _window(x, f, w, n_sigma):
    """[i0, i1) of lo <= x_i <= hi on the fp64 values (x ascending)."""
    lo, hi = f - n_sigma * w, f + n_sigma * w
    sel = np.flatnonzero((x >= lo) & (x <= hi))
    if sel.size == 0:
        return 0, 0, lo, hi
    assert sel[-1] - sel[0] + 1 == sel.size
    return int(sel[0]), int(sel[-1]) + 1, lo, hi


def guard(grid, centers, widths, n_sigma=5.0, g_lo=0, n_sh=None):
    """Per band: the distance of lo and of hi from the nearest grid point, in units of the local spacing (the smaller of
    the two).  A band wholly outside the grid measures its distance from the grid's end."""
    _, x = _shard(grid, g_lo, n_sh)
    out = np.zeros(len(centers))
    for b, (f, w) in enumerate(zip(centers, widths)):
        d = []
        for e in (f - n_sigma * w, f + n_sigma * w):
            k = int(np.searchsorted(x, e))
            a, c = max(k - 1, 0), min(k, x.size - 1)             # the neighbours on either side (one at the grid's ends)
            if a == c:
                a, c = (0, 1) if k == 0 else (x.size - 2, x.size - 1)
            d.append(min(abs(e - x[a]), abs(e - x[c])) / (x[c] - x[a]))
        out[b] = min(d)
    return out


def weights(grid, centers, widths, n_sigma=5.0, g_lo=0, n_sh=None):
    """The reference's weight table in long double, in cm-1 index order of the shard: W [n_bands, n_sh] (zero outside a
    window, and everywhere for a window of fewer than two points), T = 1 + t^2 [n_bands, n_sh], count [n_bands] (selected
    points)."""
    g, x = _shard(grid, g_lo, n_sh)
    n = x.size
    centers, widths = np.asarray(centers, np.float64), np.asarray(widths, np.float64)
    W, T = np.zeros((centers.size, n), LD), np.ones((centers.size, n), LD)
    count = np.zeros(centers.size, np.int64)
    gl, xl = g.astype(LD), x.astype(LD)
    root_2pi = np.sqrt(LD(2) * np.arctan(LD(1)) * LD(4))
    for b, (f, w) in enumerate(zip(centers, widths)):
        i0, i1, _, _ = _window(x, f, w, n_sigma)
        count[b] = i1 - i0
        if i1 - i0 < 2:
            continue
        xs, gs = xl[i0:i1], gl[i0:i1]
        t = (xs - LD(f)) / LD(w)
        with np.errstate(under="ignore"):
            u = gs * gs * _ten(-7) * (np.exp(-t * t / LD(2)) / (LD(w) * root_2pi))
        c = np.empty(i1 - i0, LD)
        c[1:-1] = (xs[2:] - xs[:-2]) / LD(2)
        c[0] = (xs[1] - xs[0]) / LD(2)
        c[-1] = (xs[-1] - xs[-2]) / LD(2)
        W[b, n - i1:n - i0] = (u * c)[::-1]
        T[b, n - i1:n - i0] = (LD(1) + t * t)[::-1]
    return W, T, count


def band_reference(grid, spec, centers, widths, n_sigma=5.0, units="Wm2", g_lo=0):
    """The band values of spec [n_spec, n_sh] (the grid points g_lo .. g_lo + n_sh - 1: a shard's PARTIAL integrals, the
    trapezoids between the shard's own points; the whole grid by default) in long double.  Returns a dict: value, A
    [n_spec, n_bands] (long double, in `units`), count [n_bands], guard [n_bands]."""
    spec = np.atleast_2d(np.asarray(spec, np.float64))
    n_sh = spec.shape[1]
    W, T, count = weights(grid, centers, widths, n_sigma, g_lo, n_sh)
    WT = np.abs(W) * T
    val, A = np.zeros((spec.shape[0], W.shape[0]), LD), np.zeros((spec.shape[0], W.shape[0]), LD)
    with np.errstate(under="ignore"):
        for r in range(spec.shape[0]):
            idx = np.flatnonzero(spec[r])             # (one-hot probes: one column of the table)
            s = spec[r, idx].astype(LD)
            val[r] = (W[:, idx] * s[None, :]).sum(axis=1)
            A[r] = (WT[:, idx] * np.abs(s)[None, :]).sum(axis=1)
    k = unit_factor(units)
    return dict(value=val * k, A=A * k, count=count, guard=guard(grid, centers, widths, n_sigma, g_lo, n_sh))


def units_of(got, ref):
    """|got - value| / (2^-53 A + 1e-290), as fp64; a NaN or Inf in `got` is an error."""
    return units_raw(got, ref["value"], ref["A"])


def units_raw(got, value, A):
    got = np.asarray(got)
    if not np.all(np.isfinite(got)):
        bad = np.argwhere(~np.isfinite(got))
        raise AssertionError("non-finite result at %d places, first at index %s" % (len(bad), tuple(bad[0])))
    with np.errstate(under="ignore"):
        u = np.abs(np.asarray(got, LD) - np.asarray(value, LD)) / (LD(EPS53) * np.asarray(A, LD) + LD(FLOOR))
    return np.asarray(u, np.float64)


def limit(k_plain):
    return KERNEL_MARGIN * max(float(k_plain), 1.0)


def worst(u, spec_names=None, band_names=None):
    """(max units, where) of a [n_spec, n_bands] units array."""
    u = np.asarray(u)
    if u.size == 0:
        return 0.0, "-"
    r, b = np.unravel_index(int(np.argmax(u)), u.shape)
    return float(u[r, b]), "%s | %s" % (spec_names[r] if spec_names is not None else "spectrum %d" % r,
                                       band_names[b] if band_names is not None else "band %d" % b)


# ------------------------------------------------------------------------------------------------------------------
# the yardstick: the plain fp64 evaluation, and a restatement that takes seeded defects
# ------------------------------------------------------------------------------------------------------------------
def oracle_plain(grid, spec, centers, widths, n_sigma=5.0, units="Wm2", g_lo=0):
    """oracle.hires_to_lowres, spectrum by spectrum; a shard: on the grid slice [g_lo : g_lo + n] with the same spectrum
    slice.  The yardstick of the tolerance (K_PLAIN), not a test subject."""
    from oracle import oracle as O
    spec = np.atleast_2d(np.asarray(spec, np.float64))
    g = np.ascontiguousarray(np.asarray(grid, np.float64)[g_lo:g_lo + spec.shape[1]])
    return np.array([O.hires_to_lowres(g, s, centers, widths, units, n_sigma) for s in spec])


DEFECTS = ("full_end_interval", "open_window", "shifted_spectrum", "chunk_last_dropped", "band16_gets_band0")


def plain_fp64(grid, spec, centers, widths, n_sigma=5.0, units="Wm2", g_lo=0, defect=None):
    """The weight-table form of the instrument step in plain numpy fp64, as the kernels organise it: a table W in cm-1
    index order, a product with the spectra, the unit factors.  defect: one of DEFECTS, a seeded fault for the tests of
    the bound's teeth (not a test subject)."""
    assert defect is None or defect in DEFECTS
    spec = np.atleast_2d(np.asarray(spec, np.float64))
    n = spec.shape[1]
    g, x = _shard(grid, g_lo, n)
    centers, widths = np.asarray(centers, np.float64), np.asarray(widths, np.float64)
    W = np.zeros((centers.size, n))
    for b, (f, w) in enumerate(zip(centers, widths)):
        lo, hi = f - n_sigma * w, f + n_sigma * w
        sel = np.flatnonzero(((x > lo) & (x < hi)) if defect == "open_window" else ((x >= lo) & (x <= hi)))
        if sel.size < 2:
            continue
        i0, i1 = int(sel[0]), int(sel[-1]) + 1
        xs, gs = x[i0:i1], g[i0:i1]
        t = (xs - f) / w
        with np.errstate(under="ignore"):
            u = ((gs * gs) * 1.e-7) * ((1 / (w * np.sqrt(2. * np.pi))) * np.exp(-0.5 * (t * t)))
        c = np.empty(i1 - i0)
        c[1:-1] = (xs[2:] - xs[:-2]) / 2.0
        half = 1.0 if defect == "full_end_interval" else 2.0
        c[0], c[-1] = (xs[1] - xs[0]) / half, (xs[-1] - xs[-2]) / half
        W[b, n - i1:n - i0] = (u * c)[::-1]
    if defect == "band16_gets_band0" and centers.size > TILE:
        W[TILE] = W[0]
    if defect == "shifted_spectrum":
        spec = np.concatenate([spec[:, 1:], np.zeros((spec.shape[0], 1))], axis=1)
    if defect == "chunk_last_dropped":
        spec = spec.copy()
        spec[:, CHUNK - 1::CHUNK] = 0.0
    v = spec @ W.T
    v = v * 1.e-3
    if units == "ergscm2":
        v = v * 1.e3
    if units == "nWcm2":
        v = v * 1.e5
    return v


# ------------------------------------------------------------------------------------------------------------------
# the field of view
# ------------------------------------------------------------------------------------------------------------------
def fov_reference(value, A, factors):
    """smm.fov_closed_form's expression in long double on the reference band values of the rays [3 n_pix, ...] (pixel p:
    rays 3p, 3p + 1, 3p + 2), with the fp64 geometry factors of engine.fov_factors [n_pix, 7] (delta, delta^3, 2 dmax^2,
    edge, m2, esse, has_edge: input data of the call).  The unit's A: the same expression over the rays' A (>= |value|:
    it carries what the band values themselves may be off, and every rounding of the expression), with
    A0 + A2 + 2 A1 for the second difference c.  Returns (value, A) [n_pix, ...]."""
    value, A = np.asarray(value, LD), np.asarray(A, LD)
    fac = np.asarray(factors, np.float64)
    shape = (-1,) + (1,) * (value.ndim - 1)
    delta, delta3, two_dmax2, edge, m2, esse, has = (fac[:, k].astype(LD).reshape(shape) for k in range(7))
    has = has != 0
    safe_edge = np.where(has, edge, LD(1))

    def expr(s1, c):
        total = LD(2) * (s1 * delta + c * delta3 / LD(3))
        return esse * np.where(has, total + s1 * edge + LD(2) * c * m2 / safe_edge, total)

    s0, s1, s2 = value[0::3], value[1::3], value[2::3]
    a0, a1, a2 = A[0::3], A[1::3], A[2::3]
    return expr(s1, (s0 + s2 - LD(2) * s1) / two_dmax2), expr(a1, (a0 + a2 + LD(2) * a1) / two_dmax2)


# ------------------------------------------------------------------------------------------------------------------
# the panel
# ------------------------------------------------------------------------------------------------------------------
def _band_over(x, i0, i1, n_sigma, below=0.5, above=0.5):
    """(f, w) of a band whose window selects exactly the nm points i0 .. i1 - 1: lo `below` spacings under x[i0], hi
    `above` spacings over x[i1 - 1] (0.5: the middle of the gap to the neighbour outside)."""
    n = x.size
    sp = lambda i: (x[min(i + 1, n - 1)] - x[min(i + 1, n - 1) - 1]) if n > 1 else 1e-3
    lo = x[i0] - below * sp(max(i0 - 1, 0))
    hi = x[i1 - 1] + above * sp(i1 - 1)
    return 0.5 * (lo + hi), (hi - lo) / (2.0 * n_sigma)


def panel(w0, step, n, n_bands, seed, n_sigma=5.0):
    """Bands and spectra of one grid.  Bands (in a seeded shuffle: unsorted): one wholly below and one wholly above the
    grid; one over the whole grid; narrow ones clipped by the first and by the last grid point; two overlapping and a
    duplicate of the first of them; windows of exactly 1, 2 and 3 points; a window wholly inside one chunk; windows that
    straddle each chunk boundary by one point on either side; windows whose range begins on a multiple of 64 and ends on
    63 mod 64; random bands (each redrawn until its guard is >= 1e-2) up to n_bands.  What the grid has no room for is
    left out; fewer than the structured bands asked for: the first n_bands of the shuffle.
    Spectra [n_spec, n]: positive noise; signed with six decades of dynamic range; one-hot spectra (a single 1.0) at each
    window's first, second and last point, at points 0 and n - 1 and on both sides of every chunk and slot boundary.
    Returns a dict: grid, step, centers, widths, band_names, n_structured, spec, spec_names, n_sigma."""
    rng = np.random.default_rng([seed, n])
    grid, step = make_grid(w0, step, n)
    x = 1e7 / grid[::-1]
    span = x[-1] - x[0]
    J = lambda ja, jb: (n - jb, n - ja)            # cm-1 index range [ja, jb) -> nm index range
    bands = [("below the grid", (x[0] - 50 * span - 1.0, 0.05 * span * 5.0 / n_sigma)),
             ("above the grid", (x[-1] + 50 * span + 1.0, 0.05 * span * 5.0 / n_sigma)),
             ("whole grid", _band_over(x, 0, n, n_sigma, 3.5, 3.5))]
    k = max(2, n // 50 + 2)
    if k <= n:
        bands.append(("clipped by the first point", _band_over(x, 0, k, n_sigma, 3.5, 0.5)))
        bands.append(("clipped by the last point", _band_over(x, n - k, n, n_sigma, 0.5, 3.5)))
    if n >= 8:
        a = _band_over(x, int(0.3 * n), int(0.6 * n), n_sigma)
        bands += [("overlap a", a), ("overlap b", _band_over(x, int(0.45 * n), int(0.75 * n), n_sigma)), ("duplicate of overlap a", a)]
    for m in (1, 2, 3):
        if n // 3 + m <= n:
            bands.append(("%d-point window" % m, _band_over(x, n // 3, n // 3 + m, n_sigma)))
    if n > CHUNK + 30:
        bands.append(("inside chunk 1", _band_over(x, *J(CHUNK + 10, min(n, 2 * CHUNK) - 10), n_sigma)))
    elif n > 30:
        bands.append(("inside chunk 0", _band_over(x, *J(10, n - 10), n_sigma)))
    for B in range(CHUNK, n, CHUNK):
        bands.append(("chunk %d: one point below" % B, _band_over(x, *J(B - 1, min(B + 40, n)), n_sigma)))
        bands.append(("chunk %d: one point above" % B, _band_over(x, *J(B - 40, B + 1), n_sigma)))
    for ja, jb in ((SLOT, 2 * SLOT), (SLOT, 4 * SLOT), (0, SLOT)):
        if jb < n:
            bands.append(("range [%d, %d)" % (ja, jb), _band_over(x, *J(ja, jb), n_sigma)))
    order = rng.permutation(len(bands))
    bands = [bands[q] for q in order]
    n_structured = len(bands)
    bands = bands[:n_bands]
    while len(bands) < n_bands:
        f = x[0] + span * rng.uniform(0.02, 0.98)
        w = span * rng.uniform(0.015, 1.0) / n_sigma
        if guard(grid, [f], [w], n_sigma)[0] >= 1e-2:
            bands.append(("random %d" % len(bands), (f, w)))
    centers = np.array([b[1][0] for b in bands])
    widths = np.array([b[1][1] for b in bands])
    # the probes
    hot = {0, n - 1}
    for f, w in zip(centers, widths):
        i0, i1, _, _ = _window(x, f, w, n_sigma)
        for i in (i0, i0 + 1, i1 - 1):
            if i0 <= i < i1:
                hot.add(n - 1 - i)
    for B in range(SLOT, n, SLOT):
        hot.update((B - 1, B))
    hot = sorted(hot)
    spec = np.zeros((2 + len(hot), n))
    spec[0] = rng.uniform(0.5, 1.5, n)
    spec[1] = rng.choice([-1.0, 1.0], n) * 10.0 ** rng.uniform(-6.0, 0.0, n)
    spec[2 + np.arange(len(hot)), hot] = 1.0
    names = ["positive noise", "signed, six decades"] + ["one-hot at %d" % j for j in hot]
    return dict(grid=grid, step=step, centers=centers, widths=widths, band_names=[b[0] for b in bands],
                n_structured=n_structured, spec=spec, spec_names=names, n_sigma=n_sigma, hot=np.array(hot))


def exact_end_cases(grid, k):
    """The two bands whose window END is bitwise the nm grid value x_k of cm-1 point k: w = 2^-2, n_sigma = 5,
    f = x_k + 1.25 (lo == x_k) and f = x_k - 1.25 (hi == x_k).  The end point belongs to the window (>=, <=).  Returns
    centers, widths, x_k; the caller asserts the bitwise identities and the guard of the two far ends."""
    xk = 1e7 / np.asarray(grid, np.float64)[k]
    return np.array([xk + 1.25, xk - 1.25]), np.array([0.25, 0.25]), xk
