"""Extended-precision CPU reference of the single-scattering solar source (sr_solar_source_rows_dev,
engine.solar_source), in numpy.longdouble, with the yardstick of its error and the case set of
tests/test_solar_source_host.py and tests/test_gpu_solar_source.py.  A helper module: no fixture, no pytest setting,
nothing that needs a GPU.

The definition (the build's own; the reference tree has no counterpart), for output row r and grid point j:

    tau[r][j] = sum_{k < n_k} U[r][k] A[k][j]
    T[r][j]   = exp(-tau[r][j])                              exactly 0 where w[r] == 0 or tau >= 700
    emi[r][j] = sca[src_row[r]][j] w[r] sun[j] T[r][j]

The bound per point, with eps = 2^-53 and K_r the row's non-zero columns:

    b_emi   = eps |emi| ((K_r + 2) tau + 8)
    b_trans = eps |T|   ((K_r + 2) tau + 5)

K_r tau is the standard bound of a K_r-term sum of non-negative addends in ANY order (K_r - 1 additions and the
products' roundings), carried through the exponential's condition number tau; two more units of tau cover one more
rounding of tau and fused or unfused products.  The constant covers the exponential (<= 1 ulp = 2 eps) and, for emi, the
three products (3 eps), with slack; trans has no products, hence 5.  A term-by-term fp64 loop (plain64) stays at 0.31 of
b_emi and of b_trans over the 200 random cases of test_solar_source_host.py (n_k 1 .. 640, tau 0.01 .. 200), which asserts
<= 1 and prints the figure.
"""
import numpy as np

LD = np.longdouble
assert np.finfo(LD).eps < 2e-19, "numpy.longdouble is not an extended-precision type here: no reference, no fallback"

EPS53 = 2.0 ** -53
TAU_DARK = 700.0

# the bound panel of the GPU test: tile, chunk and store edges
N_ROWS = (1, 15, 17, 33, 65)
N_K = (1, 3, 5, 13, 160)
N_PTS = (1, 63, 65, 257)


def reference(A, U, w, sca, sun, src_row=None):
    """(emi, trans, tau, K) in long double: emi, trans, tau [n_rows, n_pts], K [n_rows] the rows' non-zero columns.
    A [n_k, n_pts], U [n_rows, n_k], w [n_rows], sca [n_src, n_pts], sun [n_pts]: fp64 inputs taken as exact."""
    A, U = np.asarray(A, LD).reshape(-1, np.shape(A)[-1]), np.asarray(U, LD).reshape(np.shape(U)[0], -1)
    w, sca, sun = np.asarray(w, LD), np.asarray(sca, LD), np.asarray(sun, LD)
    n_rows = U.shape[0]
    src = np.arange(n_rows) if src_row is None else np.asarray(src_row)
    tau = np.zeros((n_rows, A.shape[1]), LD)
    for k in range(U.shape[1]):                       # (term by term: no BLAS in long double)
        tau = tau + U[:, k:k + 1] * A[k][None, :]
    lit = (w != 0)[:, None] & (tau < TAU_DARK)
    trans = np.where(lit, np.exp(-np.where(lit, tau, LD(0))), LD(0))
    emi = sca[src] * w[:, None] * sun[None, :] * trans
    return emi, trans, tau, np.count_nonzero(U, axis=1)


def bound_emi(emi, tau, K):
    return LD(EPS53) * np.abs(emi) * ((np.asarray(K, LD)[:, None] + 2) * tau + 8)


def bound_trans(trans, tau, K):
    return LD(EPS53) * np.abs(trans) * ((np.asarray(K, LD)[:, None] + 2) * tau + 5)


def ratio(got, ref, bound):
    """max |got - ref| / bound as fp64; where the bound is 0 the result must be exactly the reference's (0 / 0 -> 0,
    anything else -> inf).  A NaN or Inf in `got` is an error."""
    got = np.asarray(got)
    assert np.all(np.isfinite(np.asarray(got, np.float64))), "non-finite result"
    err = np.abs(np.asarray(got, LD) - ref)
    with np.errstate(divide="ignore", invalid="ignore"):
        q = np.where(bound > 0, err / np.where(bound > 0, bound, LD(1)), np.where(err == 0, LD(0), LD(np.inf)))
    return float(np.max(q)) if q.size else 0.0


def plain64(A, U, w, sca, sun, src_row=None):
    """The definition term by term in fp64, k ascending: (emi, trans)."""
    A, U = np.asarray(A, np.float64).reshape(-1, np.shape(A)[-1]), np.asarray(U, np.float64).reshape(np.shape(U)[0], -1)
    w, sca, sun = (np.asarray(v, np.float64) for v in (w, sca, sun))
    n_rows = U.shape[0]
    src = np.arange(n_rows) if src_row is None else np.asarray(src_row)
    tau = np.zeros((n_rows, A.shape[1]))
    for k in range(U.shape[1]):
        tau = tau + U[:, k:k + 1] * A[k][None, :]
    lit = (w != 0)[:, None] & (tau < TAU_DARK)
    trans = np.where(lit, np.exp(-np.where(lit, tau, 0.0)), 0.0)
    return sca[src] * ((w[:, None] * sun[None, :]) * trans), trans


def ray_columns(rng, n_rows, n_k, tau_lo=1e-3, tau_hi=300.0, a_max=1.5):
    """U [n_rows, n_k] laid out as a sun ray's columns are: row r has columns from a shell of its own on (about 40 % of
    a row zeros, the rows' own shells in random order over the first 80 % of k), and, one row in four, a few below it
    (mu < 0).  Scaled so that the row's largest optical depth over a table with values up to a_max is log-uniform in
    [tau_lo, tau_hi]."""
    U = np.zeros((n_rows, n_k))
    for r in range(n_rows):
        own = int(rng.integers(0, max(int(0.8 * n_k), 1)))
        U[r, own:] = rng.uniform(0.2, 1.0, n_k - own)
        if r % 4 == 1 and own > 0:
            U[r, max(own - 3, 0):own] = rng.uniform(0.2, 1.0, own - max(own - 3, 0))
        target = np.exp(rng.uniform(np.log(tau_lo), np.log(tau_hi)))
        U[r] *= target / (a_max * U[r].sum())
    return U


def panel_case(n_rows, n_k, n_pts, seed=0):
    """dict(A, U, w, sca, sun, src_row) of one case of the bound panel, fp64: ray_columns, a table with values in
    [0.15, 1.5] (a factor per point times a factor per entry: tau from ~1e-4 of the row's target to the target), a
    scatterer of n_src = max(n_rows // 2, 1) rows, every row lit."""
    rng = np.random.default_rng([20261020, n_rows, n_k, n_pts, seed])
    n_src = max(n_rows // 2, 1)
    A = rng.uniform(0.5, 1.5, (n_k, n_pts)) * np.exp(rng.uniform(np.log(0.3), 0.0, n_pts))[None, :]
    return dict(A=A, U=ray_columns(rng, n_rows, n_k), w=rng.uniform(0.01, 0.1, n_rows), sca=rng.uniform(1e-9, 1e-7, (n_src, n_pts)),
                sun=rng.uniform(5.0, 20.0, n_pts), src_row=rng.integers(0, n_src, n_rows).astype(np.int32))
