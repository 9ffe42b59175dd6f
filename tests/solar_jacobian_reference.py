"""Extended-precision CPU reference of the solar attenuation in the Jacobians (sr_solar_jacobian_rows_dev,
engine.solar_attenuation_jacobian), in numpy.longdouble, with the yardstick of its error and the case set of
tests/test_solar_jacobian_host.py and tests/test_gpu_solar_jacobian.py.  A helper module: no fixture, no pytest setting,
nothing that needs a GPU.

The definition (the build's own; the reference tree has no counterpart), for parameter p, ray y and grid point j:

    dtau[p][r][j] = sum_{k < n_k} dU[p][r][k] A[k][j]
    jac[y][p][j]  = - sum_{r < n_rows} Q[y][r][j] dtau[p][r][j]

The bound per element, with eps = 2^-53, K_pr the non-zero columns of row r of parameter p and R_p the parameter's rows
with any:

    b = eps sum_r |Q_r| (K_pr + R_p + 2) sum_k |dU[p][r][k]| |A[k]|          (+ eps |base - sum| under accumulate)

K_pr covers a K_pr-term sum in ANY order (K_pr - 1 additions and the products' roundings, fused or not), R_p an R_p-term
sum of the rows in any order (the rows without columns add exact zeros), 2 the rounding of Q dtau and one more of the
partial sums' regrouping.  Mixed signs: the bound is on the sum of magnitudes, not on the result.  Where b = 0 the
result must be exactly 0.  A term-by-term fp64 loop (plain64) stays below b on the 200 random cases of
test_solar_jacobian_host.py (n_k 1 .. 160, about half zeros, both signs), which asserts <= 1 and prints the figure.
"""
import numpy as np

LD = np.longdouble
assert np.finfo(LD).eps < 2e-19, "numpy.longdouble is not an extended-precision type here: no reference, no fallback"

EPS53 = 2.0 ** -53
NR = 8                      # rays per block of the kernel (engine.SOLAR_JAC_RAYS): the ray-group edge

# the bound panel of the GPU test: tile, chunk, store and ray-group edges
N_ROWS = (1, 15, 17, 33)
N_K = (1, 3, 5, 13, 160)
N_PTS = (1, 63, 65, 257)
RAYS_PARS = ((1, 1), (3, 2), (NR + 1, 5), (9, 17))


def reference(A, dU, Q):
    """(jac [n_rays, n_par, n_pts], b the same shape) in long double.  A [n_k, n_pts], dU [n_par, n_rows, n_k], Q [n_rays,
    n_rows, n_pts]: fp64 inputs taken as exact."""
    A = np.asarray(A, LD).reshape(-1, np.shape(A)[-1])
    dU = np.asarray(dU, LD).reshape(np.shape(dU)[0], np.shape(dU)[1], -1)
    Q = np.asarray(Q, LD)
    n_par, n_rows, n_k = dU.shape
    dtau, mag = np.zeros((n_par, n_rows, A.shape[1]), LD), np.zeros((n_par, n_rows, A.shape[1]), LD)
    for k in range(n_k):                              # (term by term: no BLAS in long double)
        if np.any(dU[:, :, k] != 0):
            dtau = dtau + dU[:, :, k:k + 1] * A[k][None, None, :]
            mag = mag + np.abs(dU[:, :, k:k + 1]) * np.abs(A[k])[None, None, :]
    K = np.count_nonzero(dU, axis=2).astype(LD)       # [n_par, n_rows]
    Rp = np.count_nonzero(K, axis=1).astype(LD)       # [n_par]
    weight = (K + Rp[:, None] + 2)[:, :, None] * mag
    jac, b = np.zeros((Q.shape[0], n_par, A.shape[1]), LD), np.zeros((Q.shape[0], n_par, A.shape[1]), LD)
    for r in range(n_rows):
        jac = jac - Q[:, None, r, :] * dtau[None, :, r, :]
        b = b + np.abs(Q[:, None, r, :]) * weight[None, :, r, :]
    return jac, LD(EPS53) * b


def bound_accumulated(b, total):
    """The bound of base - sum: b and the rounding of the last subtraction (total = base - sum, long double)."""
    return b + LD(EPS53) * np.abs(total)


def ratio(got, ref, bound):
    """max |got - ref| / bound as fp64; where the bound is 0 the result must be exactly the reference's (0 / 0 -> 0,
    anything else -> inf).  A NaN or Inf in `got` is an error."""
    got = np.asarray(got)
    assert np.all(np.isfinite(np.asarray(got, np.float64))), "non-finite result"
    err = np.abs(np.asarray(got, LD) - ref)
    with np.errstate(divide="ignore", invalid="ignore"):
        q = np.where(bound > 0, err / np.where(bound > 0, bound, LD(1)), np.where(err == 0, LD(0), LD(np.inf)))
    return float(np.max(q)) if q.size else 0.0


def plain64(A, dU, Q):
    """The definition term by term in fp64, k ascending, then r ascending: jac [n_rays, n_par, n_pts]."""
    A = np.asarray(A, np.float64).reshape(-1, np.shape(A)[-1])
    dU = np.asarray(dU, np.float64).reshape(np.shape(dU)[0], np.shape(dU)[1], -1)
    Q = np.asarray(Q, np.float64)
    n_par, n_rows, n_k = dU.shape
    dtau = np.zeros((n_par, n_rows, A.shape[1]))
    for k in range(n_k):
        dtau = dtau + dU[:, :, k:k + 1] * A[k][None, None, :]
    s = np.zeros((Q.shape[0], n_par, A.shape[1]))
    for r in range(n_rows):
        s = s + Q[:, None, r, :] * dtau[None, :, r, :]
    return -s


def mask_columns(rng, n_par, n_rows, n_k, empty=None):
    """dU [n_par, n_rows, n_k] laid out as geometry.solar_column_weights lays it: a parameter's mask touches a few
    neighbouring layers of ONE gas block of k (two blocks when n_k >= 8), the rows below the mask cross them and, one row
    in four, rows above it too (mu < 0); about half of those entries are zero, the others of either sign over three
    decades.  Parameter `empty` has no columns at all."""
    dU = np.zeros((n_par, n_rows, n_k))
    n_gas = 2 if n_k >= 8 else 1
    n_lay = n_k // n_gas
    for p in range(n_par):
        if p == empty:
            continue
        g = int(rng.integers(0, n_gas))
        l0 = int(rng.integers(0, n_lay))
        l1 = min(l0 + int(rng.integers(1, 5)), n_lay)
        top = int(rng.integers(1, n_rows + 1))
        rows = np.arange(n_rows)
        crossing = (rows < top) | ((rows % 4 == 1) & (rng.random(n_rows) < 0.5))
        block = rng.choice([-1.0, 1.0], (n_rows, l1 - l0)) * np.exp(rng.uniform(np.log(1e-3), 0.0, (n_rows, l1 - l0)))
        block *= (rng.random((n_rows, l1 - l0)) < 0.5) * crossing[:, None]
        dU[p, :, g * n_lay + l0:g * n_lay + l1] = block
    return dU


def panel_case(n_rows, n_k, n_pts, n_rays, n_par, seed=0):
    """dict(A, dU, Q) of one case of the bound panel, fp64: mask_columns (the second parameter, if there is one, without
    columns), solar_source_reference's table, Q of both signs over two decades with the second ray (if any) all zero."""
    rng = np.random.default_rng([20261020, 411, n_rows, n_k, n_pts, n_rays, n_par, seed])
    A = rng.uniform(0.5, 1.5, (n_k, n_pts)) * np.exp(rng.uniform(np.log(0.3), 0.0, n_pts))[None, :]
    Q = rng.choice([-1.0, 1.0], (n_rays, n_rows, n_pts)) * np.exp(rng.uniform(np.log(1e-9), np.log(1e-7), (n_rays, n_rows, n_pts)))
    if n_rays > 1:
        Q[1] = 0.0
    return dict(A=A, dU=mask_columns(rng, n_par, n_rows, n_k, empty=1 if n_par > 1 else None), Q=Q)


def panel():
    """The panel's cases: every (n_rows, n_k, n_pts) with (n_rays, n_par) cycling so that every n_pts and every n_k meets
    every shape."""
    out, n = [], 0
    for n_rows in N_ROWS:
        for n_k in N_K:
            for n_pts in N_PTS:
                out.append((n_rows, n_k, n_pts) + RAYS_PARS[(n + n // 4) % 4])
                n += 1
    return out
