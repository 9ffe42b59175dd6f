"""Inputs and references of the row-parameter tests (tests/test_state_rows_host.py, tests/test_gpu_state_rows.py): the
synthetic LOS batch at the smallest shapes at which sr_limb_jac_state_kernel's indexing can go wrong, the regime panel of
tests/limb_reference.py laid on its coefficient rows, derivative spectra, row weights and the extended-precision
reference of every ray.  A helper module: no fixture, no pytest setting, nothing that needs a GPU.

The shapes are those of _synthetic in tests/test_gpu_state_jacobian.py: 300 points (two point blocks, the last wave
straddles the end), 6 coefficient rows, 3 rays of 1, 4 and 7 segments of two sample points each.
"""
import numpy as np

import limb_reference as R

SEED = 20261018
N_PTS, N_LAYERS = 300, 6
SEG_OFF = np.array([0, 1, 5, 12], np.int32)
SEG_LAYER = np.array([3, 5, 4, 3, 4, 0, 1, 2, 5, 2, 1, 0], np.int32)
N_SEG = SEG_LAYER.size
PT_OFF = 2 * np.arange(N_SEG + 1, dtype=np.int32)


def geometry(seed):
    """x, nd [2 n_seg]: two sample points per segment, the number density falling along it (a Curtis-Godson column needs
    nd to vary)."""
    rng = np.random.default_rng([SEED, seed])
    x = (np.arange(N_SEG)[:, None] + np.array([0.0, 1.0]) * rng.uniform(0.5, 1.0, (N_SEG, 1))).reshape(-1)
    nd = (rng.uniform(0.5, 2.0, (N_SEG, 1)) * np.array([1.0, 0.8])).reshape(-1)
    return x, nd


def cg_columns(nd, x, vmr):
    """curgod_fort_2 (curgods.f:24-45) of every two-point segment in numpy fp64: [n_gas, n_seg].  What the device
    integrates, to rounding: the host tests' stand-in for LimbLOS.columns()."""
    nd, x, vmr = np.asarray(nd, float).reshape(-1, 2), np.asarray(x, float).reshape(-1, 2), np.atleast_2d(vmr)
    vmr = vmr.reshape(vmr.shape[0], -1, 2)
    dx = x[:, 1] - x[:, 0]
    A = nd[:, 0] * vmr[:, :, 0]
    B = nd[:, 0] * (vmr[:, :, 1] - vmr[:, :, 0]) / dx
    fu = nd[:, 1] / nd[:, 0]
    D = np.log(fu) / dx
    return (A * D * (fu - 1.0) + B * fu * (D * dx - 1.0) + B) / (D * D)


def panel_case(n_gas, n_row, every_ray_seen=True):
    """The regime panel on the six coefficient rows (limb_reference.panel_problem: coef_a, coef_e [G, 6, N], the columns
    col [G, 6] at which a row meets the panel's optical depth), the VMRs that give a segment on row r those columns (to
    rounding: constant along the segment, col / the column of nd alone), derivative spectra and row weights.
    dabs_g = coef_a_g m w_g with ONE factor m in (-1, 1) per (row, point) for all gases (_layer_case of
    tests/test_gpu_limb_reference.py draws tau x uniform(-1, 1)) and w_g in (0.5, 1): either sign occurs, and
    sum_g u_g dabs_g does not cancel between the gases -- a yardstick inflated by such a cancellation would mean nothing.
    demi likewise with its own m.  par_t [n_row, 6]: uniform in (-1, 1), three in ten zero, parameter 1 all zero;
    every_ray_seen: parameter 0 weights row 3 (the single-segment ray's); otherwise no parameter does and that ray meets
    no weighted row."""
    pan = R.panel_problem(N_LAYERS, n_gas, 0, SEED + n_gas)
    rng = np.random.default_rng([SEED, n_gas, n_row])
    x, nd = geometry(n_gas)
    u0 = cg_columns(nd, x, np.ones((1, 2 * N_SEG)))[0]
    vmr = np.repeat(pan["col"][:, SEG_LAYER] / u0[None, :], 2, axis=1)
    shape = pan["coef_a"].shape
    m_a, m_e = rng.uniform(-1.0, 1.0, shape[1:]), rng.uniform(-1.0, 1.0, shape[1:])
    dabs = pan["coef_a"] * m_a[None] * rng.uniform(0.5, 1.0, shape)
    demi = pan["coef_e"] * m_e[None] * rng.uniform(0.5, 1.0, shape)
    par_t = rng.uniform(-1.0, 1.0, (n_row, N_LAYERS)) * (rng.random((n_row, N_LAYERS)) > 0.3)
    if n_row > 1:
        par_t[1] = 0.0
    par_t[:, 3] = 0.0
    if every_ray_seen:
        par_t[0, 3] = 0.7
    return dict(names=pan["names"], coef_a=pan["coef_a"], coef_e=pan["coef_e"], dabs=dabs, demi=demi, par_t=par_t, x=x, nd=nd,
                vmr=vmr, n_gas=n_gas)


def ray_forms(c, col, ray, dtype):
    """tau, E [S, N] and dtau, dE [n_row, S, N] of one ray in `dtype`, the Definition's products: dtau_p =
    par_t[p][r] sum_g u_g dabs_g[r].  col [n_gas, n_seg]: the columns, fp64 inputs."""
    segs = np.arange(SEG_OFF[ray], SEG_OFF[ray + 1])
    lay = SEG_LAYER[segs]
    u = col[:, segs]
    tau, E = R.products(c["coef_a"][:, lay], u, dtype), R.products(c["coef_e"][:, lay], u, dtype)
    da, de = R.products(c["dabs"][:, lay], u, dtype), R.products(c["demi"][:, lay], u, dtype)
    w = np.asarray(c["par_t"][:, lay], dtype)[:, :, None]
    return tau, E, w * da[None], w * de[None]


def references(c, col, I0, solo=False):
    """Per ray: (the reference dict of limb_reference.recursion_reference, the plain-fp64 results (I, J))."""
    out = []
    for ray in range(len(SEG_OFF) - 1):
        ref = R.recursion_reference(*ray_forms(c, col, ray, R.LD), I0, solo=solo, thin_ulps=c["n_gas"] + 1)
        out.append((ref, R.plain_fp64(*ray_forms(c, col, ray, np.float64), I0, solo=solo)))
    return out


def k_plain(refs, n_gas, cols=None):
    """(K_PLAIN of the radiances, of the Jacobians): plain fp64 against the reference on these inputs, in the bound's
    units, over the panel columns `cols` (None: all)."""
    k_rad = k_jac = 0.0
    for ref, (I, J) in refs:
        s = slice(None) if cols is None else np.unique(cols)
        k_rad = max(k_rad, R.units(I[s], ref["I"][s], ref["A_I"][s], ref["C_I"][s], n_gas).max())
        k_jac = max(k_jac, R.units(J[:, s], ref["J"][:, s], ref["A"][:, s], ref["C"][:, s], n_gas).max())
    return float(k_rad), float(k_jac)
