"""Inputs of the ray-block tests (tests/test_state_rayblocks_host.py, tests/test_gpu_state_rayblocks.py): limb batches at
the smallest shapes at which the per-ray plan of sr_limb_jac_state_kernel can go wrong, raw weight arrays that give every
ray a chosen number of touching parameters, "touches" and the plan restated in numpy, and the extended-precision forms of
every ray.  A helper module: no fixture, no pytest setting, nothing that needs a GPU.

The main batch: 300 points (two point blocks, the last wave straddles the end), 3 gases, 12 coefficient rows, 6 limb rays
with tangent rows 11, 2, 0, 9, 5, 7 (down from row 11 to the tangent row and up again), two sample points per segment,
37 parameters (the dense plan: 3 blocks of 16).  A level or row parameter has a top row h and weights on rows h, h - 1 and
h - 3: a ray touches it iff its tangent row is <= h; the column parameters' weights are laid on the sample points of the
rays that are to touch them.  Ray 0 touches nothing, ray 1 sixteen parameters, ray 2 seventeen, ray 3 five, rays 4 and 5
thirteen and fourteen of mixed kinds, whatever the split of the 37 into kinds (while there are enough column parameters).
"""
import numpy as np

import limb_reference as R
from state_rows_cases import cg_columns

SEED = 20261019
N_PTS, N_LAYERS, N_GAS = 300, 12, 3
TANGENT = (11, 2, 0, 9, 5, 7)
TARGET = (0, 16, 17, 5, 13, 14)          # parameters that touch each ray of the main batch
LEV_TOP = (10, 9, 8, 6, 5, 4, 3, 2, 1, 0)
ROW_TOP = (10, 7, 6, 3, 1, 0)
N_LEVELS = (5, 3)                        # levels of the two level-factored gases' tables
LGAS_GAS = (2, 0)                        # their gases in the batch


def limb_batch(tangent=TANGENT, n_layers=N_LAYERS):
    seg_off, seg_layer = [0], []
    for t in tangent:
        seg_layer += list(range(n_layers - 1, t - 1, -1)) + list(range(t + 1, n_layers))
        seg_off.append(len(seg_layer))
    return np.array(seg_off, np.int32), np.array(seg_layer, np.int32)


def geometry(n_seg, seed):
    """x, nd [2 n_seg]: two sample points per segment, the number density falling along it."""
    rng = np.random.default_rng([SEED, seed])
    x = (np.arange(n_seg)[:, None] + np.array([0.0, 1.0]) * rng.uniform(0.5, 1.0, (n_seg, 1))).reshape(-1)
    nd = (rng.uniform(0.5, 2.0, (n_seg, 1)) * np.array([1.0, 0.8])).reshape(-1)
    return x, nd


def _row_weights(tops, n_layers, rng):
    w = np.zeros((len(tops), n_layers))
    for p, h in enumerate(tops):
        for r in (h, h - 1, h - 3):
            if r >= 0:
                w[p, r] = rng.uniform(0.3, 1.0) * rng.choice([-1.0, 1.0])
    return w


def main_case(n_col, n_lev, n_row, n_lgas=1, target=TARGET, tangent=TANGENT, lev_top=LEV_TOP, row_top=ROW_TOP, seed=0):
    """The regime panel of tests/limb_reference.py on the coefficient rows, VMRs that give a segment on row r the panel's
    columns, pair tables A_L = abs_g w_L, E_L = emi_g w_L' of the level gases (w in (0.1, 1): of the coefficients' size),
    derivative spectra as tests/state_rows_cases.py draws them, and the parameters.  Level parameter i has top row
    lev_top[i], row parameter i row_top[i]; ray k gets target[k] minus its level and row parameters column parameters."""
    assert n_lev <= len(lev_top) and n_row <= len(row_top)
    n_layers = N_LAYERS
    rng = np.random.default_rng([SEED, n_col, n_lev, n_row, n_lgas, seed])
    seg_off, seg_layer = limb_batch(tangent, n_layers)
    n_seg = seg_layer.size
    pan = R.panel_problem(n_layers, N_GAS, 0, SEED + seed)
    x, nd = geometry(n_seg, seed)
    u0 = cg_columns(nd, x, np.ones((1, 2 * n_seg)))[0]
    vmr = np.repeat(pan["col"][:, seg_layer] / u0[None, :], 2, axis=1)
    shape = pan["coef_a"].shape
    m_a, m_e = rng.uniform(-1.0, 1.0, shape[1:]), rng.uniform(-1.0, 1.0, shape[1:])
    dabs = pan["coef_a"] * m_a[None] * rng.uniform(0.5, 1.0, shape)
    demi = pan["coef_e"] * m_e[None] * rng.uniform(0.5, 1.0, shape)
    tabs, coef_rows = [], []
    for k in range(n_lgas):
        cr = rng.permutation(n_layers).astype(np.int32)
        tab = np.zeros((N_LEVELS[k], 2, n_layers, shape[2]))
        for L in range(N_LEVELS[k]):
            tab[L, 0, cr] = pan["coef_a"][LGAS_GAS[k]] * rng.uniform(0.1, 1.0, (n_layers, 1))
            tab[L, 1, cr] = pan["coef_e"][LGAS_GAS[k]] * rng.uniform(0.1, 1.0, (n_layers, 1))
        tabs.append(tab)
        coef_rows.append(cr)
    par_c, par_t = _row_weights(lev_top[:n_lev], n_layers, rng), _row_weights(row_top[:n_row], n_layers, rng)
    par_lgas = (np.arange(n_lev) % n_lgas).astype(np.int32)
    par_level = np.array([rng.integers(0, N_LEVELS[k]) for k in par_lgas], np.int32).reshape(-1)
    par_gas = rng.integers(0, N_GAS, n_col).astype(np.int32)
    par_w = np.zeros((n_col, 2 * n_seg))
    nxt = 0
    for ray, t in enumerate(tangent):
        lr = sum(h >= t for h in lev_top[:n_lev]) + sum(h >= t for h in row_top[:n_row])
        need = min(max(target[ray] - lr, 0), n_col)
        a, b = 2 * seg_off[ray], 2 * seg_off[ray + 1]
        for i in range(need):
            p = (nxt + i) % n_col
            w = rng.uniform(0.2, 1.0, b - a) * (rng.random(b - a) > 0.4)
            w[rng.integers(0, b - a)] = 0.5          # (at least one sample point)
            par_w[p, a:b] = w
        nxt += max(need - 1, 0)                      # the next ray shares one parameter with this one
    return dict(names=pan["names"], coef_a=pan["coef_a"], coef_e=pan["coef_e"], dabs=dabs, demi=demi, x=x, nd=nd, vmr=vmr,
                seg_off=seg_off, seg_layer=seg_layer, pt_off=2 * np.arange(n_seg + 1, dtype=np.int32), n_layers=n_layers,
                n_gas=N_GAS, n_col=n_col, n_lev=n_lev, n_row=n_row, n_lgas=n_lgas, par_gas=par_gas, par_w=par_w, par_lgas=par_lgas,
                par_level=par_level, par_c=par_c, par_t=par_t, tabs=tabs, coef_rows=coef_rows, lgas_gas=LGAS_GAS[:n_lgas])


def small_case(seed=1):
    """No ray is touched by more than 8 parameters (the NP = 8 instances): 4 + 5 + 3 parameters on the main batch's rays."""
    return main_case(4, 5, 3, target=(0, 7, 8, 3, 6, 5), lev_top=(10, 8, 5, 2, 0), row_top=(9, 4, 1), seed=seed)


def step_rows_case(seed=2):
    """A 3-D batch: a coefficient row per LOS step (n_layers = n_seg), 3 rays of 5, 9 and 7 steps; the panel lies on the
    steps.  Level and row parameters weight a few steps each -- of one ray, or of two."""
    rng = np.random.default_rng([SEED, 77, seed])
    seg_off = np.array([0, 5, 14, 21], np.int32)
    n_seg = 21
    seg_layer = np.arange(n_seg, dtype=np.int32)
    pan = R.panel_problem(n_seg, N_GAS, 0, SEED + 100 + seed)
    x, nd = geometry(n_seg, 50 + seed)
    u0 = cg_columns(nd, x, np.ones((1, 2 * n_seg)))[0]
    vmr = np.repeat(pan["col"] / u0[None, :], 2, axis=1)
    shape = pan["coef_a"].shape
    dabs = pan["coef_a"] * rng.uniform(-1.0, 1.0, shape[1:])[None] * rng.uniform(0.5, 1.0, shape)
    demi = pan["coef_e"] * rng.uniform(-1.0, 1.0, shape[1:])[None] * rng.uniform(0.5, 1.0, shape)
    cr = rng.permutation(n_seg).astype(np.int32)
    tab = np.zeros((N_LEVELS[0], 2, n_seg, shape[2]))
    for L in range(N_LEVELS[0]):
        tab[L, 0, cr] = pan["coef_a"][LGAS_GAS[0]] * rng.uniform(0.1, 1.0, (n_seg, 1))
        tab[L, 1, cr] = pan["coef_e"][LGAS_GAS[0]] * rng.uniform(0.1, 1.0, (n_seg, 1))
    n_col, n_lev, n_row = 9, 10, 6
    spans = [(5, 14), (5, 14), (14, 21), (14, 21), (3, 8), (12, 16), (5, 9), (9, 14), (16, 21), (5, 7)]   # none on ray 0 alone
    par_c, par_t = np.zeros((n_lev, n_seg)), np.zeros((n_row, n_seg))
    for p, (a, b) in enumerate(spans[:n_lev]):
        par_c[p, a:b] = rng.uniform(0.3, 1.0, b - a) * (rng.random(b - a) > 0.3)
        par_c[p, a] = 0.6
    for p, (a, b) in enumerate(spans[4:4 + n_row]):
        par_t[p, a:b] = rng.uniform(-1.0, 1.0, b - a)
    par_w = np.zeros((n_col, 2 * n_seg))
    for p, (a, b) in enumerate([(5, 14), (5, 14), (5, 14), (14, 21), (14, 21), (0, 5), (0, 9), (10, 18), (19, 21)]):
        par_w[p, 2 * a:2 * b] = rng.uniform(0.2, 1.0, 2 * (b - a))
    return dict(names=pan["names"], coef_a=pan["coef_a"], coef_e=pan["coef_e"], dabs=dabs, demi=demi, x=x, nd=nd, vmr=vmr,
                seg_off=seg_off, seg_layer=seg_layer, pt_off=2 * np.arange(n_seg + 1, dtype=np.int32), n_layers=n_seg, n_gas=N_GAS,
                n_col=n_col, n_lev=n_lev, n_row=n_row, n_lgas=1, par_gas=rng.integers(0, N_GAS, n_col).astype(np.int32), par_w=par_w,
                par_lgas=np.zeros(n_lev, np.int32), par_level=rng.integers(0, N_LEVELS[0], n_lev).astype(np.int32), par_c=par_c,
                par_t=par_t, tabs=[tab], coef_rows=[cr], lgas_gas=LGAS_GAS[:1])


# ------------------------------------------------------------------------------------------------------------------
# "touches" and the plan, restated
# ------------------------------------------------------------------------------------------------------------------
def touches(c, n_hid=0):
    """[n_rays, n_col + n_lev + n_row + n_hid] bool, the rows of jac: a column parameter touches a ray iff its weight is
    non-zero at one of the ray's sample points, a level or row parameter iff its coefficient is non-zero on the row of one
    of the ray's segments, a hidden pointing slot always."""
    n_rays = len(c["seg_off"]) - 1
    out = np.zeros((n_rays, c["n_col"] + c["n_lev"] + c["n_row"] + n_hid), bool)
    for ray in range(n_rays):
        s0, s1 = c["seg_off"][ray], c["seg_off"][ray + 1]
        rows = np.unique(c["seg_layer"][s0:s1])
        pts = slice(c["pt_off"][s0], c["pt_off"][s1])
        out[ray, :c["n_col"]] = (c["par_w"][:c["n_col"], pts] != 0).any(axis=1) if c["n_col"] else False
        out[ray, c["n_col"]:c["n_col"] + c["n_lev"]] = (c["par_c"][:c["n_lev"]][:, rows] != 0).any(axis=1) if c["n_lev"] else False
        out[ray, c["n_col"] + c["n_lev"]:c["n_col"] + c["n_lev"] + c["n_row"]] = \
            (c["par_t"][:c["n_row"]][:, rows] != 0).any(axis=1) if c["n_row"] else False
        out[ray, c["n_col"] + c["n_lev"] + c["n_row"]:] = True
    return out


def ray_lists(c, n_hid=0):
    """Per ray, the rows of jac of the parameters that touch it in the plan's order: columns (caller's order), hidden
    slots, level parameters by (level gas, level) -- stable --, row parameters."""
    T = touches(c, n_hid)
    n_col, n_lev, n_row = c["n_col"], c["n_lev"], c["n_row"]
    key = (c["par_lgas"][:n_lev].astype(np.int64) << 16 | c["par_level"][:n_lev]) if c["n_lgas"] > 1 else c["par_level"][:n_lev]
    order = np.argsort(key, kind="stable") if n_lev else np.zeros(0, int)
    lists = []
    for t in T:
        lst = [p for p in range(n_col) if t[p]] + [n_col + n_lev + n_row + g for g in range(n_hid)]
        lst += [n_col + int(p) for p in order if t[n_col + p]]
        lst += [n_col + n_lev + p for p in range(n_row) if t[n_col + n_lev + p]]
        lists.append(lst)
    return lists


def walks(c, n_hid=0):
    """(np, the (ray, block) pairs of the per-ray plan, rays x blocks of the dense plan)."""
    lists = ray_lists(c, n_hid)
    n_p = 16 if max(len(l) for l in lists) > 8 else 8
    n_par = c["n_col"] + c["n_lev"] + c["n_row"] + n_hid
    dense_np = 16 if n_par > 8 else 8
    return n_p, sum(max(1, -(-len(l) // n_p)) for l in lists), len(lists) * max(1, -(-n_par // dense_np))


# ------------------------------------------------------------------------------------------------------------------
# the extended-precision forms
# ------------------------------------------------------------------------------------------------------------------
def ray_forms(c, col, dcol, ray, dtype, observer=False):
    """tau, E [S, N] and dtau, dE [n_par, S, N] of one ray in `dtype`, the header's products: a column parameter of gas g
    dtau = abs_g D; a level parameter of level gas k dtau = c u_gas(k) A_L[row_k[r]]; a row parameter dtau = w sum_g u_g
    dabs_g[r].  col [n_gas, n_seg], dcol [n_col, n_seg]: fp64 inputs.  observer: the walk reversed."""
    segs = np.arange(c["seg_off"][ray], c["seg_off"][ray + 1])
    if observer:
        segs = segs[::-1]
    lay = c["seg_layer"][segs]
    u = col[:, segs]
    tau, E = R.products(c["coef_a"][:, lay], u, dtype), R.products(c["coef_e"][:, lay], u, dtype)
    dtau, dE = [], []
    for p in range(c["n_col"]):
        g = c["par_gas"][p]
        D = np.asarray(dcol[p, segs], dtype)[:, None]
        dtau.append(np.asarray(c["coef_a"][g, lay], dtype) * D)
        dE.append(np.asarray(c["coef_e"][g, lay], dtype) * D)
    for p in range(c["n_lev"]):
        k, L = c["par_lgas"][p], c["par_level"][p]
        w = (np.asarray(c["par_c"][p, lay], dtype) * np.asarray(u[c["lgas_gas"][k]], dtype))[:, None]
        rows = c["coef_rows"][k][lay]
        dtau.append(w * np.asarray(c["tabs"][k][L, 0, rows], dtype))
        dE.append(w * np.asarray(c["tabs"][k][L, 1, rows], dtype))
    if c["n_row"]:
        da, de = R.products(c["dabs"][:, lay], u, dtype), R.products(c["demi"][:, lay], u, dtype)
        for p in range(c["n_row"]):
            w = np.asarray(c["par_t"][p, lay], dtype)[:, None]
            dtau.append(w * da)
            dE.append(w * de)
    shape = (0,) + tau.shape
    return tau, E, (np.array(dtau) if dtau else np.zeros(shape, dtype)), (np.array(dE) if dE else np.zeros(shape, dtype))


def references(c, col, dcol, I0, solo=False, observer=False):
    """The reference dict of limb_reference.recursion_reference of every ray."""
    return [R.recursion_reference(*ray_forms(c, col, dcol, ray, R.LD, observer), I0, solo=solo, thin_ulps=c["n_gas"] + 1)
            for ray in range(len(c["seg_off"]) - 1)]
