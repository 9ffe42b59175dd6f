"""Inputs and references of the tests of ray batches of five to eight gases (tests/test_many_gases_host.py,
tests/test_gpu_many_gases.py): a synthetic batch of three limb rays on twelve coefficient rows, the eight VMR profiles and
col_scale values, the regime panel of tests/limb_reference.py laid on the rows, a state of column, level and row parameters,
and the extended-precision reference of every ray.  A helper module: no fixture, no pytest setting, nothing that needs a GPU.

The yardstick is tests/limb_reference.py as it stands: recursion_reference in numpy.longdouble, errors in units of
2^-53 (A + (n_gas + 1) C) + 1e-290 -- the bound scales with the gas count by itself -- and every row is held to
KERNEL_MARGIN x K_PLAIN, K_PLAIN being the distance of plain_fp64 from the reference on the test's own inputs (k_plain
below), never what the code under test gives.

K_PLAIN of the eight-gas panel, measured on the CPU 2026-10-20 (panel_case(8), host_columns, all 188 panel columns, the
three rays; states "all", "cols17", "lev6"): radiances 5.27 units, Jacobian rows 5.21, 7.05 and 6.40; for five gases 4.55
and 5.74, 7.20, 6.98.  All stay below the recorded K_PLAIN_RAD = 41 and K_PLAIN_JAC = 25 of tests/limb_reference.py, which
tests/test_many_gases_host.py asserts on the live measurement.  (They measure LESS than the two-gas panel's 27.4 and 18.5:
the rays here have 7 to 23 segments, not 41, and the bound's (n_gas + 1) C grows with the gas count faster than the plain
recursion's error of a tau summed from eight products does.)
"""
import numpy as np

import limb_reference as R
import state_rows_cases as S

SEED = 20261020
N_LAYERS, N_PTS = 12, 300


def make_geo(tangents):
    """Limb rays that walk the rows from the outermost down to their turning row and up again, two sample points per
    segment: seg_layer, seg_off, pt_off."""
    seg_layer = np.concatenate([np.concatenate([np.arange(N_LAYERS - 1, t, -1), np.arange(t, N_LAYERS)]) for t in tangents]).astype(np.int32)
    seg_off = np.concatenate([[0], np.cumsum([2 * (N_LAYERS - t) - 1 for t in tangents])]).astype(np.int32)
    return dict(seg_layer=seg_layer, seg_off=seg_off, pt_off=2 * np.arange(seg_layer.size + 1, dtype=np.int32), n_seg=seg_layer.size,
                n_rays=len(tangents))


GEO3 = make_geo((8, 4, 0))                        # 7, 15 and 23 segments: the state tests and the split radiance kernel
GEO33 = make_geo([r % N_LAYERS for r in range(33)])   # 33 rays x 4100 points: beyond the split kernel's launch shapes
SEG_LAYER, SEG_OFF, PT_OFF, N_SEG, N_RAYS = GEO3["seg_layer"], GEO3["seg_off"], GEO3["pt_off"], GEO3["n_seg"], GEO3["n_rays"]
# the factor on each gas's columns (an isotopic abundance; 1 for a tabulated absorber)
COL_SCALE = np.array([0.98827, 1.0, 0.0111, 6.16e-4, 1.0, 0.9926, 1.0, 3.7e-3])
# the level-factored gases of the state kinds: (gas of the batch, levels, rows of its pair tables)
LEVEL_GASES = {"lev6": [(6, 5, 14)], "lev52": [(5, 4, 13), (2, 6, 15)]}


def geometry(seed, n_seg=N_SEG):
    """x, nd [2 n_seg]: two sample points per segment, the number density falling along it."""
    rng = np.random.default_rng([SEED, seed])
    x = (np.arange(n_seg)[:, None] + np.array([0.0, 1.0]) * rng.uniform(0.5, 1.0, (n_seg, 1))).reshape(-1)
    nd = (rng.uniform(0.5, 2.0, (n_seg, 1)) * np.array([1.0, 0.8])).reshape(-1)
    return x, nd


def path_arrays(seed):
    """alt, dx, dalt [n_pt] of a pointing call: any smooth numbers do (the column derivative is linear in dx and dalt);
    the altitudes of a segment's two points differ."""
    rng = np.random.default_rng([SEED, seed, 5])
    alt = (100.0 + 20.0 * SEG_LAYER[:, None] + np.array([0.0, 1.0]) * rng.uniform(5.0, 15.0, (N_SEG, 1))).reshape(-1)
    return dict(alt=alt, dx=rng.uniform(-0.2, 0.2, 2 * N_SEG), dalt=rng.uniform(0.5, 1.0, 2 * N_SEG))


def panel_case(n_gas, geo=GEO3):
    """The regime panel on the twelve coefficient rows (limb_reference.panel_problem: coef_a, coef_e [G, 12, N] and the
    columns col [G, 12] at which a row meets the panel's optical depth) and the VMR profiles that give a segment on row r
    those columns through col_scale (to rounding: constant along the segment)."""
    pan = R.panel_problem(N_LAYERS, n_gas, 0, SEED + n_gas)
    x, nd = geometry(n_gas, geo["n_seg"])
    u0 = S.cg_columns(nd, x, np.ones((1, 2 * geo["n_seg"])))[0]
    scale = COL_SCALE[:n_gas]
    vmr = np.repeat(pan["col"][:, geo["seg_layer"]] / (scale[:, None] * u0[None, :]), 2, axis=1)
    return dict(names=pan["names"], coef_a=pan["coef_a"], coef_e=pan["coef_e"], x=x, nd=nd, vmr=vmr, col_scale=scale, n_gas=n_gas,
                geo=geo, n_col=0, n_lev=0, n_row=0)


def host_columns(c):
    """[n_gas, n_seg]: the columns in numpy fp64, the host tests' stand-in for LimbLOS.columns()."""
    return c["col_scale"][:, None] * S.cg_columns(c["nd"], c["x"], c["vmr"])


KINDS = ("cols", "cols9", "cols17", "lev6", "lev52", "rows", "all")


def state(c, kind):
    """The state of one test, added to the case: column parameters (par_gas, par_w [n_col, n_pt]), level parameters of the
    level gases (lgases [(gas, tab, rows)], par_lgas, par_level, par_c), row parameters (dabs, demi [G, 12, N], par_t).
      cols    5 column parameters on gases n_gas - 1, 4, 0, n_gas - 1, 3 (at or above 4 among them)
      cols9   9 column parameters (two blocks of eight), cols17: 17 (three), gases cycling downwards from n_gas - 1
      lev6    4 column parameters + 5 level parameters of a level gas with index 6 (n_gas - 1 below seven gases)
      lev52   3 + 6 level parameters of two level gases with indices 5 (4 in a five-gas batch) and 2
      rows    3 row parameters with derivative spectra of every gas, 2 column parameters
      all     4 column, 3 + 3 level (two level gases) and 3 row parameters
    Parameter 1 of every kind has no weights.  A level's table holds a share of its gas's own coefficients on the table
    row its map names (dtau follows tau into every regime); the derivative spectra are state_rows_cases.panel_case's."""
    n_gas = c["n_gas"]
    N = len(c["names"])
    rng = np.random.default_rng([SEED, n_gas, KINDS.index(kind)])
    n_col = dict(cols=5, cols9=9, cols17=17, lev6=4, lev52=0, rows=2, all=4)[kind]
    lg_spec = dict(lev6=LEVEL_GASES["lev6"], lev52=LEVEL_GASES["lev52"], all=LEVEL_GASES["lev52"]).get(kind, [])
    lg_spec = [(min(g, n_gas - 1) if k == 0 else g, nl, nt) for k, (g, nl, nt) in enumerate(lg_spec)]
    levs = dict(lev6=(5,), lev52=(3, 6), all=(3, 3)).get(kind, ())
    n_row = dict(rows=3, all=3).get(kind, 0)
    if kind == "cols":
        par_gas = np.array([n_gas - 1, 4, 0, n_gas - 1, 3], np.int32)
    else:
        par_gas = ((n_gas - 1 - np.arange(n_col)) % n_gas).astype(np.int32)
    seg_w = rng.uniform(0.0, 1.0, (n_col, N_SEG)) * (rng.random((n_col, N_SEG)) < 0.7)
    if n_col > 1:
        seg_w[1] = 0.0
    par_w = np.repeat(seg_w, 2, axis=1) * c["vmr"][par_gas] if n_col else np.zeros((0, 2 * N_SEG))
    lgases, n_lev = [], sum(levs)
    for gas, n_levels, n_tab in lg_spec:
        rows = rng.permutation(n_tab)[:N_LAYERS].astype(np.int32)
        tab = rng.uniform(0.1, 1.0, (n_levels, 2, n_tab, N)) * 1e-18
        w = rng.uniform(0.2, 1.0, (n_levels, 2, N_LAYERS, 1))
        tab[:, 0, rows] = w[:, 0] * c["coef_a"][gas][None]
        tab[:, 1, rows] = w[:, 1] * c["coef_e"][gas][None]
        lgases.append((gas, tab, rows))
    par_lgas = rng.permutation(np.repeat(np.arange(len(levs)), levs)).astype(np.int32) if n_lev else np.zeros(0, np.int32)
    par_level = np.array([rng.integers(0, lg_spec[k][1]) for k in par_lgas], np.int32)
    par_c = rng.uniform(-1.0, 1.0, (n_lev, N_LAYERS)) * (rng.random((n_lev, N_LAYERS)) < 0.7)
    if n_lev > 1:
        par_c[1] = 0.0
    shape = c["coef_a"].shape
    m_a, m_e = rng.uniform(-1.0, 1.0, shape[1:]), rng.uniform(-1.0, 1.0, shape[1:])
    dabs = c["coef_a"] * m_a[None] * rng.uniform(0.5, 1.0, shape)
    demi = c["coef_e"] * m_e[None] * rng.uniform(0.5, 1.0, shape)
    par_t = rng.uniform(-1.0, 1.0, (n_row, N_LAYERS)) * (rng.random((n_row, N_LAYERS)) > 0.3)
    if n_row > 1:
        par_t[1] = 0.0
    out = dict(c)
    out.update(kind=kind, n_col=n_col, n_lev=n_lev, n_row=n_row, par_gas=par_gas, par_w=par_w, lgases=lgases, par_lgas=par_lgas,
               par_level=par_level, par_c=par_c, dabs=dabs, demi=demi, par_t=par_t)
    return out


def host_dcol(c):
    """[n_col, n_seg]: the columns of the column parameters' weight profiles, with their gas's col_scale."""
    if not c["n_col"]:
        return np.zeros((0, N_SEG))
    return c["col_scale"][c["par_gas"]][:, None] * S.cg_columns(c["nd"], c["x"], c["par_w"])


def ray_forms(c, col, dcol, ray, dtype, hidden=None):
    """tau, E [S, N] and dtau, dE [P, S, N] of one ray in `dtype`, the definition's products, the rows in the caller's
    order: column parameters (a_g D), level parameters (c u_gas A_L[row]), row parameters (w sum_g u_g dabs_g); hidden
    [n_gas, n_seg] (the pointing derivative's columns): one more row per gas behind them, a_g hidden_g."""
    segs = np.arange(c["geo"]["seg_off"][ray], c["geo"]["seg_off"][ray + 1])
    lay = c["geo"]["seg_layer"][segs]
    u = col[:, segs]
    ca, ce = c["coef_a"][:, lay], c["coef_e"][:, lay]
    tau, E = R.products(ca, u, dtype), R.products(ce, u, dtype)
    dtau, dE = [], []
    for p in range(c["n_col"]):
        g, D = c["par_gas"][p], np.asarray(dcol[p, segs], dtype)[:, None]
        dtau.append(np.asarray(ca[g], dtype) * D)
        dE.append(np.asarray(ce[g], dtype) * D)
    for p in range(c["n_lev"]):
        gas, tab, rows = c["lgases"][c["par_lgas"][p]]
        ug = np.asarray(u[gas], dtype)[:, None]
        w = np.asarray(c["par_c"][p, lay], dtype)[:, None]
        L = c["par_level"][p]
        dtau.append(w * (ug * np.asarray(tab[L, 0, rows[lay]], dtype)))
        dE.append(w * (ug * np.asarray(tab[L, 1, rows[lay]], dtype)))
    if c["n_row"]:
        da, de = R.products(c["dabs"][:, lay], u, dtype), R.products(c["demi"][:, lay], u, dtype)
        for p in range(c["n_row"]):
            w = np.asarray(c["par_t"][p, lay], dtype)[:, None]
            dtau.append(w * da)
            dE.append(w * de)
    if hidden is not None:
        for g in range(c["n_gas"]):
            D = np.asarray(hidden[g, segs], dtype)[:, None]
            dtau.append(np.asarray(ca[g], dtype) * D)
            dE.append(np.asarray(ce[g], dtype) * D)
    shape = (0,) + tau.shape
    return tau, E, np.array(dtau).reshape((-1,) + tau.shape) if dtau else np.zeros(shape, dtype), \
        np.array(dE).reshape((-1,) + tau.shape) if dE else np.zeros(shape, dtype)


def references(c, col, dcol, I0, solo=False, hidden=None, cols=None):
    """Per ray: (the reference dict of limb_reference.recursion_reference, the plain-fp64 results (I, J)), on the panel
    columns `cols` (None: all of them)."""
    out = []
    sel = (lambda a: a) if cols is None else (lambda a: a[..., cols])
    for ray in range(c["geo"]["n_rays"]):
        ld = [sel(v) for v in ray_forms(c, col, dcol, ray, R.LD, hidden)]
        pl = [sel(v) for v in ray_forms(c, col, dcol, ray, np.float64, hidden)]
        ref = R.recursion_reference(*ld, sel(np.asarray(I0)), solo=solo, thin_ulps=c["n_gas"] + 1)
        out.append((ref, R.plain_fp64(*pl, sel(np.asarray(I0)), solo=solo)))
    return out


def pointing_row(ref, J, n_state, n_gas):
    """The pointing row from the per-gas hidden rows behind the state's: (value of J summed in gas order, reference sum,
    A sum, C sum) -- the row is the sum of n_gas rows, and so are its reference and its bound."""
    sl = slice(n_state, n_state + n_gas)
    got = J[n_state].copy()
    for g in range(1, n_gas):
        got = got + J[n_state + g]
    return got, ref["J"][sl].sum(axis=0), ref["A"][sl].sum(axis=0), ref["C"][sl].sum(axis=0)


def k_plain(refs, n_gas, n_state=None):
    """(K_PLAIN of the radiances, of the Jacobian rows): plain fp64 against the reference on these inputs, in the bound's
    units.  n_state (a pointing case): the rows behind it are the per-gas hidden rows, measured as their sum."""
    k_rad = k_jac = 0.0
    for ref, (I, J) in refs:
        k_rad = max(k_rad, R.units(I, ref["I"], ref["A_I"], ref["C_I"], n_gas).max())
        n = J.shape[0] if n_state is None else n_state
        if n:
            k_jac = max(k_jac, R.units(J[:n], ref["J"][:n], ref["A"][:n], ref["C"][:n], n_gas).max())
        if n_state is not None:
            k_jac = max(k_jac, R.units(*pointing_row(ref, J, n_state, n_gas), n_gas).max())
    return float(k_rad), float(k_jac)
