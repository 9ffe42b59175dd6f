"""Vibrational-temperature parameters of SEVERAL level-factored gases in one state pass
(sr_limb_rays_jac_state_gases_dev, sr_limb_rays_state_bands_gases_dev; engine.limb_rays_state_jacobian /
limb_rays_state_bands with level_gases, engine.LevelFactoredSet, retrieval.inversion_state): a level parameter of level gas
k reads that gas's table, row map and column,
    dtau_p = c[p][r] u_{g_k}[s] A^k_L[row_k[r]],   dE_p = c[p][r] u_{g_k}[s] E^k_L[row_k[r]],
and the recursion is the state call's.  Checked (A) against one existing state call per level gas, (B) against the
extended-precision recursion of tests/limb_reference.py, (C) against central differences through glevel_combine ->
limb_rays, (D) for its refusals, (E) for n_lgas = 1, (F) on the instrument's bands, (G) in the retrieval driver.
Synthetic inputs at the shapes of tests/state_rows_cases.py; the level gases' tables differ in levels, rows and row maps."""
import copy
import ctypes as C

import numpy as np
import pytest

import limb_reference as R
import state_rows_cases as S

pytestmark = pytest.mark.gpu

N_LEVELS, N_TAB = (12, 5, 3), (4, 7, 5)                     # per level gas: levels and rows of its pair tables
ROW_MAPS = (np.array([0, 2, 1, 3, 3, 0], np.int32), np.array([6, 0, 4, 4, 2, 5], np.int32), np.array([1, 1, 0, 4, 3, 2], np.int32))


@pytest.fixture(scope="module")
def eng():
    import torch
    assert torch.cuda.is_available(), "these tests need the GPU"
    from spectrobot_amd import engine
    engine.set_device(0)
    return engine


def _t(v):
    import torch
    return torch.tensor(np.ascontiguousarray(v, dtype=np.float64), device="cuda")


def _np(t):
    return t.detach().cpu().numpy()


def _row_err(a, ref):
    """max |a - ref| of every (ray, parameter) row, scaled by the row's largest |ref| (rows of zeros: absolute)."""
    s = ref.abs().amax(dim=-1)
    s = s.masked_fill(s == 0, 1.0)
    return (a - ref).abs().amax(dim=-1) / s


def _mixed(n_gas, n_col, levs, n_row, n_pts=S.N_PTS):
    """Coefficients from optically thin to thick; per level gas its own pair tables (N_LEVELS, N_TAB, ROW_MAPS) and batch
    gas -- the last gas of the batch, then gas 0, then gas 1 --; levs[k] level parameters of level gas k, interleaved in the
    caller's order; level parameter 1, column parameter 1 and row parameter 1 have no weights at all; every level gas has a
    level-0 parameter; column parameter 0 belongs to level gas 0's gas (a gas with a VMR set and Tvib sets)."""
    n_lgas, n_lev = len(levs), sum(levs)
    rng = np.random.default_rng([S.SEED, 77, n_gas, n_col, n_lev, n_row, n_lgas])
    x, nd = S.geometry(7)
    vmr = rng.uniform(0.2, 0.8, (n_gas, 2 * S.N_SEG))
    shape = (n_gas, S.N_LAYERS, n_pts)
    co = (np.exp(rng.uniform(np.log(1e-4), np.log(3.0), shape)), rng.uniform(0.1, 1.0, shape))
    dco = (co[0] * rng.uniform(-1.0, 1.0, shape), co[1] * rng.uniform(-1.0, 1.0, shape))
    gases = [n_gas - 1, 0, 1][:n_lgas]
    tabs = [rng.uniform(0.1, 1.0, (N_LEVELS[k], 2, N_TAB[k], n_pts)) for k in range(n_lgas)]
    sparse = lambda n, m: rng.uniform(-1.0, 1.0, (n, m)) * (rng.uniform(size=(n, m)) > 0.2)
    par_w, par_c, par_t = np.abs(sparse(n_col, 2 * S.N_SEG)), sparse(n_lev, S.N_LAYERS), sparse(n_row, S.N_LAYERS)
    for a in (par_w, par_c, par_t):
        if len(a) > 1:
            a[1] = 0.0
    par_lgas = rng.permutation(np.repeat(np.arange(n_lgas), levs)).astype(np.int32)
    if n_lev > 1 and par_lgas[1] != 0:                    # (the parameter without weights is one of level gas 0's several)
        j = int(np.flatnonzero(par_lgas == 0)[0])
        par_lgas[1], par_lgas[j] = par_lgas[j], par_lgas[1]
    par_level = np.array([rng.integers(0, N_LEVELS[k]) for k in par_lgas], np.int32)
    for k in range(n_lgas):                               # a level-0 parameter per level gas (not the one without weights)
        par_level[[p for p in np.flatnonzero(par_lgas == k) if p != 1][0]] = 0
    par_gas = rng.integers(0, n_gas, n_col).astype(np.int32)
    if n_col:
        par_gas[0] = gases[0]
    return dict(x=x, nd=nd, vmr=vmr, co=tuple(_t(v) for v in co), dco=tuple(_t(v) for v in dco), co_np=co, tabs_np=tabs,
                tabs=[_t(v) for v in tabs], rows=[ROW_MAPS[k] for k in range(n_lgas)], gases=gases, par_gas=par_gas, par_w=par_w,
                par_lgas=par_lgas, par_level=par_level, par_c=par_c, par_t=par_t, n_col=n_col, n_lev=n_lev, n_row=n_row,
                n_lgas=n_lgas, n_gas=n_gas)


def _los(eng, m, **opts):
    return eng.LimbLOS(S.SEG_OFF, S.SEG_LAYER, S.PT_OFF, m["x"], m["nd"], m["vmr"], **opts)


def _level_gases(m):
    return [(m["gases"][k], m["tabs"][k], m["rows"][k]) for k in range(m["n_lgas"])]


def _third(m):
    return dict(dcoeffs=m["dco"], par_t=m["par_t"]) if m["n_row"] else {}


def _one_call(eng, m, los, **kw):
    return eng.limb_rays_state_jacobian(m["co"], los, m["par_gas"], m["par_w"], par_level=m["par_level"], par_c=m["par_c"],
                                        level_gases=_level_gases(m), par_lgas=m["par_lgas"], **_third(m), **kw)


def _per_gas_call(eng, m, los, k, **kw):
    """The existing call for level gas k alone, on the same coefficient stack: (rad, jac, the level parameters it holds)."""
    idx = np.flatnonzero(m["par_lgas"] == k)
    rad, jac = eng.limb_rays_state_jacobian(m["co"], los, m["par_gas"], m["par_w"], m["tabs"][k], m["rows"][k], m["par_level"][idx],
                                            m["par_c"][idx], gas=m["gases"][k], **_third(m), **kw)
    return rad, jac, idx


# ------------------------------------------------------------------------------------------------------------------
# A: against the existing calls, one per level gas
# ------------------------------------------------------------------------------------------------------------------
SHAPES = [(0, (3, 2), 0), (3, (4, 4), 0), (5, (7, 5), 4), (0, (9, 8), 0),          # two level gases
          (0, (2, 2, 1), 0), (5, (5, 4, 3), 4)]                                     # three
OPTIONS = {"-": {}, "observer": dict(LOS_order="observer"), "solo": dict(solo_absorption=True, initial_temperature=250.0),
           "planck": dict(initial_temperature=180.0), "shard": dict(initial_temperature=200.0)}


def _check_against_per_gas(eng, m, los, tag, **kw):
    import torch
    n_col, n_lev, n_row = m["n_col"], m["n_lev"], m["n_row"]
    rad, jac = _one_call(eng, m, los, **kw)
    assert tuple(jac.shape) == (3, n_col + n_lev + n_row, jac.shape[2]) and bool(torch.isfinite(jac).all())
    err_l = err_o = d_rad = 0.0
    exact = True
    for k in range(m["n_lgas"]):
        rad_k, jac_k, idx = _per_gas_call(eng, m, los, k, **kw)
        pairs = [(jac[:, n_col + idx], jac_k[:, n_col:n_col + idx.size])]                       # level rows: that gas's own call
        pairs += [(jac[:, :n_col], jac_k[:, :n_col]), (jac[:, n_col + n_lev:], jac_k[:, n_col + idx.size:])]   # the others: either
        for i, (got, ref) in enumerate(pairs):
            if got.shape[1] == 0:
                continue
            e = float(_row_err(got, ref).max())
            err_l, err_o = (max(err_l, e), err_o) if i == 0 else (err_l, max(err_o, e))
            zero = ref.abs().amax(dim=-1) == 0
            assert bool((got.abs().amax(dim=-1)[zero] == 0).all())                              # exact zeros there: exact zeros here
            exact = exact and torch.equal(got, ref)
        assert float(jac_k[:, n_col:n_col + idx.size].abs().max()) > 0
        d_rad = max(d_rad, float((rad - rad_k).abs().max() / rad_k.abs().max()))
        exact = exact and torch.equal(rad, rad_k)
    print("\nstate gases vs per-gas calls [%s]: level rows %.2e, column and row rows %.2e (bound 1e-12 of a row's largest value); "
          "radiances %.2e (bound 1e-13); bit for bit: %s" % (tag, err_l, err_o, d_rad, exact))
    assert err_l <= 1e-12 and err_o <= 1e-12 and d_rad <= 1e-13
    assert not bool(jac[:, n_col + 1].any())                                                    # the level parameter without weights
    if n_col > 1:
        assert not bool(jac[:, 1].any())
    return rad, jac


@pytest.mark.parametrize("n_gas,n_col,levs,n_row", [(g,) + s for s in SHAPES for g in (2, 3, 4) if len(s[1]) <= g])
def test_equals_the_existing_calls_per_level_gas(eng, n_gas, n_col, levs, n_row):
    """A.  3 + 2 level parameters: eight slots, one block; 3 + 4 + 4: sixteen slots; 5 + 7 + 5 + 4 and 9 + 8: two blocks, the
    level slots of both gases in one block and split across the blocks (the plan sorts them by level gas, then level; the
    caller's order is interleaved).  Level rows of gas k against that gas's own limb_rays_state_jacobian call, column and
    row rows against every one of those calls: 1e-12 of the row's largest value, the bound of
    tests/test_gpu_state_jacobian.py::test_equals_the_two_existing_calls for the same arithmetic; radiances 1e-13; rows that
    are exact zeros there are exact zeros here."""
    m = _mixed(n_gas, n_col, levs, n_row)
    los = _los(eng, m)
    try:
        _check_against_per_gas(eng, m, los, "n_gas %d, %d + %s + %d" % (n_gas, n_col, "+".join(map(str, levs)), n_row))
    finally:
        los.close()


@pytest.mark.parametrize("opt", ["observer", "solo", "planck", "shard"])
@pytest.mark.parametrize("n_gas,n_col,levs,n_row", [(2, 3, (4, 4), 0), (3, 5, (7, 5), 4)])
def test_options_equal_the_existing_calls(eng, opt, n_gas, n_col, levs, n_row):
    """A.  Observer order, absorption alone of a Planck background, emission on a Planck background, and a spectral shard
    (points 100 .. 399 of a 400-point grid, the Planck background taken there): the same comparison."""
    from spectrobot_amd import synthetic as syn
    m = _mixed(n_gas, n_col, levs, n_row)
    los = _los(eng, m, **OPTIONS[opt])
    kw = {}
    if opt in ("solo", "planck"):
        kw = dict(grid=syn.make_grid(2975.0, 5e-4, S.N_PTS))
    if opt == "shard":
        kw = dict(grid=syn.make_grid(2975.0, 5e-4, S.N_PTS + 100), g_lo=100)
    try:
        rad, jac = _check_against_per_gas(eng, m, los, "%s, n_gas %d, %d + %s + %d" % (opt, n_gas, n_col, "+".join(map(str, levs)), n_row), **kw)
        if opt == "shard":      # not the unsharded call's numbers: the background is the shard's
            rad0, _ = _one_call(eng, m, los, grid=syn.make_grid(2975.0, 5e-4, S.N_PTS))
            assert float((rad - rad0).abs().max()) > 0
    finally:
        los.close()


# ------------------------------------------------------------------------------------------------------------------
# B: level rows of both gases against the extended-precision reference
# ------------------------------------------------------------------------------------------------------------------
def panel_levels_case(n_gas, levs):
    """The regime panel on the six coefficient rows (state_rows_cases.panel_case) with two level gases: the last gas of the
    batch with 12 levels on 7 table rows, gas 0 with 5 levels on 9; level L of level gas k holds a random share of that
    gas's own coefficients on the table row ITS map names (so that dtau follows tau into every regime), random numbers on the
    rows no coefficient row uses.  levs[k] level parameters per gas, interleaved; parameter 1 has no weights; each gas has a
    level-0 parameter."""
    c = S.panel_case(n_gas, 3)
    rng = np.random.default_rng([S.SEED, 78, n_gas, sum(levs)])
    n_levels, n_tab = (12, 5), (7, 9)
    N = len(c["names"])
    gases = [n_gas - 1, 0]
    rows = [rng.permutation(n_tab[k])[:S.N_LAYERS].astype(np.int32) for k in range(2)]
    tabs = []
    for k in range(2):
        tab = rng.uniform(0.1, 1.0, (n_levels[k], 2, n_tab[k], N)) * 1e-18
        w = rng.uniform(0.2, 1.0, (n_levels[k], 2, S.N_LAYERS, 1))
        tab[:, 0, rows[k]] = w[:, 0] * c["coef_a"][gases[k]][None]
        tab[:, 1, rows[k]] = w[:, 1] * c["coef_e"][gases[k]][None]
        tabs.append(tab)
    n_lev = sum(levs)
    par_lgas = rng.permutation(np.repeat(np.arange(2), levs)).astype(np.int32)
    par_level = np.array([rng.integers(0, n_levels[k]) for k in par_lgas], np.int32)
    for k in range(2):
        par_level[[p for p in np.flatnonzero(par_lgas == k) if p != 1][0]] = 0
    par_c = rng.uniform(-1.0, 1.0, (n_lev, S.N_LAYERS)) * (rng.random((n_lev, S.N_LAYERS)) < 0.7)
    par_c[1] = 0.0
    par_c[0, 3] = 0.7                                       # (the single-segment ray's row: parameter 0 is seen by every ray)
    c.update(tabs=tabs, rows=rows, gases=gases, par_lgas=par_lgas, par_level=par_level, par_c=par_c)
    return c


def level_forms(c, col, ray, dtype):
    """tau, E [S, N] and dtau, dE [n_lev, S, N] of one ray in `dtype`, the definition's products:
    dtau_p = c[p][r] (u_{g_k} A^k_L[row_k[r]])."""
    segs = np.arange(S.SEG_OFF[ray], S.SEG_OFF[ray + 1])
    lay = S.SEG_LAYER[segs]
    u = col[:, segs]
    tau, E = R.products(c["coef_a"][:, lay], u, dtype), R.products(c["coef_e"][:, lay], u, dtype)
    dtau, dE = [], []
    for p, (k, L) in enumerate(zip(c["par_lgas"], c["par_level"])):
        ug = np.asarray(u[c["gases"][k]], dtype)[:, None]
        w = np.asarray(c["par_c"][p, lay], dtype)[:, None]
        trow = c["rows"][k][lay]
        dtau.append(w * (ug * np.asarray(c["tabs"][k][L, 0, trow], dtype)))
        dE.append(w * (ug * np.asarray(c["tabs"][k][L, 1, trow], dtype)))
    return tau, E, np.array(dtau), np.array(dE)


PANEL_CASES = [(2, (5, 4), "-"), (3, (5, 4), "-"), (4, (5, 4), "-"), (2, (9, 8), "solo"), (3, (9, 8), "planck"), (4, (3, 2), "-")]


@pytest.mark.parametrize("n_gas,levs,opt", PANEL_CASES)
def test_level_rows_of_both_gases_against_the_extended_precision_reference(eng, n_gas, levs, opt):
    """B.  Level parameters of two level gases -- 3 + 2: eight slots; 5 + 4: sixteen; 9 + 8: two blocks -- on the regime
    panel laid on the six coefficient rows.  Every (ray, parameter) row within KERNEL_MARGIN x K_PLAIN units of the bound of
    tests/limb_reference.py, K_PLAIN being what the plain fp64 recursion measures against the reference on THESE inputs
    (radiances and Jacobians separately), never what the kernel gives -- the yardstick of DESIGN 4.5a as
    tests/test_gpu_state_rows.py applies it.  Every figure is printed before anything is asserted."""
    import torch
    from spectrobot_amd import synthetic as syn
    c = panel_levels_case(n_gas, levs)
    N = len(c["names"])
    at = R.tile_columns(N, S.N_PTS, np.random.default_rng([S.SEED, n_gas, sum(levs), 2]))
    cols = at
    solo, planck = opt == "solo", opt in ("solo", "planck")
    opts = dict(solo_absorption=True, initial_temperature=250.0) if solo else (dict(initial_temperature=180.0) if planck else {})
    grid = syn.make_grid(2975.0, 5e-4, S.N_PTS) if planck else None
    plain = eng.LimbLOS(S.SEG_OFF, S.SEG_LAYER, S.PT_OFF, c["x"], c["nd"], c["vmr"])
    col = plain.columns()
    plain.close()
    los = eng.LimbLOS(S.SEG_OFF, S.SEG_LAYER, S.PT_OFF, c["x"], c["nd"], c["vmr"], **opts)
    try:
        assert np.allclose(col, S.cg_columns(c["nd"], c["x"], c["vmr"]), rtol=1e-12)
        I0 = np.zeros(N)
        if planck:
            zero = torch.zeros((n_gas, S.N_LAYERS, S.N_PTS), dtype=torch.float64, device="cuda")
            I0 = _np(eng.limb_rays((zero, zero), los, grid=grid, resident=False))[0][:N]
            cols = cols[:N]
        refs = []
        for ray in range(3):
            ref = R.recursion_reference(*level_forms(c, col, ray, R.LD), I0, solo=solo, thin_ulps=n_gas + 1)
            refs.append((ref, R.plain_fp64(*level_forms(c, col, ray, np.float64), I0, solo=solo)))
        k_rad, k_jac = S.k_plain(refs, n_gas, cols)
        pick = lambda a: _t(a[..., at])
        rad, jac = eng.limb_rays_state_jacobian((pick(c["coef_a"]), pick(c["coef_e"])), los, grid=grid, par_level=c["par_level"],
                                                par_c=c["par_c"], par_lgas=c["par_lgas"],
                                                level_gases=[(c["gases"][k], pick(c["tabs"][k]), c["rows"][k]) for k in range(2)])
    finally:
        los.close()
    n_lev = sum(levs)
    assert tuple(jac.shape) == (3, n_lev, S.N_PTS) and tuple(rad.shape) == (3, S.N_PTS)
    rad, jac = _np(rad)[:, :len(cols)], _np(jac)[:, :, :len(cols)]
    lim_rad, lim_jac = R.KERNEL_MARGIN * k_rad, R.KERNEL_MARGIN * k_jac
    print("\nstate gases vs reference [n_gas %d, %d + %d levels, %s]: K_PLAIN rad %.3g jac %.3g, limits %.3g %.3g"
          % (n_gas, levs[0], levs[1], opt, k_rad, k_jac, lim_rad, lim_jac))
    over = []
    for r, (ref, _) in enumerate(refs):
        u_r = R.worst(R.units(rad[r], ref["I"][cols], ref["A_I"][cols], ref["C_I"][cols], n_gas), c["names"], cols)
        worst_k = []
        for k in range(2):
            idx = np.flatnonzero(c["par_lgas"] == k)
            worst_k.append(R.worst(R.units(jac[r][idx], ref["J"][idx][:, cols], ref["A"][idx][:, cols], ref["C"][idx][:, cols], n_gas),
                                   c["names"], cols))
        print("  ray %d (%d seg): rad %.3g units at %s; level rows of gas A %.3g units at %s, of gas B %.3g units at %s"
              % (r, S.SEG_OFF[r + 1] - S.SEG_OFF[r], u_r[0], u_r[1], worst_k[0][0], worst_k[0][1], worst_k[1][0], worst_k[1][1]))
        over += [("rad", r) + u_r] * (not u_r[0] <= lim_rad)
        over += [("jac gas %d" % k, r) + w for k, w in enumerate(worst_k) if not w[0] <= lim_jac]
    assert 0.0 < k_rad <= R.K_PLAIN_RAD and 0.0 < k_jac <= R.K_PLAIN_JAC
    assert not over, "over %g x K_PLAIN (rad %.3g, jac %.3g units): %s" % (R.KERNEL_MARGIN, lim_rad, lim_jac, over)
    assert not jac[:, 1].any()                                           # the parameter without weights: exact zeros
    if not solo:
        assert np.abs(jac[:, 0]).max(axis=-1).min() > 0                  # parameter 0 is seen by every ray


# ------------------------------------------------------------------------------------------------------------------
# C: central differences through glevel_combine -> limb_rays
# ------------------------------------------------------------------------------------------------------------------
def test_central_differences_of_a_population_of_the_second_level_gas(eng):
    """C.  The coefficients of the SECOND level gas are glevel_combine of its tables and populations; the best-seen level
    parameter of that gas against central differences of glevel_combine -> limb_rays on pop[:, L] +- h c[p] at h and h / 2.
    |jac - FD(h/2)| <= 2 |FD(h) - FD(h/2)| + 1e-9 max|jac| per ray in the max norm (the project's rule), and the row reaches
    1e-3 of max|rad| so that the comparison is of something."""
    m = _mixed(3, 3, (4, 4), 0)
    k = 1
    gas, tab, rows = m["gases"][k], m["tabs"][k], m["rows"][k]
    rng = np.random.default_rng([S.SEED, 79])
    pop = rng.uniform(0.2, 1.0, (S.N_LAYERS, N_LEVELS[k]))

    def stack(p):
        a, e = eng.glevel_combine(tab, rows, p)
        co_a, co_e = m["co"][0].clone(), m["co"][1].clone()
        co_a[gas], co_e[gas] = a, e
        return co_a, co_e

    m["co"] = stack(pop)
    los = _los(eng, m)
    try:
        rad, jac = _one_call(eng, m, los)
        idx = np.flatnonzero(m["par_lgas"] == k)
        seen = (jac[:, m["n_col"] + idx].abs().amax(dim=(0, 2)) / rad.abs().max()).cpu().numpy()
        p = int(idx[int(np.argmax(seen))])
        L = int(m["par_level"][p])

        def fd(h):
            out = []
            for sgn in (1.0, -1.0):
                q = pop.copy()
                q[:, L] += sgn * h * m["par_c"][p]
                out.append(eng.limb_rays(stack(q), los).clone())
            return (out[0] - out[1]) / (2.0 * h)

        h = 1e-3
        f1, f2 = fd(h), fd(0.5 * h)
    finally:
        los.close()
    row = jac[:, m["n_col"] + p]
    jm = float(row.abs().max())
    trunc = (f1 - f2).abs().amax(dim=-1)
    err = (row - f2).abs().amax(dim=-1)
    print("\nstate gases FD: max|jac| / max|rad| per level parameter of the second gas %s; parameter %d (level %d), h %.3g: "
          "|jac - FD(h/2)| / max|jac| %.2e, |FD(h) - FD(h/2)| / max|jac| %.2e"
          % (np.array2string(seen, precision=2), p, L, h, float(err.max()) / jm, float(trunc.max()) / jm))
    assert jm >= 1e-3 * float(rad.abs().max())
    assert bool((err <= 2.0 * trunc + 1e-9 * jm).all())


# ------------------------------------------------------------------------------------------------------------------
# D: refusals
# ------------------------------------------------------------------------------------------------------------------
def test_refused_calls_leave_the_outputs_untouched(eng):
    """D.  Every refused argument returns its status before anything is copied or launched (rad, jac and the bands' out keep
    their sentinel), and a valid call afterwards reproduces the earlier result bit for bit."""
    import torch
    from spectrobot_amd import _lib, synthetic as syn
    m = _mixed(3, 5, (7, 5), 4)
    grid = syn.make_grid(2975.0, 5e-4, S.N_PTS)
    lam = 1e7 / grid[150]
    cen, wid = np.array([lam, lam + 0.01]), np.array([0.02, 0.03])
    los = _los(eng, m)
    a, e = m["co"]
    da, de = m["dco"]
    n_gas, n_layers, n_pts = a.shape
    n_col, n_lev, n_row = 5, 12, 4
    par_w, par_c, par_t = (np.ascontiguousarray(m[k]) for k in ("par_w", "par_c", "par_t"))
    good_rad, good = _one_call(eng, m, los)
    good_bands = eng.limb_rays_state_bands(m["co"], los, grid, cen, wid, m["par_gas"], m["par_w"], par_level=m["par_level"],
                                           par_c=m["par_c"], level_gases=_level_gases(m), par_lgas=m["par_lgas"], **_third(m))
    torch.cuda.synchronize()
    jac = torch.full((3, n_col + n_lev + n_row, n_pts), 7.25, dtype=torch.float64, device="cuda")
    rad = torch.full((3, n_pts), 7.25, dtype=torch.float64, device="cuda")
    out = np.full((3, 1 + n_col + n_lev + n_row, 2), 7.25)
    ip_, dp_ = _lib.ip, _lib.dp
    ptr = lambda t: C.c_void_p(t.data_ptr())

    def call(bands, **kw):
        d = los.desc(grid)
        d.w0, d.step = grid[0], grid[1] - grid[0]
        if "init_mode" in kw:
            d.init_mode = kw["init_mode"]
        no = kw.get("no", ())
        gases, rows = kw.get("gases", m["gases"]), kw.get("rows", m["rows"])
        arr = (_lib.LevelGasDesc * len(gases))()
        keep = []
        for k, g in enumerate(gases):
            r = np.ascontiguousarray(rows[k], dtype=np.int32)
            keep.append(r)
            arr[k].gas, arr[k].n_levels, arr[k].n_tab_rows = g, N_LEVELS[k], N_TAB[k]
            arr[k].tab = None if ("tab", k) in no else m["tabs"][k].data_ptr()
            arr[k].coef_row = None if ("coef_row", k) in no else r.ctypes.data_as(ip_)
        plg = np.ascontiguousarray(kw.get("par_lgas", m["par_lgas"]), dtype=np.int32)
        lev = np.ascontiguousarray(kw.get("par_level", m["par_level"]), dtype=np.int32)
        head = (ptr(a), ptr(e), n_layers, kw.get("n_pts", n_pts), C.byref(d), n_col, m["par_gas"].ctypes.data_as(ip_),
                par_w.ctypes.data_as(dp_), kw.get("n_lgas", len(gases)), arr, n_lev, plg.ctypes.data_as(ip_), lev.ctypes.data_as(ip_),
                par_c.ctypes.data_as(dp_), ptr(da), ptr(de), n_row, par_t.ctypes.data_as(dp_))
        if bands:
            return _lib.lib.sr_limb_rays_state_bands_gases_dev(*head, cen.ctypes.data_as(dp_), wid.ctypes.data_as(dp_), 2, 5.0, 0, None,
                                                               out.ctypes.data_as(dp_), eng._stream_ptr())
        return _lib.lib.sr_limb_rays_jac_state_gases_dev(*head, ptr(rad), ptr(jac), eng._stream_ptr())

    first_of = lambda k: int(np.flatnonzero(m["par_lgas"] == k)[0])
    bad_lgas, bad_lev_a, bad_lev_b = m["par_lgas"].copy(), m["par_level"].copy(), m["par_level"].copy()
    bad_lgas[3] = 2
    bad_lev_a[first_of(1)] = N_LEVELS[1]                      # a level of gas A, not of gas B
    bad_lev_b[first_of(0)] = -1
    bad_rows = [m["rows"][0], m["rows"][1].copy()]
    bad_rows[1][2] = N_TAB[1]
    rows_of_a = [m["rows"][0].copy(), m["rows"][1]]
    rows_of_a[0][4] = N_TAB[0]                                # a row of gas B's tables, not of gas A's
    A_, L_ = _lib.SR_ERR_ARG, _lib.SR_ERR_LIMIT
    refused = [(dict(n_lgas=0), A_), (dict(n_lgas=5), A_), (dict(gases=[2, 2]), A_), (dict(gases=[2, 3]), A_), (dict(gases=[-1, 0]), A_),
               (dict(no=(("tab", 1),)), A_), (dict(no=(("coef_row", 0),)), A_), (dict(par_lgas=bad_lgas), A_),
               (dict(par_level=bad_lev_a), A_), (dict(par_level=bad_lev_b), A_), (dict(rows=bad_rows), A_), (dict(rows=rows_of_a), A_),
               (dict(init_mode=1), A_), (dict(n_pts=2000001), L_)]
    try:
        for bands in (False, True):
            for kw, status in refused:
                assert call(bands, **kw) == status, (bands, kw)
                torch.cuda.synchronize()
                assert bool((jac == 7.25).all()) and bool((rad == 7.25).all()) and np.all(out == 7.25), (bands, kw)
        assert call(False) == _lib.SR_OK and call(True) == _lib.SR_OK
        torch.cuda.synchronize()
        assert torch.equal(jac, good) and torch.equal(rad, good_rad) and np.array_equal(out, good_bands)
    finally:
        los.close()


# ------------------------------------------------------------------------------------------------------------------
# E: one level gas is the existing call
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_gas,n_row", [(1, 0), (3, 0), (2, 4)])
def test_one_level_gas_is_the_existing_call_bit_for_bit(eng, n_gas, n_row):
    """E.  n_lgas = 1 through the new entries: bit for bit the existing state (n_row = 0), rows and bands calls."""
    import torch
    from spectrobot_amd import synthetic as syn
    m = _mixed(n_gas, 5, (7,), n_row)
    grid = syn.make_grid(2975.0, 5e-4, S.N_PTS)
    lam = 1e7 / grid[150]
    cen, wid = np.array([lam - 0.02, lam, lam + 0.01]), np.array([0.02, 0.03, 0.01])
    los = _los(eng, m)
    try:
        old = dict(tab=m["tabs"][0], coef_row=m["rows"][0], gas=m["gases"][0], par_level=m["par_level"], par_c=m["par_c"], **_third(m))
        new = dict(level_gases=_level_gases(m), par_lgas=m["par_lgas"], par_level=m["par_level"], par_c=m["par_c"], **_third(m))
        assert not m["par_lgas"].any()
        rad0, jac0 = eng.limb_rays_state_jacobian(m["co"], los, m["par_gas"], m["par_w"], **old)
        rad1, jac1 = eng.limb_rays_state_jacobian(m["co"], los, m["par_gas"], m["par_w"], **new)
        b0 = eng.limb_rays_state_bands(m["co"], los, grid, cen, wid, m["par_gas"], m["par_w"], **old)
        b1 = eng.limb_rays_state_bands(m["co"], los, grid, cen, wid, m["par_gas"], m["par_w"], **new)
    finally:
        los.close()
    assert tuple(jac1.shape) == tuple(jac0.shape) == (3, 12 + n_row, S.N_PTS)
    assert torch.equal(jac1, jac0) and torch.equal(rad1, rad0) and np.array_equal(b0, b1) and np.any(b0 != 0.0)


# ------------------------------------------------------------------------------------------------------------------
# F: on the instrument's bands
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kinds,n,order,planck,n_extra", [((3, 5, 0), 63, "photon", False, 0), ((0, 8, 0), 257, "observer", False, 0),
                                                           ((5, 12, 3), 700, "photon", False, 30), ((2, 17, 0), 257, "photon", True, 30),
                                                           ((0, 16, 4), 700, "observer", False, 0)])
def test_bands_in_one_call_equal_the_composition(eng, kinds, n, order, planck, n_extra):
    """F.  The one call against the new spectra call -> hires_to_lowres -> fov_closed_form on the inputs of
    tests/test_gpu_state_bands.py with a second level gas (gas 1: six levels on eleven table rows; gas 2: four levels on
    five, its own row map), 7 and 37 bands, without and with the field of view: max |fused - composed| / scale <= 1e-12, that
    file's bound; the band outside the grid is exactly 0.0 in every row."""
    import torch
    import test_gpu_state_bands as TB
    from spectrobot_amd import spect_main_module as smm
    n_col, n_lev, n_row = kinds
    c = TB._case(eng, n_col, n_lev, n_row, 3, n, order=order, planck=planck, seed=11)
    rng = c["rng"]
    bands, widths = TB._bands(c["grid"], n_extra, rng)
    tab2 = rng.uniform(0, 4e-18, (4, 2, 5, n))
    tab2[:, 1] *= rng.uniform(1e-8, 1e-7, tab2[:, 1].shape)
    kw = dict(c["kw"])
    tab1, rows1, par_level = kw.pop("tab"), kw.pop("coef_row"), kw.pop("par_level").copy()
    kw.pop("gas")
    par_lgas = (rng.permutation(n_lev) % 2).astype(np.int32)
    par_level[par_lgas == 1] %= 4
    kw.update(level_gases=[(1, tab1, rows1), (2, torch.tensor(tab2, device="cuda"), (np.arange(TB.NL) % 5).astype(np.int32))],
              par_lgas=par_lgas, par_level=par_level)
    los = TB._los(eng, c)
    for with_fov in (False, True):
        rad, jac = eng.limb_rays_state_jacobian(c["coeffs"], los, grid=c["grid"], **kw)
        low = lambda r: eng.hires_to_lowres(r.contiguous(), c["grid"], bands, widths)
        u = np.concatenate([low(rad)[:, None, :], low(jac.view(los.n_rays * c["n_par"], -1)).reshape(los.n_rays, c["n_par"], -1)], axis=1)
        if with_fov:
            u = smm.fov_closed_form(u[0::3], u[1::3], u[2::3], TB.ROTS)
        f = eng.limb_rays_state_bands(c["coeffs"], los, c["grid"], bands, widths, fov=eng.fov_factors(TB.ROTS) if with_fov else None, **kw)
        assert f.shape == u.shape == ((2 if with_fov else 6), 1 + c["n_par"], bands.size)
        dist, scale = TB._distance(f, u)
        print("\nstate gases bands %s n_pts %d %s%s %d bands fov %d: max |fused - composed| / scale = %.2e (smallest scale %.2e)"
              % (kinds, n, order, " planck" if planck else "", bands.size, with_fov, dist, scale.min()))
        assert np.all(f[..., 0] == 0.0) and np.all(u[..., 0] == 0.0)          # the band outside the grid
        assert np.all(scale > 0)
        assert dist <= TB.BOUND, dist


# ------------------------------------------------------------------------------------------------------------------
# G: the driver
# ------------------------------------------------------------------------------------------------------------------
def _scene(eng, n_grid=16000, n_layers=24):
    """The scene of tests/test_gpu_inversion_state.py with its HCN-like gas on the level-factored route too: two LevelGas,
    HCN (6 levels) and CH4 (12)."""
    import bench_configs as bc
    from spectrobot_amd import retrieval, synthetic as syn
    grid = syn.make_grid(3290.0, 5e-4, n_grid)
    Lc = syn.make_lines(3000, grid, config_id=4, n_levels=12)
    Lh = syn.make_lines(800, grid, config_id=5, n_levels=6)
    Lh["a_coeff"] = Lh["a_coeff"] * 30.0
    atm = syn.make_atmosphere(n_layers, 12)
    ch4 = retrieval.LevelGas("CH4", eng.LineSet(Lc, grid, 6, 1, syn.CH4_MM, syn.CH4_LEVEL_ENERGIES), np.full(n_layers, 1.48e-4),
                             atm["tvib"], syn.CH4_ISO_RATIO)
    tv_h = np.tile(atm["temps"], (6, 1)) + np.linspace(0.0, 10.0, 6)[:, None]
    hcn = retrieval.LevelGas("HCN", eng.LineSet(Lh, grid, 23, 1, bc.HCN_MM, bc.HCN_LEVEL_ENERGIES), np.full(n_layers, 2e-6),
                             tv_h, bc.HCN_ISO_RATIO)
    lam = np.linspace(1e7 / grid[-1] + 1.2, 1e7 / grid[0] - 1.2, 12)
    scene = retrieval.LimbScene(grid, atm["z"], atm["temps"], atm["press"], [hcn, ch4], lam, np.full(12, 1.1))
    z = atm["z"]
    span = z[-1] - z[0]
    pixels = [retrieval.LimbPixel(z[0] + (0.1 + 0.16 * i) * span, fov_half=0.02 * span, pixel_rot=10.0 * (i % 3)) for i in range(5)]
    return scene, pixels


def _observe(scene, pixels, noise_frac, rng=None):
    from spectrobot_amd import retrieval
    for pix, y in zip(pixels, retrieval.radtrans(scene, pixels)):
        sig = noise_frac * np.abs(y.spectrum).max() * np.ones_like(y.spectrum)
        obs = y.spectrum + (sig * rng.standard_normal(sig.size) if rng is not None else 0.0)
        pix.observation, pix.noise = retrieval.Spectrum(obs, scene.bands_nm), retrieval.Spectrum(sig, scene.bands_nm)


def _nodes(z):
    span = z[-1] - z[0]
    return [z[0] + f * span for f in (0.1, 0.45, 0.8)], [z[0] + f * span for f in (0.15, 0.4, 0.65, 0.9)]


@pytest.mark.parametrize("bands_in_kernel", [False, True])
def test_driver_one_iteration_equals_the_composition(eng, bands_in_kernel, monkeypatch):
    """G.  HCN VMR nodes between the Tvib nodes of an HCN level and of two CH4 levels, one iteration, ONE Jacobian call of
    the new kind: bayes_set.jacobian against limb_rays_jacobian + one tvib_jacobian per gas -> hires_to_lowres ->
    smm.FOV_integr_1D(closed_form=True) within 1e-11 of a column's largest element, the update against
    smm.inversion_algebra_arrays on that K to rtol 1e-9 (the bounds of tests/test_gpu_inversion_state.py)."""
    from spectrobot_amd import retrieval, spect_main_module as smm
    scene, pixels = _scene(eng)
    z = scene.z
    hcn_nodes, tv_nodes = _nodes(z)
    scene.gas("HCN").add_clim(np.full(len(z), 2.6e-6))
    tv = scene.gas("CH4").tvib0.copy()
    tv[5] += 5.0
    tv[2] -= 3.0
    scene.gas("CH4").set_tvib(tv)
    _observe(scene, pixels, 0.004, np.random.default_rng(5))
    bs = smm.BayesSet(tag="HCN + Tvib of an HCN level and of two CH4 levels")
    bs.add_set(retrieval.TvibProfile("CH4", 5, z, tv_nodes, np.full(4, 4.0), first_guess=np.array([1.0, -0.5, 0.7, 0.2])))
    bs.add_set(smm.LinearProfile_1D_new("HCN", z, hcn_nodes, np.full(3, 2.2e-6), np.full(3, 1.1e-6)))
    bs.add_set(retrieval.TvibProfile("HCN", 1, z, tv_nodes[:3], np.full(3, 4.0), first_guess=np.array([0.5, -1.0, 0.3])))
    bs.add_set(retrieval.TvibProfile("CH4", 2, z, tv_nodes[:3], np.full(3, 4.0)))
    n_par = 13
    ref = copy.deepcopy(bs)
    retrieval._state_into_gases(scene, ref)
    pix = sorted(pixels, key=lambda p: p.limb_tg_alt)
    alts = [a for p in pix for a in p.los_alts()]
    coeffs = scene.coefficient_stack()
    los, alt = scene.los(alts)
    w = scene.state_weights(ref, alt, several_level_gases=True)
    assert [g.name for g in w.level_gases] == ["CH4", "HCN"] and w.gases == [1, 0]
    assert list(w.par_lgas) == [0] * 4 + [1] * 3 + [0] * 3 and list(w.perm) == [3, 4, 5, 6, 0, 1, 2, 7, 8, 9, 10, 11, 12]
    rad, jc = eng.limb_rays_jacobian(coeffs, los, w.par_gas, w.par_w_col)
    jl = [None] * 10
    for k, (lg, gas) in enumerate(zip(w.level_gases, w.gases)):
        idx = np.flatnonzero(w.par_lgas == k)
        _, j = lg.lf.tvib_jacobian(coeffs, los, lg.rows, lg.tvib, w.par_level[idx], w.par_w_lev[idx], gas=gas)
        for i, p in enumerate(idx):
            jl[p] = j[:, i]
    import torch
    jl = torch.stack(jl, dim=1)
    low = lambda t: eng.hires_to_lowres(t.contiguous(), scene.grid, scene.bands_nm, scene.widths_nm, out_units=scene.out_units)
    lo_r = low(rad)
    lo_j = np.concatenate([low(jc).reshape(len(alts), 3, -1), low(jl).reshape(len(alts), 10, -1)], axis=1)[:, w.perm]
    sp = lambda v: retrieval.Spectrum(v, scene.bands_nm)
    nb = len(scene.bands_nm)
    sims, K = [], np.zeros((len(pix) * nb, n_par))
    for i, p in enumerate(pix):
        sims.append(smm.FOV_integr_1D([sp(lo_r[3 * i + q]) for q in range(3)], p.pixel_rot, closed_form=True).spectrum)
        for k in range(n_par):
            K[i * nb:(i + 1) * nb, k] = smm.FOV_integr_1D([sp(lo_j[3 * i + q, k]) for q in range(3)], p.pixel_rot, closed_form=True).spectrum
    obs_vec = np.concatenate([p.observation.spectrum for p in pix])
    noi_vec = np.concatenate([p.noise.spectrum for p in pix])
    sim_vec = np.concatenate(sims)
    smm.inversion_algebra_arrays(K, obs_vec, sim_vec, noi_vec, ref, lambda_LM=0.1)
    # the driver, one iteration: one call of the new kind and no other Jacobian call
    seen = []
    for name in ("limb_rays_state_jacobian", "limb_rays_state_bands"):
        real = getattr(eng, name)
        monkeypatch.setattr(retrieval.engine, name, lambda *a, _r=real, _n=name, **k: (seen.append((_n, len(k["level_gases"]))), _r(*a, **k))[1])
    chi, obs, out, b = retrieval.inversion_state(scene, bs, pixels, max_it=1, bands_in_kernel=bands_in_kernel)
    monkeypatch.undo()
    assert seen == [("limb_rays_state_bands" if bands_in_kernel else "limb_rays_state_jacobian", 2)]
    assert b is bs and len(b.history) == 1 and b.stop == 'max_it' and chi == b.history[0]
    assert b.jacobian.shape == K.shape and len(out) == len(pix)
    col_max = np.abs(K).max(axis=0)
    dist = np.abs(b.jacobian - K).max(axis=0) / np.where(col_max > 0, col_max, 1.0)
    chi_ref = np.sum(((obs_vec - sim_vec) / noi_vec) ** 2) / (obs_vec.size - n_par)
    print("\ninversion_state, Tvib of two gases (bands in kernel %d): |K - composition| per column / the column's largest element: %s; "
          "largest |K| per column: %s" % (bands_in_kernel, np.array2string(dist, precision=2), np.array2string(col_max, precision=3)))
    print("inversion_state, Tvib of two gases: chi square %.8g (composition %.8g); update, largest relative difference %.2e"
          % (chi, chi_ref, np.max(np.abs(b.param_vector() - ref.param_vector()) / np.abs(ref.param_vector()))))
    assert np.all(col_max[4:7] > 0) and all(np.any(col_max[q] > 0) for q in (slice(0, 4), slice(7, 10), slice(10, 13)))
    assert np.all(dist <= 1e-11)
    assert np.allclose(chi, chi_ref, rtol=1e-9)
    assert np.allclose(b.param_vector(), ref.param_vector(), rtol=1e-9)
    ch4, hcn = scene.gas("CH4"), scene.gas("HCN")
    assert np.array_equal(ch4.tvib[5], ch4.tvib0[5] + b.sets["tvib:CH4:5"].profile())
    assert np.array_equal(hcn.tvib[1], hcn.tvib0[1] + b.sets["tvib:HCN:1"].profile()) and np.array_equal(hcn.tvib[2], hcn.tvib0[2])


def test_driver_with_one_level_gas_walks_the_loop_of_today(eng, monkeypatch):
    """G.  A BayesSet with the Tvib sets of ONE LevelGas: the driver makes the calls it always made -- LevelFactored.state_jacobian
    with the keywords it always passed, no LevelFactoredSet -- and the chi-square history is bit for bit that of the loop's
    statements written out here from the existing calls (state_weights without the keyword)."""
    from spectrobot_amd import retrieval, spect_main_module as smm
    scene, pixels = _scene(eng)
    z = scene.z
    hcn_nodes, tv_nodes = _nodes(z)
    truth = smm.BayesSet()
    truth.add_set(smm.LinearProfile_1D_new("HCN", z, hcn_nodes, np.full(3, 2.2e-6), np.full(3, 1.1e-6), first_guess_prof=np.full(3, 2.8e-6)))
    retrieval._state_into_gases(scene, truth)
    _observe(scene, pixels, 0.004, np.random.default_rng(6))
    bs = smm.BayesSet(tag="HCN + Tvib of two CH4 levels")
    bs.add_set(retrieval.TvibProfile("CH4", 5, z, tv_nodes, np.full(4, 4.0), first_guess=np.array([1.0, -0.5, 0.7, 0.2])))
    bs.add_set(smm.LinearProfile_1D_new("HCN", z, hcn_nodes, np.full(3, 2.2e-6), np.full(3, 1.1e-6)))
    bs.add_set(retrieval.TvibProfile("CH4", 2, z, tv_nodes[:3], np.full(3, 4.0)))
    seen = []
    real = eng.limb_rays_state_jacobian
    monkeypatch.setattr(retrieval.engine, "limb_rays_state_jacobian", lambda *a, **k: (seen.append(sorted(k)), real(*a, **k))[1])
    monkeypatch.setattr(retrieval.engine, "LevelFactoredSet", lambda *a, **k: pytest.fail("one level gas: no set"))
    chi, _, sims, b = retrieval.inversion_state(scene, copy.deepcopy(bs), pixels, max_it=3)
    monkeypatch.undo()
    today = sorted(["par_gas", "par_w", "tab", "coef_row", "par_level", "par_c", "gas", "grid", "g_lo", "want_rad", "dcoeffs", "par_t"])
    assert len(seen) == len(b.history) >= 2 and all(k == today for k in seen)
    ref = copy.deepcopy(bs)
    pix = sorted(pixels, key=lambda x: x.limb_tg_alt)
    alts = [a for p in pix for a in p.los_alts()]
    retrieval._state_into_gases(scene, ref)
    obs_vec, _, noi_vec = smm.genvec([p.observation for p in pix], [p.observation for p in pix], [p.noise for p in pix], masks=None)
    Sa_inv = np.linalg.inv(np.asarray(ref.VCM_apriori(), dtype=float))
    lowres = lambda r: eng.hires_to_lowres(r, scene.grid, scene.bands_nm, scene.widths_nm, out_units=scene.out_units)
    history = []
    for _ in range(len(b.history)):
        coeffs = scene.coefficient_stack()
        los, alt = scene.los(alts)
        w = scene.state_weights(ref, alt)
        lg = w.level_gas
        rad, jac = lg.lf.state_jacobian(coeffs, los, lg.rows, lg.tvib, w.par_level, w.par_w_lev, par_gas=w.par_gas,
                                        par_w_col=w.par_w_col, gas=w.gas)
        n_par = jac.shape[1]
        both = np.concatenate([lowres(rad)[:, None, :], lowres(jac.view(len(alts) * n_par, -1)).reshape(len(alts), n_par, -1)[:, w.perm]], axis=1)
        fov = smm.fov_closed_form(both[0::3], both[1::3], both[2::3], [p.pixel_rot for p in pix])
        low, dlow = fov[:, 0, :], fov[:, 1:, :]
        for par in ref.params():
            par.set_used()
        sim_vec = low.reshape(-1)
        history.append(np.sum(((obs_vec - sim_vec) / noi_vec) ** 2) / (len(obs_vec) - ref.n_used_par()))
        K = np.transpose(dlow, (1, 0, 2)).reshape(n_par, -1).T
        smm.inversion_algebra_arrays(K, obs_vec, sim_vec, noi_vec, ref, lambda_LM=0.1, L1_reg=False, Sa_inv=Sa_inv)
        retrieval._state_into_gases(scene, ref)
    print("\ninversion_state, one level gas: history %s, written out %s" % (b.history, history))
    assert list(b.history) == history


def test_noise_free_twin_with_the_tvib_of_two_gases(eng):
    """G.  Observations from a perturbed truth -- a bump on the Tvib of HCN level 1 and on the Tvib of CH4 level 5 -- without
    noise: chi square falls over the loop, and the state is nearer to the truth, in units of the a-priori sigma, after the
    loop than before it (the criterion of tests/test_gpu_inversion_state.py's twin; no threshold on either)."""
    from spectrobot_amd import retrieval, spect_main_module as smm
    scene, pixels = _scene(eng)
    z = scene.z
    span = z[-1] - z[0]
    _, tv_nodes = _nodes(z)
    sig = np.full(4, 4.0)
    bump = lambda a: a * np.exp(-0.5 * ((np.array(tv_nodes) - z[0] - 0.45 * span) / (0.25 * span)) ** 2)
    x_true = np.concatenate([bump(5.0), bump(-6.0)])
    truth = smm.BayesSet()
    truth.add_set(retrieval.TvibProfile("HCN", 1, z, tv_nodes, sig, first_guess=x_true[:4]))
    truth.add_set(retrieval.TvibProfile("CH4", 5, z, tv_nodes, sig, first_guess=x_true[4:]))
    retrieval._state_into_gases(scene, truth)
    _observe(scene, pixels, 0.004)
    bs = smm.BayesSet(tag="Tvib of HCN level 1 + Tvib of CH4 level 5")
    bs.add_set(retrieval.TvibProfile("HCN", 1, z, tv_nodes, sig))
    bs.add_set(retrieval.TvibProfile("CH4", 5, z, tv_nodes, sig))
    sigma = np.concatenate([sig, sig])
    before = np.linalg.norm((bs.param_vector() - x_true) / sigma)
    chi, _, sims, b = retrieval.inversion_state(scene, bs, pixels, max_it=10)
    after = np.linalg.norm((b.param_vector() - x_true) / sigma)
    print("\ninversion_state twin, Tvib of two gases: %d iterations (%s), chi square %s; state error in a-priori sigmas %.3f -> %.3f; "
          "retrieved %s, truth %s" % (len(b.history), b.stop, np.array2string(np.array(b.history), precision=4), before, after,
                                      np.array2string(b.param_vector(), precision=3), np.array2string(x_true, precision=3)))
    assert len(b.history) >= 2 and b.history[-1] < b.history[0]
    assert after < before
    assert len(sims) == len(pixels) and b.jacobian.shape == (len(pixels) * len(scene.bands_nm), 8)
