"""Radiance Jacobians for a mixed state vector in one pass (sr_limb_rays_jac_state_dev, engine.limb_rays_state_jacobian,
LevelFactored.state_jacobian): VMR-profile (column) parameters and vibrational-temperature (level) parameters in the
accumulators of one kernel.  The reference has no derivative code: the definition is the build's, checked (A) against
the two existing single-kind calls, (B) against central differences of the whole forward chain, (C) for its argument
checks.  The cases are those of tests/test_gpu_tvib_jacobian.py, with column parameters added to every one."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N_GRID = 24000
LEVELS = (1, 2, 5)                                   # three excited levels: 1311, 1533, 2830 cm-1
NODES = [150.0, 330.0, 510.0, 690.0, 850.0]          # km, nodes of every level's Tvib profile and of every gas's VMR profile
Z_TANS = [130.0, 300.0, 480.0, 650.0]
VMR_CH4, VMR_CO = 0.0148, 3e-4


@pytest.fixture(scope="module")
def eng():
    import torch
    assert torch.cuda.is_available(), "these tests need the GPU"
    from spectrobot_amd import engine
    engine.set_device(0)
    return engine


@pytest.fixture(scope="module")
def scene(eng):
    from spectrobot_amd import synthetic as syn
    grid = syn.make_grid(2990.0, 5e-4, N_GRID)
    L = syn.make_lines(9000, grid, seed=21, n_levels=12, config_id=2)
    atm = syn.make_atmosphere(7, 12)
    atm["nd"] = syn.number_density(atm["press"], atm["temps"])
    ls = eng.LineSet(L, grid, 6, 1, syn.CH4_MM, syn.CH4_LEVEL_ENERGIES)
    Lc = syn.make_lines(700, grid, seed=3, n_levels=0, co_like=True)
    lc = eng.LineSet(Lc, grid, 5, 1, syn.CO_MM, [])
    return dict(grid=grid, atm=atm, ls=ls, lc=lc)


def _level_params(eng, alt_rows, small):
    """par_level, par_w [n_lev, n_rows]: five triangular nodes for each of three levels, a parameter without weights and one
    on the ground level (E = 0): 17; small: the five nodes of one level."""
    W = eng.level_node_weights(NODES, alt_rows)
    if small:
        return np.full(5, LEVELS[2], np.int32), np.array(W)
    lev = [L for L in LEVELS for _ in NODES] + [LEVELS[1], 0]
    w = [W[i] for _ in LEVELS for i in range(len(NODES))] + [np.zeros(len(alt_rows)), W[2]]
    return np.array(lev, np.int32), np.array(w)


def _column_params(eng, alt_pts, n_gas, small):
    """par_gas, par_w [n_col, n_pt]: the five triangular nodes of EVERY gas of the batch at the LOS sample altitudes -- in
    two_gas that includes the level-factored gas itself -- and a parameter without weights (6 or 11); small: three nodes."""
    W = eng.level_node_weights(NODES, alt_pts)
    if small:
        return np.zeros(3, np.int32), np.array(W[1:4])
    gas = [g for g in range(n_gas) for _ in NODES] + [n_gas - 1]
    w = [W[i] for _ in range(n_gas) for i in range(len(NODES))] + [np.zeros(len(alt_pts))]
    # (interleaved: the caller's order is not gas order)
    order = np.argsort([i % len(NODES) for i in range(n_gas * len(NODES))] + [99], kind="stable")
    return np.array(gas, np.int32)[order], np.array(w)[order]


def _build(eng, scene, case):
    """The LOS batch, the level-factored gas's tables and coefficients, the parameters of both kinds of one case."""
    import torch
    from spectrobot_amd import synthetic as syn
    atm, ls, grid = scene["atm"], scene["ls"], scene["grid"]
    z = atm["z"]
    vm = np.full(7, VMR_CH4)
    opts = {}
    if case == "observer":
        opts["LOS_order"] = "observer"
    if case == "solo":
        opts["solo_absorption"] = True
    if case in ("planck", "shard", "solo"):      # (absorption alone of no background is zero: the solo case has one)
        opts["initial_temperature"] = 180.0
    g_lo, g_hi = (5000, 17000) if case == "shard" else (0, N_GRID)
    two = case == "two_gas"
    vmrs = [np.full(7, VMR_CO), vm] if two else [vm]
    scale = [1.0, syn.CH4_ISO_RATIO] if two else [syn.CH4_ISO_RATIO]
    if case == "3d":
        Lr = syn.limb_los_3d(z, atm["nd"], vmrs, Z_TANS[:3], 50.0, 30.0)
        step_row = Lr["seg_alt_layer"].astype(np.int32)        # a coefficient row per LOS step, seven table rows
        po = Lr["pt_off"]
        alt_rows = np.array([Lr["alt"][a:b].mean() for a, b in zip(po[:-1], po[1:])])
        exc = (atm["tvib"] - atm["temps"][None, :])[:, step_row]
        tvib = atm["temps"][step_row][None, :] + exc * (0.4 + 1.2 * np.clip(Lr["seg_mu"], 0.0, 1.0))[None, :]
    else:
        Lr = syn.limb_los(z, atm["nd"], vmrs, Z_TANS)
        step_row = np.arange(7, dtype=np.int32)
        alt_rows = z
        tvib = atm["tvib"].copy()
    los = eng.LimbLOS(Lr["seg_off"], Lr["seg_layer"], Lr["pt_off"], Lr["x"], Lr["nd"], Lr["vmr"], col_scale=scale, **opts)
    lf = eng.LevelFactored(ls, atm["temps"], atm["press"], g_lo=g_lo, g_hi=g_hi)
    co = lf.steps(step_row, tvib=tvib)
    gas = 0
    if two:
        gas = 1
        c0 = scene["lc"].abscoeff_layers(atm["temps"], atm["press"])
        co = (torch.stack([c0[0], co[0]]).contiguous(), torch.stack([c0[1], co[1]]).contiguous())
    small = case == "np_small"                  # 3 + 5 = 8 parameters: the kernel's other block size
    par_level, par_w_lev = _level_params(eng, alt_rows, small)
    par_gas, par_w_col = _column_params(eng, Lr["alt"], 2 if two else 1, small)
    return dict(los=los, lf=lf, co=co, gas=gas, step_row=step_row, tvib=tvib, par_level=par_level, par_w_lev=par_w_lev,
                par_gas=par_gas, par_w_col=par_w_col, g_lo=g_lo, grid=grid, n_gas=2 if two else 1, Lr=Lr, opts=opts, scale=scale)


def _row_err(a, ref):
    """max |a - ref| of every (ray, parameter) row, scaled by the row's largest |ref| (rows of zeros: absolute)."""
    s = ref.abs().amax(dim=-1)
    s = s.masked_fill(s == 0, 1.0)
    return (a - ref).abs().amax(dim=-1) / s


def _state(b, col=True, lev=True, **kw):
    none = np.zeros(0, np.int32)
    return b["lf"].state_jacobian(b["co"], b["los"], b["step_row"], b["tvib"], b["par_level"] if lev else none,
                                  b["par_w_lev"] if lev else np.zeros((0, len(b["step_row"]))),
                                  par_gas=b["par_gas"] if col else None, par_w_col=b["par_w_col"] if col else None,
                                  gas=b["gas"], grid=b["grid"], **kw)


def _solo_closed_form_columns(eng, b, rad):
    """Without a source term I = I_0 exp(-sum_s tau_s), so d I / d x_p = -I sum_s abs_g[r_s] D[p][s] for a column parameter
    of gas g: products and one short sum, no cancellation (the closed form of tests/test_gpu_tvib_jacobian.py for the other
    kind of parameter)."""
    import torch
    los, Lr = b["los"], b["Lr"]
    a = eng._gas_stack(b["co"])[0]
    out = torch.zeros((los.n_rays, len(b["par_gas"]), a.shape[2]), dtype=torch.float64, device="cuda")
    for p, g in enumerate(b["par_gas"]):
        D = eng.LimbLOS(Lr["seg_off"], Lr["seg_layer"], Lr["pt_off"], Lr["x"], Lr["nd"], b["par_w_col"][p][None],
                        col_scale=[b["scale"][g]]).columns()[0]
        for r in range(los.n_rays):
            sg = slice(los.seg_off[r], los.seg_off[r + 1])
            rows = torch.as_tensor(np.asarray(los.seg_layer[sg], np.int64), device="cuda")
            out[r, p] = -rad[r] * (torch.as_tensor(D[sg], device="cuda") @ a[g][rows])
    return out


CASES = ["1d", "3d", "observer", "solo", "planck", "two_gas", "shard", "np_small"]


@pytest.mark.parametrize("case", CASES)
def test_equals_the_two_existing_calls(eng, scene, case):
    """A.  The column rows against engine.limb_rays_jacobian -- with the forward-sensitivity kernel (set_jac_layer_mode(1):
    the arithmetic of the new kernel's column slots) and with the default route (0: the folded or the one-pass kernel,
    another order of summation); their spread is printed and the new rows must lie within max(1e-12, 4 x spread) of
    either --, the level rows against LevelFactored.tvib_jacobian within 1e-12 of a row (the same arithmetic in the same
    order).  Rows that must be zero -- a parameter without weights, the ground level, nodes out of a ray's reach -- are
    exactly zero; the radiances are those of limb_rays; a call with only one kind of parameter equals that kind's call.
    Under solo_absorption the column rows are held to a closed form instead of the one-pass route (see
    tests/test_gpu_tvib_jacobian.py for what that route leaves in rows of zeros).
    The test prints, per case, the spread of the two column references, the distance of the column rows to each and of
    the level rows to tvib_jacobian; figures from an MI355X run have not been recorded here yet."""
    import torch
    b = _build(eng, scene, case)
    lf, los = b["lf"], b["los"]
    n_col, n_lev = len(b["par_gas"]), len(b["par_level"])
    try:
        eng.set_jac_layer_mode(1)
        rad_f, ref_f = eng.limb_rays_jacobian(b["co"], los, b["par_gas"], b["par_w_col"], grid=b["grid"], g_lo=b["g_lo"])
        torch.cuda.synchronize()
    finally:
        eng.set_jac_layer_mode(0)
    _, ref_o = eng.limb_rays_jacobian(b["co"], los, b["par_gas"], b["par_w_col"], grid=b["grid"], g_lo=b["g_lo"])
    _, ref_l = lf.tvib_jacobian(b["co"], los, b["step_row"], b["tvib"], b["par_level"], b["par_w_lev"], gas=b["gas"],
                                grid=b["grid"])
    rad, jac = _state(b)
    assert tuple(jac.shape) == (los.n_rays, n_col + n_lev, lf.tab.shape[3]) and torch.isfinite(jac).all()
    jc, jl = jac[:, :n_col], jac[:, n_col:]
    spread = float(_row_err(ref_f, ref_o).max())
    tol = max(1e-12, 4.0 * spread)
    err_f, err_o = float(_row_err(jc, ref_f).max()), float(_row_err(jc, ref_o).max())
    err_c, err_l = min(err_f, err_o), float(_row_err(jl, ref_l).max())
    print("state jacobian [%s]: %d column + %d level parameters; column references forward vs default route %.2e; column "
          "rows vs forward %.2e, vs default %.2e (bound %.2e); level rows vs tvib_jacobian %.2e (bound 1e-12)"
          % (case, n_col, n_lev, spread, err_f, err_o, tol, err_l))
    assert float(ref_f.abs().max()) > 0 and float(ref_l.abs().max()) > 0
    assert float(torch.minimum(_row_err(jc, ref_f), _row_err(jc, ref_o)).max()) <= tol
    assert err_l <= 1e-12
    if case == "solo":
        closed = _solo_closed_form_columns(eng, b, rad)
        print("state jacobian [solo]: column rows vs the closed form %.2e, forward reference vs the closed form %.2e, default "
              "route vs the closed form %.2e" % (float(_row_err(jc, closed).max()), float(_row_err(ref_f, closed).max()),
                                                 float(_row_err(ref_o, closed).max())))
        assert float(_row_err(jc, closed).max()) <= 1e-12
        assert err_f <= 1e-12
    # rows of exact zeros
    zero_c, zero_l = ref_f.abs().amax(dim=-1) == 0, ref_l.abs().amax(dim=-1) == 0
    assert bool((jc.abs().amax(dim=-1)[zero_c] == 0).all()) and bool((jl.abs().amax(dim=-1)[zero_l] == 0).all())
    if case != "np_small":
        no_w = int(np.nonzero(np.abs(b["par_w_col"]).sum(axis=1) == 0)[0][0])
        assert bool(zero_c[:, no_w].all()) and bool(zero_l[:, -2:].all())          # no weights; no weights, ground level
        assert bool(zero_c[:, :no_w].any()) and not bool(zero_c[:, :no_w].all())    # nodes out of a ray's reach
    # the radiances: the same recursion on the same inputs
    r0 = eng.limb_rays(b["co"], los, grid=b["grid"], g_lo=b["g_lo"])
    d_rad = float((rad - r0).abs().max() / r0.abs().max())
    assert d_rad < 1e-13
    # one kind only
    r_c, j_c = _state(b, lev=False)
    r_l, j_l = _state(b, col=False, want_rad=False)
    assert r_l is None and tuple(j_c.shape) == tuple(ref_f.shape) and tuple(j_l.shape) == tuple(ref_l.shape)
    only_c = float(torch.minimum(_row_err(j_c, ref_f), _row_err(j_c, ref_o)).max())
    only_l = float(_row_err(j_l, ref_l).max())
    print("state jacobian [%s]: radiances vs limb_rays %.2e; only column parameters vs the nearer reference %.2e, only level "
          "parameters vs tvib_jacobian %.2e" % (case, d_rad, only_c, only_l))
    assert only_c <= tol and only_l <= 1e-12
    assert float((r_c - r0).abs().max() / r0.abs().max()) < 1e-13
    assert bool((j_c.abs().amax(dim=-1)[zero_c] == 0).all()) and bool((j_l.abs().amax(dim=-1)[zero_l] == 0).all())


def test_central_differences_of_the_forward_chain(eng, scene):
    """B.  The best-seen parameter of each kind (max|jac| / max|rad|) against central differences of the whole forward
    chain at h and h / 2: lf.steps -> limb_rays in Tvib (h = 0.1 K), a new batch -> limb_rays in a VMR node (h = 1e-3 of its
    value).  |jac - FD(h/2)| <= 2 |FD(h) - FD(h/2)| + 1e-9 max|jac| per ray in the max norm, and |FD(h) - FD(h/2)| < 1e-3
    max|jac| so that the bound cannot go slack.  The test prints both figures per parameter; figures from an MI355X run
    have not been recorded here yet (should a chosen parameter leave the second condition, the parameter or the node
    placement is what changes, not the condition)."""
    import torch
    b = _build(eng, scene, "1d")
    lf, los, Lr = b["lf"], b["los"], b["Lr"]
    n_col = len(b["par_gas"])
    rad, jac = _state(b)
    seen = (jac.abs().amax(dim=(0, 2)) / rad.abs().max()).cpu().numpy()
    print("state jacobian FD: max|jac| / max|rad| per unit of every parameter:", np.array2string(seen, precision=2))
    p_col, p_lev = int(np.argmax(seen[:n_col])), n_col + int(np.argmax(seen[n_col:]))

    def fd_lev(p, h):
        out = []
        for sgn in (1.0, -1.0):
            tv = b["tvib"].copy()
            tv[b["par_level"][p - n_col]] += sgn * h * b["par_w_lev"][p - n_col]
            out.append(eng.limb_rays(lf.steps(b["step_row"], tvib=tv), los).clone())
        return (out[0] - out[1]) / (2.0 * h)

    def fd_col(p, h):
        out = []
        for sgn in (1.0, -1.0):
            vmr = np.array(Lr["vmr"], dtype=float)
            vmr[b["par_gas"][p]] += sgn * h * b["par_w_col"][p]
            l2 = eng.LimbLOS(Lr["seg_off"], Lr["seg_layer"], Lr["pt_off"], Lr["x"], Lr["nd"], vmr, col_scale=b["scale"])
            out.append(eng.limb_rays(b["co"], l2, resident=False).clone())
        return (out[0] - out[1]) / (2.0 * h)

    for kind, p, fd, h in (("VMR node", p_col, fd_col, 1e-3 * VMR_CH4), ("Tvib node", p_lev, fd_lev, 0.1)):
        f1, f2 = fd(p, h), fd(p, 0.5 * h)
        jm = float(jac[:, p].abs().max())
        trunc = (f1 - f2).abs().amax(dim=-1)
        err = (jac[:, p] - f2).abs().amax(dim=-1)
        print("state jacobian FD: %s, parameter %d: max|jac| / max|rad| %.2e, h %.3g, |jac - FD(h/2)| / max|jac| %.2e, "
              "|FD(h) - FD(h/2)| / max|jac| %.2e" % (kind, p, seen[p], h, float(err.max()) / jm, float(trunc.max()) / jm))
        assert float(trunc.max()) < 1e-3 * jm
        assert bool((err <= 2.0 * trunc + 1e-9 * jm).all())


def test_refused_arguments_leave_the_output_untouched(eng, scene):
    """C.  Every refused argument returns its status before anything is copied or launched (rad and jac keep their
    sentinel), and a valid call afterwards on the same stream reproduces the earlier result bit for bit."""
    import torch
    from spectrobot_amd import _lib
    b = _build(eng, scene, "two_gas")
    lf, los = b["lf"], b["los"]
    a, e = eng._gas_stack(b["co"])
    n_gas, n_layers, n_pts = a.shape
    n_levels, n_rows = lf.tab.shape[0], lf.tab.shape[2]
    dpop = lf.ls.level_populations_dtvib(lf.temps[b["step_row"]], b["tvib"])
    par_c = np.ascontiguousarray(b["par_w_lev"] * dpop.T[b["par_level"]])
    par_w = np.ascontiguousarray(b["par_w_col"])
    n_col, n_lev = len(b["par_gas"]), len(b["par_level"])
    good_rad, good = eng.limb_rays_state_jacobian(b["co"], los, b["par_gas"], par_w, lf.tab, b["step_row"], b["par_level"],
                                                  par_c, gas=b["gas"])
    again_rad, again = _state(b)
    assert torch.equal(again, good) and torch.equal(again_rad, good_rad)       # the method is the call with par_c formed
    torch.cuda.synchronize()
    jac = torch.full((los.n_rays, n_col + n_lev, n_pts), 7.25, dtype=torch.float64, device="cuda")
    rad = torch.full((los.n_rays, n_pts), 7.25, dtype=torch.float64, device="cuda")
    ip_, dp_ = _lib.ip, _lib.dp
    ptr = lambda t: C.c_void_p(t.data_ptr())

    def call(**kw):
        d = los.desc()
        if "init_mode" in kw:
            d.init_mode = kw["init_mode"]
        row = np.ascontiguousarray(kw.get("coef_row", b["step_row"]), dtype=np.int32)
        lev = np.ascontiguousarray(kw.get("par_level", b["par_level"]), dtype=np.int32)
        pg = np.ascontiguousarray(kw.get("par_gas", b["par_gas"]), dtype=np.int32)
        return _lib.lib.sr_limb_rays_jac_state_dev(
            ptr(a), ptr(e), n_layers, kw.get("n_pts", n_pts), C.byref(d), kw.get("n_col", n_col), pg.ctypes.data_as(ip_),
            par_w.ctypes.data_as(dp_), kw.get("gas", b["gas"]), None if kw.get("no_tab") else ptr(lf.tab),
            kw.get("n_levels", n_levels), n_rows, row.ctypes.data_as(ip_), kw.get("n_lev", n_lev), lev.ctypes.data_as(ip_),
            par_c.ctypes.data_as(dp_), ptr(rad), None if kw.get("no_jac") else ptr(jac), eng._stream_ptr())

    bad_row_lo, bad_row_hi = b["step_row"].copy(), b["step_row"].copy()
    bad_row_lo[3], bad_row_hi[6] = -1, n_rows
    bad_lev_lo, bad_lev_hi = b["par_level"].copy(), b["par_level"].copy()
    bad_lev_lo[0], bad_lev_hi[-1] = -1, n_levels
    bad_gas_lo, bad_gas_hi = b["par_gas"].copy(), b["par_gas"].copy()
    bad_gas_lo[2], bad_gas_hi[-1] = -1, n_gas
    refused = [(dict(gas=-1), _lib.SR_ERR_ARG), (dict(gas=n_gas), _lib.SR_ERR_ARG),
               (dict(coef_row=bad_row_lo), _lib.SR_ERR_ARG), (dict(coef_row=bad_row_hi), _lib.SR_ERR_ARG),
               (dict(par_level=bad_lev_lo), _lib.SR_ERR_ARG), (dict(par_level=bad_lev_hi), _lib.SR_ERR_ARG),
               (dict(par_gas=bad_gas_lo), _lib.SR_ERR_ARG), (dict(par_gas=bad_gas_hi), _lib.SR_ERR_ARG),
               (dict(no_jac=True), _lib.SR_ERR_ARG), (dict(no_tab=True), _lib.SR_ERR_ARG),
               (dict(n_col=0, n_lev=0), _lib.SR_ERR_ARG), (dict(n_lev=-2), _lib.SR_ERR_ARG),
               (dict(init_mode=1), _lib.SR_ERR_ARG), (dict(n_pts=2000001), _lib.SR_ERR_LIMIT)]
    for kw, status in refused:
        assert call(**kw) == status, kw
        torch.cuda.synchronize()
        assert bool((jac == 7.25).all()) and bool((rad == 7.25).all()), kw
    assert call() == _lib.SR_OK
    torch.cuda.synchronize()
    assert torch.equal(jac, good) and torch.equal(rad, good_rad)
    # the wrappers' own checks
    with pytest.raises(ValueError):
        eng.limb_rays_state_jacobian(b["co"], los)                                                    # no parameters
    with pytest.raises(ValueError):
        eng.limb_rays_state_jacobian(b["co"], los, b["par_gas"], par_w[:, :-1])
    with pytest.raises(ValueError):
        eng.limb_rays_state_jacobian(b["co"], los, par_level=b["par_level"], par_c=par_c)             # no tables
    with pytest.raises(ValueError):
        eng.limb_rays_state_jacobian(b["co"], los, tab=lf.tab, coef_row=b["step_row"], par_level=b["par_level"][:4], par_c=par_c)
    with pytest.raises(ValueError):
        lf.state_jacobian(b["co"], los, b["step_row"], b["tvib"], b["par_level"], b["par_w_lev"][:, :5])
    with pytest.raises(RuntimeError):
        eng.limb_rays_state_jacobian(b["co"], los, tab=lf.tab, coef_row=bad_row_hi, par_level=b["par_level"], par_c=par_c)


def _synthetic(n_gas, n_par):
    """Synthetic inputs at the smallest shapes at which the level / state kernel's indexing can go wrong: 300 points (two
    point blocks, the last wave straddles the end), 6 coefficient rows on 4 table rows, 3 levels, 3 rays of 1, 4 and 7
    segments of two sample points each; parameter 1 has no coefficients at all, a fifth of the others are zero."""
    import torch
    n_pts, n_layers, n_levels, n_rows = 300, 6, 3, 4
    rng = np.random.default_rng(100 * n_gas + n_par)
    seg_off = np.array([0, 1, 5, 12], np.int32)
    seg_layer = np.array([3, 5, 4, 3, 4, 0, 1, 2, 5, 2, 1, 0], np.int32)
    n_seg = seg_layer.size
    pt_off = 2 * np.arange(n_seg + 1, dtype=np.int32)
    x = (np.arange(n_seg)[:, None] + np.array([0.0, 1.0]) * rng.uniform(0.5, 1.0, (n_seg, 1))).reshape(-1)
    nd = (rng.uniform(0.5, 2.0, (n_seg, 1)) * np.array([1.0, 0.8])).reshape(-1)   # (a Curtis-Godson column needs nd to vary)
    vmr = rng.uniform(0.2, 0.8, (n_gas, 2 * n_seg))
    cuda = lambda v: torch.as_tensor(np.ascontiguousarray(v), device="cuda")
    co = (cuda(np.exp(rng.uniform(np.log(1e-4), np.log(3.0), (n_gas, n_layers, n_pts)))),   # optically thin to thick
          cuda(rng.uniform(0.1, 1.0, (n_gas, n_layers, n_pts))))
    tab = cuda(rng.uniform(0.1, 1.0, (n_levels, 2, n_rows, n_pts)))
    par_c = rng.uniform(-1.0, 1.0, (n_par, n_layers)) * (rng.uniform(size=(n_par, n_layers)) > 0.2)
    par_c[1] = 0.0
    par_c[0, 3] = 0.7        # (every ray meets a non-zero coefficient: row 3 is the single-segment ray's)
    return dict(seg_off=seg_off, seg_layer=seg_layer, pt_off=pt_off, x=x, nd=nd, vmr=vmr, co=co, tab=tab,
                coef_row=np.array([0, 2, 1, 3, 3, 0], np.int32), par_level=rng.integers(0, n_levels, n_par).astype(np.int32),
                par_c=par_c, gas=n_gas - 1)


@pytest.mark.parametrize("n_par", [3, 17])
@pytest.mark.parametrize("n_gas", [1, 2, 3, 4])
def test_level_call_equals_state_call_without_columns(eng, n_gas, n_par):
    """D.  sr_limb_rays_jac_level_dev and sr_limb_rays_jac_state_dev with level parameters only run the two instances of one
    kernel (without and with the column code) on the same plan: every row agrees within 1e-12 of the row, the radiances of
    both equal limb_rays within 1e-13, a parameter whose coefficients are all zero has rows of exact zeros.  n_par = 3: eight
    accumulators, one block; 17: sixteen accumulators, two blocks, the second nearly empty.  The operations and their order
    are the same, so bit-for-bit equality is expected; the test prints whether it holds (what an MI355X run printed has
    not been recorded here yet)."""
    import torch
    s = _synthetic(n_gas, n_par)
    los = eng.LimbLOS(s["seg_off"], s["seg_layer"], s["pt_off"], s["x"], s["nd"], s["vmr"])
    rad_l, jac_l = eng.limb_rays_level_jacobian(s["co"], los, s["tab"], s["coef_row"], s["par_level"], s["par_c"], gas=s["gas"])
    rad_s, jac_s = eng.limb_rays_state_jacobian(s["co"], los, tab=s["tab"], coef_row=s["coef_row"], par_level=s["par_level"],
                                                par_c=s["par_c"], gas=s["gas"])
    r0 = eng.limb_rays(s["co"], los)
    assert tuple(jac_l.shape) == tuple(jac_s.shape) == (3, n_par, 300)
    assert torch.isfinite(jac_l).all() and torch.isfinite(jac_s).all()
    err = float(_row_err(jac_s, jac_l).max())
    d_l, d_s = (float((r - r0).abs().max() / r0.abs().max()) for r in (rad_l, rad_s))
    print("level vs state call [n_gas %d, n_par %d]: rows %.2e (bound 1e-12), bit for bit %s; radiances vs limb_rays: level "
          "call %.2e, state call %.2e (bound 1e-13), bit for bit %s / %s, level vs state radiances bit for bit %s"
          % (n_gas, n_par, err, torch.equal(jac_s, jac_l), d_l, d_s, torch.equal(rad_l, r0), torch.equal(rad_s, r0),
             torch.equal(rad_l, rad_s)))
    assert err <= 1e-12
    assert d_l < 1e-13 and d_s < 1e-13
    live = jac_l.abs().amax(dim=-1) > 0
    assert bool(live[:, 0].all()) and bool(live.sum() > 3)                      # every ray is seen by parameter 0
    assert bool((jac_l[:, 1] == 0).all()) and bool((jac_s[:, 1] == 0).all())    # no coefficients: exact zeros
