"""Vibrational-temperature Jacobians of limb radiances from the level tables (sr_limb_rays_jac_level_dev,
engine.limb_rays_level_jacobian, LevelFactored.tvib_jacobian).  The reference has no derivative code: the definition is
the build's, checked (A) against a composition of existing ops that is the same linear functional, (B) against central
differences of the whole forward chain in Tvib, (D) for its argument checks."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N_GRID = 24000
LEVELS = (1, 2, 5)                                   # three excited levels: 1311, 1533, 2830 cm-1
NODES = [150.0, 330.0, 510.0, 690.0, 850.0]          # km, nodes of every level's Tvib profile
Z_TANS = [130.0, 300.0, 480.0, 650.0]


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


def _params(eng, alt_rows, extra=True):
    """par_level [n_par], par_w [n_par, n_rows]: five triangular nodes for each of the three levels (15), then -- extra --
    a parameter whose weights are all zero and one on the ground level (E = 0): 17 = 16 + 1 parameters."""
    W = eng.level_node_weights(NODES, alt_rows)
    lev = [L for L in LEVELS for _ in NODES]
    w = [W[i] for _ in LEVELS for i in range(len(NODES))]
    if extra:
        lev += [LEVELS[1], 0]
        w += [np.zeros(len(alt_rows)), W[2]]
    return np.array(lev, np.int32), np.array(w)


def _build(eng, scene, case):
    """The LOS batch, the level-factored gas's tables and coefficients, the parameters of one case."""
    import torch
    from spectrobot_amd import synthetic as syn
    atm, ls, grid = scene["atm"], scene["ls"], scene["grid"]
    z = atm["z"]
    vm = np.full(7, 0.0148)
    opts = {}
    if case == "observer":
        opts["LOS_order"] = "observer"
    if case == "solo":
        opts["solo_absorption"] = True
    if case in ("planck", "shard", "solo"):      # (absorption alone of no background is zero: the solo case has one)
        opts["initial_temperature"] = 180.0
    g_lo, g_hi = (5000, 17000) if case == "shard" else (0, N_GRID)
    two = case == "two_gas"
    vmrs = [np.full(7, 3e-4), vm] if two else [vm]
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
    assert len(step_row) > len(np.unique(step_row)) or case != "3d"
    los = eng.LimbLOS(Lr["seg_off"], Lr["seg_layer"], Lr["pt_off"], Lr["x"], Lr["nd"], Lr["vmr"], col_scale=scale, **opts)
    lf = eng.LevelFactored(ls, atm["temps"], atm["press"], g_lo=g_lo, g_hi=g_hi)
    co = lf.steps(step_row, tvib=tvib)
    gas = 0
    if two:
        gas = 1
        c0 = scene["lc"].abscoeff_layers(atm["temps"], atm["press"])
        co = (torch.stack([c0[0], co[0]]).contiguous(), torch.stack([c0[1], co[1]]).contiguous())
    par_level, par_w = _params(eng, alt_rows)
    if case == "np_small":      # 9 = 8 + 1 parameters: the kernel's other block size
        par_level, par_w = par_level[:9], par_w[:9]
    return dict(los=los, lf=lf, co=co, gas=gas, step_row=step_row, tvib=tvib, par_level=par_level, par_w=par_w,
                g_lo=g_lo, grid=grid, n_gas=2 if two else 1)


def _composition(eng, b):
    """ref [n_rays, n_par, n_pts] from existing ops: per level the derivative coefficients by glevel_combine on the
    one-hot d pop / d Tvib, the per-row Jacobian by limb_rays_jacobians, contracted with the parameters' weights."""
    import torch
    lf, los = b["lf"], b["los"]
    dpop = lf.ls.level_populations_dtvib(lf.temps[b["step_row"]], b["tvib"])
    n_par = len(b["par_level"])
    ref = torch.zeros((los.n_rays, n_par, lf.tab.shape[3]), dtype=torch.float64, device="cuda")
    for L in np.unique(b["par_level"]):
        oh = np.zeros_like(dpop)
        oh[:, L] = dpop[:, L]
        da, de = eng.glevel_combine(lf.tab, b["step_row"], oh)
        if b["n_gas"] == 2:
            da = torch.stack([torch.zeros_like(da), da]).contiguous()
            de = torch.stack([torch.zeros_like(de), de]).contiguous()
        jl = eng.limb_rays_jacobians(b["co"], los, dcoeffs=(da, de), grid=b["grid"], g_lo=b["g_lo"], want_rad=False)[1]
        for p in np.nonzero(b["par_level"] == L)[0]:
            w = torch.as_tensor(b["par_w"][p], dtype=torch.float64, device="cuda")
            ref[:, p] = torch.einsum("k,rkn->rn", w, jl)
    return ref


def _row_err(a, ref):
    """max |a - ref| of every (ray, parameter) row, scaled by the row's largest |ref| (rows of zeros: absolute)."""
    s = ref.abs().amax(dim=-1)
    s = s.masked_fill(s == 0, 1.0)
    return (a - ref).abs().amax(dim=-1) / s


CASES = ["1d", "3d", "observer", "solo", "planck", "two_gas", "shard", "np_small"]


@pytest.mark.parametrize("case", CASES)
def test_equals_the_composition_of_existing_ops(eng, scene, case):
    """A.  The new call against glevel_combine (one-hot d pop / d Tvib of a level) -> limb_rays_jacobians (per-row
    Jacobian) -> contraction with the weights: the same linear functional, another order of summation.  The
    composition is run with the forward-sensitivity kernels and with the one-pass kernels; their spread is printed and
    the new kernel must lie within max(1e-12, 4 x spread) of either.  Rows that must be zero are exactly zero.
    Measured on the MI355X (spread of the composition / distance of the new kernel to the nearer one):
    1d 6.9e-16 / 5.2e-16, 3d 4.3e-16 / 6.1e-16, observer 6.9e-16 / 5.4e-16, planck 6.6e-16 / 5.4e-16, two_gas 8.2e-16 / 5.4e-16,
    shard 8.6e-16 / 5.7e-16, np_small 6.6e-16 / 4.9e-16; solo (absorption of a Planck background) 1.0 / 4.1e-16: see the
    note in the body (a closed form decides there: 5.1e-16)."""
    import torch
    b = _build(eng, scene, case)
    lf, los = b["lf"], b["los"]
    try:
        eng.set_jac_layer_mode(1)
        ref_f = _composition(eng, b)
        torch.cuda.synchronize()
    finally:
        eng.set_jac_layer_mode(0)
    ref_o = _composition(eng, b)
    rad, jac = lf.tvib_jacobian(b["co"], los, b["step_row"], b["tvib"], b["par_level"], b["par_w"], gas=b["gas"],
                                grid=b["grid"])
    assert tuple(jac.shape) == (los.n_rays, len(b["par_level"]), lf.tab.shape[3])
    spread = float(_row_err(ref_f, ref_o).max())
    err = float(torch.minimum(_row_err(jac, ref_f), _row_err(jac, ref_o)).max())
    tol = max(1e-12, 4.0 * spread)
    print("tvib jacobian [%s]: new kernel vs the forward composition %.2e, vs the one-pass composition %.2e; largest "
          "|forward| %.3e, |one-pass| %.3e, |new| %.3e" % (case, float(_row_err(jac, ref_f).max()), float(_row_err(jac, ref_o).max()),
                                                     float(ref_f.abs().max()), float(ref_o.abs().max()), float(jac.abs().max())))
    print("tvib jacobian [%s]: composition forward vs one-pass %.2e, new kernel vs the nearer %.2e (bound %.2e), %d "
          "parameters, %d coefficient rows" % (case, spread, err, tol, len(b["par_level"]), len(b["step_row"])))
    assert float(ref_o.abs().max()) > 0 and torch.isfinite(jac).all()
    assert err <= tol
    if case == "solo":
        # Here the composition's own two routes differ by 1.0 of a row (measured), so the bound above is slack.  Both
        # equal the closed form below (forward route 4.9e-16, one-pass route 3.8e-15 of a row, rows of zeros taken
        # absolutely): the difference sits in rows whose value is zero, which the one-pass route of limb_rays_jacobians
        # leaves tiny but not exactly zero under solo_absorption -- existing behaviour, not this feature's.  Without a
        # source term the radiance is closed-form, I = I_0 exp(-sum_s tau_s), and so is the derivative:
        # d I / d x_p = -I sum_s u_s c[p][r_s] A_lev[p][row[r_s]] -- products and one short sum, no cancellation: the new
        # kernel is held to 1e-12 of a row of it (measured 5.1e-16), and of the forward-sensitivity route.
        col = eng.LimbLOS(los.seg_off, los.seg_layer, los.pt_off, los.x, los.nd, los.vmr, col_scale=los.col_scale).columns()[0]
        colsum = np.zeros((los.n_rays, len(b["step_row"])))
        for r in range(los.n_rays):
            for sg in range(los.seg_off[r], los.seg_off[r + 1]):
                colsum[r, los.seg_layer[sg]] += col[sg]
        dpop = lf.ls.level_populations_dtvib(lf.temps[b["step_row"]], b["tvib"])
        m = torch.as_tensor(colsum[:, None, :] * (b["par_w"] * dpop.T[b["par_level"]])[None], device="cuda")
        A = lf.tab[torch.as_tensor(b["par_level"].astype(np.int64), device="cuda"), 0][:, torch.as_tensor(b["step_row"].astype(np.int64), device="cuda")]
        closed = -rad[:, None, :] * torch.einsum("rpk,pkn->rpn", m, A)
        print("tvib jacobian [solo]: new kernel vs the closed form %.2e, forward composition vs the closed form %.2e, "
              "one-pass composition vs the closed form %.2e" % (float(_row_err(jac, closed).max()),
                                                              float(_row_err(ref_f, closed).max()), float(_row_err(ref_o, closed).max())))
        assert float(_row_err(jac, closed).max()) <= 1e-12
        assert float(_row_err(jac, ref_f).max()) <= 1e-12
    # rows of exact zeros: the parameter without weights, the one on the ground level (E = 0), rays above a node's reach
    zero = ref_o.abs().amax(dim=-1) == 0
    assert bool((jac.abs().amax(dim=-1)[zero] == 0).all())
    if case != "np_small":
        assert bool(zero[:, -2:].all()) and not bool(zero[:, :15].all())
    # the radiances: the same recursion on the same inputs
    r0 = eng.limb_rays(b["co"], los, grid=b["grid"], g_lo=b["g_lo"])
    assert float((rad - r0).abs().max() / r0.abs().max()) < 1e-13
    # the thin wrapper with the populations themselves as the variable (c = w) and without radiances
    if case == "1d":
        pw = b["par_w"][:5]
        r1, j1 = eng.limb_rays_level_jacobian(b["co"], los, lf.tab, b["step_row"], b["par_level"][:5], pw, want_rad=False)
        assert r1 is None
        dpop = lf.ls.level_populations_dtvib(lf.temps[b["step_row"]], b["tvib"])
        # node weights of level 1 times a constant per row: d/dpop scaled row-wise is d/dTvib only where one row is
        # touched; compare through linearity instead: sum_p of the five population Jacobians = all rows moved by 1
        oh = np.zeros_like(dpop)
        oh[:, LEVELS[0]] = pw.sum(axis=0)
        da, de = eng.glevel_combine(lf.tab, b["step_row"], oh)
        jl = eng.limb_rays_jacobians(b["co"], los, dcoeffs=(da, de), want_rad=False)[1]
        assert float(_row_err(j1.sum(dim=1), jl.sum(dim=1)).max()) < tol


def test_central_differences_of_the_forward_chain(eng, scene):
    """B.  Two parameters against central differences of lf.steps -> limb_rays in Tvib at h = 0.1 K and 0.05 K.  The
    quotient's own error is its truncation, estimated by the two step sizes:
    |jac - FD(0.05)| <= 2 |FD(0.1) - FD(0.05)| + 1e-9 max|jac| per ray in the max norm, and |FD(0.1) - FD(0.05)| <
    1e-3 max|jac| so that the bound cannot go slack.  The parameters are the two the rays see best (max|jac| >= 1e-3
    max|rad| per K, so the 1e-9 floor is above the quotient's roundoff).  This pins c2 E / Tvib^2 and the absence of a Q
    term, which the composition shares with the kernel.
    Measured on the MI355X: parameters 14 and 13 (level 5, nodes 850 and 690 km), max|jac| / max|rad| 7.9e-3 and
    7.0e-3 per K, |jac - FD(0.05)| / max|jac| 1.4e-6 and 1.0e-6, |FD(0.1) - FD(0.05)| / max|jac| 4.3e-6 and 3.1e-6 (a third
    of it is the finer quotient's own error, as an h^2 truncation gives)."""
    import torch
    b = _build(eng, scene, "1d")
    lf, los = b["lf"], b["los"]
    rad, jac = lf.tvib_jacobian(b["co"], los, b["step_row"], b["tvib"], b["par_level"], b["par_w"])
    seen = (jac.abs().amax(dim=(0, 2)) / rad.abs().max()).cpu().numpy()
    picks = np.argsort(seen)[::-1][:2]
    print("tvib jacobian FD: max|jac| / max|rad| per K of every parameter:", np.array2string(seen, precision=2))

    def fd(p, h):
        out = []
        for sgn in (1.0, -1.0):
            tv = b["tvib"].copy()
            tv[b["par_level"][p]] += sgn * h * b["par_w"][p]
            out.append(eng.limb_rays(lf.steps(b["step_row"], tvib=tv), los).clone())
        return (out[0] - out[1]) / (2.0 * h)

    for p in picks:
        assert seen[p] >= 1e-3, "the rays barely see parameter %d" % p
        f1, f2 = fd(p, 0.1), fd(p, 0.05)
        jm = float(jac[:, p].abs().max())
        trunc = (f1 - f2).abs().amax(dim=-1)
        err = (jac[:, p] - f2).abs().amax(dim=-1)
        print("tvib jacobian FD: parameter %d (level %d): max|jac| / max|rad| %.2e per K, |jac - FD(0.05)| / max|jac| %.2e, "
              "|FD(0.1) - FD(0.05)| / max|jac| %.2e" % (p, b["par_level"][p], seen[p], float(err.max()) / jm,
                                                          float(trunc.max()) / jm))
        assert float(trunc.max()) < 1e-3 * jm
        assert bool((err <= 2.0 * trunc + 1e-9 * jm).all())


def test_refused_arguments_leave_the_output_untouched(eng, scene):
    """D.  Every refused argument returns its status before anything is copied or launched (the Jacobian buffer keeps
    its sentinel), and a valid call afterwards on the same stream gives the result of before."""
    import torch
    from spectrobot_amd import _lib
    b = _build(eng, scene, "1d")
    lf, los = b["lf"], b["los"]
    a, e = eng._gas_stack(b["co"])
    n_gas, n_layers, n_pts = a.shape
    n_lev, n_rows = lf.tab.shape[0], lf.tab.shape[2]
    dpop = lf.ls.level_populations_dtvib(lf.temps[b["step_row"]], b["tvib"])
    par_c = np.ascontiguousarray(b["par_w"] * dpop.T[b["par_level"]])
    n_par = len(b["par_level"])
    good_rad, good = eng.limb_rays_level_jacobian(b["co"], los, lf.tab, b["step_row"], b["par_level"], par_c)
    torch.cuda.synchronize()
    jac = torch.full((los.n_rays, n_par, n_pts), 7.25, dtype=torch.float64, device="cuda")
    rad = torch.full((los.n_rays, n_pts), 7.25, dtype=torch.float64, device="cuda")
    ip_, dp_ = _lib.ip, _lib.dp
    ptr = lambda t: C.c_void_p(t.data_ptr())

    def call(**kw):
        d = los.desc()
        if "init_mode" in kw:
            d.init_mode = kw["init_mode"]
        row = np.ascontiguousarray(kw.get("coef_row", b["step_row"]), dtype=np.int32)
        lev = np.ascontiguousarray(kw.get("par_level", b["par_level"]), dtype=np.int32)
        return _lib.lib.sr_limb_rays_jac_level_dev(
            ptr(a), ptr(e), n_layers, kw.get("n_pts", n_pts), C.byref(d), kw.get("gas", 0), ptr(lf.tab),
            kw.get("n_levels", n_lev), n_rows, row.ctypes.data_as(ip_), kw.get("n_par", n_par), lev.ctypes.data_as(ip_),
            par_c.ctypes.data_as(dp_), ptr(rad), None if kw.get("no_jac") else ptr(jac), eng._stream_ptr())

    bad_row_lo, bad_row_hi = b["step_row"].copy(), b["step_row"].copy()
    bad_row_lo[3], bad_row_hi[6] = -1, n_rows
    bad_lev_lo, bad_lev_hi = b["par_level"].copy(), b["par_level"].copy()
    bad_lev_lo[0], bad_lev_hi[-1] = -1, n_lev
    refused = [(dict(gas=-1), _lib.SR_ERR_ARG), (dict(gas=n_gas), _lib.SR_ERR_ARG),
               (dict(coef_row=bad_row_lo), _lib.SR_ERR_ARG), (dict(coef_row=bad_row_hi), _lib.SR_ERR_ARG),
               (dict(par_level=bad_lev_lo), _lib.SR_ERR_ARG), (dict(par_level=bad_lev_hi), _lib.SR_ERR_ARG),
               (dict(no_jac=True), _lib.SR_ERR_ARG), (dict(n_par=0), _lib.SR_ERR_ARG),
               (dict(init_mode=1), _lib.SR_ERR_ARG), (dict(n_pts=2000001), _lib.SR_ERR_LIMIT)]
    for kw, status in refused:
        assert call(**kw) == status, kw
        torch.cuda.synchronize()
        assert bool((jac == 7.25).all()) and bool((rad == 7.25).all()), kw
    assert call() == _lib.SR_OK
    torch.cuda.synchronize()
    assert torch.equal(jac, good) and torch.equal(rad, good_rad)
    # the wrappers' own shape checks
    with pytest.raises(ValueError):
        eng.limb_rays_level_jacobian(b["co"], los, lf.tab, b["step_row"][:5], b["par_level"], par_c)
    with pytest.raises(ValueError):
        eng.limb_rays_level_jacobian(b["co"], los, lf.tab, b["step_row"], b["par_level"][:4], par_c)
    with pytest.raises(ValueError):
        lf.tvib_jacobian(b["co"], los, b["step_row"], None, b["par_level"], b["par_w"])
    with pytest.raises(RuntimeError):
        eng.limb_rays_level_jacobian(b["co"], los, lf.tab, bad_row_hi, b["par_level"], par_c)
