"""Row parameters -- kinetic-temperature nodes -- in the one-pass state Jacobian (sr_limb_rays_jac_state_rows_dev,
engine.limb_rays_state_jacobian(dcoeffs=, par_t=), LevelFactored.state_jacobian, retrieval.TempProfile and
retrieval.inversion_state): a row parameter acts through the coefficients of every gas with a weight per coefficient row,
    dtau_p = par_t[p][r] sum_g u_g dabs_g[r],   dE_p = par_t[p][r] sum_g u_g demi_g[r],
the per-row Jacobian of sr_limb_rays_jac_layer_dev contracted with the weights inside the recursion.  The reference has no
derivative code: the definition is the build's, checked (A) against the extended-precision recursion of
tests/limb_reference.py, (B) in blocks mixed with the other two kinds against the three existing calls, (C) against
central differences of the recursion, (D) for its refusals, (E) for n_row = 0, (F) in the retrieval driver.
Synthetic inputs at the shapes of _synthetic in tests/test_gpu_state_jacobian.py (tests/state_rows_cases.py)."""
import copy
import ctypes as C

import numpy as np
import pytest

import limb_reference as R
import state_rows_cases as S

pytestmark = pytest.mark.gpu


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


# ------------------------------------------------------------------------------------------------------------------
# A: against the extended-precision reference
# ------------------------------------------------------------------------------------------------------------------
PANEL_CASES = [(g, n, "-") for n in (3, 17) for g in (1, 2, 3, 4)] + [(2, 3, "solo"), (4, 17, "solo"), (1, 17, "planck"), (3, 3, "planck")]


@pytest.mark.parametrize("n_gas,n_row,opt", PANEL_CASES)
def test_row_parameters_against_the_extended_precision_reference(eng, n_gas, n_row, opt):
    """A.  Row parameters only -- n_row 3: eight slots, one block; 17: sixteen slots, two blocks -- on the regime panel
    (thin switch, range-reduction boundaries, saturated, zero and negative optical depths) laid on the six coefficient
    rows, derivative spectra of either sign, one parameter without weights.  Every (ray, parameter) row within
    KERNEL_MARGIN x K_PLAIN units of the bound of tests/limb_reference.py, K_PLAIN being what the plain fp64 recursion
    measures against the reference on these inputs (radiances and Jacobians separately), never what the kernel gives;
    tests/test_state_rows_host.py holds that yardstick below the recorded constants.  solo: absorption alone of a
    Planck background; planck: emission and a Planck background.  Every figure is printed before anything is asserted;
    figures from an MI355X run have not been recorded here yet."""
    import torch
    from spectrobot_amd import synthetic as syn
    c = S.panel_case(n_gas, n_row)
    N = len(c["names"])
    at = R.tile_columns(N, S.N_PTS, np.random.default_rng([S.SEED, n_gas, n_row, 1]))    # panel column of every point
    cols = at
    solo, planck = opt == "solo", opt in ("solo", "planck")
    opts = dict(solo_absorption=True, initial_temperature=250.0) if solo else (dict(initial_temperature=180.0) if planck else {})
    grid = syn.make_grid(2975.0, 5e-4, S.N_PTS) if planck else None
    plain = eng.LimbLOS(S.SEG_OFF, S.SEG_LAYER, S.PT_OFF, c["x"], c["nd"], c["vmr"])
    col = plain.columns()                        # the device's Curtis-Godson columns: fp64 inputs of the reference
    plain.close()
    los = eng.LimbLOS(S.SEG_OFF, S.SEG_LAYER, S.PT_OFF, c["x"], c["nd"], c["vmr"], **opts)
    try:
        assert np.allclose(col, S.cg_columns(c["nd"], c["x"], c["vmr"]), rtol=1e-12)
        I0 = np.zeros(N)
        if planck:     # the Planck intensity as the device forms it: the radiance through empty coefficients
            zero = torch.zeros((n_gas, S.N_LAYERS, S.N_PTS), dtype=torch.float64, device="cuda")
            I0 = _np(eng.limb_rays((zero, zero), los, grid=grid, resident=False))[0][:N]
            assert np.all(I0 > 0)
            cols = cols[:N]                      # (the first tile is the panel in its own order)
        refs = S.references(c, col, I0, solo=solo)
        k_rad, k_jac = S.k_plain(refs, n_gas, cols)
        pick = lambda a: _t(a[:, :, at])
        rad, jac = eng.limb_rays_state_jacobian((pick(c["coef_a"]), pick(c["coef_e"])), los, grid=grid,
                                                dcoeffs=(pick(c["dabs"]), pick(c["demi"])), par_t=c["par_t"])
    finally:
        los.close()
    assert tuple(jac.shape) == (3, n_row, S.N_PTS) and tuple(rad.shape) == (3, S.N_PTS)
    rad, jac = _np(rad)[:, :len(cols)], _np(jac)[:, :, :len(cols)]
    lim_rad, lim_jac = R.KERNEL_MARGIN * k_rad, R.KERNEL_MARGIN * k_jac
    print("\nstate rows vs reference [n_gas %d, n_row %d, %s]: K_PLAIN rad %.3g jac %.3g, limits %.3g %.3g"
          % (n_gas, n_row, opt, k_rad, k_jac, lim_rad, lim_jac))
    over = []
    for r, (ref, _) in enumerate(refs):
        u_r = R.worst(R.units(rad[r], ref["I"][cols], ref["A_I"][cols], ref["C_I"][cols], n_gas), c["names"], cols)
        u_j = R.worst(R.units(jac[r], ref["J"][:, cols], ref["A"][:, cols], ref["C"][:, cols], n_gas), c["names"], cols)
        print("  ray %d (%d seg): rad %.3g units at %s; jac %.3g units at %s" % (r, S.SEG_OFF[r + 1] - S.SEG_OFF[r], u_r[0], u_r[1],
                                                                           u_j[0], u_j[1]))
        over += [("rad", r) + u_r] * (not u_r[0] <= lim_rad) + [("jac", r) + u_j] * (not u_j[0] <= lim_jac)
    assert k_rad <= R.K_PLAIN_RAD and k_jac <= R.K_PLAIN_JAC
    assert not over, "over %g x K_PLAIN (rad %.3g, jac %.3g units): %s" % (R.KERNEL_MARGIN, lim_rad, lim_jac, over)
    assert not jac[:, 1].any()                                           # the parameter without weights: exact zeros
    assert np.abs(jac[:, 0]).max(axis=-1).min() > 0                     # parameter 0 is seen by every ray


# ------------------------------------------------------------------------------------------------------------------
# B - E: synthetic coefficients, all three kinds
# ------------------------------------------------------------------------------------------------------------------
def _mixed(n_gas, n_col, n_lev, n_row):
    """Coefficients from optically thin to thick, pair tables on 4 table rows, 3 levels, and parameters of the three kinds;
    derivative spectra of either sign; column parameter 1, level parameter 1 and row parameter 1 have no weights at all,
    and no row parameter weights row 3, the single-segment ray's."""
    n_levels, n_tab = 3, 4
    rng = np.random.default_rng([S.SEED, n_gas, n_col, n_lev, n_row])
    x, nd = S.geometry(7)
    vmr = rng.uniform(0.2, 0.8, (n_gas, 2 * S.N_SEG))
    shape = (n_gas, S.N_LAYERS, S.N_PTS)
    co = (np.exp(rng.uniform(np.log(1e-4), np.log(3.0), shape)), rng.uniform(0.1, 1.0, shape))
    dco = (co[0] * rng.uniform(-1.0, 1.0, shape), co[1] * rng.uniform(-1.0, 1.0, shape))
    tab = rng.uniform(0.1, 1.0, (n_levels, 2, n_tab, S.N_PTS))
    sparse = lambda n, m: rng.uniform(-1.0, 1.0, (n, m)) * (rng.uniform(size=(n, m)) > 0.2)
    par_w, par_c, par_t = np.abs(sparse(n_col, 2 * S.N_SEG)), sparse(n_lev, S.N_LAYERS), sparse(n_row, S.N_LAYERS)
    for a in (par_w, par_c, par_t):
        if len(a) > 1:
            a[1] = 0.0
    par_t[:, 3] = 0.0
    par_t[0, 4] = 0.6        # (the rays of four and seven segments both meet a row that row parameter 0 weights)
    par_t[0, 2] = -0.4
    return dict(x=x, nd=nd, vmr=vmr, co=tuple(_t(v) for v in co), dco=tuple(_t(v) for v in dco), tab=_t(tab),
                coef_row=np.array([0, 2, 1, 3, 3, 0], np.int32), par_gas=rng.integers(0, n_gas, n_col).astype(np.int32),
                par_w=par_w, par_level=rng.integers(0, n_levels, n_lev).astype(np.int32), par_c=par_c, par_t=par_t,
                gas=n_gas - 1, co_np=co, dco_np=dco)


def _los(eng, m, **opts):
    return eng.LimbLOS(S.SEG_OFF, S.SEG_LAYER, S.PT_OFF, m["x"], m["nd"], m["vmr"], **opts)


def _state_rows(eng, m, los, **kw):
    return eng.limb_rays_state_jacobian(m["co"], los, m["par_gas"], m["par_w"], m["tab"], m["coef_row"], m["par_level"],
                                        m["par_c"], gas=m["gas"], dcoeffs=m["dco"], par_t=m["par_t"], **kw)


@pytest.mark.parametrize("n_gas", [1, 2, 3, 4])
@pytest.mark.parametrize("n_col,n_lev,n_row", [(2, 3, 4), (7, 6, 5)])
def test_mixed_blocks_equal_the_three_existing_calls(eng, n_gas, n_col, n_lev, n_row):
    """B.  2 + 3 + 4 parameters: one sixteen-slot block holding all three kinds; 7 + 6 + 5: two blocks, the first holding
    all kinds.  Column rows against limb_rays_jacobian (forward kernel and default route), level rows against
    limb_rays_level_jacobian, row rows against the per-row Jacobian contracted with par_t in fp64 on the host
    (limb_rays_layer_jacobian and the one-pass limb_rays_jacobians: two routes).  Per (ray, parameter) row relative to its
    largest value: max(1e-12, 4 x the spread of the reference's two routes), the rule of
    tests/test_gpu_state_jacobian.py::test_equals_the_two_existing_calls (one route: 1e-12).  Radiances against limb_rays
    within 1e-13; the parameters without weights and, for the row parameters, the ray that meets no weighted row: exact
    zeros.  Whether the column and level rows are bit for bit those of the call without row parameters is printed (expected,
    not required)."""
    import torch
    m = _mixed(n_gas, n_col, n_lev, n_row)
    los = _los(eng, m)
    try:
        try:
            eng.set_jac_layer_mode(1)
            _, ref_cf = eng.limb_rays_jacobian(m["co"], los, m["par_gas"], m["par_w"])
            torch.cuda.synchronize()
        finally:
            eng.set_jac_layer_mode(0)
        _, ref_co = eng.limb_rays_jacobian(m["co"], los, m["par_gas"], m["par_w"])
        _, ref_l = eng.limb_rays_level_jacobian(m["co"], los, m["tab"], m["coef_row"], m["par_level"], m["par_c"], gas=m["gas"])
        lay_f = eng.limb_rays_layer_jacobian(m["co"], m["dco"], los)
        _, lay_o, _ = eng.limb_rays_jacobians(m["co"], los, dcoeffs=m["dco"])
        contract = lambda j: _t(np.einsum("rkj,pk->rpj", _np(j), m["par_t"]))
        ref_rf, ref_ro = contract(lay_f), contract(lay_o)
        r0 = eng.limb_rays(m["co"], los)
        rad, jac = _state_rows(eng, m, los)
        rad_s, jac_s = eng.limb_rays_state_jacobian(m["co"], los, m["par_gas"], m["par_w"], m["tab"], m["coef_row"],
                                                    m["par_level"], m["par_c"], gas=m["gas"])
    finally:
        los.close()
    assert tuple(jac.shape) == (3, n_col + n_lev + n_row, S.N_PTS) and bool(torch.isfinite(jac).all())
    jc, jl, jr = jac[:, :n_col], jac[:, n_col:n_col + n_lev], jac[:, n_col + n_lev:]
    sp_c, sp_r = float(_row_err(ref_cf, ref_co).max()), float(_row_err(ref_rf, ref_ro).max())
    tol_c, tol_r = max(1e-12, 4.0 * sp_c), max(1e-12, 4.0 * sp_r)
    err_c = float(torch.minimum(_row_err(jc, ref_cf), _row_err(jc, ref_co)).max())
    err_l = float(_row_err(jl, ref_l).max())
    err_r = float(torch.minimum(_row_err(jr, ref_rf), _row_err(jr, ref_ro)).max())
    d_rad = float((rad - r0).abs().max() / r0.abs().max())
    print("\nstate rows mixed [n_gas %d, %d + %d + %d]: column rows %.2e (two routes apart %.2e, bound %.2e); level rows %.2e "
          "(bound 1e-12); row rows %.2e (two routes apart %.2e, bound %.2e); radiances vs limb_rays %.2e (bound 1e-13); column "
          "and level rows bit for bit those of the call without row parameters: %s, radiances: %s"
          % (n_gas, n_col, n_lev, n_row, err_c, sp_c, tol_c, err_l, err_r, sp_r, tol_r, d_rad,
             torch.equal(jac[:, :n_col + n_lev], jac_s), torch.equal(rad, rad_s)))
    assert float(ref_cf.abs().max()) > 0 and float(ref_l.abs().max()) > 0 and float(ref_rf.abs().max()) > 0
    assert err_c <= tol_c and err_l <= 1e-12 and err_r <= tol_r
    assert d_rad < 1e-13
    # exact zeros: the parameters without weights, every row the references hold at zero, the ray that meets no weighted row
    assert not bool(jc[:, 1].any()) and not bool(jl[:, 1].any()) and not bool(jr[:, 1].any())
    assert not bool(jr[0].any()) and bool(jr[1:, 0].abs().amax(dim=-1).min() > 0)
    for got, ref in ((jc, ref_cf), (jl, ref_l), (jr, ref_rf)):
        zero = ref.abs().amax(dim=-1) == 0
        assert bool((got.abs().amax(dim=-1)[zero] == 0).all())


def test_central_differences_of_the_recursion(eng):
    """C.  The best-seen row parameter (max|jac| / max|rad|) against central differences of limb_rays on
    coeffs +- h par_t[p][r] dcoeffs[r] at h and h / 2: the perturbation is exactly linear in the coefficients, so nothing
    but the recursion is differenced.  |jac - FD(h/2)| <= 2 |FD(h) - FD(h/2)| + 1e-9 max|jac| per ray in the max norm
    (DESIGN 4.7 (B)), and |FD(h) - FD(h/2)| < 1e-3 max|jac| so that the bound cannot go slack."""
    m = _mixed(3, 2, 3, 4)
    los = _los(eng, m)
    try:
        rad, jac = _state_rows(eng, m, los)
        n0 = 5
        seen = (jac[:, n0:].abs().amax(dim=(0, 2)) / rad.abs().max()).cpu().numpy()
        p = int(np.argmax(seen))
        w = m["par_t"][p][None, :, None]

        def fd(h):
            out = []
            for sgn in (1.0, -1.0):
                co = tuple(_t(c + sgn * h * w * d) for c, d in zip(m["co_np"], m["dco_np"]))
                out.append(eng.limb_rays(co, los).clone())
            return (out[0] - out[1]) / (2.0 * h)

        h = 1e-3
        f1, f2 = fd(h), fd(0.5 * h)
    finally:
        los.close()
    jm = float(jac[:, n0 + p].abs().max())
    trunc = (f1 - f2).abs().amax(dim=-1)
    err = (jac[:, n0 + p] - f2).abs().amax(dim=-1)
    print("\nstate rows FD: max|jac| / max|rad| per row parameter %s; parameter %d, h %.3g: |jac - FD(h/2)| / max|jac| %.2e, "
          "|FD(h) - FD(h/2)| / max|jac| %.2e" % (np.array2string(seen, precision=2), p, h, float(err.max()) / jm, float(trunc.max()) / jm))
    assert float(trunc.max()) < 1e-3 * jm
    assert bool((err <= 2.0 * trunc + 1e-9 * jm).all())


def test_refused_calls_leave_the_output_untouched(eng):
    """D.  Every refused argument returns its status before anything is copied or launched (rad and jac keep their
    sentinel), and a valid call afterwards reproduces the earlier result bit for bit."""
    import torch
    from spectrobot_amd import _lib
    m = _mixed(2, 7, 6, 5)
    los = _los(eng, m)
    a, e = m["co"]
    da, de = m["dco"]
    n_gas, n_layers, n_pts = a.shape
    n_levels, n_tab = m["tab"].shape[0], m["tab"].shape[2]
    n_col, n_lev, n_row = 7, 6, 5
    par_w, par_c, par_t = (np.ascontiguousarray(m[k]) for k in ("par_w", "par_c", "par_t"))
    good_rad, good = _state_rows(eng, m, los)
    torch.cuda.synchronize()
    jac = torch.full((3, n_col + n_lev + n_row, n_pts), 7.25, dtype=torch.float64, device="cuda")
    rad = torch.full((3, n_pts), 7.25, dtype=torch.float64, device="cuda")
    ip_, dp_ = _lib.ip, _lib.dp
    ptr = lambda t: C.c_void_p(t.data_ptr())

    def call(**kw):
        d = los.desc()
        if "init_mode" in kw:
            d.init_mode = kw["init_mode"]
        row = np.ascontiguousarray(kw.get("coef_row", m["coef_row"]), dtype=np.int32)
        lev = np.ascontiguousarray(kw.get("par_level", m["par_level"]), dtype=np.int32)
        pg = np.ascontiguousarray(kw.get("par_gas", m["par_gas"]), dtype=np.int32)
        no = kw.get("no", ())
        return _lib.lib.sr_limb_rays_jac_state_rows_dev(
            ptr(a), ptr(e), n_layers, kw.get("n_pts", n_pts), C.byref(d), kw.get("n_col", n_col), pg.ctypes.data_as(ip_),
            par_w.ctypes.data_as(dp_), kw.get("gas", m["gas"]), None if "tab" in no else ptr(m["tab"]),
            kw.get("n_levels", n_levels), n_tab, row.ctypes.data_as(ip_), kw.get("n_lev", n_lev), lev.ctypes.data_as(ip_),
            par_c.ctypes.data_as(dp_), None if "dabs" in no else ptr(da), None if "demi" in no else ptr(de),
            kw.get("n_row", n_row), None if "par_t" in no else par_t.ctypes.data_as(dp_), ptr(rad),
            None if "jac" in no else ptr(jac), eng._stream_ptr())

    bad_row, bad_lev, bad_gas = m["coef_row"].copy(), m["par_level"].copy(), m["par_gas"].copy()
    bad_row[5], bad_lev[0], bad_gas[-1] = n_tab, -1, n_gas
    A, L = _lib.SR_ERR_ARG, _lib.SR_ERR_LIMIT
    refused = [(dict(no=("dabs",)), A), (dict(no=("demi",)), A), (dict(no=("par_t",)), A), (dict(no=("jac",)), A),
               (dict(no=("tab",)), A), (dict(n_row=-1), A), (dict(n_col=-1), A), (dict(n_lev=-2), A),
               (dict(n_col=0, n_lev=0, n_row=0), A), (dict(gas=-1), A), (dict(gas=n_gas), A), (dict(coef_row=bad_row), A),
               (dict(par_level=bad_lev), A), (dict(par_gas=bad_gas), A), (dict(init_mode=1), A), (dict(n_pts=2000001), L)]
    try:
        for kw, status in refused:
            assert call(**kw) == status, kw
            torch.cuda.synchronize()
            assert bool((jac == 7.25).all()) and bool((rad == 7.25).all()), kw
        assert call() == _lib.SR_OK
        torch.cuda.synchronize()
        assert torch.equal(jac, good) and torch.equal(rad, good_rad)
        # the wrapper's own checks
        with pytest.raises(ValueError):
            eng.limb_rays_state_jacobian(m["co"], los, dcoeffs=m["dco"])
        with pytest.raises(ValueError):
            eng.limb_rays_state_jacobian(m["co"], los, par_t=par_t)
        with pytest.raises(ValueError):
            eng.limb_rays_state_jacobian(m["co"], los, dcoeffs=m["dco"], par_t=par_t[:, :5])
        with pytest.raises(ValueError):
            eng.limb_rays_state_jacobian(m["co"], los, dcoeffs=(da[:, :5].contiguous(), de[:, :5].contiguous()), par_t=par_t)
        with pytest.raises(ValueError):
            eng.limb_rays_state_jacobian(m["co"], los, dcoeffs=m["dco"], par_t=np.zeros((0, n_layers)))       # no parameters
    finally:
        los.close()


@pytest.mark.parametrize("n_gas", [1, 3])
def test_without_row_parameters_it_is_the_state_call(eng, n_gas):
    """E.  n_row = 0 through the new entry: bit for bit the existing entry's result."""
    import torch
    m = _mixed(n_gas, 7, 6, 5)
    los = _los(eng, m)
    try:
        args = (m["co"], los, m["par_gas"], m["par_w"], m["tab"], m["coef_row"], m["par_level"], m["par_c"])
        rad0, jac0 = eng.limb_rays_state_jacobian(*args, gas=m["gas"])
        rad1, jac1 = eng.limb_rays_state_jacobian(*args, gas=m["gas"], dcoeffs=m["dco"], par_t=np.zeros((0, S.N_LAYERS)))
    finally:
        los.close()
    assert tuple(jac1.shape) == tuple(jac0.shape) == (3, 13, S.N_PTS)
    assert torch.equal(jac1, jac0) and torch.equal(rad1, rad0)


# ------------------------------------------------------------------------------------------------------------------
# F: the driver
# ------------------------------------------------------------------------------------------------------------------
def _scene(eng, n_grid=16000, n_layers=24):
    """The scene of tests/test_gpu_inversion_state.py -- an HCN-like LTE trace gas and a non-LTE CH4 on the level-factored
    route -- with the CH4 tables also at T + dT."""
    import bench_configs as bc
    from spectrobot_amd import retrieval, synthetic as syn
    grid = syn.make_grid(3290.0, 5e-4, n_grid)
    Lc = syn.make_lines(3000, grid, config_id=4, n_levels=12)
    Lh = syn.make_lines(800, grid, config_id=5, n_levels=6)
    Lh["a_coeff"] = Lh["a_coeff"] * 30.0
    atm = syn.make_atmosphere(n_layers, 12)
    ch4 = retrieval.LevelGas("CH4", eng.LineSet(Lc, grid, 6, 1, syn.CH4_MM, syn.CH4_LEVEL_ENERGIES), np.full(n_layers, 1.48e-4),
                             atm["tvib"], syn.CH4_ISO_RATIO, dT=0.05)
    hcn = retrieval.Gas("HCN", eng.LineSet(Lh, grid, 23, 1, bc.HCN_MM, bc.HCN_LEVEL_ENERGIES), np.full(n_layers, 2e-6),
                        bc.HCN_ISO_RATIO)
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
    return ([z[0] + f * span for f in (0.1, 0.45, 0.8)], [z[0] + f * span for f in (0.15, 0.4, 0.65, 0.9)],
            [z[0] + f * span for f in (0.12, 0.5, 0.85)])


def test_driver_one_iteration_equals_the_composition(eng):
    """F.  Temperature nodes between the HCN VMR nodes and the Tvib nodes of a CH4 level, pixels with the closed-form field
    of view, one iteration: bayes_set.jacobian against limb_rays_jacobian + tvib_jacobian + limb_rays_layer_jacobian
    contracted with the node masks -> hires_to_lowres -> smm.FOV_integr_1D(closed_form=True) within 1e-11 of a column's
    largest element, the update against smm.inversion_algebra_arrays on that K to rtol 1e-9 (the bounds of
    tests/test_gpu_inversion_state.py for the Tvib state)."""
    import torch
    from spectrobot_amd import retrieval, spect_main_module as smm
    scene, pixels = _scene(eng)
    z = scene.z
    hcn_nodes, tv_nodes, t_nodes = _nodes(z)
    scene.gas("HCN").add_clim(np.full(len(z), 2.6e-6))
    _observe(scene, pixels, 0.004, np.random.default_rng(5))
    nd0 = scene.nd.copy()
    bs = smm.BayesSet(tag="HCN + T + Tvib of a CH4 level")
    bs.add_set(retrieval.TvibProfile("CH4", 5, z, tv_nodes, np.full(4, 4.0), first_guess=np.array([1.0, -0.5, 0.7, 0.2])))
    bs.add_set(retrieval.TempProfile(z, t_nodes, np.full(3, 3.0), first_guess=np.array([1.5, -1.0, 0.5])))
    bs.add_set(smm.LinearProfile_1D_new("HCN", z, hcn_nodes, np.full(3, 2.2e-6), np.full(3, 1.1e-6)))
    n_par = 10
    # the composition, at the first guess
    ref = copy.deepcopy(bs)
    retrieval._state_into_gases(scene, ref)
    assert np.array_equal(scene.temps, scene.temps0 + ref.sets["temp"].profile()) and np.abs(scene.temps - scene.temps0).max() > 1.0
    pix = sorted(pixels, key=lambda p: p.limb_tg_alt)
    alts = [a for p in pix for a in p.los_alts()]
    co, dco = (eng.gas_stack(c) for c in scene.temperature_derivatives())
    los, alt = scene.los(alts)
    w = scene.state_weights(ref, alt)
    lg = scene.gas("CH4")
    assert w.level_gas is lg and w.gas == 1 and list(w.perm) == [3, 4, 5, 6, 7, 8, 9, 0, 1, 2]
    rad, jc = eng.limb_rays_jacobian(co, los, w.par_gas, w.par_w_col)
    _, jl = lg.lf.tvib_jacobian(co, los, lg.rows, lg.tvib, w.par_level, w.par_w_lev, gas=w.gas)
    jt = torch.einsum("rkj,pk->rpj", eng.limb_rays_layer_jacobian(co, dco, los), torch.as_tensor(w.par_w_temp, device="cuda"))
    low = lambda t: eng.hires_to_lowres(t.contiguous(), scene.grid, scene.bands_nm, scene.widths_nm, out_units=scene.out_units)
    lo_r = low(rad)
    lo_j = np.concatenate([low(jc).reshape(len(alts), 3, -1), low(jl).reshape(len(alts), 4, -1),
                           low(jt).reshape(len(alts), 3, -1)], axis=1)[:, w.perm]
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
    # the driver, one iteration
    chi, obs, out, b = retrieval.inversion_state(scene, bs, pixels, max_it=1)
    assert b is bs and len(b.history) == 1 and b.stop == 'max_it' and chi == b.history[0]
    assert b.jacobian.shape == K.shape and len(out) == len(pix)
    col_max = np.abs(K).max(axis=0)
    dist = np.abs(b.jacobian - K).max(axis=0) / np.where(col_max > 0, col_max, 1.0)
    chi_ref = np.sum(((obs_vec - sim_vec) / noi_vec) ** 2) / (obs_vec.size - n_par)
    print("\ninversion_state with T: |K - composition| per column / the column's largest element:", np.array2string(dist, precision=2),
          "; largest |K| per column:", np.array2string(col_max, precision=3))
    print("inversion_state with T: chi square %.8g (composition %.8g); update, largest relative difference %.2e"
          % (chi, chi_ref, np.max(np.abs(b.param_vector() - ref.param_vector()) / np.abs(ref.param_vector()))))
    assert np.all(col_max[4:7] > 0) and np.all(dist <= 1e-11)
    assert np.allclose(chi, chi_ref, rtol=1e-9)
    assert np.allclose(np.array([s.spectrum for s in out]).ravel(), sim_vec, rtol=1e-11)
    assert np.allclose(b.param_vector(), ref.param_vector(), rtol=1e-9)
    # the scene holds the updated state; densities and columns were not touched
    assert np.array_equal(scene.temps, scene.temps0 + b.sets["temp"].profile()) and np.array_equal(scene.nd, nd0)
    assert np.array_equal(lg.tvib[5], lg.tvib0[5] + b.sets["tvib:CH4:5"].profile())
    assert np.array_equal(scene.gas("HCN").vmr, b.sets["HCN"].profile())
    # a LevelGas without dT cannot give the derivative
    lg.dT = None
    with pytest.raises(ValueError, match="dT"):
        retrieval.inversion_state(scene, copy.deepcopy(bs), pixels, max_it=1)


def test_driver_without_a_temp_set_walks_the_loop_of_today(eng, monkeypatch):
    """F.  VMR sets only: no call carries row parameters, temperature_derivatives is never asked, and the chi-square history
    is bit for bit that of the loop's statements written out here from the existing calls."""
    import bench_configs as bc
    from spectrobot_amd import retrieval, spect_main_module as smm
    scene = bc.two_gas_scene(6000, 1500, 16000, 30)
    bs, pixels, _ = bc.retrieval_problem(scene)
    seen = []
    real = eng.limb_rays_state_jacobian
    monkeypatch.setattr(retrieval.engine, "limb_rays_state_jacobian", lambda *a, **k: (seen.append(sorted(k)), real(*a, **k))[1])
    monkeypatch.setattr(retrieval.LimbScene, "temperature_derivatives", lambda self: pytest.fail("no temperature set"))
    chi, _, sims, b = retrieval.inversion_state(scene, copy.deepcopy(bs), pixels, max_it=4)
    monkeypatch.undo()
    assert len(seen) == len(b.history) >= 2 and all(k == ["par_gas", "par_w"] for k in seen)
    # the loop's statements of today, from the existing calls
    ref = copy.deepcopy(bs)
    pix = sorted(pixels, key=lambda x: x.limb_tg_alt)
    alts = [a for p in pix for a in p.los_alts()]
    with_fov = sum(p.fov_half > 0 for p in pix)
    retrieval._state_into_gases(scene, ref)
    obs_vec, _, noi_vec = smm.genvec([p.observation for p in pix], [p.observation for p in pix], [p.noise for p in pix],
                                     masks=None if all(p.mask is None for p in pix) else [p.mask for p in pix])
    assert all(p.mask is None for p in pix)
    Sa_inv = np.linalg.inv(np.asarray(ref.VCM_apriori(), dtype=float))
    lowres = lambda r: eng.hires_to_lowres(r, scene.grid, scene.bands_nm, scene.widths_nm, out_units=scene.out_units)
    history = []
    for _ in range(len(b.history)):
        coeffs = scene.coefficient_stack()
        los, alt = scene.los(alts)
        w = scene.state_weights(ref, alt)
        rad, jac = eng.limb_rays_state_jacobian(coeffs, los, par_gas=w.par_gas, par_w=w.par_w_col)
        n_par = jac.shape[1]
        both = np.concatenate([lowres(rad)[:, None, :], lowres(jac.view(len(alts) * n_par, -1)).reshape(len(alts), n_par, -1)[:, w.perm]], axis=1)
        fov = smm.fov_closed_form(both[0::3], both[1::3], both[2::3], [p.pixel_rot for p in pix]) if with_fov else both[1::3]
        low, dlow = fov[:, 0, :], fov[:, 1:, :]
        for par in ref.params():
            par.set_used()
        sim_vec = low.reshape(-1)
        history.append(np.sum(((obs_vec - sim_vec) / noi_vec) ** 2) / (len(obs_vec) - ref.n_used_par()))
        K = np.transpose(dlow, (1, 0, 2)).reshape(n_par, -1).T
        smm.inversion_algebra_arrays(K, obs_vec, sim_vec, noi_vec, ref, lambda_LM=0.1, L1_reg=False, Sa_inv=Sa_inv)
        retrieval._state_into_gases(scene, ref)
    print("\ninversion_state, VMR sets only: history %s, written out %s" % (b.history, history))
    assert list(b.history) == history


def test_noise_free_twin_of_vmr_and_temperature(eng):
    """F.  Observations from a perturbed truth -- the HCN profile scaled by 1.3, a temperature bump of 4 K -- without noise:
    chi square falls from the first iteration to the last and the loop stops by its own rule or at max_it (no convergence
    figure is fixed); the history and the recovered offsets are printed."""
    from spectrobot_amd import retrieval, spect_main_module as smm
    scene, pixels = _scene(eng)
    z = scene.z
    span = z[-1] - z[0]
    hcn_nodes, _, t_nodes = _nodes(z)
    apr_hcn, sig_hcn, sig_t = np.full(3, 2.2e-6), np.full(3, 1.1e-6), np.full(3, 3.0)
    x_true = np.concatenate([1.3 * apr_hcn, 4.0 * np.exp(-0.5 * ((np.array(t_nodes) - z[0] - 0.45 * span) / (0.25 * span)) ** 2)])
    truth = smm.BayesSet()
    truth.add_set(smm.LinearProfile_1D_new("HCN", z, hcn_nodes, apr_hcn, sig_hcn, first_guess_prof=x_true[:3]))
    truth.add_set(retrieval.TempProfile(z, t_nodes, sig_t, first_guess=x_true[3:]))
    retrieval._state_into_gases(scene, truth)
    _observe(scene, pixels, 0.004)              # (no coefficients were computed before: these are at the truth's temperatures)
    bs = smm.BayesSet(tag="HCN + T")
    bs.add_set(smm.LinearProfile_1D_new("HCN", z, hcn_nodes, apr_hcn, sig_hcn))
    bs.add_set(retrieval.TempProfile(z, t_nodes, sig_t))
    chi, _, sims, b = retrieval.inversion_state(scene, bs, pixels, max_it=6)
    print("\ninversion_state twin with T: %d iterations (%s), chi square %s; retrieved %s, truth %s"
          % (len(b.history), b.stop, np.array2string(np.array(b.history), precision=4),
             np.array2string(b.param_vector(), precision=3), np.array2string(x_true, precision=3)))
    assert len(b.history) >= 2 and b.history[-1] < b.history[0]
    assert b.stop == 'max_it' or len(b.history) < 6
    assert len(sims) == len(pixels) and b.jacobian.shape == (len(pixels) * len(scene.bands_nm), 6)
    assert np.array_equal(scene.temps, scene.temps0 + b.sets["temp"].profile())
