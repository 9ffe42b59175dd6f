"""The mixed-state Jacobian on the instrument's bands in one call (sr_limb_rays_state_bands_dev,
engine.limb_rays_state_bands, LevelFactored.state_bands, retrieval.inversion_state(bands_in_kernel=True)): the recursion
kernel integrates the bands in its epilogue and no hi-res spectrum is written.  The reference is the route that exists
without it, on the same inputs: limb_rays_state_jacobian -> hires_to_lowres on rad and on the flattened jac ->
smm.fov_closed_form.  Both run the same recursion and differ in the order of the band sums only, so the bound is that of
tests/test_gpu_limb.py::test_band_fusion_equals_the_instrument_step for the same epilogue: 1e-12 of a quantity row's
largest element.  The hi-res Jacobian is pinned to the extended-precision reference (tests/test_gpu_limb_reference.py),
hires_to_lowres to the reference's Python (tests/golden/lowres_ils.npz), and the band integrals of both routes -- weights,
window ends, ranges, the band epilogue and the field of view -- to the extended-precision reference of the instrument step
(tests/lowres_reference.py, tests/test_gpu_lowres_reference.py): this file ties the new call to their composition."""
import copy

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

BOUND = 1e-12
NL = 22                       # layers
N_LEVELS, N_TAB_ROWS = 6, 11
ROTS = [0.0, 20.0]            # the two pixels' rotations (the first has no edge term)


@pytest.fixture(scope="module")
def eng():
    import torch
    assert torch.cuda.is_available(), "these tests need the GPU"
    from spectrobot_amd import engine
    engine.set_device(0)
    return engine


def _bands(grid, n_extra, rng):
    """The seven bands of test_band_fusion_equals_the_instrument_step: one far outside the grid, one over the whole grid,
    narrow ones at both ends, two overlapping, one more; n_extra random ones behind them."""
    lam_lo, lam_hi = 1e7 / grid[-1], 1e7 / grid[0]
    span = lam_hi - lam_lo
    bands = np.array([lam_lo - 50 * span - 1.0, 0.5 * (lam_lo + lam_hi), lam_lo + 0.01 * span, lam_hi - 0.01 * span,
                      lam_lo + 0.4 * span, lam_lo + 0.45 * span, lam_lo + 0.8 * span])
    widths = np.array([0.05 * span, 3.0 * span, 0.004 * span, 0.004 * span, 0.06 * span, 0.06 * span, 0.02 * span])
    if n_extra:
        bands = np.concatenate([bands, lam_lo + span * rng.uniform(0.02, 0.98, n_extra)])
        widths = np.concatenate([widths, span * rng.uniform(0.003, 0.2, n_extra)])
    return bands, widths


def _case(eng, n_col, n_lev, n_row, n_gas, n, order="photon", solo=False, planck=False, seed=0):
    """Inputs of one mixed-state call on 22 layers and 6 limb rays: random coefficient tables, pair tables and derivative
    spectra (both routes read the same ones: they need not belong together), column masks as in the sibling test, level
    and row weights with zeros, and as LAST level / row parameter one whose weights live on the lowest two layers only."""
    import torch
    from spectrobot_amd import synthetic as syn
    rng = np.random.default_rng(1000 * seed + 100 * n_col + 10 * n_lev + n_row + n + n_gas)
    atm = syn.make_atmosphere(NL, 1)
    nd = syn.number_density(atm["press"], atm["temps"])
    z = atm["z"]
    grid = syn.make_grid(2975.0, 5e-4, n)
    t = lambda v: torch.tensor(np.ascontiguousarray(v), device="cuda")
    vm = [np.full(NL, 1.2e-2), np.linspace(2e-3, 5e-4, NL), np.full(NL, 3e-4)][:n_gas]
    a = np.array([rng.uniform(0, 4e-18, (NL, n)) * (10.0 ** (g - 1)) for g in range(n_gas)])
    e = a * rng.uniform(1e-8, 1e-7, a.shape)
    L = syn.limb_los(z, nd * 1e-6, vm, [z[0] + 5.0, z[2] + 3.0, z[5] + 1.0, z[9] + 2.0, z[12] + 1.0, z[15] + 4.0])
    c = dict(n=n, grid=grid, a=a, e=e, coeffs=(t(a), t(e)), L=L, n_par=n_col + n_lev + n_row, n_col=n_col, n_lev=n_lev, n_row=n_row,
             gas=1 if n_gas > 1 else 0, kw={}, rng=rng)
    c["los_kw"] = dict(col_scale=[0.98827, 1.0, 1.0][:n_gas], LOS_order=order, solo_absorption=solo,
                       initial_temperature=250.0 if planck else None)
    # which rays never cross the lowest two layers
    seg_layer, seg_off = np.asarray(L["seg_layer"]), np.asarray(L["seg_off"])
    c["high"] = np.array([not np.any(seg_layer[seg_off[r]:seg_off[r + 1]] <= 1) for r in range(6)])
    assert c["high"].any() and not c["high"].all() and c["high"][3:].all()      # (the second pixel: high rays only)
    if n_col:
        zz = np.append(z, z[-1] + (z[-1] - z[-2]))
        nodes = np.linspace(z[0], z[-1], max(n_col, 2))[:n_col]
        c["kw"]["par_w"] = np.array([np.interp(L["alt"], zz, np.clip(1.0 - np.abs(zz - q) / max(nodes[-1] - nodes[0], 50.0) * max(n_col - 1, 1), 0.0, None) + 0.05)
                                     for q in nodes])
        c["kw"]["par_gas"] = (np.arange(n_col) % n_gas).astype(np.int32)
    if n_lev:
        tab = rng.uniform(0, 4e-18, (N_LEVELS, 2, N_TAB_ROWS, n))
        tab[:, 1] *= rng.uniform(1e-8, 1e-7, tab[:, 1].shape)
        par_c = rng.uniform(0.2, 1.0, (n_lev, NL)) * (rng.uniform(size=(n_lev, NL)) < 0.6)
        par_c[-1] = 0.0
        par_c[-1, :2] = [0.7, 0.4]
        c["tab_np"] = tab
        c["kw"].update(tab=t(tab), coef_row=(np.arange(NL) // 2).astype(np.int32), par_c=par_c,
                       par_level=rng.integers(0, N_LEVELS, n_lev).astype(np.int32))
    if n_row:
        c["da"], c["de"] = a * rng.uniform(-0.02, 0.02, a.shape), e * rng.uniform(-0.02, 0.02, e.shape)
        par_t = rng.uniform(0.2, 1.0, (n_row, NL)) * (rng.uniform(size=(n_row, NL)) < 0.6)
        par_t[-1] = 0.0
        par_t[-1, :2] = [0.5, 0.9]
        c["kw"].update(dcoeffs=(t(c["da"]), t(c["de"])), par_t=par_t)
    c["kw"]["gas"] = c["gas"]
    # rows of [1 + n_par] that must be exact zeros for the high rays: the LAST level and the LAST row parameter
    c["zero_rows"] = ([n_col + n_lev] if n_lev else []) + ([n_col + n_lev + n_row] if n_row else [])
    return c


def _los(eng, c):
    L = c["L"]
    return eng.LimbLOS(L["seg_off"], L["seg_layer"], L["pt_off"], L["x"], L["nd"], L["vmr"], **c["los_kw"])


def _composed(eng, c, los, bands, widths, units, with_fov, kw=None, coeffs=None, g_lo=0):
    """The route of today: the hi-res state Jacobian, the instrument step on rad and on the flattened jac, numpy FOV."""
    from spectrobot_amd import spect_main_module as smm
    kw = c["kw"] if kw is None else kw
    coeffs = c["coeffs"] if coeffs is None else coeffs
    rad, jac = eng.limb_rays_state_jacobian(coeffs, los, grid=c["grid"], g_lo=g_lo, **kw)
    low = lambda r: eng.hires_to_lowres(r.contiguous(), c["grid"], bands, widths, out_units=units, g_lo=g_lo)
    both = np.concatenate([low(rad)[:, None, :], low(jac.view(los.n_rays * c["n_par"], -1)).reshape(los.n_rays, c["n_par"], -1)], axis=1)
    return smm.fov_closed_form(both[0::3], both[1::3], both[2::3], ROTS) if with_fov else both


def _fused(eng, c, los, bands, widths, units, with_fov, kw=None, coeffs=None, g_lo=0):
    kw = c["kw"] if kw is None else kw
    return eng.limb_rays_state_bands(c["coeffs"] if coeffs is None else coeffs, los, c["grid"], bands, widths, out_units=units,
                                     fov=eng.fov_factors(ROTS) if with_fov else None, g_lo=g_lo, **kw)


def _distance(f, u):
    """max |f - u| / scale, scale = the largest |u| of a quantity row over rays (pixels) and bands; and the scales."""
    scale = np.max(np.abs(u), axis=(0, 2), keepdims=True)
    return float(np.max(np.abs(f - u) / np.where(scale > 0, scale, 1.0))), scale.ravel()


# (n_col, n_lev, n_row), n_gas, n_pts, LOS order, solo_absorption, Planck background, out_units, extra bands
CASES = [
    ((3, 0, 0), 1, 63, "photon", False, False, "Wm2", 0),          # column parameters only; less than a wave
    ((3, 0, 0), 3, 700, "observer", False, False, "ergscm2", 0),
    ((0, 5, 0), 1, 257, "photon", False, False, "Wm2", 0),         # level parameters only: the COLS = false instance
    ((0, 5, 0), 3, 700, "photon", True, True, "Wm2", 0),           # solo_absorption (on a Planck background)
    ((0, 0, 4), 1, 700, "photon", False, True, "Wm2", 0),          # row parameters only; init_mode 2
    ((0, 0, 4), 3, 63, "observer", False, False, "nWcm2", 0),
    ((0, 8, 0), 3, 257, "photon", False, False, "Wm2", 0),         # NP = 8: nine rows
    ((0, 8, 0), 1, 700, "photon", False, False, "Wm2", 0),
    ((0, 16, 0), 1, 257, "photon", False, False, "Wm2", 0),        # NP = 16: seventeen rows
    ((0, 16, 0), 3, 700, "photon", False, False, "Wm2", 30),       # ... and 37 bands: three tiles
    ((0, 17, 0), 3, 257, "observer", False, False, "Wm2", 0),      # two parameter blocks
    ((0, 17, 0), 1, 63, "photon", False, False, "ergscm2", 0),
    ((5, 12, 3), 3, 700, "photon", False, False, "Wm2", 30),       # all three kinds, two parameter blocks
    ((5, 12, 3), 1, 257, "observer", False, True, "nWcm2", 0),
]


@pytest.mark.parametrize("kinds,n_gas,n,order,solo,planck,units,n_extra", CASES)
def test_fused_equals_composed(eng, kinds, n_gas, n, order, solo, planck, units, n_extra):
    """(A) the one call against limb_rays_state_jacobian -> hires_to_lowres -> fov_closed_form, without and with the field
    of view: 1e-12 of a row's largest element; the band outside the grid an exact 0.0 in every row on both routes, and so
    the parameters whose weights live on layers a ray never crosses, for that ray."""
    c = _case(eng, *kinds, n_gas, n, order=order, solo=solo, planck=planck)
    bands, widths = _bands(c["grid"], n_extra, c["rng"])
    los = _los(eng, c)
    for with_fov in (False, True):
        u = _composed(eng, c, los, bands, widths, units, with_fov)
        f = _fused(eng, c, los, bands, widths, units, with_fov)
        assert isinstance(f, np.ndarray) and f.shape == u.shape == ((2 if with_fov else 6), 1 + c["n_par"], bands.size)
        dist, scale = _distance(f, u)
        print("\nstate bands %s n_gas %d n_pts %d %s%s%s %s %d bands fov %d: max |fused - composed| / scale = %.2e (smallest scale %.2e)"
              % (kinds, n_gas, n, order, " solo" if solo else "", " planck" if planck else "", units, bands.size, with_fov, dist,
                 scale.min()))
        assert np.all(f[..., 0] == 0.0) and np.all(u[..., 0] == 0.0)          # the band outside the grid
        assert np.all(scale > 0)                                               # (every row has a ray that reaches it)
        where = np.array([1]) if with_fov else np.flatnonzero(c["high"])       # (pixel 1 = rays 3 .. 5, all of them high)
        for q in c["zero_rows"]:                                               # the designated zeros
            assert np.all(f[where, q] == 0.0) and np.all(u[where, q] == 0.0), q
            assert np.any(f[0, q] != 0.0)
        assert dist <= BOUND, dist
        assert not np.array_equal(f, u) or n <= 256                            # (two routes, not one run twice)


@pytest.mark.parametrize("planck", [False, True])
def test_shards_add_up(eng, planck):
    """(B) n_pts = 300 cut at 130: the tables' slices [0, 131) at g_lo = 0 and [130, 300) at g_lo = 130 -- a shard plus the
    next shard's first point, as sr_hires_to_lowres_shard_dev prescribes -- give partial band integrals that add up to the
    whole-grid call within the bound of (A)."""
    import torch
    c = _case(eng, 2, 5, 3, 3, 300, planck=planck, seed=7)
    bands, widths = _bands(c["grid"], 0, c["rng"])
    los = _los(eng, c)
    t = lambda v: torch.tensor(np.ascontiguousarray(v), device="cuda")

    def part(lo, hi, with_fov):
        kw = dict(c["kw"])
        kw["tab"] = t(c["tab_np"][..., lo:hi])
        kw["dcoeffs"] = (t(c["da"][..., lo:hi]), t(c["de"][..., lo:hi]))
        return _fused(eng, c, los, bands, widths, "Wm2", with_fov, kw=kw, coeffs=(t(c["a"][..., lo:hi]), t(c["e"][..., lo:hi])), g_lo=lo)

    for with_fov in (False, True):
        whole = _fused(eng, c, los, bands, widths, "Wm2", with_fov)
        p0, p1 = part(0, 131, with_fov), part(130, 300, with_fov)
        dist, scale = _distance(p0 + p1, whole)
        d_comp, _ = _distance(whole, _composed(eng, c, los, bands, widths, "Wm2", with_fov))
        print("\nstate bands shards (planck %d, fov %d): max |shard 0 + shard 1 - whole| / scale = %.2e; whole against composed %.2e"
              % (planck, with_fov, dist, d_comp))
        assert np.all(scale > 0) and np.any(p0 != 0.0) and np.any(p1 != 0.0) and not np.array_equal(p0, whole)
        assert dist <= BOUND and d_comp <= BOUND


def test_scratch_and_weight_cache(eng):
    """(C) three calls in a row in one process -- bands set 1 with few parameters, bands set 2 with more parameters and
    points (the scratch grows), bands set 1 again -- each return, bit for bit, what the same call returns on a fresh
    LimbLOS right after an unrelated instrument step has replaced the cached weight table."""
    import torch
    c1 = _case(eng, 2, 0, 0, 1, 257, seed=3)
    c2 = _case(eng, 5, 12, 3, 3, 700, seed=4)
    b1 = _bands(c1["grid"], 0, c1["rng"])
    b2 = _bands(c2["grid"], 30, c2["rng"])
    from spectrobot_amd import synthetic as syn
    other_grid = syn.make_grid(2975.0, 5e-4, 400)
    other = torch.tensor(np.random.default_rng(1).uniform(0, 1, (3, 400)), device="cuda")

    def unrelated():
        lam = 1e7 / other_grid[200]
        eng.hires_to_lowres(other, other_grid, [lam, lam + 0.01], [0.02, 0.03])

    run = lambda c, b, los: _fused(eng, c, los, b[0], b[1], "Wm2", True)
    los1, los2 = _los(eng, c1), _los(eng, c2)
    seq = [run(c1, b1, los1), run(c2, b2, los2), run(c1, b1, los1)]
    ref = []
    for c, b in ((c1, b1), (c2, b2)):
        unrelated()
        ref.append(run(c, b, _los(eng, c)))
    assert np.array_equal(seq[0], ref[0]) and np.array_equal(seq[1], ref[1]) and np.array_equal(seq[2], ref[0])
    assert np.any(seq[0][:, :, 1:] != 0.0) and np.any(seq[1][:, :, 1:] != 0.0)
    # ... and the other way round: the composed route after the fused one finds its own table
    u = _composed(eng, c1, los1, b1[0], b1[1], "Wm2", True)
    assert _distance(seq[2], u)[0] <= BOUND


def test_wrappers_refuse_the_same_shapes(eng):
    """engine.limb_rays_state_bands prepares its arguments with limb_rays_state_jacobian's helper: the same ValueErrors for
    the same bad shapes; and its own for the bands and the field of view."""
    c = _case(eng, 2, 3, 2, 3, 63)
    bands, widths = _bands(c["grid"], 0, c["rng"])
    los = _los(eng, c)
    kw = c["kw"]
    bad = [dict(kw, par_w=kw["par_w"][:, :-1]), dict(kw, par_c=kw["par_c"][:, :-1]), dict(kw, coef_row=kw["coef_row"][:-1]),
           dict(kw, par_t=kw["par_t"][:, :-1]), dict(kw, dcoeffs=(kw["dcoeffs"][0][:, :-1].contiguous(), kw["dcoeffs"][1][:, :-1].contiguous())),
           dict(kw, tab=kw["tab"][..., :-1].contiguous()), dict(kw, tab=None), dict(gas=0),
           dict(gas=0, dcoeffs=kw["dcoeffs"], par_t=np.zeros((0, NL)))]
    for k in bad:
        with pytest.raises(ValueError) as e_jac:
            eng.limb_rays_state_jacobian(c["coeffs"], los, grid=c["grid"], **k)
        with pytest.raises(ValueError) as e_bands:
            eng.limb_rays_state_bands(c["coeffs"], los, c["grid"], bands, widths, **k)
        assert str(e_bands.value) == str(e_jac.value)
    two = (c["coeffs"][0][:2].contiguous(), c["coeffs"][1][:2].contiguous())
    with pytest.raises(ValueError, match="coefficient sets"):
        eng.limb_rays_state_bands(two, los, c["grid"], bands, widths, **kw)
    with pytest.raises(ValueError, match="spectral widths"):
        eng.limb_rays_state_bands(c["coeffs"], los, c["grid"], bands, widths[:-1], **kw)
    with pytest.raises(ValueError, match="fov must be"):
        eng.limb_rays_state_bands(c["coeffs"], los, c["grid"], bands, widths, fov=np.ones((3, 7)), **kw)
    with pytest.raises(ValueError, match="outside the grid"):
        eng.limb_rays_state_bands(c["coeffs"], los, c["grid"], bands, widths, g_lo=1, **kw)


# ------------------------------------------------------------------------------------------------------------------
# (D) the driver
# ------------------------------------------------------------------------------------------------------------------
def _mixed_scene(eng, n_grid=6000, n_layers=22, dT=None):
    """The scene of tests/test_gpu_inversion_state.py at a smaller size: an HCN-like LTE trace gas and a non-LTE CH4 on the
    level-factored route (dT: its tables also at T + dT, for a temperature set)."""
    import bench_configs as bc
    from spectrobot_amd import retrieval, synthetic as syn
    grid = syn.make_grid(3290.0, 5e-4, n_grid)
    Lc = syn.make_lines(1200, grid, config_id=4, n_levels=12)
    Lh = syn.make_lines(300, grid, config_id=5, n_levels=6)
    Lh["a_coeff"] = Lh["a_coeff"] * 30.0
    atm = syn.make_atmosphere(n_layers, 12)
    ch4 = retrieval.LevelGas("CH4", eng.LineSet(Lc, grid, 6, 1, syn.CH4_MM, syn.CH4_LEVEL_ENERGIES), np.full(n_layers, 1.48e-4),
                             atm["tvib"], syn.CH4_ISO_RATIO, **({} if dT is None else {"dT": dT}))
    hcn = retrieval.Gas("HCN", eng.LineSet(Lh, grid, 23, 1, bc.HCN_MM, bc.HCN_LEVEL_ENERGIES), np.full(n_layers, 2e-6),
                        bc.HCN_ISO_RATIO)
    lam_lo, lam_hi = 1e7 / grid[-1], 1e7 / grid[0]
    lam = np.linspace(lam_lo + 0.3, lam_hi - 0.3, 8)
    scene = retrieval.LimbScene(grid, atm["z"], atm["temps"], atm["press"], [hcn, ch4], lam, np.full(8, 0.3))
    z = atm["z"]
    span = z[-1] - z[0]
    pixels = [retrieval.LimbPixel(z[0] + (0.1 + 0.16 * i) * span, fov_half=0.02 * span, pixel_rot=10.0 * (i % 3)) for i in range(5)]
    return scene, pixels


def _observe(scene, pixels, noise_frac):
    from spectrobot_amd import retrieval
    for pix, y in zip(pixels, retrieval.radtrans(scene, pixels)):
        sig = noise_frac * np.abs(y.spectrum).max() * np.ones_like(y.spectrum)
        pix.observation, pix.noise = retrieval.Spectrum(y.spectrum + 0.0, scene.bands_nm), retrieval.Spectrum(sig, scene.bands_nm)


def _twin(eng, with_temp):
    """A noise-free twin as test_noise_free_twin_of_a_mixed_state builds it: observations from a perturbed truth (the HCN
    profile scaled, a bump on the Tvib of CH4 level 5; with_temp: and on the kinetic temperature), the first guess at the
    a priori.  Returns scene, pixels, the BayesSet and its a-priori errors."""
    from spectrobot_amd import retrieval, spect_main_module as smm
    scene, pixels = _mixed_scene(eng, dT=0.05 if with_temp else None)
    z = scene.z
    span = z[-1] - z[0]
    hcn_nodes = [z[0] + f * span for f in (0.1, 0.45, 0.8)]
    tv_nodes = [z[0] + f * span for f in (0.15, 0.4, 0.65, 0.9)]
    t_nodes = [z[0] + f * span for f in (0.2, 0.5, 0.8)]
    apr_hcn, sig_hcn, sig_tv, sig_t = np.full(3, 2.2e-6), np.full(3, 1.1e-6), np.full(4, 4.0), np.full(3, 3.0)
    bump = lambda nodes, amp: amp * np.exp(-0.5 * ((np.array(nodes) - z[0] - 0.45 * span) / (0.25 * span)) ** 2)
    truth, bs = smm.BayesSet(), smm.BayesSet(tag="HCN + Tvib of CH4 level 5" + (" + T" if with_temp else ""))
    truth.add_set(smm.LinearProfile_1D_new("HCN", z, hcn_nodes, apr_hcn, sig_hcn, first_guess_prof=1.3 * apr_hcn))
    truth.add_set(retrieval.TvibProfile("CH4", 5, z, tv_nodes, sig_tv, first_guess=bump(tv_nodes, 6.0)))
    if with_temp:   # (the BayesSet's order is not the call's: the row parameters in the middle)
        bs.add_set(retrieval.TempProfile(z, t_nodes, sig_t))
        truth.add_set(retrieval.TempProfile(z, t_nodes, sig_t, first_guess=bump(t_nodes, 2.0)))
    retrieval._state_into_gases(scene, truth)
    _observe(scene, pixels, 0.004)
    bs.add_set(smm.LinearProfile_1D_new("HCN", z, hcn_nodes, apr_hcn, sig_hcn))
    bs.add_set(retrieval.TvibProfile("CH4", 5, z, tv_nodes, sig_tv))
    sigma = np.array([p.apriori_err for p in bs.params()], dtype=float)
    return scene, pixels, bs, sigma


def _drive(scene, pixels, bs, max_it, fused):
    from spectrobot_amd import retrieval
    chi, _, sims, b = retrieval.inversion_state(scene, copy.deepcopy(bs), pixels, max_it=max_it, bands_in_kernel=fused)
    return b, np.array([s.spectrum for s in sims])


def _one_iteration(scene, pixels, bs, n_par):
    """max_it = 1 on both routes: bayes_set.jacobian and the simulated spectra within the bound of (A)."""
    (bu, su), (bf, sf) = _drive(scene, pixels, bs, 1, False), _drive(scene, pixels, bs, 1, True)
    n_pix, n_b = len(pixels), len(scene.bands_nm)
    assert bu.jacobian.shape == bf.jacobian.shape == (n_pix * n_b, n_par) and su.shape == sf.shape == (n_pix, n_b)
    # as [pixel, quantity, band], the rows of (A): the radiance, then the parameters in BayesSet order
    rows = lambda b, s: np.concatenate([s[:, None, :], np.transpose(b.jacobian.reshape(n_pix, n_b, n_par), (0, 2, 1))], axis=1)
    dist, scale = _distance(rows(bf, sf), rows(bu, su))
    assert np.all(scale > 0)
    return dist, bu, bf


def test_driver_with_the_bands_in_the_kernel(eng):
    """(D) inversion_state(bands_in_kernel=True) against the default on a noise-free mixed twin: after one iteration the
    Jacobian and the simulated spectra within the bound of (A); over the whole loop the same stop, the same number of
    iterations and final parameters within 1e-6 of their a-priori errors (the project's accuracy requirement)."""
    scene, pixels, bs, sigma = _twin(eng, with_temp=False)
    dist, bu, bf = _one_iteration(scene, pixels, bs, 7)
    print("\ninversion_state, bands in the kernel, one iteration: max |fused - composed| / scale over radiance and Jacobian rows = %.2e" % dist)
    assert dist <= BOUND
    (bu, su), (bf, sf) = _drive(scene, pixels, bs, 10, False), _drive(scene, pixels, bs, 10, True)
    diff = np.abs(bf.param_vector() - bu.param_vector()) / sigma
    print("inversion_state, bands in the kernel, whole loop: %d | %d iterations (%s | %s), chi square %.6g -> %.6g | %.6g; final "
          "parameters differ by at most %.2e a-priori sigma" % (len(bu.history), len(bf.history), bu.stop, bf.stop, bu.history[0],
                                                                 bu.history[-1], bf.history[-1], diff.max()))
    assert bf.stop == bu.stop and len(bf.history) == len(bu.history) >= 2 and bu.history[-1] < bu.history[0]
    assert np.all(diff <= 1e-6)


def test_driver_with_a_temperature_set(eng):
    """(D) ... with a TempProfile between the other sets: row parameters pass through the driver (and w.perm is not the
    identity), one iteration."""
    scene, pixels, bs, _ = _twin(eng, with_temp=True)
    assert list(bs.order)[0] == "temp"
    dist, bu, bf = _one_iteration(scene, pixels, bs, 10)
    print("\ninversion_state with T, bands in the kernel, one iteration: max |fused - composed| / scale = %.2e" % dist)
    assert dist <= BOUND
    assert np.allclose(bf.param_vector(), bu.param_vector(), rtol=1e-9, atol=0.0)
