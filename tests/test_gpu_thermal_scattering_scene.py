"""Thermal scattering through the scene and the driver (retrieval.ThermalScattering, LimbScene(thermal_scattering=),
LimbScene.thermal_pass, inversion_state) on the small haze scene of tests/solar_source_cases.py (600 grid points, 12
layers): the default runs the parent's code, the night scene's rows are the engine call's, a Sun(multiple=True) shares the
one diffuse call, a scatterer with albedo 0 is the plain absorber, the frozen-row VMR Jacobian against central differences
and a noise-free night-side twin retrieval of the haze profile."""
import copy

import numpy as np
import pytest

import absorber_table_reference as AR
import solar_source_cases as SC

pytestmark = pytest.mark.gpu
GROUND = 0.3
T_GROUND = 160.0


@pytest.fixture(scope="module")
def eng():
    import torch
    assert torch.cuda.is_available(), "these tests need the GPU"
    from spectrobot_amd import engine
    engine.set_device(0)
    return engine


def _scene(eng, thermal=True, sun=None, albedo=SC.ALBEDO, ground=0.0, t_ground=None):
    """SC.solar_scene's gases in a scene with (thermal=True) a ThermalScattering; sun: None, "single" or "multiple"."""
    from spectrobot_amd import retrieval, geometry
    base = SC.solar_scene(eng, sun=False, albedo=albedo)
    s = None
    if sun is not None:
        s = retrieval.Sun(SC.SZA_DEG, SC.PHASE_DEG, geometry.solar_irradiance(base.grid), multiple=sun == "multiple", surface_albedo=ground)
    ts = retrieval.ThermalScattering(surface_temperature=t_ground, surface_albedo=ground) if thermal else None
    return retrieval.LimbScene(base.grid, base.z, base.temps, base.press, base.gases, base.bands_nm, base.widths_nm, sun=s,
                               thermal_scattering=ts)


def _pixels(scene):
    from spectrobot_amd import retrieval
    span = scene.z[-1] - scene.z[0]
    return [retrieval.LimbPixel(scene.z[0] + (0.03 + 0.09 * i) * span, fov_half=0.01 * span, pixel_rot=10.0 * (i % 3)) for i in range(6)]


def _spectra(scene, pixels):
    from spectrobot_amd import retrieval
    return np.array([y.spectrum for y in retrieval.radtrans(scene, sorted(pixels, key=lambda p: p.limb_tg_alt))])


def _stack(scene):
    import torch
    return torch.stack([(g.thermal if getattr(g, "solar", None) is not None else g.coeffs)[0] for g in scene.gases]).contiguous()


def test_the_default_gives_the_parents_radiances_bit_for_bit(eng):
    for sun in (False, True):
        plain = SC.solar_scene(eng, sun=sun)                       # (built without the argument)
        same = _scene(eng, thermal=False, sun="single" if sun else None)
        assert same.thermal_scattering is None
        pixels = _pixels(plain)
        a, b = _spectra(plain, pixels), _spectra(same, pixels)
        assert np.array_equal(a.view(np.uint64), b.view(np.uint64))
        haze = same.gas("haze")
        assert (haze.coeffs is haze.thermal) == (not sun)           # no pass at night, the solar pass with a sun


def test_the_night_scenes_rows_are_the_engine_calls(eng):
    import torch
    from spectrobot_amd import geometry
    scene = _scene(eng, ground=GROUND, t_ground=T_GROUND)
    scene.coefficients()
    haze = scene.gas("haze")
    assert haze.coeffs is not haze.thermal and haze.coeffs[0] is haze.thermal[0]
    A = _stack(scene)
    V = geometry.vertical_columns(scene.z, scene.nd, [g.vmr for g in scene.gases], R=scene.R, n_sub=scene.n_sub,
                                  col_scale=[float(g.iso_ratio) for g in scene.gases])
    rows = eng.diffuse_thermal_source(A, V, [0.0, SC.ALBEDO], [0.0, SC.ASYMMETRY], scene.temps, scene.grid, t_surface=T_GROUND,
                                      surface_albedo=GROUND, out_gas=1, own_emission=True)
    assert float(rows.min()) > 0.0 and torch.equal(haze.coeffs[1], rows)
    # more than the gas's own emission (1 - albedo) abs B: the scattered field is there (it may pass abs B where warmer
    # layers or the surface light a cold one)
    assert bool((rows > (1.0 - SC.ALBEDO) * haze.thermal[1]).all())
    # a second call makes nothing again; a moved temperature does
    before = haze.coeffs[1]
    scene.coefficients()
    assert haze.coeffs[1] is before
    scene.temps = scene.temps + 1.0
    scene.coefficients()
    assert haze.coeffs[1] is not before


def test_one_diffuse_call_serves_the_sun_and_the_thermal_source(eng, monkeypatch):
    import torch
    from spectrobot_amd import geometry
    scene = _scene(eng, sun="multiple", ground=GROUND, t_ground=T_GROUND)
    calls = dict(thermal=[], solar=0)
    real_thermal, real_solar = eng.diffuse_thermal_source, eng.diffuse_source

    def thermal(*a, **kw):
        calls["thermal"].append((a, dict(kw)))
        return real_thermal(*a, **kw)

    def solar(*a, **kw):
        calls["solar"] += 1
        return real_solar(*a, **kw)

    monkeypatch.setattr(eng, "diffuse_thermal_source", thermal)
    monkeypatch.setattr(eng, "diffuse_source", solar)
    scene.coefficients()
    assert len(calls["thermal"]) == 1 and calls["solar"] == 0
    a, kw = calls["thermal"][0]
    assert kw["beam"] is not None and kw["sun"] is not None and kw["mu0"] == scene.sun.mu and kw["own_emission"] and kw["accumulate"]
    scene.coefficients()                                            # nothing moved: no pass
    assert len(calls["thermal"]) == 1
    scene.gas("haze").add_clim(1.1 * np.asarray(scene.gas("haze").vmr))
    scene.coefficients()                                            # a moved VMR: one pass, one call
    assert len(calls["thermal"]) == 2 and calls["solar"] == 0
    monkeypatch.undo()
    # the rows: order one plus that call's rows
    haze = scene.gas("haze")
    A = _stack(scene)
    U, lit = geometry.solar_columns(scene.z, scene.nd, [g.vmr for g in scene.gases], scene.shell_midpoints(), scene.sun.mu, R=scene.R,
                                    n_sub=scene.n_sub, col_scale=[g.iso_ratio for g in scene.gases])
    sun = torch.as_tensor(scene.sun.irradiance, device="cuda").contiguous()
    single = eng.solar_source(A, U, scene.solar_weights(haze, lit), haze.thermal[0], sun)
    V, ssa, asym, beam = scene.diffuse_inputs([haze], A, sun)
    rows = eng.diffuse_thermal_source(A, V, ssa, asym, scene.temps, scene.grid, t_surface=T_GROUND, beam=beam, sun=sun, mu0=scene.sun.mu,
                                      surface_albedo=GROUND, out_gas=1, own_emission=True)
    assert float(single.min()) >= 0.0 and float(rows.min()) > 0.0
    assert torch.equal(haze.coeffs[1], single + rows)


@pytest.mark.parametrize("sunlit", [False, True])
def test_two_scatterers_share_one_solve(eng, sunlit, monkeypatch):
    """Several scatterers: one diffuse_thermal_source call for J (no rows), then per gas (1 - albedo) times its cached abs B
    and an addcmul of J with the weights of the gas's own slot.  Each gas's rows are the fused own_emission call's for
    that gas (plus order one under the sun) within the Planck allowance eps (8 + 2 x) of the rows -- the same B, the sum
    formed in another order -- and, under the sun, 4 eps of the whole row for the order-one rows taken off again."""
    import torch
    from spectrobot_amd import retrieval, geometry
    base = SC.solar_scene(eng, sun=False)
    ch4, haze = base.gases
    fine = retrieval.TableGas("fine", haze.table, 0.4 * haze.vmr, solar=dict(albedo=0.6, g=-0.2))
    s = retrieval.Sun(SC.SZA_DEG, SC.PHASE_DEG, geometry.solar_irradiance(base.grid), multiple=True, surface_albedo=GROUND) if sunlit else None
    scene = retrieval.LimbScene(base.grid, base.z, base.temps, base.press, [ch4, haze, fine], base.bands_nm, base.widths_nm, sun=s,
                                thermal_scattering=retrieval.ThermalScattering(T_GROUND, GROUND))
    scene.keep_solar_rows = True
    calls = []
    real = eng.diffuse_thermal_source
    monkeypatch.setattr(eng, "diffuse_thermal_source", lambda *a, **kw: calls.append(dict(kw)) or real(*a, **kw))
    scene.coefficients()
    monkeypatch.undo()
    assert len(calls) == 1 and calls[0].get("mean_intensity") and calls[0].get("out_gas") is None
    A = _stack(scene)
    ssa, asym = np.array([0.0, SC.ALBEDO, 0.6]), np.array([0.0, SC.ASYMMETRY, -0.2])
    kw = dict(t_surface=T_GROUND, surface_albedo=GROUND)
    if sunlit:
        sun = torch.as_tensor(scene.sun.irradiance, device="cuda").contiguous()
        V, ssa_s, asym_s, beam = scene.diffuse_inputs([haze, fine], A, sun)
        assert np.all(ssa_s == ssa) and np.all(asym_s == asym)
        kw.update(beam=beam, sun=sun, mu0=scene.sun.mu)
    else:
        V = geometry.vertical_columns(scene.z, scene.nd, [g.vmr for g in scene.gases], R=scene.R, n_sub=scene.n_sub,
                                      col_scale=[float(g.iso_ratio) for g in scene.gases])
    x = AR.C2 * scene.grid.max() / scene.temps.min()
    for i, g in ((1, haze), (2, fine)):
        rows = eng.diffuse_thermal_source(A, V, ssa, asym, scene.temps, scene.grid, out_gas=i, own_emission=True, **kw)
        assert float(rows.min()) > 0.0 and g.coeffs[1] is not g.thermal[1]
        got = g.coeffs[1] - g.solar_rows if sunlit else g.coeffs[1]
        tol = AR.EPS * (8 + 2 * x) * rows + (4 * AR.EPS * g.coeffs[1].abs() if sunlit else 0.0)
        worst = float(((got - rows).abs() / tol).max())
        print("\ntwo scatterers, %s, %s: |scene - fused call| / allowance %.3f" % ("sunlit" if sunlit else "night", g.name, worst))
        assert worst <= 1.0, g.name


def test_a_scatterer_with_albedo_0_is_the_plain_absorber(eng):
    """albedo = 0: the rows are A ((1 - 0) B + 0 J) = A B, the table's own emission up to the two kernels' Planck values:
    the band radiances agree within twice the absorber-table reference's allowance for one, eps (8 + 2 x), at the
    scene's largest x."""
    dark = _scene(eng, albedo=0.0)
    none = SC.solar_scene(eng, sun=False, albedo=0.0)
    pixels = _pixels(none)
    a, b = _spectra(dark, pixels), _spectra(none, pixels)
    haze = dark.gas("haze")
    assert haze.coeffs is not haze.thermal                          # the pass ran
    x = AR.C2 * dark.grid.max() / dark.temps.min()
    worst = float(np.max(np.abs(a - b) / np.abs(b)))
    print("\nalbedo 0 against the plain absorber: largest relative difference of a band radiance %.2e (allowance %.2e)"
          % (worst, 2 * AR.EPS * (8 + 2 * x)))
    assert np.all(b > 0) and worst <= 2 * AR.EPS * (8 + 2 * x)


def _night_twin(eng, noise=0.004):
    """The haze profile's noise-free twin on the night side: CH4 at its truth, the haze's three nodes retrieved."""
    from spectrobot_amd import retrieval, spect_main_module as smm
    import absorber_table_cases as K
    scene = _scene(eng, ground=GROUND, t_ground=T_GROUND)
    z = scene.z
    _, haze_nodes, _ = K.nodes(z)
    apr = SC.HAZE_SCALE * np.array([0.7, 0.45, 0.2])
    sig = 0.5 * apr
    truth = SC.HAZE_SCALE * np.array([1.0, 0.55, 0.14])
    pixels = _pixels(scene)

    def bayes(values=apr):
        bs = smm.BayesSet(tag="night-side haze")
        bs.add_set(smm.LinearProfile_1D_new("haze", z, haze_nodes, apr, sig, first_guess_prof=values))
        return bs

    retrieval._state_into_gases(scene, bayes(truth))
    for pix, y in zip(pixels, retrieval.radtrans(scene, pixels)):
        s = noise * np.abs(y.spectrum).max() * np.ones_like(y.spectrum)
        pix.observation, pix.noise = retrieval.Spectrum(y.spectrum.copy(), scene.bands_nm), retrieval.Spectrum(s, scene.bands_nm)
    return scene, pixels, bayes, truth, sig


def test_frozen_row_jacobian_against_central_differences(eng):
    """The criterion of the scene tests (tests/test_gpu_scene_diffuse.py), with the thermal rows frozen as the Jacobian
    holds them: |K - FD(h/2)| <= 2 |FD(h) - FD(h/2)| + 1e-9 max|K| per column."""
    from spectrobot_amd import retrieval
    scene, pixels, bayes, _, _ = _night_twin(eng)
    bs = bayes()
    x0 = bs.param_vector().copy()
    _, _, _, b = retrieval.inversion_state(scene, copy.deepcopy(bs), pixels, max_it=1)
    K1 = np.array(b.jacobian)
    retrieval._state_into_gases(scene, bayes())      # back to the first guess
    scene.coefficients()                             # ... and its thermal rows, which stay from here on
    scene.solar_frozen = True
    order = sorted(pixels, key=lambda p: p.limb_tg_alt)
    prof0 = bayes().sets["haze"].profile()
    masks = [np.asarray(par.maskgrid.mask, float) for par in bs.sets["haze"].set]

    def forward(prof):
        scene.gas("haze").add_clim(prof)
        return np.concatenate([y.spectrum for y in retrieval.radtrans(scene, order)])

    for k in range(3):
        fd = [(forward(prof0 + h * masks[k]) - forward(prof0 - h * masks[k])) / (2.0 * h) for h in (0.02 * x0[k], 0.01 * x0[k])]
        col = K1[:, k]
        jm = np.abs(col).max()
        trunc, err = np.abs(fd[0] - fd[1]).max(), np.abs(col - fd[1]).max()
        print("\nnight twin FD, haze node %d: max|K| %.3e, |K - FD(h/2)| / max|K| %.2e, |FD(h) - FD(h/2)| / max|K| %.2e"
              % (k, jm, err / jm, trunc / jm))
        assert jm > 0 and err <= 2.0 * trunc + 1e-9 * jm
    scene.gas("haze").add_clim(prof0)


def test_night_side_twin_retrieval_of_the_haze(eng):
    """The Jacobians hold the thermal rows fixed, so the loop converges linearly; the loop's own rule has to end it within
    max_it, and the truth lies inside the posterior errors (the square roots of the stored covariance's diagonal)."""
    from spectrobot_amd import retrieval
    scene, pixels, bayes, x_true, sigma = _night_twin(eng)
    bs = bayes()
    x0 = bs.param_vector().copy()
    chi, _, sims, b = retrieval.inversion_state(scene, bs, pixels, max_it=20, lambda_LM=0.0)
    hist = np.array(b.history)
    post = np.sqrt(np.diag(b.VCM))
    x = b.param_vector()
    print("\nnight-side haze twin: %d iterations (%s), chi square %s;\n  retrieved %s\n  truth     %s\n  posterior errors %s, |x - truth| / posterior error %s"
          % (len(hist), b.stop, np.array2string(hist, precision=4), np.array2string(x, precision=4), np.array2string(x_true, precision=4),
             np.array2string(post, precision=3), np.array2string(np.abs(x - x_true) / post, precision=3)))
    assert b.stop in ("converged", "raised") and len(hist) < 20           # the loop's own rule, not max_it
    assert len(hist) >= 2 and hist[-1] < hist[0]
    assert np.linalg.norm((x - x_true) / sigma) < np.linalg.norm((x0 - x_true) / sigma)
    assert np.all(np.abs(x - x_true) <= post)
