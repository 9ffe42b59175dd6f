"""Multiple scattering in the scene (retrieval.Sun(multiple=True), LimbScene.solar_pass, engine.diffuse_source) on the
sunlit haze scene of tests/solar_source_cases.py: what stays bit for bit, what the emission rows are made of, the frozen-row
Jacobian against central differences and a twin retrieval whose observations carry the diffuse light."""
import copy

import numpy as np
import pytest

import solar_source_cases as SC

pytestmark = pytest.mark.gpu
GROUND = 0.3        # the Lambertian albedo below z[0] in these tests


@pytest.fixture(scope="module")
def eng():
    import torch
    assert torch.cuda.is_available(), "these tests need the GPU"
    from spectrobot_amd import engine
    engine.set_device(0)
    return engine


def _sun(scene, **kw):
    from spectrobot_amd import retrieval
    return retrieval.Sun(SC.SZA_DEG, SC.PHASE_DEG, scene.sun.irradiance, **kw)


def _pixels(scene):
    from spectrobot_amd import retrieval
    z = scene.z
    return [retrieval.LimbPixel(z[0] + f * (z[-1] - z[0]), fov_half=2.0) for f in (0.05, 0.3, 0.6)]


def _spectra(scene, pixels):
    from spectrobot_amd import retrieval
    return np.array([y.spectrum for y in retrieval.radtrans(scene, pixels)])


def test_single_scattering_is_untouched_and_a_dark_scatterer_sees_no_sun(eng):
    plain = SC.solar_scene(eng)
    pixels = _pixels(plain)
    want = _spectra(plain, pixels)
    same = SC.solar_scene(eng)
    same.sun = _sun(same, multiple=False, surface_albedo=0.7)      # the albedo is read with multiple=True only
    assert np.array_equal(_spectra(same, pixels).view(np.uint64), want.view(np.uint64))
    # albedo 0 of the scatterer: neither order one nor the diffuse rows add anything -- the scene without a sun
    dark = SC.solar_scene(eng, albedo=0.0)
    dark.sun = _sun(dark, multiple=True, surface_albedo=GROUND)
    none = SC.solar_scene(eng, sun=False)
    assert np.array_equal(_spectra(dark, pixels).view(np.uint64), _spectra(none, pixels).view(np.uint64))
    haze = dark.gas("haze")
    assert haze.coeffs is not haze.thermal and haze.coeffs[1] is not haze.thermal[1]      # the passes ran, on a copy
    # with the albedo the diffuse light is there: more light at every point
    multi = SC.solar_scene(eng)
    multi.sun = _sun(multi, multiple=True, surface_albedo=GROUND)
    more = _spectra(multi, pixels)
    assert np.all(more >= want) and np.any(more > want)
    print("\nmultiple / single scattering, band by band: %s" % np.array2string(more / want, precision=3))


def test_emission_rows_are_thermal_plus_single_plus_diffuse(eng):
    import torch
    for keep in (True, False):
        scene = SC.solar_scene(eng)
        scene.sun = _sun(scene, multiple=True, surface_albedo=GROUND)
        scene.keep_solar_rows = keep
        scene.coefficients()
        haze = scene.gas("haze")
        if keep:
            single = haze.solar_rows                # (the single-scattered part alone, as 4.11a takes it)
        else:
            ref = SC.solar_scene(eng)
            ref.keep_solar_rows = True
            ref.coefficients()
            single = ref.gas("haze").solar_rows
        A = torch.stack([(g.thermal if g is haze else g.coeffs)[0] for g in scene.gases]).contiguous()
        sun = torch.as_tensor(scene.sun.irradiance, device="cuda").contiguous()
        V, ssa, asym, beam = scene.diffuse_inputs([haze], A, sun)
        assert np.all(ssa == [0.0, SC.ALBEDO]) and np.all(asym == [0.0, SC.ASYMMETRY]) and beam.shape == (len(scene.z) + 1, len(scene.grid))
        assert float(beam.min()) > 0.0 and float(beam.max()) <= 1.0
        diffuse = eng.diffuse_source(A, V, ssa, asym, beam, sun, scene.sun.mu, surface_albedo=GROUND, out_gas=1)
        assert float(diffuse.min()) > 0.0
        want = (haze.thermal[1] + single) + diffuse
        assert torch.equal(haze.coeffs[1], want)
        if keep:
            assert torch.equal(haze.solar_rows, single) and haze.coeffs[0] is haze.thermal[0]


def test_two_scatterers_share_one_mean_intensity(eng):
    """Several solar gases: one diffuse_source call for J and an addcmul per gas.  Each gas's rows are the fused call's for
    that gas to the roundings of w (A J) formed in another order: 4 eps of the diffuse rows."""
    import torch
    from spectrobot_amd import retrieval
    base = SC.solar_scene(eng)
    ch4, haze = base.gases
    fine = retrieval.TableGas("fine", haze.table, 0.4 * haze.vmr, solar=dict(albedo=0.6, g=-0.2))
    scene = retrieval.LimbScene(base.grid, base.z, base.temps, base.press, [ch4, haze, fine], base.bands_nm, base.widths_nm,
                                sun=_sun(base, multiple=True, surface_albedo=GROUND))
    scene.keep_solar_rows = True
    scene.coefficients()
    A = torch.stack([ch4.coeffs[0], haze.thermal[0], fine.thermal[0]]).contiguous()
    sun = torch.as_tensor(scene.sun.irradiance, device="cuda").contiguous()
    V, ssa, asym, beam = scene.diffuse_inputs([haze, fine], A, sun)
    assert np.all(ssa == [0.0, SC.ALBEDO, 0.6]) and np.all(asym == [0.0, SC.ASYMMETRY, -0.2])
    for i, g in ((1, haze), (2, fine)):
        rows = eng.diffuse_source(A, V, ssa, asym, beam, sun, scene.sun.mu, surface_albedo=GROUND, out_gas=i)
        got = g.coeffs[1] - (g.thermal[1] + g.solar_rows)
        assert float(rows.min()) > 0.0
        scale = g.coeffs[1].abs()
        assert bool(((got - rows).abs() <= 4 * 2.0 ** -53 * (rows + 2 * scale)).all()), g.name


def _multi_twin(eng, multiple=True, ground=GROUND):
    """SC.solar_twin with observations simulated under Sun(multiple=True, surface_albedo=ground); the scene that is
    returned has the sun asked for."""
    from spectrobot_amd import retrieval
    scene, pixels, bayes, x_true, sigma = SC.solar_twin(eng)
    scene.sun = _sun(scene, multiple=True, surface_albedo=ground)
    retrieval._state_into_gases(scene, bayes({"CH4": x_true[:3], "haze": x_true[3:]}))
    for pix, y in zip(pixels, retrieval.radtrans(scene, pixels)):
        s = 0.004 * np.abs(y.spectrum).max() * np.ones_like(y.spectrum)
        pix.observation, pix.noise = retrieval.Spectrum(y.spectrum.copy(), scene.bands_nm), retrieval.Spectrum(s, scene.bands_nm)
    if not multiple:
        scene.sun = _sun(scene)
    return scene, pixels, bayes, x_true, sigma


def test_state_jacobian_against_central_differences(eng):
    """The criterion of tests/test_gpu_solar_source.py's own test, with the diffuse rows among the frozen ones:
    |K - FD(h/2)| <= 2 |FD(h) - FD(h/2)| + 1e-9 max|K|."""
    from spectrobot_amd import retrieval
    scene, pixels, bayes, _, sigma = _multi_twin(eng)
    bs = bayes()
    x0 = bs.param_vector().copy()
    _, _, _, b = retrieval.inversion_state(scene, copy.deepcopy(bs), pixels, max_it=1)
    K1 = np.array(b.jacobian)
    retrieval._state_into_gases(scene, bayes())      # back to the first guess
    scene.coefficients()                             # ... and its solar rows, which stay from here on
    scene.solar_frozen = True
    order = sorted(pixels, key=lambda p: p.limb_tg_alt)

    def forward(name, prof):
        scene.gas(name).add_clim(prof)
        return np.concatenate([y.spectrum for y in retrieval.radtrans(scene, order)])

    col_at = 0
    for name in ("CH4", "haze"):
        prof0 = bayes().sets[name].profile()
        masks = [np.asarray(par.maskgrid.mask, float) for par in bs.sets[name].set]
        for k in range(3):
            fd = []
            for h in (0.02 * x0[col_at], 0.01 * x0[col_at]):
                fd.append((forward(name, prof0 + h * masks[k]) - forward(name, prof0 - h * masks[k])) / (2.0 * h))
            col = K1[:, col_at]
            jm = np.abs(col).max()
            trunc, err = np.abs(fd[0] - fd[1]).max(), np.abs(col - fd[1]).max()
            print("\nmultiple-scattering twin FD, %s node %d: max|K| %.3e, |K - FD(h/2)| / max|K| %.2e, |FD(h) - FD(h/2)| / max|K| %.2e"
                  % (name, k, jm, err / jm, trunc / jm))
            assert jm > 0 and err <= 2.0 * trunc + 1e-9 * jm
            col_at += 1
        scene.gas(name).add_clim(prof0)


def test_twin_retrieval_with_and_without_the_diffuse_light(eng):
    """The scene's grid starts above the ground: surface_albedo = 0, as Sun's docstring says.  The Jacobians hold the
    diffuse rows fixed, so the loop converges linearly, at the rate of the share of the light whose derivative is left
    out; max_it leaves it room, and the loop's own rule has to end it."""
    from spectrobot_amd import retrieval
    scene, pixels, bayes, x_true, sigma = _multi_twin(eng, ground=0.0)
    bs = bayes()
    x0 = bs.param_vector().copy()
    chi, _, sims, b = retrieval.inversion_state(scene, bs, pixels, max_it=20, lambda_LM=0.0)
    hist = np.array(b.history)
    d0, d1 = np.abs(x0 - x_true) / sigma, np.abs(b.param_vector() - x_true) / sigma
    print("\nmultiple-scattering twin: %d iterations (%s), chi square %s;\n  distance in a-priori sigmas, first guess %s -> retrieved %s"
          % (len(hist), b.stop, np.array2string(hist, precision=4), np.array2string(d0, precision=3), np.array2string(d1, precision=3)))
    assert b.stop in ("converged", "raised") and len(hist) < 20           # the loop's own rule, not max_it
    assert len(hist) >= 2 and np.all(np.diff(hist[:-1]) < 0)               # chi square falls in every accepted iteration
    if b.stop == "converged":
        assert hist[-1] < hist[0]
    for sl, name in ((slice(0, 3), "CH4"), (slice(3, 6), "haze")):
        assert np.linalg.norm(d1[sl]) < np.linalg.norm(d0[sl]), name
    # the same observations fitted with order one alone: the missing light cannot be fitted away
    scene1, pixels1, bayes1, _, _ = _multi_twin(eng, multiple=False, ground=0.0)
    _, _, _, b1 = retrieval.inversion_state(scene1, bayes1(), pixels1, max_it=20, lambda_LM=0.0)
    hist1 = np.array(b1.history)
    d2 = np.abs(b1.param_vector() - x_true) / sigma
    print("fitted with single scattering alone: %d iterations (%s), chi square %s, distance %s"
          % (len(hist1), b1.stop, np.array2string(hist1, precision=4), np.array2string(d2, precision=3)))
    assert hist1.min() > hist.min()
