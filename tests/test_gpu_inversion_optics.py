"""Haze optics in the state through the scene and the driver (retrieval.HazeOptics, LimbScene.optics_jacobian,
inversion_state with a set named "optics") on the sunlit haze scene of tests/solar_source_cases.py under
Sun(multiple=True, surface_albedo=0.3): every optics column against central differences of the whole forward model on
both routes, the two routes against each other, a BayesSet without the set bit for bit with the new scene attribute
forced on, the surface-albedo twin, and the haze's albedo beside a CH4 profile."""
import copy

import numpy as np
import pytest

import solar_source_cases as SC

pytestmark = pytest.mark.gpu
GROUND = 0.3


@pytest.fixture(scope="module")
def eng():
    import torch
    assert torch.cuda.is_available(), "these tests need the GPU"
    from spectrobot_amd import engine
    engine.set_device(0)
    return engine


def _multi_twin(eng, ground=GROUND, noise=0.004):
    """SC.solar_twin under Sun(multiple=True, surface_albedo=ground), its observations simulated with that sun at the truth;
    the scene is left at the truth."""
    from spectrobot_amd import retrieval
    scene, pixels, bayes, x_true, sigma = SC.solar_twin(eng)
    scene.sun = retrieval.Sun(SC.SZA_DEG, SC.PHASE_DEG, scene.sun.irradiance, multiple=True, surface_albedo=ground)
    retrieval._state_into_gases(scene, bayes({"CH4": x_true[:3], "haze": x_true[3:]}))
    for pix, y in zip(pixels, retrieval.radtrans(scene, pixels)):
        s = noise * np.abs(y.spectrum).max() * np.ones_like(y.spectrum)
        pix.observation, pix.noise = retrieval.Spectrum(y.spectrum.copy(), scene.bands_nm), retrieval.Spectrum(s, scene.bands_nm)
    return scene, pixels, bayes, x_true, sigma


def _first_jacobian(retrieval, scene, bs, pixels, **kw):
    _, _, _, b = retrieval.inversion_state(scene, copy.deepcopy(bs), pixels, max_it=1, **kw)
    retrieval._state_into_gases(scene, copy.deepcopy(bs))        # back to the first guess, the optics included
    return np.array(b.jacobian)


def _with_optics(retrieval, bs, **kw):
    bs.add_set(retrieval.HazeOptics(**kw))
    return bs


def test_optics_columns_against_central_differences_on_both_routes(eng):
    """|K - FD(h/2)| <= 2 |FD(h) - FD(h/2)| + 1e-9 max|K| for every optics column (the haze's albedo and g, the surface
    albedo) of inversion_state's Jacobian, hi-res route and bands_in_kernel: the differences change the value in the scene
    and redo the solar and the diffuse pass.  The two routes agree to the band sums' order, 1e-12 of the column's maximum."""
    from spectrobot_amd import retrieval
    scene, pixels, bayes, _, _ = _multi_twin(eng)
    bs = _with_optics(retrieval, bayes(), albedo={"haze": (SC.ALBEDO, 0.1)}, g={"haze": (SC.ASYMMETRY, 0.1)}, surface_albedo=(GROUND, 0.1))
    K_hi = _first_jacobian(retrieval, scene, bs, pixels)
    K_band = _first_jacobian(retrieval, scene, bs, pixels, bands_in_kernel=True)
    assert K_hi.shape[1] == 9
    scale = np.abs(K_hi).max(axis=0, keepdims=True)
    worst = float(np.max(np.abs(K_hi - K_band) / scale))
    print("\noptics state, hi-res route against bands_in_kernel: largest difference / column maximum %.2e" % worst)
    assert worst <= 1e-12
    order = sorted(pixels, key=lambda p: p.limb_tg_alt)
    haze = scene.gas("haze")

    def forward(kind, v):
        if kind == "surface_albedo":
            scene.sun.surface_albedo = v
        else:
            haze.solar[kind] = v
        return np.concatenate([y.spectrum for y in retrieval.radtrans(scene, order)])

    for at, (kind, x0) in enumerate((("albedo", SC.ALBEDO), ("g", SC.ASYMMETRY), ("surface_albedo", GROUND))):
        fd = [(forward(kind, x0 + h) - forward(kind, x0 - h)) / (2.0 * h) for h in (0.02, 0.01)]
        forward(kind, x0)
        trunc = np.abs(fd[0] - fd[1]).max()
        for route, K in (("hi-res", K_hi), ("bands", K_band)):
            col = K[:, 6 + at]
            jm, err = np.abs(col).max(), np.abs(col - fd[1]).max()
            print("\noptics twin FD, %s, %s route: max|K| %.3e, |K - FD(h/2)| / max|K| %.2e, |FD(h) - FD(h/2)| / max|K| %.2e"
                  % (kind, route, jm, err / jm, trunc / jm))
            assert jm > 0 and err <= 2.0 * trunc + 1e-9 * jm, (kind, route, err / (2.0 * trunc + 1e-9 * jm))


def test_single_scattering_has_the_direct_part_alone_and_refuses_the_ground(eng):
    from spectrobot_amd import retrieval
    scene, pixels, bayes, x_true, _ = SC.solar_twin(eng)
    bs = _with_optics(retrieval, bayes(), albedo={"haze": (SC.ALBEDO, 0.1)}, g={"haze": (SC.ASYMMETRY, 0.1)})
    K = _first_jacobian(retrieval, scene, bs, pixels)
    order = sorted(pixels, key=lambda p: p.limb_tg_alt)
    haze = scene.gas("haze")
    for at, (kind, x0) in enumerate((("albedo", SC.ALBEDO), ("g", SC.ASYMMETRY))):
        fd = []
        for h in (0.02, 0.01):
            y = []
            for s in (1.0, -1.0):
                haze.solar[kind] = x0 + s * h
                y.append(np.concatenate([v.spectrum for v in retrieval.radtrans(scene, order)]))
            fd.append((y[0] - y[1]) / (2.0 * h))
        haze.solar[kind] = x0
        col = K[:, 6 + at]
        assert np.abs(col).max() > 0 and np.abs(col - fd[1]).max() <= 2.0 * np.abs(fd[0] - fd[1]).max() + 1e-9 * np.abs(col).max()
    with pytest.raises(ValueError, match="surface_albedo"):
        retrieval.inversion_state(scene, _with_optics(retrieval, bayes(), surface_albedo=(0.3, 0.1)), pixels, max_it=1)


def test_without_the_set_nothing_changes_bit_for_bit(eng):
    """Two runs of a BayesSet without the set, one with the new scene attribute (and the state it needs) forced on: equal
    bits of the history and of every column -- the emission rows of the diffuse pass with mean_intensity=True are the rows
    without it."""
    import torch
    from spectrobot_amd import retrieval
    runs = []
    for forced in (False, True):
        scene, pixels, bayes, _, _ = _multi_twin(eng)
        scene.keep_mean_intensity = forced
        scene._solar_key = None
        _, _, _, b = retrieval.inversion_state(scene, bayes(), pixels, max_it=2, lambda_LM=0.0, solar_attenuation=True, diffuse_jacobian=True)
        runs.append((np.array(b.history), np.array(b.jacobian), scene.gas("haze").coeffs[1].clone(), scene.diffuse_J))
    assert runs[0][3] is None and runs[1][3] is not None
    assert np.array_equal(runs[0][0].view(np.uint64), runs[1][0].view(np.uint64))
    assert np.array_equal(runs[0][1].view(np.uint64), runs[1][1].view(np.uint64))
    assert torch.equal(runs[0][2], runs[1][2])


def test_surface_albedo_twin(eng):
    """The example at test size.  Scene and noise-free observations from surface_albedo = 0.3; the state is the haze
    profile's nodes plus surface_albedo, a priori and first guess 0.1 with a-priori error 0.1, lambda_LM = 0 (chosen on the
    GPU so that the assertions hold with room: six iterations to chi square 3.7e-4, albedo 0.29927 +- 0.0066, against 52.18
    with the albedo held; an error of 0.05 converges alike, 0.3 reaches chi square 1e-5 and ends as `raised` on its last
    digit, the damped loop (lambda_LM = 0.1) runs into max_it; CH4 stays at the truth).  The loop stops as converged, the retrieved albedo lies within one
    a-posteriori sigma of 0.3, and the same observations with the albedo held at 0.1 (no "optics" set) end at a larger
    chi square.  Both chi squares and iteration counts are printed (DESIGN.md 4.11d records them)."""
    from spectrobot_amd import retrieval, spect_main_module as smm
    out = {}
    for fitted in (True, False):
        scene, pixels, bayes, _, _ = _multi_twin(eng)
        full = bayes()
        bs = smm.BayesSet(tag="haze + ground")
        bs.add_set(full.sets["haze"])
        scene.sun.surface_albedo = 0.1
        if fitted:
            bs.add_set(retrieval.HazeOptics(surface_albedo=(0.1, 0.1, 0.1)))
        _, _, _, b = retrieval.inversion_state(scene, bs, pixels, max_it=20, lambda_LM=0.0)
        out[fitted] = (b.stop, np.array(b.history), scene.sun.surface_albedo, np.sqrt(np.diag(b.VCM)))
        print("\nsurface-albedo twin, albedo %s: %d iterations (%s), chi square %s, albedo %.6f, a-posteriori sigmas %s"
              % ("fitted" if fitted else "held at 0.1", len(out[fitted][1]), b.stop, np.array2string(out[fitted][1], precision=6),
                 out[fitted][2], np.array2string(out[fitted][3], precision=3)))
    stop, hist, alb, sig = out[True]
    assert stop == "converged"
    assert abs(alb - 0.3) <= sig[-1], (alb, sig[-1])
    assert out[False][1][-1] > hist[-1]
    assert out[False][2] == 0.1


def test_haze_albedo_beside_a_ch4_profile(eng):
    """The haze's single-scattering albedo beside the CH4 profile, the haze profile fixed at the truth (with the haze's
    profile in the state too, ssa x extinction is nearly one number: DESIGN.md 4.11d): first guess 0.8, truth 0.9."""
    from spectrobot_amd import retrieval, spect_main_module as smm
    scene, pixels, bayes, _, _ = _multi_twin(eng)
    bs = smm.BayesSet(tag="CH4 + haze albedo")
    bs.add_set(bayes().sets["CH4"])
    bs.add_set(retrieval.HazeOptics(albedo={"haze": (0.8, 0.2, 0.8)}))
    _, _, _, b = retrieval.inversion_state(scene, bs, pixels, max_it=20, lambda_LM=0.0, solar_attenuation=True, diffuse_jacobian=True)
    alb, sig = scene.gas("haze").solar["albedo"], float(np.sqrt(b.VCM[-1, -1]))
    print("\nCH4 + haze albedo: %d iterations (%s), chi square %s, albedo %.6f +- %.2e"
          % (len(b.history), b.stop, np.array2string(np.array(b.history), precision=6), alb, sig))
    assert b.stop == "converged" and abs(alb - SC.ALBEDO) <= sig
