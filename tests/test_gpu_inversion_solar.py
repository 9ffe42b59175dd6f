"""The sunlit twin of tests/test_gpu_inversion_haze.py: a CH4 VMR profile and the extinction profile of a haze that scatters
sunlight once into the line of sight (retrieval.TableGas(solar=...), retrieval.Sun) retrieved together from noise-free
sunlit pixels by retrieval.inversion_state, whose Jacobians hold the solar attenuation fixed within an iteration.  The sun
stands high (solar_source_cases): the solar optical depth to the lowest tangent point stays small against 1."""
import numpy as np
import pytest

import solar_source_cases as SC

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    import torch
    assert torch.cuda.is_available(), "these tests need the GPU"
    from spectrobot_amd import engine
    engine.set_device(0)
    return engine


def test_twin_retrieval_of_ch4_and_sunlit_haze(eng):
    from spectrobot_amd import retrieval
    scene, pixels, bayes, x_true, sigma = SC.solar_twin(eng)
    med, top = SC.solar_depth_to_lowest_tangent(eng, scene, pixels)
    print("\nsunlit twin: solar optical depth to the lowest tangent layer, median %.3f, largest %.3f" % (med, top))
    assert med < 0.1
    bs = bayes()
    x0 = bs.param_vector().copy()
    # lambda_LM = 0 as in the haze twin: without noise chi square has no floor for the damped step's 1 % rule
    chi, _, sims, b = retrieval.inversion_state(scene, bs, pixels, max_it=10, lambda_LM=0.0)
    hist = np.array(b.history)
    d0, d1 = np.abs(x0 - x_true) / sigma, np.abs(b.param_vector() - x_true) / sigma
    print("sunlit twin: %d iterations (%s), chi square %s;\n  retrieved %s\n  truth     %s\n  distance in a-priori sigmas, first guess %s -> retrieved %s"
          % (len(hist), b.stop, np.array2string(hist, precision=4), np.array2string(b.param_vector(), precision=4),
             np.array2string(x_true, precision=4), np.array2string(d0, precision=3), np.array2string(d1, precision=3)))
    assert b.stop in ("converged", "raised") and len(hist) <= 10          # the loop's own rule, not max_it
    assert len(hist) >= 2 and np.all(np.diff(hist[:-1]) < 0)               # chi square falls in every accepted iteration
    if b.stop == "converged":
        assert hist[-1] < hist[0]
    for sl, name in ((slice(0, 3), "CH4"), (slice(3, 6), "haze")):
        assert np.linalg.norm(d1[sl]) < np.linalg.norm(d0[sl]), name
    assert len(sims) == len(pixels) and b.jacobian.shape == (len(pixels) * len(scene.bands_nm), 6)


def test_inversion_fast_limb_redoes_the_solar_pass_between_its_iterations(eng):
    """inversion_fast_limb keeps a sunlit scene away from its loop-in-one-call route (whose coefficient rows stay fixed):
    it ends with solar rows that belong to the final VMRs, its spectra are radtrans(scene)'s at the retrieved state, and
    the rows of the first guess -- what the one-call route would have kept -- are not those."""
    import torch
    from spectrobot_amd import retrieval
    scene, pixels, bayes, x_true, sigma = SC.solar_twin(eng)
    bs = bayes()
    retrieval._state_into_gases(scene, bs)
    scene.coefficients()
    haze = scene.gas("haze")
    first = haze.coeffs[1].clone()
    chi, _, sims, b = retrieval.inversion_fast_limb(scene, bs, pixels, max_it=10, lambda_LM=0.0)
    hist = np.array(b.history)
    print("\nsunlit twin through inversion_fast_limb: %d iterations (%s), chi square %s"
          % (len(hist), b.stop, np.array2string(hist, precision=4)))
    assert b.stop in ("converged", "raised") and len(hist) >= 3 and hist[-1] < 1e-3 * hist[0]
    kept = haze.coeffs[1]                            # as the driver leaves them
    scene._solar_key = None                          # ... and made again from nothing, for the VMRs the gases hold now
    scene.coefficients()
    assert haze.coeffs[1] is not kept and torch.equal(haze.coeffs[1], kept)
    moved = float(((kept - first).abs() / kept.abs().clamp_min(1e-300)).max())
    print("solar rows, final against first guess: largest relative change %.2e" % moved)
    assert moved > 1e-3
    order = sorted(pixels, key=lambda p: p.limb_tg_alt)
    want = np.array([y.spectrum for y in retrieval.radtrans(scene, order)])
    got = np.array([y.spectrum for y in sims])
    if b.stop == "converged":                        # (the last forward model ran at the parameters that are returned)
        assert np.max(np.abs(got - want) / np.abs(want)) < 1e-9
    d0, d1 = np.abs(bayes().param_vector() - x_true) / sigma, np.abs(b.param_vector() - x_true) / sigma
    assert np.linalg.norm(d1) < 0.1 * np.linalg.norm(d0)


def test_inversion_redoes_the_solar_pass_between_its_iterations(eng):
    """The reference-shaped driver retrieval.inversion builds its coefficients before the loop; on a sunlit scene it asks
    for them again in every iteration, and only the solar pass is redone."""
    from spectrobot_amd import retrieval
    scene, pixels, bayes, _, _ = SC.solar_twin(eng)
    bs = bayes()
    retrieval._state_into_gases(scene, bs)
    scene.coefficients()
    haze, ch4 = scene.gas("haze"), scene.gas("CH4")
    first, thermal, lines = haze.coeffs[1], haze.thermal, ch4.coeffs
    rows0 = first.clone()
    retrieval.inversion(scene, bs, pixels, useLUTs=False, max_it=3)
    assert len(bs.history) >= 2 and bs.history[1] < bs.history[0]
    assert haze.coeffs[1] is not first and haze.thermal is thermal and ch4.coeffs is lines
    assert float((haze.coeffs[1] - rows0).abs().max()) > 0.0
