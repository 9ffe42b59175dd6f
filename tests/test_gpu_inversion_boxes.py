"""retrieval.inversion_boxes: the latitude-box retrieval of examples/retrieve_lat_boxes.py at 600 grid points -- an HCN-like
gas on 3 latitude boxes x 5 altitude nodes (smm.LinearProfile_2D; the closing limit's 5 parameters touch nothing), 6
BoxPixels of three rays each heading north across the box boundaries, one engine.limb_rays_state_bands call per iteration
with the parameter blocks per ray."""
import importlib.util
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    import torch
    assert torch.cuda.is_available(), "these tests need the GPU"
    from spectrobot_amd import engine
    engine.set_device(0)
    yield engine
    engine.set_state_ray_blocks(False)


@pytest.fixture(scope="module")
def example():
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples", "retrieve_lat_boxes.py")
    spec = importlib.util.spec_from_file_location("retrieve_lat_boxes", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _build(example):
    return example.build(n_grid=600, n_layers=24, n_lines=(40, 60), n_bands=6)


def test_noise_free_twin_of_the_box_profiles(eng, example):
    """Observations from the truth -- the a-priori profile scaled by 1.3, 0.8 and 1.2 in the three boxes -- without noise.
    The loop ends by the reference's stopping rule (smm.retrieval_converged: 'converged' or 'raised') within max_it, chi
    square falls over it, and the state is nearer to the truth, in units of the a-priori sigma, after the loop than
    before it -- the criterion tests/test_gpu_inversion_state.py asks of its twin.  The last call ran per ray with
    fewer walks than rays x dense blocks; the closing limit's parameters touch nothing, keep their a priori and are
    not_involved."""
    from spectrobot_amd import retrieval
    scene, pixels, bayes, true_scale = _build(example)
    truth = bayes(true_scale)
    example.observe(scene, pixels, truth, 0.004)
    x_true = truth.param_vector()
    bs = bayes()
    sigma = np.array([p.apriori_err for p in bs.params()])
    before = np.linalg.norm((bs.param_vector() - x_true) / sigma)
    max_it = 10
    chi, _, sims, b = retrieval.inversion_boxes(scene, bs, pixels, max_it=max_it)
    route, walks = eng.last_state_route()
    after = np.linalg.norm((b.param_vector() - x_true) / sigma)
    print("\ninversion_boxes twin: %d iterations (%s), chi square %s; state error in a-priori sigmas %.3f -> %.3f; touched per pixel %s; "
          "route %d, %d walks of %d rays (dense: %d)"
          % (len(b.history), b.stop, np.array2string(np.array(b.history), precision=4), before, after, b.touches.sum(axis=1).tolist(),
             route, walks, 3 * len(pixels), 3 * len(pixels) * 2))
    print("  retrieved %s\n  truth     %s" % (np.array2string(b.param_vector(), precision=3), np.array2string(x_true, precision=3)))
    assert b.stop in ("converged", "raised") and 2 <= len(b.history) <= max_it
    assert b.history[-1] < b.history[0] and after < before
    assert len(sims) == len(pixels) and b.jacobian.shape == (len(pixels) * len(scene.bands_nm), 20)
    assert route == 2 and 3 * len(pixels) <= walks < 3 * len(pixels) * 2
    assert not b.touches[:, 15:].any() and np.array_equal(b.param_vector()[15:], bayes().param_vector()[15:])
    assert all(p.not_involved for p in b.params()[15:])
    assert [p.not_involved for p in b.params()] == list(~b.touches.any(axis=0))
    assert not b.jacobian[:, 15:].any()
    assert scene.gas("HCN").vmr_boxes.shape == (4, 24) and np.array_equal(scene.gas("HCN").vmr_boxes, b.sets["HCN"].profile())
    # rows of (pixel, parameter) pairs that do not touch are exact zeros in the Jacobian
    nb = len(scene.bands_nm)
    K = b.jacobian.reshape(len(pixels), nb, 20)
    assert not K.transpose(0, 2, 1)[~b.touches].any()


def test_first_iteration_jacobian_against_central_differences(eng, example):
    """The Jacobian of the first iteration (max_it = 1) against central differences of the forward model alone
    (retrieval.simulate_boxes: limb_rays + the instrument step + the field of view on a rebuilt batch) with one box VMR
    node perturbed, for the best-seen parameter of every box: step h = 1e-3 of the node's value and h / 2, and the rule
    of tests/test_gpu_state_jacobian.py's finite-difference check: |K - FD(h/2)| <= 2 |FD(h) - FD(h/2)| + 1e-9 max|K| per
    pixel in the max norm, |FD(h) - FD(h/2)| < 1e-3 max|K|."""
    from spectrobot_amd import retrieval
    scene, pixels, bayes, true_scale = _build(example)
    example.observe(scene, pixels, bayes(true_scale), 0.004)
    b = retrieval.inversion_boxes(scene, bayes(), pixels, max_it=1)[3]
    nb, n_pix = len(scene.bands_nm), len(pixels)
    K = b.jacobian.reshape(n_pix, nb, 20)
    seen = np.abs(K).max(axis=(0, 1))

    def fd(p, h):
        out = []
        for sgn in (1.0, -1.0):
            bs = bayes()
            par = bs.params()[p]
            par.value = par.value + sgn * h
            out.append(retrieval.simulate_boxes(scene, bs, pixels))
        return (out[0] - out[1]) / (2.0 * h)

    for box in range(3):
        p = 5 * box + int(np.argmax(seen[5 * box:5 * box + 5]))
        h = 1e-3 * bayes().params()[p].value
        f1, f2 = fd(p, h), fd(p, 0.5 * h)
        jm = float(np.abs(K[:, :, p]).max())
        trunc = np.abs(f1 - f2).max(axis=-1)
        err = np.abs(K[:, :, p] - f2).max(axis=-1)
        print("\ninversion_boxes FD: box %d, parameter %d (max|K| %.3g): |K - FD(h/2)| / max|K| %.2e, |FD(h) - FD(h/2)| / max|K| %.2e"
              % (box, p, jm, float(err.max()) / jm, float(trunc.max()) / jm))
        assert jm > 0 and float(trunc.max()) < 1e-3 * jm
        assert np.all(err <= 2.0 * trunc + 1e-9 * jm)
