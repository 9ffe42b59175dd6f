"""The haze twin of examples/retrieve_haze.py at 600 grid points, noise-free: a CH4 VMR profile and a haze extinction
profile (a retrieval.TableGas) retrieved together by retrieval.inversion_state, which takes the scene unchanged."""
import copy

import numpy as np
import pytest

import absorber_table_cases as K

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    import torch
    assert torch.cuda.is_available(), "these tests need the GPU"
    from spectrobot_amd import engine
    engine.set_device(0)
    return engine


@pytest.fixture(scope="module")
def twin(eng):
    return K.haze_twin(eng)


def test_twin_retrieval_of_ch4_and_haze(eng, twin):
    from spectrobot_amd import retrieval
    scene, pixels, bayes, x_true, sigma = twin
    bs = bayes()
    x0 = bs.param_vector().copy()
    # lambda_LM = 0: without noise chi square has no noise floor, and the damped step's linear convergence (a factor ~3 per
    # iteration at the driver's default 0.1) never meets the 1 % rule within 10 iterations; the undamped Gauss-Newton
    # step reaches the floor the a priori leaves
    chi, _, sims, b = retrieval.inversion_state(scene, bs, pixels, max_it=10, lambda_LM=0.0)
    hist = np.array(b.history)
    d0, d1 = np.abs(x0 - x_true) / sigma, np.abs(b.param_vector() - x_true) / sigma
    print("\nhaze twin: %d iterations (%s), chi square %s;\n  retrieved %s\n  truth     %s\n  distance in a-priori sigmas, first guess %s -> retrieved %s"
          % (len(hist), b.stop, np.array2string(hist, precision=4), np.array2string(b.param_vector(), precision=4),
             np.array2string(x_true, precision=4), np.array2string(d0, precision=3), np.array2string(d1, precision=3)))
    assert b.stop in ("converged", "raised") and len(hist) <= 10          # the loop's own rule, not max_it
    assert len(hist) >= 2 and np.all(np.diff(hist[:-1]) < 0)               # chi square falls in every accepted iteration
    if b.stop == "converged":
        assert hist[-1] < hist[0]
    for sl, name in ((slice(0, 3), "CH4"), (slice(3, 6), "haze")):
        assert np.linalg.norm(d1[sl]) < np.linalg.norm(d0[sl]), name
    assert len(sims) == len(pixels) and b.jacobian.shape == (len(pixels) * len(scene.bands_nm), 6)


def test_first_iteration_haze_columns_against_central_differences(eng, twin):
    """The haze set's columns of the first iteration's Jacobian (band values through the closed-form field of view) against
    central differences of the forward model in the haze nodes at h and h / 2:
    |K - FD(h/2)| <= 2 |FD(h) - FD(h/2)| + 1e-9 max|K| per column."""
    from spectrobot_amd import retrieval
    scene, pixels, bayes, _, sigma = twin
    bs = bayes()
    x0 = bs.param_vector().copy()
    _, _, _, b = retrieval.inversion_state(scene, copy.deepcopy(bs), pixels, max_it=1)
    K1 = np.array(b.jacobian)
    haze0 = bayes().sets["haze"].profile()
    masks = [np.asarray(par.maskgrid.mask, float) for par in bs.sets["haze"].set]
    retrieval._state_into_gases(scene, bayes())      # back to the first guess

    def forward(prof):
        scene.gas("haze").add_clim(prof)
        return np.concatenate([y.spectrum for y in retrieval.radtrans(scene, sorted(pixels, key=lambda p: p.limb_tg_alt))])

    for k in range(3):
        fd = []
        for h in (0.02 * x0[3 + k], 0.01 * x0[3 + k]):
            fd.append((forward(haze0 + h * masks[k]) - forward(haze0 - h * masks[k])) / (2.0 * h))
        col = K1[:, 3 + k]
        jm = np.abs(col).max()
        trunc, err = np.abs(fd[0] - fd[1]).max(), np.abs(col - fd[1]).max()
        print("\nhaze twin FD, haze node %d: max|K| %.3e, |K - FD(h/2)| / max|K| %.2e, |FD(h) - FD(h/2)| / max|K| %.2e" % (k, jm, err / jm, trunc / jm))
        assert jm > 0 and err <= 2.0 * trunc + 1e-9 * jm
    scene.gas("haze").add_clim(haze0)
