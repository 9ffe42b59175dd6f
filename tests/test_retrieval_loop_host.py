"""The bookkeeping of the array retrieval loop the drivers share (retrieval._array_loop on a retrieval._Observations)
with a fake linear forward model, low = y0 + K x: no device, numpy only."""
import copy

import numpy as np
import pytest

from spectrobot_amd import retrieval as rt, spect_main_module as smm

N_PIX, N_BANDS, N_PAR = 3, 4, 2
BANDS = np.linspace(3000.0, 3300.0, N_BANDS)
RNG = np.random.default_rng(7)
K = RNG.uniform(0.5, 2.0, (N_PIX, N_PAR, N_BANDS))         # d low[pixel, band] / d x[p]
Y0 = RNG.uniform(1.0, 2.0, (N_PIX, N_BANDS))
X_TRUE = np.array([1.3, 0.7])
MASKS = [np.ones(N_BANDS, bool), np.array([True, False, True, False]), np.ones(N_BANDS, bool)]
MASKTOT = np.concatenate(MASKS)
SIGMA = 0.05


def model(x):
    return Y0 + np.einsum("ipb,p->ib", K, np.asarray(x, float))


def problem(masks=MASKS):
    """(bayes_set, pixels): two nodes of one linear profile starting at (1, 1); observations of X_TRUE, constant noise."""
    bs = smm.BayesSet()
    bs.add_set(smm.LinearProfile_1D_new("X", np.linspace(0.0, 10.0, 5), [0.0, 10.0], [1.0, 1.0], [1.0, 1.0]))
    y = model(X_TRUE)
    pixels = [rt.LimbPixel(100.0 + 50.0 * i, observation=rt.Spectrum(y[i], BANDS), noise=rt.Spectrum(np.full(N_BANDS, SIGMA), BANDS),
                           mask=None if masks is None else masks[i]) for i in range(N_PIX)]
    return bs, pixels


class Forward(object):
    """The fake forward model: counts its calls and keeps what it returned."""

    def __init__(self, bs):
        self.bs, self.calls, self.last = bs, 0, None

    def __call__(self):
        self.calls += 1
        self.last = (model(self.bs.param_vector()), K.copy())
        return self.last


def run(bs, pixels, max_it, chi_threshold=0.01):
    ob = rt._Observations(pixels, bs)
    fwd, updates = Forward(bs), []
    chi, low, dlow = rt._array_loop(ob, fwd, lambda: updates.append(bs.values()), chi_threshold, max_it, 0.1, False)
    return ob, fwd, updates, chi, low, dlow


def test_one_iteration():
    bs, pixels = problem()
    bs0 = copy.deepcopy(bs)
    ob, fwd, updates, chi, low, dlow = run(bs, pixels, 1)
    obs_vec = model(X_TRUE).reshape(-1)[MASKTOT]
    sim_vec = model([1.0, 1.0]).reshape(-1)[MASKTOT]
    noi_vec = np.full(10, SIGMA)
    assert np.array_equal(ob.obs_vec, obs_vec) and np.array_equal(ob.noi_vec, noi_vec) and np.array_equal(ob.masktot, MASKTOT)
    assert bs.history == [np.sum(((obs_vec - sim_vec) / noi_vec) ** 2) / (10 - N_PAR)] and chi == bs.history[0]
    assert bs.stop == 'max_it' and fwd.calls == 1
    jac = np.transpose(K, (1, 0, 2)).reshape(N_PAR, -1)[:, MASKTOT].T
    assert bs.jacobian.shape == (10, 2) and np.array_equal(bs.jacobian, jac)
    for par in bs0.params():
        par.set_used()
    smm.inversion_algebra_arrays(jac, obs_vec, sim_vec, noi_vec, bs0, lambda_LM=0.1, L1_reg=False,
                                 Sa_inv=np.linalg.inv(bs0.VCM_apriori()))
    assert np.array_equal(bs.param_vector(), bs0.param_vector()) and not np.array_equal(bs.param_vector(), [1.0, 1.0])
    assert np.array_equal(bs.av_kernel, bs0.av_kernel) and np.array_equal(bs.VCM, bs0.VCM)
    assert updates == [bs.values()]                        # after_update ran once, after the step


def test_no_masks_is_masktot_none():
    bs, pixels = problem(masks=None)
    ob, fwd, _, _, _, _ = run(bs, pixels, 1)
    assert ob.masks is None and ob.masktot is None and ob.obs_vec.size == N_PIX * N_BANDS
    assert np.array_equal(bs.jacobian, np.transpose(K, (1, 0, 2)).reshape(N_PAR, -1).T)


def test_a_converging_run():
    bs, pixels = problem()
    ob, fwd, updates, chi, low, dlow = run(bs, pixels, 20)
    h = bs.history
    assert len(h) == fwd.calls and 2 <= len(h) < 20 and chi == h[-1]
    assert len(updates) == len(h) - 1                      # no step after the iteration that stopped the loop
    assert bs.stop == smm.retrieval_converged(h[-1], h[-2], 0.01) and bs.stop in ('converged', 'raised')
    assert all(smm.retrieval_converged(b, a, 0.01) == '' for a, b in zip(h[:-2], h[1:-1]))
    assert low is fwd.last[0] and dlow is fwd.last[1]
    np.testing.assert_allclose(bs.param_vector(), X_TRUE, atol=1e-2)
    grid = rt._Grid(BANDS + 0.25)
    sims = ob.finish(low, dlow, grid)
    assert len(sims) == N_PIX
    for num, sp in enumerate(sims):
        assert np.array_equal(sp.spectrum, fwd.last[0][num]) and sp.spectral_grid is grid
    assert np.array_equal(bs.jacobian, np.transpose(fwd.last[1], (1, 0, 2)).reshape(N_PAR, -1)[:, MASKTOT].T)
    for ip, par in enumerate(bs.params()):
        assert len(par.derivatives) == N_PIX
        for num, der in enumerate(par.derivatives):
            assert np.array_equal(der.spectrum, fwd.last[1][num, ip]) and der.spectral_grid is grid


def test_max_it_zero():
    bs, pixels = problem()
    ob, fwd, updates, chi, low, dlow = run(bs, pixels, 0)
    assert chi is None and fwd.calls == 0 and updates == [] and bs.history == [] and bs.stop == 'max_it'
    assert ob.finish(low, dlow, rt._Grid(BANDS)) == []
    assert not hasattr(bs, "jacobian")


def test_mixed_fields_of_view_are_refused_before_the_scene_is_touched():
    bs, pixels = problem()
    pixels[1].fov_half = 3.0
    for name, call in (("inversion_state", lambda: rt.inversion_state(None, bs, pixels)),
                       ("inversion_boxes", lambda: rt.inversion_boxes(None, bs, pixels)),
                       ("simulate_boxes", lambda: rt.simulate_boxes(None, bs, pixels))):
        with pytest.raises(ValueError, match=name + " needs the closed-form field of view for every pixel, or for none"):
            call()
    for pix in pixels:                                     # every pixel has one, but not the closed form
        pix.fov_half = 3.0
    with pytest.raises(ValueError, match="inversion_state needs the closed-form"):
        rt.inversion_state(None, bs, pixels, fov_closed_form=False)
