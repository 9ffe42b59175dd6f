"""The solar attenuation in the Jacobians through the scene and the driver: on the CH4 + sunlit haze scene with the sun low
(solar_jacobian_cases: the solar optical depth reaches order 1 in the line cores) every VMR column of
inversion_state(solar_attenuation=True)'s first Jacobian meets the project's finite-difference criterion with the solar pass
redone in every perturbed run -- and the frozen Jacobian misses it by more than a factor 10 --; both routes of the driver
agree; the flag off leaves the driver's history as it was; the sunlit twin converges with the flag on, no farther from the
truth than the frozen loop."""
import copy

import numpy as np
import pytest

import solar_jacobian_cases as JC
import solar_source_cases as SC

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    import torch
    assert torch.cuda.is_available(), "these tests need the GPU"
    from spectrobot_amd import engine
    engine.set_device(0)
    return engine


def _first_jacobian(retrieval, scene, bayes, pixels, **kw):
    _, _, _, b = retrieval.inversion_state(scene, copy.deepcopy(bayes), pixels, max_it=1, **kw)
    return np.array(b.jacobian)


def test_state_jacobian_against_central_differences_of_the_whole_forward_model(eng):
    """|K - FD(h/2)| <= 2 |FD(h) - FD(h/2)| + 1e-9 max|K| for every VMR column with the flag on, solar_frozen = False: the
    differences redo the solar pass.  The frozen Jacobian (the flag off) must MISS the criterion in at least one CH4 column
    by a factor >= 10: a condition on the scene, which keeps the test from passing with a zero term."""
    from spectrobot_amd import retrieval
    scene, pixels, bayes, _, sigma = JC.low_sun_twin(eng)
    med, top = SC.solar_depth_to_lowest_tangent(eng, scene, pixels)
    print("\nlow-sun twin: solar optical depth to the lowest tangent layer, median %.3f, largest %.3f" % (med, top))
    assert top > 1.0
    bs = bayes()
    x0 = bs.param_vector().copy()
    K_frozen = _first_jacobian(retrieval, scene, bs, pixels)
    K_full = _first_jacobian(retrieval, scene, bs, pixels, solar_attenuation=True)
    retrieval._state_into_gases(scene, bayes())      # back to the first guess
    assert scene.solar_frozen is False
    order = sorted(pixels, key=lambda p: p.limb_tg_alt)

    def forward(name, prof):
        scene.gas(name).add_clim(prof)
        return np.concatenate([y.spectrum for y in retrieval.radtrans(scene, order)])

    col_at, miss = 0, {"CH4": [], "haze": []}
    for name in ("CH4", "haze"):
        prof0 = bayes().sets[name].profile()
        masks = [np.asarray(par.maskgrid.mask, float) for par in bs.sets[name].set]
        for k in range(3):
            fd = []
            for h in (0.02 * x0[col_at], 0.01 * x0[col_at]):
                fd.append((forward(name, prof0 + h * masks[k]) - forward(name, prof0 - h * masks[k])) / (2.0 * h))
            col, frozen = K_full[:, col_at], K_frozen[:, col_at]
            jm = np.abs(col).max()
            trunc, err, err_frozen = np.abs(fd[0] - fd[1]).max(), np.abs(col - fd[1]).max(), np.abs(frozen - fd[1]).max()
            allowed = 2.0 * trunc + 1e-9 * jm
            miss[name].append(err_frozen / (2.0 * trunc + 1e-9 * np.abs(frozen).max()))
            print("low-sun twin FD, %s node %d: max|K| %.3e, |K - FD(h/2)| / max|K| with the term %.2e, frozen %.2e, "
                  "|FD(h) - FD(h/2)| / max|K| %.2e; frozen misses by %.1f" % (name, k, jm, err / jm, err_frozen / jm, trunc / jm, miss[name][-1]))
            assert jm > 0 and err <= allowed, (name, k, err / allowed)
            col_at += 1
        scene.gas(name).add_clim(prof0)
    assert max(miss["CH4"]) >= 10.0, miss


def test_both_routes_agree_and_the_flag_off_changes_nothing(eng):
    from spectrobot_amd import retrieval
    scene, pixels, bayes, _, _ = JC.low_sun_twin(eng)
    bs = bayes()
    K_hi = _first_jacobian(retrieval, scene, bs, pixels, solar_attenuation=True)
    K_band = _first_jacobian(retrieval, scene, bs, pixels, solar_attenuation=True, bands_in_kernel=True)
    scale = np.abs(K_hi).max(axis=0, keepdims=True)
    worst = float(np.max(np.abs(K_hi - K_band) / scale))
    print("\nsolar attenuation, hi-res route against bands_in_kernel: largest difference / column maximum %.2e" % worst)
    assert worst <= 1e-12
    # the flag off, and a scene without a sun with the flag on: the driver's history and Jacobian, bit for bit
    runs = []
    for flag, sun in ((None, True), (False, True), (None, False), (True, False)):
        sc, px, by, _, _ = SC.solar_twin(eng)
        if not sun:
            sc.sun = None
        kw = {} if flag is None else dict(solar_attenuation=flag)
        _, _, _, b = retrieval.inversion_state(sc, by(), px, max_it=3, lambda_LM=0.0, **kw)
        runs.append((np.array(b.history), np.array(b.jacobian), sc.keep_solar_rows))
    for a, b in ((0, 1), (2, 3)):
        assert np.array_equal(runs[a][0].view(np.uint64), runs[b][0].view(np.uint64))
        assert np.array_equal(runs[a][1].view(np.uint64), runs[b][1].view(np.uint64))
    assert not any(r[2] for r in runs)


def test_sunlit_twin_with_the_term(eng):
    """The sunlit twin of test_gpu_inversion_solar.py with the flag on: it stops `converged`, and ends no farther from the
    truth than the frozen loop (the parent's code path, run here beside it) at every node, plus 1e-3 sigma.  Both chi square
    histories and iteration counts are printed, not asserted."""
    from spectrobot_amd import retrieval
    out = {}
    for flag in (False, True):
        scene, pixels, bayes, x_true, sigma = SC.solar_twin(eng)
        _, _, _, b = retrieval.inversion_state(scene, bayes(), pixels, max_it=10, lambda_LM=0.0, solar_attenuation=flag)
        out[flag] = (b.stop, np.array(b.history), np.abs(b.param_vector() - x_true) / sigma)
        print("\nsunlit twin, solar_attenuation=%s: %d iterations (%s), chi square %s\n  distance to the truth in a-priori sigmas %s"
              % (flag, len(out[flag][1]), b.stop, np.array2string(out[flag][1], precision=4), np.array2string(out[flag][2], precision=4)))
    assert out[True][0] == "converged"
    assert np.all(out[True][2] <= out[False][2] + 1e-3), (out[True][2], out[False][2])
