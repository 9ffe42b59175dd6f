"""retrieval.inversion_state under a tabulated instrument line shape (retrieval.LimbScene(..., ils=...)): the scene of
tests/test_gpu_inversion_instr.py -- the small mixed scene of tests/test_gpu_state_bands.py, its eight bands with every
window end in the middle of a gap between two grid points -- with an ASYMMETRIC response table in the Gaussian's place.
Observations are synthesised at a known band shift and width; the retrieval of BandCalibration (shift, ln width) and one
VMR set under the same table stops by the reference's rule and returns both instrument parameters within three of their
own posterior standard deviations, on both routes; the same retrieval with the Gaussian (ils=None) cannot explain those
observations as well: it ends at a larger chi square.  Needs a real MI355X."""
import copy

import numpy as np
import pytest

import lowres_reference as R

pytestmark = pytest.mark.gpu
NOISE = 0.004


@pytest.fixture(scope="module")
def eng():
    import torch
    assert torch.cuda.is_available(), "these tests need the GPU"
    from spectrobot_amd import engine
    engine.set_device(0)
    return engine


def _response(eng):
    """A skewed bell on +-5 widths, 321 knots: the steep side towards shorter wavelengths, ends of 1e-6 of the peak."""
    return eng.ILS.from_function(lambda t: np.exp(-0.5 * t * t) * (1.0 + 0.6 * np.tanh(1.5 * t)), -5.0, 5.0, 321)


def _scene(eng, ils):
    import test_gpu_state_bands as SB
    import test_gpu_inversion_instr as TI
    from spectrobot_amd import retrieval
    scene, pixels = SB._mixed_scene(eng)
    f, w = TI._mid_gap(scene.grid, scene.bands_nm, scene.widths_nm)          # (the table's window is +-5 w: the Gaussian's ends)
    scene = retrieval.LimbScene(scene.grid, scene.z, scene.temps, scene.press, scene.gases, f, w, ils=ils)
    g = R.guard(scene.grid, f, w)
    inside = (f - 5.0 * w > 1e7 / scene.grid[-1]) | (f + 5.0 * w < 1e7 / scene.grid[0])
    assert inside.any() and g[inside].min() > 0.45, g
    assert scene.ils is ils
    return scene, pixels


def _posterior_sigma(b, pixels):
    """sqrt diag (K^T Se^-1 K + Sa^-1)^-1 with the Jacobian of the last update."""
    noise = np.concatenate([p.noise.spectrum for p in sorted(pixels, key=lambda x: x.limb_tg_alt)])
    K = b.jacobian / noise[:, None]
    return np.sqrt(np.diag(np.linalg.inv(K.T @ K + np.linalg.inv(np.asarray(b.VCM_apriori(), dtype=float)))))


def test_shift_and_width_of_a_tabulated_response(eng):
    import test_gpu_state_bands as SB
    import test_gpu_inversion_instr as TI
    from spectrobot_amd import retrieval
    ils = _response(eng)
    assert abs(ils.area()[0] - 1.0) < 2e-15 and ils.phi[0, 100] != ils.phi[0, 220]       # asymmetric: knots -+1.875
    scene, pixels = _scene(eng, ils)
    x_true = np.concatenate([1.3 * np.full(3, 2.2e-6), [0.25 * scene.widths_nm0.min(), np.log(1.05)]])
    truth, _ = TI._sets(scene, first_guess=(x_true[:3], x_true[3], x_true[4]))
    retrieval._state_into_gases(scene, truth)
    SB._observe(scene, pixels, NOISE)                                         # radtrans under the scene's table
    with_table = np.array([p.observation.spectrum for p in pixels])
    scene.ils = None
    gaussian = np.array([y.spectrum for y in retrieval.radtrans(scene, pixels)])
    scene.ils = ils
    print("\nthe table against the Gaussian at the truth: largest band difference %.3g of the largest band" %
          (np.abs(with_table - gaussian).max() / np.abs(with_table).max()))
    bs, _ = TI._sets(scene)
    chis = {}
    for fused in (True, False):
        chi, _, sims, b = retrieval.inversion_state(scene, copy.deepcopy(bs), pixels, max_it=10, bands_in_kernel=fused)
        sig = _posterior_sigma(b, pixels)
        off = (b.param_vector() - x_true) / sig
        print("table, bands in kernel %d: %d iterations (%s), chi square %s; retrieved %s, truth %s, (retrieved - truth) / posterior sigma %s"
              % (fused, len(b.history), b.stop, np.array2string(np.array(b.history), precision=4),
                 np.array2string(b.param_vector(), precision=5), np.array2string(x_true, precision=5), np.array2string(off, precision=3)))
        assert b.stop in ("converged", "raised") and len(b.history) >= 2 and b.history[-1] < b.history[0]
        assert abs(off[3]) <= 3.0 and abs(off[4]) <= 3.0
        chis[fused] = b.history[-1]
    # the Gaussian on the same observations
    scene.ils = None
    chi_g, _, _, bg = retrieval.inversion_state(scene, copy.deepcopy(bs), pixels, max_it=10, bands_in_kernel=True)
    print("Gaussian on the same observations: %d iterations (%s), chi square %s; retrieved %s"
          % (len(bg.history), bg.stop, np.array2string(np.array(bg.history), precision=4), np.array2string(bg.param_vector(), precision=5)))
    print("final chi square: table %.6g (fused) %.6g (composed), Gaussian %.6g" % (chis[True], chis[False], bg.history[-1]))
    assert bg.history[-1] > chis[True] and bg.history[-1] > chis[False]
