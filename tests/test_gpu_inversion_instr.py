"""retrieval.inversion_state with the instrument's band calibration in the state (retrieval.BandCalibration, the set named
"instr": band shift and ILS width beside a VMR profile) on its two routes -- the one fused call with the instrument rows
(bands_in_kernel=True) and the state Jacobian call plus engine.hires_to_lowres_instrument on its radiance -- against each
other, against central differences of the simulated bands through scene.bands_nm / scene.widths_nm, and on a noise-free
twin.  The scene is the small mixed scene of tests/test_gpu_state_bands.py (6000 points, 22 layers, an LTE HCN and a
non-LTE CH4, five pixels with the closed-form field of view), its eight bands moved by less than a grid spacing so that
every window end inside the grid lies in the middle of a gap between two grid points.  Needs a real MI355X."""
import copy

import numpy as np
import pytest

import lowres_reference as R

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    import torch
    assert torch.cuda.is_available(), "these tests need the GPU"
    from spectrobot_amd import engine
    engine.set_device(0)
    return engine


def _mid_gap(grid, bands, widths, n_sigma=5.0):
    """The bands with every window end that lies inside the grid moved to the middle of its gap between two grid points
    (centre and width follow from the two ends): a step of a fifth of a spacing then crosses no grid point."""
    x = 1e7 / np.asarray(grid)[::-1]
    out_f, out_w = [], []
    for f, w in zip(bands, widths):
        ends = []
        for e in (f - n_sigma * w, f + n_sigma * w):
            k = int(np.searchsorted(x, e))
            ends.append(0.5 * (x[k - 1] + x[k]) if 0 < k < x.size else e)
        out_f.append(0.5 * (ends[0] + ends[1]))
        out_w.append((ends[1] - ends[0]) / (2.0 * n_sigma))
    return np.array(out_f), np.array(out_w)


def _scene(eng):
    import test_gpu_state_bands as SB
    from spectrobot_amd import retrieval
    scene, pixels = SB._mixed_scene(eng)
    f, w = _mid_gap(scene.grid, scene.bands_nm, scene.widths_nm)
    scene = retrieval.LimbScene(scene.grid, scene.z, scene.temps, scene.press, scene.gases, f, w)
    g = R.guard(scene.grid, f, w)
    inside = (f - 5.0 * w > 1e7 / scene.grid[-1]) | (f + 5.0 * w < 1e7 / scene.grid[0])
    assert inside.any() and g[inside].min() > 0.45, g
    assert np.array_equal(scene.bands_nm0, f) and np.array_equal(scene.widths_nm0, w)
    return scene, pixels


def _sets(scene, first_guess=None):
    from spectrobot_amd import retrieval, spect_main_module as smm
    z = scene.z
    span = z[-1] - z[0]
    nodes = [z[0] + q * span for q in (0.1, 0.45, 0.8)]
    apr, sig = np.full(3, 2.2e-6), np.full(3, 1.1e-6)
    fg = (None, None, None) if first_guess is None else first_guess
    bs = smm.BayesSet(tag="HCN + band shift + ILS width")
    bs.add_set(smm.LinearProfile_1D_new("HCN", z, nodes, apr, sig, first_guess_prof=fg[0]))
    shift = (0.0, 0.1) if fg[1] is None else (0.0, 0.1, fg[1])
    ln_w = (0.0, 0.1) if fg[2] is None else (0.0, 0.1, fg[2])
    bs.add_set(retrieval.BandCalibration(shift=shift, ln_width=ln_w))
    return bs, np.concatenate([sig, [0.1, 0.1]])


def _truth(scene, pixels):
    """Observations (noise-free) from a perturbed truth: the HCN profile scaled by 1.3, the band centres shifted by a quarter
    of the narrowest width, the widths scaled by 1.05.  Returns x_true in the BayesSet's order."""
    import test_gpu_state_bands as SB
    from spectrobot_amd import retrieval
    x_true = np.concatenate([1.3 * np.full(3, 2.2e-6), [0.25 * scene.widths_nm0.min(), np.log(1.05)]])
    truth, _ = _sets(scene, first_guess=(x_true[:3], x_true[3], x_true[4]))
    retrieval._state_into_gases(scene, truth)
    assert np.allclose(scene.bands_nm - scene.bands_nm0, x_true[3], rtol=0, atol=1e-12) and np.allclose(scene.widths_nm, 1.05 * scene.widths_nm0, rtol=1e-15)
    SB._observe(scene, pixels, 0.004)
    return x_true


def test_one_iteration_on_both_routes_and_central_differences(eng):
    from spectrobot_amd import retrieval
    scene, pixels = _scene(eng)
    _truth(scene, pixels)
    bs, _ = _sets(scene)
    n_pix, n_b, n_par = len(pixels), len(scene.bands_nm), 5
    out = []
    for fused in (False, True):
        chi, _, sims, b = retrieval.inversion_state(scene, copy.deepcopy(bs), pixels, max_it=1, bands_in_kernel=fused)
        assert b.jacobian.shape == (n_pix * n_b, n_par) and len(b.history) == 1 and chi == b.history[0]
        out.append((chi, b.jacobian.copy(), b.param_vector(), np.array([s.spectrum for s in sims])))
        # the scene holds the updated calibration
        st = b.sets["instr"]
        assert np.array_equal(scene.bands_nm, scene.bands_nm0 + st.value("shift")) and st.value("shift") != 0.0
        assert np.array_equal(scene.widths_nm, scene.widths_nm0 * np.exp(st.value("ln_width")))
    (chi_u, K_u, x_u, s_u), (chi_f, K_f, x_f, s_f) = out
    col_max = np.abs(K_u).max(axis=0)
    dist = np.abs(K_f - K_u).max(axis=0) / col_max
    print("\ninstr set, one iteration: |K fused - K composed| per column / the column's largest element: %s; largest |K|: %s"
          % (np.array2string(dist, precision=2), np.array2string(col_max, precision=3)))
    print("chi square %.10g | %.10g; update, largest relative difference %.2e" % (chi_u, chi_f, np.max(np.abs(x_f / x_u - 1))))
    assert np.all(col_max > 0) and np.all(dist <= 1e-11)
    assert np.allclose(chi_f, chi_u, rtol=1e-9) and np.allclose(x_f, x_u, rtol=1e-9, atol=0.0)
    assert np.allclose(s_f, s_u, rtol=1e-11, atol=0.0)
    # central differences of the simulated bands at the first guess, through scene.bands_nm and scene.widths_nm
    retrieval._state_into_gases(scene, bs)
    b0, w0 = scene.bands_nm0, scene.widths_nm0
    spacing = np.diff(1e7 / scene.grid[::-1]).min()
    sim = lambda: np.concatenate([y.spectrum for y in retrieval.radtrans(scene, pixels)])
    assert np.allclose(sim(), s_u.ravel(), rtol=1e-9, atol=0.0)             # (the same state: another route to the radiances)
    h_f = 0.2 * spacing                                   # a window end moves by h_f: a fifth of a spacing from the middle of its gap
    h_w = 0.2 * spacing / (5.0 * w0.max())                # ... by 5 w (e^h - 1)
    fd = []
    for (fp, wp), (fm, wm), step in (((b0 + h_f, w0), (b0 - h_f, w0), 2 * h_f),
                                     ((b0, w0 * np.exp(h_w)), (b0, w0 * np.exp(-h_w)), 2 * h_w)):
        for f, w in ((fp, wp), (fm, wm)):
            assert np.array_equal(R.weights(scene.grid, f, w)[2], R.weights(scene.grid, b0, w0)[2])     # the same points in every window
        scene.bands_nm, scene.widths_nm = fp, wp
        up = sim()
        scene.bands_nm, scene.widths_nm = fm, wm
        fd.append((up - sim()) / step)
    scene.bands_nm, scene.widths_nm = b0.copy(), w0.copy()
    for name, col, d in (("shift", 3, fd[0]), ("ln_width", 4, fd[1])):
        for tag, K in (("composed", K_u), ("fused", K_f)):
            err = np.abs(K[:, col] - d).max() / np.abs(d).max()
            print("  %-9s %-9s |K - central difference| / largest element = %.2e (step %.2e)" % (name, tag, err, h_f if col == 3 else h_w))
            assert err <= 1e-6, (name, tag, err)


def test_noise_free_twin(eng):
    """Chi square falls over the history, and the band shift, the ILS width and the VMR profile each end nearer the truth
    than they began (first guess: the a priori, zero shift and zero log width), on both routes."""
    from spectrobot_amd import retrieval
    scene, pixels = _scene(eng)
    x_true = _truth(scene, pixels)
    bs, sigma = _sets(scene)
    for fused in (True, False):
        b0 = copy.deepcopy(bs)
        before = np.abs(b0.param_vector() - x_true) / sigma
        chi, _, sims, b = retrieval.inversion_state(scene, b0, pixels, max_it=10, bands_in_kernel=fused)
        after = np.abs(b.param_vector() - x_true) / sigma
        print("\ninstr twin (bands in kernel %d): %d iterations (%s), chi square %s; retrieved %s, truth %s"
              % (fused, len(b.history), b.stop, np.array2string(np.array(b.history), precision=4),
                 np.array2string(b.param_vector(), precision=4), np.array2string(x_true, precision=4)))
        assert len(b.history) >= 2 and b.history[-1] < b.history[0]
        assert after[3] < before[3] and after[4] < before[4]
        assert np.linalg.norm(after[:3]) < np.linalg.norm(before[:3])
        assert len(sims) == len(pixels) and b.jacobian.shape == (len(pixels) * len(scene.bands_nm), 5)
        # the returned spectra carry the band centres they were simulated on: the last iteration's, not the first guess's
        assert b.stop == 'converged' and np.array_equal(sims[0].spectral_grid.grid, scene.bands_nm)
        assert not np.array_equal(sims[0].spectral_grid.grid, scene.bands_nm0)
        assert np.array_equal(b.params()[3].derivatives[0].spectral_grid.grid, scene.bands_nm)


def test_the_instrument_set_alone(eng):
    """A BayesSet that holds nothing but the "instr" set: the fused route calls the state kernel without any parameter, the
    other route needs no Jacobian call at all (the radiances, then the instrument step with its derivative rows).  One
    iteration on both: K, chi square, the simulated spectra and the update to the tolerances of the mixed case, and the
    update moves both parameters towards the truth."""
    from spectrobot_amd import retrieval, spect_main_module as smm
    scene, pixels = _scene(eng)
    x_true = _truth(scene, pixels)[3:]
    bs = smm.BayesSet(tag="band shift + ILS width")
    bs.add_set(retrieval.BandCalibration(shift=(0.0, 0.1), ln_width=(0.0, 0.1)))
    scene.gas("HCN").add_clim(np.full(len(scene.z), 1.3 * 2.2e-6))          # (the truth's profile: the calibration is all that is off)
    out = []
    for fused in (False, True):
        chi, _, sims, b = retrieval.inversion_state(scene, copy.deepcopy(bs), pixels, max_it=1, bands_in_kernel=fused)
        assert b.jacobian.shape == (len(pixels) * len(scene.bands_nm), 2) and len(sims) == len(pixels)
        out.append((chi, b.jacobian.copy(), b.param_vector(), np.array([s.spectrum for s in sims])))
    (chi_u, K_u, x_u, s_u), (chi_f, K_f, x_f, s_f) = out
    col_max = np.abs(K_u).max(axis=0)
    dist = np.abs(K_f - K_u).max(axis=0) / col_max
    print("\ninstr set alone, one iteration: |K fused - K composed| / largest element %s; chi square %.10g | %.10g; update %s | %s, truth %s"
          % (np.array2string(dist, precision=2), chi_u, chi_f, x_u, x_f, x_true))
    assert np.all(col_max > 0) and np.all(dist <= 1e-11)
    assert np.allclose(chi_f, chi_u, rtol=1e-9) and np.allclose(x_f, x_u, rtol=1e-9, atol=0.0)
    assert np.allclose(s_f, s_u, rtol=1e-11, atol=0.0)
    assert np.all(np.abs(x_u - x_true) < np.abs(x_true))
