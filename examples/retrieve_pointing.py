#!/usr/bin/env python3
"""Twin experiment with the pointing in the state vector: the VMR profile of an LTE trace gas (HCN-like) retrieved together
with one tangent-altitude offset common to all pixels (retrieval.Pointing, the set named "pointing") by
retrieval.inversion_state with the bands in the kernel -- per iteration the lines of sight are rebuilt at the current
offset and ONE fused call returns the band values, the VMR Jacobian rows and the pointing row (d / d tangent altitude of
every ray, the crossed shells held fixed), no hi-res spectrum written -- at the reduced size of
examples/retrieve_vmr_tvib.py.

  truth      the HCN profile scaled by 1.3, every line of sight 2 km higher than the pixels say
  "observed" the band spectra of 6 limb pixels (three lines of sight each, closed-form field of view) through the truth,
             plus noise
  retrieved  3 VMR nodes of HCN and the offset (km)

A retrieval that takes the pixels' altitudes as exact puts the same misfit into the VMR profile: its result is printed
beside.  Prints the chi-square histories and the retrieved states next to the truth.  Needs an MI355X:
python examples/retrieve_pointing.py
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from spectrobot_amd import engine, retrieval, synthetic as syn          # noqa: E402
from spectrobot_amd import spect_main_module as smm                     # noqa: E402

HCN_MM, HCN_ISO_RATIO = 27.010899, 0.985114
HCN_LEVEL_ENERGIES = np.array([0., 711.98, 1411.41, 2096.85, 3311.48, 4004.17])


def main():
    engine.set_device(0)
    n_layers = 40
    grid = syn.make_grid(2990.0, 5e-4, 40000)
    atm = syn.make_atmosphere(n_layers, 12)
    z = atm["z"]
    Lh = syn.make_lines(1200, grid, config_id=5, n_levels=6)
    Lh["a_coeff"] = Lh["a_coeff"] * 30.0
    ch4 = retrieval.LevelGas("CH4", engine.LineSet(syn.make_lines(4000, grid, config_id=3, n_levels=12), grid, 6, 1, syn.CH4_MM,
                                                   syn.CH4_LEVEL_ENERGIES), np.full(n_layers, 0.0148), atm["tvib"],
                             syn.CH4_ISO_RATIO)
    hcn = retrieval.Gas("HCN", engine.LineSet(Lh, grid, 23, 1, HCN_MM, HCN_LEVEL_ENERGIES), np.full(n_layers, 2e-6),
                        HCN_ISO_RATIO)
    bands = np.linspace(1e7 / grid[-1] + 1.0, 1e7 / grid[0] - 1.0, 10)
    scene = retrieval.LimbScene(grid, z, atm["temps"], atm["press"], [hcn, ch4], bands, np.full(10, 1.1))
    pixels = [retrieval.LimbPixel(200.0 + 90.0 * i, fov_half=15.0, pixel_rot=10.0 * (i % 3)) for i in range(6)]

    hcn_nodes = [200.0, 450.0, 750.0]
    apr, sig_hcn = np.full(3, 2e-6), np.full(3, 1e-6)
    sig_offset, true_offset = 4.0, 2.0
    x_true = np.concatenate([1.3 * apr, [true_offset]])

    def bayes(x=None, pointing=True):
        bs = smm.BayesSet(tag="HCN VMR + pointing offset")
        bs.add_set(smm.LinearProfile_1D_new("HCN", z, hcn_nodes, apr, sig_hcn, first_guess_prof=None if x is None else x[:3]))
        if pointing:
            bs.add_set(retrieval.Pointing((0.0, sig_offset)))
        return bs

    # the truth: its profile into the scene, its spectra seen from where the lines of sight really are
    retrieval._state_into_gases(scene, bayes(x_true, pointing=False))
    moved = [retrieval.LimbPixel(p.limb_tg_alt + true_offset, fov_half=p.fov_half, pixel_rot=p.pixel_rot) for p in pixels]
    rng = np.random.default_rng(7)
    for pix, y in zip(pixels, retrieval.radtrans(scene, moved)):
        sig = np.full(y.spectrum.size, 2e-4 * np.abs(y.spectrum).max())
        pix.observation = retrieval.Spectrum(y.spectrum + sig * rng.standard_normal(sig.size), bands)
        pix.noise = retrieval.Spectrum(sig, bands)

    chi, _, _, bs = retrieval.inversion_state(scene, bayes(), pixels, max_it=10, bands_in_kernel=True)
    x = bs.param_vector()
    for it, c in enumerate(bs.history):
        print("iteration %d: chi square %.3f" % (it, c))
    print("stopped: %s" % bs.stop)
    print("HCN nodes   retrieved %s  truth %s" % (np.array2string(x[:3], precision=3), np.array2string(x_true[:3], precision=3)))
    print("offset      retrieved %.4f km (+- %.4f)  truth %.4f km" % (x[3], np.sqrt(bs.VCM[3, 3]), x_true[3]))
    # the same observations with the pixels' altitudes taken as exact
    _, _, _, fixed = retrieval.inversion_state(scene, bayes(pointing=False), pixels, max_it=10, bands_in_kernel=True)
    xf = fixed.param_vector()
    print("pointing held fixed: chi square %.3f -> %.3f, HCN nodes %s" % (fixed.history[0], fixed.history[-1],
                                                                         np.array2string(xf, precision=3)))
    err = lambda v: np.linalg.norm((v[:3] - x_true[:3]) / sig_hcn)
    print("HCN profile error in a-priori sigmas: %.2f with the pointing in the state, %.2f without" % (err(x), err(xf)))
    assert bs.history[-1] < bs.history[0], "chi square did not fall"
    assert abs(x[3] - x_true[3]) < abs(x_true[3])


if __name__ == "__main__":
    main()
