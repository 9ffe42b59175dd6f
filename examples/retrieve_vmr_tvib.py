#!/usr/bin/env python3
"""Twin experiment on a mixed state vector: the VMR profile of an LTE trace gas (HCN-like) together with the
vibrational-temperature offset of one excited CH4 level, retrieved by retrieval.inversion_state -- one Jacobian call per
iteration for both kinds of parameter (LevelFactored.state_jacobian) -- at the reduced size of examples/retrieve_tvib.py.

  truth      the HCN profile scaled by 1.3, Tvib of CH4 level 5 = the atmosphere's profile + a smooth bump of 6 K
  "observed" the band spectra of 6 limb pixels (three lines of sight each, closed-form field of view) through the truth,
             plus noise
  retrieved  3 VMR nodes of HCN and 5 nodes of the Tvib offset, Levenberg-Marquardt optimal estimation

Prints the chi-square history and the retrieved state next to the truth.  Needs an MI355X:
python examples/retrieve_vmr_tvib.py
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from spectrobot_amd import engine, retrieval, synthetic as syn          # noqa: E402
from spectrobot_amd import spect_main_module as smm                     # noqa: E402

LEVEL = 5
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
    hcn = retrieval.Gas("HCN", engine.LineSet(Lh, grid, 23, 1, HCN_MM, HCN_LEVEL_ENERGIES), np.full(n_layers, 2e-6), HCN_ISO_RATIO)
    bands = np.linspace(1e7 / grid[-1] + 1.0, 1e7 / grid[0] - 1.0, 10)
    scene = retrieval.LimbScene(grid, z, atm["temps"], atm["press"], [hcn, ch4], bands, np.full(10, 1.1))
    pixels = [retrieval.LimbPixel(200.0 + 90.0 * i, fov_half=15.0, pixel_rot=10.0 * (i % 3)) for i in range(6)]

    hcn_nodes, tv_nodes = [200.0, 450.0, 750.0], list(np.linspace(200.0, 800.0, 5))
    apr, sig_hcn, sig_tv = np.full(3, 2e-6), np.full(3, 1e-6), np.full(5, 4.0)
    x_true = np.concatenate([1.3 * apr, 6.0 * np.exp(-0.5 * ((np.array(tv_nodes) - 420.0) / 130.0) ** 2)])

    def bayes(x=None):
        bs = smm.BayesSet(tag="HCN VMR + Tvib offset of CH4 level %d" % LEVEL)
        bs.add_set(smm.LinearProfile_1D_new("HCN", z, hcn_nodes, apr, sig_hcn, first_guess_prof=None if x is None else x[:3]))
        bs.add_set(retrieval.TvibProfile("CH4", LEVEL, z, tv_nodes, sig_tv, first_guess=None if x is None else x[3:]))
        return bs

    # the truth into the gases, its spectra as observations
    truth = bayes(x_true)
    hcn.add_clim(truth.sets["HCN"].profile())
    tv = ch4.tvib0.copy()
    tv[LEVEL] += truth.sets["tvib:CH4:%d" % LEVEL].profile()
    ch4.set_tvib(tv)
    rng = np.random.default_rng(7)
    for pix, y in zip(pixels, retrieval.radtrans(scene, pixels)):
        sig = np.full(y.spectrum.size, 2e-4 * np.abs(y.spectrum).max())
        pix.observation = retrieval.Spectrum(y.spectrum + sig * rng.standard_normal(sig.size), bands)
        pix.noise = retrieval.Spectrum(sig, bands)

    chi, _, _, bs = retrieval.inversion_state(scene, bayes(), pixels, max_it=10)
    x = bs.param_vector()
    sigma = np.concatenate([sig_hcn, sig_tv])
    for it, c in enumerate(bs.history):
        print("iteration %d: chi square %.3f" % (it, c))
    print("stopped: %s" % bs.stop)
    print("HCN nodes  retrieved %s  truth %s" % (np.array2string(x[:3], precision=3), np.array2string(x_true[:3], precision=3)))
    print("Tvib nodes retrieved %s  truth %s  [K]" % (np.array2string(x[3:], precision=2), np.array2string(x_true[3:], precision=2)))
    print("state error in a-priori sigmas: %.2f before, %.2f after"
          % (np.linalg.norm((bayes().param_vector() - x_true) / sigma), np.linalg.norm((x - x_true) / sigma)))
    assert bs.history[-1] < bs.history[0], "chi square did not fall"


if __name__ == "__main__":
    main()
