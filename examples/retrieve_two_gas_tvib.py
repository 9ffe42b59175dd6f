#!/usr/bin/env python3
"""Twin experiment on the vibrational temperatures of TWO non-LTE gases: the Tvib offset of one level of an HCN-like gas
together with the Tvib offsets of two excited CH4 levels, retrieved by retrieval.inversion_state -- both gases on the
level-factored route, and ONE Jacobian call per iteration for the level parameters of both
(engine.LevelFactoredSet.state_jacobian: every ray is walked once) -- at the reduced size of examples/retrieve_vmr_tvib.py.

  truth      Tvib of HCN level 1 = its reference + a smooth bump of 5 K, Tvib of CH4 level 5 + a bump of 6 K, of CH4
             level 2 - 4 K
  "observed" the band spectra of 6 limb pixels (three lines of sight each, closed-form field of view) through the truth,
             plus noise
  retrieved  4 nodes of each of the three Tvib offsets, Levenberg-Marquardt optimal estimation

Prints the chi-square history and the retrieved state next to the truth.  Needs an MI355X:
python examples/retrieve_two_gas_tvib.py
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from spectrobot_amd import engine, retrieval, synthetic as syn          # noqa: E402
from spectrobot_amd import spect_main_module as smm                     # noqa: E402

SETS = (("HCN", 1, 5.0), ("CH4", 5, 6.0), ("CH4", 2, -4.0))             # gas, level, height of the truth's bump [K]
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
    tv_hcn = np.tile(atm["temps"], (6, 1)) + np.linspace(0.0, 10.0, 6)[:, None]
    hcn = retrieval.LevelGas("HCN", engine.LineSet(Lh, grid, 23, 1, HCN_MM, HCN_LEVEL_ENERGIES), np.full(n_layers, 2e-6), tv_hcn,
                             HCN_ISO_RATIO)
    bands = np.linspace(1e7 / grid[-1] + 1.0, 1e7 / grid[0] - 1.0, 10)
    scene = retrieval.LimbScene(grid, z, atm["temps"], atm["press"], [hcn, ch4], bands, np.full(10, 1.1))
    pixels = [retrieval.LimbPixel(200.0 + 90.0 * i, fov_half=15.0, pixel_rot=10.0 * (i % 3)) for i in range(6)]

    tv_nodes = list(np.linspace(200.0, 800.0, 4))
    sig = np.full(4, 4.0)
    bump = np.exp(-0.5 * ((np.array(tv_nodes) - 420.0) / 130.0) ** 2)
    x_true = np.concatenate([h * bump for _, _, h in SETS])

    def bayes(x=None):
        bs = smm.BayesSet(tag="Tvib offsets of an HCN level and of two CH4 levels")
        for i, (gas, level, _) in enumerate(SETS):
            bs.add_set(retrieval.TvibProfile(gas, level, z, tv_nodes, sig, first_guess=None if x is None else x[4 * i:4 * i + 4]))
        return bs

    # the truth into the gases, its spectra as observations
    retrieval._state_into_gases(scene, bayes(x_true))
    rng = np.random.default_rng(7)
    for pix, y in zip(pixels, retrieval.radtrans(scene, pixels)):
        s = np.full(y.spectrum.size, 2e-4 * np.abs(y.spectrum).max())
        pix.observation = retrieval.Spectrum(y.spectrum + s * rng.standard_normal(s.size), bands)
        pix.noise = retrieval.Spectrum(s, bands)

    chi, _, _, bs = retrieval.inversion_state(scene, bayes(), pixels, max_it=10)
    x = bs.param_vector()
    sigma = np.tile(sig, len(SETS))
    for it, c in enumerate(bs.history):
        print("iteration %d: chi square %.3f" % (it, c))
    print("stopped: %s" % bs.stop)
    for i, (gas, level, _) in enumerate(SETS):
        print("Tvib nodes of %s level %d  retrieved %s  truth %s  [K]"
              % (gas, level, np.array2string(x[4 * i:4 * i + 4], precision=2), np.array2string(x_true[4 * i:4 * i + 4], precision=2)))
    print("state error in a-priori sigmas: %.2f before, %.2f after"
          % (np.linalg.norm((bayes().param_vector() - x_true) / sigma), np.linalg.norm((x - x_true) / sigma)))
    assert bs.history[-1] < bs.history[0], "chi square did not fall"


if __name__ == "__main__":
    main()
