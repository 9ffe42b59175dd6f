#!/usr/bin/env python3
"""Twin experiment on a state vector that holds the kinetic temperature: the VMR profile of an LTE trace gas (HCN-like)
together with a temperature offset profile, retrieved by retrieval.inversion_state -- per iteration the coefficients at the
current temperatures with their temperature derivatives (the non-LTE CH4 from its level tables at T and T + dT, the trace
gas by a forward difference of the coefficient op) and ONE Jacobian call for both kinds of parameter
(sr_limb_rays_jac_state_rows_dev) -- at the reduced size of examples/retrieve_vmr_tvib.py, without noise.

  truth      the HCN profile scaled by 1.3, T = the atmosphere's profile + a smooth bump of 4 K
  "observed" the band spectra of 6 limb pixels (three lines of sight each, closed-form field of view) through the truth
  retrieved  3 VMR nodes of HCN and 4 nodes of the temperature offset, Levenberg-Marquardt optimal estimation

The temperature Jacobian holds pressure, columns and vibrational temperatures fixed (number densities and LOS columns do
not follow the offset): the twin is consistent with that, truth and retrieval alike.

Prints the chi-square history and the retrieved state next to the truth.  Needs an MI355X:
python examples/retrieve_temp_vmr.py
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
                             syn.CH4_ISO_RATIO, dT=0.05)        # the tables also at T + dT: d coefficients / dT
    hcn = retrieval.Gas("HCN", engine.LineSet(Lh, grid, 23, 1, HCN_MM, HCN_LEVEL_ENERGIES), np.full(n_layers, 2e-6), HCN_ISO_RATIO)
    bands = np.linspace(1e7 / grid[-1] + 1.0, 1e7 / grid[0] - 1.0, 10)
    scene = retrieval.LimbScene(grid, z, atm["temps"], atm["press"], [hcn, ch4], bands, np.full(10, 1.1))
    pixels = [retrieval.LimbPixel(200.0 + 90.0 * i, fov_half=15.0, pixel_rot=10.0 * (i % 3)) for i in range(6)]

    hcn_nodes, t_nodes = [200.0, 450.0, 750.0], list(np.linspace(200.0, 800.0, 4))
    apr, sig_hcn, sig_t = np.full(3, 2e-6), np.full(3, 1e-6), np.full(4, 3.0)
    x_true = np.concatenate([1.3 * apr, 4.0 * np.exp(-0.5 * ((np.array(t_nodes) - 420.0) / 130.0) ** 2)])

    def bayes(x=None):
        bs = smm.BayesSet(tag="HCN VMR + temperature offset")
        bs.add_set(smm.LinearProfile_1D_new("HCN", z, hcn_nodes, apr, sig_hcn, first_guess_prof=None if x is None else x[:3]))
        bs.add_set(retrieval.TempProfile(z, t_nodes, sig_t, first_guess=None if x is None else x[3:]))
        return bs

    # the truth into the scene (temps = temps0 + offset), its spectra as observations
    retrieval._state_into_gases(scene, bayes(x_true))
    for pix, y in zip(pixels, retrieval.radtrans(scene, pixels)):
        pix.observation = retrieval.Spectrum(y.spectrum, bands)
        pix.noise = retrieval.Spectrum(np.full(y.spectrum.size, 2e-4 * np.abs(y.spectrum).max()), bands)

    chi, _, _, bs = retrieval.inversion_state(scene, bayes(), pixels, max_it=10)
    x = bs.param_vector()
    for it, c in enumerate(bs.history):
        print("iteration %d: chi square %.4g" % (it, c))
    print("stopped: %s" % bs.stop)
    print("HCN nodes retrieved %s  truth %s" % (np.array2string(x[:3], precision=3), np.array2string(x_true[:3], precision=3)))
    print("T offsets retrieved %s  truth %s  [K]" % (np.array2string(x[3:], precision=2), np.array2string(x_true[3:], precision=2)))
    assert bs.history[-1] < bs.history[0], "chi square did not fall"


if __name__ == "__main__":
    main()
