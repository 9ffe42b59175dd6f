#!/usr/bin/env python3
"""Twin experiment on a scene of SIX gas slots -- more than the four the folded kernels carry: three line gases (CH4, its
13CH4 isotopologue as a Gas of its own, an HCN-like gas), a haze and two more tabulated absorbers, each with a VMR of its
own.  retrieval.inversion_state takes up to eight slots (engine.max_gases()): the radiances and the state Jacobian run the
path-order and state kernels' instances for five to eight gases.  Nothing is folded into another gas by a ratio
(TableGas(accumulate_into=...), engine.mix_gases), so the table in slot 5 keeps a retrieval set of its own.

  truth      the CH4 profile and the profile of the table in slot 5 both off their a priori
  "observed" the band spectra of 8 limb pixels (three lines of sight each, closed-form field of view) through the truth
             (retrieval.simulate: radtrans and the loop-in-one-call drivers stay at four slots), plus noise
  retrieved  3 VMR nodes of CH4 (slot 0) and 3 nodes of the table gas in slot 5

The tables are synthetic (smooth cross-sections at two temperatures).  Prints the chi-square history and the retrieved
state next to the truth.  Needs an MI355X:  python examples/retrieve_six_gases.py
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import bench_configs as bc                                              # noqa: E402
from spectrobot_amd import engine, retrieval, synthetic as syn          # noqa: E402
from spectrobot_amd import spect_main_module as smm                     # noqa: E402


def main():
    engine.set_device(0)
    n_layers = 24
    grid = syn.make_grid(3290.0, 5e-4, 8000)
    atm = syn.make_atmosphere(n_layers, 12)
    z = atm["z"]

    def line_gas(name, n_lines, config_id, n_levels, weak, mol, iso, mm, energies, vmr, ratio):
        lines = syn.make_lines(n_lines, grid, config_id=config_id, n_levels=n_levels)
        lines["a_coeff"] = lines["a_coeff"] * weak       # weak bands: limb optical depths of order one, like the tables'
        return retrieval.Gas(name, engine.LineSet(lines, grid, mol, iso, mm, energies), np.full(n_layers, vmr), ratio)

    ch4 = line_gas("CH4", 2000, 4, 12, 1e-4, 6, 1, syn.CH4_MM, syn.CH4_LEVEL_ENERGIES, 1.48e-4, syn.CH4_ISO_RATIO)
    c13 = line_gas("13CH4", 800, 6, 12, 1e-4, 6, 1, syn.CH4_MM, syn.CH4_LEVEL_ENERGIES, 1.48e-4, 0.0111)
    hcn = line_gas("HCN", 800, 5, 6, 1e-3, 23, 1, bc.HCN_MM, bc.HCN_LEVEL_ENERGIES, 2e-6, bc.HCN_ISO_RATIO)
    v0, v1 = grid[0] - 0.05, grid[-1] + 0.05
    nu = np.linspace(v0, v1, 201)

    def table(amp, phase):
        shape = 1.0 + 0.3 * np.cos((nu - v0) / (v1 - v0) * 7.0 + phase) - 0.2 * (nu - v0) / (v1 - v0)
        return engine.AbsorberTable([(100.0, v0, nu[1] - nu[0], amp * shape), (250.0, v0, nu[1] - nu[0], 1.6 * amp * shape)])

    haze = retrieval.TableGas("haze", table(2.4e-26, 0.0), np.exp(-(z - z[0]) / 250.0))
    c2h6 = retrieval.TableGas("C2H6", table(3e-21, 1.0), np.full(n_layers, 1e-5))
    c3h8 = retrieval.TableGas("C3H8", table(2e-20, 2.0), np.full(n_layers, 2e-6))
    bands = np.linspace(1e7 / grid[-1] + 0.3, 1e7 / grid[0] - 0.3, 10)
    scene = retrieval.LimbScene(grid, z, atm["temps"], atm["press"], [ch4, c13, hcn, haze, c2h6, c3h8], bands, np.full(10, 0.3))
    print("gas slots: %d of %d (the folded kernels carry %d)" % (len(scene.gases), engine.max_gases(), engine.max_gases(folded=True)))
    pixels = [retrieval.LimbPixel(120.0 + 60.0 * i, fov_half=8.0, pixel_rot=10.0 * (i % 3)) for i in range(8)]

    nodes = {"CH4": [140.0, 350.0, 650.0], "C3H8": [130.0, 300.0, 600.0]}
    apr = {"CH4": np.full(3, 1.3e-4), "C3H8": np.full(3, 2e-6)}
    truth = {"CH4": np.array([1.7e-4, 1.5e-4, 1.15e-4]), "C3H8": np.array([2.8e-6, 2.3e-6, 1.5e-6])}

    def bayes(values):
        bs = smm.BayesSet(tag="CH4 (slot 0) + C3H8 table (slot 5)")
        for name in ("CH4", "C3H8"):
            bs.add_set(smm.LinearProfile_1D_new(name, z, nodes[name], apr[name], 0.5 * apr[name], first_guess_prof=values[name]))
        return bs

    retrieval._state_into_gases(scene, bayes(truth))
    rng = np.random.default_rng(11)
    for pix, y in zip(pixels, retrieval.simulate(scene, pixels)[0]):
        sig = 0.004 * np.abs(y.spectrum).max() * np.ones_like(y.spectrum)
        pix.observation = retrieval.Spectrum(y.spectrum + sig * rng.standard_normal(sig.size), scene.bands_nm)
        pix.noise = retrieval.Spectrum(sig, scene.bands_nm)

    chi, _, _, b = retrieval.inversion_state(scene, bayes(apr), pixels, max_it=10)
    x_true = np.concatenate([truth["CH4"], truth["C3H8"]])
    print("iterations %d (%s), chi square %s" % (len(b.history), b.stop, np.array2string(np.array(b.history), precision=4)))
    print("retrieved ", np.array2string(b.param_vector(), precision=4))
    print("truth     ", np.array2string(x_true, precision=4))
    print("a priori  ", np.array2string(np.concatenate([apr["CH4"], apr["C3H8"]]), precision=4))


if __name__ == "__main__":
    main()
