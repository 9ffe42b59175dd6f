#!/usr/bin/env python3
"""Twin experiment with an absorber that has no lines: the VMR profile of CH4 retrieved together with the extinction
profile of a haze -- a retrieval.TableGas on an engine.AbsorberTable, its "VMR" the extinction per unit density -- by
retrieval.inversion_state, which takes the scene as it is: the haze's pair sits on the coefficient rows beside the line
gas's, its retrieval set is an ordinary column set.  The pixels reach down to 120 km, below the altitude where the haze
matters (the reference's production driver throws those away).

  truth      CH4 and haze profiles both off their a priori
  "observed" the band spectra of 8 limb pixels (three lines of sight each, closed-form field of view) through the truth,
             plus noise
  retrieved  3 VMR nodes of CH4 and 3 nodes of the haze profile

The table is synthetic (a smooth extinction cross-section at two temperatures): spect_classes.read_xsc / read_cia return
the same kind of set list from HITRAN's files.  Prints the chi-square history and the retrieved state next to the truth.
Needs an MI355X:  python examples/retrieve_haze.py
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from spectrobot_amd import engine, retrieval, synthetic as syn          # noqa: E402
from spectrobot_amd import spect_main_module as smm                     # noqa: E402


def main():
    engine.set_device(0)
    n_layers = 24
    grid = syn.make_grid(3290.0, 5e-4, 8000)
    atm = syn.make_atmosphere(n_layers, 12)
    z = atm["z"]
    lines = syn.make_lines(2000, grid, config_id=4, n_levels=12)
    lines["a_coeff"] = lines["a_coeff"] * 1e-4          # a weak band: limb optical depths of order one, like the haze's
    ch4 = retrieval.Gas("CH4", engine.LineSet(lines, grid, 6, 1, syn.CH4_MM, syn.CH4_LEVEL_ENERGIES), np.full(n_layers, 1.48e-4),
                        syn.CH4_ISO_RATIO, tvib=atm["tvib"])
    v0, v1 = grid[0] - 0.05, grid[-1] + 0.05
    nu = np.linspace(v0, v1, 201)
    shape = 1.0 + 0.3 * np.cos((nu - v0) / (v1 - v0) * 7.0) - 0.2 * (nu - v0) / (v1 - v0)
    table = engine.AbsorberTable([(100.0, v0, nu[1] - nu[0], 2.4e-26 * shape), (250.0, v0, nu[1] - nu[0], 3.9e-26 * shape)])
    haze = retrieval.TableGas("haze", table, np.exp(-(z - z[0]) / 250.0))
    bands = np.linspace(1e7 / grid[-1] + 0.3, 1e7 / grid[0] - 0.3, 10)
    scene = retrieval.LimbScene(grid, z, atm["temps"], atm["press"], [ch4, haze], bands, np.full(10, 0.3))
    pixels = [retrieval.LimbPixel(120.0 + 60.0 * i, fov_half=8.0, pixel_rot=10.0 * (i % 3)) for i in range(8)]

    nodes = {"CH4": [140.0, 350.0, 650.0], "haze": [130.0, 300.0, 600.0]}
    apr = {"CH4": np.full(3, 1.3e-4), "haze": np.array([0.7, 0.45, 0.2])}
    truth = {"CH4": np.array([1.7e-4, 1.5e-4, 1.15e-4]), "haze": np.array([1.0, 0.55, 0.14])}

    def bayes(values):
        bs = smm.BayesSet(tag="CH4 VMR + haze extinction")
        for name in ("CH4", "haze"):
            bs.add_set(smm.LinearProfile_1D_new(name, z, nodes[name], apr[name], 0.5 * apr[name], first_guess_prof=values[name]))
        return bs

    retrieval._state_into_gases(scene, bayes(truth))
    rng = np.random.default_rng(11)
    for pix, y in zip(pixels, retrieval.radtrans(scene, pixels)):
        sig = 0.004 * np.abs(y.spectrum).max() * np.ones_like(y.spectrum)
        pix.observation = retrieval.Spectrum(y.spectrum + sig * rng.standard_normal(sig.size), scene.bands_nm)
        pix.noise = retrieval.Spectrum(sig, scene.bands_nm)

    chi, _, _, b = retrieval.inversion_state(scene, bayes(apr), pixels, max_it=10)
    x_true = np.concatenate([truth["CH4"], truth["haze"]])
    print("iterations %d (%s), chi square %s" % (len(b.history), b.stop, np.array2string(np.array(b.history), precision=4)))
    print("retrieved ", np.array2string(b.param_vector(), precision=4))
    print("truth     ", np.array2string(x_true, precision=4))
    print("a priori  ", np.array2string(np.concatenate([apr["CH4"], apr["haze"]]), precision=4))


if __name__ == "__main__":
    main()
