#!/usr/bin/env python3
"""The twin retrieval of examples/multiple_scattering_haze.py above a reflecting boundary, with and without the derivative
of the sunlit rows: retrieval.inversion_state(solar_attenuation=True, diffuse_jacobian=True) carries, in the VMR columns of
every iteration's Jacobian, the derivative through the single-scattering rows' optical depth and through the
two-stream solve of the diffuse rows (engine.diffuse_jacobian).  With surface_albedo = 0.3 the diffuse light
is a large share of the bands, and a Jacobian that holds it fixed is not the derivative of the forward model: the loop
then converges linearly, at the rate of the share it leaves out.  Prints the iteration counts and chi square histories of
the same noise-free observations fitted with the flags off and on.

The haze table is synthetic, the sun a black body at Saturn's distance.  Needs an MI355X:
python examples/retrieve_diffuse_haze.py
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from spectrobot_amd import engine, geometry, retrieval, synthetic as syn          # noqa: E402
from spectrobot_amd import spect_main_module as smm                               # noqa: E402

ALBEDO, G = 0.9, 0.5
SZA, PHASE, GROUND = 30.0, 60.0, 0.3


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
    haze = retrieval.TableGas("haze", table, 0.5 * np.exp(-(z - z[0]) / 250.0), solar=dict(albedo=ALBEDO, g=G))
    bands = np.linspace(1e7 / grid[-1] + 0.3, 1e7 / grid[0] - 0.3, 10)
    sun = retrieval.Sun(SZA, PHASE, geometry.solar_irradiance(grid), multiple=True, surface_albedo=GROUND)
    scene = retrieval.LimbScene(grid, z, atm["temps"], atm["press"], [ch4, haze], bands, np.full(10, 0.3), sun=sun)
    pixels = [retrieval.LimbPixel(120.0 + 60.0 * i, fov_half=8.0, pixel_rot=10.0 * (i % 3)) for i in range(8)]

    nodes = {"CH4": [140.0, 350.0, 650.0], "haze": [130.0, 300.0, 600.0]}
    apr = {"CH4": np.full(3, 1.3e-4), "haze": 0.5 * np.array([0.7, 0.45, 0.2])}
    truth = {"CH4": np.array([1.7e-4, 1.5e-4, 1.15e-4]), "haze": 0.5 * np.array([1.0, 0.55, 0.14])}

    def bayes(values):
        bs = smm.BayesSet(tag="CH4 VMR + sunlit haze above a reflecting boundary")
        for name in ("CH4", "haze"):
            bs.add_set(smm.LinearProfile_1D_new(name, z, nodes[name], apr[name], 0.5 * apr[name], first_guess_prof=values[name]))
        return bs

    retrieval._state_into_gases(scene, bayes(truth))
    for pix, yy in zip(pixels, retrieval.radtrans(scene, pixels)):        # noise-free observations, the noise as the weights
        sig = 0.004 * np.abs(yy.spectrum).max() * np.ones_like(yy.spectrum)
        pix.observation, pix.noise = retrieval.Spectrum(yy.spectrum.copy(), scene.bands_nm), retrieval.Spectrum(sig, scene.bands_nm)
    x_true = np.concatenate([truth["CH4"], truth["haze"]])
    print("truth     ", np.array2string(x_true, precision=4))
    print("a priori  ", np.array2string(np.concatenate([apr["CH4"], apr["haze"]]), precision=4))
    for name, flags in (("flags off", {}), ("flags on ", dict(solar_attenuation=True, diffuse_jacobian=True))):
        chi, _, _, b = retrieval.inversion_state(scene, bayes(apr), pixels, max_it=20, lambda_LM=0.0, **flags)
        print("%s: %d iterations (%s), chi square %s\n  retrieved %s"
              % (name, len(b.history), b.stop, np.array2string(np.array(b.history), precision=5), np.array2string(b.param_vector(), precision=4)))


if __name__ == "__main__":
    main()
