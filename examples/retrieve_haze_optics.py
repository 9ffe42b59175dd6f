#!/usr/bin/env python3
"""A wrong ground albedo, fitted: the scene of examples/retrieve_diffuse_haze.py and its noise-free observations come from a
Lambertian boundary of albedo 0.3 below the lowest level; the retrieval starts from 0.1.  The state is the haze profile's
nodes plus the surface albedo -- retrieval.HazeOptics(surface_albedo=(apriori, err, first_guess)), a set named "optics"
that inversion_state takes beside the profiles; its Jacobian column is LimbScene.optics_jacobian's, the derivative of the
two-stream diffuse rows to the boundary's albedo (engine.diffuse_optics_jacobian).  Prints the iterations,
the chi square history and the retrieved albedo with its a-posteriori sigma, and beside them the same observations fitted
with the albedo held at 0.1: the haze profile alone cannot make up for it.  HazeOptics also carries a haze's single-
scattering albedo and asymmetry parameter (albedo={"haze": spec}, g={"haze": spec}); with the haze's own profile in the
state its albedo is nearly degenerate (in thin single scattering ssa x extinction is one number).

The haze table is synthetic, the sun a black body at Saturn's distance.  Needs an MI355X:
python examples/retrieve_haze_optics.py
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

    retrieval._state_into_gases(scene, bayes(truth))                      # (CH4 stays at the truth throughout)
    for pix, yy in zip(pixels, retrieval.radtrans(scene, pixels)):        # noise-free observations, the noise as the weights
        sig = 0.004 * np.abs(yy.spectrum).max() * np.ones_like(yy.spectrum)
        pix.observation, pix.noise = retrieval.Spectrum(yy.spectrum.copy(), scene.bands_nm), retrieval.Spectrum(sig, scene.bands_nm)
    print("truth: haze nodes %s, surface albedo %.2f" % (np.array2string(truth["haze"], precision=4), GROUND))
    for fitted in (True, False):
        bs = smm.BayesSet(tag="sunlit haze above a boundary of unknown albedo")
        bs.add_set(bayes(apr).sets["haze"])
        scene.sun.surface_albedo = 0.1
        if fitted:
            bs.add_set(retrieval.HazeOptics(surface_albedo=(0.1, 0.1, 0.1)))
        chi, _, _, b = retrieval.inversion_state(scene, bs, pixels, max_it=20, lambda_LM=0.0)
        sigma = np.sqrt(np.diag(b.VCM))
        print("surface albedo %s: %d iterations (%s), chi square %s\n  retrieved %s\n  a-posteriori sigma %s"
              % ("fitted      " if fitted else "held at 0.10", len(b.history), b.stop, np.array2string(np.array(b.history), precision=5),
                 np.array2string(b.param_vector(), precision=4), np.array2string(sigma, precision=4)))


if __name__ == "__main__":
    main()
