#!/usr/bin/env python3
"""A sunlit haze on the limb with multiple scattering: retrieval.Sun(..., multiple=True) adds the diffuse field of a
plane-parallel two-stream solve under the spherical direct beam to the haze's emission rows (engine.diffuse_source; DESIGN
4.11b); order one stays the single-scattering rows of examples/solar_haze_limb.py.  Two parts:

  forward     the limb bands of the same scene with single and with multiple scattering side by side, and their ratio
              per tangent altitude -- the share of the light that order one alone leaves out
  retrieval   a twin retrieval of the haze profile (with the CH4 VMR) whose observations carry the diffuse light, fitted
              with it and -- the same observations -- with order one alone

The haze table is synthetic, the sun a black body at Saturn's distance, the scene starts above the ground
(surface_albedo = 0: everything below absorbs).  Needs an MI355X:  python examples/multiple_scattering_haze.py
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from spectrobot_amd import engine, geometry, retrieval, synthetic as syn          # noqa: E402
from spectrobot_amd import spect_main_module as smm                               # noqa: E402

ALBEDO, G = 0.9, 0.5
SZA, PHASE = 30.0, 60.0


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
    irradiance = geometry.solar_irradiance(grid)
    single, multiple = retrieval.Sun(SZA, PHASE, irradiance), retrieval.Sun(SZA, PHASE, irradiance, multiple=True, surface_albedo=0.0)
    scene = retrieval.LimbScene(grid, z, atm["temps"], atm["press"], [ch4, haze], bands, np.full(10, 0.3), sun=single)

    # ---- forward: the two suns side by side ----------------------------------------------------------------------------
    pixels = [retrieval.LimbPixel(120.0 + 60.0 * i, fov_half=8.0, pixel_rot=10.0 * (i % 3)) for i in range(8)]
    y1 = np.array([y.spectrum for y in retrieval.radtrans(scene, pixels)])
    scene.sun = multiple
    ym = np.array([y.spectrum for y in retrieval.radtrans(scene, pixels)])
    print("limb bands, single | multiple scattering (mean over the bands) and the share of the diffuse part per tangent altitude")
    for pix, a, b in zip(pixels, y1, ym):
        print("  tangent %5.0f km: %.4e | %.4e   ratio %.4f (bands %.4f .. %.4f), diffuse share %.1f %%"
              % (pix.limb_tg_alt, a.mean(), b.mean(), b.mean() / a.mean(), (b / a).min(), (b / a).max(), 100 * (1 - a.mean() / b.mean())))

    # ---- twin retrieval: the observations carry the diffuse light -------------------------------------------------------
    nodes = {"CH4": [140.0, 350.0, 650.0], "haze": [130.0, 300.0, 600.0]}
    apr = {"CH4": np.full(3, 1.3e-4), "haze": 0.5 * np.array([0.7, 0.45, 0.2])}
    truth = {"CH4": np.array([1.7e-4, 1.5e-4, 1.15e-4]), "haze": 0.5 * np.array([1.0, 0.55, 0.14])}

    def bayes(values):
        bs = smm.BayesSet(tag="CH4 VMR + sunlit haze, multiple scattering")
        for name in ("CH4", "haze"):
            bs.add_set(smm.LinearProfile_1D_new(name, z, nodes[name], apr[name], 0.5 * apr[name], first_guess_prof=values[name]))
        return bs

    retrieval._state_into_gases(scene, bayes(truth))
    rng = np.random.default_rng(11)
    for pix, yy in zip(pixels, retrieval.radtrans(scene, pixels)):
        sig = 0.004 * np.abs(yy.spectrum).max() * np.ones_like(yy.spectrum)
        pix.observation = retrieval.Spectrum(yy.spectrum + sig * rng.standard_normal(sig.size), scene.bands_nm)
        pix.noise = retrieval.Spectrum(sig, scene.bands_nm)
    x_true = np.concatenate([truth["CH4"], truth["haze"]])
    print("truth                ", np.array2string(x_true, precision=4))
    print("a priori             ", np.array2string(np.concatenate([apr["CH4"], apr["haze"]]), precision=4))
    for name, sun in (("multiple scattering", multiple), ("single scattering  ", single)):
        scene.sun = sun
        chi, _, _, b = retrieval.inversion_state(scene, bayes(apr), pixels, max_it=10)
        print("%s: %d iterations (%s), chi square %s\n  retrieved          %s"
              % (name, len(b.history), b.stop, np.array2string(np.array(b.history), precision=4), np.array2string(b.param_vector(), precision=4)))


if __name__ == "__main__":
    main()
