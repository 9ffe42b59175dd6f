#!/usr/bin/env python3
"""A scattering haze on the night-side limb: retrieval.ThermalScattering makes the haze a thermal scatterer
(engine.diffuse_thermal_source).  Without it a TableGas(solar=dict(albedo=0.9, ...)) emits abs B -- as if all
of its extinction were absorption -- and scatters no thermal light; with it the haze emits (1 - albedo) abs B by
Kirchhoff's law and scatters the diffuse field of the layers' (and the surface's) thermal emission into the line of sight.

The scene is the small haze scene of the tests (tests/absorber_table_cases.py, tests/solar_source_cases.py): a CH4-like
line gas and a synthetic haze table on 600 grid points near 3290 cm^-1 and 12 layers, no sun.  Prints the limb bands with
and without thermal_scattering and their ratio per tangent height, once above a cold space below (nothing emits) and once
above a surface at 160 K.  Needs an MI355X:  python examples/night_haze_limb.py
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from spectrobot_amd import engine, retrieval, synthetic as syn          # noqa: E402

ALBEDO, G = 0.9, 0.5
N_GRID, N_LAYERS = 600, 12


def main():
    engine.set_device(0)
    grid = syn.make_grid(3290.0, 5e-4, N_GRID)
    atm = syn.make_atmosphere(N_LAYERS, 12)
    z = atm["z"]
    lines = syn.make_lines(300, grid, config_id=4, n_levels=12)
    lines["a_coeff"] = lines["a_coeff"] * 1e-4          # a weak band: limb optical depths of order one, like the haze's
    lineset = engine.LineSet(lines, grid, 6, 1, syn.CH4_MM, syn.CH4_LEVEL_ENERGIES)
    v0, v1 = grid[0] - 0.01, grid[-1] + 0.01
    dv = (v1 - v0) / 50.0
    nu = v0 + dv * np.arange(51)
    shape = 1.0 + 0.3 * np.cos((nu - v0) / (v1 - v0) * 7.0) - 0.2 * (nu - v0) / (v1 - v0)
    table = engine.AbsorberTable([(100.0, v0, dv, 2.4e-26 * shape), (250.0, v0, dv, 3.9e-26 * shape * (1.0 + 0.1 * np.sin((nu - v0) * 9.0)))])

    def gases():        # (fresh gas objects per scene: a gas keeps its scene's emission rows)
        return [retrieval.Gas("CH4", lineset, np.full(N_LAYERS, 1.48e-4), syn.CH4_ISO_RATIO, tvib=atm["tvib"]),
                retrieval.TableGas("haze", table, 0.5 * np.exp(-(z - z[0]) / 250.0), solar=dict(albedo=ALBEDO, g=G))]

    lam = np.linspace(1e7 / grid[-1] + 0.02, 1e7 / grid[0] - 0.02, 6)
    span = z[-1] - z[0]
    pixels = [retrieval.LimbPixel(z[0] + (0.03 + 0.09 * i) * span, fov_half=0.01 * span, pixel_rot=10.0 * (i % 3)) for i in range(6)]

    def bands(thermal_scattering):
        scene = retrieval.LimbScene(grid, z, atm["temps"], atm["press"], gases(), lam, np.full(6, 0.03),
                                    thermal_scattering=thermal_scattering)
        return np.array([y.spectrum for y in retrieval.radtrans(scene, pixels)])

    plain = bands(None)
    for what, ts in (("nothing below emits", retrieval.ThermalScattering()),
                     ("a surface at 160 K, albedo 0.3, below", retrieval.ThermalScattering(surface_temperature=160.0, surface_albedo=0.3))):
        y = bands(ts)
        print("night-side limb bands, abs B | thermal scattering (mean over the bands), %s" % what)
        for pix, a, b in zip(pixels, plain, y):
            print("  tangent %5.0f km: %.4e | %.4e   ratio %.4f (bands %.4f .. %.4f)"
                  % (pix.limb_tg_alt, a.mean(), b.mean(), b.mean() / a.mean(), (b / a).min(), (b / a).max()))


if __name__ == "__main__":
    main()
