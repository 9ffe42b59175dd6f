#!/usr/bin/env python3
"""Multiple scattering on 3-D limb rays: every LOS step under its own solar zenith angle, the diffuse field included
(LimbScene.sunlit_steps, engine.diffuse_source_columns).  The three rays of examples/solar_haze_limb.py over
a reflecting lower boundary: the two-stream field is solved at n_columns solar zenith angles equally spaced in cos SZA over
the steps' range, all in one call, and each step takes the field linear in cos SZA between its two neighbours.  Printed:
the band radiances with n_columns = 1, 2, 4, 8 and their differences against 8 -- how many columns the rays need -- beside
the same rays with order one alone and without the sun.

The haze table is synthetic, the sun a black body at Saturn's distance.  Needs an MI355X:  python examples/solar_haze_limb_3d.py
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from spectrobot_amd import engine, geometry, retrieval, synthetic as syn          # noqa: E402

ALBEDO, G, GROUND = 0.9, 0.5, 0.3


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
    widths = np.full(10, 0.3)
    irradiance = geometry.solar_irradiance(grid)
    sza, phase = 30.0, 60.0

    def scene(multiple):
        return retrieval.LimbScene(grid, z, atm["temps"], atm["press"], [ch4, haze], bands, widths,
                                   sun=retrieval.Sun(sza, phase, irradiance, multiple=multiple, surface_albedo=GROUND))

    z_tans = [150.0, 300.0, 450.0]
    one = scene(False)
    L3 = geometry.limb_los_3d(z, one.nd, [ch4.vmr, haze.vmr], z_tans, sza, 40.0)
    los = engine.LimbLOS(L3["seg_off"], L3["seg_layer"], L3["pt_off"], L3["x"], L3["nd"], L3["vmr"], col_scale=[ch4.iso_ratio, 1.0])
    band = lambda pairs: engine.hires_to_lowres(engine.limb_rays(pairs, los), grid, bands, widths)
    print("%d steps on three rays; cos SZA along them %.3f .. %.3f; ground albedo %.1f" % (len(L3["seg_mu"]), L3["seg_mu"].min(), L3["seg_mu"].max(), GROUND))
    y_single = band(one.sunlit_steps(L3))
    multi = scene(True)
    y = {n: band(multi.sunlit_steps(L3, n_columns=n)) for n in (1, 2, 4, 8)}
    for r, zt in enumerate(z_tans):
        print("tangent %5.0f km: mean band radiance, order one %.4e, with the diffuse field (8 columns) %.4e (x %.3f)"
              % (zt, y_single[r].mean(), y[8][r].mean(), y[8][r].mean() / y_single[r].mean()))
    print("largest band radiance difference against 8 columns, relative, ray by ray:")
    for n in (1, 2, 4):
        print("  n_columns %d: %s" % (n, "  ".join("%.2e" % v for v in np.max(np.abs(y[n] - y[8]) / np.abs(y[8]), axis=1))))


if __name__ == "__main__":
    main()
