#!/usr/bin/env python3
"""A sunlit haze on the limb: sunlight, attenuated on its way in, scattered once into the line of sight, as an emission
coefficient like any other (engine.solar_source).  Three parts:

  3-D forward   limb rays whose LOS steps carry their own solar zenith angle (geometry.limb_los_3d: one coefficient row
                per step): the slant columns towards the sun of every step (geometry.solar_columns), one solar pass over
                the steps' rows, thermal + solar, radiances -- and the same rays without the sun
  1-D scene     retrieval.LimbScene(..., sun=retrieval.Sun(sza, phase, irradiance)) with the haze as
                retrieval.TableGas(..., solar=dict(albedo=, g=)): the tangent-SZA approximation, one solar pass over the
                layer rows inside coefficients()
  retrieval     a twin retrieval of the haze profile (with the CH4 VMR) from sunlit pixels through inversion_state; the
                Jacobians hold the solar attenuation fixed within an iteration, the pass is redone between iterations.
                inversion_state(..., solar_attenuation=True) adds the derivative through the solar optical depth to the
                VMR columns: examples/retrieve_solar_attenuation.py

The haze table is synthetic, the sun a black body at Saturn's distance.  Multiple scattering above a Lambertian
boundary is examples/multiple_scattering_haze.py; refraction is not built.  Needs an MI355X:  python examples/solar_haze_limb.py
"""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from spectrobot_amd import engine, geometry, retrieval, synthetic as syn          # noqa: E402
from spectrobot_amd import spect_main_module as smm                               # noqa: E402

ALBEDO, G = 0.9, 0.5


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
    sza, phase = 30.0, 60.0
    scene = retrieval.LimbScene(grid, z, atm["temps"], atm["press"], [ch4, haze], bands, np.full(10, 0.3),
                                sun=retrieval.Sun(sza, phase, irradiance))

    # ---- 3-D forward model: one row per LOS step, each with its own cos SZA ------------------------------------------
    z_tans = [150.0, 300.0, 450.0]
    vmrs = [ch4.vmr, haze.vmr]
    L3 = geometry.limb_los_3d(z, scene.nd, vmrs, z_tans, sza, 40.0)
    layer = L3["seg_alt_layer"]
    rows = torch.as_tensor(layer.astype(np.int64), device="cuda")
    scene.coefficients()                                             # (abs, emi) per gas on the layer rows; haze.thermal: without the sun
    abs_l = torch.stack([haze.thermal[0] if g is haze else g.coeffs[0] for g in scene.gases])
    step_abs = [abs_l[i][rows].contiguous() for i in range(2)]      # the steps' rows: here the layer's (a 1-D atmosphere)
    step_emi = [(haze.thermal if g is haze else g.coeffs)[1][rows].contiguous() for g in scene.gases]
    los = engine.LimbLOS(L3["seg_off"], L3["seg_layer"], L3["pt_off"], L3["x"], L3["nd"], L3["vmr"], col_scale=[ch4.iso_ratio, 1.0])
    rad_dark = engine.limb_rays(list(zip(step_abs, step_emi)), los).clone()
    lo, hi = L3["pt_off"][:-1], L3["pt_off"][1:] - 1
    alt_mid = 0.5 * (L3["alt"][(lo + hi) // 2] + L3["alt"][(lo + hi + 1) // 2])
    U, lit = geometry.solar_columns(z, scene.nd, vmrs, alt_mid, L3["seg_mu"], col_scale=[ch4.iso_ratio, 1.0])
    w = np.where(lit, ALBEDO * geometry.hg_phase(np.cos(np.deg2rad(180.0 - phase)), G) / (4 * np.pi), 0.0)
    sun = torch.as_tensor(irradiance, device="cuda")
    emi_sun, trans = engine.solar_source(abs_l, U, w, haze.thermal[0], sun, src_row=layer, out=step_emi[1].clone(), accumulate=True,
                                         transmission=True)
    rad_lit = engine.limb_rays([(step_abs[0], step_emi[0]), (step_abs[1], emi_sun)], los)
    print("3-D forward, %d steps, %d in shadow; cos SZA along the rays %.3f .. %.3f; solar transmission %.3f .. %.3f"
          % (len(layer), int((~lit).sum()), L3["seg_mu"].min(), L3["seg_mu"].max(), float(trans[torch.as_tensor(lit, device="cuda")].min()), float(trans.max())))
    for r, zt in enumerate(z_tans):
        print("  tangent %5.0f km: mean radiance thermal %.3e, sunlit %.3e" % (zt, float(rad_dark[r].mean()), float(rad_lit[r].mean())))

    # ---- the 1-D scene ------------------------------------------------------------------------------------------------
    pixels = [retrieval.LimbPixel(120.0 + 60.0 * i, fov_half=8.0, pixel_rot=10.0 * (i % 3)) for i in range(8)]
    y = retrieval.radtrans(scene, pixels)
    print("1-D scene (tangent SZA %.0f deg, phase %.0f deg): band radiances of the lowest pixel %s"
          % (sza, phase, np.array2string(y[0].spectrum, precision=3)))

    # ---- twin retrieval ------------------------------------------------------------------------------------------------
    nodes = {"CH4": [140.0, 350.0, 650.0], "haze": [130.0, 300.0, 600.0]}
    apr = {"CH4": np.full(3, 1.3e-4), "haze": 0.5 * np.array([0.7, 0.45, 0.2])}
    truth = {"CH4": np.array([1.7e-4, 1.5e-4, 1.15e-4]), "haze": 0.5 * np.array([1.0, 0.55, 0.14])}

    def bayes(values):
        bs = smm.BayesSet(tag="CH4 VMR + sunlit haze")
        for name in ("CH4", "haze"):
            bs.add_set(smm.LinearProfile_1D_new(name, z, nodes[name], apr[name], 0.5 * apr[name], first_guess_prof=values[name]))
        return bs

    retrieval._state_into_gases(scene, bayes(truth))
    rng = np.random.default_rng(11)
    for pix, yy in zip(pixels, retrieval.radtrans(scene, pixels)):
        sig = 0.004 * np.abs(yy.spectrum).max() * np.ones_like(yy.spectrum)
        pix.observation = retrieval.Spectrum(yy.spectrum + sig * rng.standard_normal(sig.size), scene.bands_nm)
        pix.noise = retrieval.Spectrum(sig, scene.bands_nm)
    chi, _, _, b = retrieval.inversion_state(scene, bayes(apr), pixels, max_it=10)
    x_true = np.concatenate([truth["CH4"], truth["haze"]])
    print("iterations %d (%s), chi square %s" % (len(b.history), b.stop, np.array2string(np.array(b.history), precision=4)))
    print("retrieved ", np.array2string(b.param_vector(), precision=4))
    print("truth     ", np.array2string(x_true, precision=4))
    print("a priori  ", np.array2string(np.concatenate([apr["CH4"], apr["haze"]]), precision=4))


if __name__ == "__main__":
    main()
