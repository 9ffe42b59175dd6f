#!/usr/bin/env python3
"""Twin experiment on a latitude-box profile: the VMR of an LTE trace gas (HCN-like) on 3 latitude boxes x 5 altitude nodes
(smm.LinearProfile_2D), retrieved by retrieval.inversion_boxes from limb pixels whose lines of sight head north across a
box boundary -- the counterpart of the reference's inversion(..., g3D=True).  Temperature, pressure and the coefficient
tables are 1-D; only the composition varies with latitude.  One engine.limb_rays_state_bands call per iteration for all
lines of sight and all 15 parameters, with the parameter blocks per ray (ray_blocks=True): a ray crosses two of the boxes
and sees the nodes above its tangent altitude.

  truth      the a-priori profile scaled by 1.3, 0.8 and 1.2 in the three boxes
  "observed" the band spectra of 6 limb pixels (three lines of sight each, closed-form field of view) through the truth,
             plus noise
  retrieved  15 VMR nodes, Levenberg-Marquardt optimal estimation

Prints the chi-square history, the walks of both plans and the retrieved profiles next to the truth.  Needs an MI355X:
python examples/retrieve_lat_boxes.py
"""
import os
import sys
import types

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from spectrobot_amd import engine, retrieval, synthetic as syn          # noqa: E402
from spectrobot_amd import spect_main_module as smm                     # noqa: E402

HCN_MM, HCN_ISO_RATIO = 27.010899, 0.985114
HCN_LEVEL_ENERGIES = np.array([0., 711.98, 1411.41, 2096.85, 3311.48, 4004.17])


def build(n_grid=40000, n_layers=40, n_lines=(1200, 4000), n_box=3, n_nodes=5, n_pix=6, n_bands=10):
    """The scene (HCN-like gas with the box profile, CH4 as a fixed background), the pixels, a function bayes(scale) that
    makes the BayesSet with the a-priori profile scaled per box, and the truth's scales."""
    grid = syn.make_grid(2990.0, 5e-4, n_grid)
    atm = syn.make_atmosphere(n_layers, 12)
    z = atm["z"]
    span = z[-1] - z[0]
    Lh = syn.make_lines(n_lines[0], grid, config_id=5, n_levels=6)
    Lh["a_coeff"] = Lh["a_coeff"] * 30.0
    ch4 = retrieval.Gas("CH4", engine.LineSet(syn.make_lines(n_lines[1], grid, config_id=3, n_levels=12), grid, 6, 1, syn.CH4_MM,
                                              syn.CH4_LEVEL_ENERGIES), np.full(n_layers, 0.0148), syn.CH4_ISO_RATIO)
    hcn = retrieval.Gas("HCN", engine.LineSet(Lh, grid, 23, 1, HCN_MM, HCN_LEVEL_ENERGIES), np.full(n_layers, 2e-6), HCN_ISO_RATIO)
    lam_lo, lam_hi = 1e7 / grid[-1], 1e7 / grid[0]
    margin = min(1.0, 0.1 * (lam_hi - lam_lo))
    bands = np.linspace(lam_lo + margin, lam_hi - margin, n_bands)
    scene = retrieval.LimbScene(grid, z, atm["temps"], atm["press"], [hcn, ch4], bands, np.full(n_bands, min(1.1, 0.1 * (lam_hi - lam_lo))))
    # the boxes START at lat_limits: south of the equator, then n_box - 2 boxes up to 36 N, then the rest; tangent points
    # in turn at some 10 S, 9 N and 26 N (every box holds tangent points at several altitudes), the rays head north.  smm.LinearProfile_2D, as the reference's, gives the LAST start no mask of its
    # own, so the closing limit 90 N is listed as one more start: its n_nodes parameters weight nothing, touch no ray
    # (the reference's not_involved) and stay at their a priori.
    lat_limits = [-90.0] + list(36.0 / (n_box - 1) * np.arange(n_box - 1)) + [90.0]
    pixels = [retrieval.BoxPixel(z[0] + (0.08 + 0.8 * i / n_pix) * span, tangent_lat_deg=(-10.0, 9.0, 26.0)[i % 3] + 0.5 * i,
                                 heading_deg=0.0, fov_half=0.015 * span, pixel_rot=10.0 * (i % 3)) for i in range(n_pix)]
    nodes = [z[0] + f * span for f in np.linspace(0.08, 0.9, n_nodes)]
    atmosphere = types.SimpleNamespace(grid=types.SimpleNamespace(coords={"alt": z}))
    apr, sig = np.full(n_nodes, 2e-6), np.full(n_nodes, 1e-6)

    def bayes(scale=None):
        scale = np.ones(n_box) if scale is None else np.asarray(scale, float)
        bs = smm.BayesSet(tag="HCN on %d latitude boxes x %d altitude nodes" % (n_box, n_nodes))
        st = smm.LinearProfile_2D("HCN", atmosphere, nodes, lat_limits, [apr] * (n_box + 1), [sig] * (n_box + 1))
        for j in range(n_box):                     # (the class does not pass a first guess on: set the values)
            for p in st.set[j * n_nodes:(j + 1) * n_nodes]:
                p.value = p.apriori * scale[j]
        bs.add_set(st)
        return bs

    true_scale = np.resize([1.3, 0.8, 1.2], n_box)
    return scene, pixels, bayes, true_scale


def observe(scene, pixels, truth, noise_frac, rng=None):
    """The truth's band spectra as observations (rng: with noise)."""
    for pix, y in zip(pixels, retrieval.simulate_boxes(scene, truth, pixels)):
        sig = np.full(y.size, noise_frac * np.abs(y).max())
        pix.observation = retrieval.Spectrum(y + (sig * rng.standard_normal(sig.size) if rng is not None else 0.0), scene.bands_nm)
        pix.noise = retrieval.Spectrum(sig, scene.bands_nm)


def main():
    engine.set_device(0)
    scene, pixels, bayes, true_scale = build()
    truth = bayes(true_scale)
    observe(scene, pixels, truth, 2e-4, np.random.default_rng(7))
    chi, _, _, bs = retrieval.inversion_boxes(scene, bayes(), pixels, max_it=10)
    route, walks = engine.last_state_route()
    x, x_true = bs.param_vector(), truth.param_vector()
    sigma = np.array([p.apriori_err for p in bs.params()])
    for it, c in enumerate(bs.history):
        print("iteration %d: chi square %.3f" % (it, c))
    print("stopped: %s; plan %s, %d walks of %d rays (the dense plan: %d)"
          % (bs.stop, {1: "dense", 2: "per ray"}[route], walks, 3 * len(pixels), 3 * len(pixels) * -(-len(x) // 16)))
    print("parameters touched per pixel:", bs.touches.sum(axis=1).tolist())
    n_nodes = len(x) // (len(true_scale) + 1)
    for j in range(len(true_scale)):
        s = slice(j * n_nodes, (j + 1) * n_nodes)
        print("box %d  retrieved %s  truth %s" % (j, np.array2string(x[s], precision=3), np.array2string(x_true[s], precision=3)))
    print("state error in a-priori sigmas: %.2f before, %.2f after"
          % (np.linalg.norm((bayes().param_vector() - x_true) / sigma), np.linalg.norm((x - x_true) / sigma)))
    assert bs.history[-1] < bs.history[0], "chi square did not fall"


if __name__ == "__main__":
    main()
