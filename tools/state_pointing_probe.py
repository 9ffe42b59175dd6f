#!/usr/bin/env python3
"""What the pointing row (d / d tangent altitude of every ray) costs in the fused state call, on the shapes of
tools/state_bands_probe.py -- 18 pixels x 3 lines of sight, 1e5 points, HCN + non-LTE CH4 on the level-factored route, 7 VMR
nodes + 10 Tvib nodes, 14 bands -- and what it replaces:
  fused_pointing: LevelFactored.state_bands(pointing=True) (sr_limb_rays_state_bands_path_dev): one call, n_gas hidden
                  column slots whose rows are added on the host, no hi-res spectrum;
  fused:          the same call without the row (sr_limb_rays_state_bands_dev): the parent's call;
  two_forward:    the two forward models of a central difference in the offset: the LOS batch rebuilt at z_t + h and at
                  z_t - h (geometry.limb_los from scratch, as a new offset makes it every iteration, + engine.LimbLOS),
                  engine.limb_rays, engine.hires_to_lowres, smm.fov_closed_form; geometry_ms is the host part of it alone.
HIP events around blocks of calls (about half a second each; every call ends in a stream synchronise), the routes
alternated A B C A B C ... in one process after a warm-up of every shape; per route the median over the blocks of the time
per call and the run-to-run spread (largest - smallest block).  N=<points>, LAYERS=<layers>, BLOCKS=<blocks per route> (7).
Prints one JSON line."""
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
import bench_configs as bc  # noqa: E402
from spectrobot_amd import engine, geometry, synthetic as syn, spect_main_module as smm  # noqa: E402

engine.set_device(0)
n = int(os.environ.get("N", "100000"))
n_layers = int(os.environ.get("LAYERS", "55"))
n_blocks = int(os.environ.get("BLOCKS", "7"))
n_pix = 18
H_KM = 1e-3
grid = syn.make_grid(3290.0, 5e-4, n)
atm = syn.make_atmosphere(n_layers, 12)
z, temps, press = atm["z"], atm["temps"], atm["press"]
span = z[-1] - z[0]
Lc = syn.make_lines(max(n // 8, 200), grid, config_id=4, n_levels=12)
Lh = syn.make_lines(max(n // 40, 50), grid, config_id=5, n_levels=6)
Lh["a_coeff"] = Lh["a_coeff"] * 30.0
ls_c = engine.LineSet(Lc, grid, 6, 1, syn.CH4_MM, syn.CH4_LEVEL_ENERGIES)
ls_h = engine.LineSet(Lh, grid, 23, 1, bc.HCN_MM, bc.HCN_LEVEL_ENERGIES)
step_row = np.arange(n_layers, dtype=np.int32)
lf = engine.LevelFactored(ls_c, temps, press)
co_c = lf.steps(step_row, tvib=atm["tvib"])
co_h = ls_h.abscoeff_layers(temps, press)
coeffs = engine.gas_stack([co_h, co_c])      # CH4 is gas 1
GAS = 1
vmr = [np.full(n_layers, 2e-6), np.full(n_layers, 1.48e-4)]
nd = syn.number_density(press, temps)
tang = np.array([z[0] + (0.06 + 0.045 * i) * span + d * 0.02 * span for i in range(n_pix) for d in (-1.0, 0.0, 1.0)])
scale = [bc.HCN_ISO_RATIO, syn.CH4_ISO_RATIO]


def batch(z_tans, path):
    geometry._LOS_GEOMETRY.clear()           # a new offset is a new geometry: nothing cached
    geometry._LOS_PATH.clear()
    L = geometry.limb_los(z, nd, vmr, z_tans, path=path)
    return engine.LimbLOS(L["seg_off"], L["seg_layer"], L["pt_off"], L["x"], L["nd"], L["vmr"], col_scale=scale,
                          path=dict(alt=L["alt"], dx=L["dx_dzt"], dalt=L["dalt_dzt"]) if path else None), L


los, Lr = batch(tang, True)
rots = [10.0 * (i % 3) for i in range(n_pix)]
fov_fac = engine.fov_factors(rots)
nodes = lambda fr: [z[0] + f * span for f in fr]
par_w_col = np.concatenate([engine.level_node_weights(nodes((0.06, 0.3, 0.55, 0.85)), Lr["alt"]),
                            engine.level_node_weights(nodes((0.1, 0.45, 0.8)), Lr["alt"])])
par_gas = np.array([1, 1, 1, 1, 0, 0, 0], np.int32)
W5 = engine.level_node_weights(nodes((0.1, 0.3, 0.5, 0.7, 0.9)), z)
par_level, par_w_lev = np.repeat(np.array([5, 2], np.int32), 5), np.concatenate([W5, W5])
lam_lo, lam_hi = 1e7 / grid[-1], 1e7 / grid[0]
margin = min(1.2, 0.1 * (lam_hi - lam_lo))
bands = (np.linspace(lam_lo + margin, lam_hi - margin, 14), np.full(14, min(1.1, 0.1 * (lam_hi - lam_lo))))


def fused(pointing=False):
    return lf.state_bands(coeffs, los, step_row, atm["tvib"], par_level, par_w_lev, grid, bands[0], bands[1], fov=fov_fac,
                          pointing=pointing, par_gas=par_gas, par_w_col=par_w_col, gas=GAS)


def forward(z_tans):
    b, _ = batch(z_tans, False)
    low = engine.hires_to_lowres(engine.limb_rays(coeffs, b, resident=False), grid, bands[0], bands[1])
    return smm.fov_closed_form(low[0::3], low[1::3], low[2::3], rots)


def two_forward():
    return (forward(tang + H_KM) - forward(tang - H_KM)) / (2.0 * H_KM)


def block_ms(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / reps


routes = (("fused_pointing", lambda: fused(True)), ("fused", fused), ("two_forward", two_forward))
f, p, d = fused(True), fused(), two_forward()
assert np.array_equal(f[:, :p.shape[1]], p)           # the parent's rows, bit for bit
row = f[:, p.shape[1]]
agree = float(np.abs(row - d).max() / np.abs(row).max())
for _, fn in routes:                                  # warm-up of every shape
    block_ms(fn, 3)
reps = {name: max(3, int(np.ceil(500.0 / block_ms(fn, 3)))) for name, fn in routes}
res = {name: [] for name, _ in routes}
for _ in range(n_blocks):                             # A B C A B C ...
    for name, fn in routes:
        res[name].append(round(block_ms(fn, reps[name]), 4))
t0 = time.perf_counter()
for _ in range(5):
    batch(tang + H_KM, False)
    batch(tang - H_KM, False)
geometry_ms = (time.perf_counter() - t0) / 5 * 1e3
med = {k: float(np.median(v)) for k, v in res.items()}
spread = {k: round(max(v) - min(v), 4) for k, v in res.items()}
extra = med["fused_pointing"] - med["fused"]
print(json.dumps(dict(n_pts=n, n_layers=n_layers, n_rays=los.n_rays, n_par=p.shape[1] - 1, n_bands=int(bands[0].size), blocks_ms=res,
                      median_ms={k: round(v, 4) for k, v in med.items()}, spread_ms=spread, calls_per_block=reps,
                      pointing_row_ms=round(extra, 4), pointing_row_percent_of_fused=round(100.0 * extra / med["fused"], 2),
                      pointing_row_in_spreads=round(extra / max(spread["fused_pointing"], spread["fused"], 1e-9), 1),
                      two_forward_over_pointing_row=round(med["two_forward"] / max(extra, 1e-9), 2),
                      two_forward_geometry_ms=round(geometry_ms, 4), row_vs_central_difference=agree,
                      device=engine.device_info()["name"])), flush=True)
