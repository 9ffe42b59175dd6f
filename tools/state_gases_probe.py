#!/usr/bin/env python3
"""What one state pass for the vibrational temperatures of TWO level-factored gases saves: one iteration's Jacobian on the
scene of tools/state_bands_probe.py -- shaped like BASELINE configs[4]: 18 pixels x 3 lines of sight, 1e5 points -- with
BOTH gases on the level-factored route (an HCN-like gas with 6 levels, CH4 with 12) and 7 VMR nodes (4 CH4 + 3 HCN) +
10 Tvib nodes of CH4 (5 for each of two levels) + 6 Tvib nodes of HCN (3 for each of two levels), timed on both routes:
  spectra: per_gas = one LevelFactored.state_jacobian per level gas, the only route without the new call (the first call
           carries the VMR nodes, each call walks every ray and writes the radiances again);
           one_call = LevelFactoredSet.state_jacobian (sr_limb_rays_jac_state_gases_dev);
  bands:   per_gas = one LevelFactored.state_bands per level gas (14 bands, field of view), the rows joined in numpy;
           one_call = LevelFactoredSet.state_bands (sr_limb_rays_state_bands_gases_dev).
HIP events around blocks of calls (about half a second each), the two routes alternated A B A B ... in one process after a
warm-up of every shape; per route the median over the blocks of the time per call and the run-to-run spread (largest -
smallest block).  N=<points>, LAYERS=<layers>, BLOCKS=<blocks per route> (7) for other sizes.  RAY_BLOCKS=1: every call
with the parameter blocks per ray (engine.set_state_ray_blocks; the JSON lines say so and carry the walks of the last
call).  Prints one JSON line per case and a last line with the medians."""
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
import bench_configs as bc  # noqa: E402
from spectrobot_amd import engine, synthetic as syn  # noqa: E402

engine.set_device(0)
ray_blocks = os.environ.get("RAY_BLOCKS", "0") not in ("", "0")
engine.set_state_ray_blocks(ray_blocks)
n = int(os.environ.get("N", "100000"))
n_layers = int(os.environ.get("LAYERS", "55"))
n_blocks = int(os.environ.get("BLOCKS", "7"))
n_pix = 18
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
lf_c = engine.LevelFactored(ls_c, temps, press)
lf_h = engine.LevelFactored(ls_h, temps, press)
tv_c = atm["tvib"]
tv_h = np.tile(temps, (6, 1)) + np.linspace(0.0, 10.0, 6)[:, None]
coeffs = engine.gas_stack([lf_h.steps(step_row, tvib=tv_h), lf_c.steps(step_row, tvib=tv_c)])      # HCN is gas 0, CH4 gas 1
vmr = [np.full(n_layers, 2e-6), np.full(n_layers, 1.48e-4)]
tang = [z[0] + (0.06 + 0.045 * i) * span + d * 0.02 * span for i in range(n_pix) for d in (-1.0, 0.0, 1.0)]
Lr = syn.limb_los(z, syn.number_density(press, temps), vmr, tang)
los = engine.LimbLOS(Lr["seg_off"], Lr["seg_layer"], Lr["pt_off"], Lr["x"], Lr["nd"], Lr["vmr"],
                     col_scale=[bc.HCN_ISO_RATIO, syn.CH4_ISO_RATIO])
fov_fac = engine.fov_factors([10.0 * (i % 3) for i in range(n_pix)])
nodes = lambda fr: [z[0] + f * span for f in fr]
par_w_col = np.concatenate([engine.level_node_weights(nodes((0.06, 0.3, 0.55, 0.85)), Lr["alt"]),
                            engine.level_node_weights(nodes((0.1, 0.45, 0.8)), Lr["alt"])])
par_gas = np.array([1, 1, 1, 1, 0, 0, 0], np.int32)
W5 = engine.level_node_weights(nodes((0.1, 0.3, 0.5, 0.7, 0.9)), z)
W3 = engine.level_node_weights(nodes((0.15, 0.5, 0.85)), z)
lev_c, w_c = np.repeat(np.array([5, 2], np.int32), 5), np.concatenate([W5, W5])                    # 10 Tvib nodes of CH4
lev_h, w_h = np.repeat(np.array([1, 4], np.int32), 3), np.concatenate([W3, W3])                    # 6 of HCN
both = engine.LevelFactoredSet([(lf_c, 1, step_row, tv_c), (lf_h, 0, step_row, tv_h)])
par_lgas = np.concatenate([np.zeros(10, np.int32), np.ones(6, np.int32)])
par_level, par_w_lev = np.concatenate([lev_c, lev_h]), np.concatenate([w_c, w_h])
lam_lo, lam_hi = 1e7 / grid[-1], 1e7 / grid[0]
margin = min(1.2, 0.1 * (lam_hi - lam_lo))
bands = (np.linspace(lam_lo + margin, lam_hi - margin, 14), np.full(14, min(1.1, 0.1 * (lam_hi - lam_lo))))


def spectra_per_gas():
    rad, j_c = lf_c.state_jacobian(coeffs, los, step_row, tv_c, lev_c, w_c, par_gas=par_gas, par_w_col=par_w_col, gas=1)
    _, j_h = lf_h.state_jacobian(coeffs, los, step_row, tv_h, lev_h, w_h, gas=0)
    return rad, j_c, j_h


def spectra_one_call():
    return both.state_jacobian(coeffs, los, par_lgas, par_level, par_w_lev, par_gas=par_gas, par_w_col=par_w_col)


def bands_per_gas():
    b_c = lf_c.state_bands(coeffs, los, step_row, tv_c, lev_c, w_c, grid, bands[0], bands[1], par_gas=par_gas, par_w_col=par_w_col,
                           gas=1, fov=fov_fac)
    b_h = lf_h.state_bands(coeffs, los, step_row, tv_h, lev_h, w_h, grid, bands[0], bands[1], gas=0, fov=fov_fac)
    return np.concatenate([b_c, b_h[:, 1:]], axis=1)


def bands_one_call():
    return both.state_bands(coeffs, los, par_lgas, par_level, par_w_lev, grid, bands[0], bands[1], par_gas=par_gas,
                            par_w_col=par_w_col, fov=fov_fac)


def block_ms(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / reps


def row_err(a, ref):
    s = ref.abs().amax(dim=-1).clamp_min(1e-300)
    return float(((a - ref).abs().amax(dim=-1) / s).max())


rad_p, j_c, j_h = spectra_per_gas()
rad_o, j_o = spectra_one_call()
agree = dict(spectra=max(row_err(j_o[:, :17], j_c), row_err(j_o[:, 17:], j_h[:, 0:]), row_err(rad_o, rad_p)))
del rad_p, j_c, j_h, rad_o, j_o
u, f = bands_per_gas(), bands_one_call()
scale = np.max(np.abs(u), axis=(0, 2), keepdims=True)
agree["bands"] = float(np.max(np.abs(f - u) / np.where(scale > 0, scale, 1.0)))
summary = {}
for case, routes in (("spectra", (("per_gas", spectra_per_gas), ("one_call", spectra_one_call))),
                     ("bands_14", (("per_gas", bands_per_gas), ("one_call", bands_one_call)))):
    for _, fn in routes:                              # warm-up of every shape
        block_ms(fn, 3)
    reps = {name: max(3, int(np.ceil(500.0 / block_ms(fn, 3)))) for name, fn in routes}
    res = {name: [] for name, _ in routes}
    for _ in range(n_blocks):                         # A B A B ...
        for name, fn in routes:
            res[name].append(round(block_ms(fn, reps[name]), 4))
    med = {k: float(np.median(v)) for k, v in res.items()}
    spread = {k: round(max(v) - min(v), 4) for k, v in res.items()}
    summary[case] = dict(per_gas_ms=round(med["per_gas"], 4), one_call_ms=round(med["one_call"], 4),
                         per_gas_over_one_call=round(med["per_gas"] / med["one_call"], 3))
    print(json.dumps(dict(case=case, n_pts=n, n_layers=n_layers, n_rays=los.n_rays, n_col=7, n_lev=[10, 6], blocks_ms=res,
                          median_ms={k: round(v, 4) for k, v in med.items()}, spread_ms=spread, calls_per_block=reps,
                          per_gas_over_one_call=round(med["per_gas"] / med["one_call"], 3),
                          margin_in_spreads=round((med["per_gas"] - med["one_call"]) / max(spread["per_gas"], spread["one_call"], 1e-9), 1),
                          one_call_vs_per_gas_row_err=agree["spectra" if case == "spectra" else "bands"],
                          ray_blocks=ray_blocks, last_state_route=engine.last_state_route(),
                          device=engine.device_info()["name"])), flush=True)
print(json.dumps(dict(summary=summary)))
