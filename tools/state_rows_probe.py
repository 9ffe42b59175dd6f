#!/usr/bin/env python3
"""Time of kinetic-temperature parameters in the one-pass state Jacobian on one set of the `--config 3 --3d` workload
(bench_configs.config3_3d: 2e5 points, 8 rays fanned in azimuth, ~900 LOS steps with a coefficient row each, 12 levels;
tools/tvib_jac_probe.py's set): 7 triangular temperature nodes alone, and the 7 together with 7 vibrational-temperature
nodes for each of 3 excited levels (28 parameters).
  (a) ONE call: engine.limb_rays_state_jacobian(dcoeffs=, par_t=) / LevelFactored.state_jacobian
      (sr_limb_rays_jac_state_rows_dev): 8 x 7 (8 x 28) x n_pts written;
  (b) the route that exists without it: limb_rays_jacobians(dcoeffs=) -- the per-row Jacobian, 8 x n_rows x n_pts written
      -- and the contraction with the node masks; for the 28, limb_rays_level_jacobian for the 21 beside it.
HIP events around blocks of calls of at least a second each, the two routes alternated in one process after warm-up;
per route the median over the blocks of the time per call and its run-to-run spread (largest - smallest block).
N=<points> (= lines) for a reduced size, BLOCKS=<blocks per route> (7).  Prints one JSON line."""
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
import bench_configs as bc  # noqa: E402
from spectrobot_amd import engine, synthetic as syn  # noqa: E402

engine.set_device(0)
n = int(os.environ.get("N", "200000"))
n_layers, n_rays, levels, n_nodes = 80, 8, (3, 8, 11), 7
grid, L, atm, e_lev = bc.ch4_case(n, n, n_layers, config_id=3, w0=2950.0)
ls = engine.LineSet(L, grid, 6, 1, syn.CH4_MM, e_lev)
Lr = bc.los_3d_set(atm, np.full(n_layers, 0.0148), 120.0 + 60.0 * np.arange(n_rays), 30.0, 22.5 * np.arange(n_rays))
los = engine.LimbLOS(Lr["seg_off"], Lr["seg_layer"], Lr["pt_off"], Lr["x"], Lr["nd"], Lr["vmr"], col_scale=[syn.CH4_ISO_RATIO])
st = Lr["state"]
T_rows, P_rows, step_row = engine.LevelFactored.unique_rows(st["temps"], st["press"])
n_steps = len(step_row)
lf = engine.LevelFactored(ls, T_rows, P_rows, dT=0.05)
co, dco = lf.steps(step_row, tvib=st["tvib"], derivative=True)
W = engine.level_node_weights(np.linspace(150.0, 800.0, n_nodes), atm["z"][Lr["seg_alt_layer"]])     # [7, n_steps]
par_level = np.repeat(np.array(levels, np.int32), n_nodes)
par_w = np.concatenate([W] * len(levels))
par_c = np.ascontiguousarray(par_w * ls.level_populations_dtvib(T_rows[step_row], st["tvib"]).T[par_level])
w_dev = torch.as_tensor(W, dtype=torch.float64, device="cuda")
none = np.zeros(0, np.int32)


def temp_one_call():
    return engine.limb_rays_state_jacobian(co, los, dcoeffs=dco, par_t=W, want_rad=False)[1]


def temp_composition():
    return torch.einsum("pk,rkn->rpn", w_dev, engine.limb_rays_jacobians(co, los, dcoeffs=dco, want_rad=False)[1])


def both_one_call():
    return lf.state_jacobian(co, los, step_row, st["tvib"], par_level, par_w, dcoeffs=dco, par_w_temp=W, want_rad=False)[1]


def both_composition():
    jl = engine.limb_rays_level_jacobian(co, los, lf.tab, step_row, par_level, par_c, want_rad=False)[1]
    return torch.cat([jl, temp_composition()], dim=1)


def block_ms(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / reps


routes = (("temp_composition", temp_composition), ("temp_one_call", temp_one_call),
          ("both_composition", both_composition), ("both_one_call", both_one_call))
s = lambda ref: ref.abs().amax(dim=-1).clamp_min(1e-300)
ja, jb = temp_one_call(), temp_composition()
agree_t = float(((ja - jb).abs().amax(dim=-1) / s(jb)).max())
ja, jb = both_one_call(), both_composition()
agree_b = float(((ja - jb).abs().amax(dim=-1) / s(jb)).max())
del ja, jb
for _, fn in routes:                              # warm-up of every shape
    block_ms(fn, 3)
reps = {name: max(3, int(np.ceil(1000.0 / block_ms(fn, 3)))) for name, fn in routes}
res = {name: [] for name, _ in routes}
for _ in range(int(os.environ.get("BLOCKS", "7"))):
    for name, fn in routes:
        res[name].append(round(block_ms(fn, reps[name]), 4))
med = {k: float(np.median(v)) for k, v in res.items()}
spread = {k: round(max(v) - min(v), 4) for k, v in res.items()}
print(json.dumps(dict(blocks_ms=res, median_ms={k: round(v, 4) for k, v in med.items()}, spread_ms=spread, calls_per_block=reps,
                      ratio_temp_composition_over_one_call=round(med["temp_composition"] / med["temp_one_call"], 3),
                      ratio_both_composition_over_one_call=round(med["both_composition"] / med["both_one_call"], 3),
                      temp_margin_in_spreads=round((med["temp_composition"] - med["temp_one_call"])
                                                   / max(spread["temp_composition"], spread["temp_one_call"], 1e-9), 1),
                      both_margin_in_spreads=round((med["both_composition"] - med["both_one_call"])
                                                   / max(spread["both_composition"], spread["both_one_call"], 1e-9), 1),
                      n_pts=n, n_rays=n_rays, n_steps=n_steps, table_rows=int(len(T_rows)), n_temp=n_nodes,
                      n_tvib=int(len(par_level)), one_call_vs_composition_row_err=dict(temp=agree_t, both=agree_b),
                      device=engine.device_info()["name"])))
