#!/usr/bin/env python3
"""Time of the vibrational-temperature Jacobian on one set of the `--config 3 --3d` workload (bench_configs.config3_3d:
2e5 points, 8 rays fanned in azimuth, ~900 LOS steps with a coefficient row each, 12 levels): 7 triangular parameters
for each of 3 excited levels, HIP events, medians of 20 calls after 3 warm-up calls, three times over for the spread.
  (a) LevelFactored.tvib_jacobian's device call (engine.limb_rays_level_jacobian): one launch, 8 x 21 x n_pts written;
  (b) the composition of existing ops for the same 21 parameters: per level glevel_combine on the one-hot
      d pop / d Tvib, limb_rays_jacobians (per-row Jacobian, 8 x n_rows x n_pts), contraction over the rows;
  (c) limb_rays_jacobians for the per-level VMR Jacobian alone: the scale of one recursion pass.
N=<points> (= lines) for a reduced size; prints one JSON line."""
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
lf = engine.LevelFactored(ls, T_rows, P_rows)
co = lf.steps(step_row, tvib=st["tvib"])
alt_step = atm["z"][Lr["seg_alt_layer"]]
nodes = np.linspace(150.0, 800.0, n_nodes)
W = engine.level_node_weights(nodes, alt_step)
par_level = np.repeat(np.array(levels, np.int32), n_nodes)
par_w = np.concatenate([W] * len(levels))
dpop = ls.level_populations_dtvib(T_rows[step_row], st["tvib"])
par_c = np.ascontiguousarray(par_w * dpop.T[par_level])
Wv = bc.layer_vmr_weights(atm["z"], Lr["alt"])
pg = np.zeros(n_layers, np.int32)
w_dev = torch.as_tensor(W, dtype=torch.float64, device="cuda")


def new_call():
    return engine.limb_rays_level_jacobian(co, los, lf.tab, step_row, par_level, par_c, want_rad=False)[1]


def composition():
    out = []
    for lv in levels:
        oh = np.zeros_like(dpop)
        oh[:, lv] = dpop[:, lv]
        dco = engine.glevel_combine(lf.tab, step_row, oh)
        jl = engine.limb_rays_jacobians(co, los, dcoeffs=dco, want_rad=False)[1]
        out.append(torch.einsum("pk,rkn->rpn", w_dev, jl))
    return torch.cat(out, dim=1)


def vmr_pass():
    return engine.limb_rays_jacobians(co, los, par_gas=pg, par_w=Wv, want_rad=False)[2]


def median_ms(fn, n_rep=20, warm=3):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(n_rep):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ts.append(e0.elapsed_time(e1))
    return float(np.median(ts))


ja, jb = new_call(), composition()
s = jb.abs().amax(dim=-1).clamp_min(1e-300)
agree = float(((ja - jb).abs().amax(dim=-1) / s).max())
del ja, jb
res = {}
for name, fn in (("new_call_ms", new_call), ("composition_ms", composition), ("vmr_pass_ms", vmr_pass)):
    res[name] = [round(median_ms(fn), 4) for _ in range(3)]
a, b = np.median(res["new_call_ms"]), np.median(res["composition_ms"])
print(json.dumps(dict(res, n_pts=n, n_rays=n_rays, n_steps=n_steps, table_rows=int(len(T_rows)), n_par=int(len(par_level)),
                      levels=list(levels), ratio_composition_over_new=round(float(b / a), 3),
                      new_vs_composition_row_err=agree,
                      kernel="sr_limb_jac_state_kernel<1, 16, false>: 83 VGPRs, no spills (tools/kernel_resources.sh)",
                      device=engine.device_info()["name"])))
