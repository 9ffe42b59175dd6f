#!/usr/bin/env python3
"""Time of the radiance budget on one set of the `--config 3 --3d` workload (bench_configs.config3_3d: 2e5 points, 8 rays
fanned in azimuth, ~900 LOS steps with a coefficient row each, 12 levels: the set of tools/tvib_jac_probe.py): the
radiance every level emits plus the gas part, HIP events, medians of 20 calls after 3 warm-up calls, three times over for
the spread, the candidates alternating in one process.
  (a) engine.limb_rays_parts: one launch, 8 x 14 x n_pts written;
  (b) the composition of existing ops for the same 13 parts: per level glevel_combine on the one-hot populations (the
      level's emission rows) and limb_rays with the total absorption; the gas part by limb_rays on the gas's emission;
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
n_layers, n_rays, n_lev = 80, 8, 12
grid, L, atm, e_lev = bc.ch4_case(n, n, n_layers, config_id=3, w0=2950.0)
ls = engine.LineSet(L, grid, 6, 1, syn.CH4_MM, e_lev)
Lr = bc.los_3d_set(atm, np.full(n_layers, 0.0148), 120.0 + 60.0 * np.arange(n_rays), 30.0, 22.5 * np.arange(n_rays))
los = engine.LimbLOS(Lr["seg_off"], Lr["seg_layer"], Lr["pt_off"], Lr["x"], Lr["nd"], Lr["vmr"], col_scale=[syn.CH4_ISO_RATIO])
st = Lr["state"]
T_rows, P_rows, step_row = engine.LevelFactored.unique_rows(st["temps"], st["press"])
n_steps = len(step_row)
lf = engine.LevelFactored(ls, T_rows, P_rows)
co = lf.steps(step_row, tvib=st["tvib"])
pop = ls.level_populations(T_rows[step_row], tvib=st["tvib"])          # [n_steps, n_levels]
part_gas = np.zeros(n_lev + 1, np.int32)
part_level = np.array(list(range(n_lev)) + [-1], np.int32)
part_c = np.ascontiguousarray(np.concatenate([pop.T, np.zeros((1, n_steps))]))
Wv = bc.layer_vmr_weights(atm["z"], Lr["alt"])
pg = np.zeros(n_layers, np.int32)
zero_e = torch.zeros_like(co[1])


def new_call():
    return engine.limb_rays_parts(co, los, part_gas, part_level, part_c=part_c, tab=lf.tab, coef_row=step_row, want_rad=False)[1]


def composition():
    out = []
    for lv in range(n_lev):
        oh = np.zeros_like(pop)
        oh[:, lv] = pop[:, lv]
        out.append(engine.limb_rays((co[0], engine.glevel_combine(lf.tab, step_row, oh)[1]), los))
    out.append(engine.limb_rays(co, los))                              # the gas part: one gas, no background
    out.append(engine.limb_rays((co[0], zero_e), los))                 # the background (zero: no initial intensity)
    return torch.stack(out, dim=1)


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


pa, pb = new_call(), composition()
s = pb.abs().amax(dim=-1)
s = s.masked_fill(s == 0, 1.0)
agree = float(((pa - pb).abs().amax(dim=-1) / s).max())
del pa, pb
res = {"new_call_ms": [], "composition_ms": [], "vmr_pass_ms": []}
for _ in range(3):
    for name, fn in (("new_call_ms", new_call), ("composition_ms", composition), ("vmr_pass_ms", vmr_pass)):
        res[name].append(round(median_ms(fn), 4))
a, b = np.median(res["new_call_ms"]), np.median(res["composition_ms"])
print(json.dumps(dict(res, n_pts=n, n_rays=n_rays, n_steps=n_steps, table_rows=int(len(T_rows)), n_part=int(len(part_level)),
                      ratio_composition_over_new=round(float(b / a), 3), new_vs_composition_row_err=agree,
                      kernel="sr_limb_parts_kernel<1, 16>: 149 VGPRs, no scratch, no vector-register spills, 4 scalars parked in vector lanes "
                             "(hipcc -Rpass-analysis=kernel-resource-usage)", device=engine.device_info()["name"])))
