#!/usr/bin/env python3
"""Time of the mixed-state Jacobian on BASELINE configs[4]'s LOS batch with a non-LTE CH4: HCN + CH4 on the benchmark's
scene (bench_configs.two_gas_scene(40000, 8000, 60000, 60): 60000-point grid, 60 layers), 6 pixels x 3 lines of sight =
18 rays, 7 VMR nodes (4 CH4 + 3 HCN, bench_configs.retrieval_problem's) + 9 Tvib nodes (5 of CH4 level 5, 4 of level 2)
= 16 parameters.
  (a) ONE call: LevelFactored.state_jacobian (sr_limb_rays_jac_state_dev);
  (b) the pair that gives the same K without it: engine.limb_rays_jacobian + LevelFactored.tvib_jacobian.
HIP events around blocks of calls of at least a second each, the two routes alternated in one process after warm-up;
per route the median over the blocks of the time per call, and the pair's run-to-run spread (largest - smallest block).
N=<points>, LAYERS=<layers> for a reduced size; TRACE=1: a few calls of each route only (for rocprofv3 --kernel-trace).
Prints one JSON line."""
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
import bench_configs as bc  # noqa: E402
from spectrobot_amd import engine, retrieval, synthetic as syn  # noqa: E402

engine.set_device(0)
n = int(os.environ.get("N", "60000"))
n_layers = int(os.environ.get("LAYERS", "60"))
trace = os.environ.get("TRACE", "0") == "1"
scene = bc.two_gas_scene(40000 * n // 60000, 8000 * n // 60000, n, n_layers)
old = scene.gas("CH4")
ch4 = retrieval.LevelGas("CH4", old.lineset, old.vmr, old.tvib, old.iso_ratio)
hcn = scene.gas("HCN")
hcn.tvib = None                                  # the LTE trace gas
scene.gases = [ch4, hcn]
bs, pixels, _ = bc.retrieval_problem(scene)      # 4 + 3 VMR nodes, 6 pixels with a field of view
z = scene.z
span = z[-1] - z[0]
bs.add_set(retrieval.TvibProfile("CH4", 5, z, [z[0] + f * span for f in (0.1, 0.3, 0.5, 0.7, 0.9)], np.full(5, 4.0)))
bs.add_set(retrieval.TvibProfile("CH4", 2, z, [z[0] + f * span for f in (0.15, 0.4, 0.65, 0.9)], np.full(4, 4.0)))
retrieval._state_into_gases(scene, bs)
alts = [a for pix in sorted(pixels, key=lambda p: p.limb_tg_alt) for a in pix.los_alts()]
coeffs = scene.coefficient_stack()
los, alt = scene.los(alts)
w = scene.state_weights(bs, alt)
lf, rows, tvib = ch4.lf, ch4.rows, ch4.tvib
assert los.n_rays == 18 and len(w.par_gas) == 7 and len(w.par_level) == 9


def one_call():
    return lf.state_jacobian(coeffs, los, rows, tvib, w.par_level, w.par_w_lev, par_gas=w.par_gas, par_w_col=w.par_w_col, gas=w.gas)


def pair():
    rad, jc = engine.limb_rays_jacobian(coeffs, los, w.par_gas, w.par_w_col)
    _, jl = lf.tvib_jacobian(coeffs, los, rows, tvib, w.par_level, w.par_w_lev, gas=w.gas, want_rad=False)
    return rad, jc, jl


def block_ms(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / reps


(ra, ja), (rb, jc, jl) = one_call(), pair()
s = lambda ref: ref.abs().amax(dim=-1).clamp_min(1e-300)
agree_c = float(((ja[:, :7] - jc).abs().amax(dim=-1) / s(jc)).max())
agree_l = float(((ja[:, 7:] - jl).abs().amax(dim=-1) / s(jl)).max())
del ra, ja, rb, jc, jl
if trace:
    for _ in range(5):
        one_call()
        pair()
    torch.cuda.synchronize()
    print(json.dumps(dict(trace=True, n_pts=n, n_layers=n_layers)))
    sys.exit(0)
for fn in (one_call, pair):                       # warm-up of every shape
    block_ms(fn, 5)
reps = {name: max(3, int(np.ceil(1000.0 / block_ms(fn, 5)))) for name, fn in (("one_call", one_call), ("pair", pair))}
res = {"one_call": [], "pair": []}
for _ in range(int(os.environ.get("BLOCKS", "7"))):
    for name, fn in (("pair", pair), ("one_call", one_call)):
        res[name].append(round(block_ms(fn, reps[name]), 4))
a, b = float(np.median(res["one_call"])), float(np.median(res["pair"]))
print(json.dumps(dict(one_call_ms=res["one_call"], pair_ms=res["pair"], one_call_median_ms=round(a, 4), pair_median_ms=round(b, 4),
                      pair_spread_ms=round(max(res["pair"]) - min(res["pair"]), 4),
                      one_call_spread_ms=round(max(res["one_call"]) - min(res["one_call"]), 4),
                      ratio_pair_over_one_call=round(b / a, 3), calls_per_block=reps, n_pts=n, n_layers=n_layers, n_rays=los.n_rays,
                      n_col=7, n_lev=9, column_rows_vs_pair=agree_c, level_rows_vs_pair=agree_l,
                      device=engine.device_info()["name"])))
