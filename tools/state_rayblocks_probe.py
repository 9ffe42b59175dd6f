#!/usr/bin/env python3
"""What the parameter blocks per ray save on a latitude-box state: the scene of examples/retrieve_lat_boxes.py scaled to 7
boxes x 10 altitude nodes (80 parameters with the closing limit's ten, which touch nothing), 18 pixels x 3 lines of sight
and 1e5 points, one iteration's engine.limb_rays_state_bands call (14 bands, field of view) timed on both plans:
  dense    the parameter list of the batch in blocks of 16: every ray is walked once per block;
  per_ray  ray_blocks=True: every ray is walked once per block of the parameters that touch it.
HIP events around blocks of calls (about half a second each), the two plans alternated A B A B ... in one process after a
warm-up; per plan the median over the blocks of the time per call and the run-to-run spread (largest - smallest block).
The walks of both plans come from the library (engine.last_state_route).  N=<points>, BLOCKS=<blocks per plan> (7) for other
sizes.  Prints one JSON line; OUT=<file> writes it there too (profiles/state_rayblocks_probe.json)."""
import importlib.util
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
from spectrobot_amd import engine, retrieval  # noqa: E402

spec = importlib.util.spec_from_file_location("retrieve_lat_boxes", os.path.join(ROOT, "examples", "retrieve_lat_boxes.py"))
example = importlib.util.module_from_spec(spec)
spec.loader.exec_module(example)

engine.set_device(0)
n = int(os.environ.get("N", "100000"))
n_blocks = int(os.environ.get("BLOCKS", "7"))
n_box, n_nodes, n_pix = 7, 10, 18
scene, pixels, bayes, true_scale = example.build(n_grid=n, n_layers=55, n_lines=(max(n // 40, 50), max(n // 8, 200)), n_box=n_box,
                                                 n_nodes=n_nodes, n_pix=n_pix, n_bands=14)
bs = bayes(true_scale)
B = retrieval.box_batch(scene, bs, pixels)
L3 = B.L3
los = engine.LimbLOS(L3["seg_off"], L3["seg_layer"], L3["pt_off"], L3["x"], L3["nd"], B.vmr(scene, bs),
                     col_scale=[g.iso_ratio for g in scene.gases])
coeffs = scene.coefficient_stack()
fov = engine.fov_factors([pix.pixel_rot for pix in pixels])


def call(ray_blocks):
    return engine.limb_rays_state_bands(coeffs, los, scene.grid, scene.bands_nm, scene.widths_nm, par_gas=B.par_gas, par_w=B.par_w,
                                        fov=fov, ray_blocks=ray_blocks)


def block_ms(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / reps


routes = (("dense", lambda: call(False)), ("per_ray", lambda: call(True)))
out_d = call(False)
walks = dict(dense=engine.last_state_route()[1])
out_r = call(True)
walks["per_ray"] = engine.last_state_route()[1]
scale = np.max(np.abs(out_d), axis=(0, 2), keepdims=True)
agree = float(np.max(np.abs(out_r - out_d) / np.where(scale > 0, scale, 1.0)))
for _, fn in routes:
    block_ms(fn, 3)
reps = {name: max(3, int(np.ceil(500.0 / block_ms(fn, 3)))) for name, fn in routes}
res = {name: [] for name, _ in routes}
for _ in range(n_blocks):                         # A B A B ...
    for name, fn in routes:
        res[name].append(round(block_ms(fn, reps[name]), 4))
med = {k: float(np.median(v)) for k, v in res.items()}
spread = {k: round(max(v) - min(v), 4) for k, v in res.items()}
touched = B.par_w.reshape(len(B.par_gas), -1)
pt = np.asarray(L3["pt_off"])[np.asarray(L3["seg_off"])]
per_ray_touch = [int((touched[:, pt[r]:pt[r + 1]] != 0).any(axis=1).sum()) for r in range(los.n_rays)]
line = json.dumps(dict(case="state_bands_lat_boxes", n_pts=n, n_layers=len(scene.z), n_rays=los.n_rays, n_par=len(B.par_gas), n_box=n_box,
                       n_nodes=n_nodes, touched_per_ray=dict(min=min(per_ray_touch), max=max(per_ray_touch),
                                                             mean=round(float(np.mean(per_ray_touch)), 2)),
                       walks=walks, blocks_ms=res, median_ms={k: round(v, 4) for k, v in med.items()}, spread_ms=spread,
                       calls_per_block=reps, dense_over_per_ray=round(med["dense"] / med["per_ray"], 3),
                       margin_in_spreads=round((med["dense"] - med["per_ray"]) / max(spread["dense"], spread["per_ray"], 1e-9), 1),
                       per_ray_vs_dense_row_err=agree, equal_bits=bool(np.array_equal(out_r, out_d)),
                       device=engine.device_info()["name"]))
print(line, flush=True)
if os.environ.get("OUT"):
    with open(os.environ["OUT"], "w") as f:
        f.write(line + "\n")
los.close()
