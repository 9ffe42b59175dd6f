#!/usr/bin/env python3
"""What a gas slot above four costs: the state-bands call (engine.limb_rays_state_bands, one column parameter per gas) and
engine.limb_rays for batches of 4, 5, 6 and 8 gases on the shape of tools/state_bands_probe.py -- 18 pixels x 3 lines of
sight, 55 layers, 1e5 points, 14 bands, field of view.  The coefficient tables are synthetic (random, thin to thick): the
recursion kernels' time does not depend on their values.  Four gases run the instances of sr_limb.hip (the folded sweep
for limb_rays: route 2) and of sr_limb_state_34_np8.hip, five to eight those of sr_limb_many.hip (path order, route 1; five gases on the six-gas state
instance).  HIP events around every call, the median of 20 calls after 3, three repeats of that; per gas count the median
of the repeats, their spread, the ratio to the four-gas call of the same run, and the waves per SIMD the instance's VGPR
count leaves (512 VGPRs per lane and SIMD, allocated in blocks of 8; the counts are read from
profiles/many_gases_kernel_resources.txt, those of the four-gas instances are copied, see vgpr_of).  N=<points>, LAYERS=<layers> for other sizes; OUT=<file> also writes the lines there.  One JSON line per case
and a last line with the summary."""
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
from spectrobot_amd import engine, synthetic as syn  # noqa: E402

engine.set_device(0)
n = int(os.environ.get("N", "100000"))
n_layers = int(os.environ.get("LAYERS", "55"))
n_pix = 18
grid = syn.make_grid(3290.0, 5e-4, n)
atm = syn.make_atmosphere(n_layers, 12)
z, temps, press = atm["z"], atm["temps"], atm["press"]
span = z[-1] - z[0]
tang = [z[0] + (0.06 + 0.045 * i) * span + d * 0.02 * span for i in range(n_pix) for d in (-1.0, 0.0, 1.0)]
fov_fac = engine.fov_factors([10.0 * (i % 3) for i in range(n_pix)])
lam_lo, lam_hi = 1e7 / grid[-1], 1e7 / grid[0]
margin = min(1.2, 0.1 * (lam_hi - lam_lo))
bands = (np.linspace(lam_lo + margin, lam_hi - margin, 14), np.full(14, min(1.1, 0.1 * (lam_hi - lam_lo))))
# VGPRs of the instances the calls run.  Five to eight gases: read from profiles/many_gases_kernel_resources.txt, the output
# of `tools/kernel_resources.sh sr_` for the kernels of sr_limb_many.hip, kept with the code (regenerate it when the kernels
# change); four gases: COPIED from `tools/kernel_resources.sh sr_` of 2026-10-20 -- the JSON says so.
RES = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "many_gases_kernel_resources.txt")
VGPR_FOUR = {"state_bands": 116, "limb_rays": 76}    # sr_limb_jac_state_kernel<4, 8, true, false, true, false>, sr_limb_fold_fwd_kernel<4>


def vgpr_of(name, n_gas):
    if n_gas <= 4:
        return VGPR_FOUR[name], "copied 2026-10-20"
    ng = n_gas + (n_gas & 1) if name == "state_bands" else n_gas      # (five gases run the six-gas state instance)
    kernel = "sr_limb_jac_state_kernel<%d, 8, true, false, true, false>" % ng if name == "state_bands" else "sr_limb_kernel<%d>" % ng
    for line in open(RES):
        if line.startswith(kernel + " "):
            return int(line.split("vgpr")[1].split()[0]), os.path.basename(RES)
    raise RuntimeError("%s is not in %s" % (kernel, RES))


def waves_per_simd(vgpr):
    return min(8, 512 // (8 * ((vgpr + 7) // 8)))


def event_ms(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def median_of_20_after_3(fn):
    for _ in range(3):
        fn()
    return float(np.median([event_ms(fn) for _ in range(20)]))


lines, summary = [], {}
gen = torch.Generator(device="cuda").manual_seed(1)
for n_gas in (4, 5, 6, 8):
    vmr = [np.full(n_layers, 1e-4 * (g + 1)) for g in range(n_gas)]
    Lr = syn.limb_los(z, syn.number_density(press, temps), vmr, tang)
    los = engine.LimbLOS(Lr["seg_off"], Lr["seg_layer"], Lr["pt_off"], Lr["x"], Lr["nd"], Lr["vmr"])
    u = torch.rand((n_gas, n_layers, n), dtype=torch.float64, device="cuda", generator=gen)
    a = torch.exp(-50.0 + 12.0 * u) / n_gas          # optical depths from thin to thick along a limb path
    coeffs = (a, a * torch.rand((n_gas, n_layers, n), dtype=torch.float64, device="cuda", generator=gen))
    par_gas = np.arange(n_gas, dtype=np.int32)
    par_w = np.array([np.asarray(Lr["vmr"])[g] for g in range(n_gas)])
    calls = {"state_bands": lambda: engine.limb_rays_state_bands(coeffs, los, grid, bands[0], bands[1], par_gas, par_w, fov=fov_fac),
             "limb_rays": lambda: engine.limb_rays(coeffs, los)}
    for name, fn in calls.items():
        reps = [round(median_of_20_after_3(fn), 4) for _ in range(3)]
        route = engine.last_state_route()[0] if name == "state_bands" else engine.last_limb_route()
        rec = dict(call=name, n_gas=n_gas, n_pts=n, n_layers=n_layers, n_rays=los.n_rays, n_par=n_gas, n_bands=14, repeats_ms=reps,
                   median_ms=float(np.median(reps)), spread_ms=round(max(reps) - min(reps), 4), route=route,
                   vgpr=vgpr_of(name, n_gas)[0], vgpr_source=vgpr_of(name, n_gas)[1], waves_per_simd=waves_per_simd(vgpr_of(name, n_gas)[0]),
                   device=engine.device_info()["name"])
        summary.setdefault(name, {})[n_gas] = rec["median_ms"]
        lines.append(rec)
        print(json.dumps(rec), flush=True)
    los.close()
ratios = {name: {str(g): round(ms / v[4], 3) for g, ms in v.items()} for name, v in summary.items()}
last = dict(summary_ms={k: {str(g): ms for g, ms in v.items()} for k, v in summary.items()}, ratio_to_four_gases=ratios)
print(json.dumps(last))
if os.environ.get("OUT"):
    with open(os.environ["OUT"], "w") as f:
        json.dump(dict(cases=lines, **last), f, indent=1)
        f.write("\n")
