#!/usr/bin/env python3
"""Pressure shift and self-broadening in the coefficient op (engine.LineSet.set_line_shape / set_self_pressure): how
much they move the coefficients, and what the op costs with and without the data.

Two layer stacks on the line list of BASELINE configs[1] (CH4-like, 12 levels, non-LTE; N points, LINES lines):
  configs1  the 80 Titan limb layers of configs[1] (10 hPa and less);
  nadir     40 layers from 1450 hPa (Titan's surface) to 0.01 hPa, equal steps in log P.
Shifts uniform in [-0.012, +0.002] cm^-1/atm, gamma_self in [0.05, 0.12], p_self = 0.05 P.

Per stack:
  effect   per layer, the largest change of the emission coefficient as a fraction of the layer's largest value, for the
           shift alone and for self-broadening alone (a few layers are printed: the first, every tenth, the last);
  time     the folded coefficient op without the data, with the shift, and with both: HIP events around blocks of
           calls, the three variants alternated A B C A B C ... in one process after a warm-up of each, the median
           over BLOCKS blocks of the time per call and the spread (largest - smallest block).  What the data cost is
           the wider near zone (the zone and pole bounds grow by the shift in grid points) where the pressure is high.
N=<points> (100000), LINES=<lines> (N), BLOCKS=<blocks per variant> (7), CALLS=<calls per block> (5).  Prints one JSON
line per stack."""
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
import bench_configs as bc  # noqa: E402
from spectrobot_amd import engine, synthetic as syn  # noqa: E402

engine.set_device(0)
n = int(os.environ.get("N", "100000"))
n_lines = int(os.environ.get("LINES", str(n)))
n_blocks = int(os.environ.get("BLOCKS", "7"))
n_calls = int(os.environ.get("CALLS", "5"))

grid, L, atm, lev = bc.ch4_case(n_lines, n, 80, 12, config_id=2)
rng = np.random.default_rng(3)
p_shift = rng.uniform(-0.012, 0.002, n_lines)
self_broad = rng.uniform(0.05, 0.12, n_lines)
ls = engine.LineSet(L, grid, 6, 1, syn.CH4_MM, lev)

nadir_p = 1450.0 * (0.01 / 1450.0) ** (np.arange(40) / 39.0)
nadir_t = 94.0 + 80.0 * (np.arange(40) / 39.0) ** 2
stacks = {
    "configs1": (atm["temps"], atm["press"], atm["tvib"]),
    "nadir": (nadir_t, nadir_p, np.vstack([nadir_t] + [nadir_t + 30.0] * 11)),
}


def variant(which, press):
    ls.set_line_shape(p_shift if which in ("shift", "both") else None, self_broad if which in ("self", "both") else None)
    ls.set_self_pressure(0.05 * press if which in ("self", "both") else None)


def effect(a, b):
    return ((a - b).abs().amax(dim=1) / b.abs().amax(dim=1)).cpu().numpy()


for name, (T, P, tv) in stacks.items():
    out = (torch.empty((len(T), n), dtype=torch.float64, device="cuda"), torch.empty((len(T), n), dtype=torch.float64, device="cuda"))
    variant("none", P)
    em0 = ls.abscoeff_layers(T, P, tvib=tv)[1].clone()
    eff = {}
    for which in ("shift", "self"):
        variant(which, P)
        eff[which] = effect(ls.abscoeff_layers(T, P, tvib=tv, out=out)[1], em0)
    pick = sorted(set(list(range(0, len(T), 10)) + [len(T) - 1]))
    ms = {w: [] for w in ("none", "shift", "both")}
    for w in ms:                                   # warm-up of every variant
        variant(w, P)
        ls.abscoeff_layers(T, P, tvib=tv, out=out)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    ls.abscoeff_layers(T, P, tvib=tv, out=out)
    e1.record()
    e1.synchronize()
    n_calls = max(1, min(n_calls, int(300.0 / max(e0.elapsed_time(e1), 1e-3))))   # a block of about 0.3 s at most
    for _ in range(n_blocks):
        for w in ms:
            variant(w, P)
            ls.abscoeff_layers(T, P, tvib=tv, out=out)   # (the first call after a change of the data: not timed)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(n_calls):
                ls.abscoeff_layers(T, P, tvib=tv, out=out)
            e1.record()
            e1.synchronize()
            ms[w].append(e0.elapsed_time(e1) / n_calls)
    variant("none", P)
    print(json.dumps({
        "stack": name, "n_points": n, "n_lines": n_lines, "n_layers": len(T),
        "layers": [int(k) for k in pick], "press_hpa": [float("%.4g" % P[k]) for k in pick],
        "effect_shift": [float("%.3g" % eff["shift"][k]) for k in pick],
        "effect_self": [float("%.3g" % eff["self"][k]) for k in pick],
        "ms_per_call": {w: {"median": round(float(np.median(v)), 3), "spread": round(float(max(v) - min(v)), 3)} for w, v in ms.items()},
    }))
