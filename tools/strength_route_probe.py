#!/usr/bin/env python3
"""Cost of the strength route at BASELINE configs[1] size (1e5 lines x 1e5 points x 80 layers, 12 non-LTE levels):
abscoeff_layers (G weights) against abscoeff_layers_from_strengths (HITRAN weights, same kernels) and line_strengths
(both sources), each timed with HIP events over --reps calls after --warmup.  Prints one JSON line (ms per call,
medians).  usage: python tools/strength_route_probe.py [--reps 20] [--warmup 3]"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed(fn, reps, warmup):
    import torch
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return float(np.median(ms)), float(np.min(ms))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()
    import __graft_entry__ as ge
    ge.ensure_built()
    import torch
    import bench_configs as bc
    from spectrobot_amd import engine, spect_classes as sc, synthetic as syn
    engine.set_device(0)
    grid, L, atm, lev = bc.ch4_case(100000, 100000, 80, 12, config_id=2)
    ls = engine.LineSet(L, grid, 6, 1, syn.CH4_MM, lev)
    q296 = sc.CalcPartitionSum(6, 1, temp=296.0)
    ls.set_strengths(sc.Einstein_A_to_LineStrength_hitran(L["a_coeff"], L["freq"], 296.0, q296, L["g_up"], L["e_lower"],
                                                          syn.CH4_ISO_RATIO), iso_ab=syn.CH4_ISO_RATIO)
    T, P, tv = atm["temps"], atm["press"], atm["tvib"]
    n = len(T)
    out = (torch.empty((n, grid.size), dtype=torch.float64, device="cuda"),
           torch.empty((n, grid.size), dtype=torch.float64, device="cuda"))
    g_med, g_min = timed(lambda: ls.abscoeff_layers(T, P, tvib=tv, out=out), args.reps, args.warmup)
    s_med, s_min = timed(lambda: ls.abscoeff_layers_from_strengths(T, P, tvib=tv, out=out), args.reps, args.warmup)
    h_med, h_min = timed(lambda: ls.line_strengths(T, tvib=tv, source="hitran"), args.reps, args.warmup)
    e_med, e_min = timed(lambda: ls.line_strengths(T, tvib=tv, source="einstein", iso_ab=syn.CH4_ISO_RATIO),
                         args.reps, args.warmup)
    print(json.dumps({
        "probe": "strength_route", "device": engine.device_info(),
        "workload": "BASELINE configs[1]: %d lines x %d points x %d layers, 12 non-LTE levels" % (len(L["freq"]), grid.size, n),
        "reps": args.reps, "warmup": args.warmup,
        "abscoeff_layers_ms": round(g_med, 4), "abscoeff_layers_min_ms": round(g_min, 4),
        "from_strengths_ms": round(s_med, 4), "from_strengths_min_ms": round(s_min, 4),
        "strength_over_g": round(s_med / g_med, 4),
        "line_strengths_hitran_ms": round(h_med, 4), "line_strengths_einstein_ms": round(e_med, 4),
        "line_strengths_bytes": 2 * 8 * n * len(L["freq"]),
        "line_strengths_hitran_gbps": round(2 * 8 * n * len(L["freq"]) / (h_med * 1e-3) / 1e9, 1),
    }))
    ls.close()


if __name__ == "__main__":
    main()
