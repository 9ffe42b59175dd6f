#!/usr/bin/env python3
"""Times engine.AbsorberTable.layers (sr_absorber_table_kernel) at 1e5 grid points x 80 rows, with and without the
derivative and accumulation, beside a plain device-to-device copy of as many bytes as the call writes (plus, accumulating,
the bytes it reads back) -- same process, same device.  HIP events, medians of 20 calls after 3 warm-ups, three repeats
to show the spread.  Writes profiles/absorber_table_probe.json (or --out).  Needs an MI355X:
python tools/absorber_table_probe.py"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def median_ms(fn, calls=20, warmup=3):
    import torch
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(calls):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return float(np.median(ms))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=100000)
    ap.add_argument("--rows", type=int, default=80)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "absorber_table_probe.json"))
    a = ap.parse_args()
    import torch
    from spectrobot_amd import engine, synthetic as syn
    engine.set_device(0)
    grid = syn.make_grid(2950.0, 1e-3, a.points)
    rng = np.random.default_rng(3)
    v0, v1 = grid[0] - 0.5, grid[-1] + 0.5
    # 8 temperature sets at 0.015 cm^-1 (a cross-section file's spacing): ~7e3 values each, resident in L2
    n = int((v1 - v0) / 0.015) + 2
    tab = engine.AbsorberTable([(100.0 + 20.0 * k, v0, (v1 - v0) / (n - 1), 1e-20 * rng.uniform(0.1, 1.0, n)) for k in range(8)])
    temps = np.linspace(105.0, 235.0, a.rows)
    scale = np.full(a.rows, 3.0e17)
    res = dict(points=a.points, rows=a.rows, device=engine.device_info()["name"], cases=[])
    for derivative in (False, True):
        for accumulate in (False, True):
            n_out = 4 if derivative else 2
            bufs = [torch.zeros((a.rows, a.points), dtype=torch.float64, device="cuda") for _ in range(n_out)]
            out = ((bufs[0], bufs[1]), (bufs[2], bufs[3])) if derivative else (bufs[0], bufs[1])
            n_bytes = 8 * a.rows * a.points * n_out * (2 if accumulate else 1)    # written (+ read back when accumulating)
            src = torch.empty(n_bytes // 2, dtype=torch.uint8, device="cuda")      # a copy moves its bytes twice: read + write
            dst = torch.empty_like(src)
            call = lambda: tab.layers(temps, grid, scale=scale, derivative=derivative, out=out, accumulate=accumulate)
            copy = lambda: dst.copy_(src)
            rep = [(median_ms(call), median_ms(copy)) for _ in range(3)]
            case = dict(derivative=derivative, accumulate=accumulate, bytes=n_bytes, call_ms=[r[0] for r in rep], copy_ms=[r[1] for r in rep],
                        ratio=[r[0] / r[1] for r in rep])
            res["cases"].append(case)
            print("derivative %d accumulate %d: %.1f MB; layers %s ms, copy of as many bytes %s ms, ratio %s"
                  % (derivative, accumulate, n_bytes / 1e6, np.round(case["call_ms"], 4), np.round(case["copy_ms"], 4), np.round(case["ratio"], 2)))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
