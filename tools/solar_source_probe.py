#!/usr/bin/env python3
"""Times engine.solar_source (sr_solar_source_kernel) at two shapes, 1e5 grid points each:

  scene   the 1-D scene's pass: 80 layer rows, 2 gases x 80 layers, the sun at 60 deg
  batch   a 3-D batch's pass: 18 limb rays of geometry.limb_los_3d (one row per LOS step, ~100 each), 6 gases x 80 layers

with the columns geometry.solar_columns gives (their real sparsity).  Beside each, in alternating rounds in the same
process on the same device: the composed torch route sca[src] * w * sun * exp(-(U @ A)) (the time partner: a dense fp64
matrix product and three passes over an n_rows x n_pts intermediate) and a device-to-device copy of as many bytes as the
call writes.  HIP events, medians of 20 calls after 3 warm-ups, three repeats to show the spread.  Then ONE counter pass of
its own (a child process under rocprofv3 --pmc FETCH_SIZE, no tracing beside it, tools/pmc_cmd_one.sh) takes the bytes the
kernel fetched at the batch shape against the n_k x n_pts x 8 of the absorption rows.  Writes
profiles/solar_source_probe.json (or --out).  Needs an MI355X:  python tools/solar_source_probe.py"""
import argparse
import json
import os
import re
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


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


def shapes(points):
    """{name: dict(A, U, w, sca, sun, src)}: device tensors and host columns of the two shapes."""
    import torch
    from spectrobot_amd import geometry as G
    rng = np.random.default_rng(7)
    z = np.linspace(100.0, 890.0, 80)
    nd = 3e17 * np.exp(-(z - 100.0) / 63.0)
    zz = np.append(z, 2 * z[-1] - z[-2])
    out = {}
    for name, n_gas in (("scene", 2), ("batch", 6)):
        vmr = np.array([10.0 ** -(2 + g) * (1.0 + 0.2 * g * (z - 100.0) / 800.0) for g in range(n_gas)])
        if name == "scene":
            alt, mu, src = 0.5 * (zz[:-1] + zz[1:]), np.cos(np.deg2rad(60.0)), np.arange(80)
        else:
            L3 = G.limb_los_3d(z, nd, vmr, np.linspace(120.0, 460.0, 18), 75.0, 30.0)
            mid = (L3["pt_off"][:-1] + L3["pt_off"][1:] - 1) // 2          # the step's middle sample point (n_sub + 1 = 4: the lower one)
            alt = 0.5 * (L3["alt"][mid] + L3["alt"][mid + 1])
            mu, src = L3["seg_mu"], L3["seg_alt_layer"]
        U, lit = G.solar_columns(z, nd, vmr, alt, mu)
        n_rows = U.shape[0]
        A = torch.as_tensor(rng.uniform(1e-24, 1e-22, (n_gas, 80, points)), device="cuda")
        out[name] = dict(A=A, U=U, w=np.where(lit, 0.07, 0.0), sca=A[n_gas - 1].contiguous(),
                         sun=torch.as_tensor(rng.uniform(5.0, 20.0, points), device="cuda"), src=src.astype(np.int32), n_rows=n_rows)
    return out


def counter_pass(points):
    """The child's body under rocprofv3 --pmc: one fused call at the batch shape."""
    import torch
    from spectrobot_amd import engine
    engine.set_device(0)
    s = shapes(points)["batch"]
    engine.solar_source(s["A"], s["U"], s["w"], s["sca"], s["sun"], src_row=s["src"])
    torch.cuda.synchronize()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=100000)
    ap.add_argument("--counter-pass", action="store_true", help="one fused call at the batch shape (run under rocprofv3 --pmc)")
    ap.add_argument("--no-counters", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "solar_source_probe.json"))
    a = ap.parse_args()
    if a.counter_pass:
        return counter_pass(a.points)
    import torch
    from spectrobot_amd import engine
    engine.set_device(0)
    res = dict(points=a.points, device=engine.device_info()["name"], cases=[])
    for name, s in shapes(a.points).items():
        n_rows, n_k = s["n_rows"], s["U"].shape[1] * s["U"].shape[2]
        out = torch.empty((n_rows, a.points), dtype=torch.float64, device="cuda")
        Ud = torch.as_tensor(s["U"].reshape(n_rows, n_k), device="cuda")
        wd, srcd = torch.as_tensor(s["w"], device="cuda"), torch.as_tensor(s["src"], device="cuda").long()
        A2 = s["A"].view(n_k, a.points)
        off, ch = engine.solar_chunk_lists(s["U"], s["w"])
        src_b, dst_b = (torch.empty(8 * n_rows * a.points, dtype=torch.uint8, device="cuda") for _ in range(2))
        fused = lambda: engine.solar_source(s["A"], s["U"], s["w"], s["sca"], s["sun"], src_row=s["src"], out=out)
        composed = lambda: s["sca"][srcd] * wd[:, None] * s["sun"][None, :] * torch.exp(-(Ud @ A2))
        copy = lambda: dst_b.copy_(src_b)
        rep = [(median_ms(fused), median_ms(composed), median_ms(copy)) for _ in range(3)]     # alternating rounds
        host = []                                            # the host's share of a fused call: checks, lists, staging, launch
        for _ in range(20):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fused()
            host.append(1e3 * (time.perf_counter() - t0))
        diff = float((fused() - composed()).abs().max() / composed().abs().max())
        case = dict(shape=name, n_rows=n_rows, n_k=n_k, zero_fraction=float((s["U"] == 0).mean()),
                    chunks_listed=int(ch.size), chunks_all=int((len(off) - 1) * ((n_k + 3) // 4)), bytes_written=8 * n_rows * a.points,
                    bytes_of_A=8 * n_k * a.points, fused_ms=[r[0] for r in rep], composed_ms=[r[1] for r in rep], copy_ms=[r[2] for r in rep],
                    fused_host_ms=float(np.median(host)), max_rel_difference=diff)
        res["cases"].append(case)
        print("%s: %d rows x %d k (%.0f %% zeros, %d of %d chunks listed): fused %s ms, composed %s ms, copy of the written bytes %s ms; host share of a fused call %.3f ms"
              % (name, n_rows, n_k, 100 * case["zero_fraction"], case["chunks_listed"], case["chunks_all"], np.round(case["fused_ms"], 3),
                 np.round(case["composed_ms"], 3), np.round(case["copy_ms"], 3), case["fused_host_ms"]))
    if not a.no_counters:
        # FETCH_SIZE is in kilobytes (rocprofv3's derived counter)
        cmd = ["bash", os.path.join(ROOT, "tools", "pmc_cmd_one.sh"), "sr_solar", "tools/solar_source_probe.py --counter-pass --points %d" % a.points, "FETCH_SIZE"]
        txt = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=400).stdout.strip()
        m = re.search(r"FETCH_SIZE\s+(\d+)\s+([0-9.eE+-]+)", txt)
        batch = res["cases"][-1]
        res["counters"] = dict(raw=txt, fetched_bytes=None if not m else 1024.0 * float(m[2]) / max(int(m[1]), 1), bytes_of_A=batch["bytes_of_A"])
        print("counter pass:", txt or "(no output)")
        if m:
            print("fetched %.3g bytes against %.3g of the absorption rows: %.2f x" % (res["counters"]["fetched_bytes"], batch["bytes_of_A"],
                                                                                    res["counters"]["fetched_bytes"] / batch["bytes_of_A"]))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
