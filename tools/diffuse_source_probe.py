#!/usr/bin/env python3
"""Times engine.diffuse_source (sr_diffuse_field_kernel) at the shape of a scene's solar pass -- 1e5 grid points, 80
layers, the haze scene's two gases (a line gas and the scattering haze), the fused accumulate into the haze's rows -- with
the two engine.solar_source calls of the same pass beside it (the single-scattering rows of 80 layer points, and the
direct beam at the 80 layer middles plus the lower boundary, transmission=True), in alternating rounds in the same process
on the same device.  HIP events, medians of 20 calls after 3 warm-ups, three repeats to show the spread.

The op's bytes per (layer, point) -- 8 n_gas (A) + 8 (beam) + 32 (workspace out) going up, 32 (workspace back) + 8 (the
scatterer's row) + 16 (emi read and written under accumulate) coming down -- are set against the rate of a device-to-
device copy of as many bytes (half read, half written) measured beside it: the floor the memory system allows.
Writes profiles/diffuse_source_probe.json (or --out).  Needs an MI355X:  python tools/diffuse_source_probe.py"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.solar_source_probe import median_ms      # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=100000)
    ap.add_argument("--layers", type=int, default=80)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "diffuse_source_probe.json"))
    a = ap.parse_args()
    import torch
    from spectrobot_amd import engine, geometry as G
    engine.set_device(0)
    n_pts, N, n_gas = a.points, a.layers, 2
    rng = np.random.default_rng(7)
    z = np.linspace(100.0, 890.0, N)
    nd = 3e17 * np.exp(-(z - 100.0) / 63.0)
    zz = np.append(z, 2 * z[-1] - z[-2])
    vmr = np.array([1.48e-4 * np.ones(N), 0.5 * np.exp(-(z - z[0]) / 250.0)])
    ssa, asym, mu0 = np.array([0.0, 0.9]), np.array([0.0, 0.5]), float(np.cos(np.deg2rad(60.0)))
    mids = 0.5 * (zz[:-1] + zz[1:])
    U1, lit1 = G.solar_columns(z, nd, vmr, mids, mu0)
    scale = 1.0 - ssa * np.maximum(asym, 0.0) ** 2
    U2, lit2 = G.solar_columns(z, nd, vmr, np.append(mids, z[0]), mu0, col_scale=scale)
    V = G.vertical_columns(z, nd, vmr)
    # absorption rows that give the haze a vertical optical depth of order one and the line gas a few tenths
    A = torch.as_tensor(np.stack([rng.uniform(0.5, 1.5, (N, n_pts)) * 0.3 / V[0].sum(), rng.uniform(0.5, 1.5, (N, n_pts)) * 1.0 / V[1].sum()]),
                        device="cuda")
    sun = torch.as_tensor(rng.uniform(5.0, 20.0, n_pts), device="cuda")
    emi = torch.zeros((N, n_pts), dtype=torch.float64, device="cuda")
    w1 = np.where(lit1, 0.9 * G.hg_phase(-0.5, 0.5) / (4 * np.pi), 0.0)
    single = lambda: engine.solar_source(A, U1, w1, A[1], sun, out=emi, accumulate=True)
    beam_call = lambda: engine.solar_source(A, U2, np.where(lit2, 1.0, 0.0), A[1], sun, src_row=np.zeros(N + 1, np.int32), transmission=True)
    _, beam = beam_call()
    diffuse = lambda: engine.diffuse_source(A, V, ssa, asym, beam, sun, mu0, surface_albedo=0.0, out_gas=1, out=emi, accumulate=True)
    per_cell = 8 * n_gas + 8 + 32 + 32 + 8 + 16
    op_bytes = per_cell * N * n_pts
    src_b, dst_b = (torch.empty(op_bytes // 2, dtype=torch.uint8, device="cuda") for _ in range(2))
    copy = lambda: dst_b.copy_(src_b)
    rep = [(median_ms(diffuse), median_ms(single), median_ms(beam_call), median_ms(copy)) for _ in range(3)]
    d_ms, s_ms, b_ms, c_ms = (float(np.median([r[i] for r in rep])) for i in range(4))
    J = engine.diffuse_source(A, V, ssa, asym, beam, sun, mu0, mean_intensity=True)
    res = dict(points=n_pts, layers=N, n_gas=n_gas, device=engine.device_info()["name"], bytes_per_layer_point=per_cell, op_bytes=op_bytes,
               diffuse_ms=[r[0] for r in rep], single_scattering_ms=[r[1] for r in rep], beam_ms=[r[2] for r in rep], copy_ms=[r[3] for r in rep],
               copy_rate_TBps=op_bytes / (c_ms * 1e-3) / 1e12, floor_ms=c_ms, time_over_floor=d_ms / c_ms,
               vertical_optical_depth=[float(0.3), float(1.0)], mean_J_over_sun=float((J / sun[None, :]).mean()))
    print("diffuse_source, %d points x %d layers x %d gases: %s ms; beside it the single-scattering rows %s ms and the beam %s ms"
          % (n_pts, N, n_gas, np.round(res["diffuse_ms"], 3), np.round(res["single_scattering_ms"], 3), np.round(res["beam_ms"], 3)))
    print("bytes: %d per (layer, point), %.3f GB; a copy of as many bytes %s ms (%.2f TB/s): the op takes %.2f x that floor"
          % (per_cell, op_bytes / 1e9, np.round(res["copy_ms"], 3), res["copy_rate_TBps"], res["time_over_floor"]))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
