#!/usr/bin/env python3
"""Times engine.diffuse_thermal_source (sr_diffuse_field_kernel) at the shape of a scene's pass -- 1e5 grid points, 80
layers, the haze scene's two gases, the fused accumulate into the haze's rows with own_emission -- as the call with both
sources (sun and thermal emission) and as the night call (thermal emission alone), beside engine.diffuse_source on the
same arrays, in alternating rounds in the same process on the same device.  HIP events, medians of 20 calls after 3
warm-ups, three rounds to show the spread.

The bytes per (layer, point): the call with both sources counts diffuse_source's 112 -- 8 n_gas (A) + 8 (beam) + 32
(workspace out) going up, 32 (workspace back) + 8 (the scatterer's row) + 16 (emi read and written under accumulate)
coming down; the Planck values are formed in registers --, the night call saves the 8 of beam.  Each is set against a
device-to-device copy of as many bytes (half read, half written) measured beside it.  The question the numbers answer:
does one fused call cost clearly less than diffuse_source plus a separate thermal walk (the night call) would?
Writes profiles/diffuse_thermal_probe.json (or --out).  Needs an MI355X:  python tools/diffuse_thermal_probe.py"""
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "diffuse_thermal_probe.json"))
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
    temps = np.linspace(94.0, 180.0, N)
    grid = 600.0 + 0.0078125 * np.arange(n_pts)      # (an exact step: engine.grid_params)
    mids = 0.5 * (zz[:-1] + zz[1:])
    scale = 1.0 - ssa * np.maximum(asym, 0.0) ** 2
    U2, lit2 = G.solar_columns(z, nd, vmr, np.append(mids, z[0]), mu0, col_scale=scale)
    V = G.vertical_columns(z, nd, vmr)
    A = torch.as_tensor(np.stack([rng.uniform(0.5, 1.5, (N, n_pts)) * 0.3 / V[0].sum(), rng.uniform(0.5, 1.5, (N, n_pts)) * 1.0 / V[1].sum()]),
                        device="cuda")
    sun = torch.as_tensor(rng.uniform(5.0, 20.0, n_pts), device="cuda")
    emi = torch.zeros((N, n_pts), dtype=torch.float64, device="cuda")
    _, beam = engine.solar_source(A, U2, np.where(lit2, 1.0, 0.0), A[1], sun, src_row=np.zeros(N + 1, np.int32), transmission=True)
    kw = dict(t_surface=94.0, surface_albedo=0.1, out_gas=1, out=emi, accumulate=True, own_emission=True)
    both = lambda: engine.diffuse_thermal_source(A, V, ssa, asym, temps, grid, beam=beam, sun=sun, mu0=mu0, **kw)
    night = lambda: engine.diffuse_thermal_source(A, V, ssa, asym, temps, grid, **kw)
    parent = lambda: engine.diffuse_source(A, V, ssa, asym, beam, sun, mu0, surface_albedo=0.1, out_gas=1, out=emi, accumulate=True)
    cell_both = 8 * n_gas + 8 + 32 + 32 + 8 + 16
    cell_night = cell_both - 8
    bufs = {c: tuple(torch.empty(c * N * n_pts // 2, dtype=torch.uint8, device="cuda") for _ in range(2)) for c in (cell_both, cell_night)}
    copy_both = lambda: bufs[cell_both][1].copy_(bufs[cell_both][0])
    copy_night = lambda: bufs[cell_night][1].copy_(bufs[cell_night][0])
    calls = (("both_ms", both), ("night_ms", night), ("diffuse_source_ms", parent), ("copy_both_ms", copy_both), ("copy_night_ms", copy_night))
    rounds = [{name: median_ms(fn) for name, fn in calls} for _ in range(3)]
    res = dict(points=n_pts, layers=N, n_gas=n_gas, device=engine.device_info()["name"], bytes_per_layer_point=dict(both=cell_both, night=cell_night))
    for name, _ in calls:
        res[name] = [r[name] for r in rounds]
    med = {name: float(np.median(res[name])) for name, _ in calls}
    res["both_over_copy"] = med["both_ms"] / med["copy_both_ms"]
    res["night_over_copy"] = med["night_ms"] / med["copy_night_ms"]
    res["both_over_diffuse_source"] = med["both_ms"] / med["diffuse_source_ms"]
    res["both_over_diffuse_source_plus_night"] = med["both_ms"] / (med["diffuse_source_ms"] + med["night_ms"])
    print("%d points x %d layers x %d gases: both sources %s ms, night %s ms, diffuse_source %s ms"
          % (n_pts, N, n_gas, np.round(res["both_ms"], 3), np.round(res["night_ms"], 3), np.round(res["diffuse_source_ms"], 3)))
    print("copies of the counted bytes: %d B per (layer, point) %s ms, %d B %s ms: both %.2f x its copy, night %.2f x its copy"
          % (cell_both, np.round(res["copy_both_ms"], 3), cell_night, np.round(res["copy_night_ms"], 3), res["both_over_copy"], res["night_over_copy"]))
    print("one fused call / (diffuse_source + a separate thermal walk): %.2f; / diffuse_source alone: %.2f"
          % (res["both_over_diffuse_source_plus_night"], res["both_over_diffuse_source"]))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
