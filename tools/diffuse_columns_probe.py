#!/usr/bin/env python3
"""Times engine.diffuse_source_columns (sr_diffuse_columns_kernel) at the shape of a 3-D batch's diffuse pass -- 1e5 grid
points, 80 layers, the haze scene's two gases, 480 step rows -- for n_col = 1, 2, 4, 8, one call each, against the route a
user had before it: n_col engine.diffuse_source(mean_intensity=True) calls, each followed by the torch gather of J on the
steps' layers times the column's weights, and one multiply by the scatterer's rows.  Both routes in alternating rounds in
the same process on the same device; HIP events, medians of 20 calls after 3 warm-ups, three rounds to show the spread.
The two routes' rows are compared before they are timed.
Writes profiles/diffuse_columns_probe.json (or --out).  Needs an MI355X:  python tools/diffuse_columns_probe.py"""
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
    ap.add_argument("--rows", type=int, default=480)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "diffuse_columns_probe.json"))
    a = ap.parse_args()
    import torch
    from spectrobot_amd import engine, geometry as G
    engine.set_device(0)
    n_pts, N, n_rows, n_gas = a.points, a.layers, a.rows, 2
    rng = np.random.default_rng(7)
    z = np.linspace(100.0, 890.0, N)
    nd = 3e17 * np.exp(-(z - 100.0) / 63.0)
    zz = np.append(z, 2 * z[-1] - z[-2])
    vmr = np.array([1.48e-4 * np.ones(N), 0.5 * np.exp(-(z - z[0]) / 250.0)])
    ssa, asym = np.array([0.0, 0.9]), np.array([0.0, 0.5])
    pts = np.append(0.5 * (zz[:-1] + zz[1:]), z[0])
    scale = 1.0 - ssa * np.maximum(asym, 0.0) ** 2
    V = G.vertical_columns(z, nd, vmr)
    A = torch.as_tensor(np.stack([rng.uniform(0.5, 1.5, (N, n_pts)) * 0.3 / V[0].sum(), rng.uniform(0.5, 1.5, (N, n_pts)) * 1.0 / V[1].sum()]),
                        device="cuda")
    sun = torch.as_tensor(rng.uniform(5.0, 20.0, n_pts), device="cuda")
    # the steps: six per layer, cos SZA between 0.15 and 0.75 along the rays
    layer = np.repeat(np.arange(N), (n_rows + N - 1) // N)[:n_rows].astype(np.int32)
    rng.shuffle(layer)
    seg_mu = rng.uniform(0.15, 0.75, n_rows)
    layer_t = torch.as_tensor(layer.astype(np.int64), device="cuda")
    w_out = float(ssa[1] * (1.0 - max(asym[1], 0.0) ** 2))
    res = dict(points=n_pts, layers=N, rows=n_rows, n_gas=n_gas, device=engine.device_info()["name"], columns={})
    for n_col in (1, 2, 4, 8):
        mu0s, col_w = G.sza_columns(seg_mu, n_col)
        n_col = len(mu0s)
        cols = [G.solar_columns(z, nd, vmr, pts, float(m), col_scale=scale) for m in mu0s]
        Ub, lit = np.concatenate([c[0] for c in cols]), np.concatenate([c[1] for c in cols])
        _, beams = engine.solar_source(A, Ub, np.where(lit, 1.0, 0.0), A[1], sun, src_row=np.zeros(len(lit), np.int32), transmission=True)
        beams = beams.view(n_col, N + 1, n_pts)
        w_t = torch.as_tensor(col_w, device="cuda")
        out = torch.empty((n_rows, n_pts), dtype=torch.float64, device="cuda")
        fused = lambda: engine.diffuse_source_columns(A, V, ssa, asym, beams, sun, mu0s, col_w, layer, surface_albedo=0.3, out_gas=1, out=out)

        def composed():
            acc = None
            for c in range(n_col):
                J = engine.diffuse_source(A, V, ssa, asym, beams[c], sun, float(mu0s[c]), surface_albedo=0.3, mean_intensity=True)
                term = J[layer_t] * w_t[:, c:c + 1]
                acc = term if acc is None else acc.add_(term)
            return acc.mul_(A[1][layer_t]).mul_(w_out)

        a_rows, b_rows = fused().clone(), composed()
        rel = float(((a_rows - b_rows).abs() / b_rows.abs().clamp_min(1e-300)).max())
        del a_rows, b_rows
        rounds = [(median_ms(fused), median_ms(composed)) for _ in range(3)]
        f_ms, c_ms = [r[0] for r in rounds], [r[1] for r in rounds]
        res["columns"][str(n_col)] = dict(fused_ms=f_ms, composed_ms=c_ms, speedup=float(np.median(c_ms) / np.median(f_ms)),
                                          margin_ms=float(min(c_ms) - max(f_ms)), spread_ms=float(max(max(f_ms) - min(f_ms), max(c_ms) - min(c_ms))),
                                          max_rel_difference=rel)
        print("n_col %d: one call %s ms, %d diffuse_source calls + gather %s ms (x %.2f); the rows differ by %.1e of their value"
              % (n_col, np.round(f_ms, 3), n_col, np.round(c_ms, 3), res["columns"][str(n_col)]["speedup"], rel))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
