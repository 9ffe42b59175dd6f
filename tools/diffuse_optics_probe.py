#!/usr/bin/env python3
"""Times engine.diffuse_optics_jacobian (sr_diffuse_tangent_kernel's optics instance + sr_diffuse_contract_kernel) at the
shape of a scene's solar pass -- 1e5 grid points, 80 layers, the haze scene's two gases, 18 rays -- for the three optics
parameters of a haze (ssa, g, surface albedo) and for a surface-albedo direction alone, beside
  - what it replaces: 2 n_par central-difference engine.diffuse_source passes (mean_intensity=True) and the torch
    contraction of their differences with Q;
  - engine.diffuse_jacobian with as many parameters and a dense dV (every layer inside the range: the like-for-like
    partner of an ssa / g direction) and with dV = 0 (every layer outside it: the partner of the albedo alone);
  - a device-to-device copy of the op's counted bytes, the byte floor.
Alternating rounds in the same process on the same device; HIP events, medians of 20 calls after 3 warm-ups, three rounds.

The op's counted bytes per (parameter, layer, point) are diffuse_jacobian's (tools/diffuse_jacobian_probe.py): the
direction itself is 25 doubles per parameter in scalar loads.  Writes profiles/diffuse_optics_probe.json (or --out).
Needs an MI355X: python tools/diffuse_optics_probe.py"""
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
    ap.add_argument("--rays", type=int, default=18)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "diffuse_optics_probe.json"))
    a = ap.parse_args()
    import torch
    from spectrobot_amd import engine, geometry as G
    engine.set_device(0)
    n_pts, N, n_gas, n_rays = a.points, a.layers, 2, a.rays
    NP, NR = engine.DIFFUSE_JAC_PARS, engine.DIFFUSE_JAC_RAYS
    rng = np.random.default_rng(7)
    z = np.linspace(100.0, 890.0, N)
    nd = 3e17 * np.exp(-(z - 100.0) / 63.0)
    zz = np.append(z, 2 * z[-1] - z[-2])
    vmr = np.array([1.48e-4 * np.ones(N), 0.5 * np.exp(-(z - z[0]) / 250.0)])
    ssa, asym, mu0, albedo = np.array([0.0, 0.9]), np.array([0.0, 0.5]), float(np.cos(np.deg2rad(60.0))), 0.3
    pts = np.append(0.5 * (zz[:-1] + zz[1:]), z[0])
    scale = 1.0 - ssa * np.maximum(asym, 0.0) ** 2
    U2, lit2 = G.solar_columns(z, nd, vmr, pts, mu0, col_scale=scale)
    V = G.vertical_columns(z, nd, vmr)
    A = torch.as_tensor(np.stack([rng.uniform(0.5, 1.5, (N, n_pts)) * 0.3 / V[0].sum(), rng.uniform(0.5, 1.5, (N, n_pts)) * 1.0 / V[1].sum()]),
                        device="cuda")
    sun = torch.as_tensor(rng.uniform(5.0, 20.0, n_pts), device="cuda")
    _, beam = engine.solar_source(A, U2, np.where(lit2, 1.0, 0.0), A[1], sun, src_row=np.zeros(N + 1, np.int32), transmission=True)
    Q = torch.as_tensor(rng.uniform(0.1, 1.0, (n_rays, N, n_pts)), device="cuda")
    res = dict(points=n_pts, layers=N, n_gas=n_gas, n_rays=n_rays, device=engine.device_info()["name"], pars_per_tile=NP, rays_per_tile=NR,
               cases=[])
    e = lambda *rows: np.array(rows, float)
    for name, dssa, dasym, dalb in (("ssa, g, surface albedo", e([0, 1], [0, 0], [0, 0]), e([0, 0], [0, 1], [0, 0]), e(0, 0, 1)),
                                    ("surface albedo alone", None, None, e(1))):
        n_par = dalb.shape[0]
        zero2 = np.zeros((n_par, n_gas))
        dlnbeam = torch.as_tensor(rng.uniform(-0.1, 0.1, (n_par, N + 1, n_pts)), device="cuda")
        out = torch.empty((n_rays, n_par, n_pts), dtype=torch.float64, device="cuda")
        fused = lambda: engine.diffuse_optics_jacobian(A, V, ssa, asym, beam, sun, mu0, dssa, dasym, dalb, dlnbeam, Q,
                                                       surface_albedo=albedo, out=out)
        dense = np.broadcast_to(V[None], (n_par, n_gas, N)).copy()
        columns_in = lambda: engine.diffuse_jacobian(A, V, ssa, asym, beam, sun, mu0, dense, dlnbeam, Q, surface_albedo=albedo, out=out)
        columns_out = lambda: engine.diffuse_jacobian(A, V, ssa, asym, beam, sun, mu0, 0.0 * dense, dlnbeam, Q, surface_albedo=albedo,
                                                      out=out)
        h = 1e-3
        ds, da = (zero2 if x is None else x for x in (dssa, dasym))

        def differences():
            jac = torch.empty((n_rays, n_par, n_pts), dtype=torch.float64, device="cuda")
            for p in range(n_par):
                J = [engine.diffuse_source(A, V, ssa + s * h * ds[p], asym + s * h * da[p], beam * torch.exp(s * h * dlnbeam[p]), sun, mu0,
                                           surface_albedo=albedo + s * h * dalb[p], mean_intensity=True) for s in (1.0, -1.0)]
                jac[:, p] = torch.einsum("rlj,lj->rj", Q, (J[0] - J[1]) / (2 * h))
            return jac

        per_cell = (8 * n_gas + 8) / NP + 8 + 2 * 8 * (3 + 4 * NP) / NP + 8 + 8 * ((n_rays + NR - 1) // NR) + 8 * n_rays / NP
        op_bytes = int(per_cell * n_par * N * n_pts)
        src_b, dst_b = (torch.empty(op_bytes // 2, dtype=torch.uint8, device="cuda") for _ in range(2))
        copy_ = lambda: dst_b.copy_(src_b)
        rep = [(median_ms(fused), median_ms(differences, calls=5, warmup=1), median_ms(columns_in), median_ms(columns_out), median_ms(copy_))
               for _ in range(3)]
        ref = differences()
        diff = float((fused() - ref).abs().max() / ref.abs().max())
        f_ms, c_ms = (float(np.median([r[i] for r in rep])) for i in (0, 4))
        case = dict(direction=name, n_par=n_par, bytes_per_par_layer_point=per_cell, op_bytes=op_bytes, fused_ms=[r[0] for r in rep],
                    differences_ms=[r[1] for r in rep], column_op_dense_dV_ms=[r[2] for r in rep], column_op_zero_dV_ms=[r[3] for r in rep],
                    copy_ms=[r[4] for r in rep], copy_rate_TBps=op_bytes / (c_ms * 1e-3) / 1e12, time_over_floor=f_ms / c_ms,
                    max_rel_difference_to_differences=diff)
        res["cases"].append(case)
        print("%s (%d parameters): fused %s ms, 2 n_par difference passes + contraction %s ms, the column op with a dense dV %s ms, "
              "with dV = 0 %s ms; counted bytes %.3f GB, a copy of as many %s ms (%.2f TB/s): the op takes %.2f x that floor; largest "
              "relative difference to the differences %.1e"
              % (name, n_par, np.round(case["fused_ms"], 3), np.round(case["differences_ms"], 3), np.round(case["column_op_dense_dV_ms"], 3),
                 np.round(case["column_op_zero_dV_ms"], 3), op_bytes / 1e9, np.round(case["copy_ms"], 3), case["copy_rate_TBps"],
                 case["time_over_floor"], diff))
        del src_b, dst_b, out, dlnbeam, ref
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
