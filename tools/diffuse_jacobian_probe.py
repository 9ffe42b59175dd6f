#!/usr/bin/env python3
"""Times engine.diffuse_jacobian (sr_diffuse_tangent_kernel + sr_diffuse_contract_kernel) at the shape of a scene's solar
pass -- 1e5 grid points, 80 layers, the haze scene's two gases, 18 rays -- with 6 and with 17 column parameters (node
triangles of three layers), beside what replaces it today: 2 n_par central-difference engine.diffuse_source passes
(mean_intensity=True, the beam scaled on the device) and the torch contraction of their differences with Q; the Q pass
(engine.limb_rays_layer_jacobian); a device-to-device copy of the op's counted bytes; and one inversion_state iteration
on the tests' multiple-scattering twin with the flag off and on.  Alternating rounds in the same process on the same
device; HIP events, medians of 20 calls after 3 warm-ups, three repeats to show the spread.

The op's counted bytes per (parameter, layer, point), NP = 4 parameters per tile, NR = 8 rays per tile: going up
(8 n_gas + 8) / NP (A and beam, read once per tile) + 8 (dlnbeam) + 8 (3 + 4 NP) / NP (workspace out); coming down the same
workspace back + 8 (dJ out); in the contraction 8 ceil(n_rays / NR) (dJ once per ray tile) + 8 n_rays / NP (Q once per
parameter tile).  Writes profiles/diffuse_jacobian_probe.json (or --out).  Needs an MI355X:
python tools/diffuse_jacobian_probe.py"""
import argparse
import copy
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.solar_source_probe import median_ms      # noqa: E402


def iteration_ms(flag, calls=20, warmup=3):
    """One inversion_state iteration on the tests' twin under Sun(multiple=True, surface_albedo=0.3), wall clock around
    synchronised calls; flag on: both solar terms."""
    import torch
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import solar_source_cases as SC
    from spectrobot_amd import engine, retrieval
    scene, pixels, bayes, _, _ = SC.solar_twin(engine)
    scene.sun = retrieval.Sun(SC.SZA_DEG, SC.PHASE_DEG, scene.sun.irradiance, multiple=True, surface_albedo=0.3)
    kw = dict(solar_attenuation=True, diffuse_jacobian=True) if flag else {}
    bs, ms = bayes(), []
    for i in range(warmup + calls):
        b = copy.deepcopy(bs)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        retrieval.inversion_state(scene, b, pixels, max_it=1, **kw)
        torch.cuda.synchronize()
        if i >= warmup:
            ms.append(1e3 * (time.perf_counter() - t0))
    return float(np.median(ms))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=100000)
    ap.add_argument("--layers", type=int, default=80)
    ap.add_argument("--rays", type=int, default=18)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "diffuse_jacobian_probe.json"))
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
    ssa, asym, mu0 = np.array([0.0, 0.9]), np.array([0.0, 0.5]), float(np.cos(np.deg2rad(60.0)))
    pts = np.append(0.5 * (zz[:-1] + zz[1:]), z[0])
    scale = 1.0 - ssa * np.maximum(asym, 0.0) ** 2
    U2, lit2 = G.solar_columns(z, nd, vmr, pts, mu0, col_scale=scale)
    V = G.vertical_columns(z, nd, vmr)
    A = torch.as_tensor(np.stack([rng.uniform(0.5, 1.5, (N, n_pts)) * 0.3 / V[0].sum(), rng.uniform(0.5, 1.5, (N, n_pts)) * 1.0 / V[1].sum()]),
                        device="cuda")
    sun = torch.as_tensor(rng.uniform(5.0, 20.0, n_pts), device="cuda")
    _, beam = engine.solar_source(A, U2, np.where(lit2, 1.0, 0.0), A[1], sun, src_row=np.zeros(N + 1, np.int32), transmission=True)
    emi = torch.as_tensor(rng.uniform(1e-32, 1e-30, (n_gas, N, n_pts)), device="cuda")
    L = G.limb_los(z, nd, vmr, np.linspace(110.0, 800.0, n_rays))
    los = engine.LimbLOS(L["seg_off"], L["seg_layer"], L["pt_off"], L["x"], L["nd"], L["vmr"])
    W = torch.zeros_like(A)
    W[1] = A[1] * float(ssa[1] * scale[1])
    zeros = torch.zeros_like(A)
    q_pass = lambda: engine.limb_rays_layer_jacobian((A, emi), (zeros, W), los)
    Q = q_pass()
    hat = lambda i: np.clip(1.0 - np.abs(np.arange(N) - i) / 2.0, 0.0, None)          # a node triangle of three layers
    res = dict(points=n_pts, layers=N, n_gas=n_gas, n_rays=n_rays, device=engine.device_info()["name"], pars_per_tile=NP, rays_per_tile=NR,
               cases=[])
    for n_par in (6, 17):
        par_gas = [p % n_gas for p in range(n_par)]
        masks = np.array([hat(2 + (N - 5) * p // max(n_par - 1, 1)) for p in range(n_par)]) * vmr[par_gas]
        dV = G.vertical_column_weights(z, nd, masks, par_gas, n_gas)
        dUb, _ = G.solar_column_weights(z, nd, masks, par_gas, n_gas, pts, mu0, col_scale=scale)
        dub = torch.as_tensor(np.ascontiguousarray(dUb.reshape(n_par * (N + 1), n_gas * N)), device="cuda")
        dlnbeam = torch.matmul(dub, A.reshape(n_gas * N, n_pts)).neg_().reshape(n_par, N + 1, n_pts)
        out = torch.empty((n_rays, n_par, n_pts), dtype=torch.float64, device="cuda")
        fused = lambda: engine.diffuse_jacobian(A, V, ssa, asym, beam, sun, mu0, dV, dlnbeam, Q, out=out)
        h = 1e-3

        def differences():
            jac = torch.empty((n_rays, n_par, n_pts), dtype=torch.float64, device="cuda")
            for p in range(n_par):
                Jp = engine.diffuse_source(A, V + h * dV[p], ssa, asym, beam * torch.exp(h * dlnbeam[p]), sun, mu0, mean_intensity=True)
                Jm = engine.diffuse_source(A, V - h * dV[p], ssa, asym, beam * torch.exp(-h * dlnbeam[p]), sun, mu0, mean_intensity=True)
                jac[:, p] = torch.einsum("rlj,lj->rj", Q, (Jp - Jm) / (2 * h))
            return jac

        per_cell = (8 * n_gas + 8) / NP + 8 + 2 * 8 * (3 + 4 * NP) / NP + 8 + 8 * ((n_rays + NR - 1) // NR) + 8 * n_rays / NP
        op_bytes = int(per_cell * n_par * N * n_pts)
        src_b, dst_b = (torch.empty(op_bytes // 2, dtype=torch.uint8, device="cuda") for _ in range(2))
        copy_ = lambda: dst_b.copy_(src_b)
        rep = [(median_ms(fused), median_ms(differences, calls=5, warmup=1), median_ms(copy_), median_ms(q_pass)) for _ in range(3)]
        ref = differences()
        diff = float((fused() - ref).abs().max() / ref.abs().max())
        f_ms, c_ms = (float(np.median([r[i] for r in rep])) for i in (0, 2))
        case = dict(n_par=n_par, mask_layers=3, bytes_per_par_layer_point=per_cell, op_bytes=op_bytes, fused_ms=[r[0] for r in rep],
                    differences_ms=[r[1] for r in rep], copy_ms=[r[2] for r in rep], q_pass_ms=[r[3] for r in rep],
                    copy_rate_TBps=op_bytes / (c_ms * 1e-3) / 1e12, time_over_floor=f_ms / c_ms, max_rel_difference_to_differences=diff)
        res["cases"].append(case)
        print("%d parameters: fused %s ms, 2 n_par difference passes + contraction %s ms, Q pass %s ms; counted bytes %.3f GB "
              "(%.1f per (parameter, layer, point)), a copy of as many %s ms (%.2f TB/s): the op takes %.2f x that floor; largest "
              "relative difference to the differences %.1e"
              % (n_par, np.round(case["fused_ms"], 3), np.round(case["differences_ms"], 3), np.round(case["q_pass_ms"], 3), op_bytes / 1e9,
                 per_cell, np.round(case["copy_ms"], 3), case["copy_rate_TBps"], case["time_over_floor"], diff))
        del src_b, dst_b, out, dlnbeam, ref
    it = [(iteration_ms(False), iteration_ms(True)) for _ in range(3)]
    res["iteration"] = dict(scene="tests/solar_source_cases.solar_twin, Sun(multiple=True, surface_albedo=0.3)", off_ms=[r[0] for r in it],
                            on_ms=[r[1] for r in it])
    print("one inversion_state iteration on the tests' twin: flags off %s ms, on %s ms"
          % (np.round(res["iteration"]["off_ms"], 3), np.round(res["iteration"]["on_ms"], 3)))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
