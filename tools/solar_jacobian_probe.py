#!/usr/bin/env python3
"""Times engine.solar_attenuation_jacobian (sr_solar_jac_kernel) at two shapes, 54 limb rays x 80 layer rows x 1e5 grid
points each:

  scene   the 1-D scene's shape: 2 gases x 80 layers, 7 column parameters (4 + 3 hat masks), the sun at 60 deg
  wide    4 gases x 80 layers, 17 column parameters

with the dU geometry.solar_column_weights gives (its real sparsity) and Q from engine.limb_rays_layer_jacobian on the same
rays.  Beside each, in alternating rounds in the same process on the same device: the composed torch route -- dU @ A, then
the product with Q and the row sum in chunks of four rows, so that [n_rays, n_par, n_rows, n_pts] is never whole -- and the Q
pass itself (what a fusion into the recursion would remove) with the bytes it writes.  Then one inversion_state iteration
with solar_attenuation on against off, on the sunlit twin of the tests (600 grid points, 12 layers, 18 lines of sight:
the scene at hand, not the shape above).  HIP events (the iteration: wall clock around a synchronised call), medians of 20
calls after 3 warm-ups, three repeats to show the spread.  Writes profiles/solar_jacobian_probe.json (or --out).  Needs an
MI355X:  python tools/solar_jacobian_probe.py"""
import argparse
import json
import os
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


def shapes(points, n_rays=54):
    """{name: dict(A, dU, Q, q_pass)}: device tensors, the host dU and the call that makes Q."""
    import torch
    from spectrobot_amd import engine, geometry as G
    rng = np.random.default_rng(7)
    z = np.linspace(100.0, 890.0, 80)
    nd = 3e17 * np.exp(-(z - 100.0) / 63.0)
    zz = np.append(z, 2 * z[-1] - z[-2])
    hat = lambda zc, h: np.clip(1.0 - np.abs(z - zc) / h, 0.0, None)
    out = {}
    for name, n_gas, nodes in (("scene", 2, (4, 3)), ("wide", 4, (5, 4, 4, 4))):
        vmr = np.array([10.0 ** -(2 + g) * (1.0 + 0.2 * g * (z - 100.0) / 800.0) for g in range(n_gas)])
        masks, par_gas = [], []
        for g, n in enumerate(nodes):
            for zc in np.linspace(120.0, 860.0, n):
                masks.append(hat(zc, 740.0 / max(n - 1, 1)))
                par_gas.append(g)
        dU, lit = G.solar_column_weights(z, nd, np.array(masks), par_gas, n_gas, 0.5 * (zz[:-1] + zz[1:]), np.cos(np.deg2rad(60.0)))
        A = torch.as_tensor(rng.uniform(1e-24, 1e-22, (n_gas, 80, points)), device="cuda")
        emi = torch.as_tensor(rng.uniform(1e-32, 1e-30, (n_gas, 80, points)), device="cuda")
        sol = torch.zeros_like(emi)
        sol[n_gas - 1] = emi[n_gas - 1] * 0.5
        L = G.limb_los(z, nd, vmr, np.linspace(110.0, 800.0, n_rays))
        los = engine.LimbLOS(L["seg_off"], L["seg_layer"], L["pt_off"], L["x"], L["nd"], L["vmr"])
        zeros = torch.zeros_like(A)
        q_pass = lambda A=A, emi=emi, zeros=zeros, sol=sol, los=los: engine.limb_rays_layer_jacobian((A, emi), (zeros, sol), los)
        out[name] = dict(A=A, dU=dU, q_pass=q_pass, n_par=len(masks), n_k=n_gas * 80)
    return out


def composed(A2, dUd, Q, chunk=4):
    import torch
    dtau = dUd @ A2                                           # [n_par, n_rows, n_pts]
    out = torch.zeros((Q.shape[0], dUd.shape[0], A2.shape[1]), dtype=torch.float64, device="cuda")
    for r in range(0, Q.shape[1], chunk):
        out -= (Q[:, None, r:r + chunk] * dtau[None, :, r:r + chunk]).sum(dim=2)
    return out


def iteration_ms(flag, calls=20, warmup=3):
    """One inversion_state iteration on the tests' sunlit twin, wall clock around synchronised calls."""
    import copy
    import torch
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import solar_source_cases as SC
    from spectrobot_amd import engine, retrieval
    scene, pixels, bayes, _, _ = SC.solar_twin(engine)
    bs, ms = bayes(), []
    for i in range(warmup + calls):
        b = copy.deepcopy(bs)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        retrieval.inversion_state(scene, b, pixels, max_it=1, solar_attenuation=flag)
        torch.cuda.synchronize()
        if i >= warmup:
            ms.append(1e3 * (time.perf_counter() - t0))
    return float(np.median(ms))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=100000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "solar_jacobian_probe.json"))
    a = ap.parse_args()
    import torch
    from spectrobot_amd import engine
    engine.set_device(0)
    res = dict(points=a.points, device=engine.device_info()["name"], rays_per_block=engine.SOLAR_JAC_RAYS, cases=[])
    for name, s in shapes(a.points).items():
        Q = s["q_pass"]()
        n_par, n_rows, n_k = s["n_par"], Q.shape[1], s["n_k"]
        out = torch.empty((Q.shape[0], n_par, a.points), dtype=torch.float64, device="cuda")
        dUd = torch.as_tensor(s["dU"].reshape(n_par, n_rows, n_k), device="cuda")
        A2 = s["A"].view(n_k, a.points)
        off, ch = engine.solar_jacobian_chunk_lists(s["dU"])
        fused = lambda: engine.solar_attenuation_jacobian(s["A"], s["dU"], Q, out=out)
        comp = lambda: composed(A2, dUd, Q)
        rep = [(median_ms(fused), median_ms(comp), median_ms(s["q_pass"])) for _ in range(3)]     # alternating rounds
        ref = comp()
        diff = float((fused() - ref).abs().max() / ref.abs().max())
        case = dict(shape=name, n_rays=int(Q.shape[0]), n_rows=int(n_rows), n_k=n_k, n_par=n_par, zero_fraction=float((s["dU"] == 0).mean()),
                    chunks_listed=int(ch.size), chunks_all=int((len(off) - 1) * ((n_k + 3) // 4)), bytes_of_Q=8 * Q.numel(),
                    bytes_written=8 * out.numel(), fused_ms=[r[0] for r in rep], composed_ms=[r[1] for r in rep],
                    q_pass_ms=[r[2] for r in rep], max_rel_difference=diff)
        res["cases"].append(case)
        print("%s: %d rays x %d rows x %d k, %d parameters (%.1f %% zeros, %d of %d chunks listed): fused %s ms, composed %s ms, "
              "Q pass %s ms for %.2f GB; largest relative difference %.1e"
              % (name, case["n_rays"], n_rows, n_k, n_par, 100 * case["zero_fraction"], case["chunks_listed"], case["chunks_all"],
                 np.round(case["fused_ms"], 3), np.round(case["composed_ms"], 3), np.round(case["q_pass_ms"], 3), 1e-9 * case["bytes_of_Q"], diff))
        del Q, out, dUd, ref
    it = [(iteration_ms(False), iteration_ms(True)) for _ in range(3)]
    res["iteration"] = dict(scene="tests/solar_source_cases.solar_twin", off_ms=[r[0] for r in it], on_ms=[r[1] for r in it])
    print("one inversion_state iteration on the tests' sunlit twin: flag off %s ms, on %s ms"
          % (np.round(res["iteration"]["off_ms"], 3), np.round(res["iteration"]["on_ms"], 3)))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
