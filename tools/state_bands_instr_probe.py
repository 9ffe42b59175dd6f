#!/usr/bin/env python3
"""What the two instrument rows (band centre, ILS width) cost in the fused state call, on the shapes of
tools/state_bands_probe.py -- 18 pixels x 3 lines of sight, 1e5 points, HCN + non-LTE CH4 on the level-factored route --
three routes to one iteration's band values, Jacobian rows and field of view:
  fused_instr: LevelFactored.state_bands(instrument=True) (sr_limb_rays_state_bands_instr_dev): one call, the two
               instrument rows from the band epilogue, no hi-res spectrum;
  fused:       the same call without them (sr_limb_rays_state_bands_dev): the parent's call;
  composed:    LevelFactored.state_jacobian (rad and jac written) -> engine.hires_to_lowres_instrument on rad (the value
               and the two instrument rows) and engine.hires_to_lowres on the flattened jac -> smm.fov_closed_form.
Cases: "mixed" = 7 VMR nodes + 10 Tvib nodes with 14 and with 37 bands; "rows20" = 20 kinetic-temperature nodes, 14 bands.
HIP events around blocks of calls (about half a second each; every call ends in a stream synchronise), the routes
alternated A B C A B C ... in one process after a warm-up of every shape; per route the median over the blocks of the time
per call and the run-to-run spread (largest - smallest block).  N=<points>, LAYERS=<layers>, BLOCKS=<blocks per route> (7),
CASES=<comma-separated case names> for other sizes.  Prints one JSON line per case and a last line with the medians."""
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
import bench_configs as bc  # noqa: E402
from spectrobot_amd import engine, synthetic as syn, spect_main_module as smm  # noqa: E402

engine.set_device(0)
n = int(os.environ.get("N", "100000"))
n_layers = int(os.environ.get("LAYERS", "55"))
n_blocks = int(os.environ.get("BLOCKS", "7"))
n_pix = 18
grid = syn.make_grid(3290.0, 5e-4, n)
atm = syn.make_atmosphere(n_layers, 12)
z, temps, press = atm["z"], atm["temps"], atm["press"]
span = z[-1] - z[0]
Lc = syn.make_lines(max(n // 8, 200), grid, config_id=4, n_levels=12)
Lh = syn.make_lines(max(n // 40, 50), grid, config_id=5, n_levels=6)
Lh["a_coeff"] = Lh["a_coeff"] * 30.0
ls_c = engine.LineSet(Lc, grid, 6, 1, syn.CH4_MM, syn.CH4_LEVEL_ENERGIES)
ls_h = engine.LineSet(Lh, grid, 23, 1, bc.HCN_MM, bc.HCN_LEVEL_ENERGIES)
step_row = np.arange(n_layers, dtype=np.int32)
lf = engine.LevelFactored(ls_c, temps, press, dT=0.05)
co_c, dco_c = lf.steps(step_row, tvib=atm["tvib"], derivative=True)
co_h = ls_h.abscoeff_layers(temps, press)
_, dco_h = engine.coefficients_dT(ls_h, temps, press, scheme="forward", coeffs=co_h)
coeffs, dcoeffs = engine.gas_stack([co_h, co_c]), engine.gas_stack([dco_h, dco_c])      # CH4 is gas 1
GAS = 1
vmr = [np.full(n_layers, 2e-6), np.full(n_layers, 1.48e-4)]
tang = [z[0] + (0.06 + 0.045 * i) * span + d * 0.02 * span for i in range(n_pix) for d in (-1.0, 0.0, 1.0)]
Lr = syn.limb_los(z, syn.number_density(press, temps), vmr, tang)
los = engine.LimbLOS(Lr["seg_off"], Lr["seg_layer"], Lr["pt_off"], Lr["x"], Lr["nd"], Lr["vmr"],
                     col_scale=[bc.HCN_ISO_RATIO, syn.CH4_ISO_RATIO])
rots = [10.0 * (i % 3) for i in range(n_pix)]
fov_fac = engine.fov_factors(rots)
nodes = lambda fr: [z[0] + f * span for f in fr]
par_w_col = np.concatenate([engine.level_node_weights(nodes((0.06, 0.3, 0.55, 0.85)), Lr["alt"]),
                            engine.level_node_weights(nodes((0.1, 0.45, 0.8)), Lr["alt"])])
par_gas = np.array([1, 1, 1, 1, 0, 0, 0], np.int32)
W5 = engine.level_node_weights(nodes((0.1, 0.3, 0.5, 0.7, 0.9)), z)
par_level, par_w_lev = np.repeat(np.array([5, 2], np.int32), 5), np.concatenate([W5, W5])
W20 = engine.level_node_weights(list(np.linspace(z[0] + 0.03 * span, z[-1] - 0.03 * span, 20)), z)
lam_lo, lam_hi = 1e7 / grid[-1], 1e7 / grid[0]
margin = min(1.2, 0.1 * (lam_hi - lam_lo))
bands14 = (np.linspace(lam_lo + margin, lam_hi - margin, 14), np.full(14, min(1.1, 0.1 * (lam_hi - lam_lo))))
bands37 = (np.linspace(lam_lo + margin, lam_hi - margin, 37), np.full(37, min(1.1, 0.1 * (lam_hi - lam_lo))))
MIXED = dict(par_level=par_level, par_w_level=par_w_lev, kw=dict(par_gas=par_gas, par_w_col=par_w_col, gas=GAS))
ROWS20 = dict(par_level=np.zeros(0, np.int32), par_w_level=None, kw=dict(gas=GAS, dcoeffs=dcoeffs, par_w_temp=W20))


def composed(par, bands):
    rad, jac = lf.state_jacobian(coeffs, los, step_row, atm["tvib"], par["par_level"], par["par_w_level"], **par["kw"])
    n_los, n_par = jac.shape[0], jac.shape[1]
    three = engine.hires_to_lowres_instrument(rad, grid, bands[0], bands[1])
    dlow = engine.hires_to_lowres(jac.view(n_los * n_par, -1), grid, bands[0], bands[1]).reshape(n_los, n_par, -1)
    both = np.concatenate([three[0][:, None, :], dlow, three[1][:, None, :], three[2][:, None, :]], axis=1)
    return smm.fov_closed_form(both[0::3], both[1::3], both[2::3], rots)


def fused(par, bands, instrument=False):
    return lf.state_bands(coeffs, los, step_row, atm["tvib"], par["par_level"], par["par_w_level"], grid, bands[0], bands[1],
                          fov=fov_fac, instrument=instrument, **par["kw"])


def block_ms(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / reps


summary = {}
wanted = [c for c in os.environ.get("CASES", "").split(",") if c]
for case, par, bands in (("mixed_14_bands", MIXED, bands14), ("mixed_37_bands", MIXED, bands37), ("rows20_14_bands", ROWS20, bands14)):
    if wanted and case not in wanted:
        continue
    routes = (("fused_instr", lambda: fused(par, bands, True)), ("fused", lambda: fused(par, bands)), ("composed", lambda: composed(par, bands)))
    u, f, p = composed(par, bands), fused(par, bands, True), fused(par, bands)
    assert np.array_equal(f[:, :p.shape[1]], p)       # the parent's rows, bit for bit
    scale = np.max(np.abs(u), axis=(0, 2), keepdims=True)
    agree = float(np.max(np.abs(f - u) / np.where(scale > 0, scale, 1.0)))
    for _, fn in routes:                              # warm-up of every shape
        block_ms(fn, 3)
    reps = {name: max(3, int(np.ceil(500.0 / block_ms(fn, 3)))) for name, fn in routes}
    res = {name: [] for name, _ in routes}
    for _ in range(n_blocks):                         # A B C A B C ...
        for name, fn in routes:
            res[name].append(round(block_ms(fn, reps[name]), 4))
    med = {k: float(np.median(v)) for k, v in res.items()}
    spread = {k: round(max(v) - min(v), 4) for k, v in res.items()}
    n_par = p.shape[1] - 1
    extra = med["fused_instr"] - med["fused"]
    summary[case] = dict(fused_instr_ms=round(med["fused_instr"], 4), fused_ms=round(med["fused"], 4), composed_ms=round(med["composed"], 4),
                         instrument_rows_ms=round(extra, 4), instrument_rows_percent_of_fused=round(100.0 * extra / med["fused"], 2),
                         composed_over_fused_instr=round(med["composed"] / med["fused_instr"], 3))
    print(json.dumps(dict(case=case, n_pts=n, n_layers=n_layers, n_rays=los.n_rays, n_par=n_par, n_bands=int(bands[0].size),
                          blocks_ms=res, median_ms={k: round(v, 4) for k, v in med.items()}, spread_ms=spread,
                          calls_per_block=reps, instrument_rows_ms=round(extra, 4),
                          instrument_rows_percent_of_fused=round(100.0 * extra / med["fused"], 2),
                          instrument_rows_in_spreads=round(extra / max(spread["fused_instr"], spread["fused"], 1e-9), 1),
                          fused_vs_composed_row_err=agree, device=engine.device_info()["name"])), flush=True)
print(json.dumps(dict(summary=summary)))
