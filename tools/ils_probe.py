#!/usr/bin/env python3
"""What building the weight table costs under the Gaussian and under a tabulated line shape (engine.ILS), on the shapes of a
configs[4] iteration's instrument step: 1e5 grid points, 14 bands, 144 spectra.  Routes through
engine.hires_to_lowres (and, with the prefix instr_, hires_to_lowres_instrument: three tables), each call ending in a
stream synchronise:
  cached:                 the Gaussian with the key unchanged -- no weights kernel, the apply and sum kernels and the copy back;
  gauss_rebuild:          the Gaussian with n_sigma alternating between two values a rounding apart -- the key changes with
                          every call: the bands' upload and sr_lowres_weights_kernel on top;
  table_rebuild:          one table for all bands passed as ils= -- every binding is a new generation, so every call
                          rebuilds: the bands' and the table's upload and sr_lowres_weights_tab_kernel on top of `cached`;
  table_per_band_rebuild: the same with one table per band.
The differences to `cached` are what a key change costs; a table is rebuilt by every call that passes ils= (the wrapper
binds and unbinds), a caller that binds once through sr_set_ils pays it once per key change as with the Gaussian.
Wall-clock time around blocks of calls (about a quarter of a second each), the routes alternated A B C A B C ... in one
process after a warm-up of every route; per route the median over the blocks of the time per call and the run-to-run
spread (largest - smallest block).  N=<points>, BANDS=<bands>, SPECTRA=<spectra>, BLOCKS=<blocks per route> (7).
Writes profiles/ils_probe.json and prints it."""
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
from spectrobot_amd import engine, synthetic as syn  # noqa: E402

engine.set_device(0)
n = int(os.environ.get("N", "100000"))
n_bands = int(os.environ.get("BANDS", "14"))
n_spec = int(os.environ.get("SPECTRA", "144"))
n_blocks = int(os.environ.get("BLOCKS", "7"))
grid = syn.make_grid(3290.0, 5e-4, n)
lam_lo, lam_hi = 1e7 / grid[-1], 1e7 / grid[0]
width = min(1.1, 0.02 * (lam_hi - lam_lo))
centers, widths = np.linspace(lam_lo + 6 * width, lam_hi - 6 * width, n_bands), np.full(n_bands, width)
rad = torch.rand((n_spec, n), dtype=torch.float64, device="cuda")
ils = engine.ILS.from_function(lambda t: np.exp(-0.5 * t * t) * (1.0 + 0.6 * np.tanh(1.5 * t)), -5.0, 5.0, 641)
ils_b = engine.ILS(-5.0, 5.0, np.tile(ils.phi, (n_bands, 1)), normalize=False)
flip = [0]


def n_sigma():
    flip[0] ^= 1
    return 5.0 if flip[0] else 5.000000000000001


ROUTES = {
    "cached": lambda: engine.hires_to_lowres(rad, grid, centers, widths),
    "gauss_rebuild": lambda: engine.hires_to_lowres(rad, grid, centers, widths, n_sigma=n_sigma()),
    "table_rebuild": lambda: engine.hires_to_lowres(rad, grid, centers, widths, ils=ils),
    "table_per_band_rebuild": lambda: engine.hires_to_lowres(rad, grid, centers, widths, ils=ils_b),
    "instr_cached": lambda: engine.hires_to_lowres_instrument(rad, grid, centers, widths),
    "instr_gauss_rebuild": lambda: engine.hires_to_lowres_instrument(rad, grid, centers, widths, n_sigma=n_sigma()),
    "instr_table_rebuild": lambda: engine.hires_to_lowres_instrument(rad, grid, centers, widths, ils=ils),
}


def block(fn, n_calls):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(n_calls):
        fn()
    return (time.perf_counter() - t0) / n_calls


def main():
    calls = {}
    for name, fn in ROUTES.items():                     # warm-up, and the block length for about a quarter of a second
        for _ in range(3):
            fn()
        calls[name] = max(5, int(0.25 / max(block(fn, 5), 1e-6)))
    times = {name: [] for name in ROUTES}
    for _ in range(n_blocks):
        for name, fn in ROUTES.items():
            if name in ("cached", "instr_cached"):
                fn()                                    # (the call before left another key behind: put this route's back)
            times[name].append(block(fn, calls[name]))
    out = {"shape": {"n_pts": n, "n_bands": n_bands, "n_spectra": n_spec, "n_tab": ils.n_tab, "blocks": n_blocks},
           "device": engine.device_info().get("name"), "unit": "us per call (wall clock, every call synchronises)", "routes": {}}
    for name, t in times.items():
        t = 1e6 * np.array(t)
        out["routes"][name] = {"median": round(float(np.median(t)), 2), "spread": round(float(t.max() - t.min()), 2), "calls_per_block": calls[name]}
    med = lambda k: out["routes"][k]["median"]
    out["key_change_costs_us"] = {"gaussian": round(med("gauss_rebuild") - med("cached"), 2),
                                 "table": round(med("table_rebuild") - med("cached"), 2),
                                 "table_per_band": round(med("table_per_band_rebuild") - med("cached"), 2),
                                 "instr_gaussian": round(med("instr_gauss_rebuild") - med("instr_cached"), 2),
                                 "instr_table": round(med("instr_table_rebuild") - med("instr_cached"), 2)}
    out["note"] = ("differences of medians: the bands' (and table's) upload plus the weights kernel; information, not an acceptance "
                   "criterion")
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "ils_probe.json")
    if os.environ.get("ILS_PROBE_OUT"):
        path = os.environ["ILS_PROBE_OUT"]
    with open(path, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
