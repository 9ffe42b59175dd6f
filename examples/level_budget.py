#!/usr/bin/env python3
"""Which vibrational level makes the band, and where along the path: the radiance budget of the synthetic CH4 limb case
of examples/retrieve_tvib.py (LevelFactored.level_radiances -> engine.limb_rays_parts: every part in one pass over the
rays, from the resident level tables).

Per ray it prints the band integral of the radiance every level emits (as a share of the ray's band integral) and the
altitude band -- below 350 km, 350 to 550 km, above -- that share comes from.  The level with the largest share is the
one a Tvib retrieval of these rays should start with.  Needs an MI355X:  python examples/level_budget.py
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from spectrobot_amd import engine, synthetic as syn                      # noqa: E402

BANDS = [(-np.inf, 350.0), (350.0, 550.0), (550.0, np.inf)]            # km


def main():
    engine.set_device(0)
    n_layers, n_lev = 40, 12
    grid = syn.make_grid(2990.0, 5e-4, 40000)
    ls = engine.LineSet(syn.make_lines(4000, grid, config_id=3, n_levels=n_lev), grid, 6, 1, syn.CH4_MM,
                        syn.CH4_LEVEL_ENERGIES)
    atm = syn.make_atmosphere(n_layers, n_lev)
    z = atm["z"]
    Lr = syn.limb_los(z, syn.number_density(atm["press"], atm["temps"]), [np.full(n_layers, 0.0148)],
                      180.0 + 70.0 * np.arange(7))
    los = engine.LimbLOS(Lr["seg_off"], Lr["seg_layer"], Lr["pt_off"], Lr["x"], Lr["nd"], Lr["vmr"],
                         col_scale=[syn.CH4_ISO_RATIO])
    lf = engine.LevelFactored(ls, atm["temps"], atm["press"])           # the pair tables, once
    rows = np.arange(n_layers, dtype=np.int32)
    co = lf.steps(rows, tvib=atm["tvib"])
    step = grid[1] - grid[0]
    integral = lambda t: t.sum(dim=-1).cpu().numpy() * step             # band integral over the whole grid

    # every level and the gas
    rad, parts, labels = lf.level_radiances(co, los, rows, atm["tvib"])
    total = integral(rad)                                               # [n_rays]
    share = integral(parts) / total[:, None]                            # [n_rays, 12 levels + gas + background]
    # every level in three altitude bands: 36 parts in the same pass
    masks = np.array([(z >= lo) & (z < hi) for lo, hi in BANDS], float)
    levels = np.repeat(np.arange(n_lev), len(BANDS))
    _, banded, _ = lf.level_radiances(co, los, rows, atm["tvib"], levels=levels, weights=np.tile(masks, (n_lev, 1)),
                                      gas_parts=False)
    where = integral(banded)[:, :-1].reshape(los.n_rays, n_lev, len(BANDS)) / total[:, None, None]

    for r in range(los.n_rays):
        best = int(np.argmax(share[r, :n_lev]))
        print("ray %d, tangent height %.0f km: levels add up to %.6f of the band integral, gas part %.6f; level %d "
              "(%.0f cm-1) emits %.1f%%" % (r, 180.0 + 70.0 * r, share[r, :n_lev].sum(), share[r, n_lev], best,
                                            syn.CH4_LEVEL_ENERGIES[best], 100.0 * share[r, best]))
        for L in np.argsort(share[r, :n_lev])[::-1][:4]:
            print("    level %2d (%4.0f cm-1): %5.1f%%   below 350 km %5.1f%%, 350-550 km %5.1f%%, above %5.1f%%"
                  % (L, syn.CH4_LEVEL_ENERGIES[L], 100.0 * share[r, L], 100.0 * where[r, L, 0], 100.0 * where[r, L, 1],
                     100.0 * where[r, L, 2]))
    assert np.all(np.abs(share[:, :n_lev].sum(axis=1) - share[:, n_lev]) < 1e-9)
    assert np.all(np.abs(where.sum(axis=2) - share[:, :n_lev]) < 1e-9)


if __name__ == "__main__":
    main()
