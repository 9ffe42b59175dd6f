#!/usr/bin/env python3
"""Twin experiment: recover the vibrational-temperature profile of one excited CH4 level from limb spectra with the
level-table Jacobian (LevelFactored.tvib_jacobian) -- the synthetic CH4 limb case of examples/ch4_limb.py at reduced
size.

  truth      Tvib of level 5 = the atmosphere's profile + a smooth bump of 6 K around 420 km
  "observed" the band spectra of 7 limb rays through the truth, plus noise
  retrieved  6 triangular nodes of an offset profile, Levenberg-Marquardt steps of the optimal-estimation algebra
             (spect_main_module.inversion_algebra_arrays) with d rad / d Tvib-node from the resident level tables: no
             finite differences, no second table build.

Prints chi square and the largest profile error per iteration.  Needs an MI355X:  python examples/retrieve_tvib.py
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from spectrobot_amd import engine, synthetic as syn                      # noqa: E402
from spectrobot_amd import spect_main_module as smm                       # noqa: E402

LEVEL = 5          # 2830 cm-1: the level these rays see best


def main():
    engine.set_device(0)
    n_layers = 40
    grid = syn.make_grid(2990.0, 5e-4, 40000)
    ls = engine.LineSet(syn.make_lines(4000, grid, config_id=3, n_levels=12), grid, 6, 1, syn.CH4_MM,
                        syn.CH4_LEVEL_ENERGIES)
    atm = syn.make_atmosphere(n_layers, 12)
    z = atm["z"]
    Lr = syn.limb_los(z, syn.number_density(atm["press"], atm["temps"]), [np.full(n_layers, 0.0148)],
                      180.0 + 70.0 * np.arange(7))
    los = engine.LimbLOS(Lr["seg_off"], Lr["seg_layer"], Lr["pt_off"], Lr["x"], Lr["nd"], Lr["vmr"],
                         col_scale=[syn.CH4_ISO_RATIO])
    lf = engine.LevelFactored(ls, atm["temps"], atm["press"])           # the pair tables, once
    rows = np.arange(n_layers, dtype=np.int32)
    bands = np.linspace(1e7 / grid[-1] + 1.0, 1e7 / grid[0] - 1.0, 10)
    widths = np.full(10, 1.1)

    nodes = np.linspace(200.0, 800.0, 6)                               # inside the tangent heights' reach
    W = engine.level_node_weights(nodes, z)                            # [6, n_layers]
    par_level = np.full(len(nodes), LEVEL, np.int32)

    def tvib_of(x):
        tv = atm["tvib"].copy()
        tv[LEVEL] += x @ W
        return tv

    def forward(tv, jacobian=False):
        co = lf.steps(rows, tvib=tv)
        if not jacobian:
            return engine.hires_to_lowres(engine.limb_rays(co, los), grid, bands, widths).ravel(), None
        rad, jac = lf.tvib_jacobian(co, los, rows, tv, par_level, W)
        y = engine.hires_to_lowres(rad, grid, bands, widths).ravel()
        K = engine.hires_to_lowres(jac, grid, bands, widths).reshape(los.n_rays, len(nodes), -1)
        return y, K.transpose(0, 2, 1).reshape(-1, len(nodes))         # [n_obs, n_par]

    bump = 6.0 * np.exp(-0.5 * ((z - 420.0) / 130.0) ** 2)
    tv_true = atm["tvib"].copy()
    tv_true[LEVEL] += bump
    y_true, _ = forward(tv_true)
    rng = np.random.default_rng(7)
    noise = np.full(y_true.size, 2e-4 * np.abs(y_true).max())
    obs = y_true + noise * rng.standard_normal(y_true.size)

    bs = smm.BayesSet(tag="Tvib offset of level %d" % LEVEL)
    bs.add_set(smm.LinearProfile_1D_new("tvib", z, list(nodes), np.zeros(len(nodes)), np.full(len(nodes), 4.0)))
    for p in bs.params():
        p.constrain_positive = False                                   # an offset may have either sign
    inside = (z >= nodes[0]) & (z <= nodes[-1])
    chis = []
    for it in range(8):
        x = bs.param_vector()
        y, K = forward(tvib_of(x), jacobian=True)
        chis.append(float(np.sum(((obs - y) / noise) ** 2) / (obs.size - len(nodes))))
        print("iteration %d: chi square %.3f, largest profile error %.2f K" % (it, chis[-1], np.abs(x @ W - bump)[inside].max()))
        smm.inversion_algebra_arrays(K, obs, y, noise, bs, lambda_LM=0.1)
    x = bs.param_vector()
    y, _ = forward(tvib_of(x))
    chis.append(float(np.sum(((obs - y) / noise) ** 2) / (obs.size - len(nodes))))
    print("final:       chi square %.3f, largest profile error %.2f K (bump of %.1f K)"
          % (chis[-1], np.abs(x @ W - bump)[inside].max(), bump.max()))
    assert chis[-1] < chis[0], "chi square did not fall"


if __name__ == "__main__":
    main()
