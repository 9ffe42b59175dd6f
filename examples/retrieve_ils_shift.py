#!/usr/bin/env python3
"""examples/retrieve_band_shift.py with a MEASURED instrument response: the channels of the instrument are not Gaussian
but an asymmetric, tabulated shape (engine.ILS: knots at reduced offsets (x - centre) / width, cubic Hermite interpolation
between them), given to the scene as LimbScene(..., ils=...).  Every band integral of the forward model and the two
instrument rows of the state Jacobian (d / d band centre, d / d ln width) are then taken with the table -- per iteration
still ONE fused call, no hi-res spectrum written.

  truth      the HCN profile scaled by 1.3, every band centre 0.25 nm off its nominal place, the response 5 % wider
  "observed" the band spectra of 6 limb pixels (three lines of sight each, closed-form field of view) through the truth
             under the tabulated response, plus noise
  retrieved  3 VMR nodes of HCN, the band shift (nm) and the logarithm of the width factor -- once with the table, once
             with a Gaussian of the table's second moment, which is what could be done without it

Prints the chi-square histories and the retrieved states next to the truth.  Needs an MI355X:
python examples/retrieve_ils_shift.py
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from spectrobot_amd import engine, retrieval, synthetic as syn          # noqa: E402
from spectrobot_amd import spect_main_module as smm                     # noqa: E402

HCN_MM, HCN_ISO_RATIO = 27.010899, 0.985114
HCN_LEVEL_ENERGIES = np.array([0., 711.98, 1411.41, 2096.85, 3311.48, 4004.17])


def response():
    """A grating channel with a shoulder on its long-wavelength side: a bell and a weaker, wider one 1.2 widths off."""
    return engine.ILS.from_function(lambda t: np.exp(-0.5 * t * t) + 0.35 * np.exp(-0.5 * ((t - 1.2) / 1.4) ** 2), -6.0, 6.0, 385)


def main():
    engine.set_device(0)
    n_layers = 40
    grid = syn.make_grid(2990.0, 5e-4, 40000)
    atm = syn.make_atmosphere(n_layers, 12)
    z = atm["z"]
    Lh = syn.make_lines(1200, grid, config_id=5, n_levels=6)
    Lh["a_coeff"] = Lh["a_coeff"] * 30.0
    ch4 = retrieval.LevelGas("CH4", engine.LineSet(syn.make_lines(4000, grid, config_id=3, n_levels=12), grid, 6, 1, syn.CH4_MM,
                                                   syn.CH4_LEVEL_ENERGIES), np.full(n_layers, 0.0148), atm["tvib"],
                             syn.CH4_ISO_RATIO)
    hcn = retrieval.Gas("HCN", engine.LineSet(Lh, grid, 23, 1, HCN_MM, HCN_LEVEL_ENERGIES), np.full(n_layers, 2e-6),
                        HCN_ISO_RATIO)
    bands = np.linspace(1e7 / grid[-1] + 1.0, 1e7 / grid[0] - 1.0, 10)
    ils = response()
    # the table's first two moments: what a Gaussian model of this channel would be given
    t = ils.knots()
    trapz = lambda y: float(np.sum(0.5 * (y[1:] + y[:-1]) * np.diff(t)))
    mean = trapz(t * ils.phi[0])
    sigma = np.sqrt(trapz((t - mean) ** 2 * ils.phi[0]))
    print("response table: %d knots on [%g, %g], area %.15f, mean %.3f and sigma %.3f widths" % (ils.n_tab, ils.t_lo, ils.t_hi, ils.area()[0],
                                                                                              mean, sigma))
    width = 0.9
    scene = retrieval.LimbScene(grid, z, atm["temps"], atm["press"], [hcn, ch4], bands, np.full(10, width), ils=ils)
    pixels = [retrieval.LimbPixel(200.0 + 90.0 * i, fov_half=15.0, pixel_rot=10.0 * (i % 3)) for i in range(6)]

    hcn_nodes = [200.0, 450.0, 750.0]
    apr, sig_hcn = np.full(3, 2e-6), np.full(3, 1e-6)
    sig_shift, sig_lnw = 0.5, 0.1
    x_true = np.concatenate([1.3 * apr, [0.25, np.log(1.05)]])

    def bayes(x=None):
        bs = smm.BayesSet(tag="HCN VMR + band shift + response width")
        bs.add_set(smm.LinearProfile_1D_new("HCN", z, hcn_nodes, apr, sig_hcn, first_guess_prof=None if x is None else x[:3]))
        bs.add_set(retrieval.BandCalibration(shift=(0.0, sig_shift) + (() if x is None else (x[3],)),
                                             ln_width=(0.0, sig_lnw) + (() if x is None else (x[4],))))
        return bs

    # the truth into the scene (profile, band centres, widths), its spectra under the table as observations
    retrieval._state_into_gases(scene, bayes(x_true))
    rng = np.random.default_rng(7)
    for pix, y in zip(pixels, retrieval.radtrans(scene, pixels)):
        sig = np.full(y.spectrum.size, 2e-4 * np.abs(y.spectrum).max())
        pix.observation = retrieval.Spectrum(y.spectrum + sig * rng.standard_normal(sig.size), bands)
        pix.noise = retrieval.Spectrum(sig, bands)

    def report(tag, bs):
        x = bs.param_vector()
        print("%s: chi square %s, stopped: %s" % (tag, " -> ".join("%.3f" % c for c in bs.history), bs.stop))
        print("  HCN nodes   retrieved %s  truth %s" % (np.array2string(x[:3], precision=3), np.array2string(x_true[:3], precision=3)))
        print("  band shift  retrieved %.4f nm  truth %.4f nm" % (x[3], x_true[3]))
        print("  width       retrieved x %.4f  truth x %.4f" % (np.exp(x[4]), np.exp(x_true[4])))
        return x

    _, _, _, with_table = retrieval.inversion_state(scene, bayes(), pixels, max_it=10, bands_in_kernel=True)
    x = report("tabulated response", with_table)
    # the same observations under a Gaussian of the table's mean and second moment
    gauss = retrieval.LimbScene(grid, z, atm["temps"], atm["press"], [hcn, ch4], bands + mean * width, np.full(10, sigma * width))
    _, _, _, with_gauss = retrieval.inversion_state(gauss, bayes(), pixels, max_it=10, bands_in_kernel=True)
    xg = report("Gaussian of the same second moment", with_gauss)
    err = lambda v: np.linalg.norm((v[:3] - x_true[:3]) / sig_hcn)
    print("HCN profile error in a-priori sigmas: %.2f with the table, %.2f with the Gaussian" % (err(x), err(xg)))
    assert with_table.history[-1] < with_table.history[0], "chi square did not fall"
    assert abs(x[3] - x_true[3]) < abs(x_true[3]) and abs(x[4] - x_true[4]) < abs(x_true[4])
    assert with_gauss.history[-1] > with_table.history[-1]


if __name__ == "__main__":
    main()
