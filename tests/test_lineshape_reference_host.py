"""The reference of the pressure-shift / self-broadening tests (tests/lineshape_reference.py) pinned to the oracle, the
size of the two effects on the inputs the GPU tests use, and the host-side pieces of the feature.  No GPU."""
import os

import numpy as np
import pytest

import lineshape_reference as R

HERE = os.path.dirname(os.path.abspath(__file__))
PRESS = np.array([1450.0, 300.0, 10.0, 0.01])


@pytest.fixture(scope="module")
def case(oracle):
    from spectrobot_amd import synthetic as syn
    grid = syn.make_grid(2975.0, 5e-4, 20000)
    L = syn.make_lines(200, grid, config_id=7, n_levels=12)
    atm = syn.make_atmosphere(4, 12)
    q = oracle.partition_sums(6, 1, atm["temps"])
    rng = np.random.default_rng(11)
    n = len(L["freq"])
    c = dict(grid=grid, L=L, temps=atm["temps"], press=PRESS, tvib=atm["tvib"], q=q,
             p_shift=rng.uniform(-0.012, 0.002, n), self_broad=rng.uniform(0.05, 0.12, n), p_self=0.05 * PRESS)
    c["plain"] = R.abscoeff_layers(L, syn.CH4_MM, syn.CH4_LEVEL_ENERGIES, c["temps"], PRESS, q, c["tvib"], grid)
    return c


def test_reference_without_the_data_is_the_oracle_bit_for_bit(case, oracle):
    from spectrobot_amd import synthetic as syn
    abo, emo = oracle.abscoeff_layers(case["L"], syn.CH4_MM, syn.CH4_LEVEL_ENERGIES, case["temps"], case["press"], case["q"],
                                      case["tvib"], case["grid"], mode=1, n_threads=4)
    ab, em = case["plain"]
    assert np.array_equal(ab, abo) and np.array_equal(em, emo)
    # zero arrays and no self pressure: the same expressions with exact zeros
    n = len(case["L"]["freq"])
    ab0, em0 = R.abscoeff_layers(case["L"], syn.CH4_MM, syn.CH4_LEVEL_ENERGIES, case["temps"][:2], case["press"][:2], case["q"][:2],
                                 case["tvib"][:, :2], case["grid"], p_shift=np.zeros(n), self_broad=np.zeros(n))
    assert np.array_equal(ab0, abo[:2]) and np.array_equal(em0, emo[:2])


def test_both_effects_are_far_above_the_parity_tolerance(case):
    """At P >= 10 hPa the shift and the self-broadening each move the emission coefficient by more than 1e-3 of the
    layer's largest value: seven orders above the 1e-10 of the parity tests, so the GPU tests' inputs tell the feature
    from its absence."""
    from spectrobot_amd import synthetic as syn
    args = (case["L"], syn.CH4_MM, syn.CH4_LEVEL_ENERGIES, case["temps"], case["press"], case["q"], case["tvib"], case["grid"])
    _, em = case["plain"]
    _, em_s = R.abscoeff_layers(*args, p_shift=case["p_shift"])
    _, em_b = R.abscoeff_layers(*args, self_broad=case["self_broad"], p_self=case["p_self"])
    e_s, e_b = R.effect(em_s, em), R.effect(em_b, em)
    print("effect of shift per layer:", e_s, " of self-broadening:", e_b)
    dense = case["press"] >= 10.0
    assert np.all(e_s[dense] > 1e-3) and np.all(e_b[dense] > 1e-3)
    assert e_s[-1] < 1e-3 and e_b[-1] < 1e-3   # and both fade with the pressure
    # self_broad without a self pressure changes nothing
    _, em_n = R.abscoeff_layers(case["L"], syn.CH4_MM, syn.CH4_LEVEL_ENERGIES, case["temps"][:1], case["press"][:1], case["q"][:1],
                                case["tvib"][:, :1], case["grid"], self_broad=case["self_broad"])
    assert np.array_equal(em_n, em[:1])


def test_new_symbols_and_abi_version():
    from spectrobot_amd import _lib
    assert "sr_lineset_set_line_shape" in _lib.SYMBOLS and "sr_lineset_set_self_pressure" in _lib.SYMBOLS
    assert _lib.lib.sr_abi_version() == 1
    hdr = open(os.path.join(os.path.dirname(HERE), "include", "spectrobot_hip.h")).read()
    assert "int sr_lineset_set_line_shape(" in hdr and "int sr_lineset_set_self_pressure(" in hdr


def test_line_shape_of_hitran_sample(golden):
    from spectrobot_amd import spect_classes as spcl
    g = golden("hitran_sample")
    lines = spcl.read_line_database(os.path.join(HERE, "golden", "hitran_sample.par"))
    p_shift, self_broad = spcl.line_shape_of(lines)
    assert p_shift.dtype == np.float64 and self_broad.dtype == np.float64
    assert np.array_equal(p_shift, g["P_shift"]) and np.array_equal(self_broad, g["Self_broad"])
    assert np.any(p_shift != 0.0) and np.all(self_broad > 0.0)
    soa = spcl.lines_to_soa(lines)
    assert "p_shift" not in soa and len(soa["freq"]) == p_shift.size   # the line arrays of the engine are unchanged
