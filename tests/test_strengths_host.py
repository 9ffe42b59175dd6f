"""Line-strength family of spect_classes on the host, against the reference's own outputs
(tests/golden/line_strengths.npz, written by tests/golden/make_golden_strengths.py), and the C-ABI surface of the
device entry points (no GPU needed)."""
import os
import re

import numpy as np
import pytest

from spectrobot_amd import _lib
from spectrobot_amd import spect_base_module as sbm
from spectrobot_amd import spect_classes as sc

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
TOL = 1e-13


@pytest.fixture(scope="module")
def fx():
    return dict(np.load(os.path.join(HERE, "golden", "line_strengths.npz")))


def make_lines(fx):
    """SpectLine objects of the fixture's lines and the iso-molecule their level labels link to."""
    iso = sbm.IsoMolec(int(fx["mol"]), int(fx["iso"]), float(fx["mm"]))
    for i, e in enumerate(fx["level_energies"]):
        iso.add_level("L%02d" % i, e)
    lines = []
    for i in range(len(fx["freq"])):
        up = "L%02d" % fx["lev_up"][i] if fx["lev_up"][i] >= 0 else "??"
        lo = "L%02d" % fx["lev_lo"][i] if fx["lev_lo"][i] >= 0 else "??"
        lines.append(sc.SpectLine(dict(Mol=int(fx["mol"]), Iso=int(fx["iso"]), Freq=float(fx["freq"][i]),
                                       Strength=float(fx["strength"][i]), A_coeff=float(fx["a_coeff"][i]),
                                       Air_broad=float(fx["air_broad"][i]), Self_broad=0.0,
                                       E_lower=float(fx["e_lower"][i]), T_dep_broad=float(fx["t_dep_broad"][i]),
                                       P_shift=0.0, Up_lev_str=up, Lo_lev_str=lo, Q_num_up="", Q_num_lo="",
                                       g_up=float(fx["g_up"][i]), g_lo=float(fx["g_lo"][i]))))
    return lines, iso


def rel(a, b):
    a, b = np.asarray(a, dtype=float), np.asarray(b, dtype=float)
    scale = np.where(b != 0.0, np.abs(b), 1.0)
    return float(np.max(np.abs(a - b) / scale))


def test_spectline_strengths_match_reference(fx):
    lines, iso = make_lines(fx)
    n_linked = int(fx["n_linked"])
    nc, nt, n = fx["ein_ab"].shape
    got = {k: np.zeros((nc, nt, n)) for k in ("ein_ab", "ein_em", "str_ab", "str_em", "nonlte")}
    for i, l in enumerate(lines):
        linked = i < n_linked
        for c in range(nc):
            for k, T in enumerate(fx["temps"]):
                tl, tu = fx["tvib_lo"][c, k, i], fx["tvib_up"][c, k, i]
                got["ein_ab"][c, k, i], got["ein_em"][c, k, i] = l.CalcStrength_from_Einstein(
                    T, iso_ab=float(fx["iso_ab"]), isomolec=iso if linked else None, T_vib_lower=tl, T_vib_upper=tu)
                got["str_ab"][c, k, i], got["str_em"][c, k, i] = l.CalcStrength_from_Strength(
                    T, iso_ab=float(fx["iso_ab"]), T_vib_lower=tl, T_vib_upper=tu)
                got["nonlte"][c, k, i] = l.CalcStrength_nonLTE(T, tl, tu) if l.A_coeff != 0.0 else 0.0
    for k, v in got.items():
        assert rel(v, fx[k]) <= TOL, k
    cs = np.array([[l.CalcStrength(T) for l in lines] for T in fx["temps"]])
    assert rel(cs, fx["calc_strength"]) <= TOL
    a = np.array([l.calc_A_coeff_from_strength(iso_ab=float(fx["iso_ab"])) for l in lines])
    assert rel(a, fx["a_from_strength"]) <= TOL
    # the A = 0 line: no Einstein strength, a HITRAN one
    assert fx["a_coeff"][7] == 0.0 and np.all(got["ein_ab"][:, :, 7] == 0.0) and np.all(got["str_ab"][:, :, 7] != 0.0)


def test_module_functions_match_reference(fx):
    mol, iso = int(fx["mol"]), int(fx["iso"])
    temps, q_t = fx["temps"], fx["q_t"]
    assert rel([sc.CalcPartitionSum(mol, iso, temp=T) for T in temps], q_t) <= TOL
    at_t = np.array([[sc.CalcStrength_at_T(mol, iso, s, w, e, T, T_ref=float(fx["t_ref2"]))
                      for s, w, e in zip(fx["strength"], fx["freq"], fx["e_lower"])] for T in temps])
    assert rel(at_t, fx["calc_strength_at_t"]) <= TOL
    assert rel(sc.Einstein_B21_to_A(fx["b21"], fx["freq"]), fx["b21_to_a"]) <= TOL
    nl = np.array([sc.Einstein_A_to_LineStrength_nonLTE(fx["a_coeff"], fx["freq"], fx["e_lower"], 0.9 * T, 1.3 * T,
                                                        fx["g_lo"], fx["g_up"], q, iso_ab=float(fx["iso_ab"]))
                   for T, q in zip(temps, q_t)])
    assert rel(nl, fx["nonlte_fn"]) <= TOL
    pop = np.array([sc.Boltz_pop_at_T(fx["e_lower"], T, fx["g_lo"], q) for T, q in zip(temps, q_t)])
    assert rel(pop, fx["boltz_pop"]) <= TOL
    al = np.array([sc.alpha_nlte(fx["freq"], T, fx["r1"], fx["r2"]) for T in temps])
    assert rel(al, fx["alpha_nlte"]) <= TOL
    assert rel([sc.BB(T, fx["freq"]) for T in temps], fx["bb"]) <= TOL
    assert rel([sc.BB_erg(T, fx["freq"]) for T in temps], fx["bb_erg"]) <= TOL


def test_vibtemp_to_ratio():
    assert sbm.vibtemp_to_ratio(0.0, 150.0, 100.0) == 1.0
    assert sbm.vibtemp_to_ratio(1311.0, 100.0, 100.0) == 1.0
    r = sbm.vibtemp_to_ratio(np.array([1311.0, 3019.0]), 180.0, 150.0)
    want = np.exp(-sc.c2 * np.array([1311.0, 3019.0]) * (1 / 180.0 - 1 / 150.0))
    assert np.max(np.abs(r / want - 1)) < 1e-13


def test_a_coeff_round_trip(fx):
    """calc_A_coeff_from_strength inverts Einstein_A_to_LineStrength_hitran at 296 K."""
    lines, _ = make_lines(fx)
    mol, iso, iso_ab = int(fx["mol"]), int(fx["iso"]), float(fx["iso_ab"])
    q296 = sc.CalcPartitionSum(mol, iso, temp=296.0)
    worst = 0.0
    for l in lines:
        if l.A_coeff == 0.0:
            continue
        l.Strength = sc.Einstein_A_to_LineStrength_hitran(l.A_coeff, l.Freq, 296.0, q296, l.g_up, l.E_lower, iso_ab)
        a = l.calc_A_coeff_from_strength(iso_ab=iso_ab, Q_part=q296)
        worst = max(worst, abs(a / l.A_coeff - 1))
        a_old = l.A_coeff
        assert l.calc_A_coeff_from_strength(iso_ab=iso_ab, Q_part=q296, set_attr=True) == a and l.A_coeff == a
        l.A_coeff = a_old
    assert worst <= TOL


def test_strengths_of_and_soa_unchanged(fx):
    lines, iso = make_lines(fx)
    s = sc.strengths_of(lines)
    assert s.dtype == np.float64 and np.array_equal(s, fx["strength"])
    assert "strength" not in sc.lines_to_soa(lines, iso)


def test_abi_surface():
    hdr = open(os.path.join(ROOT, "include", "spectrobot_hip.h")).read()
    for name in ("sr_lineset_set_strengths", "sr_line_strengths_dev", "sr_abscoeff_layers_from_strengths_dev"):
        assert re.search(r"\bint %s\(" % name, hdr), name
        assert name in _lib.SYMBOLS, name
        assert hasattr(_lib.lib, name)
    assert re.search(r"SR_STRENGTH_EINSTEIN = 0, SR_STRENGTH_HITRAN = 1", hdr)
    assert (_lib.SR_STRENGTH_EINSTEIN, _lib.SR_STRENGTH_HITRAN) == (0, 1)
    assert _lib.lib.sr_abi_version() == 1
