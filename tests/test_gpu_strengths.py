"""Line strengths on the GPU (sr_line_strengths_dev) and coefficient spectra weighted by them
(sr_abscoeff_layers_from_strengths_dev): against the reference's outputs (tests/golden/line_strengths.npz), against
the G-coefficient route they must reproduce when the intensities come from the Einstein A (the reference author's LTE
check, spect_main_Titan.py:186), against the oracle's line windows, and their refusals.  Run with `pytest -m gpu`."""
import os

import numpy as np
import pytest

from conftest import far_tol, relerr

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def eng():
    import torch
    assert torch.cuda.is_available(), "these tests need the GPU"
    from spectrobot_amd import engine
    engine.set_device(0)
    return engine


@pytest.fixture(scope="module")
def fx():
    return dict(np.load(os.path.join(HERE, "golden", "line_strengths.npz")))


def _np(t):
    return t.cpu().numpy()


def _fx_lines(fx, sel):
    keys = ("freq", "a_coeff", "e_lower", "g_up", "g_lo", "air_broad", "t_dep_broad", "lev_up", "lev_lo")
    return {k: np.ascontiguousarray(fx[k][sel]) for k in keys}


def _s_ref_from_a(sc, L, mol, iso, iso_ab):
    """HITRAN intensities at 296 K that carry the same physics as the Einstein A (fp64, numpy)."""
    q296 = sc.CalcPartitionSum(mol, iso, temp=296.0)
    return sc.Einstein_A_to_LineStrength_hitran(L["a_coeff"], L["freq"], 296.0, q296, L["g_up"], L["e_lower"], iso_ab)


def test_line_strengths_against_reference(eng, fx):
    """Both sources, LTE and three non-LTE cases, linked lines and the 'all' set, against the reference's output."""
    from spectrobot_amd import synthetic as syn
    grid = syn.make_grid(2975.0, 5e-4, 20000)       # most of the fixture's lines lie outside it: outer lines
    temps, iso_ab = fx["temps"], float(fx["iso_ab"])
    n, n_linked = len(fx["freq"]), int(fx["n_linked"])
    linked = np.arange(n) < n_linked
    ls = eng.LineSet(_fx_lines(fx, slice(None)), grid, int(fx["mol"]), int(fx["iso"]), float(fx["mm"]),
                     fx["level_energies"])
    assert ls.n_kept == n_linked
    ls.set_strengths(fx["strength"], t_ref=296.0, iso_ab=iso_ab)
    all_sel = np.arange(n_linked, n)
    lsa = eng.LineSet(_fx_lines(fx, all_sel), grid, int(fx["mol"]), int(fx["iso"]), float(fx["mm"]))
    lsa.set_strengths(fx["strength"][all_sel], iso_ab=iso_ab)
    for c in range(fx["tvib"].shape[0]):
        tvib = None if c == 0 else fx["tvib"][c]
        for source, key in (("einstein", "ein"), ("hitran", "str")):
            ab, em = ls.line_strengths(temps, tvib=tvib, source=source, iso_ab=iso_ab)
            ab, em = _np(ab), _np(em)
            assert ab.shape == (len(temps), n)
            assert np.all(ab[:, ~linked] == 0.0) and np.all(em[:, ~linked] == 0.0)
            assert relerr(ab[:, linked], fx[key + "_ab"][c][:, linked]) <= 1e-12, (c, source)
            assert relerr(em[:, linked], fx[key + "_em"][c][:, linked]) <= 1e-12, (c, source)
            # the 'all' set: E_vib = 0, r = 1 whatever the vibrational temperatures
            ab, em = lsa.line_strengths(temps, source=source, iso_ab=iso_ab)
            assert relerr(_np(ab), fx[key + "_ab"][c][:, all_sel]) <= 1e-12, (c, source)
            assert relerr(_np(em), fx[key + "_em"][c][:, all_sel]) <= 1e-12, (c, source)
    ls.close()
    lsa.close()


def test_per_line_identity_hitran_vs_einstein(eng, fx):
    """s_ref from the A: the HITRAN s_ab IS the Einstein s_ab (LTE and non-LTE); s_em differs by BB_erg's constants."""
    from spectrobot_amd import spect_classes as sc
    from spectrobot_amd import synthetic as syn
    grid = syn.make_grid(2975.0, 5e-4, 20000)
    mol, iso, iso_ab = int(fx["mol"]), int(fx["iso"]), float(fx["iso_ab"])
    L = _fx_lines(fx, slice(None))
    ls = eng.LineSet(L, grid, mol, iso, float(fx["mm"]), fx["level_energies"])
    ls.set_strengths(_s_ref_from_a(sc, L, mol, iso, iso_ab), iso_ab=iso_ab)
    temps = fx["temps"]
    ok = (np.arange(len(L["freq"])) < int(fx["n_linked"])) & (L["a_coeff"] != 0.0)
    bb_factor = np.array([sc.BB_erg(T, L["freq"]) / sc.Calc_BB_single(L["freq"], T) for T in temps])
    assert 0.997 < bb_factor[:, ok].min() and bb_factor[:, ok].max() < 1.0
    for tvib in (None, fx["tvib"][1], fx["tvib"][3]):
        hab, hem = (_np(x) for x in ls.line_strengths(temps, tvib=tvib, source="hitran"))
        eab, eem = (_np(x) for x in ls.line_strengths(temps, tvib=tvib, source="einstein", iso_ab=iso_ab))
        assert relerr(hab[:, ok], eab[:, ok]) <= 1e-12
        assert np.max(np.abs(hem[:, ok] / eem[:, ok] - bb_factor[:, ok])) <= 1e-12
    ls.close()


def _case(n_lines, n_grid, n_layers):
    import bench_configs as bc
    return bc.ch4_case(n_lines, n_grid, n_layers, 12, config_id=2)


def _strength_lineset(eng, grid, L, lev, iso_ab):
    from spectrobot_amd import spect_classes as sc
    from spectrobot_amd import synthetic as syn
    ls = eng.LineSet(L, grid, 6, 1, syn.CH4_MM, lev)
    ls.set_strengths(_s_ref_from_a(sc, L, 6, 1, iso_ab), iso_ab=iso_ab)
    return ls


def _per_layer_close(a, b, tol):
    scale = np.max(np.abs(b), axis=1)
    return float(np.max(np.max(np.abs(a - b), axis=1) / scale)) <= tol


def test_spectrum_identity_full_size(eng):
    """BASELINE configs[1] (1e5 lines x 1e5 points x 80 layers, 12 levels, non-LTE): the strength route's abs is the
    G route's, far-field mode; then the exact mode on a reduced grid."""
    from spectrobot_amd import synthetic as syn
    grid, L, atm, lev = _case(100000, 100000, 80)
    ls = _strength_lineset(eng, grid, L, lev, syn.CH4_ISO_RATIO)
    ab_g, _ = ls.abscoeff_layers(atm["temps"], atm["press"], tvib=atm["tvib"])
    ab_s, em_s = ls.abscoeff_layers_from_strengths(atm["temps"], atm["press"], tvib=atm["tvib"])
    assert _per_layer_close(_np(ab_s), _np(ab_g), 1e-12)
    assert np.all(np.isfinite(_np(em_s))) and float(em_s.min()) >= 0.0
    ls.close()
    grid, L, atm, lev = _case(20000, 20000, 8)
    eng.set_far_field(0)
    try:
        ls = _strength_lineset(eng, grid, L, lev, syn.CH4_ISO_RATIO)
        ab_g, _ = ls.abscoeff_layers(atm["temps"], atm["press"], tvib=atm["tvib"])
        ab_s, _ = ls.abscoeff_layers_from_strengths(atm["temps"], atm["press"], tvib=atm["tvib"])
        assert _per_layer_close(_np(ab_s), _np(ab_g), 1e-12)
        ls.close()
    finally:
        eng.set_far_field(eng.FAR_FIELD_DEFAULT)


def _oracle_strength_spectra(oracle, L, s_ref, grid, temps, press, tvib, lev, mm, iso_ab):
    """abs / emi from the oracle's line windows (closest_grid + make_shape, spect_classes.py:1440-1457, 1113-1120)
    weighted by the host CalcStrength_from_Strength / iso_ab."""
    from spectrobot_amd import spect_classes as sc
    n, half = grid.size, 13010 // 2
    s = grid[1] - grid[0]
    lin_grid = np.arange(-13010 * s / 2, 13010 * s / 2, s)
    ab = np.zeros((len(temps), n))
    em = np.zeros((len(temps), n))
    for i in range(len(L["freq"])):
        lu, ll = int(L["lev_up"][i]), int(L["lev_lo"][i])
        if lu < 0 or ll < 0 or lu == ll:
            continue
        line = sc.SpectLine(dict(Mol=6, Iso=1, Freq=float(L["freq"][i]), Strength=float(s_ref[i]),
                                 E_lower=float(L["e_lower"][i])))
        ic = oracle.closest_grid(grid, L["freq"][i])
        j0 = ic - half
        mlo, mhi = max(0, -j0), min(13010, n - j0)
        for k, (T, P) in enumerate(zip(temps, press)):
            lw = oracle.lorenz_width(T, oracle.convert_to_atm(P), L["t_dep_broad"][i], L["air_broad"][i])
            dw = oracle.doppler_width(T, mm, L["freq"][i])
            shape = oracle.make_shape(lin_grid + grid[ic], L["freq"][i], lw, dw)
            sab, sem = line.CalcStrength_from_Strength(T, T_vib_lower=tvib[ll, k], T_vib_upper=tvib[lu, k],
                                                       E_vib_lo=lev[ll], E_vib_up=lev[lu])
            ab[k, j0 + mlo:j0 + mhi] += shape[mlo:mhi] * (sab / iso_ab)
            em[k, j0 + mlo:j0 + mhi] += shape[mlo:mhi] * (sem / iso_ab)
    return ab, em


@pytest.mark.parametrize("far", [3, 0])
def test_strength_spectra_vs_oracle(eng, oracle, far):
    """~300 lines x 2e4 points x 6 layers, outer lines beyond both grid ends, intensities not tied to the A."""
    from spectrobot_amd import spect_classes as sc
    from spectrobot_amd import synthetic as syn
    grid = syn.make_grid(2975.0, 5e-4, 20000)
    L = syn.make_lines(300, grid, config_id=11, n_levels=12)
    rng = np.random.default_rng(5)
    L["freq"][:6] = grid[0] - 6505 * 5e-4 - rng.uniform(0.01, 4.0, 6)
    L["freq"][-6:] = grid[-1] + 6505 * 5e-4 + rng.uniform(0.01, 4.0, 6)
    order = np.argsort(L["freq"], kind="stable")
    L = {k: np.ascontiguousarray(v[order]) for k, v in L.items()}
    atm = syn.make_atmosphere(6, 12)
    lev = syn.CH4_LEVEL_ENERGIES
    s_ref = _s_ref_from_a(sc, L, 6, 1, syn.CH4_ISO_RATIO) * 10.0 ** rng.uniform(-1.0, 1.0, len(L["freq"]))
    abo, emo = _oracle_strength_spectra(oracle, L, s_ref, grid, atm["temps"], atm["press"], atm["tvib"], lev,
                                        syn.CH4_MM, syn.CH4_ISO_RATIO)
    eng.set_far_field(far)
    try:
        ls = eng.LineSet(L, grid, 6, 1, syn.CH4_MM, lev)
        ls.set_strengths(s_ref, iso_ab=syn.CH4_ISO_RATIO)
        ab, em = ls.abscoeff_layers_from_strengths(atm["temps"], atm["press"], tvib=atm["tvib"])
        assert relerr(_np(ab), abo) < 1e-10
        assert relerr(_np(em), emo) < 1e-10
        ls.close()
    finally:
        eng.set_far_field(eng.FAR_FIELD_DEFAULT)


def test_shards_and_streams(eng):
    import torch
    from spectrobot_amd import synthetic as syn
    grid, L, atm, lev = _case(3000, 30000, 6)
    ls = _strength_lineset(eng, grid, L, lev, 1.0)
    args = (atm["temps"], atm["press"])
    ab, em = (_np(x) for x in ls.abscoeff_layers_from_strengths(*args, tvib=atm["tvib"]))
    for lo, hi in ((0, 13000), (13000, 30000)):
        a, e = (_np(x) for x in ls.abscoeff_layers_from_strengths(*args, tvib=atm["tvib"], g_lo=lo, g_hi=hi))
        assert relerr(a, ab[:, lo:hi]) < far_tol(1e-12)
        assert relerr(e, em[:, lo:hi]) < far_tol(1e-12)
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        a2, e2 = ls.abscoeff_layers_from_strengths(*args, tvib=atm["tvib"])
        sab, sem = ls.line_strengths(atm["temps"], tvib=atm["tvib"], source="hitran")
    s.synchronize()
    assert relerr(_np(a2), ab) <= 1e-14 and relerr(_np(e2), em) <= 1e-14
    sab0, sem0 = ls.line_strengths(atm["temps"], tvib=atm["tvib"], source="hitran")
    assert np.array_equal(_np(sab), _np(sab0)) and np.array_equal(_np(sem), _np(sem0))
    ls.close()


def test_input_order_dropped_and_outer_lines(eng):
    """Shuffled input with dropped lines and outer lines: strengths come back in input order, spectra unchanged."""
    from spectrobot_amd import spect_classes as sc
    from spectrobot_amd import synthetic as syn
    grid = syn.make_grid(2975.0, 5e-4, 20000)
    L = syn.make_lines(400, grid, config_id=12, n_levels=12)
    L["freq"][:4] = grid[0] - 3.3 - np.arange(4)
    L["freq"][-4:] = grid[-1] + 3.3 + np.arange(4)
    L["lev_up"][10], L["lev_lo"][11] = -1, -1
    L["lev_lo"][12] = L["lev_up"][12]
    s_ref = _s_ref_from_a(sc, L, 6, 1, 1.0) * np.linspace(0.5, 2.0, 400)
    rng = np.random.default_rng(3)
    perm = rng.permutation(400)
    Lp = {k: np.ascontiguousarray(v[perm]) for k, v in L.items()}
    lev = syn.CH4_LEVEL_ENERGIES
    atm = syn.make_atmosphere(5, 12)
    ls = eng.LineSet(L, grid, 6, 1, syn.CH4_MM, lev)
    lsp = eng.LineSet(Lp, grid, 6, 1, syn.CH4_MM, lev)
    ls.set_strengths(s_ref)
    lsp.set_strengths(s_ref[perm])
    dropped = (L["lev_up"] < 0) | (L["lev_lo"] < 0) | (L["lev_up"] == L["lev_lo"])
    assert dropped.sum() >= 3 and ls.n_kept == 400 - dropped.sum()
    for source in ("einstein", "hitran"):
        a, e = (_np(x) for x in ls.line_strengths(atm["temps"], tvib=atm["tvib"], source=source))
        ap, ep = (_np(x) for x in lsp.line_strengths(atm["temps"], tvib=atm["tvib"], source=source))
        assert np.array_equal(ap, a[:, perm]) and np.array_equal(ep, e[:, perm])
        assert np.all(a[:, dropped] == 0.0) and np.all(a[:, ~dropped] != 0.0) and np.all(e[:, ~dropped] > 0.0)
    ab, em = (_np(x) for x in ls.abscoeff_layers_from_strengths(atm["temps"], atm["press"], tvib=atm["tvib"]))
    abp, emp = (_np(x) for x in lsp.abscoeff_layers_from_strengths(atm["temps"], atm["press"], tvib=atm["tvib"]))
    assert relerr(abp, ab) < 1e-13 and relerr(emp, em) < 1e-13
    ls.close()
    lsp.close()


def test_hitran_file_strengths_round_trip(eng):
    """A HITRAN file from disk to the device: at 296 K in LTE the HITRAN source returns the file's own Strength."""
    from spectrobot_amd import spect_classes as sc
    from spectrobot_amd import synthetic as syn
    lines = sc.read_line_database(os.path.join(HERE, "golden", "hitran_sample.par"), mol=6, iso=1)
    assert len(lines) > 20
    grid = syn.make_grid(2990.0, 5e-4, 20000)
    ls = eng.LineSet(sc.lines_to_soa(lines), grid, 6, 1, syn.CH4_MM)
    ls.set_strengths(sc.strengths_of(lines), t_ref=296.0)
    s_ab, s_em = ls.line_strengths([296.0], source="hitran")
    want = np.array([l.Strength for l in lines])
    assert relerr(_np(s_ab)[0], want) <= 1e-14
    assert np.all(_np(s_em) > 0.0)
    ls.close()


def test_refusals(eng):
    import torch
    from spectrobot_amd import _lib
    from spectrobot_amd import synthetic as syn
    grid, L, atm, lev = _case(500, 20000, 3)
    ls = eng.LineSet(L, grid, 6, 1, syn.CH4_MM, lev)
    args = (atm["temps"], atm["press"])
    # the HITRAN source and the strength route without intensities
    with pytest.raises(_lib.SpectRobotHipError) as e:
        ls.line_strengths(atm["temps"], source="hitran")
    assert e.value.status == _lib.SR_ERR_ARG
    with pytest.raises(_lib.SpectRobotHipError) as e:
        ls.abscoeff_layers_from_strengths(*args)
    assert e.value.status == _lib.SR_ERR_ARG
    ls.line_strengths(atm["temps"], source="einstein")          # needs none
    # a wrong number of intensities: refused by the wrapper and by the library
    s = np.full(500, 1e-20)
    with pytest.raises(ValueError):
        ls.set_strengths(s[:-1])
    assert _lib.lib.sr_lineset_set_strengths(ls._h, s.ctypes.data_as(_lib.dp), 499, 296.0, 0.0, 1.0) == _lib.SR_ERR_ARG
    with pytest.raises(ValueError):
        ls.line_strengths(atm["temps"], source="G")
    ls.set_strengths(s)
    ls.abscoeff_layers_from_strengths(*args)
    # linearised weights have no strength form
    ls.set_bounds_temps(atm["temps"], linear_weights=True)
    with pytest.raises(_lib.SpectRobotHipError) as e:
        ls.abscoeff_layers_from_strengths(*args)
    assert e.value.status == _lib.SR_ERR_UNSUPPORTED
    ls.set_bounds_temps(None)
    ls.abscoeff_layers_from_strengths(*args)
    torch.cuda.synchronize()
    ls.close()
    # an iso-molecule the TIPS tables lack: Q must be given (q_ref and q_part)
    lsx = eng.LineSet(L, grid, 99, 1, syn.CH4_MM, lev)
    lsx.set_strengths(s)
    with pytest.raises(_lib.SpectRobotHipError) as e:
        lsx.line_strengths(atm["temps"], source="hitran", q_part=np.full(3, 500.0))
    assert e.value.status == _lib.SR_ERR_TABLE
    lsx.set_strengths(s, q_ref=600.0)
    with pytest.raises(_lib.SpectRobotHipError) as e:
        lsx.line_strengths(atm["temps"], source="hitran")
    assert e.value.status == _lib.SR_ERR_TABLE
    a, _ = lsx.line_strengths(atm["temps"], source="hitran", q_part=np.full(3, 500.0))
    assert np.all(np.isfinite(_np(a)))
    lsx.close()
