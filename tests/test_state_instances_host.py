"""Host side of the census of sr_limb_jac_state_kernel's compiled instances (no GPU): the export sr_last_state_instance,
the table tests/state_instances_cases.EXPECTED against the set the launcher's rules generate and against the host path's
own routing (which entry, which unit, which slots per block -- the per-ray plan from sr_state_ray_plan, which touches no
device), the shapes the table has to contain, the generalised states against many_gases_cases bit for bit, and the live
K_PLAIN of every case against the recorded constants of tests/limb_reference.py."""
import ctypes as C
import os
import threading

import numpy as np
import pytest

import limb_reference as R
import many_gases_cases as M
import state_instances_cases as X
from spectrobot_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SENTINEL = -7.25
ENTRIES = [X.entry_dict(e) for e in X.EXPECTED]


def test_the_export():
    from spectrobot_amd import engine
    assert _lib.SYMBOLS["sr_last_state_instance"] == (C.c_int, [_lib.ip])
    header = open(os.path.join(ROOT, "include", "spectrobot_hip.h")).read()
    assert "int sr_last_state_instance(int32_t out[8]);" in header
    assert _lib.lib.sr_last_state_instance(None) == _lib.SR_ERR_ARG          # a null pointer
    out, seen = np.full(8, 77, np.int32), []

    def fresh():                          # the record is the calling thread's: a new thread has launched nothing
        seen.append((_lib.lib.sr_last_state_instance(out.ctypes.data_as(_lib.ip)), engine.last_state_instance()))

    t = threading.Thread(target=fresh)
    t.start()
    t.join()
    assert seen == [(_lib.SR_ERR_ARG, None)] and np.all(out == 77)
    assert engine.StateInstance._fields == ("ng", "np", "cols", "rows", "bands", "instr", "several", "rayblk")
    assert _lib.lib.sr_abi_version() == 1


def test_expected_is_the_set_the_rules_generate():
    keys = [e["key"] for e in ENTRIES]
    assert len(keys) == len(set(keys)) == 432
    assert set(keys) == X.compiled_instances()
    per_ng = {ng: sum(k[0] == ng for k in keys) for ng in (1, 2, 3, 4, 6, 8)}
    assert per_ng == {1: 48, 2: 96, 3: 96, 4: 96, 6: 48, 8: 48}
    assert X.BARRED == ()
    for e in ENTRIES:
        assert e["option"] in X.OPTIONS and e["call"] in ("level", "state", "bands", "instr") and 1 <= e["n_gas"] <= 8
        assert X.flags_of((e["ng"], e["np"]) + tuple(f != "-" for f in e["flags"])) == e["key"]


def _routed(e, s, los):
    """(NG, NP, flags) of the instance the host path launches for entry e: the rules of engine's call (which library
    entry), of that entry (column slots), of launch_limb_jac_state (the unit) and of the plans (slots per block)."""
    from spectrobot_amd import engine
    n_gas, pointing, several = e["n_gas"], e["option"] == "pointing", len(e["levs"]) == 2
    n_hid = n_gas if pointing else 0
    n_par = e["n_state"] + n_hid
    bands, instr = e["call"] in ("bands", "instr"), e["call"] == "instr"
    # the engine's argument checks: a parameter, unless the call returns something without
    assert e["n_state"] >= 1 or instr or pointing
    if e["call"] == "level":              # limb_rays_level_jacobian: sr_limb_rays_jac_level_dev, no column code
        assert e["n_col"] == e["n_row"] == 0 and not several and not pointing and e["n_state"] >= 1
        cols = False
    elif bands or pointing or several:    # the bands entries; the path entries; sr_limb_rays_jac_state_gases_dev
        cols = e["n_col"] > 0 or pointing
    elif e["n_row"]:                      # sr_limb_rays_jac_state_rows_dev
        cols = e["n_col"] > 0
    else:                                 # sr_limb_rays_jac_state_dev: the state call, always with column slots
        cols = True
    ng = n_gas if n_gas <= 4 else 6 if n_gas <= 6 else 8
    if n_gas > 4:
        n_p = 8
    elif e["ray_blocks"]:
        P = engine.state_ray_plan(los, X.N_LAYERS, s["par_gas"], s["par_w"], s["par_level"], s["par_c"], s["par_t"] if s["n_row"] else None,
                                  s["par_lgas"] if several else None, n_hid=n_hid)
        n_p = P["np"]
    else:
        n_p = 16 if n_par > 8 else 8
    return X.flags_of((ng, n_p, cols, e["n_row"] > 0, bands, instr, several, e["ray_blocks"]))


@pytest.mark.parametrize("n_gas", range(1, 9))
def test_every_entry_is_routed_to_its_instance(n_gas):
    from spectrobot_amd import engine
    c = X.panel_case(n_gas)
    g = c["geo"]
    los = engine.LimbLOS(g["seg_off"], g["seg_layer"], g["pt_off"], c["x"], c["nd"], c["vmr"], col_scale=c["col_scale"])
    mine = [e for e in ENTRIES if e["n_gas"] == n_gas]
    assert mine
    for e in mine:
        s = X.state(c, e["n_col"], e["levs"], e["n_row"])
        assert _routed(e, s, los) == e["key"], e
        assert (e["option"] == "pointing") <= ("C" in e["flags"])
    los.close()


def test_the_shapes_the_table_has_to_contain():
    n_par = lambda e: e["n_state"] + (e["n_gas"] if e["option"] == "pointing" else 0)
    dense = [e for e in ENTRIES if not e["ray_blocks"]]
    assert {8, 9, 16, 17} <= {n_par(e) for e in dense if e["ng"] <= 4}       # a full NP8 block, the switch, a full NP16 block, a second
    assert {8, 9, 17} <= {n_par(e) for e in ENTRIES if e["ng"] >= 6}         # five to eight gases: blocks of eight whatever the count
    empty = [e for e in ENTRIES if e["n_state"] == 0]
    assert empty and all(e["flags"] == "--BI--" and e["np"] == 8 and e["option"] != "pointing" for e in empty)
    assert {e["ng"] for e in empty} == {1, 2, 3, 4, 6, 8}
    assert any(e["ng"] == 6 and e["n_gas"] == 6 for e in ENTRIES) and any(e["ng"] == 6 and e["n_gas"] == 5 for e in ENTRIES)
    assert any(e["ng"] == 8 and e["n_gas"] == 7 for e in ENTRIES) and any(e["ng"] == 8 and e["n_gas"] == 8 for e in ENTRIES)
    for ng in (1, 2, 3, 4, 6, 8):
        assert {e["option"] for e in ENTRIES if e["ng"] == ng} == set(X.OPTIONS), ng
    for opt in X.OPTIONS:                 # no option is seen with one setting of a flag only (pointing is COLS)
        for k, f in enumerate(X.FLAGS):
            seen = {e["flags"][k] for e in ENTRIES if e["option"] == opt}
            assert seen == ({"C"} if (opt, f) == ("pointing", "C") else {f, "-"}), (opt, f)
    by_key = {e["key"]: e for e in ENTRIES}
    for e in ENTRIES:                     # a bands entry has the state and the option of its spectra twin
        t = by_key[e["twin"]]
        assert t["call"] in ("level", "state") and (t["n_gas"], t["option"]) == (e["n_gas"], e["option"])
        if e["n_state"]:
            assert (t["n_col"], t["levs"], t["n_row"]) == (e["n_col"], e["levs"], e["n_row"])


def test_a_call_without_any_parameter_is_refused_unless_it_has_instrument_rows():
    """The one refusal next to the table: sr_limb_rays_state_bands_dev with no parameter answers SR_ERR_ARG before any
    copy or launch, the outputs untouched (its _instr form is the table's entry without a parameter)."""
    lib, ip, dp = _lib.lib, _lib.ip, _lib.dp
    so, sl, po = np.array([0, 2], np.int32), np.array([1, 3], np.int32), np.array([0, 2, 4], np.int32)
    xx, one = np.array([0.0, 1.0, 1.0, 2.0]), np.ones(4)
    d = _lib.LosDesc()
    d.n_rays, d.n_gas = 1, 1
    d.seg_off, d.seg_layer, d.pt_off = (a.ctypes.data_as(ip) for a in (so, sl, po))
    d.x, d.nd, d.vmr = xx.ctypes.data_as(dp), one.ctypes.data_as(dp), one.ctypes.data_as(dp)
    d.w0, d.step = 3000.0, 0.01
    fake = C.c_void_p(4096)
    cen, wid, out = np.array([3333.2, 3333.3]), np.array([0.02, 0.02]), np.full(64, SENTINEL)
    rc = lib.sr_limb_rays_state_bands_dev(fake, fake, 4, 10, C.byref(d), 0, None, None, 0, None, 0, 0, None, 0, None, None, None, None, 0,
                                          None, cen.ctypes.data_as(dp), wid.ctypes.data_as(dp), 2, 5.0, 0, None, out.ctypes.data_as(dp), None)
    assert rc == _lib.SR_ERR_ARG and np.all(out == SENTINEL)


@pytest.mark.parametrize("n_gas", [5, 8])
def test_the_generalised_states_are_many_gases_cases_bit_for_bit(n_gas):
    c = X.panel_case(n_gas)
    col = X.host_columns(c)
    N = len(c["names"])
    at = R.tile_columns(N, X.N_PTS, np.random.default_rng([X.SEED, n_gas, 77]))
    for kind in M.KINDS:
        want, got = M.state(c, kind), X.state(c, **X.kind_spec(n_gas, kind))
        for key in ("par_gas", "par_w", "par_lgas", "par_level", "par_c", "dabs", "demi", "par_t"):
            assert got[key].dtype == want[key].dtype and np.array_equal(got[key], want[key]), (kind, key)
        assert len(got["lgases"]) == len(want["lgases"])
        for (g0, t0, r0), (g1, t1, r1) in zip(got["lgases"], want["lgases"]):
            assert g0 == g1 and np.array_equal(t0, t1) and np.array_equal(r0, r1)
        if kind in ("cols", "all"):
            dcol = X.host_dcol(want)
            for a, b in ((M.references(want, col, dcol, np.zeros(N)), X.references(got, col, dcol)),
                         (M.references(want, col, dcol, np.zeros(N), cols=at), X.references(got, col, dcol, at=at))):
                for (ra, (Ia, Ja)), (rb, (Ib, Jb)) in zip(a, b):
                    assert all(np.array_equal(ra[k], rb[k]) for k in ra) and np.array_equal(Ia, Ib) and np.array_equal(Ja, Jb)


@pytest.mark.parametrize("n_gas", range(1, 9))
def test_k_plain_of_every_case_stays_below_the_recorded_constants(n_gas):
    """The live K_PLAIN (plain fp64 against the extended-precision reference; columns from the host's Curtis-Godson
    restatement, spect_classes.Calc_BB_single at the first points of the grid for the Planck start, scaled columns for the
    pointing derivative's) of every distinct (state, option) of the table's entries of this gas count."""
    from spectrobot_amd import spect_classes
    c = X.panel_case(n_gas)
    col = X.host_columns(c)
    N = len(c["names"])
    rng = np.random.default_rng([X.SEED, n_gas, 78])
    planck = np.array([spect_classes.Calc_BB_single(2975.0 + 5e-4 * j, X.T_PLANCK) for j in range(N)])
    cases = sorted({(e["n_col"], e["levs"], e["n_row"], e["option"] or "") for e in ENTRIES if e["n_gas"] == n_gas and e["n_state"]})
    worst_r = worst_j = 0.0
    for n_col, levs, n_row, option in cases:
        s = X.state(c, n_col, levs, n_row)
        _, solo, observer = X.options_of(option or None)
        I0 = planck if option in ("planck", "solo") else None
        hidden = col * rng.uniform(-1.0, 1.0, col.shape) if option == "pointing" else None
        refs = X.references(s, col, X.host_dcol(s), I0, solo=solo, hidden=hidden, observer=observer)
        k_rad, k_jac = X.k_plain(refs, n_gas, n_state=s["n_col"] + s["n_lev"] + s["n_row"] if hidden is not None else None)
        worst_r, worst_j = max(worst_r, k_rad), max(worst_j, k_jac)
    print("\nK_PLAIN of the %d cases of %d gases: radiances %.3g (recorded %.3g), Jacobian rows %.3g (recorded %.3g)"
          % (len(cases), n_gas, worst_r, R.K_PLAIN_RAD, worst_j, R.K_PLAIN_JAC))
    assert 0.0 < worst_r <= R.K_PLAIN_RAD and 0.0 < worst_j <= R.K_PLAIN_JAC
