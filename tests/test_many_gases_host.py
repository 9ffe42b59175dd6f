"""Host side of ray batches of five to eight gases (no GPU): the export sr_limb_max_gases, the argument checks of the
entries -- all made before any device call, so they answer on a machine without a GPU and leave the outputs alone --, the
state plans with three bits per column slot, the ValueErrors of engine and retrieval.LimbScene's drivers, the live K_PLAIN
of the eight-gas panel against the recorded constants, and the stand-alone harness tools/many_gases_host (the kernel text
under AddressSanitizer and UBSan; nothing is loaded into Python).

The entries that take a resident batch WITH parameters (sr_limb_rays_jac_los_dev, sr_retrieval_forward_dev, _step_dev,
_loop_dev) need a handle, which only a GPU can make: here they are refused where that handle would be made
(sr_los_create_par with parameters answers SR_ERR_LIMIT for five gases); tests/test_gpu_many_gases.py repeats it there."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import limb_reference as R
import many_gases_cases as M
from spectrobot_amd import _lib
from spectrobot_amd import spect_main_module as smm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SENTINEL = -7.25


def test_the_export():
    from spectrobot_amd import engine
    assert _lib.lib.sr_limb_max_gases(0) == 8 and _lib.lib.sr_limb_max_gases(1) == 4 and _lib.lib.sr_limb_max_gases(7) == 4
    assert _lib.SYMBOLS["sr_limb_max_gases"] == (C.c_int, [C.c_int])
    header = open(os.path.join(ROOT, "include", "spectrobot_hip.h")).read()
    assert "int sr_limb_max_gases(int folded);" in header and "n_gas <= 4" not in header
    assert engine.max_gases() == 8 and engine.max_gases(folded=False) == 8 and engine.max_gases(folded=True) == 4
    assert _lib.lib.sr_abi_version() == 1


def _desc(n_gas):
    """A one-ray, two-segment batch of n_gas gases on four layers; the arrays it points into."""
    ip, dp = _lib.ip, _lib.dp
    so, sl, po = np.array([0, 2], np.int32), np.array([1, 3], np.int32), np.array([0, 2, 4], np.int32)
    xx, one = np.array([0.0, 1.0, 1.0, 2.0]), np.ones(4 * max(n_gas, 1))
    d = _lib.LosDesc()
    d.n_rays, d.n_gas = 1, n_gas
    d.seg_off, d.seg_layer, d.pt_off = (a.ctypes.data_as(ip) for a in (so, sl, po))
    d.x, d.nd, d.vmr = xx.ctypes.data_as(dp), one.ctypes.data_as(dp), one.ctypes.data_as(dp)
    d.w0, d.step = 3000.0, 0.01
    return d, [so, sl, po, xx, one]


ALL = ("sr_los_columns", "sr_los_columns_dz", "sr_los_create", "sr_los_create_par", "sr_limb_rays_dev", "sr_limb_rays_jac_dev",
       "sr_limb_rays_jac_layer_dev", "sr_limb_rays_jacobians_dev", "sr_limb_rays_jac_state_gases_dev",
       "sr_limb_rays_state_bands_gases_dev", "sr_state_ray_plan", "sr_limb_rays_parts_dev")
STATE = ("sr_limb_rays_jac_state_gases_dev", "sr_limb_rays_state_bands_gases_dev")


def _entries(n_gas, only, par_gas=0, lgas=((2, 5, 2), (0, 3, 3))):
    """{entry: status} of the entries `only` on a batch of n_gas gases -- only calls that are to be REFUSED are made: the
    buffers that stand for device memory are not device memory, and a call that got as far as a copy or a launch would
    not return a status of its own (sr_state_ray_plan never touches a device)."""
    ip, dp, lib = _lib.ip, _lib.dp, _lib.lib
    d, keep = _desc(n_gas)
    n_layers, n_pts = 4, 10
    fake = C.c_void_p(4096)
    pg, pw = np.array([par_gas], np.int32), np.ones((1, 4))
    pc, pt = np.ones((2, n_layers)), np.ones((1, n_layers))
    plg, lv = np.array([0, 1], np.int32), np.array([1, 2], np.int32)
    cen, wid = np.array([3333.2, 3333.3]), np.array([0.02, 0.02])
    out = np.full(4096, SENTINEL)
    rows = [np.zeros(n_layers, np.int32) for _ in lgas]
    arr = (_lib.LevelGasDesc * len(lgas))()
    for k, (g, nl, nr) in enumerate(lgas):
        arr[k].gas, arr[k].n_levels, arr[k].n_tab_rows, arr[k].tab, arr[k].coef_row = g, nl, nr, 4096, rows[k].ctypes.data_as(ip)
    P = lambda a: a.ctypes.data_as(dp if a.dtype == np.float64 else ip)
    path = _lib.LosPath()
    path.alt = path.dx_dz = path.dalt_dz = P(np.ones(4))
    h = C.c_void_p()
    state = (fake, fake, n_layers, n_pts, C.byref(d), 1, P(pg), P(pw), len(lgas), arr, 2, P(plg), P(lv), P(pc), fake, fake, 1, P(pt))
    band = (P(cen), P(wid), 2, 5.0, 0, None, P(out), None)
    sizes = np.zeros(4, np.int32)
    calls = {
        "sr_los_columns": lambda: lib.sr_los_columns(C.byref(d), P(out)),
        "sr_los_columns_dz": lambda: lib.sr_los_columns_dz(C.byref(d), C.byref(path), P(out)),
        "sr_los_create": lambda: lib.sr_los_create(C.byref(d), n_layers, C.byref(h)),
        "sr_los_create_par": lambda: lib.sr_los_create_par(C.byref(d), n_layers, 1, P(pg), P(pw), C.byref(h)),
        "sr_limb_rays_dev": lambda: lib.sr_limb_rays_dev(fake, fake, n_layers, n_pts, C.byref(d), fake, None),
        "sr_limb_rays_jac_dev": lambda: lib.sr_limb_rays_jac_dev(fake, fake, n_layers, n_pts, C.byref(d), 1, P(pg), P(pw), fake, fake, None),
        "sr_limb_rays_jac_layer_dev": lambda: lib.sr_limb_rays_jac_layer_dev(fake, fake, fake, fake, n_layers, n_pts, C.byref(d), fake, None),
        "sr_limb_rays_jacobians_dev": lambda: lib.sr_limb_rays_jacobians_dev(fake, fake, None, None, n_layers, n_pts, C.byref(d), None, 0, 1, P(pg),
                                                                     P(pw), fake, None, fake, None),
        "sr_limb_rays_parts_dev": lambda: lib.sr_limb_rays_parts_dev(fake, fake, n_layers, n_pts, C.byref(d), 0, None, 0, 0, None, 1, P(pg),
                                                                     P(np.array([-1], np.int32)), None, fake, fake, None),
        "sr_limb_rays_jac_state_gases_dev": lambda: lib.sr_limb_rays_jac_state_gases_dev(*state, fake, fake, None),
        "sr_limb_rays_state_bands_gases_dev": lambda: lib.sr_limb_rays_state_bands_gases_dev(*state, *band),
        "sr_state_ray_plan": lambda: lib.sr_state_ray_plan(C.byref(d), n_layers, 1, P(pg), P(pw), 0, None, None, None, 0, None, 0, P(sizes),
                                                   None, None, None, None, None, None, None, None),
    }
    res = {k: calls[k]() for k in only}
    assert h.value is None and np.all(out == SENTINEL)
    return res


def test_nine_gases_are_refused_by_every_entry():
    res = _entries(9, ALL)
    assert all(v == _lib.SR_ERR_LIMIT for v in res.values()), res


def test_five_gases_are_refused_by_the_entries_of_the_four_slot_kernels():
    """... with SR_ERR_LIMIT: the folded, adjoint and forward-sensitivity entries, and the resident batch with parameters
    that the retrieval entries run on; a column parameter of gas 5 in a five-gas batch is SR_ERR_ARG in the entries that
    take such a batch; a level gas with index 7 of eight passes the checks of its index (the next refusal in the order of
    the checks, too many levels for an entry's word, is what answers -- index 8 is SR_ERR_ARG)."""
    four = ("sr_los_create_par", "sr_limb_rays_jac_dev", "sr_limb_rays_jac_layer_dev", "sr_limb_rays_jacobians_dev", "sr_limb_rays_parts_dev")
    res = _entries(5, four + ("sr_state_ray_plan",))
    assert all(res[k] == _lib.SR_ERR_LIMIT for k in four), res
    assert res["sr_state_ray_plan"] == _lib.SR_OK
    state = STATE
    bad = _entries(5, state + ("sr_state_ray_plan",), par_gas=5)
    assert all(v == _lib.SR_ERR_ARG for v in bad.values()), bad
    deep = _entries(8, state, lgas=((7, 70000, 2), (2, 3, 3)))
    assert all(deep[k] == _lib.SR_ERR_LIMIT for k in state), deep
    out_of_range = _entries(8, state, lgas=((8, 70000, 2), (2, 3, 3)))
    assert all(out_of_range[k] == _lib.SR_ERR_ARG for k in state), out_of_range
    five_lgas = _entries(8, state, lgas=((7, 3, 2), (2, 3, 3), (1, 3, 3), (0, 3, 3), (4, 3, 3)))   # at most four are level-factored
    assert all(five_lgas[k] == _lib.SR_ERR_ARG for k in state), five_lgas


def _plan_case(n_gas):
    from spectrobot_amd import engine
    c = M.panel_case(n_gas)
    los = engine.LimbLOS(M.SEG_OFF, M.SEG_LAYER, M.PT_OFF, c["x"], c["nd"], c["vmr"], col_scale=c["col_scale"])
    return engine, c, los


def test_plans_pack_three_bits_per_column_slot():
    """sr_state_ray_plan of an eight-gas batch with column parameters of gases 0, 4, 7, 5, 3 and the eight hidden slots:
    np == 8 whatever the count, every column slot's gas in three bits; the same call on four gases gives the words of
    two bits and sixteen slots."""
    engine, c, los = _plan_case(8)
    par_gas = np.array([0, 4, 7, 5, 3], np.int32)
    par_w = np.ones((5, los.n_pt))
    P = engine.state_ray_plan(los, M.N_LAYERS, par_gas, par_w, n_hid=8)
    assert P["np"] == 8 and P["n_blocks"] == 2 and list(P["ray_blk_off"]) == [0, 2, 4, 6]
    want = list(par_gas) + list(range(8))
    for ray in range(3):
        got = []
        for rb in range(P["ray_blk_off"][ray], P["ray_blk_off"][ray + 1]):
            nc, word = P["blk"][rb]
            got += [(int(word) >> (3 * q)) & 7 for q in range(nc)]
            assert nc <= 8 and 0 <= int(word) < (1 << 24)
        assert got == want, (ray, got)
        rows = [int(P["col_row"][P["ray_blk_off"][ray] + q // 8, q % 8]) for q in range(13)]
        assert rows == list(range(13))
    # many parameters: still eight slots per block
    P = engine.state_ray_plan(los, M.N_LAYERS, np.arange(17, dtype=np.int32) % 8, np.ones((17, los.n_pt)))
    assert P["np"] == 8 and P["n_blocks"] == 3
    los.close()
    engine, c, los = _plan_case(4)
    par_gas = np.array([0, 3, 2, 1, 3], np.int32)
    P = engine.state_ray_plan(los, M.N_LAYERS, par_gas, np.ones((5, los.n_pt)), n_hid=4)
    assert P["np"] == 16 and P["n_blocks"] == 1
    want = list(par_gas) + list(range(4))
    for rb in range(3):
        nc, word = P["blk"][rb]
        assert nc == 9 and [(int(word) >> (2 * q)) & 3 for q in range(nc)] == want
    with pytest.raises(Exception):
        engine.state_ray_plan(los, M.N_LAYERS, par_gas, np.ones((5, los.n_pt)), n_hid=5)       # (a hidden slot per gas, four here)
    los.close()


class _Los(object):
    n_gas, n_rays, n_pt = 5, 2, 9


def test_the_engine_refuses_the_four_slot_calls_before_any_device_call(monkeypatch):
    from spectrobot_amd import engine
    monkeypatch.setattr(engine, "_gas_stack", lambda c: pytest.fail("a device call"))
    los = _Los()
    calls = {"limb_rays_jacobian": lambda: engine.limb_rays_jacobian(None, los, [0], None),
             "limb_rays_jacobians": lambda: engine.limb_rays_jacobians(None, los),
             "limb_rays_parts": lambda: engine.limb_rays_parts(None, los, [0], [-1]),
             "retrieval_forward": lambda: engine.retrieval_forward(None, los, [0], None, [1.0], None, [1.0], [1.0]),
             "retrieval_step": lambda: engine.retrieval_step(None, los, [0], None, [1.0], None, [1.0], [1.0], None),
             "retrieval_loop": lambda: engine.retrieval_loop(None, los, [0], None, [1.0], None, [1.0], [1.0], None, [True], 0)}
    for name, call in calls.items():
        with pytest.raises(ValueError, match=r"%s: a batch of 5 gases.*max_gases\(folded=True\) = 4" % name):
            call()
    with pytest.raises(ValueError, match="5 members"):
        engine.LevelFactoredSet([(None, g, None, None) for g in range(5)])


class _LS(object):
    iso, level_energies = 1, np.zeros(0)


def test_the_drivers_refuse_a_scene_of_more_than_four_slots():
    from spectrobot_amd import retrieval as rt
    z = np.linspace(100.0, 900.0, 9)
    gases = [rt.Gas("G%d" % k, _LS(), np.full(9, 1e-6)) for k in range(5)]
    gases.append(rt.TableGas("T", None, np.ones(9)))
    gases.append(rt.TableGas("folded", None, None, accumulate_into="G0"))          # takes no slot
    scene = rt.LimbScene(np.linspace(3000.0, 3001.0, 11), z, np.full(9, 160.0), np.geomspace(1.0, 1e-6, 9), gases, [3330.0], [1.0])
    assert len(scene.gases) == 6
    bs = smm.BayesSet()
    bs.add_set(smm.LinearProfile_1D_new("G0", z, [200.0, 500.0], np.full(2, 1e-6), np.full(2, 1e-6)))
    pix = [rt.LimbPixel(300.0)]
    for name, call in (("simulate with a bayes_set", lambda: rt.simulate(scene, pix, bs)),
                       ("inversion_fast_limb", lambda: rt.inversion_fast_limb(scene, bs, pix)),
                       ("inversion", lambda: rt.inversion(scene, bs, pix)), ("radtrans", lambda: rt.radtrans(scene, pix))):
        with pytest.raises(ValueError, match=r"%s: a scene of 6 gas slots.*max_gases\(folded=True\) = 4" % name):
            call()
    assert "eight" in rt.TableGas.__doc__ and "four" in rt.TableGas.__doc__ and "eight" in rt.Gas.__doc__


@pytest.mark.parametrize("n_gas", [5, 8])
def test_k_plain_of_the_panel_stays_below_the_recorded_constants(n_gas):
    """The live K_PLAIN of the five- and eight-gas panels (plain fp64 against the extended-precision reference, columns
    from the host's Curtis-Godson restatement) for every kind of state the GPU tests use: below K_PLAIN_RAD and K_PLAIN_JAC
    of tests/limb_reference.py, which stay as they are."""
    c = M.panel_case(n_gas)
    col = M.host_columns(c)
    worst_r = worst_j = 0.0
    for kind in M.KINDS:
        s = M.state(c, kind)
        k_rad, k_jac = M.k_plain(M.references(s, col, M.host_dcol(s), np.zeros(len(c["names"]))), n_gas)
        worst_r, worst_j = max(worst_r, k_rad), max(worst_j, k_jac)
    print("\nK_PLAIN of the %d-gas panel: radiances %.3g (recorded %.3g), Jacobian rows %.3g (recorded %.3g)"
          % (n_gas, worst_r, R.K_PLAIN_RAD, worst_j, R.K_PLAIN_JAC))
    assert 0.0 < worst_r <= R.K_PLAIN_RAD and 0.0 < worst_j <= R.K_PLAIN_JAC


def test_the_kernel_text_on_the_host_under_the_sanitizers():
    """tools/many_gases_host: sr_limb_kernel<8>, sr_limb_split_kernel<5>, the state kernel's eight-gas instances with
    column, level, row slots, the band epilogue, two level gases and blocks per ray against plain loops, and the padded
    launches against the unpadded instances, and the dense and per-ray plans with gases 0, 4, 7, 5, 3 and eight hidden slots
    decoded word by word (today's words on four gases); a stand-alone program under AddressSanitizer and UBSan."""
    r = subprocess.run(["bash", os.path.join(ROOT, "tools", "host_sim", "run.sh"), "many_gases_host"], capture_output=True, text=True)
    print(r.stdout[-3000:], r.stderr[-3000:])
    assert r.returncode == 0 and "all cases agree" in r.stdout and "0 values differ" in r.stdout
    assert "plan words that do not decode to their gases and rows: 0" in r.stdout
