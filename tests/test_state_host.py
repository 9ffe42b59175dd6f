"""Host side of the mixed state vector (no GPU): the ABI surface of sr_limb_rays_jac_state_dev and its argument checks --
all of them made before any device call, so they answer on a machine without a GPU --, the masks of TvibProfile and the
split of a BayesSet into the call's two parameter blocks (LimbScene.state_weights)."""
import ctypes as C

import numpy as np
import pytest

from spectrobot_amd import _lib
from spectrobot_amd import spect_main_module as smm


def test_abi_surface_of_the_state_call():
    res, args = _lib.SYMBOLS["sr_limb_rays_jac_state_dev"]
    ip, dp, vp, ci = _lib.ip, _lib.dp, C.c_void_p, C.c_int
    assert res is C.c_int
    assert list(args) == [vp, vp, ci, C.c_int64, C.POINTER(_lib.LosDesc),      # abs_c, emi_c, n_layers, n_pts, los
                          ci, ip, dp,                                          # n_col, par_gas, par_w
                          ci, vp, ci, ci, ip,                                  # gas, tab, n_levels, n_tab_rows, coef_row
                          ci, ip, dp,                                          # n_lev, par_level, par_c
                          vp, vp, vp]                                          # rad, jac, stream
    assert hasattr(_lib.lib, "sr_limb_rays_jac_state_dev")
    assert _lib.lib.sr_abi_version() == 1


def test_refused_arguments_return_before_any_device_call():
    """Every refused argument returns its status from the host checks (the buffers below are not device memory: a call
    that got as far as a copy or a launch would not return a status of its own)."""
    ip, dp = _lib.ip, _lib.dp
    n_layers, n_pts, n_levels, n_rows = 4, 10, 3, 2
    so, sl, po = np.array([0, 2], np.int32), np.array([1, 3], np.int32), np.array([0, 2, 4], np.int32)
    xx = np.array([0.0, 1.0, 1.0, 2.0])
    one = np.ones(8)
    d = _lib.LosDesc()
    d.n_rays, d.n_gas = 1, 2
    d.seg_off, d.seg_layer, d.pt_off = (a.ctypes.data_as(ip) for a in (so, sl, po))
    d.x, d.nd, d.vmr = xx.ctypes.data_as(dp), one.ctypes.data_as(dp), one.ctypes.data_as(dp)
    fake = C.c_void_p(4096)               # stands for a device buffer: never dereferenced by a refused call
    row = np.array([0, 1, 1, 0], np.int32)
    pg = np.array([1, 0, 1], np.int32)
    pw = np.ones((3, 4))
    pl = np.array([0, 2], np.int32)
    pc = np.ones((2, n_layers))

    def call(**kw):
        dd = kw.get("los", d)
        r = np.ascontiguousarray(kw.get("coef_row", row), dtype=np.int32)
        g = np.ascontiguousarray(kw.get("par_gas", pg), dtype=np.int32)
        lv = np.ascontiguousarray(kw.get("par_level", pl), dtype=np.int32)
        no = kw.get("no", ())
        return _lib.lib.sr_limb_rays_jac_state_dev(
            None if "abs" in no else fake, None if "emi" in no else fake, n_layers, kw.get("n_pts", n_pts),
            C.byref(dd) if dd is not None else None, kw.get("n_col", 3), None if "par_gas" in no else g.ctypes.data_as(ip),
            None if "par_w" in no else pw.ctypes.data_as(dp), kw.get("gas", 1), None if "tab" in no else fake,
            kw.get("n_levels", n_levels), kw.get("n_rows", n_rows), None if "coef_row" in no else r.ctypes.data_as(ip),
            kw.get("n_lev", 2), None if "par_level" in no else lv.ctypes.data_as(ip),
            None if "par_c" in no else pc.ctypes.data_as(dp), fake, None if "jac" in no else fake, None)

    d1 = _lib.LosDesc()
    C.memmove(C.byref(d1), C.byref(d), C.sizeof(d))
    d1.init_mode = 1
    refused = [dict(no=("abs",)), dict(no=("emi",)), dict(no=("jac",)), dict(los=None),                  # NULLs
               dict(no=("par_gas",)), dict(no=("par_w",)), dict(no=("tab",)), dict(no=("coef_row",)),
               dict(no=("par_level",)), dict(no=("par_c",)),
               dict(n_col=0, n_lev=0), dict(n_col=-1), dict(n_lev=-1), dict(n_levels=0), dict(n_rows=0),  # no parameters
               dict(par_gas=[1, 2, 1]), dict(par_gas=[-1, 0, 1]),                                         # par_gas out of range
               dict(par_level=[0, n_levels]), dict(par_level=[-1, 2]),                                    # par_level out of range
               dict(coef_row=[0, 1, n_rows, 0]), dict(coef_row=[-1, 1, 1, 0]),                            # coef_row out of range
               dict(gas=2), dict(gas=-1),                                                                 # gas out of range
               dict(los=d1)]                                                                              # init_mode 1
    for kw in refused:
        assert call(**kw) == _lib.SR_ERR_ARG, kw
    assert call(n_pts=2000001) == _lib.SR_ERR_LIMIT
    # an empty kind needs none of its arrays -- but the other kind is still checked
    assert call(n_lev=0, no=("tab", "coef_row", "par_level", "par_c"), par_gas=[0, 0, 2]) == _lib.SR_ERR_ARG
    assert call(n_col=0, no=("par_gas", "par_w"), par_level=[0, 3]) == _lib.SR_ERR_ARG


def test_tvib_profile_masks_are_the_level_node_weights():
    from spectrobot_amd import engine, retrieval as rt
    z = np.linspace(100.0, 900.0, 23)
    nodes = [150.0, 330.0, 510.0, 690.0, 850.0]
    tp = rt.TvibProfile("CH4", 5, z, nodes, np.full(5, 4.0))
    assert tp.name == "tvib:CH4:5" and (tp.gas, tp.level) == ("CH4", 5)
    assert np.array_equal(tp.mask_matrix(), engine.level_node_weights(nodes, z))
    assert all(p.constrain_positive is False for p in tp.set)
    assert [p.value for p in tp.set] == [0.0] * 5 and [p.apriori_err for p in tp.set] == [4.0] * 5
    bs = smm.BayesSet()
    bs.add_set(tp)                       # (add_set copies the set: the copy keeps what the scene reads)
    assert all(p.constrain_positive is False for p in bs.params()) and bs.order == ["tvib:CH4:5"]
    assert np.array_equal(bs.sets["tvib:CH4:5"].profile(), np.zeros(23))


class _LS(object):
    def __init__(self, n_lev):
        self.iso, self.level_energies = 1, np.arange(float(n_lev))


def _scene():
    from spectrobot_amd import retrieval as rt
    z = np.linspace(100.0, 900.0, 17)
    temps, press = np.linspace(170.0, 150.0, 17), np.geomspace(1.0, 1e-6, 17)
    gases = [rt.Gas("HCN", _LS(0), np.full(17, 1e-6)), rt.LevelGas("CH4", _LS(12), np.full(17, 1e-2), np.full((12, 17), 160.0)),
             rt.Gas("CO", _LS(0), np.full(17, 1e-5)), rt.LevelGas("C2H2", _LS(4), np.full(17, 1e-6), np.full((4, 17), 160.0))]
    return rt.LimbScene(np.linspace(3000.0, 3001.0, 11), z, temps, press, gases, [3330.0], [1.0]), z


def test_state_weights_round_trip_a_shuffled_bayes_set():
    """The two blocks hold every parameter once, in BayesSet order within its kind, and perm leads back: row perm[i] of
    the call's Jacobian (column parameters, then level parameters) belongs to BayesSet parameter i."""
    from spectrobot_amd import retrieval as rt
    scene, z = _scene()
    n_hcn, n_ch4, n_t5, n_t2 = [200.0, 500.0, 800.0], [150.0, 450.0, 600.0, 850.0], [200.0, 400.0, 700.0], [300.0, 600.0]
    sets = {"HCN": smm.LinearProfile_1D_new("HCN", z, n_hcn, np.full(3, 1e-6), np.full(3, 1e-6)),
            "CH4": smm.LinearProfile_1D_new("CH4", z, n_ch4, np.full(4, 1e-2), np.full(4, 1e-2)),
            "tvib:CH4:5": rt.TvibProfile("CH4", 5, z, n_t5, np.full(3, 4.0)),
            "tvib:CH4:2": rt.TvibProfile("CH4", 2, z, n_t2, np.full(2, 4.0))}
    alt = np.random.default_rng(3).uniform(90.0, 1000.0, 41)
    rng = np.random.default_rng(11)
    for _ in range(6):
        order = list(rng.permutation(list(sets)))
        bs = smm.BayesSet()
        for name in order:
            bs.add_set(sets[name])
        w = scene.state_weights(bs, alt)
        params = bs.params()
        n_col = 7
        assert w.par_gas.dtype == np.int32 and w.par_level.dtype == np.int32
        assert w.par_w_col.shape == (7, 41) and w.par_w_lev.shape == (5, 17) and w.level_gas is scene.gas("CH4") and w.gas == 1
        assert sorted(w.perm) == list(range(12))
        kinds = [0 if p.nameset in ("HCN", "CH4") else 1 for p in params]
        # within a kind the blocks keep the BayesSet's order
        assert [w.perm[i] for i, k in enumerate(kinds) if k == 0] == list(range(n_col))
        assert [w.perm[i] for i, k in enumerate(kinds) if k == 1] == list(range(n_col, 12))
        top = z[-1] + (z[-1] - z[-2])
        for i, par in enumerate(params):
            q = w.perm[i]
            m = np.asarray(par.maskgrid.mask, float)
            if kinds[i] == 0:
                assert w.par_gas[q] == ["HCN", "CH4"].index(par.nameset)
                assert np.array_equal(w.par_w_col[q], np.interp(alt, np.append(z, top), np.append(m, m[-1])))
            else:
                assert w.par_level[q - n_col] == int(par.nameset.split(":")[2])
                assert np.array_equal(w.par_w_lev[q - n_col], m)
        # a Jacobian in call order, permuted: the columns of BayesSet order
        call_rows = np.arange(12.0)
        assert np.array_equal(call_rows[w.perm], np.array([w.perm[i] for i in range(12)], float))
    # only VMR sets: the weights of profile_weights, no level gas
    bs = smm.BayesSet()
    bs.add_set(sets["CH4"])
    bs.add_set(sets["HCN"])
    w = scene.state_weights(bs, alt)
    pg, pw = scene.profile_weights(bs, alt)
    assert w.level_gas is None and w.gas is None and w.par_level.size == 0 and w.par_w_lev.shape == (0, 17)
    assert np.array_equal(w.par_gas, pg) and np.array_equal(w.par_w_col, pw) and list(w.perm) == list(range(7))


def test_state_weights_refuses_unknown_sets_and_two_level_gases():
    from spectrobot_amd import retrieval as rt
    scene, z = _scene()
    nodes = [200.0, 500.0, 800.0]
    alt = np.linspace(100.0, 900.0, 9)

    def bayes(*sets):
        bs = smm.BayesSet()
        for st in sets:
            bs.add_set(st)
        return bs

    vmr = lambda name: smm.LinearProfile_1D_new(name, z, nodes, np.full(3, 1e-6), np.full(3, 1e-6))
    tv = lambda gas, lev: rt.TvibProfile(gas, lev, z, nodes, np.full(3, 4.0))
    for bad in (vmr("N2"), tv("N2", 1), tv("HCN", 1), tv("CH4", 12), vmr("tvib:CH4"), vmr("tvib:CH4:x"), vmr("temp:CH4:1")):
        with pytest.raises(ValueError, match="names neither a gas"):
            scene.state_weights(bayes(vmr("HCN"), bad), alt)
    with pytest.raises(ValueError, match="more than one gas"):
        scene.state_weights(bayes(tv("CH4", 5), vmr("HCN"), tv("C2H2", 1)), alt)
    w = scene.state_weights(bayes(tv("C2H2", 3), vmr("C2H2")), alt)          # the other level gas alone is fine
    assert w.gas == 3 and list(w.perm) == [3, 4, 5, 0, 1, 2]
    with pytest.raises(ValueError):
        rt.LevelGas("CH4", _LS(12), np.full(17, 1e-2), np.full((11, 17), 160.0))
