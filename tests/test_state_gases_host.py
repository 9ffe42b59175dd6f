"""Host side of the vibrational-temperature parameters of several level-factored gases in one state pass (no GPU): the ABI
surface of sr_limb_rays_jac_state_gases_dev and sr_limb_rays_state_bands_gases_dev, their argument checks -- all made
before any device call, so they answer on a machine without a GPU and leave the outputs alone --, the wrappers' own
refusals, and the split of a BayesSet with the Tvib sets of two LevelGas into the call's blocks
(LimbScene.state_weights(several_level_gases=True))."""
import ctypes as C

import numpy as np
import pytest

from spectrobot_amd import _lib
from spectrobot_amd import spect_main_module as smm


def test_abi_surface_of_the_two_entries():
    ip, dp, vp, ci = _lib.ip, _lib.dp, C.c_void_p, C.c_int
    res, args = _lib.SYMBOLS["sr_limb_rays_jac_state_gases_dev"]
    assert res is C.c_int
    state = [vp, vp, ci, C.c_int64, C.POINTER(_lib.LosDesc),                   # abs_c, emi_c, n_layers, n_pts, los
             ci, ip, dp,                                                       # n_col, par_gas, par_w
             ci, C.POINTER(_lib.LevelGasDesc),                                 # n_lgas, lgas
             ci, ip, ip, dp,                                                   # n_lev, par_lgas, par_level, par_c
             vp, vp, ci, dp]                                                   # dabs_c, demi_c, n_row, par_t
    assert list(args) == state + [vp, vp, vp]                                  # rad, jac, stream
    rows = list(_lib.SYMBOLS["sr_limb_rays_jac_state_rows_dev"][1])
    assert list(args[:8]) == rows[:8] and list(args[14:]) == rows[16:]         # as the rows call around the level block
    res, args = _lib.SYMBOLS["sr_limb_rays_state_bands_gases_dev"]
    bands = list(_lib.SYMBOLS["sr_limb_rays_state_bands_dev"][1])
    assert res is C.c_int and list(args) == state + bands[20:]                 # the band arguments of the one-gas entry
    assert [f[0] for f in _lib.LevelGasDesc._fields_] == ["gas", "n_levels", "n_tab_rows", "tab", "coef_row"]
    assert C.sizeof(_lib.LevelGasDesc) == 32
    assert hasattr(_lib.lib, "sr_limb_rays_jac_state_gases_dev") and hasattr(_lib.lib, "sr_limb_rays_state_bands_gases_dev")
    assert _lib.lib.sr_abi_version() == 1


SENTINEL = -7.25


def _calls():
    """call(bands, **kw) -> status of one of the two entries on a two-ray, three-gas batch with two level gases; the
    buffers that stand for device memory are not device memory: a call that got as far as a copy or a launch would not
    return a status of its own."""
    ip, dp = _lib.ip, _lib.dp
    n_layers, n_pts = 4, 10
    so, sl, po = np.array([0, 2], np.int32), np.array([1, 3], np.int32), np.array([0, 2, 4], np.int32)
    xx, one = np.array([0.0, 1.0, 1.0, 2.0]), np.ones(12)
    d = _lib.LosDesc()
    d.n_rays, d.n_gas = 1, 3
    d.seg_off, d.seg_layer, d.pt_off = (a.ctypes.data_as(ip) for a in (so, sl, po))
    d.x, d.nd, d.vmr = xx.ctypes.data_as(dp), one.ctypes.data_as(dp), one.ctypes.data_as(dp)
    d.w0, d.step = 3000.0, 0.01
    fake = C.c_void_p(4096)
    pg, pw = np.array([1, 0, 2], np.int32), np.ones((3, 4))
    pc, pt = np.ones((3, n_layers)), np.ones((2, n_layers))
    cen, wid = np.array([3333.2, 3333.3]), np.array([0.02, 0.02])
    out = np.full((1, 1 + 3 + 3 + 2, 2), SENTINEL)
    keep = [so, sl, po, xx, one]                  # (the descriptor only points into them)

    def call(bands=False, **kw):
        dd = kw.get("los", d)
        no = kw.get("no", ())
        gases = kw.get("gases", [(2, 5, 2, [0, 1, 1, 0]), (0, 3, 3, [2, 0, 1, 2])])   # gas, n_levels, n_tab_rows, coef_row
        arr = (_lib.LevelGasDesc * max(len(gases), 1))()
        for k, (g, nl, nr, cr) in enumerate(gases):
            cr = np.ascontiguousarray(cr, dtype=np.int32)
            keep.append(cr)
            arr[k].gas, arr[k].n_levels, arr[k].n_tab_rows = g, nl, nr
            arr[k].tab = None if ("tab", k) in no else 4096
            arr[k].coef_row = None if ("coef_row", k) in no else cr.ctypes.data_as(ip)
        plg = np.ascontiguousarray(kw.get("par_lgas", [1, 0, 0]), dtype=np.int32)
        lv = np.ascontiguousarray(kw.get("par_level", [2, 4, 0]), dtype=np.int32)
        g = np.ascontiguousarray(kw.get("par_gas", pg), dtype=np.int32)
        head = (None if "abs" in no else fake, fake, n_layers, kw.get("n_pts", n_pts), C.byref(dd) if dd is not None else None,
                kw.get("n_col", 3), g.ctypes.data_as(ip), pw.ctypes.data_as(dp),
                kw.get("n_lgas", len(gases)), None if "lgas" in no else arr,
                kw.get("n_lev", 3), None if "par_lgas" in no else plg.ctypes.data_as(ip),
                None if "par_level" in no else lv.ctypes.data_as(ip), None if "par_c" in no else pc.ctypes.data_as(dp),
                None if "dabs" in no else fake, fake, kw.get("n_row", 2), pt.ctypes.data_as(dp))
        if bands:
            return _lib.lib.sr_limb_rays_state_bands_gases_dev(*head, cen.ctypes.data_as(dp), wid.ctypes.data_as(dp), 2, 5.0, 0, None,
                                                               None if "out" in no else out.ctypes.data_as(dp), None)
        return _lib.lib.sr_limb_rays_jac_state_gases_dev(*head, fake, None if "out" in no else fake, None)

    return call, d, out


def test_refused_arguments_return_before_any_device_call_and_leave_the_outputs():
    call, d, out = _calls()
    d1 = _lib.LosDesc()
    C.memmove(C.byref(d1), C.byref(d), C.sizeof(d))
    d1.init_mode = 1
    A, B = (2, 5, 2, [0, 1, 1, 0]), (0, 3, 3, [2, 0, 1, 2])
    refused = [dict(n_lgas=0), dict(n_lgas=-1), dict(n_lgas=5),                                        # n_lgas outside 1 .. n_gas
               dict(gases=[A, B, (1, 2, 2, [0, 0, 0, 0]), (1, 2, 2, [0, 0, 0, 0])]),                   # four for three gases
               dict(gases=[A, (2, 3, 3, [2, 0, 1, 2])]),                                               # a gas named twice
               dict(gases=[A, (3, 3, 3, [2, 0, 1, 2])]), dict(gases=[(-1, 5, 2, [0, 1, 1, 0]), B]),    # a gas out of range
               dict(no=(("tab", 0),)), dict(no=(("tab", 1),)), dict(no=(("coef_row", 0),)), dict(no=(("coef_row", 1),)),
               dict(no=("lgas",)), dict(no=("par_lgas",)), dict(no=("par_level",)), dict(no=("par_c",)),
               dict(par_lgas=[1, 2, 0]), dict(par_lgas=[-1, 0, 0]),                                    # par_lgas out of range
               dict(par_level=[3, 4, 0]), dict(par_level=[2, 5, 0]), dict(par_level=[2, 4, -1]),       # not a level of ITS gas
               dict(gases=[(2, 5, 2, [0, 2, 1, 0]), B]), dict(gases=[A, (0, 3, 3, [2, 0, 3, 2])]),     # coef_row outside ITS tables
               dict(gases=[A, (0, 3, 3, [2, -1, 1, 2])]),
               dict(gases=[(2, 0, 2, [0, 1, 1, 0]), B]), dict(gases=[A, (0, 3, 0, [0, 0, 0, 0])]),     # no levels, no rows
               dict(no=("abs",)), dict(no=("out",)), dict(no=("dabs",)), dict(los=None), dict(los=d1),
               dict(par_gas=[1, 3, 2]), dict(n_lev=-1), dict(n_col=0, n_lev=0, n_row=0)]
    for bands in (False, True):
        for kw in refused:
            assert call(bands, **kw) == _lib.SR_ERR_ARG, (bands, kw)
        assert call(bands, n_pts=2000001) == _lib.SR_ERR_LIMIT
        # more levels than an entry's word holds, with several gases only
        assert call(bands, gases=[(2, 70000, 2, [0, 1, 1, 0]), B]) == _lib.SR_ERR_LIMIT
        # par_level is held against its own gas: level 4 exists in gas A (five levels), not in B (three)
        assert call(bands, par_lgas=[1, 1, 0], par_level=[2, 4, 0]) == _lib.SR_ERR_ARG
        # one level gas is the existing entry, checks and all; a par_lgas that names another gas is refused
        assert call(bands, gases=[A], par_lgas=[0, 1, 0]) == _lib.SR_ERR_ARG
        assert call(bands, gases=[A], par_lgas=[0, 0, 0], par_level=[2, 5, 0]) == _lib.SR_ERR_ARG
        assert call(bands, gases=[A], par_lgas=[0, 0, 0], n_pts=2000001) == _lib.SR_ERR_LIMIT
        assert call(bands, gases=[A], no=("par_lgas",), los=d1) == _lib.SR_ERR_ARG
        # without level parameters the tables are not asked for -- the gases still are
        assert call(bands, n_lev=0, no=(("tab", 0), ("coef_row", 1), "par_lgas", "par_level", "par_c"), n_pts=2000001) == _lib.SR_ERR_LIMIT
        assert call(bands, n_lev=0, gases=[A, (2, 3, 3, [2, 0, 1, 2])]) == _lib.SR_ERR_ARG
    assert np.all(out == SENTINEL)


class _LS(object):
    def __init__(self, n_lev):
        self.iso, self.level_energies = 1, np.arange(float(n_lev))


def _scene():
    from spectrobot_amd import retrieval as rt
    z = np.linspace(100.0, 900.0, 17)
    temps, press = np.linspace(170.0, 150.0, 17), np.geomspace(1.0, 1e-6, 17)
    gases = [rt.LevelGas("HCN", _LS(5), np.full(17, 1e-6), np.full((5, 17), 165.0)),
             rt.Gas("CO", _LS(0), np.full(17, 1e-5)),
             rt.LevelGas("CH4", _LS(12), np.full(17, 1e-2), np.full((12, 17), 160.0), dT=0.05)]
    return rt.LimbScene(np.linspace(3000.0, 3001.0, 11), z, temps, press, gases, [3330.0], [1.0]), z


def _sets(z):
    from spectrobot_amd import retrieval as rt
    return {"CO": smm.LinearProfile_1D_new("CO", z, [200.0, 500.0, 800.0], np.full(3, 1e-5), np.full(3, 1e-5)),
            "CH4": smm.LinearProfile_1D_new("CH4", z, [150.0, 450.0, 600.0, 850.0], np.full(4, 1e-2), np.full(4, 1e-2)),
            "tvib:CH4:5": rt.TvibProfile("CH4", 5, z, [200.0, 400.0, 700.0], np.full(3, 4.0)),
            "tvib:HCN:1": rt.TvibProfile("HCN", 1, z, [250.0, 650.0], np.full(2, 4.0)),
            "temp": rt.TempProfile(z, [150.0, 300.0, 450.0, 600.0, 750.0, 880.0], np.full(6, 3.0)),
            "tvib:CH4:2": rt.TvibProfile("CH4", 2, z, [300.0, 600.0], np.full(2, 4.0)),
            "tvib:HCN:4": rt.TvibProfile("HCN", 4, z, [200.0, 500.0, 800.0], np.full(3, 4.0))}


def test_state_weights_with_the_tvib_sets_of_two_level_gases():
    """Shuffled BayesSets with VMR sets, "temp" and the Tvib sets of two LevelGas: every parameter once, in BayesSet order
    within its kind; par_lgas names the gas of every level parameter; perm leads back to BayesSet order.  The default
    still refuses them."""
    scene, z = _scene()
    sets = _sets(z)
    alt = np.random.default_rng(3).uniform(90.0, 1000.0, 41)
    rng = np.random.default_rng(11)
    n_col, n_lev, n_row = 7, 10, 6
    n_par = n_col + n_lev + n_row
    kind_of = lambda par: 0 if par.nameset in ("CO", "CH4") else (2 if par.nameset == "temp" else 1)
    for _ in range(8):
        order = list(rng.permutation(list(sets)))
        bs = smm.BayesSet()
        for name in order:
            bs.add_set(sets[name])
        with pytest.raises(ValueError, match="more than one gas"):
            scene.state_weights(bs, alt)
        w = scene.state_weights(bs, alt, several_level_gases=True)
        params = bs.params()
        assert w.par_w_col.shape == (n_col, 41) and w.par_w_lev.shape == (n_lev, 17) and w.par_w_temp.shape == (n_row, 17)
        assert w.par_lgas.shape == (n_lev,) and w.par_lgas.dtype == np.int32 and w.par_level.shape == (n_lev,)
        first_named = [n.split(":")[1] for n in order if n.startswith("tvib:")]
        first_named = [n for i, n in enumerate(first_named) if n not in first_named[:i]]
        assert [g.name for g in w.level_gases] == first_named and w.gases == [{"HCN": 0, "CH4": 2}[n] for n in first_named]
        assert w.level_gas is w.level_gases[0] and w.gas == w.gases[0]
        assert sorted(w.perm) == list(range(n_par))
        kinds = [kind_of(p) for p in params]
        first = {0: 0, 1: n_col, 2: n_col + n_lev}
        for k, n in ((0, n_col), (1, n_lev), (2, n_row)):
            assert [w.perm[i] for i, kk in enumerate(kinds) if kk == k] == list(range(first[k], first[k] + n))
        for i, par in enumerate(params):
            q = w.perm[i]
            m = np.asarray(par.maskgrid.mask, float)
            if kinds[i] == 1:
                _, gas, level = par.nameset.split(":")
                assert w.level_gases[w.par_lgas[q - n_col]].name == gas and w.par_level[q - n_col] == int(level)
                assert np.array_equal(w.par_w_lev[q - n_col], m)
            elif kinds[i] == 2:
                assert np.array_equal(w.par_w_temp[q - n_col - n_lev], m)
            else:
                assert scene.gases[w.par_gas[q]].name == par.nameset
        call_rows = np.concatenate([np.zeros(n_col), np.full(n_lev, 1.0), np.full(n_row, 2.0)])
        assert np.array_equal(call_rows[w.perm], np.array(kinds, float))


def test_one_level_gas_gives_the_same_arrays_with_the_keyword_on_and_off():
    from spectrobot_amd import retrieval as rt
    scene, z = _scene()
    sets = _sets(z)
    alt = np.random.default_rng(4).uniform(90.0, 1000.0, 23)
    for names in (["tvib:CH4:5", "CO", "temp", "tvib:CH4:2", "CH4"], ["CO", "tvib:HCN:4"], ["CH4", "temp"], ["CO"]):
        bs = smm.BayesSet()
        for name in names:
            bs.add_set(sets[name])
        off, on = scene.state_weights(bs, alt), scene.state_weights(bs, alt, several_level_gases=True)
        for f in ("par_gas", "par_w_col", "par_level", "par_w_lev", "perm", "par_w_temp", "par_lgas"):
            assert np.array_equal(getattr(off, f), getattr(on, f)) and getattr(off, f).dtype == getattr(on, f).dtype, f
        assert off.level_gas is on.level_gas and off.gas == on.gas and off.gases == on.gases
        assert len(off.level_gases) == len(on.level_gases) <= 1 and all(a is b for a, b in zip(off.level_gases, on.level_gases))
        assert not on.par_lgas.any()
    # StateWeights as existing callers build it: one level gas or none, all level parameters its own
    old = rt.StateWeights(np.zeros(0, np.int32), np.zeros((0, 41)), scene.gas("CH4"), 2, np.array([5, 2], np.int32), np.zeros((2, 17)),
                          np.arange(2))
    assert old.level_gases == [scene.gas("CH4")] and old.gases == [2] and list(old.par_lgas) == [0, 0]
    none = rt.StateWeights(np.zeros(0, np.int32), np.zeros((0, 41)), None, None, np.zeros(0, np.int32), np.zeros((0, 17)), np.zeros(0, int))
    assert none.level_gases == [] and none.gases == [] and none.par_lgas.size == 0
    import inspect
    assert inspect.signature(rt.LimbScene.state_weights).parameters["several_level_gases"].default is False


class _Los(object):
    n_gas, n_rays, n_pt = 3, 2, 9


def test_the_wrappers_refuse_what_does_not_fit(monkeypatch):
    """The ValueErrors of the level_gases / par_lgas keywords are raised by the shared preparation (_state_args), before any
    pointer is formed: plain objects stand for the tensors here."""
    import torch
    from spectrobot_amd import engine
    n_layers, n_pts = 4, 10
    class Co(object):       # ... and of the stacked coefficients
        is_cuda, dtype, shape = True, torch.float64, (3, n_layers, n_pts)
        is_contiguous, dim = (lambda self: True), (lambda self: 3)

    co = (Co(), Co())
    monkeypatch.setattr(engine, "_gas_stack", lambda c: c)     # (no device here to hold real ones)
    row = np.zeros(n_layers, np.int32)

    class Tab(object):      # what _level_gases_args looks at of a table
        is_cuda, dtype, shape = True, torch.float64, (5, 2, 2, n_pts)
        is_contiguous, dim, data_ptr = (lambda self: True), (lambda self: 4), (lambda self: 4096)

    class Short(Tab):
        shape = (5, 2, 2, n_pts - 1)

    class Host(Tab):
        is_cuda = False

    t = Tab()
    pc = np.ones((2, n_layers))
    for fn, lead in ((engine.limb_rays_state_jacobian, ()), (engine.limb_rays_state_bands, (np.linspace(3000.0, 3001.0, n_pts), [3333.0], [1.0]))):
        def call(**kw):
            args = dict(level_gases=[(0, t, row), (2, t, row)], par_lgas=[0, 1], par_level=[1, 4], par_c=pc)
            args.update(kw)
            return fn(co, _Los(), *lead, **args)
        for kw, text in ((dict(par_lgas=None), "needs par_lgas"), (dict(tab=t), "no tab / coef_row"), (dict(coef_row=row), "no tab / coef_row"),
                         (dict(level_gases=[]), "0 level gases"), (dict(level_gases=[(0, t, row)] * 4), "4 level gases"),
                         (dict(level_gases=[(0, t, row), (0, t, row)]), "named twice"), (dict(level_gases=[(0, t, row), (3, t, row)]), "out of range"),
                         (dict(level_gases=[(0, t, row), (2, Short(), row)]), "tables of 9 points"),
                         (dict(level_gases=[(0, t, row), (2, Host(), row)]), "level gas 1: its tables must be"),
                         (dict(level_gases=[(0, t, row), (2, t, row[:3])]), "coef_row must be"),
                         (dict(par_lgas=[0, 1, 1]), "par_lgas must be"), (dict(par_lgas=[0, 2]), "par_lgas out of range"),
                         (dict(par_lgas=[-1, 0]), "par_lgas out of range"), (dict(par_c=None), "need par_c"),
                         (dict(par_c=np.ones((3, n_layers))), "par_c must be"), (dict(par_level=[1, 5]), "par_level out of range"),
                         (dict(dcoeffs=co), "both dcoeffs and par_t")):
            with pytest.raises(ValueError, match=text):
                call(**kw)
        with pytest.raises(ValueError, match="belongs to level_gases"):
            fn(co, _Los(), *lead, par_lgas=[0, 1], par_level=[1, 4], par_c=pc, tab=t, coef_row=row)
    with pytest.raises(ValueError, match="at least one"):
        engine.LevelFactoredSet([])


def test_level_factored_set_forms_par_c_per_member_and_refuses_mismatches(monkeypatch):
    """LevelFactoredSet hands limb_rays_state_jacobian each member's (gas, tab, step_row) and a par_c whose rows are the
    member's own _state_level_args rows (the populations' Tvib derivative times the node weights), in the caller's order."""
    from spectrobot_amd import engine

    class LS(object):
        def __init__(self, n_lev, f):
            self.level_energies, self.f = np.arange(float(n_lev)), f

        def level_populations_dtvib(self, temps, tvib, q_part=None):
            return self.f * np.outer(temps, 1.0 + np.arange(self.level_energies.size)) + np.asarray(tvib).T

    def member(n_lev, f, shard=(0, None)):
        lf = engine.LevelFactored.__new__(engine.LevelFactored)
        lf.ls, lf.temps, lf._shard, lf.tab = LS(n_lev, f), np.linspace(150.0, 170.0, 3), shard, object()
        return lf

    a, b = member(5, 1.0), member(3, -2.0)
    rows_a, rows_b = np.array([0, 1, 2, 1], np.int32), np.array([2, 2, 0, 1], np.int32)
    tv_a, tv_b = np.full((5, 4), 3.0), np.arange(12.0).reshape(3, 4)
    S = engine.LevelFactoredSet([(a, 2, rows_a, tv_a), (b, 0, rows_b, tv_b)])
    seen = {}
    monkeypatch.setattr(engine, "limb_rays_state_jacobian", lambda *x, **k: seen.update(k) or "out")
    par_lgas, par_level = [1, 0, 1, 0], [2, 4, 0, 0]
    w = np.random.default_rng(2).uniform(0.1, 1.0, (4, 4))
    assert S.state_jacobian("co", "los", par_lgas, par_level, w, par_gas=[1], par_w_col="pw", want_rad=False) == "out"
    assert [g[0] for g in seen["level_gases"]] == [2, 0] and seen["level_gases"][0][1] is a.tab and seen["level_gases"][1][1] is b.tab
    assert np.array_equal(seen["level_gases"][1][2], rows_b) and list(seen["par_lgas"]) == par_lgas and list(seen["par_level"]) == par_level
    assert seen["par_gas"] == [1] and seen["par_w"] == "pw" and seen["want_rad"] is False and seen["g_lo"] == 0
    for p, (k, L) in enumerate(zip(par_lgas, par_level)):
        lf, rows, tv = ((a, rows_a, tv_a), (b, rows_b, tv_b))[k]
        _, _, one = lf._state_level_args(rows, tv, [L], w[p:p + 1], None)
        assert np.array_equal(seen["par_c"][p], one[0])
    for kw, text in ((dict(par_lgas=[0, 2, 0, 0]), "par_lgas out of range"), (dict(par_lgas=[0, 1]), "par_lgas must be"),
                     (dict(par_level=[2, 4, 3, 0]), "par_level out of range"), (dict(w=w[:, :3]), "par_w_level must be")):
        args = dict(par_lgas=par_lgas, par_level=par_level, w=w)
        args.update(kw)
        with pytest.raises(ValueError, match=text):
            S.state_jacobian("co", "los", args["par_lgas"], args["par_level"], args["w"])
    with pytest.raises(ValueError, match="share their spectral shard"):
        engine.LevelFactoredSet([(a, 2, rows_a, tv_a), (member(3, 1.0, shard=(5, 9)), 0, rows_b, tv_b)])
    with pytest.raises(ValueError, match="named twice"):
        engine.LevelFactoredSet([(a, 2, rows_a, tv_a), (b, 2, rows_b, tv_b)])
    with pytest.raises(ValueError, match="one length"):
        engine.LevelFactoredSet([(a, 2, rows_a, tv_a), (b, 0, rows_b[:3], tv_b[:, :3])]).state_jacobian("co", "los", [1], [0], w[:1])
