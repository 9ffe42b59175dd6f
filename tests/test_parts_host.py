"""Host side of the radiance budget (no GPU): the ABI surface of sr_limb_rays_parts_dev, its argument checks -- all of
them made before any device call, so they answer on a machine without a GPU --, smm.track_all_levels and the key / tag
bookkeeping of radtrans' single_rads."""
import ctypes as C

import numpy as np
import pytest

from spectrobot_amd import _lib
from spectrobot_amd import spect_main_module as smm


def test_abi_surface_of_the_parts_call():
    res, args = _lib.SYMBOLS["sr_limb_rays_parts_dev"]
    assert res is C.c_int and len(args) == 17
    assert args[4] == C.POINTER(_lib.LosDesc) and args[3] is C.c_int64
    assert hasattr(_lib.lib, "sr_limb_rays_parts_dev")
    assert _lib.lib.sr_abi_version() == 1


def test_refused_arguments_return_before_any_device_call():
    """Every refused argument returns SR_ERR_ARG from the host checks (the buffers below are not device memory: a call
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
    pg = np.array([1, 1, 0, 1], np.int32)
    pl = np.array([0, 2, -1, -1], np.int32)
    pc = np.ones((4, n_layers))

    def call(**kw):
        dd = kw.get("los", d)
        r = np.ascontiguousarray(kw.get("coef_row", row), dtype=np.int32)
        g = np.ascontiguousarray(kw.get("part_gas", pg), dtype=np.int32)
        lv = np.ascontiguousarray(kw.get("part_level", pl), dtype=np.int32)
        return _lib.lib.sr_limb_rays_parts_dev(
            fake, fake, n_layers, n_pts, C.byref(dd) if dd is not None else None, kw.get("gas", 1),
            None if kw.get("no_tab") else fake, n_levels, n_rows, None if kw.get("no_row") else r.ctypes.data_as(ip),
            kw.get("n_part", 4), g.ctypes.data_as(ip), lv.ctypes.data_as(ip),
            None if kw.get("no_c") else pc.ctypes.data_as(dp), fake, None if kw.get("no_parts") else fake, None)

    d1 = _lib.LosDesc()
    C.memmove(C.byref(d1), C.byref(d), C.sizeof(d))
    d1.init_mode = 1
    refused = [dict(no_parts=True), dict(n_part=0), dict(n_part=-3),
               dict(part_level=[0, n_levels, -1, -1]), dict(part_level=[0, 2, -2, -1]),      # level out of range
               dict(part_gas=[1, 0, 0, 1]), dict(gas=0),                                      # level part of another gas
               dict(no_tab=True), dict(no_row=True), dict(no_c=True),                         # level parts without tables
               dict(part_gas=[1, 1, 2, 1]), dict(part_gas=[1, 1, -1, 1]),                     # part_gas out of range
               dict(coef_row=[0, 1, n_rows, 0]), dict(coef_row=[-1, 1, 1, 0]),                # coef_row out of range
               dict(los=d1), dict(los=None)]
    for kw in refused:
        assert call(**kw) == _lib.SR_ERR_ARG, kw


def test_track_all_levels_on_a_two_gas_scene():
    """The stand-in scene (a list of gases with line sets) and the reference's planet (dicts of molecules, all_iso,
    .levels per iso-molecule, spect_main_module.py:151-159)."""
    from spectrobot_amd import retrieval as rt

    class _LS(object):
        def __init__(self, iso, n_lev):
            self.iso, self.level_energies = iso, np.arange(float(n_lev))

    class _Scene(object):
        gases = [rt.Gas("CO", _LS(1, 0), [1e-4]), rt.Gas("CH4", _LS(2, 12), [1e-2])]

    tl = smm.track_all_levels(_Scene())
    assert list(tl) == [("CO", "iso_1"), ("CH4", "iso_2")]
    assert tl[("CO", "iso_1")] == [] and tl[("CH4", "iso_2")] == ["lev_%02d" % i for i in range(12)]

    class _Iso(object):
        levels = ["lev_00", "lev_01"]

    class _Mol(object):
        all_iso = ["iso_1"]
        iso_1 = _Iso()

    class _Planet(object):
        gases = {"HCN": _Mol()}

    assert smm.track_all_levels(_Planet()) == {("HCN", "iso_1"): ["lev_00", "lev_01"]}


def test_keys_and_tags_of_single_rads():
    from spectrobot_amd import retrieval as rt

    class _LS(object):
        def __init__(self, iso, n_lev):
            self.iso, self.level_energies = iso, np.arange(float(n_lev))

    gases = [rt.Gas("CO", _LS(1, 0), [1e-4]), rt.Gas("CH4", _LS(1, 12), [1e-2])]
    keys = rt.single_rad_keys(gases, {("CH4", "iso_1"): ["lev_03", 7]})
    assert keys == [(("CO", "iso_1"), 0, None), (("CH4", "iso_1"), 1, None), (("CH4", "iso_1", "lev_03"), 1, 3),
                    (("CH4", "iso_1", 7), 1, 7)]
    assert [k for k, _, _ in rt.single_rad_keys(gases)] == [("CO", "iso_1"), ("CH4", "iso_1")]
    with pytest.raises(ValueError):
        rt.single_rad_keys(gases, {("CH4", "iso_1"): [12]})
    with pytest.raises(ValueError):
        rt.single_rad_keys(gases, {("CO", "iso_1"): [0]})          # no levels at all
    with pytest.raises(ValueError):
        rt.single_rad_keys(gases, {("HCN", "iso_1"): []})
    with pytest.raises(ValueError):
        rt.single_rad_keys(gases, {("CH4", "iso_1"): ["level3"]})
    tags = rt.los_tags(3)
    assert tags == ["LOS00", "LOS01", "LOS02"]
    bands = np.array([3300.0, 3310.0])
    low = np.arange(5 * 3 * 2, dtype=float).reshape(5, 3, 2)
    radtrans, single = rt.pack_single_rads(keys, tags, low, bands)
    assert sorted(radtrans) == tags and list(single) == [k for k, _, _ in keys]
    assert np.array_equal(radtrans["LOS01"].spectrum, low[0, 1])
    assert np.array_equal(single[("CH4", "iso_1", 7)]["LOS02"].spectrum, low[4, 2])
    assert np.array_equal(single[("CO", "iso_1")]["LOS00"].spectrum, low[1, 0])
    assert np.array_equal(radtrans["LOS00"].spectral_grid.grid, bands)
    with pytest.raises(ValueError):
        rt.pack_single_rads(keys, tags, low[:4], bands)
