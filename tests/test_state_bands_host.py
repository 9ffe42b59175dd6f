"""Host side of the state Jacobian on the instrument's bands (no GPU): the ABI surface of sr_limb_rays_state_bands_dev,
its argument checks -- all of them made before any device call, so they answer on a machine without a GPU and leave the
host output untouched --, and the refusals the two Python wrappers share with limb_rays_state_jacobian / state_jacobian
(those that are reached before a device tensor is looked at; the rest: tests/test_gpu_state_bands.py)."""
import ctypes as C

import numpy as np
import pytest

from spectrobot_amd import _lib

N_HEAD = 20          # the arguments of sr_limb_rays_jac_state_rows_dev up to par_t


def test_abi_surface_of_the_bands_call():
    res, args = _lib.SYMBOLS["sr_limb_rays_state_bands_dev"]
    ip, dp, vp, ci = _lib.ip, _lib.dp, C.c_void_p, C.c_int
    assert res is C.c_int
    rows = list(_lib.SYMBOLS["sr_limb_rays_jac_state_rows_dev"][1])
    assert len(rows) == N_HEAD + 3 and rows[N_HEAD - 2:N_HEAD] == [ci, dp]       # ..., n_row, par_t | rad, jac, stream
    assert list(args[:N_HEAD]) == rows[:N_HEAD]
    assert list(args[N_HEAD:]) == [dp, dp, ci, C.c_double, ci,                   # centers_nm, widths_nm, n_bands, n_sigma, out_units
                                   dp, dp, vp]                                   # fov, out, stream
    assert hasattr(_lib.lib, "sr_limb_rays_state_bands_dev")
    assert _lib.lib.sr_abi_version() == 1


def test_refused_arguments_return_before_any_device_call_and_leave_out_untouched():
    """Every refused argument returns its status from the host checks (the buffers below are not device memory: a call
    that got as far as a copy or a launch would not return a status of its own), and `out` keeps its sentinel."""
    ip, dp = _lib.ip, _lib.dp
    n_layers, n_pts, n_levels, n_rows, n_bands = 4, 10, 3, 2, 3
    SENT = -7.25
    so3, sl3, po3 = np.array([0, 2, 4, 6], np.int32), np.array([1, 3, 1, 3, 2, 3], np.int32), np.arange(0, 13, 2, dtype=np.int32)
    so2, sl2, po2 = so3[:3].copy(), sl3[:4].copy(), po3[:5].copy()
    xx = np.tile([0.0, 1.0], 6)
    one = np.ones(24)

    def desc(n_rays=3, step=5e-4, w0=3000.0, g_lo=0, init_mode=0):
        d = _lib.LosDesc()
        d.n_rays, d.n_gas = n_rays, 2
        arrs = (so3, sl3, po3) if n_rays == 3 else (so2, sl2, po2)
        d.seg_off, d.seg_layer, d.pt_off = (a.ctypes.data_as(ip) for a in arrs)
        d.x, d.nd, d.vmr = xx.ctypes.data_as(dp), one.ctypes.data_as(dp), one.ctypes.data_as(dp)
        d.w0, d.step, d.g_lo, d.init_mode = w0, step, g_lo, init_mode
        return d

    d = desc()
    n_pt = 12
    fake = C.c_void_p(4096)               # stands for a device buffer: never dereferenced by a refused call
    row = np.array([0, 1, 1, 0], np.int32)
    pg = np.array([1, 0, 1], np.int32)
    pw = np.ones((3, n_pt))
    pl = np.array([0, 2], np.int32)
    pc = np.ones((2, n_layers))
    pt = np.ones((2, n_layers))
    cen = np.array([3331.0, 3332.0, 3333.0])
    wid = np.array([0.5, 0.5, 0.5])
    fov = np.ones((1, 7))
    out = np.full((3, 1 + 7, n_bands), SENT)

    def call(**kw):
        dd = kw.get("los", d)
        r = np.ascontiguousarray(kw.get("coef_row", row), dtype=np.int32)
        g = np.ascontiguousarray(kw.get("par_gas", pg), dtype=np.int32)
        lv = np.ascontiguousarray(kw.get("par_level", pl), dtype=np.int32)
        w = np.ascontiguousarray(kw.get("widths", wid), dtype=np.float64)
        no = kw.get("no", ())
        return _lib.lib.sr_limb_rays_state_bands_dev(
            None if "abs" in no else fake, None if "emi" in no else fake, n_layers, kw.get("n_pts", n_pts),
            C.byref(dd) if dd is not None else None, kw.get("n_col", 3), None if "par_gas" in no else g.ctypes.data_as(ip),
            None if "par_w" in no else pw.ctypes.data_as(dp), kw.get("gas", 1), None if "tab" in no else fake,
            kw.get("n_levels", n_levels), kw.get("n_rows", n_rows), None if "coef_row" in no else r.ctypes.data_as(ip),
            kw.get("n_lev", 2), None if "par_level" in no else lv.ctypes.data_as(ip),
            None if "par_c" in no else pc.ctypes.data_as(dp), None if "dabs" in no else fake, None if "demi" in no else fake,
            kw.get("n_row", 2), None if "par_t" in no else pt.ctypes.data_as(dp),
            None if "centers" in no else cen.ctypes.data_as(dp), None if "widths" in no else w.ctypes.data_as(dp),
            kw.get("n_bands", n_bands), kw.get("n_sigma", 5.0), kw.get("out_units", 0),
            fov.ctypes.data_as(dp) if kw.get("fov", False) else None, None if "out" in no else out.ctypes.data_as(dp), None)

    refused = [dict(no=("abs",)), dict(no=("emi",)), dict(los=None),                                      # NULLs
               dict(no=("par_gas",)), dict(no=("par_w",)), dict(no=("tab",)), dict(no=("coef_row",)),
               dict(no=("par_level",)), dict(no=("par_c",)),
               dict(no=("dabs",)), dict(no=("demi",)), dict(no=("par_t",)),                               # ... of the third kind
               dict(n_col=-1), dict(n_lev=-1), dict(n_row=-1), dict(n_levels=0), dict(n_rows=0),          # negative counts
               dict(n_col=0, n_lev=0, n_row=0),                                                           # no parameters at all
               dict(par_gas=[1, 2, 1]), dict(par_gas=[-1, 0, 1]),                                         # par_gas out of range
               dict(par_level=[0, n_levels]), dict(par_level=[-1, 2]),                                    # par_level out of range
               dict(coef_row=[0, 1, n_rows, 0]), dict(coef_row=[-1, 1, 1, 0]),                            # coef_row out of range
               dict(gas=2), dict(gas=-1),                                                                 # gas out of range
               dict(los=desc(init_mode=1)),                                                               # init_mode 1
               # the band side
               dict(n_bands=0), dict(n_bands=-1), dict(no=("centers",)), dict(no=("widths",)), dict(no=("out",)),
               dict(widths=[0.5, 0.0, 0.5]), dict(widths=[0.5, 0.5, -1.0]), dict(widths=[np.nan, 0.5, 0.5]),
               dict(out_units=-1), dict(out_units=3), dict(n_sigma=0.0), dict(n_sigma=-5.0),
               dict(n_pts=1),                                                                             # no trapezoid
               dict(los=desc(step=0.0)), dict(los=desc(step=-5e-4)), dict(los=desc(w0=0.0)),              # no grid
               dict(los=desc(g_lo=-1)),
               dict(los=desc(n_rays=2), fov=True)]                                                        # fov: three rays per pixel
    for kw in refused:
        assert call(**kw) == _lib.SR_ERR_ARG, kw
    assert call(n_pts=2000001) == _lib.SR_ERR_LIMIT
    assert call(n_pts=2000001, n_col=0, n_lev=0, no=("par_gas", "par_w", "tab", "coef_row", "par_level", "par_c")) == _lib.SR_ERR_LIMIT
    assert call(los=desc(g_lo=1999995)) == _lib.SR_ERR_LIMIT                   # the shard's end beyond the limit
    # an empty kind needs none of its arrays -- but the other kinds are still checked
    assert call(n_lev=0, no=("tab", "coef_row", "par_level", "par_c"), par_gas=[0, 0, 2]) == _lib.SR_ERR_ARG
    assert call(n_col=0, no=("par_gas", "par_w"), par_level=[0, 3]) == _lib.SR_ERR_ARG
    assert call(n_col=0, n_lev=0, no=("par_gas", "par_w", "tab", "coef_row", "par_level", "par_c", "dabs")) == _lib.SR_ERR_ARG
    # n_row = 0 needs no dabs_c / demi_c / par_t: the other checks answer
    assert call(n_row=0, no=("dabs", "demi", "par_t"), gas=2) == _lib.SR_ERR_ARG
    assert call(n_row=0, no=("dabs", "demi", "par_t"), n_pts=2000001) == _lib.SR_ERR_LIMIT
    assert call(n_row=0, no=("dabs", "demi", "par_t"), los=desc(init_mode=1)) == _lib.SR_ERR_ARG
    assert call(n_row=0, no=("dabs", "demi", "par_t"), n_bands=0) == _lib.SR_ERR_ARG
    assert call(n_row=0, no=("dabs", "demi", "par_t"), los=desc(step=0.0)) == _lib.SR_ERR_ARG
    assert np.all(out == SENT)


def test_row_parameters_need_both_arguments_in_the_bands_call_too():
    """The first refusal of limb_rays_state_jacobian, made before anything else is looked at, is the bands call's too."""
    from spectrobot_amd import engine
    grid, cen, wid = np.linspace(3000.0, 3001.0, 11), [3331.0], [0.5]
    for kw in (dict(dcoeffs=(None, None)), dict(par_t=np.ones((2, 4)))):
        with pytest.raises(ValueError, match="both dcoeffs and par_t") as e_jac:
            engine.limb_rays_state_jacobian(None, None, **kw)
        with pytest.raises(ValueError, match="both dcoeffs and par_t") as e_bands:
            engine.limb_rays_state_bands(None, None, grid, cen, wid, **kw)
        assert str(e_bands.value) == str(e_jac.value)


class _LS(object):
    def __init__(self, n_lev):
        self.iso, self.level_energies = 1, np.arange(float(n_lev))


def test_level_factored_wrappers_refuse_the_same_shapes():
    """LevelFactored.state_bands forms par_c through the helper state_jacobian uses: the same ValueErrors for the same bad
    level arguments (raised before any table or device tensor is touched)."""
    from spectrobot_amd import engine
    lf = object.__new__(engine.LevelFactored)
    lf.ls, lf._shard, lf.tab, lf.temps = _LS(5), (0, None), None, np.full(4, 200.0)
    grid, cen, wid = np.linspace(3000.0, 3001.0, 11), [3331.0], [0.5]
    rows = np.array([0, 1, 2, 3], np.int32)
    bad = [((rows, None, [0, 1], np.ones((2, 3))), "par_w_level must be"),        # n_steps wrong
           ((rows, None, [0, 1], np.ones((3, 4))), "par_w_level must be"),        # n_lev wrong
           ((rows, None, [0, 5], np.ones((2, 4))), "par_level out of range"),
           ((rows, None, [-1, 2], np.ones((2, 4))), "par_level out of range")]
    for args, msg in bad:
        with pytest.raises(ValueError, match=msg) as e_jac:
            lf.state_jacobian(None, None, *args)
        with pytest.raises(ValueError, match=msg) as e_bands:
            lf.state_bands(None, None, *args, grid, cen, wid)
        assert str(e_bands.value) == str(e_jac.value)
    # ... and the refusal of the call underneath comes through both
    for kw in (dict(dcoeffs=(None, None)), dict(par_w_temp=np.ones((2, 4)))):
        with pytest.raises(ValueError, match="both dcoeffs and par_t"):
            lf.state_jacobian(None, None, rows, None, [], None, **kw)
        with pytest.raises(ValueError, match="both dcoeffs and par_t"):
            lf.state_bands(None, None, rows, None, [], None, grid, cen, wid, **kw)


def test_inversion_state_has_the_switch_and_it_is_off():
    import inspect
    from spectrobot_amd import retrieval as rt
    assert inspect.signature(rt.inversion_state).parameters["bands_in_kernel"].default is False
