"""Host side of the pointing derivative (no GPU): the extended-precision geometry reference of tests/pointing_reference.py
against differences of rebuilt geometry, geometry.limb_los(path=True) against that reference, the recorded yardstick
constant, the Pointing retrieval set (construction, refusals by the drivers that have no pointing row, placement of its
Jacobian column beside an "instr" set) and the new library entries' refusals, which all come before the first copy or
launch: the tables and outputs below are not device memory."""
import ctypes as C

import numpy as np
import pytest

import pointing_reference as P

from spectrobot_amd import _lib, geometry

ARG, LIMIT, UNSUPPORTED = _lib.SR_ERR_ARG, _lib.SR_ERR_LIMIT, _lib.SR_ERR_UNSUPPORTED


# ------------------------------------------------------------------------------------------------------------------
# the reference
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("zt", P.Z_TANS)
def test_analytic_dcol_against_extrapolated_differences(zt):
    """The long double analytic d col / d z_t against Richardson-extrapolated long double central differences of rebuilt
    geometry (shells held fixed): within 4 x the extrapolation's own error estimate, the difference of its values at two
    step sizes, per gas in the largest |d col| of the ray."""
    G, _ = P.ray_case(zt)
    ref = P.dcol_reference(G)
    value, estimate = P.richardson(zt, P.RICHARDSON_STEP[zt])
    scale = np.abs(ref).max(axis=1)
    err = np.asarray(np.abs(ref - value).max(axis=1) / scale, float)
    est = np.asarray(estimate.max(axis=1) / scale, float)
    print("\nz_t %.2f km, first step %g km: analytic - extrapolated %s, the extrapolation's estimate %s"
          % (zt, P.RICHARDSON_STEP[zt], err, est))
    assert np.all(np.abs(ref).max(axis=1) > 0) and np.all(est < 1e-9)      # (an estimate that supports a real statement)
    assert np.all(err <= 4.0 * est), (err, est)


def test_dcol_is_zero_without_path_derivatives_and_finite_on_a_flat_segment():
    _, F = P.ray_case(260.0)
    zero = np.zeros_like(F["dx"])
    for dtype in (P.LD, np.float64):
        assert np.all(P.dcol_forward(F["x"], F["nd"], F["vmr"], F["alt"], zero, zero, dtype) == 0.0)
        flat = F["alt"].copy()
        flat[0, :] = flat[0, 0]                                            # alt_last == alt_first: zero slopes, no NaN
        assert np.all(np.isfinite(np.asarray(P.dcol_forward(F["x"], F["nd"], F["vmr"], flat, F["dx"], F["dalt"], dtype), float)))


def test_recorded_yardstick_constant():
    k, rows = P.measure_k_plain_dcol()
    for zt, d in rows:
        print("\nz_t %.2f km: plain fp64 d col against the reference, per gas %s" % (zt, d))
    print("K_PLAIN_DCOL live %.3g, recorded %.3g (measured %.3g)" % (k, P.K_PLAIN_DCOL, P.K_PLAIN_DCOL_MEASURED))
    assert k <= P.K_PLAIN_DCOL
    assert P.K_PLAIN_DCOL <= 2.0 * P.K_PLAIN_DCOL_MEASURED


# ------------------------------------------------------------------------------------------------------------------
# geometry.limb_los(path=True)
# ------------------------------------------------------------------------------------------------------------------
def _within_ulps(got, ref_ld, n):
    ref = np.asarray(ref_ld, np.float64)
    return np.all(np.abs(got - ref) <= n * np.spacing(np.abs(ref)))


def test_limb_los_path_against_the_reference():
    z, nd, vmr = P.case_profiles()
    L = geometry.limb_los(z, nd, vmr, P.Z_TANS, R=P.R_KM, n_sub=P.N_SUB, path=True)
    los, path, rays = P.batch_inputs()
    assert np.array_equal(L["seg_off"], los["seg_off"]) and np.array_equal(L["seg_layer"], los["seg_layer"])
    assert L["dx_dzt"].shape == L["dalt_dzt"].shape == L["x"].shape
    dx = np.concatenate([np.asarray(G["dx"]).reshape(-1) for G in rays])
    dalt = np.concatenate([np.asarray(G["dalt"]).reshape(-1) for G in rays])
    u = lambda got, ref: float(np.nanmax(np.abs(got - np.asarray(ref, float)) / np.spacing(np.abs(np.asarray(ref, float)))))
    print("\nlimb_los(path=True): dx_dzt %.1f ulp, dalt_dzt %.1f ulp from the reference" % (u(L["dx_dzt"], dx), u(L["dalt_dzt"], dalt)))
    assert _within_ulps(L["dx_dzt"], dx, 16) and _within_ulps(L["dalt_dzt"], dalt, 16)
    # 0 on the shell boundaries, 1 at the tangent points, exactly
    ends = np.zeros(L["x"].size, bool)
    ends[L["pt_off"][:-1]] = ends[L["pt_off"][1:] - 1] = True
    tangent = L["x"] == 0.0
    assert tangent.sum() == 2 * len(P.Z_TANS)
    assert np.all(L["dalt_dzt"][ends & ~tangent] == 0.0) and np.all(L["dalt_dzt"][tangent] == 1.0)
    assert np.all(L["dx_dzt"][tangent] == 0.0)
    # the path itself is the one the derivatives belong to (x to the conditioning of sqrt(hi^2 - r_t^2) in fp64)
    assert np.allclose(L["x"], los["x"], rtol=0, atol=1e-12 * np.abs(los["x"]).max())


def _limb_los_before(z, nd_levels, vmr_levels, z_tans, R, n_sub):
    """limb_los as it stood before `path`, restated from the module's own pieces."""
    z, zz, ln, vv = geometry._profiles(z, nd_levels, vmr_levels)
    seg_off, lay, xs, alts = [0], [], [], []
    for zt in np.atleast_1d(np.asarray(z_tans, float)):
        k, a, b = geometry._limb_crossings(zz, zt, R)
        s = geometry._sample(a, b, n_sub)
        lay.append(k)
        xs.append(s.ravel())
        alts.append((np.sqrt(s * s + (R + zt) ** 2) - R).ravel())
        seg_off.append(seg_off[-1] + len(k))
    n_seg = seg_off[-1]
    alts = np.clip(np.concatenate(alts), z[0], zz[-1])
    return dict(seg_off=np.array(seg_off, np.int32), seg_layer=np.concatenate(lay).astype(np.int32),
                pt_off=(np.arange(n_seg + 1) * (n_sub + 1)).astype(np.int32), x=np.concatenate(xs) * 1e5,
                nd=np.exp(np.interp(alts, zz, ln)), vmr=np.array([np.interp(alts, zz, v) for v in vv]), alt=alts)


def test_limb_los_without_path_is_unchanged():
    z, nd, vmr = P.case_profiles()
    for first in (False, True):          # (whichever of the two fills the geometry cache)
        geometry._LOS_GEOMETRY.clear()
        geometry._LOS_PATH.clear()
        if first:
            geometry.limb_los(z, nd, vmr, P.Z_TANS, R=P.R_KM, n_sub=P.N_SUB, path=True)
        L = geometry.limb_los(z, nd, vmr, P.Z_TANS, R=P.R_KM, n_sub=P.N_SUB)
        before = _limb_los_before(z, nd, vmr, P.Z_TANS, P.R_KM, P.N_SUB)
        assert sorted(L) == sorted(before)
        for key in before:
            assert L[key].dtype == before[key].dtype and np.array_equal(L[key], before[key]), key
        with_path = geometry.limb_los(z, nd, vmr, P.Z_TANS, R=P.R_KM, n_sub=P.N_SUB, path=True)
        assert sorted(with_path) == sorted(list(before) + ["dx_dzt", "dalt_dzt"])
        for key in before:
            assert np.array_equal(with_path[key], before[key]), key


# ------------------------------------------------------------------------------------------------------------------
# the Pointing set
# ------------------------------------------------------------------------------------------------------------------
def test_pointing_set_construction():
    from spectrobot_amd import retrieval, spect_main_module as smm
    p = retrieval.Pointing((0.0, 2.0))
    assert p.name == retrieval.POINTING_SET == "pointing" and p.n_par == 1 and p.offset() == 0.0
    assert p.set[0].key == "offset" and not p.set[0].constrain_positive and p.set[0].apriori_err == 2.0
    assert retrieval.Pointing((0.0, 2.0, 0.7)).offset() == 0.7
    for bad in ((1.0,), (1.0, 2.0, 3.0, 4.0)):
        with pytest.raises(ValueError):
            retrieval.Pointing(bad)
    bs = smm.BayesSet()
    bs.add_set(p)
    assert [par.nameset for par in bs.params()] == ["pointing"]


def test_the_other_drivers_refuse_the_set():
    from spectrobot_amd import retrieval, spect_main_module as smm
    bs = smm.BayesSet()
    bs.add_set(retrieval.Pointing((0.0, 2.0)))
    for driver in (retrieval.simulate, retrieval.inversion_fast_limb, retrieval.inversion):
        with pytest.raises(ValueError, match="pointing"):
            driver(None, [], bs) if driver is retrieval.simulate else driver(None, bs, [])


def test_state_weights_skips_the_set():
    from spectrobot_amd import retrieval, spect_main_module as smm
    scene = retrieval.LimbScene.__new__(retrieval.LimbScene)
    scene.z, scene.gases = np.linspace(100.0, 500.0, 9), []
    bs = smm.BayesSet()
    bs.add_set(retrieval.Pointing((0.0, 2.0)))
    bs.add_set(retrieval.BandCalibration(shift=(0.0, 1.0)))
    w = scene.state_weights(bs, np.zeros(3))
    assert len(w.perm) == 0 and w.par_w_col.shape == (0, 3) and w.par_w_temp.shape[0] == 0


def test_the_pointing_column_stands_where_the_set_stands():
    """A stub Jacobian: rows [radiance, 3 profile rows, pointing row, d / d centre, d / d ln width] of two pixels on four
    bands, for a BayesSet ordered (profile a, pointing, instr shift + ln_width, profiles b, c)."""
    from spectrobot_amd import retrieval
    instr = retrieval.BandCalibration(shift=(0.0, 1.0), ln_width=(0.0, 0.1))
    bands0 = np.array([1000.0, 1010.0, 1020.0, 1030.0])
    rows = np.arange(2 * 7 * 4, dtype=float).reshape(2, 7, 4) + 0.5
    is_point = np.array([0, 1, 0, 0, 0, 0], bool)
    is_instr = np.array([0, 0, 1, 1, 0, 0], bool)
    out = retrieval._rows_in_bayes_order(rows, 3, is_point, is_instr, instr, bands0)
    assert out.shape == (2, 7, 4)
    assert np.array_equal(out[:, 0], rows[:, 0])
    assert np.array_equal(out[:, 1], rows[:, 1]) and np.array_equal(out[:, 5], rows[:, 2]) and np.array_equal(out[:, 6], rows[:, 3])
    assert np.array_equal(out[:, 2], rows[:, 4])                                  # the pointing row
    assert np.array_equal(out[:, 3:5], instr.jacobian_rows(bands0, rows[:, 5], rows[:, 6]))
    # the pointing set alone, and without any instrument rows
    alone = retrieval._rows_in_bayes_order(rows[:, :5], 3, np.array([1, 0, 0, 0], bool), np.zeros(4, bool), None, bands0)
    assert np.array_equal(alone[:, 1], rows[:, 4]) and np.array_equal(alone[:, 2:], rows[:, 1:4])


# ------------------------------------------------------------------------------------------------------------------
# the library entries
# ------------------------------------------------------------------------------------------------------------------
N_LAYERS, N_PTS = 4, 10
FAKE = C.c_void_p(4096)    # stands for a device buffer: never dereferenced by a refused call
_SO, _SL, _PO = np.array([0, 2], np.int32), np.array([1, 3], np.int32), np.array([0, 2, 4], np.int32)
_X, _ONE = np.array([0.0, 1.0, 1.0, 2.0]), np.ones(8)
_PAR_W = np.ones((2, 4))
_BANDS, _WIDTHS = np.array([3000.0, 3001.0]), np.array([0.5, 0.5])


def _los(kw):
    if kw.get("no_los"):
        return None, None
    seg_layer = np.ascontiguousarray(kw.get("seg_layer", _SL), dtype=np.int32)
    d = _lib.LosDesc()
    d.n_rays, d.n_gas, d.init_mode, d.los_order = 1, 2, kw.get("init_mode", 0), kw.get("los_order", 0)
    d.w0, d.step = 2000.0, 0.001
    d.seg_off, d.seg_layer, d.pt_off = (a.ctypes.data_as(_lib.ip) for a in (_SO, seg_layer, _PO))
    d.x, d.nd, d.vmr = (a.ctypes.data_as(_lib.dp) for a in (_X, _ONE, _ONE))
    return d, seg_layer


def _path(kw):
    if kw.get("no_path"):
        return None
    p = _lib.LosPath()
    p.alt, p.dx_dz, p.dalt_dz = (None if kw.get("no_" + name) else _ONE.ctypes.data_as(_lib.dp) for name in ("alt", "dx", "dalt"))
    return p


def _state(kw):
    d, keep = _los(kw)
    p = _path(kw)
    tab = None if kw.get("no_tab") else FAKE
    pg = np.ascontiguousarray(kw.get("par_gas", [0, 1]), dtype=np.int32)
    lgas = (_lib.LevelGasDesc * 1)()
    lgas[0].gas = kw.get("level_gas", 0)
    head = (tab, tab, N_LAYERS, kw.get("n_pts", N_PTS), None if d is None else C.byref(d), kw.get("n_col", 2),
            pg.ctypes.data_as(_lib.ip), _PAR_W.ctypes.data_as(_lib.dp), 1, lgas, 0, None, None, None, None, None, 0, None)
    return head, None if p is None else C.byref(p), (d, keep, p, pg, lgas)


def jac_state_path(**kw):
    head, path, _keep = _state(kw)
    return _lib.lib.sr_limb_rays_jac_state_path_dev(*head, path, FAKE, None if kw.get("no_jac") else FAKE, None)


def state_bands_path(**kw):
    head, path, _keep = _state(kw)
    out = np.full((1, 1 + 2 + 1 + 2, 2), -7.25)
    status = _lib.lib.sr_limb_rays_state_bands_path_dev(
        *head, _BANDS.ctypes.data_as(_lib.dp), _WIDTHS.ctypes.data_as(_lib.dp), kw.get("n_bands", 2), 5.0, 0, None,
        None if kw.get("no_jac") else out.ctypes.data_as(_lib.dp), None, kw.get("instrument", 0), path)
    assert np.all(out == -7.25)
    return status


def columns_dz(**kw):
    d, _keep = _los(kw)
    p = _path(kw)
    out = np.full((2, 2), -7.25)
    status = _lib.lib.sr_los_columns_dz(None if d is None else C.byref(d), None if p is None else C.byref(p),
                                        None if kw.get("no_out") else out.ctypes.data_as(_lib.dp))
    assert np.all(out == -7.25)
    return status


_PATH = [(dict(no_path=True), ARG), (dict(no_alt=True), ARG), (dict(no_dx=True), ARG), (dict(no_dalt=True), ARG),
         (dict(los_order=1), UNSUPPORTED)]
_TWIN = [(dict(no_tab=True), ARG), (dict(no_los=True), ARG), (dict(n_pts=0), ARG), (dict(n_pts=2000001), LIMIT),
         (dict(seg_layer=[1, N_LAYERS]), ARG), (dict(seg_layer=[-1, 3]), ARG), (dict(par_gas=[0, 2]), ARG),
         (dict(par_gas=[-1, 1]), ARG), (dict(n_col=-1), ARG), (dict(init_mode=1), ARG), (dict(no_jac=True), ARG),
         (dict(level_gas=2), ARG)]
REFUSED = {
    jac_state_path: _PATH + _TWIN,
    state_bands_path: _PATH + _TWIN + [(dict(n_bands=0), ARG), (dict(instrument=1, no_path=True), ARG)],
    columns_dz: _PATH + [(dict(no_los=True), ARG), (dict(no_out=True), ARG)],
}


@pytest.mark.parametrize("entry", list(REFUSED), ids=lambda f: f.__name__)
def test_refused_calls_return_their_status_before_any_device_call(entry):
    for kw, status in REFUSED[entry]:
        assert entry(**kw) == status, kw


def test_observer_order_is_refused_with_a_message():
    assert jac_state_path(los_order=1) == UNSUPPORTED
    assert b"photon order" in _lib.lib.sr_last_error()


def test_abi_surface():
    assert _lib.lib.sr_abi_version() == 1
    for name in ("sr_los_columns_dz", "sr_limb_rays_jac_state_path_dev", "sr_limb_rays_state_bands_path_dev"):
        assert hasattr(_lib.lib, name) and name in _lib.SYMBOLS
    assert [f[0] for f in _lib.LosPath._fields_] == ["alt", "dx_dz", "dalt_dz"]


def test_a_batch_without_path_raises():
    from spectrobot_amd import engine
    los = engine.LimbLOS(_SO, _SL, _PO, _X, _ONE[:4], np.ones((2, 4)))
    with pytest.raises(ValueError, match="path"):
        engine.los_columns_dz(los)
    with pytest.raises(ValueError, match="path"):
        engine.limb_rays_state_jacobian(None, los, pointing=True)
    with pytest.raises(ValueError, match="path"):
        engine.limb_rays_state_bands(None, los, None, None, None, pointing=True)
    with pytest.raises(ValueError, match=r"\[n_pt\]"):
        engine.LimbLOS(_SO, _SL, _PO, _X, _ONE[:4], np.ones((2, 4)), path=dict(alt=np.ones(3), dx=np.ones(4), dalt=np.ones(4)))
