"""The solar attenuation in the Jacobians (engine.solar_attenuation_jacobian, geometry.solar_column_weights,
LimbScene.keep_solar_rows, inversion_state(solar_attenuation=), sr_solar_jacobian_rows_dev) checked on the host, no GPU: the
ABI surface and every refusal with fake device pointers, the reference against its own fp64 restatement, the column
weights against the columns they are the derivative of, the kernel's chunk lists against a numpy statement, the driver's
refusal above four gas slots and the default solar pass, which must run the statements it ran before."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import columns_reference as CR
import solar_jacobian_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("sr_solar_jacobian_rows_dev", "sr_solar_jacobian_chunk_lists")


def test_abi_surface():
    from spectrobot_amd import _lib, engine
    header = open(os.path.join(ROOT, "include", "spectrobot_hip.h")).read()
    for name in NAMES:
        assert re.search(r"^int %s\(" % name, header, re.M), name
        assert name in _lib.SYMBOLS and hasattr(_lib.lib, name)
    assert _lib.lib.sr_abi_version() == 1
    plan = open(os.path.join(ROOT, "spectrobot_amd", "csrc", "sr_solar_plan.hpp")).read()
    assert int(re.search(r"kSolarJacRays = (\d+);", plan)[1]) == engine.SOLAR_JAC_RAYS == R.NR


def test_reference_against_its_fp64_restatement():
    """A term-by-term fp64 loop stays inside the bound on 200 random cases (n_k 1 .. 160, about half zeros, both signs) and
    on the panel case of n_k = 259."""
    rng = np.random.default_rng(20261020)
    worst = 0.0
    for case in range(200):
        n_k = int(np.exp(rng.uniform(0.0, np.log(160.0)))) if case % 10 else (1, 160)[case // 10 % 2]
        n_par, n_rows, n_rays, n_pts = int(rng.integers(1, 4)), int(rng.integers(1, 20)), int(rng.integers(1, 3)), 4
        A = rng.uniform(0.5, 1.5, (n_k, n_pts)) * np.exp(rng.uniform(np.log(0.3), 0.0, n_pts))[None, :]
        dU = rng.normal(size=(n_par, n_rows, n_k)) * (rng.random((n_par, n_rows, n_k)) < 0.5)
        Q = rng.normal(size=(n_rays, n_rows, n_pts)) * 1e-8
        jac, b = R.reference(A, dU, Q)
        worst = max(worst, R.ratio(R.plain64(A, dU, Q), jac, b))
    c = R.panel_case(17, 259, 65, R.NR + 1, 2)       # the GPU test's case of a second batch of chunks
    jac, b = R.reference(c["A"], c["dU"], c["Q"])
    worst = max(worst, R.ratio(R.plain64(c["A"], c["dU"], c["Q"]), jac, b))
    print("plain fp64 against the reference, in units of the bound: %.3f" % worst)
    assert worst <= 1.0


def test_reference_exact_cases():
    A = np.full((3, 2), 2.0)
    dU = np.zeros((2, 2, 3))
    dU[0, 1, 2] = -0.5
    Q = np.array([[[1.0, 2.0], [3.0, 4.0]]])
    jac, b = R.reference(A, dU, Q)
    assert np.all(jac[0, 0] == np.array([3.0, 4.0], R.LD)) and np.all(jac[0, 1] == 0) and np.all(b[0, 1] == 0)
    assert np.all(b[0, 0] == R.LD(R.EPS53) * np.array([3.0, 4.0], R.LD) * 4)      # K = 1, R = 1: (1 + 1 + 2) |Q| |dU| A
    assert R.ratio(np.zeros(2), jac[0, 1], b[0, 1]) == 0.0 and R.ratio(np.full(2, 1e-300), jac[0, 1], b[0, 1]) == np.inf


def test_every_refusal_before_any_device_work():
    """Fake device pointers: a refused call returns before it would touch one of them."""
    from spectrobot_amd import _lib
    lib, dp, ip = _lib.lib, _lib.dp, _lib.ip
    n_par, n_rows, n_k, n_rays, n_pts, n_jac = 3, 17, 5, 2, 65, 4
    dU = R.mask_columns(np.random.default_rng(1), n_par, n_rows, n_k)
    slot = np.array([2, 0, 3], np.int32)
    fake = C.c_void_p(0x1000)
    good = dict(du=dU, n_par=n_par, n_rows=n_rows, A=fake, n_k=n_k, q=fake, n_rays=n_rays, n_pts=n_pts, slot=slot, jac=fake,
                n_jac=n_jac, desc=True)

    def call(**kw):
        a = dict(good, **kw)
        d = _lib.SolarJacDesc()
        d.n_par, d.n_rows = a["n_par"], a["n_rows"]
        d.du = None if a["du"] is None else a["du"].ctypes.data_as(dp)
        return lib.sr_solar_jacobian_rows_dev(C.byref(d) if a["desc"] else None, a["A"], a["n_k"], a["q"], a["n_rays"], a["n_pts"],
                                              None if a["slot"] is None else a["slot"].ctypes.data_as(ip), a["jac"], a["n_jac"], 0, None)

    def edited(arr, at, v):
        out = arr.copy()
        out[at] = v
        return out

    ARG, LIMIT = _lib.SR_ERR_ARG, _lib.SR_ERR_LIMIT
    cases = [("null desc", dict(desc=False), ARG), ("null du", dict(du=None), ARG), ("null tab_abs", dict(A=None), ARG),
             ("null q", dict(q=None), ARG), ("null par_slot", dict(slot=None), ARG), ("null jac", dict(jac=None), ARG),
             ("n_par 0", dict(n_par=0), ARG), ("n_rows 0", dict(n_rows=0), ARG), ("n_rows < 0", dict(n_rows=-2), ARG),
             ("n_k 0", dict(n_k=0), ARG), ("n_rays 0", dict(n_rays=0), ARG), ("n_pts 0", dict(n_pts=0), ARG),
             ("n_jac_rows 0", dict(n_jac=0), ARG), ("du nan", dict(du=edited(dU, (0, 0, 0), np.nan)), ARG),
             ("du inf", dict(du=edited(dU, (2, 16, 4), np.inf)), ARG), ("du -inf", dict(du=edited(dU, (1, 9, 2), -np.inf)), ARG),
             ("par_slot too large", dict(slot=edited(slot, 1, n_jac)), ARG), ("par_slot negative", dict(slot=edited(slot, 0, -1)), ARG),
             ("par_slot repeated", dict(slot=edited(slot, 2, 2)), ARG), ("n_pts beyond the limit", dict(n_pts=2000001), LIMIT),
             ("n_rows beyond the limit", dict(n_rows=_lib.SR_MAX_ABS_ROWS + 1), LIMIT)]
    for what, kw, status in cases:
        assert call(**kw) == status, what
    big = np.zeros((2, 2048, 2049))                  # n_par n_rows n_k beyond SR_MAX_SOLAR_VALUES
    assert call(du=big, n_par=2, n_rows=2048, n_k=2049, slot=np.array([0, 1], np.int32)) == LIMIT
    assert call(n_rays=2 ** 31 - 1, n_pts=2000000) == LIMIT          # more blocks than a grid has


def test_engine_value_errors():
    from spectrobot_amd import engine
    dU = np.zeros((2, 3, 4))
    for bad in (np.zeros((3, 4)), np.zeros((0, 3, 4)), np.zeros((2, 0, 4))):
        with pytest.raises(ValueError):
            engine.solar_jacobian_chunk_lists(bad)
    with pytest.raises(ValueError):
        engine.solar_attenuation_jacobian(np.zeros((4, 8)), dU, np.zeros((1, 3, 8)))      # not CUDA tensors


# ----------------------------------------------------------------------------------------------------------------------
# geometry
# ----------------------------------------------------------------------------------------------------------------------
def _atmosphere():
    z = np.linspace(100.0, 690.0, 60) + np.where(np.arange(60) % 2, 1.5, 0.0)      # uneven shells
    return z, 3e17 * np.exp(-(z - 100.0) / 63.0), np.array([0.98827, 1.0, 0.5])


def _plain_columns(L, col_scale):
    """Curtis-Godson columns of a LOS dict in plain fp64 (columns_reference): the same routine for both sides."""
    col, _ = CR.columns(2, L["x"], L["nd"], L["vmr"], pt_off=L["pt_off"], dtype=np.float64, scale=col_scale)
    return np.asarray(col, float)


def test_solar_column_weights_are_the_derivative_of_solar_columns():
    """sum_p x_p dU_p against solar_columns of the profiles sum_p x_p m_p, to 64 eps of the row's column sum (of
    magnitudes: the masks have both signs), with mu > 0, = 0, < 0 and in shadow."""
    from spectrobot_amd import geometry as G
    z, nd, cs = _atmosphere()
    rng = np.random.default_rng(7)
    n_gas, n_par = 3, 11                             # more masks than one column call takes
    par_gas = rng.integers(0, n_gas, n_par)
    par_gas[:3] = [0, 1, 2]
    masks = np.zeros((n_par, z.size))
    for p in range(n_par):                           # hats over a few levels, either sign
        c, h = int(rng.integers(0, z.size)), int(rng.integers(2, 12))
        masks[p] = np.clip(1.0 - np.abs(np.arange(z.size) - c) / h, 0.0, None) * rng.choice([-1.0, 1.0])
    x = rng.uniform(0.5, 2.0, n_par) * 1e-3
    R0 = G.TITAN_RADIUS_KM
    mu_graze = -np.sqrt(1.0 - ((R0 + z[0]) / (R0 + 300.0)) ** 2)
    alt = np.array([z[0], 203.7, 300.0, 300.0, 300.0, 655.0, 300.0])
    mu = np.array([0.7, 0.0, mu_graze * 0.999, mu_graze * 1.001, -1.0, -0.05, 1.0])
    args = (G.TITAN_RADIUS_KM, 3, cs, _plain_columns)
    dU, lit = G._solar_column_weights(z, nd, masks, par_gas, n_gas, alt, mu, *args)
    assert dU.shape == (n_par, alt.size, n_gas, z.size) and list(lit) == [True, True, True, False, False, True, True]
    assert np.all(dU[:, ~lit] == 0) and np.all(np.isfinite(dU)) and (dU < 0).any() and (dU > 0).any()
    for p in range(n_par):                           # a parameter's columns stand in its gas alone
        others = np.setdiff1d(np.arange(n_gas), [par_gas[p]])
        assert np.all(dU[p][:, others] == 0) and np.any(dU[p][:, par_gas[p]] != 0)
    profiles = np.zeros((n_gas, z.size))
    for p in range(n_par):
        profiles[par_gas[p]] += x[p] * masks[p]
    U, lit2 = G._solar_columns(z, nd, profiles, alt, mu, *args)
    assert np.array_equal(lit, lit2)
    got = np.tensordot(x, dU, axes=(0, 0))
    # the row's column sum: over all its columns k = (gas, layer), of magnitudes (a signed sum of these masks can cancel to
    # nothing).  Taken per gas instead, the row at 655 km with mu = -0.05 reaches 1.24: 45 eps of ONE element in the shell
    # of its tangent point, where the column routine's own form (nd nearly constant along the crossing) amplifies the last
    # bit of the interpolated profile; the other rows stay below 0.36 either way.
    size = np.tensordot(np.abs(x), np.abs(dU), axes=(0, 0)).sum(axis=(1, 2), keepdims=True)
    tol = 64 * 2.0 ** -53 * np.maximum(size, 1e-300)
    print("sum_p x_p dU_p against solar_columns, in units of 64 eps of the row's column sum: %.3f" % float(np.max(np.abs(got - U) / tol)))
    assert np.all(np.abs(got - U) <= tol), float(np.max(np.abs(got - U) / tol))
    # one parameter per gas with the gas's own profile as its mask: the columns themselves, bit for bit
    vmr = np.array([0.0148 * (1.0 + (z - 100.0) / 900.0), 4e-5 * np.exp(-(z - 100.0) / 300.0), np.full(z.size, 1.0)])
    dU3, _ = G._solar_column_weights(z, nd, vmr, [0, 1, 2], 3, alt, mu, *args)
    U3, _ = G._solar_columns(z, nd, vmr, alt, mu, *args)
    assert all(np.array_equal(dU3[g][:, g], U3[:, g]) for g in range(3))
    with pytest.raises(ValueError):
        G._solar_column_weights(z, nd, masks, np.full(n_par, 3), n_gas, alt, mu, *args)
    with pytest.raises(ValueError):
        G._solar_column_weights(z, nd, masks[:, :-1], par_gas, n_gas, alt, mu, *args)


# ----------------------------------------------------------------------------------------------------------------------
# small pieces
# ----------------------------------------------------------------------------------------------------------------------
def _lists(dU, full=False):
    n_par, n_rows, n_k = dU.shape
    off, ch = [0], []
    for p in range(n_par):
        for t in range((n_rows + 15) // 16):
            nz = dU[p, 16 * t:min(16 * t + 16, n_rows)] != 0
            ch += [c for c in range((n_k + 3) // 4) if full or nz[:, 4 * c:4 * c + 4].any()]
            off.append(len(ch))
    return np.array(off), np.array(ch, dtype=int)


@pytest.mark.parametrize("n_par,n_rows,n_k", [(1, 1, 1), (2, 15, 3), (5, 17, 5), (17, 33, 13), (3, 33, 160)])
def test_chunk_lists(n_par, n_rows, n_k):
    from spectrobot_amd import engine
    dU = R.mask_columns(np.random.default_rng([3, n_par, n_rows, n_k]), n_par, n_rows, n_k, empty=1 if n_par > 1 else None)
    for full in (False, True):
        engine.set_solar_full_lists(full)
        try:
            off, ch = engine.solar_jacobian_chunk_lists(dU)
        finally:
            engine.set_solar_full_lists(False)
        want_off, want_ch = _lists(dU, full)
        assert np.array_equal(off, want_off) and np.array_equal(ch, want_ch)
    if n_par > 1:                                    # the parameter without columns lists nothing
        n_tiles = (n_rows + 15) // 16
        off, _ = engine.solar_jacobian_chunk_lists(dU)
        assert off[n_tiles] == off[2 * n_tiles]
    # the four-dimensional form is the same array
    if n_k % 2 == 0:
        off3, ch3 = engine.solar_jacobian_chunk_lists(dU)
        off4, ch4 = engine.solar_jacobian_chunk_lists(dU.reshape(n_par, n_rows, 2, n_k // 2))
        assert np.array_equal(off4, off3) and np.array_equal(ch4, ch3)


@pytest.mark.parametrize("n_rows,n_k", [(1, 1), (15, 3), (17, 5), (33, 13), (33, 160), (65, 160)])
def test_one_parameter_of_non_negative_columns_lists_what_the_source_lists(n_rows, n_k):
    """The two plans are one walk: dU >= 0 as ONE parameter against the same array as the source's U with every row lit."""
    from spectrobot_amd import engine
    dU = np.abs(R.mask_columns(np.random.default_rng([9, n_rows, n_k]), 1, n_rows, n_k))[0]
    for full in (False, True):
        engine.set_solar_full_lists(full)
        try:
            off_j, ch_j = engine.solar_jacobian_chunk_lists(dU[None])
            off_s, ch_s = engine.solar_chunk_lists(dU, np.ones(n_rows))
        finally:
            engine.set_solar_full_lists(False)
        assert np.array_equal(off_j, off_s) and np.array_equal(ch_j, ch_s)


def test_chunk_lists_refusals():
    from spectrobot_amd import engine, _lib
    for bad in (np.full((2, 3, 5), np.nan), np.full((2, 3, 5), -np.inf)):
        with pytest.raises(_lib.SpectRobotHipError) as e:
            engine.solar_jacobian_chunk_lists(bad)
        assert e.value.status == _lib.SR_ERR_ARG
    with pytest.raises(_lib.SpectRobotHipError) as e:
        engine.solar_jacobian_chunk_lists(np.zeros((2, 2048, 2049)))
    assert e.value.status == _lib.SR_ERR_LIMIT


class _Gas(object):
    def __init__(self, name, vmr, tab):
        self.name, self.vmr, self.iso_ratio, self.coeffs, self.thermal, self.solar = name, np.asarray(vmr, float), 1.0, (tab, tab), None, None


def _scene(n_gases):
    from spectrobot_amd import retrieval as rt
    grid = 2950.0 + 0.01 * np.arange(8)
    z = np.linspace(100.0, 400.0, 4)
    haze = rt.TableGas("haze", None, np.ones(4), solar=dict(albedo=0.9, g=0.5))
    haze.coeffs = haze.thermal = (object(), object())
    gases = [_Gas("gas%d" % i, np.full(4, 0.01), object()) for i in range(n_gases - 1)] + [haze]
    return rt.LimbScene(grid, z, np.full(4, 150.0), np.full(4, 1.0), gases, [3389.0], [5.0], sun=rt.Sun(60.0, 30.0, np.ones(8)))


def test_inversion_state_refuses_the_term_above_four_gas_slots():
    from spectrobot_amd import retrieval as rt, spect_main_module as smm
    scene = _scene(5)
    bs = smm.BayesSet(tag="five slots")
    bs.add_set(smm.LinearProfile_1D_new("gas0", scene.z, scene.z[[0, 3]], np.full(2, 0.01), np.full(2, 0.005)))
    pix = rt.LimbPixel(150.0, observation=rt.Spectrum(np.ones(1), scene.bands_nm), noise=rt.Spectrum(np.ones(1), scene.bands_nm))
    with pytest.raises(ValueError, match="four-gas"):
        rt.inversion_state(scene, bs, [pix], solar_attenuation=True)
    assert scene.keep_solar_rows is False             # refused before anything was changed


def test_default_solar_pass_runs_the_statements_it_ran(monkeypatch):
    """keep_solar_rows off (the default): ONE accumulating engine.solar_source call per solar gas on a clone of the thermal
    emission rows, no other engine call, no solar_rows kept; on: one overwrite call, the rows kept and added."""
    import torch
    from spectrobot_amd import retrieval as rt, geometry as G
    scene = _scene(2)
    gas, haze = scene.gases
    tab = torch.arange(32, dtype=torch.float64).reshape(4, 8)
    gas.coeffs = (tab, tab)
    haze.coeffs = haze.thermal = (tab + 1.0, tab + 2.0)
    calls = []

    def fake_source(A, U, w, sca, sun, src_row=None, out=None, accumulate=False, transmission=False):
        calls.append(dict(A=A, sca=sca, out=out, accumulate=accumulate))
        if out is None:
            return torch.full((4, 8), 0.25, dtype=torch.float64)
        out += 0.25
        return out

    monkeypatch.setattr(rt.engine, "solar_source", fake_source)
    monkeypatch.setattr(G, "solar_columns", lambda *a, **k: (np.zeros((4, 2, 4)), np.ones(4, bool)))
    monkeypatch.setattr(torch, "as_tensor", lambda a, device=None: torch.tensor(np.asarray(a)))
    assert scene.keep_solar_rows is False
    scene.solar_pass(0, 8)
    assert len(calls) == 1 and calls[0]["accumulate"] is True and calls[0]["sca"] is haze.thermal[0]
    assert calls[0]["out"] is haze.coeffs[1] and haze.coeffs[1] is not haze.thermal[1] and haze.coeffs[0] is haze.thermal[0]
    assert torch.equal(haze.coeffs[1], haze.thermal[1] + 0.25) and not hasattr(haze, "solar_rows")
    scene.solar_pass(0, 8)                           # nothing moved: nothing redone
    assert len(calls) == 1
    scene.keep_solar_rows = True
    scene.solar_pass(0, 8)                           # asked for the rows: made again, by an overwrite call
    assert len(calls) == 2 and calls[1]["accumulate"] is False and calls[1]["out"] is None
    assert torch.equal(haze.solar_rows, torch.full((4, 8), 0.25, dtype=torch.float64))
    assert torch.equal(haze.coeffs[1], haze.thermal[1] + haze.solar_rows)
    scene.solar_pass(0, 8)
    assert len(calls) == 2
