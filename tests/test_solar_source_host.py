"""The single-scattering solar source (engine.solar_source, geometry.solar_columns, retrieval.Sun / TableGas(solar=),
sr_solar_source_rows_dev) checked on the host, no GPU: the ABI surface, the reference against its own fp64 restatement,
the sun ray's columns against the builders that already exist, the phase function's normalisation, the kernel's chunk
lists against a numpy statement, the scene's cache key and the refusals of the host layers."""
import os
import re

import numpy as np
import pytest

import columns_reference as CR
import solar_source_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("sr_solar_source_rows_dev", "sr_solar_chunk_lists", "sr_set_solar_full_lists")


def test_abi_surface():
    from spectrobot_amd import _lib
    header = open(os.path.join(ROOT, "include", "spectrobot_hip.h")).read()
    for name in NAMES:
        assert re.search(r"^int %s\(" % name, header, re.M), name
        assert name in _lib.SYMBOLS and hasattr(_lib.lib, name)
    assert int(re.search(r"#define SR_MAX_SOLAR_VALUES (\d+)", header)[1]) == _lib.SR_MAX_SOLAR_VALUES
    assert _lib.lib.sr_abi_version() == 1


def test_reference_against_its_fp64_restatement():
    """A term-by-term fp64 loop stays inside the bound on 200 random cases (n_k 1 .. 640, tau 0.01 .. 200) and on the panel
    case of n_k = 259."""
    rng = np.random.default_rng(20261020)
    worst_e = worst_t = 0.0
    for case in range(200):
        n_k = int(np.exp(rng.uniform(0.0, np.log(640.0)))) if case % 10 else (1, 640)[case // 10 % 2]
        n_rows, n_pts = int(rng.integers(1, 4)), 4
        A = rng.uniform(0.5, 1.5, (n_k, n_pts)) * np.exp(rng.uniform(np.log(0.3), 0.0, n_pts))[None, :]
        U = R.ray_columns(rng, n_rows, n_k, tau_lo=0.01, tau_hi=200.0)
        w, sca, sun = rng.uniform(0.01, 0.1, n_rows), rng.uniform(1e-9, 1e-7, (n_rows, n_pts)), rng.uniform(5.0, 20.0, n_pts)
        emi, trans, tau, K = R.reference(A, U, w, sca, sun)
        e64, t64 = R.plain64(A, U, w, sca, sun)
        worst_e = max(worst_e, R.ratio(e64, emi, R.bound_emi(emi, tau, K)))
        worst_t = max(worst_t, R.ratio(t64, trans, R.bound_trans(trans, tau, K)))
    c = R.panel_case(17, 259, 65)                    # the GPU test's case of a second batch of chunks
    emi, trans, tau, K = R.reference(c["A"], c["U"], c["w"], c["sca"], c["sun"], c["src_row"])
    e64, t64 = R.plain64(c["A"], c["U"], c["w"], c["sca"], c["sun"], c["src_row"])
    worst_e = max(worst_e, R.ratio(e64, emi, R.bound_emi(emi, tau, K)))
    worst_t = max(worst_t, R.ratio(t64, trans, R.bound_trans(trans, tau, K)))
    print("plain fp64 against the reference, in units of the bound: emi %.3f trans %.3f" % (worst_e, worst_t))
    assert worst_e <= 1.0 and worst_t <= 1.0


def test_reference_exact_cases():
    A = np.full((3, 2), 400.0)
    U = np.array([[1.0, 1.0, 0.0], [0.0, 0.0, 0.0], [1e-3, 0.0, 0.0], [1e-3, 0.0, 0.0]])
    emi, trans, tau, K = R.reference(A, U, [0.1, 0.1, 0.0, 0.1], np.ones((4, 2)), np.ones(2))
    assert np.all(emi[0] == 0) and np.all(trans[0] == 0)            # tau = 800 >= 700
    assert np.all(trans[1] == 1) and np.all(emi[1] == np.longdouble(0.1))
    assert np.all(emi[2] == 0) and np.all(trans[2] == 0)            # in shadow
    assert np.all(emi[3] > 0) and list(K) == [2, 0, 1, 1]


# ----------------------------------------------------------------------------------------------------------------------
# geometry
# ----------------------------------------------------------------------------------------------------------------------
def _atmosphere():
    z = np.linspace(100.0, 690.0, 60) + np.where(np.arange(60) % 2, 1.5, 0.0)      # uneven shells
    nd = 3e17 * np.exp(-(z - 100.0) / 63.0)
    vmr = np.array([0.0148 * (1.0 + (z - 100.0) / 900.0), 4e-5 * np.exp(-(z - 100.0) / 300.0), np.full(z.size, 1.0)])
    return z, nd, vmr, np.array([0.98827, 1.0, 0.5])


def _plain_columns(L, col_scale):
    """Curtis-Godson columns of a LOS dict in plain fp64 (columns_reference): the same routine for both sides."""
    col, _ = CR.columns(2, L["x"], L["nd"], L["vmr"], pt_off=L["pt_off"], dtype=np.float64, scale=col_scale)
    return np.asarray(col, float)


def _sun(z, nd, vmr, alt, mu, cs=None):
    """geometry.solar_columns with the plain column routine (its own body, _solar_columns, at the defaults)."""
    from spectrobot_amd import geometry as G
    return G._solar_columns(z, nd, vmr, alt, mu, G.TITAN_RADIUS_KM, 3, cs, _plain_columns)


def _per_layer(L, col, ray, n_layers, segs=None):
    """[n_gas, n_layers]: the columns of ray `ray`'s segments (or of the mask `segs` over them) added into their layers."""
    a, b = L["seg_off"][ray], L["seg_off"][ray + 1]
    keep = np.ones(b - a, bool) if segs is None else segs
    out = np.zeros((col.shape[0], n_layers))
    for g in range(col.shape[0]):
        np.add.at(out[g], L["seg_layer"][a:b][keep], col[g, a:b][keep])
    return out


def _close(U_row, want, amp=1.0):
    """Rounding-level agreement in units of the row's column sum per gas: 64 eps x amp, amp the condition number of the
    chord's ends to the tangent radius (r / distance to the nearest level) where the two sides form it differently."""
    tol = 64 * 2.0 ** -53 * amp * np.maximum(want.sum(axis=1, keepdims=True), 1e-300)
    assert np.all(np.abs(U_row - want) <= tol), float(np.max(np.abs(U_row - want) / tol))


def test_solar_columns_zenith_sun_equals_slant_los():
    from spectrobot_amd import geometry as G
    z, nd, vmr, cs = _atmosphere()
    S = G.slant_los(z, nd, vmr, [0.0])
    want = _per_layer(S, _plain_columns(S, cs), 0, z.size)
    for i in (0, 7, 58, 59):
        U, lit = _sun(z, nd, vmr, [z[i]], 1.0, cs)
        assert lit[0] and U.shape == (1, 3, z.size) and np.all(U[0][:, :i] == 0)
        above = want.copy()
        above[:, :i] = 0
        _close(U[0], above)


def test_solar_columns_horizontal_sun_equals_half_a_limb_ray():
    from spectrobot_amd import geometry as G
    z, nd, vmr, cs = _atmosphere()
    alts = [z[0], 203.7, z[11], 655.0]
    L = G.limb_los(z, nd, vmr, alts)
    col = _plain_columns(L, cs)
    U, lit = _sun(z, nd, vmr, alts, 0.0, cs)
    assert lit.all() and np.all(U >= 0)
    for r in range(len(alts)):
        n = L["seg_off"][r + 1] - L["seg_off"][r]
        near = np.arange(n) >= n // 2                        # photon order: far side first
        _close(U[r], _per_layer(L, col, r, z.size, near))


def test_solar_columns_sun_below_the_horizon():
    """mu < 0 with the tangent radius above z[0]: the tangent ray's far half (by symmetry its near half) plus the part of
    the near half below the point, which sits on a level."""
    from spectrobot_amd import geometry as G
    z, nd, vmr, cs = _atmosphere()
    R0 = G.TITAN_RADIUS_KM
    for zt, i in ((203.7, 20), (z[3] + 2.0, 9)):
        rt, rp = R0 + zt, R0 + z[i]
        mu = -np.sqrt((rp - rt) * (rp + rt)) / rp
        L = G.limb_los(z, nd, vmr, [zt])
        col = _plain_columns(L, cs)
        n = L["seg_off"][1]
        near = np.arange(n) >= n // 2
        below = near & (L["seg_layer"] < i)
        want = _per_layer(L, col, 0, z.size, near) + _per_layer(L, col, 0, z.size, below)
        U, lit = _sun(z, nd, vmr, [z[i]], mu, cs)
        assert lit[0] and np.all(U >= 0)
        gap = min(abs(zt - z).min(), 1.0)
        _close(U[0], want, amp=rp / gap)


def test_solar_columns_shadow_and_signs():
    from spectrobot_amd import geometry as G
    z, nd, vmr, cs = _atmosphere()
    R0 = G.TITAN_RADIUS_KM
    mu_graze = -np.sqrt(1.0 - ((R0 + z[0]) / (R0 + 300.0)) ** 2)
    mus = [mu_graze * 1.001, mu_graze * 0.999, -1.0, 0.3]
    U, lit = _sun(z, nd, vmr, [300.0] * 4, mus, cs)
    assert list(lit) == [False, True, False, True]
    assert np.all(U[0] == 0) and np.all(U[2] == 0) and U[1].sum() > U[3].sum() > 0
    assert np.all(U >= 0) and np.all(np.isfinite(U))
    # a point above the top boundary: lit, nothing on the way
    U, lit = _sun(z, nd, vmr, [5000.0], 0.5)
    assert lit[0] and np.all(U == 0)
    with pytest.raises(ValueError):
        _sun(z, nd, vmr, [300.0], 1.5)


@pytest.mark.parametrize("g", [0.0, 0.5, -0.3])
def test_hg_phase_integrates_to_one(g):
    from spectrobot_amd import geometry as G
    x, wq = np.polynomial.legendre.leggauss(64)
    assert abs(0.5 * np.sum(wq * G.hg_phase(x, g)) - 1.0) < 1e-13       # (1 / 4 pi) int P dOmega
    if g == 0.0:
        assert np.all(G.hg_phase(x, g) == 1.0)
    with pytest.raises(ValueError):
        G.hg_phase(0.0, 1.0)


def test_solar_irradiance():
    from spectrobot_amd import geometry as G, spect_classes as sc
    grid = 2950.0 + 0.01 * np.arange(5)
    F = G.solar_irradiance(grid, 5772.0, 695700.0, 1.4e9)
    want = np.pi * sc.Calc_BB_single(grid, 5772.0) * (695700.0 / 1.4e9) ** 2
    assert np.max(np.abs(F - want) / want) < 1e-14


# ----------------------------------------------------------------------------------------------------------------------
# small pieces
# ----------------------------------------------------------------------------------------------------------------------
def _lists(U, w, full=False):
    n_rows, n_k = U.shape
    off, ch = [0], []
    for t in range((n_rows + 15) // 16):
        rows = slice(16 * t, min(16 * t + 16, n_rows))
        nz = (U[rows] != 0) & (np.asarray(w)[rows] != 0)[:, None]
        hit = [c for c in range((n_k + 3) // 4) if full or nz[:, 4 * c:4 * c + 4].any()]
        ch += hit
        off.append(len(ch))
    return np.array(off), np.array(ch, dtype=int)


@pytest.mark.parametrize("n_rows,n_k", [(1, 1), (15, 3), (17, 5), (33, 13), (65, 160)])
def test_chunk_lists(n_rows, n_k):
    from spectrobot_amd import engine
    c = R.panel_case(n_rows, n_k, 1)
    w = c["w"].copy()
    w[::5] = 0.0
    for full in (False, True):
        engine.set_solar_full_lists(full)
        try:
            off, ch = engine.solar_chunk_lists(c["U"], w)
        finally:
            engine.set_solar_full_lists(False)
        want_off, want_ch = _lists(c["U"], w, full)
        assert np.array_equal(off, want_off) and np.array_equal(ch, want_ch)
    # a tile whose rows are all in shadow lists nothing; U itself is read as it is
    off, ch = engine.solar_chunk_lists(c["U"], np.zeros(n_rows))
    assert ch.size == 0 and np.all(off == 0)


def test_chunk_lists_refusals():
    from spectrobot_amd import engine, _lib
    U = np.ones((3, 5))
    for bad_U, bad_w in ((-U, np.ones(3)), (U * np.nan, np.ones(3)), (U, [-1.0, 1, 1]), (U, [np.inf, 1, 1])):
        with pytest.raises(_lib.SpectRobotHipError) as e:
            engine.solar_chunk_lists(bad_U, bad_w)
        assert e.value.status == _lib.SR_ERR_ARG
    with pytest.raises(_lib.SpectRobotHipError) as e:
        engine.solar_chunk_lists(np.zeros((4096, 4096)), 1.0)
    assert e.value.status == _lib.SR_ERR_LIMIT


class _Gas(object):
    def __init__(self, name, vmr, tab):
        self.name, self.vmr, self.iso_ratio, self.coeffs, self.thermal, self.solar = name, np.asarray(vmr, float), 1.0, (tab, tab), None, None


def test_scene_solar_key_and_value_errors():
    from spectrobot_amd import retrieval as rt
    grid = 2950.0 + 0.01 * np.arange(8)
    z = np.linspace(100.0, 400.0, 4)
    sun = rt.Sun(60.0, 30.0, np.ones(8))
    haze = rt.TableGas("haze", None, np.ones(4), solar=dict(albedo=0.9, g=0.5))
    haze.coeffs = haze.thermal = (object(), object())
    gas = _Gas("CH4", np.full(4, 0.01), object())
    scene = rt.LimbScene(grid, z, np.full(4, 150.0), np.full(4, 1.0), [gas, haze], [3389.0], [5.0], sun=sun)
    assert scene.solar_gases() == [haze]
    k0 = scene.solar_key(0, 8)
    assert scene.solar_key(0, 8) == k0 and scene.solar_key(0, 4) != k0
    gas.vmr = gas.vmr * 1.01                        # a VMR iteration moves the key ...
    k1 = scene.solar_key(0, 8)
    assert k1 != k0
    haze.vmr = haze.vmr * 2.0                       # ... the scatterer's own profile too
    k2 = scene.solar_key(0, 8)
    assert k2 != k1
    gas.coeffs = (object(), gas.coeffs[1])          # a rebuilt absorption table
    k3 = scene.solar_key(0, 8)
    assert k3 != k2
    scene.sun = rt.Sun(61.0, 30.0, np.ones(8))
    assert scene.solar_key(0, 8) != k3
    scene.sun = rt.Sun(60.0, 30.0, np.full(8, 2.0))
    assert scene.solar_key(0, 8) != k3
    # rows in shadow get weight 0, the others albedo P(180 deg - phase) / 4 pi
    from spectrobot_amd import geometry as G
    w = scene.solar_weights(haze, np.array([True, False, True, True]))
    assert w[1] == 0.0 and np.all(w[[0, 2, 3]] == 0.9 * G.hg_phase(np.cos(np.deg2rad(150.0)), 0.5) / (4 * np.pi))
    # without a sun nothing is solar
    assert rt.LimbScene(grid, z, np.full(4, 150.0), np.full(4, 1.0), [gas, haze], [3389.0], [5.0]).solar_gases() == []
    with pytest.raises(ValueError):
        rt.TableGas("haze", None, np.ones(4), accumulate_into="CH4", solar=dict(albedo=0.9, g=0.5))
    with pytest.raises(ValueError):
        rt.TableGas("haze", None, np.ones(4), solar=dict(albedo=1.9, g=0.5))
    with pytest.raises(ValueError):
        rt.TableGas("haze", None, np.ones(4), solar=dict(albedo=0.9))
    with pytest.raises(ValueError):
        rt.single_rad_keys([haze], {("haze", "iso_0"): [0]})            # tracked levels of such a gas
    with pytest.raises(ValueError):
        rt.LimbScene(grid, z, np.full(4, 150.0), np.full(4, 1.0), [gas, haze], [3389.0], [5.0], sun=rt.Sun(60.0, 30.0, np.ones(7)))
    with pytest.raises(ValueError):
        rt.Sun(60.0, 30.0, [-1.0])
