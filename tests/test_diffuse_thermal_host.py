"""Thermal emission as a source of the two-stream diffuse field (engine.diffuse_thermal_source,
retrieval.ThermalScattering, LimbScene(thermal_scattering=), sr_diffuse_thermal_rows_dev) checked on the host, no GPU: the
ABI surface, the reference's two statements against each other, the fp64 restatement of the kernel's formulas against the
reference, exact zeros, empty layers, superposition, the deep interior of an isothermal column, and the refusals of the
host layers."""
import os
import re

import numpy as np
import pytest

import absorber_table_reference as AR
import diffuse_source_reference as R
import diffuse_thermal_reference as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LD = np.longdouble
KEYS = ("emi", "J", "flux")


def _bounds(c, ref):
    n_gas, n_layers = c["A"].shape[:2]
    xm = T.x_max(c)
    return {k: T.bound(ref[k], n_gas, n_layers, xm) for k in KEYS}


def test_abi_surface():
    from spectrobot_amd import _lib
    header = open(os.path.join(ROOT, "include", "spectrobot_hip.h")).read()
    assert re.search(r"^int sr_diffuse_thermal_rows_dev\(const sr_diffuse_desc \*desc, const sr_diffuse_thermal_desc \*th,", header, re.M)
    assert re.search(r"\} sr_diffuse_thermal_desc;", header)
    assert "sr_diffuse_thermal_rows_dev" in _lib.SYMBOLS and hasattr(_lib.lib, "sr_diffuse_thermal_rows_dev")
    names = [n for n, _ in _lib.DiffuseThermalDesc._fields_]
    assert names == ["temps", "t_surface", "w0", "step", "g_lo", "own_emission"]
    assert _lib.lib.sr_abi_version() == 1


def test_adding_form_against_the_interface_system():
    """`reference` against `reference_bvp`, both in long double, on bvp_case-style columns (co >= ~1e-2), thermal alone and
    with the sun, under the allowance of tests/test_diffuse_source_host.py: b 2^-11 / (co min(k dtau', 1)), |ref| of b the
    column's largest value of that output."""
    rng = np.random.default_rng(20261022)
    worst = 0.0
    for case in range(40):
        n_layers = (1, 2, 3, 7, 17)[case % 5]
        c = T.bvp_case(rng, n_layers, empty=0.2 if case % 4 == 3 else 0.0)
        co, dt = R.min_co(*R.args(c)[:4]), R.min_dtau(*R.args(c)[:4])
        if not np.isfinite(dt):
            continue
        assert co >= 1e-3
        solar, own = bool(case % 2), bool((case // 2) % 2)
        ref, bvp = T.reference(c, solar, own), T.reference_bvp(c, solar, own)
        allow = 2.0 ** -11 / (co * min(np.sqrt(3.0 * co) * dt, 1.0))
        for key in KEYS:
            top = np.max(np.abs(ref[key]).reshape(-1, ref[key].shape[-1]), axis=0)
            b = T.bound(np.broadcast_to(top, ref[key].shape), 2, n_layers, T.x_max(c)) * LD(allow)
            assert np.all(b > 0)
            worst = max(worst, float(np.max(np.abs(bvp[key] - ref[key]) / b)))
    print("adding form against the interface system, in units of b 2^-11 / (co min(k dtau, 1)): %.3f" % worst)
    assert worst <= 1.0


def test_fp64_restatement_against_the_reference():
    """plain64 stays at <= 0.5 of b over the GPU panel's cases and 300 random columns (70 .. 200 K per layer, nu in 500 ..
    3300 cm^-1), thermal alone and with the sun, own_emission off and on."""
    worst = dict.fromkeys(KEYS, 0.0)
    cases = [T.panel_case(n, g, p) for n in T.N_LAYERS for g in T.N_GAS for p in T.N_PTS] + list(T.random_columns())
    x_top = 0.0
    for i, c in enumerate(cases):
        x_top = max(x_top, float(np.max(T.x_max(c))))
        for solar in (False, True):
            own = bool((i + solar) % 2)
            ref, p64 = T.reference(c, solar, own), T.plain64(c, solar, own)
            b = _bounds(c, ref)
            for key in KEYS:
                assert np.all(ref[key] >= 0) and np.all(p64[key] >= 0), key
                worst[key] = max(worst[key], T.ratio(p64[key], ref[key], b[key]))
    print("plain fp64 against the reference, in units of b (C_PLANCK = %d, x up to %.1f): emi %.3f J %.3f flux %.3f"
          % (T.C_PLANCK, x_top, worst["emi"], worst["J"], worst["flux"]))
    assert x_top > 60.0
    assert max(worst.values()) <= 0.5


def test_exact_zeros():
    c = T.panel_case(3, 3, 5)
    for fn in (T.reference, T.plain64):
        # no absorber anywhere (every ssa = 1), no sun, no emitting surface: nothing emits, every output is an exact 0
        o = fn(dict(c, ssa=np.ones(3), t_surface=0.0), solar=False, own=True)
        assert all(np.all(o[k] == 0) for k in KEYS)
        # the same column above an emitting surface: light, and it is the surface's alone
        o = fn(dict(c, ssa=np.ones(3), t_surface=150.0, albedo=0.25), solar=False)
        assert np.all(o["flux"][0] > 0)
        # one layer without an absorber between two that have one: its source is 0 -- taking its temperature to 1000 K
        # changes no bit
        V = np.maximum(c["V"], 1e-3)
        A = c["A"].copy()
        ssa = np.array([1.0, 0.0, 0.0])
        V[1:, 1] = 0.0
        hot = c["temps"].copy()
        hot[1] = 1000.0
        a = fn(dict(c, V=V, A=A, ssa=ssa), solar=False)
        b = fn(dict(c, V=V, A=A, ssa=ssa, temps=hot), solar=False)
        assert all(np.array_equal(a[k], b[k]) for k in KEYS) and np.all(a["J"] > 0)


def test_an_empty_layer_changes_nothing_but_the_index():
    c = T.panel_case(3, 3, 5)
    c["V"] = np.maximum(c["V"], 1e-3)
    A2 = np.insert(c["A"], 1, 0.7, axis=1)
    V2 = np.insert(c["V"], 1, 0.0, axis=1)
    beam2 = np.insert(c["beam"], 1, 0.5 * (c["beam"][0] + c["beam"][1]), axis=0)
    temps2 = np.insert(c["temps"], 1, 333.0)
    for fn in (T.reference, T.plain64):
        for solar in (False, True):
            a = fn(c, solar, True)
            b = fn(dict(c, A=A2, V=V2, beam=beam2, temps=temps2), solar, True)
            assert np.all(np.delete(b["flux"], 1, axis=1) == a["flux"]) and np.all(b["flux"][:, 1] == b["flux"][:, 2])
            assert np.all(np.delete(b["emi"], 1, axis=0) == a["emi"])
            assert np.all(np.delete(b["J"], 1, axis=0) == a["J"])


def test_superposition_in_long_double():
    """The equations are linear in their sources: both sources = the sun's alone (diffuse_source_reference.reference) plus
    thermal emission alone, to long double's rounding (b 2^-10)."""
    for key in ((17, 3, 5), (3, 8, 2), (1, 1, 3), (80, 3, 2)):
        c = T.panel_case(*key)
        both, night, sol = T.reference(c, True), T.reference(c, False), R.reference(*R.args(c))
        b = _bounds(c, both)
        for k in KEYS:
            assert T.ratio(night[k] + sol[k], both[k], b[k] * LD(2.0 ** -10)) <= 1.0, (key, k)


def test_deep_interior_of_an_isothermal_column():
    """17 layers of k dtau' >= 6 each at one temperature, the surface at the same temperature, asym <= 0: the middle of
    the middle layer has 8.5 layers on either side (17 layers leave no layer with 9), so the boundaries' share is below
    e^-51 there and below e^-48 at its two interfaces: |J - B| <= b, and the own_emission rows are within b of A B."""
    rng = np.random.default_rng(20261023)
    n_layers, n_pts = 17, 4
    for asym0, ssa0 in ((0.0, 0.6), (-0.4, 0.95), (-0.2, 0.3)):
        ssa, asym = np.array([ssa0, 0.0]), np.array([asym0, 0.0])
        A = rng.uniform(0.8, 1.2, (2, n_layers, n_pts))
        # k = sqrt(3 co (1 - om g)) >= sqrt(3 co) with g <= 0; dtau' chosen so that k dtau' >= 6 at the smallest A
        co_min = (1.0 - ssa0) * 0.8 / ((1.0 - ssa0) * 0.8 + ssa0 * 1.2)
        V = np.full((2, n_layers), 0.5 * 6.5 / (np.sqrt(3.0 * co_min) * 0.8))
        c = dict(A=A, V=V, ssa=ssa, asym=asym, beam=np.zeros((n_layers + 1, n_pts)), sun=np.zeros(n_pts), mu0=0.0, albedo=0.3,
                 out_gas=0, temps=np.full(n_layers, 140.0), t_surface=140.0, w0=900.0, step=0.25, g_lo=7)
        sp, al, sg = R.optics_definition(A, V, ssa, asym)
        assert float(np.min(np.sqrt(3.0 * al / (sp + al)) * (sp + al))) >= 6.0
        for fn in (T.reference, T.plain64):
            o = fn(c, solar=False, own=True)
            B = T.planck_rows(T.nu_of(c), c["temps"], LD)
            b = T.bound(B, 2, n_layers, T.x_max(c))
            mid = slice(8, 9)
            assert np.all(np.abs(np.asarray(o["J"], LD)[mid] - B[mid]) <= b[mid]), fn.__name__
            AB = np.asarray(A[0], LD) * B
            assert np.all(np.abs(np.asarray(o["emi"], LD)[mid] - AB[mid]) <= T.bound(AB, 2, n_layers, T.x_max(c))[mid]), fn.__name__
            # everything at one temperature: F+- = 2 pi B / sqrt3 at every interface but the top's F-
            F = np.asarray(o["flux"], LD)
            want = T._k_thermal(LD) * B[0]
            assert np.all(np.abs(F[0, :9] - want) <= T.bound(want, 2, n_layers, T.x_max(c)))


def _small_scene(rt, **kw):
    grid = 2950.0 + 0.01 * np.arange(8)
    z = np.linspace(100.0, 400.0, 4)
    haze = rt.TableGas("haze", None, np.ones(4), solar=kw.pop("solar", dict(albedo=0.9, g=0.4)), source=kw.pop("source", True))
    return rt.LimbScene(grid, z, np.full(4, 150.0), np.full(4, 1.0), [haze], [3389.0], [5.0], **kw)


def test_thermal_scattering_value_errors_and_scene_refusals():
    from spectrobot_amd import retrieval as rt, spect_main_module as smm
    ts = rt.ThermalScattering()
    assert ts.surface_temperature is None and ts.surface_albedo == 0.0 and ts.key() == (None, 0.0)
    assert rt.ThermalScattering(94.0, 0.2).key() == (94.0, 0.2)
    for bad in (0.0, -3.0, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            rt.ThermalScattering(surface_temperature=bad)
    for bad in (-0.1, 1.1, float("nan")):
        with pytest.raises(ValueError):
            rt.ThermalScattering(surface_albedo=bad)
    assert _small_scene(rt).thermal_scattering is None
    scene = _small_scene(rt, thermal_scattering=ts)
    assert scene.thermal_scattering is ts and [g.name for g in scene.thermal_scatterers()] == ["haze"]
    with pytest.raises(ValueError, match="g >= -0.5"):
        _small_scene(rt, thermal_scattering=ts, solar=dict(albedo=0.9, g=-0.7))
    with pytest.raises(ValueError, match="source=False"):
        _small_scene(rt, thermal_scattering=ts, source=False)
    irr = np.ones(8)
    _small_scene(rt, thermal_scattering=rt.ThermalScattering(surface_albedo=0.3), sun=rt.Sun(60.0, 30.0, irr, multiple=True, surface_albedo=0.3))
    _small_scene(rt, thermal_scattering=rt.ThermalScattering(surface_albedo=0.3), sun=rt.Sun(60.0, 30.0, irr))   # (not read without multiple)
    with pytest.raises(ValueError, match="one surface"):
        _small_scene(rt, thermal_scattering=ts, sun=rt.Sun(60.0, 30.0, irr, multiple=True, surface_albedo=0.3))
    # the three Jacobian flags: refused before any device call, with the reason
    z = scene.z
    pixels = [rt.LimbPixel(150.0)]
    prof = lambda: smm.LinearProfile_1D_new("haze", z, z[[0, 3]], np.ones(2), np.full(2, 0.5))
    bs = smm.BayesSet()
    bs.add_set(prof())
    with pytest.raises(ValueError, match="tangent kernels do not know the thermal source"):
        rt.inversion_state(scene, bs, pixels, diffuse_jacobian=True)
    bs = smm.BayesSet()
    bs.add_set(prof())
    bs.add_set(rt.HazeOptics(albedo={"haze": (0.9, 0.1)}))
    with pytest.raises(ValueError, match="tangent kernels do not know the thermal source"):
        rt.inversion_state(scene, bs, pixels)
    bs = smm.BayesSet()
    bs.add_set(prof())
    bs.add_set(rt.TempProfile(z, z[[0, 3]], np.full(2, 3.0)))
    with pytest.raises(ValueError, match="tangent kernels do not know the thermal source"):
        rt.inversion_state(scene, bs, pixels)
    with pytest.raises(ValueError, match="tangent kernels do not know the thermal source"):
        scene.temperature_derivatives()


def test_engine_refusals_need_no_gpu():
    """The Python entry checks the rules among its arguments, then the grid, temps and g_lo, then its tensors: each class is
    refused before any device call (A is a host array throughout, which is itself refused last)."""
    from spectrobot_amd import engine
    grid = 2950.0 + 0.0078125 * np.arange(3)
    A, V, temps = np.ones((1, 2, 3)), np.ones((1, 2)), np.full(2, 150.0)
    call = lambda *a, **kw: engine.diffuse_thermal_source(A, V, [0.5], [0.1], *a, **kw)
    with pytest.raises(ValueError, match="both .* or neither"):        # exactly one of beam and sun
        call(temps, grid, beam=np.ones((3, 3)), out_gas=0)
    with pytest.raises(ValueError, match="both .* or neither"):
        call(temps, grid, sun=np.ones(3), out_gas=0)
    with pytest.raises(ValueError, match="belong to the rows of out_gas"):
        call(temps, grid, own_emission=True, mean_intensity=True)
    with pytest.raises(ValueError, match="belong to the rows of out_gas"):
        call(temps, grid, accumulate=True, fluxes=True)
    with pytest.raises(ValueError, match="nothing asked for"):
        call(temps, grid)
    with pytest.raises(ValueError, match="accumulate=True adds to out"):
        call(temps, grid, out_gas=0, accumulate=True)
    with pytest.raises(ValueError, match="not an np.arange grid"):
        call(temps, np.array([2950.0, 2950.5, 2951.5]), out_gas=0)
    with pytest.raises(ValueError, match=r"temps must be \[n_layers\] and g_lo"):
        call(np.full((2, 1), 150.0), grid, out_gas=0)
    with pytest.raises(ValueError, match=r"temps must be \[n_layers\] and g_lo"):
        call(temps, grid, out_gas=0, g_lo=-1)
    with pytest.raises(ValueError, match=r"temps must be \[n_layers\] and g_lo"):
        call(temps, grid, out_gas=0, g_lo=3)
    with pytest.raises(ValueError, match="contiguous CUDA float64"):   # what is left: the host array itself
        call(temps, grid, out_gas=0)
    with pytest.raises(ValueError, match="contiguous CUDA float64"):
        call(temps, grid, beam=np.ones((3, 3)), sun=np.ones(3), mu0=0.5, out_gas=0)
