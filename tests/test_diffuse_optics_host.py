"""The diffuse rows along a direction in the haze optics (engine.diffuse_optics_jacobian, geometry.hg_phase_dg,
sr_diffuse_optics_jacobian_rows_dev) checked on the host, no GPU: the ABI surface, the analytic tangent against differences
of the forward reference in ssa, asym and the surface albedo, its edge cases, the fp64 restatement of the kernel's formulas
against the reference, every refusal with fake device pointers, the engine's value errors and hg_phase_dg."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import diffuse_jacobian_reference as DJ
import diffuse_optics_reference as DO
import diffuse_source_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LD = np.longdouble


def test_abi_surface():
    from spectrobot_amd import _lib, engine
    header = open(os.path.join(ROOT, "include", "spectrobot_hip.h")).read()
    assert re.search(r"^int sr_diffuse_optics_jacobian_rows_dev\(const sr_diffuse_desc \*desc, const sr_diffuse_optics_desc \*odesc,", header, re.M)
    assert re.search(r"typedef struct \{\s*int32_t n_par;\s*const double \*dssa, \*dasym, \*dalb;[^}]*\} sr_diffuse_optics_desc;", header)
    name = "sr_diffuse_optics_jacobian_rows_dev"
    assert name in _lib.SYMBOLS and hasattr(_lib.lib, name)
    assert [n for n, _ in _lib.DiffuseOpticsDesc._fields_] == ["n_par", "dssa", "dasym", "dalb"]
    # the arguments behind the two descriptors are sr_diffuse_jacobian_rows_dev's
    assert _lib.SYMBOLS[name][1][2:] == _lib.SYMBOLS["sr_diffuse_jacobian_rows_dev"][1][2:]
    assert _lib.lib.sr_abi_version() == 1
    assert name in open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert callable(engine.diffuse_optics_jacobian)
    assert DO.PANEL is DJ.PANEL and DO.C_OPTICS >= DJ.C_LAYER


def test_reference_against_differences_of_the_forward_reference():
    """The analytic tangent along (dssa, dasym, dalb, dlnbeam) together against central differences of the long-double adding
    form (diffuse_jacobian_reference's steps, two Richardson levels), 40 random columns away from the kinks.  Asserted, the
    project's criterion: |reference - fd| <= 2 |r1b - r1a|, both as the largest over the same cases in units of the
    column's largest |dJ| -- asserted column by column, so that one column's large truncation cannot hide a miss in another;
    the largest figures are printed.  (The steps are absolute steps of 1e-3 in ssa, asym and the albedo, so |r1b - r1a| is set
    by the differences' truncation, 5.7e-12, not by rounding as for a relative step of a column: measured |reference - fd|
    9.9e-15.)"""
    self_worst = diff_worst = 0.0
    n = 0
    for c in DO.fd_columns():
        assert np.all((c["ssa"] >= 0.05) & (c["ssa"] <= 0.95)) and np.all((np.abs(c["asym"]) >= 0.05) & (c["asym"] >= -0.4) & (c["asym"] <= 0.9))
        assert 0.05 <= c["albedo"] <= 0.95 and np.all(c["dssa"] != 0) and np.all(c["dasym"] != 0) and np.all(c["dalb"] != 0)
        ref = DO.reference(c)["dJ"][0]
        fd, own = DO.fd_reference(c)
        top = np.max(np.abs(ref))
        assert top > 0
        n += 1
        assert np.max(np.abs(ref - fd)) <= 2 * np.max(own), (n, float(np.max(np.abs(ref - fd)) / np.max(own)))
        self_worst = max(self_worst, float(np.max(own) / top))
        diff_worst = max(diff_worst, float(np.max(np.abs(ref - fd)) / top))
    print("optics tangent against differences on %d columns, in units of the column's largest |dJ|: |r1b - r1a| %.2e, "
          "|reference - fd| %.2e = %.2e |r1b - r1a|" % (n, self_worst, diff_worst, diff_worst / self_worst))
    assert n == 40 and diff_worst <= 2 * self_worst


def _one(c, **kw):
    """The case with one parameter's directions given as keywords (the others zero), the beam held fixed, no Q."""
    n_gas = c["A"].shape[0]
    d = dict(dssa=np.zeros((1, n_gas)), dasym=np.zeros((1, n_gas)), dalb=np.zeros(1))
    d.update({k: np.asarray(v, float).reshape(d[k].shape) for k, v in kw.items()})
    return dict(c, dlnbeam=None, Q=None, **d)


def _agree(c):
    """plain64 within the bound of the reference, which is within the criterion of its own differences; returns it."""
    ref = DO.reference(c, yardstick=True)
    n_gas, n_layers = c["A"].shape[:2]
    assert R.ratio(DO.plain64(c)["dJ"], ref["dJ"], DO.bound(ref["S_dJ"], n_gas, n_layers)) <= 0.5
    fd, own = DO.fd_reference(c)
    assert np.all(np.abs(ref["dJ"][0] - fd) <= 2 * np.max(own) + 1e-25)
    return ref["dJ"][0]


def test_edge_cases_of_the_tangent():
    rng = np.random.default_rng(5)
    base = R.column_case(rng, 5, 2, 3, tau_lo=0.3, tau_hi=3.0, conservative=0.0, empty=0.0, albedo=0.4, mu0=0.6)
    base = dict(base, ssa=np.array([0.8, 0.3]), asym=np.array([0.5, -0.2]))
    # asym == 0 exactly: f = max(asym, 0)^2 has df = 0; asym < 0 likewise
    for ft in (LD, np.float64):
        dcs, dca, dcg = DO.coefficient_tangents([0.8, 0.8, 0.8], [0.0, -0.3, 0.5], np.zeros((1, 3)), np.ones((1, 3)), ft)
        assert dcs[0, 0] == 0 and dcs[0, 1] == 0 and dcs[0, 2] == -ft(0.8) * (2 * ft(0.5)) and np.all(dca == 0)
        assert dcg[0, 0] == ft(0.8) and dcg[0, 1] == ft(0.8) and dcg[0, 2] == ft(0.8) * (1 - 2 * ft(0.5))
        dcs, dca, dcg = DO.coefficient_tangents([0.8], [-0.3], np.ones((1, 1)), np.zeros((1, 1)), ft)
        assert dcs[0, 0] == 1 and dca[0, 0] == -1 and dcg[0, 0] == ft(-0.3)
    zero_g = dict(base, asym=np.array([0.0, -0.2]))
    a = DO.reference(_one(zero_g, dasym=[1.0, 0.0]))["dJ"]
    assert np.all(np.isfinite(a.astype(float))) and np.any(a != 0)
    # ... and is the tangent of the branch asym <= 0: the one-sided difference from below in long double
    h = LD(1e-6)
    J = lambda g0: R._adding(*R.optics_definition(zero_g["A"], zero_g["V"], zero_g["ssa"], np.array([g0, LD(-0.2)], LD), LD), zero_g["beam"],
                             zero_g["sun"], zero_g["mu0"], zero_g["albedo"], LD)[1]
    one_sided = (J(LD(0)) - J(-h)) / h
    assert np.max(np.abs(a[0] - one_sided)) <= 1e-5 * np.max(np.abs(a))
    _agree(_one(base, dasym=[0.0, 1.0]))                                # asym < 0
    # ssa == 1 on every gas: co sits at its floor with derivative 0, d dtau still moves (f > 0); with f == 0 nothing moves
    cons = dict(base, ssa=np.array([1.0, 1.0]), asym=np.array([0.5, 0.3]))
    a = DO.reference(_one(cons, dssa=[-1.0, 0.0]))["dJ"]
    assert np.all(np.isfinite(a.astype(float))) and np.any(a != 0)
    n_gas, n_layers = cons["A"].shape[:2]
    ref = DO.reference(_one(cons, dssa=[-1.0, 0.0]), yardstick=True)
    assert R.ratio(DO.plain64(_one(cons, dssa=[-1.0, 0.0]))["dJ"], ref["dJ"], DO.bound(ref["S_dJ"], n_gas, n_layers)) <= 0.5
    still = dict(base, ssa=np.array([1.0, 1.0]), asym=np.array([0.0, 0.0]))
    for fn in (DO.reference, DO.plain64):
        assert np.all(fn(_one(still, dssa=[-1.0, 0.5]))["dJ"] == 0)      # dsp = -dal exactly (d dtau = 0), g = 0 stays: nothing moves
    # ssa == 0 on a gas (g = 0 where nothing scatters has derivative 0), and on every gas under a bright ground
    _agree(_one(dict(base, ssa=np.array([0.8, 0.0])), dssa=[0.0, 1.0], dasym=[0.0, 1.0]))
    dark = _one(dict(base, ssa=np.array([0.0, 0.0])), dssa=[1.0, 0.5], dasym=[1.0, 1.0], dalb=[1.0])
    for fn in (DO.reference, DO.plain64):
        assert np.all(np.isfinite(np.asarray(fn(dark)["dJ"], float))) and np.any(fn(dark)["dJ"] != 0)
    # albedo 0 and 1: no division by the albedo (the differences take the adding form beyond [0, 1], where it is the same rational function)
    for alb in (0.0, 1.0):
        a = _agree(_one(dict(base, albedo=alb), dalb=[1.0]))
        assert np.all(a > 0)
    # a direction in the albedo with the sun at or below the horizon: the boundary sends no direct light, d Ub_0 = 0, d Rb_0 stays
    for mu0 in (0.0, -0.2):
        a = _agree(_one(dict(base, mu0=mu0), dalb=[1.0]))
        assert np.all(a > 0)
        night = _one(dict(base, mu0=mu0, sun=np.zeros_like(base["sun"])), dalb=[1.0])
        for fn in (DO.reference, DO.plain64):
            assert np.all(fn(night)["dJ"] == 0)
    # an empty layer: its range is not widened and no bit changes where a direction's gas has no column
    V = np.array(base["V"])
    V[:, 2] = 0.0
    c = _one(dict(base, V=V), dssa=[0.5, 0.0], dasym=[0.2, 0.0], dalb=[0.3])
    _agree(c)
    V2 = V.copy()
    V2[1, 4] = 0.0                                                      # gas 1 leaves the top layer: gas 1's direction stops below it
    c2 = _one(dict(base, V=V2), dssa=[0.0, 0.5])
    assert DO.masks(DO._filled(c2)).tolist() == [[0, 4]] and DO.masks(DO._filled(c)).tolist() == [[0, 5]]
    assert DO.masks(DO._filled(_one(base, dalb=[1.0]))).tolist() == [[0, 0]]
    _agree(c2)


def test_exact_cases_of_the_reference():
    c = DO.panel_case(3, 3, 65, 5, 8)
    zero = dict(c, dssa=0 * c["dssa"], dasym=0 * c["dasym"], dalb=0 * c["dalb"], dlnbeam=0 * c["dlnbeam"])
    twice = dict(c, dssa=2 * c["dssa"], dasym=2 * c["dasym"], dalb=2 * c["dalb"], dlnbeam=2 * c["dlnbeam"])
    for fn in (DO.reference, DO.plain64):
        o = fn(zero)
        assert np.all(o["dJ"] == 0) and np.all(o["jac"] == 0)
        a, b = fn(c), fn(twice)
        assert np.all(b["dJ"] == 2 * a["dJ"]) and np.all(b["jac"] == 2 * a["jac"]) and np.any(a["jac"] != 0)
        o = fn(dict(c, sun=np.zeros_like(c["sun"])))
        assert np.all(o["dJ"] == 0) and np.all(o["jac"] == 0)
        # a None is zeros
        some = fn(dict(c, dssa=None, dlnbeam=None))
        same = fn(dict(c, dssa=0 * c["dssa"], dlnbeam=0 * c["dlnbeam"]))
        assert np.array_equal(some["jac"], same["jac"])


def test_fp64_restatement_against_the_reference():
    """plain64 (the kernel's formulas in fp64) stays at <= 0.5 of b = eps (n_gas + C_OPTICS n_layers + 16) S over the GPU
    panel and 300 random columns: what fixes C_OPTICS (diffuse_optics_reference: 0.75 with C = 64)."""
    worst = dict(jac=(0.0, None), dJ=(0.0, None))
    cases = [(key, DO.panel_case(*key)) for key in DO.PANEL] + [(("random", i), c) for i, c in enumerate(DO.random_columns())]
    seen_zero_co = seen_empty = seen_albedo_only = seen_negative_g = False
    for key, c in cases:
        n_gas, n_layers = c["A"].shape[:2]
        seen_zero_co |= R.min_co(*R.args(c)[:4]) == 0.0
        seen_empty |= bool(np.any(c["V"].sum(axis=0) == 0.0))
        m = DO.masks(c)
        seen_albedo_only |= bool(np.any((m[:, 1] == 0) & (c["dalb"] != 0)))
        seen_negative_g |= bool(np.any((c["dasym"] != 0) & (np.asarray(c["asym"]) < 0)[None, :]))
        ref, p64 = DO.reference(c, yardstick=True), DO.plain64(c)
        for k in worst:
            r = R.ratio(p64[k], ref[k], DO.bound(ref["S_" + k], n_gas, n_layers))
            if r > worst[k][0]:
                worst[k] = (r, key + c["A"].shape)
    assert seen_zero_co and seen_empty and seen_albedo_only and seen_negative_g
    print("plain fp64 against the reference, optics directions, in units of b (C_OPTICS = %d): jac %.3f at %s, dJ %.3f at %s"
          % ((DO.C_OPTICS,) + worst["jac"] + worst["dJ"]))
    assert max(worst["jac"][0], worst["dJ"][0]) <= 0.5


def test_every_refusal_before_any_device_work():
    """Fake device pointers: a refused call returns before it would touch one of them."""
    from spectrobot_amd import _lib
    lib, dp, ip = _lib.lib, _lib.dp, _lib.ip
    n_gas, n_layers, n_par, n_rays, n_pts, n_jac = 3, 17, 5, 2, 65, 7
    rng = np.random.default_rng(1)
    V, ssa, asym = rng.uniform(0.0, 1.0, (n_gas, n_layers)), np.array([0.9, 0.0, 0.5]), np.array([0.6, 0.0, -0.2])
    dssa, dasym, dalb = rng.normal(size=(n_par, n_gas)), rng.normal(size=(n_par, n_gas)), rng.normal(size=n_par)
    slot = np.array([2, 0, 3, 6, 5], np.int32)
    fake = C.c_void_p(0x1000)
    good = dict(v=V, ssa=ssa, asym=asym, dssa=dssa, dasym=dasym, dalb=dalb, n_gas=n_gas, n_layers=n_layers, n_par=n_par, mu0=0.5, alb=0.3,
                A=fake, beam=fake, sun=fake, dlnb=fake, q=fake, n_rays=n_rays, n_pts=n_pts, slot=slot, jac=fake, rows=n_jac, dj=fake,
                desc=True, odesc=True)
    hp = lambda a: None if a is None else a.ctypes.data_as(dp)

    def call(**kw):
        a = dict(good, **kw)
        d, od = _lib.DiffuseDesc(), _lib.DiffuseOpticsDesc()
        d.n_gas, d.n_layers, d.v, d.ssa, d.asym = a["n_gas"], a["n_layers"], hp(a["v"]), hp(a["ssa"]), hp(a["asym"])
        d.mu0, d.surface_albedo = a["mu0"], a["alb"]
        od.n_par, od.dssa, od.dasym, od.dalb = a["n_par"], hp(a["dssa"]), hp(a["dasym"]), hp(a["dalb"])
        return lib.sr_diffuse_optics_jacobian_rows_dev(C.byref(d) if a["desc"] else None, C.byref(od) if a["odesc"] else None, a["A"],
                                                       a["beam"], a["sun"], a["dlnb"], a["q"], a["n_rays"], a["n_pts"],
                                                       None if a["slot"] is None else a["slot"].ctypes.data_as(ip), a["jac"],
                                                       a["rows"], 0, a["dj"], None)

    def edited(arr, at, v):
        out = arr.copy()
        out[at] = v
        return out

    ARG, LIMIT = _lib.SR_ERR_ARG, _lib.SR_ERR_LIMIT
    nan, inf = np.nan, np.inf
    cases = [("null desc", dict(desc=False), ARG), ("null odesc", dict(odesc=False), ARG), ("null v", dict(v=None), ARG),
             ("null ssa", dict(ssa=None), ARG), ("null asym", dict(asym=None), ARG),
             ("all three directions null", dict(dssa=None, dasym=None, dalb=None), ARG),
             ("null tab_abs", dict(A=None), ARG), ("null beam", dict(beam=None), ARG), ("null sun", dict(sun=None), ARG),
             ("n_gas 0", dict(n_gas=0), ARG), ("n_layers 0", dict(n_layers=0), ARG), ("n_pts 0", dict(n_pts=0), ARG),
             ("n_par 0", dict(n_par=0), ARG), ("n_par < 0", dict(n_par=-3), ARG), ("q without jac", dict(jac=None), ARG),
             ("jac without q", dict(q=None), ARG), ("no output", dict(q=None, jac=None, dj=None), ARG),
             ("jac without par_slot", dict(slot=None), ARG), ("n_rays 0", dict(n_rays=0), ARG), ("n_jac_rows 0", dict(rows=0), ARG),
             ("v negative", dict(v=edited(V, (2, 16), -1e-30)), ARG), ("v nan", dict(v=edited(V, (0, 0), nan)), ARG),
             ("ssa above 1", dict(ssa=edited(ssa, 2, 1.0 + 2.0 ** -52)), ARG), ("asym 1", dict(asym=edited(asym, 2, 1.0)), ARG),
             ("mu0 nan", dict(mu0=nan), ARG), ("albedo negative", dict(alb=-0.01), ARG), ("albedo above 1", dict(alb=1.01), ARG),
             ("dssa nan", dict(dssa=edited(dssa, (4, 2), nan)), ARG), ("dssa inf", dict(dssa=edited(dssa, (0, 0), inf)), ARG),
             ("dasym nan", dict(dasym=edited(dasym, (1, 1), nan)), ARG), ("dasym -inf", dict(dasym=edited(dasym, (2, 0), -inf)), ARG),
             ("dalb nan", dict(dalb=edited(dalb, 3, nan)), ARG), ("dalb inf", dict(dalb=edited(dalb, 0, inf)), ARG),
             ("dalb nan alone", dict(dssa=None, dasym=None, dalb=edited(dalb, 4, nan)), ARG),
             ("n_gas beyond the limit", dict(n_gas=9), LIMIT), ("n_layers beyond the limit", dict(n_layers=_lib.SR_MAX_ABS_ROWS + 1), LIMIT),
             ("n_pts beyond the limit", dict(n_pts=2000001), LIMIT),
             ("n_par beyond the limit", dict(n_par=2 ** 23 // (n_gas * n_layers) + 1), LIMIT),
             ("par_slot too large", dict(slot=edited(slot, 1, n_jac)), ARG), ("par_slot negative", dict(slot=edited(slot, 0, -1)), ARG),
             ("par_slot repeated", dict(slot=edited(slot, 2, 2)), ARG)]
    for what, kw, status in cases:
        assert call(**kw) == status, what
    # a direction that is not finite is reported before a par_slot out of range
    assert call(dalb=edited(dalb, 0, nan), slot=edited(slot, 0, -1)) == ARG


def test_engine_value_errors_need_no_gpu():
    """The Python entry's own refusals that need no tensor come first and are reached without a device: no direction at
    all, directions without a parameter, nothing asked for, out= without Q=.  Then the state is looked at: host arrays are
    refused before any device call.  The shapes of dssa / dasym / dalbedo against A's n_gas can only be compared once A
    is a CUDA tensor: those refusals are in tests/test_gpu_diffuse_optics.py."""
    from spectrobot_amd import engine
    state = (np.ones((1, 2, 3)), np.ones((1, 2)), [0.5], [0.1], np.ones((3, 3)), np.ones(3), 0.5)
    Q = np.ones((1, 2, 3))
    for dirs, q, kw, what in (((None, None, None), Q, {}, "nothing to differentiate"), ((np.zeros((0, 1)), None, None), Q, {}, "n_par"),
                              ((np.zeros(2), None, None), Q, {}, "n_par, n_gas"), ((None, None, 0.5), Q, {}, "n_par"),
                              ((np.zeros((2, 1)), None, np.zeros(3)), Q, {}, "n_par"),
                              ((np.zeros((2, 1)), None, None), None, {}, "nothing asked for"),
                              ((np.zeros((2, 1)), None, None), None, dict(tangent=True, accumulate=True), "belong to the product"),
                              ((np.zeros((2, 1)), None, None), Q, {}, "CUDA")):
        with pytest.raises(ValueError, match=what):
            engine.diffuse_optics_jacobian(*state, *dirs, None, q, **kw)


def test_pure_asym_directions_against_the_column_s_largest_tangent():
    """The directions the yardstick's S cannot bound pointwise (asym alone, the beam held fixed: dsg's path by itself), over
    the panel's shapes: plain64 against the reference within 0.5 eps (n_gas + C_OPTICS n_layers + 16) of the column's largest S
    (DO.column_bound: the yardstick with S's maximum over the layers), times sum_l Q for jac.  The GPU test asserts 1 on the same cases."""
    worst = 0.0
    for key in DO.PANEL:
        c = DO.pure_asym_case(*key)
        ref, p64 = DO.reference(c, yardstick=True), DO.plain64(c)
        b = DO.column_bound(ref, c["Q"], *c["A"].shape[:2])
        worst = max(worst, R.ratio(p64["dJ"], ref["dJ"], b["dJ"]), R.ratio(p64["jac"], ref["jac"], b["jac"]))
    print("pure asym directions, plain fp64 against the reference in units of the column bound: %.3f" % worst)
    assert worst <= 0.5


class _Gas(object):
    def __init__(self, name, solar=None):
        self.name, self.vmr, self.iso_ratio, self.solar, self.coeffs, self.thermal = name, np.ones(4), 1.0, solar, None, None


def test_haze_optics_projection_and_refusals():
    from spectrobot_amd import retrieval as rt, spect_main_module as smm
    ho = rt.HazeOptics(albedo={"haze": (0.9, 0.1)}, g={"haze": (0.5, 0.1, 0.4)}, surface_albedo=(0.3, 0.2, 0.1))
    assert ho.name == "optics" and ho.n_par == 3 and ho.keys == [("albedo", "haze"), ("g", "haze"), ("surface_albedo", None)]
    assert ho.values() == [0.9, 0.4, 0.1] and isinstance(ho, smm.RetSet)
    for values, want in (([1.3, 1.7, -0.2], [1.0, rt.HazeOptics.G_MAX, 0.0]), ([-0.1, -0.8, 1.5], [0.0, -0.5, 1.0]),
                         ([1.0, 0.0, 0.0], [1.0, 0.0, 0.0])):
        for par, v in zip(ho.set, values):
            par.value = v
        ho.project()
        assert ho.values() == want and ho.values()[1] < 1.0            # closed ends at 0, 1 and -0.5; open at g = 1
    for bad in (dict(), dict(albedo={"haze": (1.2, 0.1)}), dict(g={"haze": (1.0, 0.1)}), dict(g={"haze": (0.5, 0.1, -0.6)}),
                dict(surface_albedo=(0.3, 0.0)), dict(surface_albedo=(0.3,)), dict(surface_albedo=(0.3, 0.1, 0.2, 0.1))):
        with pytest.raises(ValueError):
            rt.HazeOptics(**bad)
    # into the scene: projected first, then g.solar and the sun; solar_key sees both
    z = np.linspace(100.0, 400.0, 4)
    haze = rt.TableGas("haze", None, np.ones(4), solar=dict(albedo=0.9, g=0.5))
    haze.coeffs = haze.thermal = (object(), object())
    scene = rt.LimbScene(2950.0 + 0.01 * np.arange(8), z, np.full(4, 150.0), np.full(4, 1.0), [haze], [3389.0], [5.0],
                         sun=rt.Sun(60.0, 30.0, np.ones(8), multiple=True, surface_albedo=0.3))
    key0 = scene.solar_key(0, 8)
    bs = smm.BayesSet(tag="optics")
    bs.add_set(ho)
    for par, v in zip(bs.sets["optics"].set, (0.7, 1.4, 0.25)):      # (the BayesSet holds its own copy of the set)
        par.value = v
    rt._state_into_gases(scene, bs)
    assert haze.solar == dict(albedo=0.7, g=rt.HazeOptics.G_MAX) and scene.sun.surface_albedo == 0.25
    assert scene.solar_key(0, 8) != key0
    haze.solar["g"] = 0.5
    scene.sun.surface_albedo = 0.3
    haze.solar["albedo"] = 0.9
    assert scene.solar_key(0, 8) == key0
    # every other driver refuses the set; the scene method refuses the ground without multiple scattering
    with pytest.raises(ValueError, match="optics"):
        rt._refuse_instr(bs, "inversion_fast_limb")
    scene.sun = rt.Sun(60.0, 30.0, np.ones(8))
    with pytest.raises(ValueError, match="surface_albedo"):
        scene.optics_jacobian(None, None, [("surface_albedo", None)], None)
    with pytest.raises(ValueError):
        scene.optics_jacobian(None, None, [("albedo", "nothing")], None)
    assert scene.keep_mean_intensity is False and scene.diffuse_J is None


def test_hg_phase_dg_against_differences_of_hg_phase():
    from spectrobot_amd import geometry as G
    c = np.linspace(-1.0, 1.0, 41)
    for g in (-0.45, -0.1, 0.0, 0.3, 0.7, 0.9):
        h = 1e-5
        fd1 = (G.hg_phase(c, g + h) - G.hg_phase(c, g - h)) / (2 * h)
        fd2 = (G.hg_phase(c, g + h / 2) - G.hg_phase(c, g - h / 2)) / h
        K = G.hg_phase_dg(c, g)
        assert np.all(np.abs(K - fd2) <= 2 * np.abs(fd1 - fd2) + 1e-9 * np.max(np.abs(K)))
    assert np.all(G.hg_phase_dg(c, 0.0) == 3.0 * c)                     # P = 1 + 3 g cos Theta + O(g^2)
    mu = np.polynomial.legendre.leggauss(64)
    assert abs(np.sum(mu[1] * G.hg_phase_dg(mu[0], 0.6))) <= 1e-12      # the normalisation does not move
    with pytest.raises(ValueError):
        G.hg_phase_dg(0.5, 1.0)
