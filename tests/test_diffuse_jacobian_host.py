"""The diffuse rows in the Jacobians (engine.diffuse_jacobian, geometry.vertical_column_weights,
LimbScene.keep_diffuse_state, inversion_state(diffuse_jacobian=), sr_diffuse_jacobian_rows_dev) checked on the host, no GPU:
the ABI surface, the analytic tangent against differences of the forward reference, the fp64 restatement of the kernel's
formulas against the reference, exact cases, the column weights against the columns they are the derivative of, every
refusal with fake device pointers, the driver's refusal above four gas slots and the default passes, which must run the
statements they ran before."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import columns_reference as CR
import diffuse_jacobian_reference as DJ
import diffuse_source_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LD = np.longdouble


def test_abi_surface():
    from spectrobot_amd import _lib, engine
    header = open(os.path.join(ROOT, "include", "spectrobot_hip.h")).read()
    assert re.search(r"^int sr_diffuse_jacobian_rows_dev\(const sr_diffuse_desc \*desc, const sr_diffuse_jac_desc \*jdesc,", header, re.M)
    assert re.search(r"\} sr_diffuse_jac_desc;", header)
    assert "sr_diffuse_jacobian_rows_dev" in _lib.SYMBOLS and hasattr(_lib.lib, "sr_diffuse_jacobian_rows_dev")
    assert [n for n, _ in _lib.DiffuseJacDesc._fields_] == ["n_par", "dv"]
    assert _lib.lib.sr_abi_version() == 1
    plan = open(os.path.join(ROOT, "spectrobot_amd", "csrc", "sr_solar_plan.hpp")).read()
    assert int(re.search(r"kDiffuseJacPars = (\d+);", plan)[1]) == engine.DIFFUSE_JAC_PARS == DJ.PAR_TILE
    assert int(re.search(r"kDiffuseJacRays = (\d+);", plan)[1]) == engine.DIFFUSE_JAC_RAYS == DJ.RAY_TILE
    # the panel crosses a parameter tile and a ray tile, and holds every value of the five lists
    for i, want in enumerate(((1, 2, 3, 17, 80), (1, 3, 8), (1, 63, 65, 257), (1, 2, 5, 9), (1, 8, 9))):
        assert sorted(set(k[i] for k in DJ.PANEL)) == list(want)


def test_reference_against_differences_of_the_forward_reference():
    """The analytic tangent against central differences of diffuse_source_reference's long-double adding form (two
    Richardson levels), on 40 random columns, both figures as the largest over the same cases, in units of the column's
    largest |dJ|.  Asserted: |reference - fd| <= 2 x |r1b - r1a|, the agreement of the two first-level values (measured:
    0.86 of it).  The distance of the last two levels, |r2 - r1b|, is a fifteenth of that by construction, and r2 carries
    0.9 of the rounding of r1b - r1a (fd_reference's docstring): ten times |r2 - r1b| is 0.67 |r1b - r1a|, below r2's own
    rounding, so that form of the bound is printed (measured: 12.9 x |r2 - r1b|) and the one in |r1b - r1a| asserted."""
    self_worst = diff_worst = 0.0
    n = 0
    for c in DJ.fd_columns():
        ref = DJ.reference(c)["dJ"][0]
        fd, own = DJ.fd_reference(c)
        top = np.max(np.abs(ref))
        if top == 0:
            assert np.all(fd == 0)
            continue
        n += 1
        self_worst = max(self_worst, float(np.max(own) / top))
        diff_worst = max(diff_worst, float(np.max(np.abs(ref - fd)) / top))
    print("tangent against differences on %d columns, in units of the column's largest |dJ|: |r1b - r1a| %.2e, |r2 - r1b| %.2e, "
          "|reference - fd| %.2e = %.2f |r1b - r1a| = %.1f |r2 - r1b|"
          % (n, self_worst, self_worst / 15, diff_worst, diff_worst / self_worst, 15 * diff_worst / self_worst))
    assert n >= 30 and diff_worst <= 2 * self_worst


def test_fp64_restatement_against_the_reference():
    """plain64 (the kernel's formulas in fp64) stays at <= 0.5 of b over the GPU panel and 300 random columns: what fixes
    C_LAYER."""
    worst = dict(jac=(0.0, None), dJ=(0.0, None))
    cases = [(key, DJ.panel_case(*key)) for key in DJ.PANEL] + [(("random", i), c) for i, c in enumerate(DJ.random_columns())]
    seen_zero_co = seen_empty = seen_beam_only = False
    for key, c in cases:
        n_gas, n_layers = c["A"].shape[:2]
        seen_zero_co |= R.min_co(*R.args(c)[:4]) == 0.0
        seen_empty |= bool(np.any(c["V"].sum(axis=0) == 0.0))
        seen_beam_only |= bool(c["dV"].shape[0] > 1 and not c["dV"][1].any())
        assert not np.any(c["dV"][:, :, c["V"].sum(axis=0) == 0.0])          # dV on non-empty layers only
        ref, p64 = DJ.reference(c, yardstick=True), DJ.plain64(c)
        for k in worst:
            r = R.ratio(p64[k], ref[k], DJ.bound(ref["S_" + k], n_gas, n_layers))
            if r > worst[k][0]:
                worst[k] = (r, key + c["A"].shape)
    assert seen_zero_co and seen_empty and seen_beam_only
    print("plain fp64 against the reference, in units of b (C_LAYER = %d): jac %.3f at %s, dJ %.3f at %s"
          % ((DJ.C_LAYER,) + worst["jac"] + worst["dJ"]))
    assert max(worst["jac"][0], worst["dJ"][0]) <= 0.5


def test_fp64_restatement_with_physical_directions():
    """The directions a scene really makes -- dlnbeam the shadow of the parameter's own column, opposite in sign to its dV --
    against the yardstick by parts (the dV part and the dlnbeam part of a source layer as addends of their own): plain64
    at <= 0.5 of b over the panel and 100 random columns, with the same C_LAYER."""
    worst = dict(jac=(0.0, None), dJ=(0.0, None))
    cases = [(key, DJ.panel_case(*key)) for key in DJ.PANEL] + [(("random", i), c) for i, c in enumerate(DJ.random_columns(100))]
    for key, c in cases:
        c = DJ.physical_directions(c)
        n_gas, n_layers = c["A"].shape[:2]
        moved = np.any(c["dV"] != 0, axis=1)
        assert np.all(c["dlnbeam"][:, :-1][moved] * np.sign(c["dV"].sum(axis=1))[moved][:, None] <= 0)
        ref, p64 = DJ.reference(c, yardstick="parts"), DJ.plain64(c)
        for k in worst:
            r = R.ratio(p64[k], ref[k], DJ.bound(ref["S_" + k], n_gas, n_layers))
            if r > worst[k][0]:
                worst[k] = (r, key + c["A"].shape)
    print("plain fp64 against the reference, physical directions, in units of b by parts (C_LAYER = %d): jac %.3f at %s, dJ %.3f at %s"
          % ((DJ.C_LAYER,) + worst["jac"] + worst["dJ"]))
    assert max(worst["jac"][0], worst["dJ"][0]) <= 0.5


def test_exact_cases_of_the_reference():
    c = DJ.panel_case(3, 3, 65, 5, 8)
    zero = dict(c, dV=np.zeros_like(c["dV"]), dlnbeam=np.zeros_like(c["dlnbeam"]))
    twice = dict(c, dV=2.0 * c["dV"], dlnbeam=2.0 * c["dlnbeam"])
    for fn in (DJ.reference, DJ.plain64):
        o = fn(zero)                                                   # no direction: zeros
        assert np.all(o["dJ"] == 0) and np.all(o["jac"] == 0)
        a, b = fn(c), fn(twice)                                        # a direction x 2: bits x 2
        assert np.all(b["dJ"] == 2 * a["dJ"]) and np.all(b["jac"] == 2 * a["jac"]) and np.any(a["jac"] != 0)
        o = fn(dict(c, sun=np.zeros_like(c["sun"])))                   # shadow
        assert np.all(o["dJ"] == 0) and np.all(o["jac"] == 0)


def test_tangent_rules_of_the_floor_the_empty_layer_and_the_pure_absorber():
    for ft in (LD, np.float64):
        one = lambda v: np.array([v], ft)
        kw = dict(D=one(3.0), mu0=0.6, dD=one(0.0), ft=ft)
        # the floor: al / dtau = 1e-17 <= 2^-52, so co is the constant 2^-52 and only dtau moves -- the same tangent whether
        # dtau grows by an absorber's column or by the scatterer's with g kept (without the rule d co would be 1 against 0)
        sp, al, sg = one(1.0), one(1e-17), one(0.3)
        a = DJ.layer_tangent(sp, al, sg, dsp=one(0.0), dal=one(1.0), dsg=one(0.0), **kw)
        b = DJ.layer_tangent(sp, al, sg, dsp=one(1.0), dal=one(0.0), dsg=one(0.3), **kw)
        for k in a:
            assert abs(a[k][0] - b[k][0]) <= 8 * np.finfo(ft).eps * max(abs(a[k][0]), abs(b[k][0])), (k, a[k], b[k])
        assert a["T"][0] < 0
        # above the floor the two directions differ
        a = DJ.layer_tangent(sp, one(1e-3), sg, dsp=one(0.0), dal=one(1.0), dsg=one(0.0), **kw)
        b = DJ.layer_tangent(sp, one(1e-3), sg, dsp=one(1.0), dal=one(0.0), dsg=one(0.3), **kw)
        assert abs(a["R"][0] - b["R"][0]) > 0.1 * abs(b["R"][0])
        # sp == 0 (a pure absorber): g = 0 as built, with derivative 0 -- dsg does not enter
        a = DJ.layer_tangent(one(0.0), one(0.5), one(0.0), dsp=one(0.2), dal=one(0.1), dsg=one(0.0), **kw)
        b = DJ.layer_tangent(one(0.0), one(0.5), one(0.0), dsp=one(0.2), dal=one(0.1), dsg=one(0.15), **kw)
        assert all(np.array_equal(a[k], b[k]) for k in a) and a["R"][0] != 0
        # dtau == 0: every operator derivative is 0 whatever the direction
        a = DJ.layer_tangent(one(0.0), one(0.0), one(0.0), dsp=one(0.2), dal=one(0.1), dsg=one(0.05), **dict(kw, dD=one(1.0)))
        assert all(v[0] == 0 for v in a.values())
    # through the whole solve: dV on an empty layer changes no bit
    c = DJ.panel_case(17, 3, 65, 5, 8)
    V = np.array(c["V"])
    V[:, 5] = 0.0
    dV = np.array(c["dV"])
    dV[:, :, 5] = 0.0
    dV2 = dV.copy()
    dV2[0, 1, 5], dV2[3, 0, 5] = 0.3, -2.0
    for fn in (DJ.reference, DJ.plain64):
        a, b = fn(dict(c, V=V, dV=dV)), fn(dict(c, V=V, dV=dV2))
        assert np.array_equal(a["dJ"], b["dJ"]) and np.array_equal(a["jac"], b["jac"])
    assert np.array_equal(DJ.masks(dV, V), DJ.masks(dV2, V))


def _plain_columns(L, col_scale):
    col, _ = CR.columns(2, L["x"], L["nd"], L["vmr"], pt_off=L["pt_off"], dtype=np.float64, scale=col_scale)
    return np.asarray(col, float)


def test_vertical_column_weights_are_the_derivative_of_vertical_columns():
    """sum_p x_p dV_p against vertical_columns of the profiles sum_p x_p m_p, to 64 eps of the column sum of magnitudes (the
    tolerance of the solar column weights' own test), a plain column routine on both sides."""
    from spectrobot_amd import geometry as G
    z = np.linspace(100.0, 690.0, 60) + np.where(np.arange(60) % 2, 1.5, 0.0)
    nd, cs = 3e17 * np.exp(-(z - 100.0) / 63.0), np.array([0.98827, 1.0, 0.5])
    rng = np.random.default_rng(9)
    n_gas, n_par = 3, 11
    par_gas = rng.integers(0, n_gas, n_par)
    par_gas[:3] = [0, 1, 2]
    masks = np.zeros((n_par, z.size))
    for p in range(n_par):
        c, h = int(rng.integers(0, z.size)), int(rng.integers(2, 12))
        masks[p] = np.clip(1.0 - np.abs(np.arange(z.size) - c) / h, 0.0, None) * rng.choice([-1.0, 1.0])
    x = rng.uniform(0.5, 2.0, n_par) * 1e-3
    args = (G.TITAN_RADIUS_KM, 3, cs, _plain_columns)
    dV = G._vertical_column_weights(z, nd, masks, par_gas, n_gas, *args)
    assert dV.shape == (n_par, n_gas, z.size) and np.all(np.isfinite(dV)) and (dV < 0).any() and (dV > 0).any()
    for p in range(n_par):
        others = np.setdiff1d(np.arange(n_gas), [par_gas[p]])
        assert np.all(dV[p][others] == 0) and np.any(dV[p][par_gas[p]] != 0)
    profiles = np.zeros((n_gas, z.size))
    for p in range(n_par):
        profiles[par_gas[p]] += x[p] * masks[p]
    V = G._vertical_columns(z, nd, profiles, *args)
    got = np.tensordot(x, dV, axes=(0, 0))
    size = np.tensordot(np.abs(x), np.abs(dV), axes=(0, 0)).sum()
    tol = 64 * 2.0 ** -53 * size
    print("sum_p x_p dV_p against vertical_columns, in units of 64 eps of the column sum: %.3f" % float(np.max(np.abs(got - V)) / tol))
    assert np.all(np.abs(got - V) <= tol)
    # it is solar_column_weights' row for the point z[0] with mu = 1
    dU, _ = G._solar_column_weights(z, nd, masks, par_gas, n_gas, [z[0]], 1.0, *args)
    assert np.array_equal(dV, dU[:, 0])


def test_every_refusal_before_any_device_work():
    """Fake device pointers: a refused call returns before it would touch one of them."""
    from spectrobot_amd import _lib
    lib, dp, ip = _lib.lib, _lib.dp, _lib.ip
    n_gas, n_layers, n_par, n_rays, n_pts, n_jac = 3, 17, 5, 2, 65, 7
    rng = np.random.default_rng(1)
    V, ssa, asym = rng.uniform(0.0, 1.0, (n_gas, n_layers)), np.array([0.9, 0.0, 0.5]), np.array([0.6, 0.0, -0.2])
    dV = rng.normal(size=(n_par, n_gas, n_layers)) * (rng.random((n_par, n_gas, n_layers)) < 0.1)
    slot = np.array([2, 0, 3, 6, 5], np.int32)
    fake = C.c_void_p(0x1000)
    good = dict(v=V, ssa=ssa, asym=asym, dv=dV, n_gas=n_gas, n_layers=n_layers, n_par=n_par, mu0=0.5, alb=0.3, A=fake, beam=fake,
                sun=fake, dlnb=fake, q=fake, n_rays=n_rays, n_pts=n_pts, slot=slot, jac=fake, rows=n_jac, dj=fake, desc=True, jdesc=True)
    hp = lambda a: None if a is None else a.ctypes.data_as(dp)

    def call(**kw):
        a = dict(good, **kw)
        d, jd = _lib.DiffuseDesc(), _lib.DiffuseJacDesc()
        d.n_gas, d.n_layers, d.v, d.ssa, d.asym = a["n_gas"], a["n_layers"], hp(a["v"]), hp(a["ssa"]), hp(a["asym"])
        d.mu0, d.surface_albedo = a["mu0"], a["alb"]
        jd.n_par, jd.dv = a["n_par"], hp(a["dv"])
        return lib.sr_diffuse_jacobian_rows_dev(C.byref(d) if a["desc"] else None, C.byref(jd) if a["jdesc"] else None, a["A"], a["beam"],
                                                a["sun"], a["dlnb"], a["q"], a["n_rays"], a["n_pts"],
                                                None if a["slot"] is None else a["slot"].ctypes.data_as(ip), a["jac"], a["rows"], 0,
                                                a["dj"], None)

    def edited(arr, at, v):
        out = arr.copy()
        out[at] = v
        return out

    ARG, LIMIT = _lib.SR_ERR_ARG, _lib.SR_ERR_LIMIT
    nan, inf = np.nan, np.inf
    cases = [("null desc", dict(desc=False), ARG), ("null jdesc", dict(jdesc=False), ARG), ("null v", dict(v=None), ARG),
             ("null ssa", dict(ssa=None), ARG), ("null asym", dict(asym=None), ARG), ("null dv", dict(dv=None), ARG),
             ("null tab_abs", dict(A=None), ARG), ("null beam", dict(beam=None), ARG), ("null sun", dict(sun=None), ARG),
             ("n_gas 0", dict(n_gas=0), ARG), ("n_layers 0", dict(n_layers=0), ARG), ("n_pts 0", dict(n_pts=0), ARG),
             ("n_par 0", dict(n_par=0), ARG), ("n_par < 0", dict(n_par=-3), ARG), ("q without jac", dict(jac=None), ARG),
             ("jac without q", dict(q=None), ARG), ("no output", dict(q=None, jac=None, dj=None), ARG),
             ("jac without par_slot", dict(slot=None), ARG), ("n_rays 0", dict(n_rays=0), ARG), ("n_jac_rows 0", dict(rows=0), ARG),
             ("v negative", dict(v=edited(V, (2, 16), -1e-30)), ARG), ("v nan", dict(v=edited(V, (0, 0), nan)), ARG),
             ("v inf", dict(v=edited(V, (1, 3), inf)), ARG), ("ssa negative", dict(ssa=edited(ssa, 0, -0.1)), ARG),
             ("ssa above 1", dict(ssa=edited(ssa, 2, 1.0 + 2.0 ** -52)), ARG), ("ssa nan", dict(ssa=edited(ssa, 1, nan)), ARG),
             ("asym below -0.5", dict(asym=edited(asym, 0, -0.5000001)), ARG), ("asym 1", dict(asym=edited(asym, 2, 1.0)), ARG),
             ("mu0 above 1", dict(mu0=1.0000001), ARG), ("mu0 nan", dict(mu0=nan), ARG), ("albedo negative", dict(alb=-0.01), ARG),
             ("albedo above 1", dict(alb=1.01), ARG),
             ("dv nan", dict(dv=edited(dV, (4, 2, 16), nan)), ARG), ("dv inf", dict(dv=edited(dV, (0, 0, 0), inf)), ARG),
             ("dv -inf", dict(dv=edited(dV, (2, 1, 7), -inf)), ARG),
             ("n_gas beyond the limit", dict(n_gas=9), LIMIT), ("n_layers beyond the limit", dict(n_layers=_lib.SR_MAX_ABS_ROWS + 1), LIMIT),
             ("n_pts beyond the limit", dict(n_pts=2000001), LIMIT),
             ("dv beyond the limit", dict(n_par=2 ** 23 // (n_gas * n_layers) + 1), LIMIT),
             ("par_slot too large", dict(slot=edited(slot, 1, n_jac)), ARG), ("par_slot negative", dict(slot=edited(slot, 0, -1)), ARG),
             ("par_slot repeated", dict(slot=edited(slot, 2, 2)), ARG)]
    for what, kw, status in cases:
        assert call(**kw) == status, what
    # a dv that is not finite is reported before a par_slot out of range
    assert call(dv=edited(dV, (0, 0, 0), nan), slot=edited(slot, 0, -1)) == ARG


def test_engine_value_errors_need_no_gpu():
    """The Python entry looks at its tensors first: host arrays are refused before any device call."""
    from spectrobot_amd import engine
    with pytest.raises(ValueError):
        engine.diffuse_jacobian(np.ones((1, 2, 3)), np.ones((1, 2)), [0.5], [0.1], np.ones((3, 3)), np.ones(3), 0.5, np.zeros((2, 1, 2)),
                                None, np.ones((1, 2, 3)))


class _Gas(object):
    def __init__(self, name, vmr, tab):
        self.name, self.vmr, self.iso_ratio, self.coeffs, self.thermal, self.solar = name, np.asarray(vmr, float), 1.0, (tab, tab), None, None


def _scene(n_gases, multiple=True):
    from spectrobot_amd import retrieval as rt
    grid = 2950.0 + 0.01 * np.arange(8)
    z = np.linspace(100.0, 400.0, 4)
    haze = rt.TableGas("haze", None, np.ones(4), solar=dict(albedo=0.9, g=0.5))
    haze.coeffs = haze.thermal = (object(), object())
    gases = [_Gas("gas%d" % i, np.full(4, 0.01), object()) for i in range(n_gases - 1)] + [haze]
    return rt.LimbScene(grid, z, np.full(4, 150.0), np.full(4, 1.0), gases, [3389.0], [5.0],
                        sun=rt.Sun(60.0, 30.0, np.ones(8), multiple=multiple, surface_albedo=0.3))


def test_inversion_state_refuses_the_term_above_four_gas_slots():
    from spectrobot_amd import retrieval as rt, spect_main_module as smm
    scene = _scene(5)
    bs = smm.BayesSet(tag="five slots")
    bs.add_set(smm.LinearProfile_1D_new("gas0", scene.z, scene.z[[0, 3]], np.full(2, 0.01), np.full(2, 0.005)))
    pix = rt.LimbPixel(150.0, observation=rt.Spectrum(np.ones(1), scene.bands_nm), noise=rt.Spectrum(np.ones(1), scene.bands_nm))
    with pytest.raises(ValueError, match="four-gas"):
        rt.inversion_state(scene, bs, [pix], diffuse_jacobian=True)
    assert scene.keep_diffuse_state is False             # refused before anything was changed
    with pytest.raises(ValueError, match="keep_diffuse_state"):
        _scene(2).diffuse_jacobian(None, None, None, None)


def test_default_passes_run_the_statements_they_ran(monkeypatch):
    """keep_diffuse_state off (the default): the solar pass of a Sun(multiple=True) makes its accumulating solar_source
    call, the beam's transmission call and ONE accumulating diffuse_source call on the same rows, and keeps nothing; on: the
    same calls, and the diffuse call's own inputs kept."""
    import torch
    from spectrobot_amd import retrieval as rt, geometry as G
    scene = _scene(2)
    gas, haze = scene.gases
    tab = torch.arange(32, dtype=torch.float64).reshape(4, 8)
    gas.coeffs = (tab, tab)
    haze.coeffs = haze.thermal = (tab + 1.0, tab + 2.0)
    calls = []

    def fake_source(A, U, w, sca, sun, src_row=None, out=None, accumulate=False, transmission=False):
        calls.append(("solar", dict(out=out, accumulate=accumulate, transmission=transmission)))
        if transmission:
            return None, torch.full((5, 8), 0.5, dtype=torch.float64)
        out += 0.25
        return out

    def fake_diffuse(A, V, ssa, asym, beam, sun, mu0, **kw):
        calls.append(("diffuse", dict(kw, A=A, V=V, beam=beam, sun=sun)))
        kw["out"] += 0.125
        return kw["out"]

    monkeypatch.setattr(rt.engine, "solar_source", fake_source)
    monkeypatch.setattr(rt.engine, "diffuse_source", fake_diffuse)
    monkeypatch.setattr(G, "solar_columns", lambda z, nd, vmr, alt, mu, **k: (np.zeros((len(alt), 2, 4)), np.ones(len(alt), bool)))
    monkeypatch.setattr(G, "vertical_columns", lambda *a, **k: np.full((2, 4), 0.75))
    monkeypatch.setattr(torch, "as_tensor", lambda a, device=None: torch.tensor(np.asarray(a)))
    assert scene.keep_diffuse_state is False
    scene.solar_pass(0, 8)
    kinds = [k for k, _ in calls]
    assert kinds == ["solar", "solar", "diffuse"]
    assert calls[0][1]["accumulate"] is True and calls[0][1]["out"] is haze.coeffs[1] and calls[1][1]["transmission"] is True
    d = calls[2][1]
    assert d["out"] is haze.coeffs[1] and d["accumulate"] is True and d["out_gas"] == 1 and d["surface_albedo"] == 0.3
    assert set(d) == {"out", "accumulate", "out_gas", "surface_albedo", "A", "V", "beam", "sun"}
    assert torch.equal(haze.coeffs[1], haze.thermal[1] + 0.375) and scene.diffuse_state is None
    scene.solar_pass(0, 8)                           # nothing moved: nothing redone
    assert len(calls) == 3
    scene.keep_diffuse_state = True
    scene._solar_key = None                          # (what inversion_state does with the flag)
    scene.solar_pass(0, 8)
    assert [k for k, _ in calls[3:]] == kinds
    d = calls[5][1]
    A, V, ssa, asym, beam, sun = scene.diffuse_state
    assert A is d["A"] and V is d["V"] and beam is d["beam"] and sun is d["sun"]
    assert list(ssa) == [0.0, 0.9] and list(asym) == [0.0, 0.5]
    assert torch.equal(haze.coeffs[1], haze.thermal[1] + 0.375)
