"""The diffuse field for several columns of illumination on the GPU (engine.diffuse_source_columns,
sr_diffuse_source_columns_dev, LimbScene.sunlit_steps) against the extended-precision reference of
tests/diffuse_columns_reference.py: the bound panel over every instance and padded calls, one column against
engine.diffuse_source, column independence, exact zeros and kept bits, repeatability, accumulate, point chunks, every
refusal class, and the 3-D scene route."""
import ctypes as C

import numpy as np
import pytest

import absorber_table_cases as K
import diffuse_columns_reference as DC
import diffuse_source_reference as R

pytestmark = pytest.mark.gpu
LD, EPS = R.LD, R.EPS53
KEYS = ("rows", "J", "flux")


@pytest.fixture(scope="module")
def eng():
    import torch
    assert torch.cuda.is_available(), "these tests need the GPU"
    from spectrobot_amd import engine
    engine.set_device(0)
    return engine


def _np(t):
    return t.detach().cpu().numpy()


def _dev(a):
    import torch
    return torch.as_tensor(np.array(a, dtype=np.float64), device="cuda")     # (a copy: the shared cases are read-only)


def _call(eng, c, **kw):
    kw.setdefault("out_gas", c["out_gas"])
    kw.setdefault("surface_albedo", c["albedo"])
    if kw["out_gas"] is not None:
        kw.setdefault("sca", _dev(c["sca"]))
        kw.setdefault("src_row", c["src_row"])
    return eng.diffuse_source_columns(_dev(c["A"]), c["V"], c["ssa"], c["asym"], _dev(c["beams"]), _dev(c["sun"]), c["mu0s"],
                                      c["col_w"], c["row_layer"], **kw)


def _case(n_layers, n_gas, n_pts, n_col):
    """A panel case with its columns, rows and reference, made once and shared (read-only)."""
    key = (n_layers, n_gas, n_pts, n_col)
    if key not in _case.cache:
        c = R.panel_case(n_layers, n_gas, n_pts)
        rng = np.random.default_rng([20261021, 41, *key])
        mu0s, beams = DC.columns_of(c, n_col)
        w, layer, src = DC.rows_of(rng, n_layers, n_col)
        sca = rng.uniform(0.5, 1.5, (n_layers + 1, n_pts))
        ref = DC.reference(c, mu0s, beams, w, layer, sca, src)
        b = DC.bounds(ref, n_gas, n_layers, n_col)
        c = dict(c, mu0s=mu0s, beams=beams, col_w=w, row_layer=layer, src_row=src, sca=sca, **{"ref_" + k: ref[k] for k in KEYS},
                 **{"b_" + k: b[k] for k in KEYS})
        for v in c.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        _case.cache[key] = c
    return _case.cache[key]


_case.cache = {}


def _panel():
    """(n_layers, n_gas, n_pts, n_col) of the panel: n_col cycles through 1, 2, 3, 5, 8."""
    i = 0
    for n_layers in R.N_LAYERS:
        for n_gas in R.N_GAS:
            for n_pts in R.N_PTS:
                yield n_layers, n_gas, n_pts, DC.N_COL[i % len(DC.N_COL)]
                i += 1


@pytest.mark.parametrize("n_layers", R.N_LAYERS)
def test_panel_inside_the_bound(eng, n_layers):
    worst = dict.fromkeys(KEYS, 0.0)
    for key in _panel():
        if key[0] != n_layers:
            continue
        c = _case(*key)
        n_rows = 2 * n_layers + 3
        assert c["col_w"].shape == (n_rows, key[3]) and np.sum(~c["col_w"].any(axis=1)) == 1
        count = np.bincount(c["row_layer"], minlength=n_layers)
        assert count.max() >= 3 and (n_layers == 1 or count.min() == 0)
        got = dict(zip(KEYS, _call(eng, c, mean_intensity=True, fluxes=True)))
        for k in KEYS:
            g = _np(got[k])
            assert np.all(np.isfinite(g)) and np.all(g >= 0), (k, key)
            worst[k] = max(worst[k], R.ratio(g, c["ref_" + k], c["b_" + k]))
        # the other instances give the same bits
        assert np.array_equal(_np(_call(eng, c)), _np(got["rows"]))
        e2, j2 = _call(eng, c, mean_intensity=True)
        assert np.array_equal(_np(e2), _np(got["rows"])) and np.array_equal(_np(j2), _np(got["J"]))
        j3, f3 = _call(eng, c, out_gas=None, mean_intensity=True, fluxes=True)
        assert np.array_equal(_np(j3), _np(got["J"])) and np.array_equal(_np(f3), _np(got["flux"]))
    print("\ndiffuse columns panel, n_layers %d: |GPU - reference| / b %s" % (n_layers, worst))
    assert max(worst.values()) <= 1.0, worst


def test_one_column_against_the_single_source(eng):
    """n_col = 1 and row_layer = arange: within 2 b of engine.diffuse_source on the same inputs (each within b of the
    reference; the sources are factored in another order)."""
    worst = 0.0
    for key in ((17, 3, 257), (80, 8, 65), (2, 1, 63)):
        c = R.panel_case(*key)
        n_layers, n_gas = key[0], key[1]
        ref = R.reference(*R.args(c))
        A, beam, sun = _dev(c["A"]), _dev(c["beam"]), _dev(c["sun"])
        one = eng.diffuse_source(A, c["V"], c["ssa"], c["asym"], beam, sun, c["mu0"], surface_albedo=c["albedo"], out_gas=0,
                                 mean_intensity=True, fluxes=True)
        col = eng.diffuse_source_columns(A, c["V"], c["ssa"], c["asym"], beam[None].contiguous(), sun, [c["mu0"]], np.ones((n_layers, 1)),
                                         np.arange(n_layers), surface_albedo=c["albedo"], out_gas=0, mean_intensity=True, fluxes=True)
        for k, a, b in zip(("emi", "J", "flux"), one, col):
            b = _np(b)[0] if k != "emi" else _np(b)
            worst = max(worst, R.ratio(_np(a) - b, np.zeros(b.shape, LD), 2 * R.bound(ref[k], n_gas, n_layers)))
    print("\none column against diffuse_source: |difference| / 2 b %.3f" % worst)
    assert worst <= 1.0


def test_a_column_does_not_depend_on_its_neighbours(eng):
    c = _case(17, 3, 65, 3)
    j3, f3 = _call(eng, c, out_gas=None, mean_intensity=True, fluxes=True)
    pick = [2, 0]
    c2 = dict(c, mu0s=c["mu0s"][pick], beams=np.ascontiguousarray(c["beams"][pick]))
    j2, f2 = _call(eng, c2, out_gas=None, mean_intensity=True, fluxes=True)
    for a, b in ((j3, j2), (f3, f2)):
        assert np.array_equal(_np(a)[pick].view(np.uint64), _np(b).view(np.uint64))


def test_exact_zeros_and_untouched_bits(eng):
    import torch
    c = _case(17, 3, 65, 3)
    zero = np.zeros(3)
    n_rows = c["col_w"].shape[0]
    dark_row = int(np.flatnonzero(~c["col_w"].any(axis=1))[0])
    # no scatterer, a black lower boundary: no diffuse light at all
    e, J, F = _call(eng, dict(c, ssa=zero), surface_albedo=0.0, mean_intensity=True, fluxes=True)
    assert not _np(e).any() and not _np(J).any() and not _np(F).any()
    # no sunlight in any column and a black boundary
    e, J, F = _call(eng, dict(c, beams=np.zeros_like(c["beams"])), surface_albedo=0.0, mean_intensity=True, fluxes=True)
    assert not _np(e).any() and not _np(J).any() and not _np(F).any()
    # a row whose weights are all zero is an exact 0 ...
    e = _np(_call(eng, c))
    assert not e[dark_row].any() and np.all(np.delete(e, dark_row, axis=0) > 0)
    # ... and under accumulate it keeps its bits (a -0.0 among them); so does every row when the gas scatters nothing
    base = np.random.default_rng(3).uniform(-1.0, 1.0, (n_rows, 65))
    base[:, 7] = -0.0
    acc = _dev(base)
    _call(eng, c, out=acc, accumulate=True)
    assert np.array_equal(_np(acc)[dark_row].view(np.uint64), base[dark_row].view(np.uint64))
    assert np.all(np.delete(_np(acc), dark_row, axis=0) >= np.delete(base, dark_row, axis=0))
    acc = _dev(base)
    ssa0 = np.array(c["ssa"])
    ssa0[0] = 0.0
    _call(eng, dict(c, ssa=ssa0, mu0s=np.full(3, 0.8)), surface_albedo=0.6, out=acc, accumulate=True)
    assert np.array_equal(_np(acc).view(np.uint64), base.view(np.uint64))
    e, F = _call(eng, dict(c, ssa=ssa0, mu0s=np.full(3, 0.8)), surface_albedo=0.6, fluxes=True)
    assert not _np(e).any() and np.all(_np(F)[:, 0] > 0)


def test_two_calls_give_the_same_bits_and_accumulate_adds(eng):
    c = _case(80, 3, 257, 5)
    a, b = _call(eng, c, mean_intensity=True, fluxes=True), _call(eng, c, mean_intensity=True, fluxes=True)
    for x, y in zip(a, b):
        assert np.array_equal(_np(x).view(np.uint64), _np(y).view(np.uint64))
    base = np.random.default_rng(5).uniform(0.0, 2.0, _np(a[0]).shape) * float(_np(a[0]).max())
    acc = _dev(base)
    _call(eng, c, out=acc, accumulate=True)
    assert np.array_equal(_np(acc), base + _np(a[0]))                # overwrite plus base, one rounding


def test_a_call_in_point_chunks_gives_the_bits_of_its_parts(eng):
    """4096 layers x 512 points x 8 columns need 288 MiB of workspace: above 256 MiB the entry launches point chunks (here
    two of 256 points) on one workspace.  The points are independent, so each part called alone gives the same bits."""
    import torch
    rng = np.random.default_rng(17)
    N, n_pts, n_col, n_rows = 4096, 512, 8, 64
    A = torch.as_tensor(rng.uniform(0.5, 1.5, (1, N, n_pts)), device="cuda")
    depth = np.exp(-np.linspace(3.0, 0.0, N + 1))
    beams = torch.as_tensor(np.stack([depth ** (0.5 + 0.1 * k) for k in range(n_col)])[:, :, None] * rng.uniform(0.9, 1.0, (n_col, N + 1, n_pts)),
                            device="cuda")
    sun = torch.as_tensor(rng.uniform(5.0, 20.0, n_pts), device="cuda")
    V = np.full((1, N), 2.0 / N)
    mu0s = np.linspace(-0.1, 0.8, n_col)
    w = rng.uniform(0.0, 1.0, (n_rows, n_col))
    layer = rng.integers(0, N, n_rows)
    call = lambda sl: eng.diffuse_source_columns(A[:, :, sl].contiguous(), V, [0.95], [0.6], beams[:, :, sl].contiguous(),
                                                 sun[sl].contiguous(), mu0s, w, layer, surface_albedo=0.4, out_gas=0, fluxes=True)
    e, F = call(slice(0, n_pts))
    assert bool(torch.isfinite(e).all()) and float(e.min()) > 0.0
    for sl in (slice(0, 256), slice(256, n_pts)):
        e1, F1 = call(sl)
        assert torch.equal(e1, e[:, sl]) and torch.equal(F1, F[:, :, :, sl])


def test_every_refusal_leaves_the_outputs_untouched(eng):
    import torch
    from spectrobot_amd import _lib
    lib, dp, ip = _lib.lib, _lib.dp, _lib.ip
    n_layers, n_gas, n_pts, n_col = 17, 3, 65, 3
    c = _case(n_layers, n_gas, n_pts, n_col)
    n_rows, n_src = c["col_w"].shape[0], c["sca"].shape[0]
    A, beams, sun, sca = _dev(c["A"]), _dev(c["beams"]), _dev(c["sun"]), _dev(c["sca"])
    shapes = ((n_rows, n_pts), (n_col, n_layers, n_pts), (n_col, 2, n_layers + 1, n_pts))
    bufs = [torch.full(s, -7.0, dtype=torch.float64, device="cuda") for s in shapes]
    V, ssa, asym = np.array(c["V"]), np.array(c["ssa"]), np.array(c["asym"])
    mu0s, w = np.array(c["mu0s"]), np.array(c["col_w"])
    layer, src = np.array(c["row_layer"], np.int32), np.array(c["src_row"], np.int32)
    good = dict(v=V, ssa=ssa, asym=asym, n_gas=n_gas, n_layers=n_layers, mu0=np.nan, alb=c["albedo"], A=A, beams=beams, sun=sun,
                n_pts=n_pts, sca=sca, n_src=n_src, G=0, acc=0, e=bufs[0], j=bufs[1], f=bufs[2], desc=True, cols=True, n_col=n_col,
                n_rows=n_rows, mu0s=mu0s, w=w, layer=layer, src=src)     # (desc's own mu0 is not read: a NaN there is fine)
    ptr = lambda t: None if t is None else C.c_void_p(t.data_ptr())
    hp = lambda a: None if a is None else a.ctypes.data_as(dp)
    hi = lambda a: None if a is None else a.ctypes.data_as(ip)

    def call(**kw):
        a = dict(good, **kw)
        d = _lib.DiffuseDesc()
        d.n_gas, d.n_layers, d.v, d.ssa, d.asym = a["n_gas"], a["n_layers"], hp(a["v"]), hp(a["ssa"]), hp(a["asym"])
        d.mu0, d.surface_albedo = a["mu0"], a["alb"]
        cd = _lib.DiffuseColumnsDesc()
        cd.n_col, cd.n_rows, cd.mu0, cd.col_w, cd.row_layer, cd.src_row = a["n_col"], a["n_rows"], hp(a["mu0s"]), hp(a["w"]), hi(a["layer"]), hi(a["src"])
        return lib.sr_diffuse_source_columns_dev(C.byref(d) if a["desc"] else None, C.byref(cd) if a["cols"] else None, ptr(a["A"]),
                                                 ptr(a["beams"]), ptr(a["sun"]), a["n_pts"], ptr(a["sca"]), a["n_src"], a["G"], a["acc"],
                                                 ptr(a["e"]), ptr(a["j"]), ptr(a["f"]), None)

    def edited(arr, at, v):
        out = arr.copy()
        out[at] = v
        return out

    ARG, LIMIT = _lib.SR_ERR_ARG, _lib.SR_ERR_LIMIT
    nan, inf = np.nan, np.inf
    many = _lib.SR_MAX_ABS_ROWS + 1
    cases = [("null desc", dict(desc=False), ARG), ("null cols", dict(cols=False), ARG), ("null v", dict(v=None), ARG),
             ("null ssa", dict(ssa=None), ARG), ("null asym", dict(asym=None), ARG), ("null tab_abs", dict(A=None), ARG),
             ("null beam", dict(beams=None), ARG), ("null sun", dict(sun=None), ARG), ("null mu0", dict(mu0s=None), ARG),
             ("null col_w", dict(w=None), ARG), ("null row_layer", dict(layer=None), ARG), ("null src_row", dict(src=None), ARG),
             ("null sca_abs", dict(sca=None), ARG), ("n_src 0", dict(n_src=0), ARG),
             ("n_gas 0", dict(n_gas=0), ARG), ("n_layers 0", dict(n_layers=0), ARG), ("n_pts 0", dict(n_pts=0), ARG),
             ("n_col 0", dict(n_col=0), ARG), ("n_col negative", dict(n_col=-1), ARG), ("n_rows negative", dict(n_rows=-1), ARG),
             ("v negative", dict(v=edited(V, (2, 16), -1e-30)), ARG), ("v nan", dict(v=edited(V, (0, 0), nan)), ARG),
             ("ssa above 1", dict(ssa=edited(ssa, 2, 1.0 + 2.0 ** -52)), ARG), ("asym 1", dict(asym=edited(asym, 2, 1.0)), ARG),
             ("albedo negative", dict(alb=-0.01), ARG), ("albedo nan", dict(alb=nan), ARG),
             ("mu0 above 1", dict(mu0s=edited(mu0s, 1, 1.0000001)), ARG), ("mu0 below -1", dict(mu0s=edited(mu0s, 0, -1.5)), ARG),
             ("mu0 nan", dict(mu0s=edited(mu0s, 2, nan)), ARG),
             ("col_w negative", dict(w=edited(w, (3, 1), -1e-300)), ARG), ("col_w nan", dict(w=edited(w, (0, 0), nan)), ARG),
             ("col_w inf", dict(w=edited(w, (n_rows - 1, 2), inf)), ARG),
             ("row_layer too large", dict(layer=edited(layer, 4, n_layers)), ARG), ("row_layer negative", dict(layer=edited(layer, 0, -1)), ARG),
             ("src_row too large", dict(src=edited(src, n_rows - 1, n_src)), ARG), ("src_row negative", dict(src=edited(src, 2, -1)), ARG),
             ("out_gas too large", dict(G=n_gas), ARG), ("out_gas below -1", dict(G=-2), ARG),
             ("emi_out without out_gas", dict(G=-1), ARG), ("out_gas without emi_out", dict(e=None), ARG),
             ("emi_out without rows", dict(n_rows=0), ARG), ("rows without emi_out", dict(G=-1, e=None), ARG),
             ("no output", dict(G=-1, e=None, j=None, f=None, n_rows=0), ARG),
             ("n_col beyond the limit", dict(n_col=_lib.SR_MAX_DIFFUSE_COLUMNS + 1), LIMIT), ("n_rows beyond the limit", dict(n_rows=many), LIMIT),
             ("n_gas beyond the limit", dict(n_gas=9), LIMIT), ("n_layers beyond the limit", dict(n_layers=many), LIMIT),
             ("n_pts beyond the limit", dict(n_pts=2000001), LIMIT)]
    for what, kw, status in cases:
        assert call(**kw) == status, what
    torch.cuda.synchronize()
    assert all(bool((b == -7.0).all()) for b in bufs)
    # a valid call afterwards gives the reference's numbers; so does one without rows
    assert call() == 0
    torch.cuda.synchronize()
    for k, b in zip(KEYS, bufs):
        assert R.ratio(_np(b), c["ref_" + k], c["b_" + k]) <= 1.0
    keep = _np(bufs[1]).copy()
    assert call(G=-1, e=None, n_rows=0, w=None, layer=None, src=None, sca=None, n_src=0) == 0
    torch.cuda.synchronize()
    assert np.array_equal(_np(bufs[1]), keep)
    # the host layer's own refusals
    args = (A, V, ssa, asym, beams, sun, mu0s, w, layer)
    with pytest.raises(ValueError):
        eng.diffuse_source_columns(*args, out_gas=0, accumulate=True)
    with pytest.raises(ValueError):
        eng.diffuse_source_columns(A, V, ssa, asym, beams, sun, mu0s[:-1], w, layer, out_gas=0)
    with pytest.raises(ValueError):
        eng.diffuse_source_columns(A, V, ssa, asym, beams, sun, mu0s, w[:, :-1], layer, out_gas=0)
    with pytest.raises(ValueError):
        eng.diffuse_source_columns(A, V, ssa, asym, beams[:, :-1].contiguous(), sun, mu0s, w, layer, out_gas=0)
    with pytest.raises(ValueError):
        eng.diffuse_source_columns(*args)


# ---- the 3-D scene -------------------------------------------------------------------------------------------------------
N_LEVELS, N_GRID = 17, 65
GROUND = 0.3
SZA_DEG, PHASE_DEG, AZIMUTH_DEG = 55.0, 60.0, 40.0
ALBEDO, ASYMMETRY = 0.9, 0.5


def _scene(eng, multiple):
    from spectrobot_amd import retrieval, geometry, synthetic as syn
    grid = syn.make_grid(3290.0, 5e-4, N_GRID)
    atm = syn.make_atmosphere(N_LEVELS, 12)
    z = atm["z"]
    lines = syn.make_lines(60, grid, config_id=4, n_levels=12)
    lines["a_coeff"] = lines["a_coeff"] * 1e-4
    ch4 = retrieval.Gas("CH4", eng.LineSet(lines, grid, 6, 1, syn.CH4_MM, syn.CH4_LEVEL_ENERGIES), np.full(N_LEVELS, 1.48e-4),
                        syn.CH4_ISO_RATIO, tvib=atm["tvib"])
    haze = retrieval.TableGas("haze", eng.AbsorberTable(K.haze_sets(grid)), 0.5 * K.haze_profile(z), solar=dict(albedo=ALBEDO, g=ASYMMETRY))
    lam = np.linspace(1e7 / grid[-1] + 0.005, 1e7 / grid[0] - 0.005, 2)
    sun = retrieval.Sun(SZA_DEG, PHASE_DEG, geometry.solar_irradiance(grid), multiple=multiple, surface_albedo=GROUND)
    return retrieval.LimbScene(grid, z, atm["temps"], atm["press"], [ch4, haze], lam, np.full(2, 0.003), sun=sun)


def _batch(scene):
    from spectrobot_amd import geometry
    z = scene.z
    z_tans = [z[0] + f * (z[-1] - z[0]) for f in (0.1, 0.35, 0.6)]
    return geometry.limb_los_3d(z, scene.nd, [g.vmr for g in scene.gases], z_tans, SZA_DEG, AZIMUTH_DEG)


def _manual_steps(eng, scene, L3):
    """The composition of examples/solar_haze_limb.py: thermal rows gathered by the steps' shells, then order one with the
    per-step SZA under accumulate."""
    import torch
    from spectrobot_amd import geometry
    ch4, haze = scene.gases
    layer = L3["seg_alt_layer"]
    rows = torch.as_tensor(layer.astype(np.int64), device="cuda")
    scene.coefficients()
    abs_l = torch.stack([haze.thermal[0] if g is haze else g.coeffs[0] for g in scene.gases])
    step_abs = [abs_l[i][rows].contiguous() for i in range(2)]
    step_emi = [(haze.thermal if g is haze else g.coeffs)[1][rows].contiguous() for g in scene.gases]
    lo, hi = L3["pt_off"][:-1], L3["pt_off"][1:] - 1
    alt_mid = 0.5 * (L3["alt"][(lo + hi) // 2] + L3["alt"][(lo + hi + 1) // 2])
    U, lit = geometry.solar_columns(scene.z, scene.nd, [ch4.vmr, haze.vmr], alt_mid, L3["seg_mu"], col_scale=[ch4.iso_ratio, 1.0])
    w = np.where(lit, ALBEDO * geometry.hg_phase(np.cos(np.deg2rad(180.0 - PHASE_DEG)), ASYMMETRY) / (4 * np.pi), 0.0)
    sun = torch.as_tensor(scene.sun.irradiance, device="cuda")
    emi_sun = eng.solar_source(abs_l, U, w, haze.thermal[0], sun, src_row=layer, out=step_emi[1].clone(), accumulate=True)
    return abs_l, step_abs, step_emi, emi_sun, sun


def test_scene_steps_are_the_manual_composition(eng):
    import torch
    from spectrobot_amd import geometry
    scene = _scene(eng, multiple=False)
    L3 = _batch(scene)
    assert len(scene.z) == N_LEVELS and len(scene.grid) == N_GRID and len(L3["pt_off"]) - 1 == len(L3["seg_mu"])
    assert L3["seg_mu"].max() - L3["seg_mu"].min() > 0.1
    abs_l, step_abs, step_emi, emi_sun, sun = _manual_steps(eng, scene, L3)
    pairs = _scene(eng, multiple=False).sunlit_steps(L3)
    assert torch.equal(pairs[0][0], step_abs[0]) and torch.equal(pairs[1][0], step_abs[1])
    assert torch.equal(pairs[0][1], step_emi[0]) and torch.equal(pairs[1][1], emi_sun)
    # with the diffuse field: those rows plus a direct call, bit for bit
    multi = _scene(eng, multiple=True)
    for n_columns in (1, 4):
        got = multi.sunlit_steps(L3, n_columns=n_columns)
        mu_nodes, col_w = geometry.sza_columns(L3["seg_mu"], n_columns)
        ch4, haze = multi.gases
        ssa, asym, iso, pts, beam_scale = multi.diffuse_geometry([haze])
        cols = [geometry.solar_columns(multi.z, multi.nd, [ch4.vmr, haze.vmr], pts, float(m), col_scale=beam_scale) for m in mu_nodes]
        Ub, lit_b = np.concatenate([c[0] for c in cols]), np.concatenate([c[1] for c in cols])
        _, beams = eng.solar_source(abs_l, Ub, np.where(lit_b, 1.0, 0.0), abs_l[1], sun, src_row=np.zeros(len(lit_b), np.int32),
                                    transmission=True)
        beams = beams.view(len(mu_nodes), len(pts), -1)
        V = geometry.vertical_columns(multi.z, multi.nd, [ch4.vmr, haze.vmr], col_scale=iso)
        want = emi_sun.clone()
        eng.diffuse_source_columns(abs_l, V, ssa, asym, beams, sun, mu_nodes, col_w, L3["seg_alt_layer"], surface_albedo=GROUND, out_gas=1,
                                   out=want, accumulate=True)
        assert torch.equal(got[1][1], want) and torch.equal(got[0][1], step_emi[0]) and bool((want >= emi_sun).all())
        assert bool((want > emi_sun).any())


def test_scene_with_one_sza_is_the_one_dimensional_diffuse_pass(eng):
    """seg_mu overwritten by the constant sun.mu and n_columns = 1: the diffuse part of the steps' rows is
    engine.diffuse_source on scene.diffuse_inputs, gathered by the steps' shells, within 2 b."""
    import torch
    scene = _scene(eng, multiple=True)
    L3 = dict(_batch(scene))
    L3["seg_mu"] = np.full_like(L3["seg_mu"], scene.sun.mu)
    single = _scene(eng, multiple=False).sunlit_steps(L3)
    got = scene.sunlit_steps(L3, n_columns=1)
    ch4, haze = scene.gases
    A = torch.stack([ch4.coeffs[0], haze.thermal[0]]).contiguous()
    sun = torch.as_tensor(scene.sun.irradiance, device="cuda").contiguous()
    V, ssa, asym, beam = scene.diffuse_inputs([haze], A, sun)
    rows = _np(eng.diffuse_source(A, V, ssa, asym, beam, sun, scene.sun.mu, surface_albedo=GROUND, out_gas=1))[L3["seg_alt_layer"]]
    # the steps' rows are fl(thermal + order one + diffuse part), the accumulate's one rounding: eps of the sum on top of 2 b
    total = _np(got[1][1]).astype(LD)
    b = 2 * R.bound(rows, 2, N_LEVELS) + LD(EPS) * np.abs(total)
    worst = float(np.max(np.abs(total - (_np(single[1][1]).astype(LD) + rows.astype(LD))) / b))
    print("\nscene, one SZA: |steps' rows - (thermal + order one + diffuse_source gathered)| / (2 b + eps |rows|) %.3f" % worst)
    assert rows.min() > 0 and worst <= 1.0


def test_scene_radiances(eng):
    import torch
    scene = _scene(eng, multiple=True)
    L3 = _batch(scene)
    ch4, haze = scene.gases
    los = eng.LimbLOS(L3["seg_off"], L3["seg_layer"], L3["pt_off"], L3["x"], L3["nd"], L3["vmr"], col_scale=[ch4.iso_ratio, 1.0])
    lit = eng.limb_rays(scene.sunlit_steps(L3), los).clone()
    rows = torch.as_tensor(L3["seg_alt_layer"].astype(np.int64), device="cuda")
    dark_pairs = [(p[0][rows].contiguous(), p[1][rows].contiguous()) for p in (ch4.coeffs, haze.thermal)]
    dark = eng.limb_rays(dark_pairs, los)
    assert bool(torch.isfinite(lit).all()) and bool((lit >= dark).all()) and bool((lit > dark).any())
