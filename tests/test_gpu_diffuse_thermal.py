"""Thermal emission as a source of the two-stream diffuse field on the GPU (engine.diffuse_thermal_source,
sr_diffuse_thermal_rows_dev) against the extended-precision reference of tests/diffuse_thermal_reference.py: the bound
panel (thermal alone and with the sun, own_emission off and on), exact zeros, repeatability, accumulate, point chunks,
superposition on the device, the own rows of a pure absorber against AbsorberTable.layers, and every refusal class."""
import ctypes as C

import numpy as np
import pytest

import absorber_table_reference as AR
import diffuse_source_reference as R
import diffuse_thermal_reference as T

pytestmark = pytest.mark.gpu
LD = T.LD
KEYS = ("emi", "J", "flux")


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


def _grid(c):
    return c["w0"] + np.arange(c["g_lo"] + c["A"].shape[2]) * c["step"]


def _call(eng, c, solar, **kw):
    kw.setdefault("out_gas", c["out_gas"])
    kw.setdefault("surface_albedo", c["albedo"])
    kw.setdefault("t_surface", c["t_surface"])
    if solar:
        kw.update(beam=_dev(c["beam"]), sun=_dev(c["sun"]), mu0=c["mu0"])
    return eng.diffuse_thermal_source(_dev(c["A"]), c["V"], c["ssa"], c["asym"], c["temps"], _grid(c), g_lo=c["g_lo"], **kw)


def _case(n_layers, n_gas, n_pts):
    """A panel case with its references (thermal alone / with the sun, own_emission off / on), made once and shared."""
    key = (n_layers, n_gas, n_pts)
    if key not in _case.cache:
        c = T.panel_case(*key)
        xm = T.x_max(c)
        for solar in (False, True):
            for own in (False, True):
                ref = T.reference(c, solar, own)
                c["ref", solar, own] = ref
                c["b", solar, own] = {k: T.bound(ref[k], n_gas, n_layers, xm) for k in KEYS}
        for v in c.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        _case.cache[key] = c
    return _case.cache[key]


_case.cache = {}


@pytest.mark.parametrize("n_layers", T.N_LAYERS)
def test_panel_inside_the_bound(eng, n_layers):
    worst = dict.fromkeys(KEYS, 0.0)
    for n_gas in T.N_GAS:
        for n_pts in T.N_PTS:
            c = _case(n_layers, n_gas, n_pts)
            for solar in (False, True):
                for own in (False, True):
                    got = dict(zip(KEYS, _call(eng, c, solar, own_emission=own, mean_intensity=True, fluxes=True)))
                    for k in KEYS:
                        g = _np(got[k])
                        assert np.all(np.isfinite(g)) and np.all(g >= 0), (k, n_gas, n_pts, solar, own)
                        worst[k] = max(worst[k], T.ratio(g, c["ref", solar, own][k], c["b", solar, own][k]))
                # the other instances give the same bits (own_emission on)
                assert np.array_equal(_np(_call(eng, c, solar, own_emission=True)), _np(got["emi"]))
                e2, j2 = _call(eng, c, solar, own_emission=True, mean_intensity=True)
                assert np.array_equal(_np(e2), _np(got["emi"])) and np.array_equal(_np(j2), _np(got["J"]))
                j3, f3 = _call(eng, c, solar, out_gas=None, mean_intensity=True, fluxes=True)
                assert np.array_equal(_np(j3), _np(got["J"])) and np.array_equal(_np(f3), _np(got["flux"]))
    print("\ndiffuse thermal panel, n_layers %d: |GPU - reference| / b %s" % (n_layers, worst))
    assert max(worst.values()) <= 1.0, worst


def test_exact_zeros_and_untouched_bits(eng):
    import torch
    c = _case(17, 3, 65)
    # a row with ssa_G = 0, own_emission off: no rows -- and under accumulate the rows keep their bits
    zero = np.zeros(3)
    e, F = _call(eng, dict(c, ssa=zero), False, fluxes=True)
    assert not _np(e).any() and np.all(_np(F)[0, -1] > 0)
    base = torch.as_tensor(np.random.default_rng(3).uniform(-1.0, 1.0, (17, 65)), device="cuda")
    keep = _np(base).copy()
    _call(eng, dict(c, ssa=zero), False, out=base, accumulate=True)
    assert np.array_equal(_np(base).view(np.uint64), keep.view(np.uint64))
    # at night, a point where no layer has an absorber (gas 0 scatters alone there) and no surface emits: exact zeros
    # there, light at its neighbours
    A = np.array(c["A"])
    A[1:, :, 7] = 0.0
    V = np.maximum(np.array(c["V"]), 1e-4)
    e, J, F = _call(eng, dict(c, A=A, V=V, ssa=np.array([1.0, 0.2, 0.0])), False, own_emission=True, t_surface=0.0, mean_intensity=True,
                    fluxes=True)
    for t in (e, J, F[0]):                 # (F-[top] is 0 everywhere: F+ alone is looked at for light)
        a = _np(t)
        assert not a[..., 7].any() and np.all(np.delete(a, 7, axis=-1)[-1] > 0)
    assert not _np(F)[1, :, 7].any()
    # ... and every output is an exact 0 with every ssa = 1, no sun, no emitting surface
    e, J, F = _call(eng, dict(c, ssa=np.ones(3)), False, own_emission=True, t_surface=0.0, mean_intensity=True, fluxes=True)
    assert not _np(e).any() and not _np(J).any() and not _np(F).any()


def test_two_calls_give_the_same_bits_and_accumulate_adds(eng):
    c = _case(80, 3, 257)
    for solar in (False, True):
        kw = dict(own_emission=True, mean_intensity=True, fluxes=True)
        a, b = _call(eng, c, solar, **kw), _call(eng, c, solar, **kw)
        for x, y in zip(a, b):
            assert np.array_equal(_np(x).view(np.uint64), _np(y).view(np.uint64))
        base = np.random.default_rng(5).uniform(0.0, 2.0, (80, 257)) * float(_np(a[0]).max())
        acc = _dev(base)
        _call(eng, c, solar, out=acc, accumulate=True, own_emission=True)
        assert np.array_equal(_np(acc), base + _np(a[0]))                # overwrite plus base, one rounding


def test_a_call_in_point_chunks_gives_the_bits_of_its_parts(eng):
    """4096 layers x 2304 points need 288 MiB of workspace: above 256 MiB the entry launches point chunks (here 2048 and
    256 points) on one workspace.  The points are independent, so each part called alone -- with its own g_lo -- gives the
    same bits."""
    import torch
    rng = np.random.default_rng(17)
    N, n_pts = 4096, 2304
    A = torch.as_tensor(rng.uniform(0.5, 1.5, (2, N, n_pts)), device="cuda")
    V = np.stack([np.full(N, 2.0 / N), np.full(N, 0.2 / N)])
    temps = rng.uniform(90.0, 180.0, N)
    grid = 1200.0 + np.arange(n_pts + 11) * 0.25
    call = lambda sl: eng.diffuse_thermal_source(A[:, :, sl].contiguous(), V, [0.95, 0.0], [0.6, 0.0], temps, grid, t_surface=120.0,
                                                 surface_albedo=0.4, out_gas=0, own_emission=True, fluxes=True, g_lo=11 + sl.start)
    e, F = call(slice(0, n_pts))
    assert bool(torch.isfinite(e).all()) and float(e.min()) > 0.0
    for sl in (slice(0, 2048), slice(2048, n_pts)):
        e1, F1 = call(sl)
        assert torch.equal(e1, e[:, sl]) and torch.equal(F1, F[:, :, sl])


def test_superposition_on_the_device(eng):
    """The call with both sources against diffuse_source's J plus the night call's J, within the sum of their bounds."""
    worst = 0.0
    for key in ((17, 3, 257), (3, 8, 65), (80, 1, 63)):
        c = _case(*key)
        n_layers, n_gas = key[0], key[1]
        J_both = _np(_call(eng, c, True, out_gas=None, mean_intensity=True))
        J_night = _np(_call(eng, c, False, out_gas=None, mean_intensity=True))
        J_sun = _np(eng.diffuse_source(_dev(c["A"]), c["V"], c["ssa"], c["asym"], _dev(c["beam"]), _dev(c["sun"]), c["mu0"],
                                       surface_albedo=c["albedo"], mean_intensity=True))
        b = (c["b", True, False]["J"] + c["b", False, False]["J"] + R.bound(R.reference(*R.args(c))["J"], n_gas, n_layers))
        worst = max(worst, T.ratio(J_both - (J_sun + J_night), np.zeros(J_both.shape, LD), b))
    print("\nboth sources against the sun's plus the night's: |difference| / sum of bounds %.3f" % worst)
    assert worst <= 1.0


@pytest.mark.parametrize("key", [(2, 1, 63), (17, 3, 257)])
def test_a_thermal_source_of_zero_gives_the_bits_of_diffuse_source(eng, key):
    """Every ssa = 1 (alpha exactly 0 in every layer), no emitting surface, own_emission off, the sun on: the thermal
    source is an exact 0, x + 0.0 keeps x and E+- is never -0 (E+ + E- >= +0), so the instance with both sources gives
    the bits of the sun's alone.  Exact by construction: the two are instances of one kernel text."""
    import torch
    c = dict(T.panel_case(*key), ssa=np.ones(key[1]))
    both = _call(eng, c, True, t_surface=0.0, own_emission=False, mean_intensity=True, fluxes=True)
    sun = eng.diffuse_source(_dev(c["A"]), c["V"], c["ssa"], c["asym"], _dev(c["beam"]), _dev(c["sun"]), c["mu0"],
                             surface_albedo=c["albedo"], out_gas=c["out_gas"], mean_intensity=True, fluxes=True)
    assert bool((sun[1] > 0).any())
    for k, b, s in zip(KEYS, both, sun):
        assert torch.equal(b, s), k


def test_own_rows_of_an_absorber_are_the_table_emission(eng):
    """ssa = 0: the own_emission rows are A B, what AbsorberTable.layers gives as emi for the same table and temperatures --
    within twice the absorber-table reference's allowance for the emission (the two kernels restate one Planck
    evaluation, so the bits are expected to agree)."""
    w0, step, n = AR.GRID
    grid = w0 + np.arange(n) * step
    sets = [(s[0], s[1], s[2], np.abs(s[3]) + 1e-21) for s in AR.panel_sets(0)[:2]]
    tab = eng.AbsorberTable(sets)
    temps = AR.ROW_TEMPS
    ab, em = tab.layers(temps, grid)
    set2, w2, dw2 = tab.plan(temps)
    ref = AR.evaluate(sets, set2, w2, dw2, temps, None, w0, step, 0, n)
    rows = eng.diffuse_thermal_source(ab[None].contiguous(), np.ones((1, temps.size)), [0.0], [0.0], temps, grid, out_gas=0,
                                      own_emission=True)
    diff = np.abs(_np(rows).astype(LD) - _np(em).astype(LD))
    worst = float(np.max(diff / (2 * ref["b_emi"])))
    print("\nown rows of an absorber against AbsorberTable.layers: |difference| / (2 b_emi) %.3f, equal bits: %s"
          % (worst, bool(np.array_equal(_np(rows), _np(em)))))
    assert np.all(_np(em) > 0) and worst <= 1.0


def test_every_refusal_leaves_the_outputs_untouched(eng):
    import torch
    from spectrobot_amd import _lib
    lib, dp = _lib.lib, _lib.dp
    c = _case(17, 3, 65)
    n_layers, n_gas, n_pts = 17, 3, 65
    A, beam, sun = _dev(c["A"]), _dev(c["beam"]), _dev(c["sun"])
    shapes = ((n_layers, n_pts), (n_layers, n_pts), (2, n_layers + 1, n_pts))
    bufs = [torch.full(s, -7.0, dtype=torch.float64, device="cuda") for s in shapes]
    V, ssa, asym, temps = np.array(c["V"]), np.array(c["ssa"]), np.array(c["asym"]), np.array(c["temps"])
    good = dict(v=V, ssa=ssa, asym=asym, n_gas=n_gas, n_layers=n_layers, mu0=c["mu0"], alb=c["albedo"], A=A, beam=beam, sun=sun,
                n_pts=n_pts, G=0, acc=0, e=bufs[0], j=bufs[1], f=bufs[2], desc=True, th=True, temps=temps, ts=c["t_surface"],
                w0=c["w0"], step=c["step"], g_lo=c["g_lo"], own=1)
    ptr = lambda t: None if t is None else C.c_void_p(t.data_ptr())
    hp = lambda a: None if a is None else a.ctypes.data_as(dp)

    def call(**kw):
        a = dict(good, **kw)
        d, th = _lib.DiffuseDesc(), _lib.DiffuseThermalDesc()
        d.n_gas, d.n_layers, d.v, d.ssa, d.asym = a["n_gas"], a["n_layers"], hp(a["v"]), hp(a["ssa"]), hp(a["asym"])
        d.mu0, d.surface_albedo = a["mu0"], a["alb"]
        th.temps, th.t_surface, th.w0, th.step, th.g_lo, th.own_emission = hp(a["temps"]), a["ts"], a["w0"], a["step"], a["g_lo"], a["own"]
        return lib.sr_diffuse_thermal_rows_dev(C.byref(d) if a["desc"] else None, C.byref(th) if a["th"] else None, ptr(a["A"]),
                                               ptr(a["beam"]), ptr(a["sun"]), a["n_pts"], a["G"], a["acc"], ptr(a["e"]), ptr(a["j"]),
                                               ptr(a["f"]), None)

    def edited(arr, at, v):
        out = arr.copy()
        out[at] = v
        return out

    ARG, LIMIT = _lib.SR_ERR_ARG, _lib.SR_ERR_LIMIT
    nan, inf = np.nan, np.inf
    cases = [("null desc", dict(desc=False), ARG), ("null v", dict(v=None), ARG), ("null ssa", dict(ssa=None), ARG),
             ("null asym", dict(asym=None), ARG), ("null tab_abs", dict(A=None), ARG),
             ("n_gas 0", dict(n_gas=0), ARG), ("n_layers 0", dict(n_layers=0), ARG), ("n_pts 0", dict(n_pts=0), ARG),
             ("v negative", dict(v=edited(V, (2, 16), -1e-30)), ARG), ("v nan", dict(v=edited(V, (0, 0), nan)), ARG),
             ("v inf", dict(v=edited(V, (1, 3), inf)), ARG),
             ("ssa negative", dict(ssa=edited(ssa, 0, -0.1)), ARG), ("ssa above 1", dict(ssa=edited(ssa, 2, 1.0 + 2.0 ** -52)), ARG),
             ("ssa nan", dict(ssa=edited(ssa, 1, nan)), ARG),
             ("asym below -0.5", dict(asym=edited(asym, 0, -0.5000001)), ARG), ("asym 1", dict(asym=edited(asym, 2, 1.0)), ARG),
             ("asym nan", dict(asym=edited(asym, 1, nan)), ARG),
             ("mu0 above 1", dict(mu0=1.0000001), ARG), ("mu0 below -1", dict(mu0=-1.5), ARG), ("mu0 nan", dict(mu0=nan), ARG),
             ("albedo negative", dict(alb=-0.01), ARG), ("albedo above 1", dict(alb=1.01), ARG), ("albedo inf", dict(alb=inf), ARG),
             ("out_gas too large", dict(G=n_gas), ARG), ("out_gas below -1", dict(G=-2), ARG),
             ("emi_out without out_gas", dict(G=-1, own=0), ARG), ("out_gas without emi_out", dict(e=None, own=0), ARG),
             ("no output", dict(G=-1, e=None, j=None, f=None, own=0), ARG),
             ("n_gas beyond the limit", dict(n_gas=9), LIMIT), ("n_layers beyond the limit", dict(n_layers=_lib.SR_MAX_ABS_ROWS + 1), LIMIT),
             ("n_pts beyond the limit", dict(n_pts=2000001), LIMIT),
             # the thermal call's own
             ("null th", dict(th=False), ARG), ("null temps", dict(temps=None), ARG),
             ("temperature 0", dict(temps=edited(temps, 3, 0.0)), ARG), ("temperature negative", dict(temps=edited(temps, 0, -90.0)), ARG),
             ("temperature nan", dict(temps=edited(temps, 16, nan)), ARG), ("temperature inf", dict(temps=edited(temps, 5, inf)), ARG),
             ("t_surface negative", dict(ts=-1.0), ARG), ("t_surface nan", dict(ts=nan), ARG), ("t_surface inf", dict(ts=inf), ARG),
             ("w0 nan", dict(w0=nan), ARG), ("w0 inf", dict(w0=inf), ARG), ("step nan", dict(step=nan), ARG), ("step inf", dict(step=-inf), ARG),
             ("g_lo negative", dict(g_lo=-1), ARG),
             ("beam without sun", dict(sun=None), ARG), ("sun without beam", dict(beam=None), ARG),
             ("own_emission without emi_out", dict(G=-1, e=None), ARG),
             ("g_lo + n_pts beyond int32", dict(g_lo=2 ** 31 - n_pts), LIMIT)]
    for what, kw, status in cases:
        assert call(**kw) == status, what
    torch.cuda.synchronize()
    assert all(bool((b == -7.0).all()) for b in bufs)
    # mu0 is not read at night: a value out of range passes, and the valid calls give the reference's numbers
    for solar, kw in ((True, {}), (False, dict(beam=None, sun=None, mu0=nan))):
        assert call(**kw) == 0
        torch.cuda.synchronize()
        for k, b in zip(KEYS, bufs):
            assert T.ratio(_np(b), c["ref", solar, True][k], c["b", solar, True][k]) <= 1.0
    assert call(g_lo=2 ** 31 - 1 - n_pts, j=None, f=None) == 0        # the last grid a call takes
    torch.cuda.synchronize()
    # the host layer's own refusals
    grid = _grid(c)
    kw = dict(g_lo=c["g_lo"])
    with pytest.raises(ValueError):
        eng.diffuse_thermal_source(A, V, ssa, asym, temps, grid, out_gas=0, accumulate=True, **kw)
    with pytest.raises(ValueError):
        eng.diffuse_thermal_source(A, V[:, :-1], ssa, asym, temps, grid, out_gas=0, **kw)
    with pytest.raises(ValueError):
        eng.diffuse_thermal_source(A, V, ssa, asym, temps[:-1], grid, out_gas=0, **kw)
    with pytest.raises(ValueError):
        eng.diffuse_thermal_source(A, V, ssa, asym, temps, grid, beam=beam, out_gas=0, **kw)
    with pytest.raises(ValueError):
        eng.diffuse_thermal_source(A, V, ssa, asym, temps, grid, beam=beam[:-1].contiguous(), sun=sun, mu0=0.5, out_gas=0, **kw)
    with pytest.raises(ValueError):
        eng.diffuse_thermal_source(A, V, ssa, asym, temps, grid, **kw)
    with pytest.raises(ValueError):
        eng.diffuse_thermal_source(A, V, ssa, asym, temps, grid, own_emission=True, mean_intensity=True, **kw)
    with pytest.raises(ValueError):
        eng.diffuse_thermal_source(A, V, ssa, asym, temps, grid, out_gas=0, g_lo=c["g_lo"] + 1)
