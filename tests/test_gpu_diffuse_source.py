"""The two-stream diffuse source on the GPU (engine.diffuse_source, sr_diffuse_source_rows_dev) against the extended-
precision reference of tests/diffuse_source_reference.py: the bound panel, signs, exact zeros, repeatability, accumulate,
conservation on the device's fluxes, the composed torch route and every refusal class."""
import ctypes as C

import numpy as np
import pytest

import diffuse_source_reference as R

pytestmark = pytest.mark.gpu
LD, EPS = R.LD, R.EPS53
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


def _call(eng, c, **kw):
    kw.setdefault("out_gas", c["out_gas"])
    kw.setdefault("surface_albedo", c["albedo"])
    return eng.diffuse_source(_dev(c["A"]), c["V"], c["ssa"], c["asym"], _dev(c["beam"]), _dev(c["sun"]), c["mu0"], **kw)


def _with_reference(c):
    ref = R.reference(*R.args(c))
    n_gas, n_layers = c["A"].shape[:2]
    c = dict(c, **{"ref_" + k: ref[k] for k in KEYS}, **{"b_" + k: R.bound(ref[k], n_gas, n_layers) for k in KEYS})
    for v in c.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return c


def _case(n_layers, n_gas, n_pts):
    """A panel case with its reference, made once and shared (read-only)."""
    key = (n_layers, n_gas, n_pts)
    if key not in _case.cache:
        _case.cache[key] = _with_reference(R.panel_case(*key))
    return _case.cache[key]


_case.cache = {}


@pytest.mark.parametrize("n_layers", R.N_LAYERS)
def test_panel_inside_the_bound(eng, n_layers):
    worst = dict.fromkeys(KEYS, 0.0)
    for n_gas in R.N_GAS:
        for n_pts in R.N_PTS:
            c = _case(n_layers, n_gas, n_pts)
            got = dict(zip(KEYS, _call(eng, c, mean_intensity=True, fluxes=True)))
            for k in KEYS:
                g = _np(got[k])
                assert np.all(np.isfinite(g)) and np.all(g >= 0), (k, n_gas, n_pts)
                worst[k] = max(worst[k], R.ratio(g, c["ref_" + k], c["b_" + k]))
            # the other instances give the same bits
            assert np.array_equal(_np(_call(eng, c)), _np(got["emi"]))
            e2, j2 = _call(eng, c, mean_intensity=True)
            assert np.array_equal(_np(e2), _np(got["emi"])) and np.array_equal(_np(j2), _np(got["J"]))
            j3, f3 = _call(eng, c, out_gas=None, mean_intensity=True, fluxes=True)
            assert np.array_equal(_np(j3), _np(got["J"])) and np.array_equal(_np(f3), _np(got["flux"]))
    print("\ndiffuse source panel, n_layers %d: |GPU - reference| / b %s" % (n_layers, worst))
    assert max(worst.values()) <= 1.0, worst


def test_exact_zeros_and_untouched_bits(eng):
    import torch
    c = _case(17, 3, 65)
    zero = np.zeros(3)
    # no scatterer, a black lower boundary: no diffuse light at all
    e, J, F = _call(eng, dict(c, ssa=zero), surface_albedo=0.0, mean_intensity=True, fluxes=True)
    assert not _np(e).any() and not _np(J).any() and not _np(F).any()
    # no scatterer above a reflecting ground: light, but no rows -- and under accumulate the rows keep their bits
    e, F = _call(eng, dict(c, ssa=zero, mu0=0.8), surface_albedo=0.6, fluxes=True)
    assert not _np(e).any() and np.all(_np(F)[0] > 0)
    base = torch.as_tensor(np.random.default_rng(3).uniform(-1.0, 1.0, (17, 65)), device="cuda")
    keep = _np(base).copy()
    _call(eng, dict(c, ssa=zero, mu0=0.8), surface_albedo=0.6, out=base, accumulate=True)
    assert np.array_equal(_np(base).view(np.uint64), keep.view(np.uint64))
    # no sunlight on any row and a black boundary
    e, J, F = _call(eng, dict(c, beam=np.zeros_like(c["beam"])), surface_albedo=0.0, mean_intensity=True, fluxes=True)
    assert not _np(e).any() and not _np(J).any() and not _np(F).any()


def test_two_calls_give_the_same_bits_and_accumulate_adds(eng):
    import torch
    c = _case(80, 3, 257)
    a, b = _call(eng, c, mean_intensity=True, fluxes=True), _call(eng, c, mean_intensity=True, fluxes=True)
    for x, y in zip(a, b):
        assert np.array_equal(_np(x).view(np.uint64), _np(y).view(np.uint64))
    base = np.random.default_rng(5).uniform(0.0, 2.0, (80, 257)) * float(_np(a[0]).max())
    acc = _dev(base)
    _call(eng, c, out=acc, accumulate=True)
    assert np.array_equal(_np(acc), base + _np(a[0]))                # overwrite plus base, one rounding


def test_a_call_in_point_chunks_gives_the_bits_of_its_parts(eng):
    """4096 layers x 2304 points need 288 MiB of workspace: above 256 MiB the entry launches point chunks (here 2048 and
    256 points) on one workspace.  The points are independent, so each part called alone gives the same bits."""
    import torch
    rng = np.random.default_rng(17)
    N, n_pts = 4096, 2304
    A = torch.as_tensor(rng.uniform(0.5, 1.5, (1, N, n_pts)), device="cuda")
    beam = torch.as_tensor(np.exp(-np.linspace(3.0, 0.0, N + 1))[:, None] * rng.uniform(0.9, 1.0, (N + 1, n_pts)), device="cuda")
    sun = torch.as_tensor(rng.uniform(5.0, 20.0, n_pts), device="cuda")
    V = np.full((1, N), 2.0 / N)
    call = lambda sl: eng.diffuse_source(A[:, :, sl].contiguous(), V, [0.95], [0.6], beam[:, sl].contiguous(), sun[sl].contiguous(), 0.7,
                                         surface_albedo=0.4, out_gas=0, fluxes=True)
    e, F = call(slice(0, n_pts))
    assert bool(torch.isfinite(e).all()) and float(e.min()) > 0.0
    for sl in (slice(0, 2048), slice(2048, n_pts)):
        e1, F1 = call(sl)
        assert torch.equal(e1, e[:, sl]) and torch.equal(F1, F[:, :, sl])


@pytest.mark.parametrize("n_layers", [1, 17, 80])
def test_conservation_on_the_device(eng, n_layers):
    c = R.conservation_case(n_layers, 65)
    want = R.absorbed_input(c)
    F = _np(_call(eng, c, out_gas=None, fluxes=True))
    out = F[0, -1].astype(LD) + F[1, 0].astype(LD)
    worst = float(np.max(np.abs(out - want) / R.bound(want, 1, n_layers)))
    print("\nconservation, n_layers %d: |F+_N + F-_0 - input| / b %.3f" % (n_layers, worst))
    assert worst <= 1.0


def _torch_layer(torch, sp, al, sg, D, mu0):
    """R.layer_operators in torch, term by term."""
    r3 = 1.7320508075688772
    dtau = sp + al
    live = dtau > 0
    one = torch.ones_like(dtau)
    safe = torch.where(live, dtau, one)
    co = torch.clamp(torch.where(live, al, one) / safe, min=2.0 ** -52)
    om = 1.0 - co
    g = torch.where(sp > 0, sg / torch.where(sp > 0, sp, one), torch.zeros_like(sp))
    d, s = r3 * co, r3 * (1.0 - om * g)
    sd, ss = torch.sqrt(d), torch.sqrt(s)
    k, g1 = sd * ss, 0.5 * (s + d)
    g2 = 0.5 * (r3 * om * (1.0 - g))
    rg = 1.0 / (g1 + k)
    Gm, u = g2 * rg, sd * (sd + ss) * rg
    x = k * dtau
    e, m = torch.exp(-x), -torch.expm1(-x)
    ge = 1.0 + Gm * e
    rden = 1.0 / ((u + Gm * m) * ge)
    Rr, T = Gm * m * (1.0 + e) * rden, e * u * (1.0 + Gm) * rden
    oneR, absb, oneT = u * (1.0 + Gm * e * e) * rden, m * u * (1.0 - Gm * e) * rden, m * (u + Gm * ge) * rden
    src = om * D
    es = src * (sd + ss) * rg * (m / sd) / ge
    ed = -(src * (r3 * g * mu0)) / s * (oneT + Rr)
    pick = lambda v, idle: torch.where(live, v, torch.full_like(v, idle))
    return pick(Rr, 0.0), pick(T, 1.0), pick(0.5 * (es + ed), 0.0), pick(0.5 * (es - ed), 0.0), pick(oneR, 1.0), pick(absb, 0.0), live


def _composed(torch, c):
    """The same formulas composed from torch operators on the device: (emi, J, F)."""
    A, beam, sun = _dev(c["A"]), _dev(c["beam"]), _dev(c["sun"])
    V, ssa, asym = (np.asarray(c[k], float) for k in ("V", "ssa", "asym"))
    f = np.maximum(asym, 0.0) ** 2
    cs, ca, cg = ssa * (1.0 - f), 1.0 - ssa, ssa * (asym - f)
    n_gas, N, n_pts = A.shape
    sp, al, sg = (torch.zeros((N, n_pts), dtype=torch.float64, device="cuda") for _ in range(3))
    for g in range(n_gas):
        t = _dev(V[g])[:, None] * A[g]
        sp, al, sg = sp + cs[g] * t, al + ca[g] * t, sg + cg[g] * t
    alb, mu0 = c["albedo"], c["mu0"]
    Rb, Cb = torch.full_like(sun, alb), torch.full_like(sun, 1.0 - alb)
    Ub = alb * (max(mu0, 0.0) * (sun * beam[N]))
    keep = []
    for l in range(N):
        Rr, T, Ep, Em, oneR, absb, live = _torch_layer(torch, sp[l], al[l], sg[l], sun * beam[l], mu0)
        q = torch.where(live, 1.0 / (Cb + Rb * oneR), torch.ones_like(Cb))
        keep.append((T * q, (Em + Rr * Ub) * q, Rb, Ub))
        Ub, Cb, Rb = Ep + T * (Ub + Rb * Em) * q, (oneR * Cb + Rb * absb * (oneR + T)) * q, Rr + T * T * Rb * q
    F = torch.zeros((2, N + 1, n_pts), dtype=torch.float64, device="cuda")
    J = torch.zeros((N, n_pts), dtype=torch.float64, device="cuda")
    F[0, N] = Ub
    kJ = 1.7320508075688772 / (8.0 * 3.141592653589793)
    for l in range(N - 1, -1, -1):
        tq, cq, rb, ub = keep[l]
        F[1, l] = tq * F[1, l + 1] + cq
        F[0, l] = ub + rb * F[1, l]
        J[l] = kJ * ((F[0, l] + F[1, l]) + (F[0, l + 1] + F[1, l + 1]))
    G = c["out_gas"]
    return (cs[G] * A[G]) * J, J, F


def test_composed_torch_route_agrees(eng):
    import torch
    worst = 0.0
    for key in ((17, 3, 257), (3, 8, 65), (2, 1, 63)):
        c = _case(*key)
        fused = _call(eng, c, mean_intensity=True, fluxes=True)
        for k, a, b in zip(KEYS, fused, _composed(torch, c)):
            worst = max(worst, R.ratio(_np(a) - _np(b), np.zeros(a.shape, LD), 2 * c["b_" + k]))
    print("\nfused against composed: |difference| / 2 b %.3f" % worst)
    assert worst <= 1.0


def test_every_refusal_leaves_the_outputs_untouched(eng):
    import torch
    from spectrobot_amd import _lib
    lib, dp = _lib.lib, _lib.dp
    c = _case(17, 3, 65)
    n_layers, n_gas, n_pts = 17, 3, 65
    A, beam, sun = _dev(c["A"]), _dev(c["beam"]), _dev(c["sun"])
    shapes = ((n_layers, n_pts), (n_layers, n_pts), (2, n_layers + 1, n_pts))
    bufs = [torch.full(s, -7.0, dtype=torch.float64, device="cuda") for s in shapes]
    V, ssa, asym = np.array(c["V"]), np.array(c["ssa"]), np.array(c["asym"])
    good = dict(v=V, ssa=ssa, asym=asym, n_gas=n_gas, n_layers=n_layers, mu0=c["mu0"], alb=c["albedo"], A=A, beam=beam, sun=sun,
                n_pts=n_pts, G=0, acc=0, e=bufs[0], j=bufs[1], f=bufs[2], desc=True)
    ptr = lambda t: None if t is None else C.c_void_p(t.data_ptr())
    hp = lambda a: None if a is None else a.ctypes.data_as(dp)

    def call(**kw):
        a = dict(good, **kw)
        d = _lib.DiffuseDesc()
        d.n_gas, d.n_layers, d.v, d.ssa, d.asym = a["n_gas"], a["n_layers"], hp(a["v"]), hp(a["ssa"]), hp(a["asym"])
        d.mu0, d.surface_albedo = a["mu0"], a["alb"]
        return lib.sr_diffuse_source_rows_dev(C.byref(d) if a["desc"] else None, ptr(a["A"]), ptr(a["beam"]), ptr(a["sun"]),
                                              a["n_pts"], a["G"], a["acc"], ptr(a["e"]), ptr(a["j"]), ptr(a["f"]), None)

    def edited(arr, at, v):
        out = arr.copy()
        out[at] = v
        return out

    ARG, LIMIT = _lib.SR_ERR_ARG, _lib.SR_ERR_LIMIT
    nan, inf = np.nan, np.inf
    cases = [("null desc", dict(desc=False), ARG), ("null v", dict(v=None), ARG), ("null ssa", dict(ssa=None), ARG),
             ("null asym", dict(asym=None), ARG), ("null tab_abs", dict(A=None), ARG), ("null beam", dict(beam=None), ARG),
             ("null sun", dict(sun=None), ARG), ("n_gas 0", dict(n_gas=0), ARG), ("n_layers 0", dict(n_layers=0), ARG),
             ("n_pts 0", dict(n_pts=0), ARG),
             ("v negative", dict(v=edited(V, (2, 16), -1e-30)), ARG), ("v nan", dict(v=edited(V, (0, 0), nan)), ARG),
             ("v inf", dict(v=edited(V, (1, 3), inf)), ARG),
             ("ssa negative", dict(ssa=edited(ssa, 0, -0.1)), ARG), ("ssa above 1", dict(ssa=edited(ssa, 2, 1.0 + 2.0 ** -52)), ARG),
             ("ssa nan", dict(ssa=edited(ssa, 1, nan)), ARG),
             ("asym below -0.5", dict(asym=edited(asym, 0, -0.5000001)), ARG), ("asym 1", dict(asym=edited(asym, 2, 1.0)), ARG),
             ("asym nan", dict(asym=edited(asym, 1, nan)), ARG),
             ("mu0 above 1", dict(mu0=1.0000001), ARG), ("mu0 below -1", dict(mu0=-1.5), ARG), ("mu0 nan", dict(mu0=nan), ARG),
             ("albedo negative", dict(alb=-0.01), ARG), ("albedo above 1", dict(alb=1.01), ARG), ("albedo inf", dict(alb=inf), ARG),
             ("out_gas too large", dict(G=n_gas), ARG), ("out_gas below -1", dict(G=-2), ARG),
             ("emi_out without out_gas", dict(G=-1), ARG), ("out_gas without emi_out", dict(e=None), ARG),
             ("no output", dict(G=-1, e=None, j=None, f=None), ARG),
             ("n_gas beyond the limit", dict(n_gas=9), LIMIT), ("n_layers beyond the limit", dict(n_layers=_lib.SR_MAX_ABS_ROWS + 1), LIMIT),
             ("n_pts beyond the limit", dict(n_pts=2000001), LIMIT)]
    for what, kw, status in cases:
        assert call(**kw) == status, what
    torch.cuda.synchronize()
    assert all(bool((b == -7.0).all()) for b in bufs)
    # a valid call afterwards gives the reference's numbers
    assert call() == 0
    torch.cuda.synchronize()
    for k, b in zip(KEYS, bufs):
        assert R.ratio(_np(b), c["ref_" + k], c["b_" + k]) <= 1.0
    # the host layer's own refusals
    with pytest.raises(ValueError):
        eng.diffuse_source(A, V, ssa, asym, beam, sun, 0.5, out_gas=0, accumulate=True)
    with pytest.raises(ValueError):
        eng.diffuse_source(A, V[:, :-1], ssa, asym, beam, sun, 0.5, out_gas=0)
    with pytest.raises(ValueError):
        eng.diffuse_source(A, V, ssa, asym, beam[:-1].contiguous(), sun, 0.5, out_gas=0)
    with pytest.raises(ValueError):
        eng.diffuse_source(A, V, ssa, asym, beam, sun, 0.5)
