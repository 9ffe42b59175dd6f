"""The diffuse rows in the Jacobians on the GPU (engine.diffuse_jacobian, sr_diffuse_jacobian_rows_dev) against the extended-
precision reference of tests/diffuse_jacobian_reference.py: the bound panel for jac and dJ, exact zeros, scaling,
repeatability, accumulate / par_slot, the torch contraction of dJ, a call across the workspace cap, central differences
of engine.diffuse_source on the device, and every refusal class."""
import ctypes as C

import numpy as np
import pytest

import diffuse_jacobian_reference as DJ
import diffuse_source_reference as R

pytestmark = pytest.mark.gpu
LD = R.LD


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
    return None if a is None else torch.as_tensor(np.array(a, dtype=np.float64), device="cuda")    # (a copy: the cases are read-only)


def _call(eng, c, **kw):
    kw.setdefault("surface_albedo", c["albedo"])
    return eng.diffuse_jacobian(_dev(c["A"]), c["V"], c["ssa"], c["asym"], _dev(c["beam"]), _dev(c["sun"]), c["mu0"], c["dV"],
                                _dev(c["dlnbeam"]), _dev(c["Q"]), **kw)


def _case(*key):
    """A panel case with its reference and bounds, made once and shared (read-only)."""
    if key not in _case.cache:
        c = DJ.panel_case(*key)
        ref = DJ.reference(c, yardstick=True)
        n_gas, n_layers = c["A"].shape[:2]
        c = dict(c, ref_dJ=ref["dJ"], ref_jac=ref["jac"], b_dJ=DJ.bound(ref["S_dJ"], n_gas, n_layers),
                 b_jac=DJ.bound(ref["S_jac"], n_gas, n_layers))
        for v in c.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        _case.cache[key] = c
    return _case.cache[key]


_case.cache = {}


@pytest.mark.parametrize("n_layers", R.N_LAYERS)
def test_panel_inside_the_bound(eng, n_layers):
    worst = dict(jac=0.0, dJ=0.0)
    for key in DJ.PANEL:
        if key[0] != n_layers:
            continue
        c = _case(*key)
        jac, dJ = _call(eng, c, tangent=True)
        for k, got in (("jac", jac), ("dJ", dJ)):
            r = R.ratio(_np(got), c["ref_" + k], c["b_" + k])
            print("\ndiffuse jacobian panel %s: |GPU - reference| / b, %s %.3f" % (key, k, r))
            worst[k] = max(worst[k], r)
        # the other instances give the same bits
        assert np.array_equal(_np(_call(eng, c)), _np(jac))
        assert np.array_equal(_np(_call(eng, dict(c, Q=None), tangent=True)), _np(dJ))
    print("diffuse jacobian panel, n_layers %d: worst %s" % (n_layers, worst))
    assert max(worst.values()) <= 1.0, worst


def test_physical_directions_inside_the_bound_by_parts(eng):
    """dlnbeam as the shadow of the parameter's own column (opposite in sign to its dV, what every scene call makes), against
    the yardstick whose addends are a source layer's two parts."""
    worst = dict(jac=0.0, dJ=0.0)
    for key in ((1, 3, 63, 2, 8), (3, 3, 65, 5, 8), (17, 8, 257, 9, 8), (80, 3, 65, 9, 9), (80, 8, 65, 5, 9)):
        c = DJ.physical_directions(DJ.panel_case(*key))
        ref = DJ.reference(c, yardstick="parts")
        jac, dJ = _call(eng, c, tangent=True)
        for k, got in (("jac", jac), ("dJ", dJ)):
            r = R.ratio(_np(got), ref[k], DJ.bound(ref["S_" + k], *c["A"].shape[:2]))
            print("\ndiffuse jacobian, physical directions %s: |GPU - reference| / b by parts, %s %.3f" % (key, k, r))
            worst[k] = max(worst[k], r)
    assert max(worst.values()) <= 1.0, worst


def test_exact_zeros(eng):
    c = _case(17, 3, 257, 5, 8)
    zero = lambda a: np.zeros_like(a)
    jac, dJ = _call(eng, dict(c, dV=zero(c["dV"]), dlnbeam=zero(c["dlnbeam"])), tangent=True)       # no direction
    assert not _np(jac).any() and not _np(dJ).any()
    jac, dJ = _call(eng, dict(c, dV=zero(c["dV"]), dlnbeam=None), tangent=True)                     # the beam held fixed
    assert not _np(jac).any() and not _np(dJ).any()
    jac, dJ = _call(eng, dict(c, Q=zero(c["Q"])), tangent=True)                                    # no ray sees J
    assert not _np(jac).any() and _np(dJ).any()
    jac, dJ = _call(eng, dict(c, sun=zero(c["sun"])), tangent=True)                                # shadow
    assert not _np(jac).any() and not _np(dJ).any()
    jac, dJ = _call(eng, dict(c, ssa=np.zeros(3)), surface_albedo=0.0, tangent=True)               # nothing scatters or reflects
    assert not _np(jac).any() and not _np(dJ).any()


def test_an_empty_layer_has_no_operator_tangent(eng):
    """dV on a layer with dtau == 0 is passed over: the bits of the call with that dV taken out."""
    c = _case(17, 3, 65, 5, 8)
    V = np.array(c["V"])
    V[:, 5] = 0.0
    dV = np.array(c["dV"])
    dV[:, :, 5] = 0.0
    dV2 = dV.copy()
    dV2[0, 1, 5], dV2[3, 0, 5] = 0.3, -2.0
    a = _call(eng, dict(c, V=V, dV=dV), tangent=True)
    b = _call(eng, dict(c, V=V, dV=dV2), tangent=True)
    for x, y in zip(a, b):
        assert np.array_equal(_np(x).view(np.uint64), _np(y).view(np.uint64))


def test_scaling_repeatability_accumulate_and_slots(eng):
    import torch
    c = _case(80, 3, 257, 2, 8)
    jac, dJ = _call(eng, c, tangent=True)
    jac2, dJ2 = _call(eng, dict(c, dV=2.0 * c["dV"], dlnbeam=2.0 * c["dlnbeam"]), tangent=True)      # a direction x 2: bits x 2
    assert np.array_equal(_np(jac2), 2.0 * _np(jac)) and np.array_equal(_np(dJ2), 2.0 * _np(dJ))
    again = _call(eng, c, tangent=True)                                                             # two calls: the same bits
    assert np.array_equal(_np(again[0]).view(np.uint64), _np(jac).view(np.uint64))
    assert np.array_equal(_np(again[1]).view(np.uint64), _np(dJ).view(np.uint64))
    n_rays, n_pts = jac.shape[0], jac.shape[2]
    base = np.random.default_rng(5).uniform(-1.0, 1.0, (n_rays, 5, n_pts)) * float(_np(jac).max())
    out = _dev(base)
    res = _call(eng, c, out=out, par_slot=[3, 1], accumulate=True)                                  # rows 3 and 1, added
    assert res is out
    got = _np(out)
    assert np.array_equal(got[:, 3], base[:, 3] + _np(jac)[:, 0]) and np.array_equal(got[:, 1], base[:, 1] + _np(jac)[:, 1])
    for row in (0, 2, 4):
        assert np.array_equal(got[:, row].view(np.uint64), base[:, row].view(np.uint64))            # unnamed rows keep their bits
    out = _dev(base)
    _call(eng, c, out=out, par_slot=[4, 0])                                                         # overwrite
    got = _np(out)
    assert np.array_equal(got[:, 4], _np(jac)[:, 0]) and np.array_equal(got[:, 0], _np(jac)[:, 1])
    for row in (1, 2, 3):
        assert np.array_equal(got[:, row].view(np.uint64), base[:, row].view(np.uint64))


def test_the_torch_contraction_of_the_tangent_agrees(eng):
    """dJ contracted with Q in torch against the fused jac, inside twice the bound: no shared error in the fused sum."""
    import torch
    worst = 0.0
    for key in ((17, 1, 65, 9, 9), (80, 8, 65, 5, 9), (3, 3, 65, 5, 8)):
        c = _case(*key)
        jac, dJ = _call(eng, c, tangent=True)
        composed = torch.einsum("rlj,plj->rpj", _dev(c["Q"]), dJ)
        worst = max(worst, R.ratio(_np(jac) - _np(composed), np.zeros(jac.shape, LD), 2 * c["b_jac"]))
    print("\nfused against composed: |difference| / 2 b %.3f" % worst)
    assert worst <= 1.0


def test_a_call_across_the_workspace_cap_gives_the_bits_of_its_parts(eng):
    """4096 layers need 23 x 8 x 4096 bytes of workspace per (parameter tile, point): 256 MiB hold 356 of them, so 512
    points x 5 parameters (two tiles) run as two point chunks of 256 x two tiles, on one workspace.  Points and parameters
    are independent, so each part called alone gives the same bits."""
    import torch
    rng = np.random.default_rng(19)
    N, n_pts, n_par, n_rays = 4096, 512, 5, 2
    A = torch.as_tensor(rng.uniform(0.5, 1.5, (1, N, n_pts)), device="cuda")
    beam = torch.as_tensor(np.exp(-np.linspace(3.0, 0.0, N + 1))[:, None] * rng.uniform(0.9, 1.0, (N + 1, n_pts)), device="cuda")
    sun = torch.as_tensor(rng.uniform(5.0, 20.0, n_pts), device="cuda")
    Q = torch.as_tensor(rng.uniform(0.1, 1.0, (n_rays, N, n_pts)), device="cuda")
    dlnb = torch.as_tensor(rng.uniform(-1.0, 1.0, (n_par, N + 1, n_pts)), device="cuda")
    V = np.full((1, N), 2.0 / N)
    dV = np.zeros((n_par, 1, N))
    for p in range(n_par):
        dV[p, 0, 700 * p + 5:700 * p + 8] = (0.5 / N, -1.0 / N, 0.5 / N) if p % 2 else (0.5 / N, 1.0 / N, 0.5 / N)
    call = lambda sl, ps: eng.diffuse_jacobian(A[:, :, sl].contiguous(), V, [0.95], [0.6], beam[:, sl].contiguous(), sun[sl].contiguous(),
                                               0.7, dV[ps], dlnb[ps][:, :, sl].contiguous(), Q[:, :, sl].contiguous(),
                                               surface_albedo=0.4)
    whole = call(slice(0, n_pts), slice(0, n_par))
    assert bool(torch.isfinite(whole).all()) and bool((whole != 0).all())
    for sl in (slice(0, 256), slice(256, n_pts)):
        for ps in (slice(0, 4), slice(4, n_par)):
            assert torch.equal(call(sl, ps), whole[:, ps, sl])


def test_central_differences_of_the_source_on_the_device(eng):
    """K = dJ against central differences of engine.diffuse_source(mean_intensity=True) at V +- h dV, beam exp(+- h dlnbeam):
    |K - FD(h/2)| <= 2 |FD(h) - FD(h/2)| + 1e-9 max |K|, h = 1e-2 of relative directions (the truncation term leads: the
    rounding of a difference at this step is 1e-14 of J)."""
    rng = np.random.default_rng(23)
    c = DJ.directions(rng, R.bvp_case(rng, 17, n_pts=65), 3, 0, relative=True)
    assert np.any(c["dV"][0] != 0) and np.any(c["dV"][2] != 0)
    K = _np(_call(eng, c, tangent=True))
    A, sun = _dev(c["A"]), _dev(c["sun"])

    def J(p, h):
        return _np(eng.diffuse_source(A, c["V"] + h * c["dV"][p], c["ssa"], c["asym"], _dev(c["beam"] * np.exp(h * c["dlnbeam"][p])),
                                      sun, c["mu0"], surface_albedo=c["albedo"], mean_intensity=True))

    h = 1e-2
    for p in range(3):
        fd1, fd2 = (J(p, h) - J(p, -h)) / (2 * h), (J(p, h / 2) - J(p, -h / 2)) / h
        slack = 2 * np.abs(fd1 - fd2) + 1e-9 * np.max(np.abs(K[p]))
        miss = np.abs(K[p] - fd2) / slack
        print("\nparameter %d: |K - FD(h/2)| / (2 |FD(h) - FD(h/2)| + 1e-9 max|K|) <= %.3f" % (p, float(miss.max())))
        assert np.all(miss <= 1.0)


def test_every_refusal_leaves_the_outputs_untouched(eng):
    import torch
    from spectrobot_amd import _lib
    lib, dp, ip = _lib.lib, _lib.dp, _lib.ip
    c = _case(17, 3, 65, 5, 8)
    n_layers, n_gas, n_pts, n_par, n_rays = 17, 3, 65, 5, 8
    A, beam, sun, dlnb, Q = (_dev(c[k]) for k in ("A", "beam", "sun", "dlnbeam", "Q"))
    bufs = [torch.full(s, -7.0, dtype=torch.float64, device="cuda") for s in ((n_rays, n_par, n_pts), (n_par, n_layers, n_pts))]
    V, ssa, asym, dV = (np.array(c[k]) for k in ("V", "ssa", "asym", "dV"))
    slot = np.arange(n_par, dtype=np.int32)
    good = dict(v=V, ssa=ssa, asym=asym, dv=dV, n_gas=n_gas, n_layers=n_layers, n_par=n_par, mu0=c["mu0"], alb=c["albedo"], A=A,
                beam=beam, sun=sun, dlnb=dlnb, q=Q, n_rays=n_rays, n_pts=n_pts, slot=slot, jac=bufs[0], rows=n_par, acc=0,
                dj=bufs[1], desc=True, jdesc=True)
    ptr = lambda t: None if t is None else C.c_void_p(t.data_ptr())
    hp = lambda a: None if a is None else a.ctypes.data_as(dp)

    def call(**kw):
        a = dict(good, **kw)
        d, jd = _lib.DiffuseDesc(), _lib.DiffuseJacDesc()
        d.n_gas, d.n_layers, d.v, d.ssa, d.asym = a["n_gas"], a["n_layers"], hp(a["v"]), hp(a["ssa"]), hp(a["asym"])
        d.mu0, d.surface_albedo = a["mu0"], a["alb"]
        jd.n_par, jd.dv = a["n_par"], hp(a["dv"])
        return lib.sr_diffuse_jacobian_rows_dev(C.byref(d) if a["desc"] else None, C.byref(jd) if a["jdesc"] else None, ptr(a["A"]),
                                                ptr(a["beam"]), ptr(a["sun"]), ptr(a["dlnb"]), ptr(a["q"]), a["n_rays"], a["n_pts"],
                                                None if a["slot"] is None else a["slot"].ctypes.data_as(ip), ptr(a["jac"]), a["rows"],
                                                a["acc"], ptr(a["dj"]), None)

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
             ("n_par 0", dict(n_par=0), ARG), ("q without jac", dict(jac=None), ARG), ("jac without q", dict(q=None), ARG),
             ("no output", dict(q=None, jac=None, dj=None), ARG), ("jac without par_slot", dict(slot=None), ARG),
             ("n_rays 0", dict(n_rays=0), ARG), ("n_jac_rows 0", dict(rows=0), ARG),
             ("v negative", dict(v=edited(V, (2, 16), -1e-30)), ARG), ("v nan", dict(v=edited(V, (0, 0), nan)), ARG),
             ("ssa above 1", dict(ssa=edited(ssa, 2, 1.0 + 2.0 ** -52)), ARG), ("asym 1", dict(asym=edited(asym, 2, 1.0)), ARG),
             ("mu0 nan", dict(mu0=nan), ARG), ("albedo above 1", dict(alb=1.01), ARG),
             ("dv nan", dict(dv=edited(dV, (4, 2, 16), nan)), ARG), ("dv inf", dict(dv=edited(dV, (0, 0, 0), -inf)), ARG),
             ("n_gas beyond the limit", dict(n_gas=9), LIMIT), ("n_layers beyond the limit", dict(n_layers=_lib.SR_MAX_ABS_ROWS + 1), LIMIT),
             ("n_pts beyond the limit", dict(n_pts=2000001), LIMIT), ("dv beyond the limit", dict(n_par=2 ** 23 // (n_gas * n_layers) + 1), LIMIT),
             ("par_slot negative", dict(slot=edited(slot, 0, -1)), ARG), ("par_slot beyond the rows", dict(slot=edited(slot, 4, n_par)), ARG),
             ("par_slot twice", dict(slot=edited(slot, 3, 1)), ARG)]
    for what, kw, status in cases:
        assert call(**kw) == status, what
    torch.cuda.synchronize()
    assert all(bool((b == -7.0).all()) for b in bufs)
    # a valid call afterwards gives the reference's numbers
    assert call() == 0
    torch.cuda.synchronize()
    assert R.ratio(_np(bufs[0]), c["ref_jac"], c["b_jac"]) <= 1.0 and R.ratio(_np(bufs[1]), c["ref_dJ"], c["b_dJ"]) <= 1.0
    # the host layer's own refusals
    a = (A, V, ssa, asym, beam, sun, 0.5, dV, dlnb, Q)
    with pytest.raises(ValueError):
        eng.diffuse_jacobian(*a, accumulate=True)
    with pytest.raises(ValueError):
        eng.diffuse_jacobian(*a, par_slot=[0, 1, 2, 3, 4])
    with pytest.raises(ValueError):
        eng.diffuse_jacobian(*a[:7], dV[:, :, :-1], dlnb, Q)
    with pytest.raises(ValueError):
        eng.diffuse_jacobian(*a[:8], dlnb[:, :-1].contiguous(), Q)
    with pytest.raises(ValueError):
        eng.diffuse_jacobian(*a[:9], Q[:, :-1].contiguous())
    with pytest.raises(ValueError):
        eng.diffuse_jacobian(*a[:9], None)
    with pytest.raises(ValueError):
        eng.diffuse_jacobian(*a, out=bufs[0], par_slot=[0, 1, 2])
