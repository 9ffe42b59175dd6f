"""The diffuse rows along a direction in the haze optics on the GPU (engine.diffuse_optics_jacobian,
sr_diffuse_optics_jacobian_rows_dev) against the extended-precision reference of tests/diffuse_optics_reference.py: the
bound panel for jac and dJ, the cross-check through sr_diffuse_jacobian_rows_dev, central differences of
engine.diffuse_source on the device in ssa, asym and the surface albedo, exact zeros, scaling, repeatability, accumulate /
par_slot, a call across the workspace cap, and every refusal class."""
import ctypes as C

import numpy as np
import pytest

import diffuse_jacobian_reference as DJ
import diffuse_optics_reference as DO
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
    return eng.diffuse_optics_jacobian(_dev(c["A"]), c["V"], c["ssa"], c["asym"], _dev(c["beam"]), _dev(c["sun"]), c["mu0"], c["dssa"],
                                       c["dasym"], c["dalb"], _dev(c["dlnbeam"]), _dev(c["Q"]), **kw)


def _case(*key):
    """A panel case with its reference and bounds, made once and shared (read-only)."""
    if key not in _case.cache:
        c = DO.panel_case(*key)
        ref = DO.reference(c, yardstick=True)
        n_gas, n_layers = c["A"].shape[:2]
        c = dict(c, ref_dJ=ref["dJ"], ref_jac=ref["jac"], b_dJ=DO.bound(ref["S_dJ"], n_gas, n_layers),
                 b_jac=DO.bound(ref["S_jac"], n_gas, n_layers))
        for v in c.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        _case.cache[key] = c
    return _case.cache[key]


_case.cache = {}


@pytest.mark.parametrize("n_layers", R.N_LAYERS)
def test_panel_inside_the_bound(eng, n_layers):
    worst = dict(jac=0.0, dJ=0.0)
    for key in DO.PANEL:
        if key[0] != n_layers:
            continue
        c = _case(*key)
        jac, dJ = _call(eng, c, tangent=True)
        for k, got in (("jac", jac), ("dJ", dJ)):
            r = R.ratio(_np(got), c["ref_" + k], c["b_" + k])
            print("\ndiffuse optics panel %s: |GPU - reference| / b, %s %.3f" % (key, k, r))
            worst[k] = max(worst[k], r)
        # the other instances give the same bits
        assert np.array_equal(_np(_call(eng, c)), _np(jac))
        assert np.array_equal(_np(_call(eng, dict(c, Q=None), tangent=True)), _np(dJ))
    print("diffuse optics panel, n_layers %d: worst %s" % (n_layers, worst))
    assert max(worst.values()) <= 1.0, worst


def test_pure_asym_directions_over_the_panel(eng):
    """Asym alone with the beam held fixed (dsg's path by itself), which the yardstick's S cannot bound pointwise, over every
    shape of the panel: |GPU - reference| within eps (n_gas + C_OPTICS n_layers + 16) of the column's largest S
    (DO.column_bound: the yardstick with S's maximum over the layers; times sum_l Q for jac) -- the restatement's 0.5 on the host times the project's factor 2."""
    worst = 0.0
    for key in DO.PANEL:
        c = DO.pure_asym_case(*key)
        ref = DO.reference(c, yardstick=True)
        b = DO.column_bound(ref, c["Q"], *c["A"].shape[:2])
        jac, dJ = _call(eng, c, tangent=True)
        worst = max(worst, R.ratio(_np(dJ), ref["dJ"], b["dJ"]), R.ratio(_np(jac), ref["jac"], b["jac"]))
    print("\npure asym directions over the panel: |GPU - reference| / column bound %.3f" % worst)
    assert worst <= 1.0


def test_cross_check_through_the_column_entry(eng):
    """A one-gas column of albedo w has the layer sums of a two-gas column on the same absorption rows: a pure scatterer
    (ssa 1) with V_a = w V and a pure absorber (ssa 0) with V_b = (1 - w) V, both at the same asym.  So dssa = 1 on the one
    gas is dV_a = V, dV_b = -V through sr_diffuse_jacobian_rows_dev: the two agree within the sum of the two bounds."""
    worst = 0.0
    for n_layers, n_pts, w, g in ((1, 63, 0.9, 0.6), (3, 65, 0.5, -0.3), (17, 257, 0.97, 0.75), (80, 65, 0.3, 0.0)):
        rng = np.random.default_rng([20261023, 77, n_layers])
        base = R.column_case(rng, n_layers, 1, n_pts, tau_lo=1e-3, tau_hi=20.0, conservative=0.0, empty=0.1)
        n_par, n_rays = 2, 3
        dlnb = rng.uniform(-1.0, 1.0, (n_par, n_layers + 1, n_pts))
        dlnb[1] = 0.0
        Q = rng.uniform(0.1, 1.0, (n_rays, n_layers, n_pts))
        V = base["V"]
        one = dict(base, ssa=np.array([w]), asym=np.array([g]), dssa=np.ones((n_par, 1)), dasym=None, dalb=None, dlnbeam=dlnb, Q=Q)
        two = dict(base, A=np.concatenate([base["A"], base["A"]]), V=np.concatenate([w * V, (1.0 - w) * V]), ssa=np.array([1.0, 0.0]),
                   asym=np.array([g, g]), dV=np.broadcast_to(np.concatenate([V, -V])[None], (n_par, 2, n_layers)).copy(), dlnbeam=dlnb, Q=Q)
        ro, rt = DO.reference(one, yardstick=True), DJ.reference(two, yardstick=True)
        b = {k: DO.bound(ro["S_" + k], 1, n_layers) + DJ.bound(rt["S_" + k], 2, n_layers) for k in ("jac", "dJ")}
        jac_o, dJ_o = _call(eng, one, tangent=True)
        jac_t, dJ_t = eng.diffuse_jacobian(_dev(two["A"]), two["V"], two["ssa"], two["asym"], _dev(two["beam"]), _dev(two["sun"]),
                                           two["mu0"], two["dV"], _dev(dlnb), _dev(Q), surface_albedo=two["albedo"], tangent=True)
        assert _np(jac_o).any()
        for k, x, y in (("jac", jac_o, jac_t), ("dJ", dJ_o, dJ_t)):
            r = R.ratio(_np(x) - _np(y), np.zeros(x.shape, LD), b[k])
            print("\noptics entry against the column entry, %d layers, %s: |difference| / (b + b) %.3f" % (n_layers, k, r))
            worst = max(worst, r)
    assert worst <= 1.0


def test_central_differences_of_the_source_on_the_device(eng):
    """K = dJ against central differences of engine.diffuse_source(mean_intensity=True) in ssa, asym and the surface
    albedo, one at a time, the beam held fixed: |K - FD(h/2)| <= 2 |FD(h) - FD(h/2)| + 1e-9 max |K|, h = 1e-2.  The asym
    directions are the pure ones the yardstick's panel leaves out (a gas with asym > 0 and one with asym < 0)."""
    rng = np.random.default_rng(29)
    c = R.bvp_case(rng, 17, n_pts=65)
    c = dict(c, ssa=np.array([0.7, 0.2]), asym=np.array([0.5, -0.2]), albedo=0.4)
    dssa = np.array([[1.0, 0.0], [0.0, 0.0], [0.0, 0.0], [0.0, 0.0]])
    dasym = np.array([[0.0, 0.0], [1.0, 0.0], [0.0, 1.0], [0.0, 0.0]])
    dalb = np.array([0.0, 0.0, 0.0, 1.0])
    c = dict(c, dssa=dssa, dasym=dasym, dalb=dalb, dlnbeam=None, Q=None)
    K = _np(_call(eng, c, tangent=True))
    A, beam, sun = _dev(c["A"]), _dev(c["beam"]), _dev(c["sun"])

    def J(p, h):
        return _np(eng.diffuse_source(A, c["V"], c["ssa"] + h * dssa[p], c["asym"] + h * dasym[p], beam, sun, c["mu0"],
                                      surface_albedo=c["albedo"] + h * dalb[p], mean_intensity=True))

    h = 1e-2
    for p in range(4):
        fd1, fd2 = (J(p, h) - J(p, -h)) / (2 * h), (J(p, h / 2) - J(p, -h / 2)) / h
        slack = 2 * np.abs(fd1 - fd2) + 1e-9 * np.max(np.abs(K[p]))
        miss = np.abs(K[p] - fd2) / slack
        print("\noptics parameter %d: |K - FD(h/2)| / (2 |FD(h) - FD(h/2)| + 1e-9 max|K|) <= %.3f" % (p, float(miss.max())))
        assert np.any(K[p] != 0) and np.all(miss <= 1.0)


def test_exact_zeros(eng):
    c = _case(17, 3, 257, 5, 8)
    zero = lambda a: np.zeros_like(a)
    none = dict(c, dssa=zero(c["dssa"]), dasym=zero(c["dasym"]), dalb=zero(c["dalb"]))
    jac, dJ = _call(eng, dict(none, dlnbeam=zero(c["dlnbeam"])), tangent=True)                      # no direction
    assert not _np(jac).any() and not _np(dJ).any()
    jac, dJ = _call(eng, dict(none, dlnbeam=None, dssa=None, dasym=None), tangent=True)            # ... with the beam held fixed
    assert not _np(jac).any() and not _np(dJ).any()
    jac, dJ = _call(eng, dict(c, Q=zero(c["Q"])), tangent=True)                                    # no ray sees J
    assert not _np(jac).any() and _np(dJ).any()
    jac, dJ = _call(eng, dict(c, sun=zero(c["sun"])), tangent=True)                                # shadow
    assert not _np(jac).any() and not _np(dJ).any()
    # a direction in the albedo with the sun at or below the horizon and no light from above: the ground has nothing to return
    beam = zero(c["beam"])
    beam[-1] = 1.0
    dark = dict(c, beam=beam, dssa=None, dasym=None, dalb=np.ones(5), dlnbeam=None)
    for mu0 in (0.0, -0.3):
        jac, dJ = _call(eng, dict(dark, mu0=mu0), tangent=True)
        assert not _np(jac).any() and not _np(dJ).any()
    jac, dJ = _call(eng, dict(dark, mu0=0.5), tangent=True)                                        # (above the horizon it does)
    assert _np(jac).all() and _np(dJ).all()


def test_scaling_repeatability_accumulate_and_slots(eng):
    c = _case(80, 3, 257, 2, 8)
    jac, dJ = _call(eng, c, tangent=True)
    twice = dict(c, dssa=2.0 * c["dssa"], dasym=2.0 * c["dasym"], dalb=2.0 * c["dalb"], dlnbeam=2.0 * c["dlnbeam"])
    jac2, dJ2 = _call(eng, twice, tangent=True)                                                     # a direction x 2: bits x 2
    assert np.array_equal(_np(jac2), 2.0 * _np(jac)) and np.array_equal(_np(dJ2), 2.0 * _np(dJ)) and _np(jac).any()
    again = _call(eng, c, tangent=True)                                                             # two calls: the same bits
    assert np.array_equal(_np(again[0]).view(np.uint64), _np(jac).view(np.uint64))
    assert np.array_equal(_np(again[1]).view(np.uint64), _np(dJ).view(np.uint64))
    n_rays, n_pts = jac.shape[0], jac.shape[2]
    base = np.random.default_rng(5).uniform(-1.0, 1.0, (n_rays, 5, n_pts)) * float(np.abs(_np(jac)).max())
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
    # a parameter's rows do not depend on its neighbours in the tile: the albedo-only direction alone
    c9 = _case(17, 1, 65, 9, 9)
    full = _np(_call(eng, c9))
    for p in (2, 5):
        alone = dict(c9, dssa=c9["dssa"][p:p + 1], dasym=c9["dasym"][p:p + 1], dalb=c9["dalb"][p:p + 1], dlnbeam=c9["dlnbeam"][p:p + 1])
        assert np.array_equal(_np(_call(eng, alone))[:, 0], full[:, p])


def test_a_call_across_the_workspace_cap_gives_the_bits_of_its_parts(eng):
    """4096 layers x 512 points x 5 parameters (two tiles): the workspace cap makes it two point chunks of 256 x two tiles
    (test_gpu_diffuse_jacobian.py has the arithmetic).  Points and parameters are independent, so each part called alone
    gives the same bits."""
    import torch
    rng = np.random.default_rng(31)
    N, n_pts, n_par, n_rays = 4096, 512, 5, 2
    A = torch.as_tensor(rng.uniform(0.5, 1.5, (1, N, n_pts)), device="cuda")
    beam = torch.as_tensor(np.exp(-np.linspace(3.0, 0.0, N + 1))[:, None] * rng.uniform(0.9, 1.0, (N + 1, n_pts)), device="cuda")
    sun = torch.as_tensor(rng.uniform(5.0, 20.0, n_pts), device="cuda")
    Q = torch.as_tensor(rng.uniform(0.1, 1.0, (n_rays, N, n_pts)), device="cuda")
    dlnb = torch.as_tensor(rng.uniform(-1.0, 1.0, (n_par, N + 1, n_pts)), device="cuda")
    V = np.full((1, N), 2.0 / N)
    dssa = np.array([[0.5], [0.0], [0.0], [-1.0], [0.3]])
    dasym = np.array([[0.0], [1.0], [0.0], [0.5], [0.0]])
    dalb = np.array([0.0, 0.0, 1.0, -0.5, 0.0])
    call = lambda sl, ps: eng.diffuse_optics_jacobian(A[:, :, sl].contiguous(), V, [0.95], [0.6], beam[:, sl].contiguous(),
                                                      sun[sl].contiguous(), 0.7, dssa[ps], dasym[ps], dalb[ps],
                                                      dlnb[ps][:, :, sl].contiguous(), Q[:, :, sl].contiguous(), surface_albedo=0.4)
    whole = call(slice(0, n_pts), slice(0, n_par))
    assert bool(torch.isfinite(whole).all()) and bool((whole != 0).all())
    for sl in (slice(0, 256), slice(256, n_pts)):
        for ps in (slice(0, 4), slice(4, n_par)):
            assert torch.equal(call(sl, ps), whole[:, ps, sl])


def test_every_refusal_leaves_the_outputs_untouched(eng):
    import torch
    from spectrobot_amd import _lib
    lib, dp, ip = _lib.lib, _lib.dp, _lib.ip
    c = _case(17, 3, 65, 5, 8)
    n_layers, n_gas, n_pts, n_par, n_rays = 17, 3, 65, 5, 8
    A, beam, sun, dlnb, Q = (_dev(c[k]) for k in ("A", "beam", "sun", "dlnbeam", "Q"))
    bufs = [torch.full(s, -7.0, dtype=torch.float64, device="cuda") for s in ((n_rays, n_par, n_pts), (n_par, n_layers, n_pts))]
    V, ssa, asym, dssa, dasym, dalb = (np.array(c[k]) for k in ("V", "ssa", "asym", "dssa", "dasym", "dalb"))
    slot = np.arange(n_par, dtype=np.int32)
    good = dict(v=V, ssa=ssa, asym=asym, dssa=dssa, dasym=dasym, dalb=dalb, n_gas=n_gas, n_layers=n_layers, n_par=n_par, mu0=c["mu0"],
                alb=c["albedo"], A=A, beam=beam, sun=sun, dlnb=dlnb, q=Q, n_rays=n_rays, n_pts=n_pts, slot=slot, jac=bufs[0], rows=n_par,
                acc=0, dj=bufs[1], desc=True, odesc=True)
    ptr = lambda t: None if t is None else C.c_void_p(t.data_ptr())
    hp = lambda a: None if a is None else a.ctypes.data_as(dp)

    def call(**kw):
        a = dict(good, **kw)
        d, od = _lib.DiffuseDesc(), _lib.DiffuseOpticsDesc()
        d.n_gas, d.n_layers, d.v, d.ssa, d.asym = a["n_gas"], a["n_layers"], hp(a["v"]), hp(a["ssa"]), hp(a["asym"])
        d.mu0, d.surface_albedo = a["mu0"], a["alb"]
        od.n_par, od.dssa, od.dasym, od.dalb = a["n_par"], hp(a["dssa"]), hp(a["dasym"]), hp(a["dalb"])
        return lib.sr_diffuse_optics_jacobian_rows_dev(C.byref(d) if a["desc"] else None, C.byref(od) if a["odesc"] else None,
                                                       ptr(a["A"]), ptr(a["beam"]), ptr(a["sun"]), ptr(a["dlnb"]), ptr(a["q"]),
                                                       a["n_rays"], a["n_pts"], None if a["slot"] is None else a["slot"].ctypes.data_as(ip),
                                                       ptr(a["jac"]), a["rows"], a["acc"], ptr(a["dj"]), None)

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
             ("n_par 0", dict(n_par=0), ARG), ("q without jac", dict(jac=None), ARG), ("jac without q", dict(q=None), ARG),
             ("no output", dict(q=None, jac=None, dj=None), ARG), ("jac without par_slot", dict(slot=None), ARG),
             ("n_rays 0", dict(n_rays=0), ARG), ("n_jac_rows 0", dict(rows=0), ARG),
             ("v negative", dict(v=edited(V, (2, 16), -1e-30)), ARG), ("v nan", dict(v=edited(V, (0, 0), nan)), ARG),
             ("ssa above 1", dict(ssa=edited(ssa, 2, 1.0 + 2.0 ** -52)), ARG), ("asym 1", dict(asym=edited(asym, 2, 1.0)), ARG),
             ("mu0 nan", dict(mu0=nan), ARG), ("albedo above 1", dict(alb=1.01), ARG),
             ("dssa nan", dict(dssa=edited(dssa, (4, 2), nan)), ARG), ("dasym inf", dict(dasym=edited(dasym, (0, 0), -inf)), ARG),
             ("dalb nan", dict(dalb=edited(dalb, 2, nan)), ARG),
             ("n_gas beyond the limit", dict(n_gas=9), LIMIT), ("n_layers beyond the limit", dict(n_layers=_lib.SR_MAX_ABS_ROWS + 1), LIMIT),
             ("n_pts beyond the limit", dict(n_pts=2000001), LIMIT), ("n_par beyond the limit", dict(n_par=2 ** 23 // (n_gas * n_layers) + 1), LIMIT),
             ("par_slot negative", dict(slot=edited(slot, 0, -1)), ARG), ("par_slot beyond the rows", dict(slot=edited(slot, 4, n_par)), ARG),
             ("par_slot twice", dict(slot=edited(slot, 3, 1)), ARG)]
    for what, kw, status in cases:
        assert call(**kw) == status, what
    torch.cuda.synchronize()
    assert all(bool((b == -7.0).all()) for b in bufs)
    # a valid call afterwards gives the reference's numbers; so does one with a NULL direction in place of zeros
    assert call() == 0
    torch.cuda.synchronize()
    assert R.ratio(_np(bufs[0]), c["ref_jac"], c["b_jac"]) <= 1.0 and R.ratio(_np(bufs[1]), c["ref_dJ"], c["b_dJ"]) <= 1.0
    # the host layer's own refusals
    a = (A, V, ssa, asym, beam, sun, 0.5, dssa, dasym, dalb, dlnb, Q)
    with pytest.raises(ValueError):
        eng.diffuse_optics_jacobian(*a, accumulate=True)
    with pytest.raises(ValueError):
        eng.diffuse_optics_jacobian(*a, par_slot=[0, 1, 2, 3, 4])
    with pytest.raises(ValueError):
        eng.diffuse_optics_jacobian(*a[:7], None, None, None, dlnb, Q)
    with pytest.raises(ValueError):
        eng.diffuse_optics_jacobian(*a[:7], dssa[:, :-1], dasym, dalb, dlnb, Q)
    with pytest.raises(ValueError):
        eng.diffuse_optics_jacobian(*a[:9], dalb[:-1], dlnb, Q)
    with pytest.raises(ValueError):
        eng.diffuse_optics_jacobian(*a[:10], dlnb[:, :-1].contiguous(), Q)
    with pytest.raises(ValueError):
        eng.diffuse_optics_jacobian(*a[:11], Q[:, :-1].contiguous())
    with pytest.raises(ValueError):
        eng.diffuse_optics_jacobian(*a[:11], None)
    with pytest.raises(ValueError):
        eng.diffuse_optics_jacobian(*a, out=bufs[0], par_slot=[0, 1, 2])
