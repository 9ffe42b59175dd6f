"""The single-scattering solar source on the GPU: sr_solar_source_kernel through engine.solar_source against the long-double
definition of tests/solar_source_reference.py inside its bound on the panel of tile, chunk and store edges (n_rows 1, 15,
17, 33, 65 x n_k 1, 3, 5, 13, 160 x n_pts 1, 63, 65, 257), the exact cases, a second batch of chunks (n_k 259), every
refusal, and the plumbing above it: a homogeneous segment through engine.limb_rays against S (1 - exp(-tau_los)), the
composed torch route, a scene with a sun whose scatterer has albedo 0 against the scene without one, and the state Jacobian
of a line gas + sunlit haze scene against central differences with the solar rows frozen."""
import copy
import ctypes as C

import numpy as np
import pytest

import solar_source_cases as SC
import solar_source_reference as R

pytestmark = pytest.mark.gpu
LD, EPS = R.LD, R.EPS53


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
    return eng.solar_source(_dev(c["A"]), c["U"], c["w"], _dev(c["sca"]), _dev(c["sun"]), src_row=c["src_row"], **kw)


def _case(n_rows, n_k, n_pts):
    """A panel case with its reference, made once and shared (read-only)."""
    key = (n_rows, n_k, n_pts)
    if key not in _case.cache:
        c = R.panel_case(*key)
        emi, trans, tau, K = R.reference(c["A"], c["U"], c["w"], c["sca"], c["sun"], c["src_row"])
        c.update(emi=emi, trans=trans, tau=tau, b_emi=R.bound_emi(emi, tau, K), b_trans=R.bound_trans(trans, tau, K))
        for v in c.values():
            v.setflags(write=False)
        _case.cache[key] = c
    return _case.cache[key]


_case.cache = {}


@pytest.mark.parametrize("n_rows", R.N_ROWS)
def test_panel_inside_the_bound(eng, n_rows):
    worst = {"emi": 0.0, "trans": 0.0}
    lo, hi = np.inf, 0.0
    for n_k in R.N_K:
        for n_pts in R.N_PTS:
            c = _case(n_rows, n_k, n_pts)
            emi, trans = _call(eng, c, transmission=True)
            worst["emi"] = max(worst["emi"], R.ratio(_np(emi), c["emi"], c["b_emi"]))
            worst["trans"] = max(worst["trans"], R.ratio(_np(trans), c["trans"], c["b_trans"]))
            only = _call(eng, c)                                    # the instance without the transmission: the same bits
            assert np.array_equal(_np(only), _np(emi))
            lit = c["tau"][c["tau"] > 0]
            if lit.size:
                lo, hi = min(lo, float(lit.min())), max(hi, float(lit.max()))
    print("\nsolar source panel, n_rows %d: tau %.2e .. %.1f, |GPU - reference| / bound %s" % (n_rows, lo, hi, worst))
    assert worst["emi"] <= 1.0 and worst["trans"] <= 1.0, worst


def _exact_case():
    c = {k: np.array(v) for k, v in R.panel_case(33, 160, 65).items()}
    c["U"][:16, :64] = 0.0                           # the first tile's rows start at k = 64: sixteen chunks to skip
    c["U"][3] = 0.0                                  # no columns: trans == 1
    c["w"][[5, 20]] = 0.0                            # in shadow (their columns stay)
    c["U"][7, -1] = 701.0 / c["A"][-1].min()         # tau >= 700 at every point
    c["U"][24, 2] = 1e6                              # ... and far beyond
    return c


def test_exact_cases(eng):
    import torch
    c = _exact_case()
    emi, trans = _call(eng, c, transmission=True)
    e, t = _np(emi), _np(trans)
    assert np.all(t[3] == 1.0)
    want3 = c["sca"][c["src_row"][3]] * ((c["w"][3] * c["sun"]) * 1.0)
    assert np.max(np.abs(e[3] - want3)) <= 2 * EPS * want3.max()
    assert np.all(e[[5, 20]] == 0.0) and np.all(t[[5, 20]] == 0.0)
    assert np.all(e[[7, 24]] == 0.0) and np.all(t[[7, 24]] == 0.0)
    ref_e, ref_t, tau, K = R.reference(c["A"], c["U"], c["w"], c["sca"], c["sun"], c["src_row"])
    assert R.ratio(e, ref_e, R.bound_emi(ref_e, tau, K)) <= 1.0 and R.ratio(t, ref_t, R.bound_trans(ref_t, tau, K)) <= 1.0
    # two calls: identical bits
    emi2, trans2 = _call(eng, c, transmission=True)
    assert torch.equal(emi, emi2) and torch.equal(trans, trans2)
    # full chunk lists: the skipped chunks only add exact zeros
    off, ch = eng.solar_chunk_lists(c["U"], c["w"])
    eng.set_solar_full_lists(True)
    try:
        emi3, trans3 = _call(eng, c, transmission=True)
        off_f, ch_f = eng.solar_chunk_lists(c["U"], c["w"])
    finally:
        eng.set_solar_full_lists(False)
    assert torch.equal(emi, emi3) and torch.equal(trans, trans3)
    assert ch.size < ch_f.size                       # (the sparse call did skip chunks)
    # accumulate: the overwrite result plus the base, to one rounding; rows in shadow keep their bits
    base = torch.as_tensor(np.random.default_rng(5).uniform(-1e-8, 1e-8, e.shape), device="cuda")
    base[20] = float("nan")                          # (a row in shadow is not even read)
    acc = base.clone()
    out, trans4 = _call(eng, c, out=acc, accumulate=True, transmission=True)
    assert out is acc and torch.equal(trans4, trans)
    a, b = _np(acc), _np(base)
    assert np.array_equal(a[[5, 20]].view(np.uint64), b[[5, 20]].view(np.uint64))
    rows = np.setdiff1d(np.arange(33), [5, 20])
    s = b[rows].astype(LD) + e[rows].astype(LD)
    assert np.all(np.abs(a[rows].astype(LD) - s) <= EPS * np.abs(s))
    acc2 = base.clone()
    _call(eng, c, out=acc2, accumulate=True)         # ... without the transmission too
    assert np.array_equal(_np(acc2).view(np.uint64), a.view(np.uint64))


def test_a_second_batch_of_chunks(eng):
    """n_k = 259 is 65 chunks: with every chunk listed a tile walks one whole batch of 64 through LDS, then a batch of one
    chunk padded to a pair, the last chunk of three k -- on 17 rows (a second row tile of one row) and 65 points (a partial
    quad).  Overwrite with the transmission and accumulate, each inside the bound with full lists and bit for bit the
    sparse-list call."""
    import torch
    c = _case(17, 259, 65)
    base = np.random.default_rng(5).uniform(-1e-8, 1e-8, (17, 65))

    def both():
        emi, trans = _call(eng, c, transmission=True)
        acc = _call(eng, c, out=_dev(base), accumulate=True)
        return emi, trans, acc

    sparse = both()
    eng.set_solar_full_lists(True)
    try:
        full = both()
        off_f, ch_f = eng.solar_chunk_lists(c["U"], c["w"])
    finally:
        eng.set_solar_full_lists(False)
    assert list(np.diff(off_f)) == [65, 65] and ch_f[64] == 64            # (a second batch in every tile)
    e, t, a = (_np(x) for x in full)
    assert R.ratio(e, c["emi"], c["b_emi"]) <= 1.0 and R.ratio(t, c["trans"], c["b_trans"]) <= 1.0
    s = base.astype(LD) + e.astype(LD)                                    # the overwrite result plus the base, to one rounding
    assert np.all(np.abs(a.astype(LD) - s) <= EPS * np.abs(s))
    for x, y in zip(sparse, full):
        assert torch.equal(x, y)


def test_every_refusal_leaves_the_outputs_untouched(eng):
    import torch
    from spectrobot_amd import _lib
    lib, dp, ip = _lib.lib, _lib.dp, _lib.ip
    c = _case(17, 5, 65)
    n_rows, n_k, n_pts, n_src = 17, 5, 65, c["sca"].shape[0]
    A, sca, sun = _dev(c["A"]), _dev(c["sca"]), _dev(c["sun"])
    bufs = [torch.full((n_rows, n_pts), -7.0, dtype=torch.float64, device="cuda") for _ in range(2)]
    U, w, src = np.array(c["U"]), np.array(c["w"]), np.array(c["src_row"], dtype=np.int32)
    good = dict(u=U, w=w, src=src, n_rows=n_rows, A=A, n_k=n_k, sca=sca, n_src=n_src, sun=sun, n_pts=n_pts, acc=0, e=bufs[0], t=bufs[1], desc=True)
    ptr = lambda t: None if t is None else C.c_void_p(t.data_ptr())

    def call(**kw):
        a = dict(good, **kw)
        d = _lib.SolarDesc()
        d.n_rows = a["n_rows"]
        d.u = None if a["u"] is None else a["u"].ctypes.data_as(dp)
        d.w = None if a["w"] is None else a["w"].ctypes.data_as(dp)
        d.src_row = None if a["src"] is None else a["src"].ctypes.data_as(ip)
        return lib.sr_solar_source_rows_dev(C.byref(d) if a["desc"] else None, ptr(a["A"]), a["n_k"], ptr(a["sca"]), a["n_src"],
                                            ptr(a["sun"]), a["n_pts"], a["acc"], ptr(a["e"]), ptr(a["t"]), None)

    def edited(arr, at, v):
        out = arr.copy()
        out[at] = v
        return out

    ARG, LIMIT = _lib.SR_ERR_ARG, _lib.SR_ERR_LIMIT
    cases = [("null desc", dict(desc=False), ARG), ("null u", dict(u=None), ARG), ("null w", dict(w=None), ARG),
             ("null src_row", dict(src=None), ARG), ("null tab_abs", dict(A=None), ARG), ("null sca_abs", dict(sca=None), ARG),
             ("null sun", dict(sun=None), ARG), ("null emi_out", dict(e=None), ARG), ("n_rows 0", dict(n_rows=0), ARG),
             ("n_rows < 0", dict(n_rows=-2), ARG), ("n_k 0", dict(n_k=0), ARG), ("n_src 0", dict(n_src=0), ARG), ("n_pts 0", dict(n_pts=0), ARG),
             ("u negative", dict(u=edited(U, (16, 4), -1e-30)), ARG), ("u nan", dict(u=edited(U, (0, 0), np.nan)), ARG),
             ("u inf", dict(u=edited(U, (9, 2), np.inf)), ARG), ("w negative", dict(w=edited(w, 3, -0.1)), ARG),
             ("w nan", dict(w=edited(w, 16, np.nan)), ARG), ("w inf", dict(w=edited(w, 0, np.inf)), ARG),
             ("src_row too large", dict(src=edited(src, 16, n_src)), ARG), ("src_row negative", dict(src=edited(src, 0, -1)), ARG),
             ("n_pts beyond the limit", dict(n_pts=2000001), LIMIT), ("n_rows beyond the limit", dict(n_rows=_lib.SR_MAX_ABS_ROWS + 1), LIMIT)]
    for what, kw, status in cases:
        assert call(**kw) == status, what
    big = np.zeros((4096, 2049))                     # n_rows n_k beyond SR_MAX_SOLAR_VALUES
    assert call(u=big, w=np.ones(4096), src=np.zeros(4096, np.int32), n_rows=4096, n_k=2049) == LIMIT
    torch.cuda.synchronize()
    assert all(bool((b == -7.0).all()) for b in bufs)
    # a valid call afterwards gives the reference's numbers
    assert call() == 0
    torch.cuda.synchronize()
    assert R.ratio(_np(bufs[0]), c["emi"], c["b_emi"]) <= 1.0 and R.ratio(_np(bufs[1]), c["trans"], c["b_trans"]) <= 1.0
    # the host layer's own refusals
    with pytest.raises(ValueError):
        eng.solar_source(A, U, w, sca, sun, src_row=src, accumulate=True)
    with pytest.raises(ValueError):
        eng.solar_source(A, U[:, :4], w, sca, sun, src_row=src)
    with pytest.raises(ValueError):
        eng.solar_source(A, U, w, sca, sun[:-1].contiguous(), src_row=src)


def test_homogeneous_segment_against_the_closed_form(eng):
    """Three rays of ONE segment each in a layer whose coefficients are (given absorption rows, the solar rows as emi),
    optically thin, tau_los ~ 1 and thick, through engine.limb_rays: rad = (emi / abs) (1 - exp(-tau_los)).  The tolerance
    is test_gpu_absorber_table.py's slab form with the solar bound in b_emi's place; the absorption rows are inputs here
    (exact), so their term is 0: |want| (b / |emi| + 16 eps)."""
    c = _case(15, 13, 257)
    n_pts, layer = 257, 4
    rng = np.random.default_rng(11)
    a_rows = rng.uniform(2e-24, 6e-24, (15, n_pts))
    emi = _call(eng, c)
    co = (_dev(a_rows), emi)
    nd = 4.0e17
    a_mid = float(np.median(a_rows[layer]))
    x = np.tile(np.array([0.0, 2.0e6, 4.0e6]), 3)
    vmr = np.repeat(np.array([1e-6, 1.0, 200.0]) / (a_mid * nd * 4.0e6), 3)
    los = eng.LimbLOS([0, 1, 2, 3], [layer] * 3, [0, 3, 6, 9], x, np.tile(nd * np.array([1.0, 0.96, 0.92]), 3), vmr[None, :])
    col = los.columns()[0]
    rad = _np(eng.limb_rays(co, los))
    S = c["emi"][layer] / a_rows[layer].astype(LD)
    rel = c["b_emi"][layer] / np.abs(c["emi"][layer])
    worst = []
    for r in range(3):
        tau = a_rows[layer].astype(LD) * LD(col[r])
        want = S * -np.expm1(-tau)
        tol = np.abs(want) * (rel + 16 * EPS)
        worst.append(float(np.max(np.abs(rad[r].astype(LD) - want) / tol)))
        print("\nsolar rows through limb_rays, tau_los %.3g .. %.3g: |rad - S (1 - exp(-tau))| / tolerance %.3f"
              % (float(tau.min()), float(tau.max()), worst[-1]))
    assert max(worst) <= 1.0, worst


def test_composed_torch_route_agrees(eng):
    import torch
    worst = 0.0
    for key in ((65, 160, 257), (33, 13, 65), (17, 5, 63)):
        c = _case(*key)
        A, sca, sun = _dev(c["A"]), _dev(c["sca"]), _dev(c["sun"])
        U, w = _dev(c["U"]), _dev(c["w"])
        src = torch.as_tensor(np.array(c["src_row"]), device="cuda").long()
        composed = sca[src] * w[:, None] * sun[None, :] * torch.exp(-(U @ A))
        fused = _call(eng, c)
        worst = max(worst, R.ratio(_np(fused) - _np(composed), np.zeros(key[::2], LD), 2 * c["b_emi"]))
    print("\nfused against composed: |difference| / 2 b %.3f" % worst)
    assert worst <= 1.0


def test_scene_with_a_dark_scatterer_equals_the_scene_without_a_sun(eng):
    """w = 0 everywhere (albedo 0) under accumulate: the existing routes give the same bits."""
    from spectrobot_amd import retrieval
    lit, dark = SC.solar_scene(eng, sun=True, albedo=0.0), SC.solar_scene(eng, sun=False)
    z = lit.z
    pixels = [retrieval.LimbPixel(z[0] + f * (z[-1] - z[0]), fov_half=2.0) for f in (0.05, 0.3)]
    got = np.array([y.spectrum for y in retrieval.radtrans(lit, pixels)])
    want = np.array([y.spectrum for y in retrieval.radtrans(dark, pixels)])
    haze = lit.gas("haze")
    assert haze.coeffs is not haze.thermal and haze.coeffs[1] is not haze.thermal[1]      # the solar pass ran, on a copy
    assert np.array_equal(got.view(np.uint64), want.view(np.uint64))
    # ... and with the albedo the sun is there
    bright = SC.solar_scene(eng, sun=True)
    more = np.array([y.spectrum for y in retrieval.radtrans(bright, pixels)])
    assert np.all(more > 10.0 * want)


def test_per_step_rows_of_a_3d_batch_at_constant_sza(eng):
    """The 3-D route -- geometry.limb_los_3d's rows, src_row = seg_alt_layer -- against the 1-D scene's layer rows: with
    the same sun on every step and every step's point at the middle of its shell, a step's columns are its layer's, and
    its solar rows the layer's rows gathered by seg_alt_layer, bit for bit (another tiling, other chunk lists).  Then
    the route as the example uses it (seg_mu, the steps' own middles) against the reference."""
    import torch
    from spectrobot_amd import geometry as G
    rng = np.random.default_rng(3)
    z = np.linspace(100.0, 540.0, 12)
    nd = 3e17 * np.exp(-(z - 100.0) / 63.0)
    vmr = np.array([np.full(12, 1e-2), 1e-3 * (1.0 + (z - 100.0) / 500.0)])
    zz = np.append(z, 2 * z[-1] - z[-2])
    n_pts = 130
    A = rng.uniform(1e-22, 1e-21, (2, 12, n_pts))
    sun, mu = rng.uniform(5.0, 20.0, n_pts), float(np.cos(np.deg2rad(50.0)))
    L3 = G.limb_los_3d(z, nd, vmr, [130.0, 260.0, 410.0], 50.0, 35.0)
    layer = L3["seg_alt_layer"]
    assert len(layer) > 32 and layer.max() == 11
    mid_shell = 0.5 * (zz[:-1] + zz[1:])
    U1, lit1 = G.solar_columns(z, nd, vmr, mid_shell, mu, col_scale=[0.9, 1.0])
    U3, lit3 = G.solar_columns(z, nd, vmr, mid_shell[layer], mu, col_scale=[0.9, 1.0])
    assert lit1.all() and lit3.all() and np.array_equal(U3, U1[layer])
    Ad, sca, sund = _dev(A), _dev(A[1]), _dev(sun)
    rows1 = eng.solar_source(Ad, U1, 0.05, sca, sund)
    rows3 = eng.solar_source(Ad, U3, 0.05, sca, sund, src_row=layer)
    assert torch.equal(rows3, rows1[torch.as_tensor(layer.astype(np.int64), device="cuda")])
    # per-step SZA and the steps' own middle altitudes
    lo, hi = L3["pt_off"][:-1], L3["pt_off"][1:] - 1
    alt_mid = 0.5 * (L3["alt"][(lo + hi) // 2] + L3["alt"][(lo + hi + 1) // 2])
    U, lit = G.solar_columns(z, nd, vmr, alt_mid, L3["seg_mu"], col_scale=[0.9, 1.0])
    assert U.shape == (len(layer), 2, 12) and np.all(U >= 0) and lit.all()
    assert np.all(U[np.arange(len(layer)), :, layer] > 0)             # the rest of the step's own shell
    up = np.flatnonzero(L3["seg_mu"] >= 0)
    assert up.size and all(np.all(U[r, :, :layer[r]] == 0) for r in up)   # the sun above the horizon: nothing below the step
    w = np.where(lit, 0.05, 0.0)
    emi, trans = eng.solar_source(Ad, U, w, sca, sund, src_row=layer, transmission=True)
    ref_e, ref_t, tau, K = R.reference(A.reshape(24, n_pts), U, w, A[1], sun, layer)
    assert float(tau.max()) > 0.01
    assert R.ratio(_np(emi), ref_e, R.bound_emi(ref_e, tau, K)) <= 1.0 and R.ratio(_np(trans), ref_t, R.bound_trans(ref_t, tau, K)) <= 1.0


def test_solar_pass_is_redone_for_new_vmrs_only(eng):
    scene = SC.solar_scene(eng)
    scene.coefficients()
    haze, ch4 = scene.gas("haze"), scene.gas("CH4")
    emi0, thermal0, ch4_0 = haze.coeffs[1], haze.thermal, ch4.coeffs
    scene.coefficients()
    assert haze.coeffs[1] is emi0                                                       # nothing moved: nothing redone
    ch4.add_clim(ch4.vmr * 1.2)
    scene.coefficients()
    assert haze.coeffs[1] is not emi0 and haze.thermal is thermal0 and ch4.coeffs is ch4_0   # the solar pass and nothing else
    assert float((haze.coeffs[1] - emi0).abs().max()) > 0.0
    scene.solar_frozen = True
    emi1 = haze.coeffs[1]
    ch4.add_clim(ch4.vmr * 1.2)
    scene.coefficients()
    assert haze.coeffs[1] is emi1


def test_state_jacobian_against_central_differences(eng):
    """Every column of inversion_state's first Jacobian on the line gas + sunlit haze scene, the solar rows frozen across
    the perturbed forward runs (what the Jacobians hold fixed): |K - FD(h/2)| <= 2 |FD(h) - FD(h/2)| + 1e-9 max|K|."""
    from spectrobot_amd import retrieval
    scene, pixels, bayes, _, sigma = SC.solar_twin(eng)
    bs = bayes()
    x0 = bs.param_vector().copy()
    _, _, _, b = retrieval.inversion_state(scene, copy.deepcopy(bs), pixels, max_it=1)
    K1 = np.array(b.jacobian)
    retrieval._state_into_gases(scene, bayes())      # back to the first guess
    scene.coefficients()                             # ... and its solar rows, which stay from here on
    scene.solar_frozen = True
    order = sorted(pixels, key=lambda p: p.limb_tg_alt)

    def forward(name, prof):
        scene.gas(name).add_clim(prof)
        return np.concatenate([y.spectrum for y in retrieval.radtrans(scene, order)])

    col_at = 0
    for name in ("CH4", "haze"):
        prof0 = bayes().sets[name].profile()
        masks = [np.asarray(par.maskgrid.mask, float) for par in bs.sets[name].set]
        for k in range(3):
            fd = []
            for h in (0.02 * x0[col_at], 0.01 * x0[col_at]):
                fd.append((forward(name, prof0 + h * masks[k]) - forward(name, prof0 - h * masks[k])) / (2.0 * h))
            col = K1[:, col_at]
            jm = np.abs(col).max()
            trunc, err = np.abs(fd[0] - fd[1]).max(), np.abs(col - fd[1]).max()
            print("\nsunlit twin FD, %s node %d: max|K| %.3e, |K - FD(h/2)| / max|K| %.2e, |FD(h) - FD(h/2)| / max|K| %.2e"
                  % (name, k, jm, err / jm, trunc / jm))
            assert jm > 0 and err <= 2.0 * trunc + 1e-9 * jm
            col_at += 1
        scene.gas(name).add_clim(prof0)
