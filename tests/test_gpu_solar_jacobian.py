"""The solar attenuation in the Jacobians on the GPU: sr_solar_jac_kernel through engine.solar_attenuation_jacobian
against the long-double definition of tests/solar_jacobian_reference.py inside its bound on the panel of tile, chunk, store
and ray-group edges (n_rows 1, 15, 17, 33 x n_k 1, 3, 5, 13, 160 x n_pts 1, 63, 65, 257, (n_rays, n_par) cycling through
(1, 1), (3, 2), (NR + 1, 5), (9, 17)), the exact cases, a second batch of chunks (n_k 259), every refusal, and the
composition it stands for: Q from engine.limb_rays_layer_jacobian, dU @ A and the row sum in torch."""
import ctypes as C

import numpy as np
import pytest

import solar_jacobian_reference as R

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
    return eng.solar_attenuation_jacobian(_dev(c["A"]), c["dU"], _dev(c["Q"]), **kw)


def _case(*key):
    """A panel case with its reference, made once and shared (read-only)."""
    if key not in _case.cache:
        c = R.panel_case(*key)
        c["jac"], c["b"] = R.reference(c["A"], c["dU"], c["Q"])
        for v in c.values():
            v.setflags(write=False)
        _case.cache[key] = c
    return _case.cache[key]


_case.cache = {}


@pytest.mark.parametrize("n_rows", R.N_ROWS)
def test_panel_inside_the_bound(eng, n_rows):
    worst, zeros = 0.0, 0
    for key in R.panel():
        if key[0] != n_rows:
            continue
        c = _case(*key)
        got = _np(_call(eng, c))
        worst = max(worst, R.ratio(got, c["jac"], c["b"]))
        zeros += int(np.count_nonzero(c["b"] == 0))
        if key[4] > 1:                               # the parameter without columns, the ray that sees no row: exact zeros
            assert np.all(got[:, 1] == 0.0)
        if key[3] > 1:
            assert np.all(got[1] == 0.0)
    print("\nsolar Jacobian panel, n_rows %d: |GPU - reference| / bound %.3f (%d elements with bound 0)" % (n_rows, worst, zeros))
    assert worst <= 1.0, worst


def test_exact_cases(eng):
    import torch
    c = _case(33, 160, 257, R.NR + 1, 5)
    n_rays, n_par, n_pts = R.NR + 1, 5, 257
    jac = _call(eng, c)
    # two calls: identical bits
    assert torch.equal(jac, _call(eng, c))
    # full chunk lists: the skipped chunks and tiles only add exact zeros
    off, ch = eng.solar_jacobian_chunk_lists(c["dU"])
    eng.set_solar_full_lists(True)
    try:
        jac_full = _call(eng, c)
        off_f, ch_f = eng.solar_jacobian_chunk_lists(c["dU"])
    finally:
        eng.set_solar_full_lists(False)
    assert torch.equal(jac, jac_full) and ch.size < ch_f.size
    # accumulate: overwrite plus base to one rounding; the parameter without columns keeps its bits (a NaN among them)
    base = torch.as_tensor(np.random.default_rng(5).uniform(-1e-8, 1e-8, (n_rays, n_par, n_pts)), device="cuda")
    base[0, 1, 3] = float("nan")
    acc = base.clone()
    out = _call(eng, c, out=acc, accumulate=True)
    assert out is acc
    a, b, j = _np(acc), _np(base), _np(jac)
    assert np.array_equal(a[:, 1].view(np.uint64), b[:, 1].view(np.uint64))
    rows = [0, 2, 3, 4]
    s = b[:, rows].astype(LD) + j[:, rows].astype(LD)
    assert np.all(np.abs(a[:, rows].astype(LD) - s) <= EPS * np.abs(s))
    total = b[:, rows].astype(LD) + c["jac"][:, rows]
    assert R.ratio(a[:, rows], total, R.bound_accumulated(c["b"][:, rows], total)) <= 1.0
    eng.set_solar_full_lists(True)                   # ... and the same bits with every chunk listed
    try:
        acc_full = _call(eng, c, out=base.clone(), accumulate=True)
    finally:
        eng.set_solar_full_lists(False)
    assert np.array_equal(_np(acc_full).view(np.uint64), a.view(np.uint64))
    # par_slot places the rows; the rows that are not named keep their bits
    slots = np.array([6, 0, 3, 1, 4])
    wide = torch.full((n_rays, 8, n_pts), -7.0, dtype=torch.float64, device="cuda")
    _call(eng, c, out=wide, par_slot=slots)
    w = _np(wide)
    assert np.array_equal(w[:, slots].view(np.uint64), j.view(np.uint64))
    assert np.all(w[:, [2, 5, 7]] == -7.0)


def test_a_second_batch_of_chunks(eng):
    """n_k = 259 is 65 chunks: with every chunk listed a tile walks one whole batch of 64 through LDS, then a batch of one
    chunk padded to a pair, the last chunk of three k -- on 17 rows (a second row tile of one row), 65 points (a partial
    quad), NR + 1 rays and two parameters.  Overwrite and accumulate, each inside the bound with full lists and bit for bit
    the sparse-list call."""
    import torch
    key = (17, 259, 65, R.NR + 1, 2)
    c = _case(*key)
    base = np.random.default_rng(5).uniform(-1e-8, 1e-8, (R.NR + 1, 2, 65))
    both = lambda: (_call(eng, c), _call(eng, c, out=_dev(base), accumulate=True))
    sparse = both()
    eng.set_solar_full_lists(True)
    try:
        full = both()
        off_f, ch_f = eng.solar_jacobian_chunk_lists(c["dU"])
    finally:
        eng.set_solar_full_lists(False)
    assert list(np.diff(off_f)) == [65] * 4 and ch_f[64] == 64            # (a second batch in every tile of both parameters)
    jac, acc = (_np(x) for x in full)
    assert R.ratio(jac, c["jac"], c["b"]) <= 1.0
    total = base.astype(LD) + c["jac"]
    assert R.ratio(acc, total, R.bound_accumulated(c["b"], total)) <= 1.0
    for x, y in zip(sparse, full):
        assert torch.equal(x, y)


def test_every_refusal_leaves_jac_untouched(eng):
    import torch
    from spectrobot_amd import _lib
    lib, dp, ip = _lib.lib, _lib.dp, _lib.ip
    key = (17, 5, 65, 3, 2)
    c = _case(*key)
    n_rows, n_k, n_pts, n_rays, n_par = key
    A, Q = _dev(c["A"]), _dev(c["Q"])
    jac = torch.full((n_rays, 3, n_pts), -7.0, dtype=torch.float64, device="cuda")
    dU, slot = np.array(c["dU"]), np.array([2, 0], np.int32)
    good = dict(du=dU, n_par=n_par, n_rows=n_rows, A=A, n_k=n_k, q=Q, n_rays=n_rays, n_pts=n_pts, slot=slot, jac=jac, n_jac=3, desc=True)
    ptr = lambda t: None if t is None else C.c_void_p(t.data_ptr())

    def call(**kw):
        a = dict(good, **kw)
        d = _lib.SolarJacDesc()
        d.n_par, d.n_rows = a["n_par"], a["n_rows"]
        d.du = None if a["du"] is None else a["du"].ctypes.data_as(dp)
        return lib.sr_solar_jacobian_rows_dev(C.byref(d) if a["desc"] else None, ptr(a["A"]), a["n_k"], ptr(a["q"]), a["n_rays"],
                                              a["n_pts"], None if a["slot"] is None else a["slot"].ctypes.data_as(ip), ptr(a["jac"]),
                                              a["n_jac"], 0, None)

    def edited(arr, at, v):
        out = arr.copy()
        out[at] = v
        return out

    assert call() == 0
    torch.cuda.synchronize()
    first = jac.clone()
    assert bool((first[:, 1] == -7.0).all()) and R.ratio(_np(first[:, [2, 0]]), c["jac"], c["b"]) <= 1.0
    jac.fill_(-7.0)
    ARG, LIMIT = _lib.SR_ERR_ARG, _lib.SR_ERR_LIMIT
    cases = [("null desc", dict(desc=False), ARG), ("null du", dict(du=None), ARG), ("null tab_abs", dict(A=None), ARG),
             ("null q", dict(q=None), ARG), ("null par_slot", dict(slot=None), ARG), ("null jac", dict(jac=None), ARG),
             ("n_par 0", dict(n_par=0), ARG), ("n_rows 0", dict(n_rows=0), ARG), ("n_k 0", dict(n_k=0), ARG),
             ("n_rays 0", dict(n_rays=0), ARG), ("n_pts 0", dict(n_pts=0), ARG), ("n_jac_rows 0", dict(n_jac=0), ARG),
             ("du nan", dict(du=edited(dU, (0, 0, 0), np.nan)), ARG), ("du inf", dict(du=edited(dU, (1, 16, 4), np.inf)), ARG),
             ("par_slot too large", dict(slot=edited(slot, 1, 3)), ARG), ("par_slot negative", dict(slot=edited(slot, 0, -1)), ARG),
             ("par_slot repeated", dict(slot=edited(slot, 1, 2)), ARG), ("n_pts beyond the limit", dict(n_pts=2000001), LIMIT),
             ("n_rows beyond the limit", dict(n_rows=_lib.SR_MAX_ABS_ROWS + 1), LIMIT)]
    for what, kw, status in cases:
        assert call(**kw) == status, what
    big = np.zeros((2, 2048, 2049))                  # n_par n_rows n_k beyond SR_MAX_SOLAR_VALUES
    assert call(du=big, n_par=2, n_rows=2048, n_k=2049) == LIMIT
    torch.cuda.synchronize()
    assert bool((jac == -7.0).all())
    # a valid call afterwards: bit for bit the earlier one
    assert call() == 0
    torch.cuda.synchronize()
    assert torch.equal(jac, first)
    # the host layer's own refusals
    with pytest.raises(ValueError):
        eng.solar_attenuation_jacobian(A, dU, Q, accumulate=True)
    with pytest.raises(ValueError):
        eng.solar_attenuation_jacobian(A, dU[:, :, :4], Q)
    with pytest.raises(ValueError):
        eng.solar_attenuation_jacobian(A, dU, Q[:, :-1].contiguous())
    with pytest.raises(ValueError):
        eng.solar_attenuation_jacobian(A, dU, Q, par_slot=[0, 1])
    with pytest.raises(ValueError):
        eng.solar_attenuation_jacobian(A, dU, Q, out=jac[:, :, :-1].contiguous())


def test_composition_with_the_layer_jacobian(eng):
    """Q as the driver makes it -- limb_rays_layer_jacobian with dabs = 0 and demi = the solar rows -- then the fused
    call against dU @ A and the row sum in torch, within 2 b (b from the Q the GPU made, taken as exact)."""
    import torch
    from spectrobot_amd import geometry as G
    rng = np.random.default_rng(17)
    z = np.linspace(100.0, 540.0, 12)
    nd = 3e17 * np.exp(-(z - 100.0) / 63.0)
    vmr = np.array([np.full(12, 1e-2), 1e-3 * (1.0 + (z - 100.0) / 500.0)])
    zz = np.append(z, 2 * z[-1] - z[-2])
    n_pts = 130
    A = rng.uniform(1e-22, 1e-21, (2, 12, n_pts))
    emi = rng.uniform(1e-30, 1e-29, (2, 12, n_pts))
    sol = np.zeros_like(emi)
    sol[1] = rng.uniform(1e-30, 1e-29, (12, n_pts))
    L = G.limb_los(z, nd, vmr, [130.0, 260.0, 410.0])
    los = eng.LimbLOS(L["seg_off"], L["seg_layer"], L["pt_off"], L["x"], L["nd"], L["vmr"])
    co = (_dev(A), _dev(emi + sol))
    Q = eng.limb_rays_layer_jacobian(co, (_dev(np.zeros_like(A)), _dev(sol)), los)
    masks = np.array([np.clip(1.0 - np.abs(z - zc) / 120.0, 0.0, None) for zc in (150.0, 300.0, 450.0)] * 2)
    masks[4] *= -1.0
    par_gas = [0, 0, 0, 1, 1, 1]
    dU, lit = G.solar_column_weights(z, nd, masks, par_gas, 2, 0.5 * (zz[:-1] + zz[1:]), float(np.cos(np.deg2rad(75.0))))
    assert lit.all() and dU.shape == (6, 12, 2, 12)
    fused = eng.solar_attenuation_jacobian(co[0], dU, Q)
    dtau = _dev(dU.reshape(6, 12, 24)) @ co[0].reshape(24, n_pts)                  # [n_par, n_rows, n_pts]
    composed = -(Q[:, None] * dtau[None]).sum(dim=2)
    ref, b = R.reference(A.reshape(24, n_pts), dU, _np(Q))
    assert float(np.abs(ref).max()) > 0
    print("\nfused against composed: |difference| / 2 b %.3f; fused against the reference / b %.3f"
          % (R.ratio(_np(fused) - _np(composed), np.zeros(ref.shape, LD), 2 * b), R.ratio(_np(fused), ref, b)))
    assert R.ratio(_np(fused) - _np(composed), np.zeros(ref.shape, LD), 2 * b) <= 1.0
    assert R.ratio(_np(fused), ref, b) <= 1.0
