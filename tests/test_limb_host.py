"""Host side of the limb and radiance entry points (no GPU): every refused call returns its status from the argument
checks, which all come before the first copy, launch or handle mutation.  The coefficient tables and outputs below are
not device memory: a call that got as far as a copy or a launch would not return a status of its own.  One table of
refused calls per entry point; the statuses are those the library has always answered, except the NULL `los` of
sr_limb_rays_jacobians_dev, which used to be dereferenced."""
import ctypes as C

import numpy as np
import pytest

from spectrobot_amd import _lib

ARG, LIMIT, UNSUPPORTED = _lib.SR_ERR_ARG, _lib.SR_ERR_LIMIT, _lib.SR_ERR_UNSUPPORTED
N_LAYERS, N_PTS, N_PAR = 4, 10, 2
FAKE = C.c_void_p(4096)    # stands for a device buffer: never dereferenced by a refused call
_SO, _SL, _PO = np.array([0, 2], np.int32), np.array([1, 3], np.int32), np.array([0, 2, 4], np.int32)
_X, _ONE = np.array([0.0, 1.0, 1.0, 2.0]), np.ones(8)
_SEG_COL = np.ones(2)
_PAR_W = np.ones((N_PAR, 4))
_DCOL = np.ones((N_PAR, 2))


def _los(seg_layer=_SL, init_mode=0):
    d = _lib.LosDesc()
    d.n_rays, d.n_gas, d.init_mode = 1, 2, init_mode
    d.seg_off, d.seg_layer, d.pt_off = (a.ctypes.data_as(_lib.ip) for a in (_SO, seg_layer, _PO))
    d.x, d.nd, d.vmr = (a.ctypes.data_as(_lib.dp) for a in (_X, _ONE, _ONE))
    return d


def _common(kw):
    """The arguments every entry point shares: tables, grid, LOS (None: a NULL pointer)."""
    tab = None if kw.get("no_tab") else FAKE
    seg_layer = np.ascontiguousarray(kw.get("seg_layer", _SL), dtype=np.int32)
    d = None if kw.get("no_los") else _los(seg_layer, kw.get("init_mode", 0))
    keep = (seg_layer, d)  # (alive until the call has returned)
    return tab, kw.get("n_pts", N_PTS), C.byref(d) if d is not None else None, keep


def _par_gas(kw):
    return np.ascontiguousarray(kw.get("par_gas", [0, 1]), dtype=np.int32)


def limb_rays(**kw):
    tab, n_pts, los, _keep = _common(kw)
    return _lib.lib.sr_limb_rays_dev(tab, tab, N_LAYERS, n_pts, los, None if kw.get("no_rad") else FAKE, None)


def limb_rays_jac(**kw):
    tab, n_pts, los, _keep = _common(kw)
    pg = _par_gas(kw)
    return _lib.lib.sr_limb_rays_jac_dev(tab, tab, N_LAYERS, n_pts, los, kw.get("n_par", N_PAR), pg.ctypes.data_as(_lib.ip),
                                         _PAR_W.ctypes.data_as(_lib.dp), FAKE, None if kw.get("no_jac") else FAKE, None)


def limb_rays_jac_layer(**kw):
    tab, n_pts, los, _keep = _common(kw)
    return _lib.lib.sr_limb_rays_jac_layer_dev(tab, tab, None if kw.get("no_dtab") else FAKE, FAKE, N_LAYERS, n_pts, los, FAKE,
                                               None)


def limb_rays_jacobians(**kw):
    """kinds: "layer", "par" or "both"."""
    tab, n_pts, los, _keep = _common(kw)
    kinds = kw.get("kinds", "both")
    lay = FAKE if kinds in ("layer", "both") else None
    n_par = N_PAR if kinds in ("par", "both") else 0
    pg = _par_gas(kw)
    return _lib.lib.sr_limb_rays_jacobians_dev(
        tab, tab, lay, lay, N_LAYERS, n_pts, los, None, 0, n_par, pg.ctypes.data_as(_lib.ip) if n_par else None,
        _PAR_W.ctypes.data_as(_lib.dp) if n_par else None, None if kw.get("no_rad") else FAKE, lay,
        FAKE if n_par else None, None)


def _segments(kw):
    seg_layer = np.ascontiguousarray(kw.get("seg_layer", _SL), dtype=np.int32)
    seg_off = np.ascontiguousarray(kw.get("seg_off", _SO), dtype=np.int32)
    return (None if kw.get("no_seg_off") else seg_off.ctypes.data_as(_lib.ip),
            None if kw.get("no_seg_layer") else seg_layer.ctypes.data_as(_lib.ip), _SEG_COL.ctypes.data_as(_lib.dp),
            (seg_layer, seg_off))


def radiance_rays(**kw):
    tab = None if kw.get("no_tab") else FAKE
    so, sl, sc, _keep = _segments(kw)
    return _lib.lib.sr_radiance_rays_dev(tab, tab, N_LAYERS, kw.get("n_pts", N_PTS), 1, so, sl, sc, 0,
                                         None if kw.get("no_rad") else FAKE, None)


def radiance_jac(**kw):
    tab = None if kw.get("no_tab") else FAKE
    so, sl, sc, _keep = _segments(kw)
    return _lib.lib.sr_radiance_jac_dev(tab, tab, N_LAYERS, kw.get("n_pts", N_PTS), 1, so, sl, sc,
                                        None if kw.get("no_dcol") else _DCOL.ctypes.data_as(_lib.dp), kw.get("n_par", N_PAR),
                                        FAKE, FAKE, None)


def radiance_jac_layer(**kw):
    tab = None if kw.get("no_tab") else FAKE
    so, sl, sc, _keep = _segments(kw)
    return _lib.lib.sr_radiance_jac_layer_dev(tab, tab, None if kw.get("no_dtab") else FAKE, FAKE, N_LAYERS,
                                              kw.get("n_pts", N_PTS), 1, so, sl, sc, FAKE, None)


# (every table: NULL tables, NULL los -- NULL seg_off for the calls that take the segment lists themselves --, n_pts 0 and
# 2 000 001, a seg_layer out of range on either side, par_gas out of range where there are parameters, init_mode 1
# where the call refuses it)
_GRID_AND_LOS = [(dict(no_tab=True), ARG), (dict(no_los=True), ARG), (dict(n_pts=0), ARG), (dict(n_pts=2000001), LIMIT),
                 (dict(seg_layer=[1, N_LAYERS]), ARG), (dict(seg_layer=[-1, 3]), ARG)]
_GRID_AND_SEGMENTS = [(dict(no_tab=True), ARG), (dict(no_seg_off=True), ARG), (dict(n_pts=0), ARG),
                      (dict(n_pts=2000001), LIMIT), (dict(seg_layer=[1, N_LAYERS]), ARG), (dict(seg_layer=[-1, 3]), ARG),
                      (dict(no_seg_layer=True), ARG), (dict(seg_off=[1, 2]), ARG)]
_PAR_GAS = [(dict(par_gas=[0, 2]), ARG), (dict(par_gas=[-1, 1]), ARG)]

REFUSED = {
    limb_rays: _GRID_AND_LOS + [(dict(no_rad=True), ARG)],
    limb_rays_jac: _GRID_AND_LOS + _PAR_GAS + [(dict(n_par=0), ARG), (dict(no_jac=True), ARG)],
    limb_rays_jac_layer: _GRID_AND_LOS + [(dict(init_mode=1), UNSUPPORTED), (dict(no_dtab=True), ARG)],
    limb_rays_jacobians: [(dict(k, kinds=kinds), st) for kinds in ("layer", "par", "both") for k, st in _GRID_AND_LOS] +
                         [(dict(k, kinds=kinds), st) for kinds in ("par", "both") for k, st in _PAR_GAS] +
                         [(dict(init_mode=1, kinds="layer"), UNSUPPORTED), (dict(init_mode=1, kinds="both"), UNSUPPORTED),
                          (dict(init_mode=1, kinds="par", no_rad=True), ARG)],
    radiance_rays: _GRID_AND_SEGMENTS + [(dict(no_rad=True), ARG)],
    radiance_jac: _GRID_AND_SEGMENTS + [(dict(n_par=0), ARG), (dict(no_dcol=True), ARG), (dict(seg_off=[0, 0]), ARG)],
    radiance_jac_layer: _GRID_AND_SEGMENTS + [(dict(no_dtab=True), ARG), (dict(seg_off=[0, 0]), ARG)],
}


@pytest.mark.parametrize("entry", list(REFUSED), ids=lambda f: f.__name__)
def test_refused_calls_return_their_status_before_any_device_call(entry):
    for kw, status in REFUSED[entry]:
        assert entry(**kw) == status, kw


def test_abi_surface_is_unchanged():
    assert _lib.lib.sr_abi_version() == 1
    for name in ("sr_limb_rays_dev", "sr_limb_rays_jac_dev", "sr_limb_rays_jac_layer_dev", "sr_limb_rays_jacobians_dev",
                 "sr_radiance_rays_dev", "sr_radiance_jac_dev", "sr_radiance_jac_layer_dev"):
        assert hasattr(_lib.lib, name)


# ------------------------------------------------------------------------------------------------------------------
# the key of a resident batch with parameters (engine.LimbLOS.handle_par, retrieval.Sun): an array's content
# ------------------------------------------------------------------------------------------------------------------
def _swapped(a, i, j):
    b = a.copy()
    flat = b.reshape(-1)
    flat[i], flat[j] = flat[j], flat[i]
    return b


def test_content_key_tells_two_words_that_change_places():
    """Tables above 4096 bytes are keyed by two reductions over their 64-bit words.  Elements 1 and 2 changing places
    (positions that shared a multiplier when position i was weighted by i | 1) and any two neighbours of a 6 x 90 table
    of weights give another key; so do x and -x side by side, which differ in the sign bit alone."""
    from spectrobot_amd import engine
    rng = np.random.default_rng(20261021)
    big = rng.uniform(0.0, 1.0, 1000)
    assert big.nbytes > 4096 and engine._content_key(big) == engine._content_key(big.copy())
    assert engine._content_key(_swapped(big, 1, 2)) != engine._content_key(big)
    W = rng.uniform(0.0, 1.0, (6, 90)) * (rng.random((6, 90)) < 0.7)
    assert W.nbytes > 4096
    key = engine._content_key(W)
    for i in range(W.size - 1):
        if W.reshape(-1)[i] != W.reshape(-1)[i + 1]:
            assert engine._content_key(_swapped(W, i, i + 1)) != key, i
    signs = np.tile([1.5, -1.5], 300)
    assert engine._content_key(_swapped(signs, 6, 7)) != engine._content_key(signs)
    assert engine._content_key(W.astype(np.float32).astype(np.float64)) != key and engine._content_key(W.reshape(90, 6)) != key


def test_array_key_takes_identity_only_for_an_array_that_owns_its_data():
    """A read-only array that owns its data cannot change under its identity; a read-only VIEW of a writable base can --
    it is keyed by content, and an edit through the base changes the key."""
    from spectrobot_amd import engine
    base = np.random.default_rng(5).uniform(0.0, 1.0, (6, 90))
    own = base.copy()
    own.setflags(write=False)
    assert engine._array_key(own) == ("id", id(own))
    view = base.view()
    view.setflags(write=False)
    assert view.base is base and not view.flags.writeable
    before = engine._array_key(view)
    assert before == engine._content_key(base) and before[0] != "id"
    base[0, 1], base[0, 2] = base[0, 2], base[0, 1]
    assert engine._array_key(view) != before
    part = own[1:]                        # a view of a read-only array: by content too (its base is not None)
    assert engine._array_key(part) == engine._content_key(part)
    assert engine._array_key(base) == engine._content_key(base) and engine._array_key([1, 2, 3]) == engine._content_key([1, 2, 3])
