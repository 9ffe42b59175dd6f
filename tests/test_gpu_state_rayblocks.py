"""Parameter blocks PER RAY in the mixed-state pass (sr_set_state_ray_blocks, ray_blocks= of engine.limb_rays_state_jacobian
and limb_rays_state_bands): every ray is walked once per block of the parameters that touch IT, not once per block of
the batch's list.  On the batches of tests/state_rayblocks_cases.py -- 300 points, 3 gases, 12 rows, 6 limb rays, 37
parameters of which ray 0 touches none, ray 1 sixteen, ray 2 seventeen, ray 3 five; a batch for the eight-slot instances;
a batch with a coefficient row per LOS step --:
 1. the route getter reports the plan that ran and the walk count is the plan's, restated in numpy;
 2. rows of (ray, parameter) pairs that do not touch are exact zeros, in spectra and in bands;
 3. radiances and touched rows against the extended-precision recursion of tests/limb_reference.py, within
    KERNEL_MARGIN x K_PLAIN_RAD / K_PLAIN_JAC units -- the limit tests/test_gpu_limb_reference.py holds the dense kernel to;
 4. the per-ray route against the dense route of the same call, in the same units, held to the same limit (equal bits are
    expected and reported, not required: two template instances may contract differently);
 5. bands: per ray against dense at the bound tests/test_gpu_state_bands.py holds between its two routes.
Measured on an MI355X (2026-10-19): see the figures in the docstrings below."""
import functools

import numpy as np
import pytest

import limb_reference as R
import state_rayblocks_cases as B
from test_gpu_state_bands import BOUND

pytestmark = pytest.mark.gpu
LIM_RAD, LIM_JAC = R.KERNEL_MARGIN * R.K_PLAIN_RAD, R.KERNEL_MARGIN * R.K_PLAIN_JAC


@pytest.fixture(scope="module")
def eng():
    import torch
    assert torch.cuda.is_available(), "these tests need the GPU"
    from spectrobot_amd import engine
    engine.set_device(0)
    yield engine
    engine.set_state_ray_blocks(False)


def _t(v):
    import torch
    return torch.tensor(np.ascontiguousarray(v, dtype=np.float64), device="cuda")


def _np(t):
    return t.detach().cpu().numpy()


@functools.lru_cache(maxsize=None)
def _data(name):
    if name == "main":
        return B.main_case(21, 10, 6)
    if name == "two level gases":
        return B.main_case(21, 10, 6, n_lgas=2)
    if name == "eight slots":
        return B.small_case()
    assert name == "row per step"
    return B.step_rows_case()


@functools.lru_cache(maxsize=None)
def _at(name):
    """Panel column of every point (the first tile is the panel in its own order)."""
    return R.tile_columns(len(_data(name)["names"]), B.N_PTS, np.random.default_rng([B.SEED, len(name)]))


def _subset(c, kinds):
    """The case with the kinds of parameters named in `kinds` ("c", "l", "r") only: a view of the same batch."""
    s = dict(c)
    if "c" not in kinds:
        s["n_col"] = 0
    if "l" not in kinds:
        s["n_lev"] = 0
    if "r" not in kinds:
        s["n_row"] = 0
    return s


def _kw(c, at):
    """The parameters of a case as limb_rays_state_jacobian / limb_rays_state_bands take them."""
    kw = {}
    pick = lambda a: _t(a[..., at])
    if c["n_col"]:
        kw.update(par_gas=c["par_gas"][:c["n_col"]], par_w=c["par_w"][:c["n_col"]])
    if c["n_lev"]:
        kw.update(par_level=c["par_level"][:c["n_lev"]], par_c=c["par_c"][:c["n_lev"]])
        if c["n_lgas"] > 1:
            kw.update(level_gases=[(g, pick(t), cr) for g, t, cr in zip(c["lgas_gas"], c["tabs"], c["coef_rows"])],
                      par_lgas=c["par_lgas"][:c["n_lev"]])
        else:
            kw.update(tab=pick(c["tabs"][0]), coef_row=c["coef_rows"][0], gas=c["lgas_gas"][0])
    if c["n_row"]:
        kw.update(dcoeffs=(pick(c["dabs"]), pick(c["demi"])), par_t=c["par_t"][:c["n_row"]])
    return kw


def _los(eng, c, **opts):
    return eng.LimbLOS(c["seg_off"], c["seg_layer"], c["pt_off"], c["x"], c["nd"], c["vmr"], **opts)


def _columns(eng, c):
    """The device's Curtis-Godson columns of the gases and of the column parameters' weights: the reference's fp64 inputs."""
    los = _los(eng, c)
    col = los.columns()
    los.close()
    dcol = np.zeros((c["n_col"], c["seg_layer"].size))
    for p0 in range(0, c["n_col"], 4):
        w = eng.LimbLOS(c["seg_off"], c["seg_layer"], c["pt_off"], c["x"], c["nd"], c["par_w"][p0:p0 + 4])
        dcol[p0:p0 + 4] = w.columns()
        w.close()
    return col, dcol


# name -> (data, kinds, LimbLOS options, pointing)
SPECTRA = {
    "columns": ("main", "c", {}, False),
    "columns + levels": ("main", "cl", {}, False),
    "all kinds": ("main", "clr", {}, False),
    "two level gases": ("two level gases", "clr", {}, False),
    "solo absorption": ("main", "clr", dict(solo_absorption=True, initial_temperature=250.0), False),
    "planck": ("main", "clr", dict(initial_temperature=180.0), False),
    "observer": ("main", "clr", dict(LOS_order="observer"), False),
    "row per step": ("row per step", "clr", {}, False),
    "eight slots": ("eight slots", "clr", {}, False),
}


@pytest.mark.parametrize("name", list(SPECTRA))
def test_spectra_per_ray_against_dense_and_the_reference(eng, name):
    """Items 1 - 4 for the calls that return spectra.  The reference is formed for the parameters that touch a ray (the
    others are asserted to be exact zeros): tau, E, dtau, dE from the call's own inputs in long double, the columns as the
    device integrates them.  Every figure is printed before anything is asserted.
    MI355X (2026-10-19): against the reference at most 24.9 units in the radiances (solo absorption) and 28 in the
    Jacobians (Planck background), 5.7 / 11.6 in the other cases, of limits 328 / 200; per ray against dense 0 units in
    the radiances and the Jacobians of every case: equal bits."""
    import torch
    from spectrobot_amd import synthetic as syn
    data, kinds, opts, _ = SPECTRA[name]
    c, at = _subset(_data(data), kinds), _at(data)
    N = len(c["names"])
    solo, planck, observer = bool(opts.get("solo_absorption")), "initial_temperature" in opts, opts.get("LOS_order") == "observer"
    grid = syn.make_grid(2975.0, 5e-4, B.N_PTS) if planck else None
    coeffs = (_t(c["coef_a"][..., at]), _t(c["coef_e"][..., at]))
    kw = _kw(c, at)
    col, dcol = _columns(eng, c)
    los = _los(eng, c, **opts)
    try:
        I0, cols = np.zeros(N), at
        if planck:
            zero = torch.zeros_like(coeffs[0])
            I0 = _np(eng.limb_rays((zero, zero), los, grid=grid, resident=False))[0][:N]
            assert np.all(I0 > 0)
            cols = at[:N]
        rad_d, jac_d = eng.limb_rays_state_jacobian(coeffs, los, grid=grid, ray_blocks=False, **kw)
        route_d = eng.last_state_route()
        rad_r, jac_r = eng.limb_rays_state_jacobian(coeffs, los, grid=grid, ray_blocks=True, **kw)
        route_r = eng.last_state_route()
        eng.limb_rays_state_jacobian(coeffs, los, grid=grid, **kw)          # the keyword restored the default
        route_0 = eng.last_state_route()
    finally:
        los.close()
    n_p, n_walks, n_dense = B.walks(c)
    T = B.touches(c)
    n_par = T.shape[1]
    print("\nray blocks [%s]: %d parameters, touched per ray %s; NP %d, walks %d (dense %d); routes dense %s per ray %s"
          % (name, n_par, T.sum(axis=1).tolist(), n_p, n_walks, n_dense, route_d, route_r))
    same_bits = torch.equal(jac_d, jac_r) and torch.equal(rad_d, rad_r)
    rad_d, jac_d, rad_r, jac_r = (_np(v)[..., :len(cols)] for v in (rad_d, jac_d, rad_r, jac_r))
    worst = dict(rad=(0.0, "-"), jac=(0.0, "-"), rad_dr=(0.0, "-"), jac_dr=(0.0, "-"))
    for ray in range(T.shape[0]):
        par = np.flatnonzero(T[ray])
        forms = B.ray_forms(c, col, dcol, ray, R.LD, observer)
        ref = R.recursion_reference(forms[0], forms[1], forms[2][par], forms[3][par], I0, solo=solo, thin_ulps=c["n_gas"] + 1)
        sel = lambda k: ref[k][..., cols]
        u = dict(rad=R.units(rad_r[ray], sel("I"), sel("A_I"), sel("C_I"), c["n_gas"]),
                 rad_dr=R.units(rad_r[ray], rad_d[ray], sel("A_I"), sel("C_I"), c["n_gas"]))
        if par.size:
            u["jac"] = R.units(jac_r[ray, par], sel("J"), sel("A"), sel("C"), c["n_gas"])
            u["jac_dr"] = R.units(jac_r[ray, par], jac_d[ray, par], sel("A"), sel("C"), c["n_gas"])
        for k, v in u.items():
            w = R.worst(v, c["names"], cols)
            worst[k] = max(worst[k], (w[0], "ray %d, %s" % (ray, w[1])))
    print("  against the reference: rad %.3g units at %s; jac %.3g units at %s (limits %.3g, %.3g)"
          % (worst["rad"] + worst["jac"] + (LIM_RAD, LIM_JAC)))
    print("  per ray against dense: rad %.3g units, jac %.3g units at %s; equal bits: %s"
          % (worst["rad_dr"][0], worst["jac_dr"][0], worst["jac_dr"][1], same_bits))
    # 1: the routes and the walks
    assert route_d == (1, n_dense) and route_r == (2, n_walks) and route_0 == route_d
    if data == "main" and kinds == "clr":
        assert tuple(T.sum(axis=1)) == B.TARGET and n_par == 37 and n_dense == 18
    if data != "eight slots":
        assert n_walks < n_dense
    else:
        assert n_p == 8
    # 2: exact zeros where nothing touches, on both routes
    assert not jac_r[~T].any() and not jac_d[~T].any()
    assert np.all(np.abs(jac_r[T]).max(axis=-1) > 0)
    # 3, 4
    assert worst["rad"][0] <= LIM_RAD and worst["jac"][0] <= LIM_JAC
    assert worst["rad_dr"][0] <= LIM_RAD and worst["jac_dr"][0] <= LIM_JAC


def _path(c, rng):
    """Path arrays of a synthetic batch: altitudes that differ between a segment's two sample points, derivatives of O(1)."""
    n_pt = c["x"].size
    return dict(alt=100.0 + 3.0 * np.arange(n_pt)[::-1] + rng.uniform(0.0, 1.0, n_pt), dx=rng.uniform(0.5, 1.5, n_pt),
                dalt=rng.uniform(0.5, 1.0, n_pt))


def test_pointing_rows_exist_for_every_ray(eng):
    """pointing=True: the hidden per-gas slots touch every ray, so every ray -- ray 0 too, which touches no parameter --
    carries them in its block 0 and the pointing row behind the state's rows is that of the dense route; the walks count
    the three hidden slots.  The state rows against the dense route in the reference's units would repeat the test above:
    here rows are compared per (ray, row) relative to the row's largest value, bound 1e-12 (equal bits expected)."""
    import torch
    c, at = _data("main"), _at("main")
    coeffs = (_t(c["coef_a"][..., at]), _t(c["coef_e"][..., at]))
    los = _los(eng, c, path=_path(c, np.random.default_rng([B.SEED, 5])))
    try:
        _, jac_d = eng.limb_rays_state_jacobian(coeffs, los, pointing=True, ray_blocks=False, **_kw(c, at))
        route_d = eng.last_state_route()
        _, jac_r = eng.limb_rays_state_jacobian(coeffs, los, pointing=True, ray_blocks=True, **_kw(c, at))
        route_r = eng.last_state_route()
    finally:
        los.close()
    n_p, n_walks, n_dense = B.walks(c, n_hid=3)
    T = B.touches(c)
    scale = jac_d.abs().amax(dim=-1)
    err = ((jac_r - jac_d).abs().amax(dim=-1) / scale.masked_fill(scale == 0, 1.0)).max()
    print("\nray blocks [pointing]: walks %d (dense %d), routes %s %s; per ray against dense %.2e of a row's largest value; equal bits %s"
          % (n_walks, n_dense, route_d, route_r, float(err), torch.equal(jac_r, jac_d)))
    assert tuple(jac_r.shape) == (6, 38, B.N_PTS)
    assert route_d == (1, n_dense) and route_r == (2, n_walks) and n_walks < n_dense
    assert bool((jac_r[:, 37].abs().amax(dim=-1) > 0).all())              # the pointing row of every ray
    assert not _np(jac_r[:, :37])[~T].any() and not _np(jac_d[:, :37])[~T].any()
    assert float(err) <= 1e-12


BANDS = {
    "bands": ("main", {}, False, False, 0),
    "bands, field of view": ("main", {}, False, True, 0),
    "bands, instrument rows": ("main", {}, True, False, 0),
    "bands, instrument rows, field of view, Planck": ("main", dict(initial_temperature=200.0), True, True, 0),
    "bands, two level gases": ("two level gases", {}, False, False, 0),
    "bands, eight slots, instrument rows": ("eight slots", {}, True, False, 0),
    "bands, spectral shard": ("main", {}, False, False, 57),
    "bands, row per step": ("row per step", {}, False, False, 0),
}


@pytest.mark.parametrize("name", list(BANDS))
def test_bands_per_ray_against_dense(eng, name):
    """Items 1, 2 and 5 for the bands calls: the per-ray call against the dense call within BOUND (1e-12) of a quantity
    row's largest element over rays and bands -- the bound of tests/test_gpu_state_bands.py --, rows that do not touch
    exact zeros (without the field of view, which mixes a pixel's three rays: there a row is zero where none of the three
    touches), the instrument rows present for every ray.  A spectral shard (g_lo = 57 on a grid of 400 points) gives its
    partial integrals on both routes.
    MI355X (2026-10-19): per ray against dense 0.0 in all eight cases, equal bits."""
    from spectrobot_amd import synthetic as syn
    data, opts, instrument, with_fov, g_lo = BANDS[name]
    c, at = _data(data), _at(data)
    n_grid = B.N_PTS + (100 if g_lo else 0)
    grid = syn.make_grid(2975.0, 5e-4, n_grid)
    lam_lo, lam_hi = 1e7 / grid[-1], 1e7 / grid[0]
    span = lam_hi - lam_lo
    rng = np.random.default_rng([B.SEED, 9])
    bands = np.concatenate([[lam_lo - 50 * span - 1.0, 0.5 * (lam_lo + lam_hi)], lam_lo + span * rng.uniform(0.02, 0.98, 17)])
    widths = np.concatenate([[0.05 * span, 3.0 * span], span * rng.uniform(0.003, 0.2, 17)])          # 19 bands: two tiles
    coeffs = (_t(c["coef_a"][..., at]), _t(c["coef_e"][..., at]))
    fov = eng.fov_factors([0.0, 20.0][:len(c["seg_off"]) // 3]) if with_fov else None
    los = _los(eng, c, **opts)
    try:
        call = lambda rb: eng.limb_rays_state_bands(coeffs, los, grid, bands, widths, fov=fov, g_lo=g_lo, instrument=instrument,
                                                    ray_blocks=rb, **_kw(c, at))
        dense = call(False)
        route_d = eng.last_state_route()
        per_ray = call(True)
        route_r = eng.last_state_route()
    finally:
        los.close()
    n_p, n_walks, n_dense = B.walks(c)
    T = B.touches(c)
    n_par = T.shape[1]
    scale = np.max(np.abs(dense), axis=(0, 2), keepdims=True)
    dist = float(np.max(np.abs(per_ray - dense) / np.where(scale > 0, scale, 1.0)))
    print("\nray blocks [%s]: walks %d (dense %d), routes %s %s; per ray against dense %.2e of a row's largest element (bound %.0e); "
          "equal bits: %s" % (name, n_walks, n_dense, route_d, route_r, dist, BOUND, np.array_equal(per_ray, dense)))
    assert per_ray.shape == dense.shape == (T.shape[0] // (3 if with_fov else 1), 1 + n_par + (2 if instrument else 0), 19)
    assert np.all(np.isfinite(per_ray)) and route_d == (1, n_dense) and route_r == (2, n_walks)
    if with_fov:
        T = T.reshape(-1, 3, n_par).any(axis=1)
    assert not per_ray[:, 1:1 + n_par][~T].any() and not dense[:, 1:1 + n_par][~T].any()
    assert np.all(np.abs(per_ray[:, 1:1 + n_par][T]).max(axis=-1) > 0)
    assert not per_ray[:, :, 0].any()                                     # the band outside the grid
    if instrument:
        assert np.all(np.abs(per_ray[:, 1 + n_par:]).max(axis=-1) > 0)    # of every ray, the one without parameters too
    assert dist <= BOUND
