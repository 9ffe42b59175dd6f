"""The pointing derivative on the GPU (sr_los_columns_dz, sr_limb_rays_jac_state_path_dev,
sr_limb_rays_state_bands_path_dev; engine.los_columns_dz and pointing=True on the mixed-state calls): d I / d z_t of every
limb ray's own tangent altitude, the crossed shells held fixed, on the case set of tests/pointing_reference.py (five rays
through nine levels: mid-shell, just above a level, 1 km below a level, the top shell).

1. The column kernel against the extended-precision d col / d z_t, within 8 x the plain fp64 yardstick's distance on the
   same inputs.
2. The spectra route against limb_reference.recursion_reference with one parameter per gas (dtau, dE from the device's own
   d col, which 1. holds): the pointing row within KERNEL_MARGIN x K_PLAIN_JAC units of the SUM over the gases of the
   per-row bounds; the state rows and the radiance bitwise those of the call without pointing.
3. The bands route against the extended-precision band integrals (tests/lowres_reference.py) of the spectra route's
   pointing row, with and without the field of view and the instrument rows; every other row bitwise that of the fused
   call without pointing.
4. End to end against central differences of engine.limb_rays on rebuilt batches.
5. Refusals leave the outputs untouched.
Needs a real MI355X."""
import numpy as np
import pytest

import limb_reference as R
import lowres_reference as B
import pointing_reference as P

pytestmark = pytest.mark.gpu
SEED = 20261019
COL_SCALE = [0.98827, 1.0, 0.5, 1.0]
N_LEVELS, N_TAB_ROWS = 4, 5
ROTS = [0.0, 20.0]
N_LAYERS = len(P.LEVELS)                  # one coefficient row per shell, the top shell included


@pytest.fixture(scope="module")
def eng():
    import torch
    assert torch.cuda.is_available(), "these tests need the GPU"
    from spectrobot_amd import engine
    engine.set_device(0)
    return engine


def _t(v):
    import torch
    return torch.tensor(np.ascontiguousarray(v, dtype=np.float64), device="cuda")


def coefficients(n_gas, n_pts, seed=0):
    """abs 10^U(-21, -17) cm^2 (segment optical depths from thin to about 30 with the case set's columns), emi = abs x
    U(1e-8, 1e-7), [n_gas, N_LAYERS, n_pts]."""
    rng = np.random.default_rng([SEED, n_gas, n_pts, seed])
    a = 10.0 ** rng.uniform(-21.0, -17.0, (n_gas, N_LAYERS, n_pts))
    return a, a * rng.uniform(1e-8, 1e-7, a.shape)


def _batch(eng, n_gas, z_tans=P.Z_TANS, **opts):
    los, path, rays = P.batch_inputs(z_tans, n_gas)
    return eng.LimbLOS(los["seg_off"], los["seg_layer"], los["pt_off"], los["x"], los["nd"], los["vmr"],
                       col_scale=COL_SCALE[:n_gas], path=path, **opts), los, path, rays


def ray_forms(a, e, lay, u, du, dtype):
    """tau, E [S, N] and dtau, dE [n_gas, S, N] of one ray in `dtype`: one parameter per gas, gas g's column moving by
    du[g] (its d col / d z_t)."""
    tau, E = R.products(a[:, lay], u, dtype), R.products(e[:, lay], u, dtype)
    dtau = np.array([np.asarray(a[g, lay], dtype) * np.asarray(du[g], dtype)[:, None] for g in range(a.shape[0])])
    dE = np.array([np.asarray(e[g, lay], dtype) * np.asarray(du[g], dtype)[:, None] for g in range(a.shape[0])])
    return tau, E, dtau, dE


# ------------------------------------------------------------------------------------------------------------------
# 1. the column kernel
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_gas", [1, 2, 4])
def test_column_kernel_against_the_reference(eng, n_gas):
    los, arrays, path, rays = _batch(eng, n_gas)
    got = eng.los_columns_dz(los)
    assert got.shape == (n_gas, los.n_seg)
    scale = np.asarray(COL_SCALE[:n_gas])
    k_plain, figures = 0.0, []
    for r, G in enumerate(rays):
        seg = slice(arrays["seg_off"][r], arrays["seg_off"][r + 1])
        pts = slice(arrays["pt_off"][seg.start], arrays["pt_off"][seg.stop])
        shape = G["x"].shape
        F = dict(x=arrays["x"][pts].reshape(shape), nd=arrays["nd"][pts].reshape(shape),
                 vmr=arrays["vmr"][:, pts].reshape((n_gas,) + shape), alt=path["alt"][pts].reshape(shape),
                 dx=path["dx"][pts].reshape(shape), dalt=path["dalt"][pts].reshape(shape))
        ref = P.dcol_reference(G) * scale.astype(P.LD)[:, None]
        plain = scale[:, None] * P.dcol_forward(F["x"], F["nd"], F["vmr"], F["alt"], F["dx"], F["dalt"], np.float64)
        k_plain = max(k_plain, float(P.dist(plain, ref).max()))
        figures.append((P.Z_TANS[r], P.dist(got[:, seg], ref)))
    limit = P.KERNEL_MARGIN * k_plain
    print("\nd col / d z_t, %d gases: yardstick on these inputs %.3g (recorded K_PLAIN_DCOL %.3g), limit %.3g"
          % (n_gas, k_plain, P.K_PLAIN_DCOL, limit))
    for zt, d in figures:
        print("  z_t %7.2f km: kernel against the reference, per gas %s" % (zt, d))
    assert k_plain <= P.K_PLAIN_DCOL
    assert all(np.all(d <= limit) for _, d in figures), (figures, limit)


def test_column_kernel_exact_zero_and_flat_segments(eng):
    """Path derivatives of zero: an exact 0.0 in every segment.  A segment whose first and last altitude coincide takes
    zero slopes: finite, and equal to the plain fp64 statement's value to its rounding."""
    _, arrays, path, rays = _batch(eng, 2)
    mk = lambda p: eng.LimbLOS(arrays["seg_off"], arrays["seg_layer"], arrays["pt_off"], arrays["x"], arrays["nd"], arrays["vmr"], path=p)
    zero = np.zeros_like(path["dx"])
    assert np.all(eng.los_columns_dz(mk(dict(alt=path["alt"], dx=zero, dalt=zero))) == 0.0)
    flat = path["alt"].copy()
    flat[:P.N_SUB + 1] = flat[0]
    got = eng.los_columns_dz(mk(dict(alt=flat, dx=path["dx"], dalt=path["dalt"])))
    assert np.all(np.isfinite(got))
    shape = rays[0]["x"].shape
    n0 = shape[0] * shape[1]
    want = P.dcol_forward(arrays["x"][:n0].reshape(shape), arrays["nd"][:n0].reshape(shape), arrays["vmr"][:, :n0].reshape((2,) + shape),
                          flat[:n0].reshape(shape), path["dx"][:n0].reshape(shape), path["dalt"][:n0].reshape(shape), np.float64)
    assert np.allclose(got[:, 0], want[:, 0], rtol=1e-12, atol=0.0)


# ------------------------------------------------------------------------------------------------------------------
# 2. the spectra route
# ------------------------------------------------------------------------------------------------------------------
def _state_kw(n_gas, n_col, n_lev, n_row, alt, a, e, n_pts):
    """The other kinds of parameter beside the pointing: column masks on the sample altitudes, level parameters on pair
    tables and row parameters on derivative spectra with zeros among their weights (the builders of
    tests/test_gpu_state_bands.py and tests/state_rows_cases.py at this batch's shapes)."""
    rng = np.random.default_rng([SEED, n_gas, n_col, n_lev, n_row])
    kw = {}
    if n_col:
        nodes = np.linspace(P.LEVELS[0], P.LEVELS[-1], max(n_col, 2))[:n_col]
        kw["par_w"] = np.array([np.clip(1.0 - np.abs(alt - q) / 120.0, 0.0, None) + 0.05 for q in nodes])
        kw["par_gas"] = (np.arange(n_col) % n_gas).astype(np.int32)
    if n_lev:
        tab = 10.0 ** rng.uniform(-21.0, -18.0, (N_LEVELS, 2, N_TAB_ROWS, n_pts))
        tab[:, 1] *= rng.uniform(1e-8, 1e-7, tab[:, 1].shape)
        kw.update(tab=_t(tab), coef_row=(np.arange(N_LAYERS) // 2).astype(np.int32), gas=n_gas - 1,
                  par_c=rng.uniform(0.2, 1.0, (n_lev, N_LAYERS)) * (rng.random((n_lev, N_LAYERS)) < 0.6),
                  par_level=rng.integers(0, N_LEVELS, n_lev).astype(np.int32))
    if n_row:
        m_a, m_e = rng.uniform(-1.0, 1.0, a.shape[1:]), rng.uniform(-1.0, 1.0, a.shape[1:])
        da, de = a * m_a[None] * rng.uniform(0.5, 1.0, a.shape), e * m_e[None] * rng.uniform(0.5, 1.0, a.shape)
        kw.update(dcoeffs=(_t(da), _t(de)), par_t=rng.uniform(-1.0, 1.0, (n_row, N_LAYERS)) * (rng.random((n_row, N_LAYERS)) > 0.3))
    return kw


def _pointing_row_units(eng, los, arrays, a, e, row):
    """Per ray: the units of the pointing row [n_rays, n_pts] against the reference recursion with one parameter per gas
    and the device's own columns and d col / d z_t, bounded by the sum over the gases of the per-row bounds."""
    n_gas = a.shape[0]
    col, dcol = los.columns(), eng.los_columns_dz(los)
    out = []
    for r in range(los.n_rays):
        seg = slice(arrays["seg_off"][r], arrays["seg_off"][r + 1])
        lay = arrays["seg_layer"][seg]
        ref = R.recursion_reference(*ray_forms(a, e, lay, col[:, seg], dcol[:, seg], R.LD), np.zeros(a.shape[2]), thin_ulps=n_gas + 1)
        u = R.units(row[r], ref["J"].sum(axis=0), ref["A"].sum(axis=0), ref["C"].sum(axis=0), n_gas)
        out.append((float(u.max()), int(np.argmax(u))))
    return out


# (n_gas, n_col, n_lev, n_row)
SPECTRA_CASES = [(1, 0, 0, 0),      # pointing alone
                 (2, 7, 0, 0),      # 9 column slots: past an 8-slot block
                 (4, 13, 0, 0),     # 17 column slots: past a 16-slot block
                 (2, 3, 5, 3)]      # with level and row parameters


@pytest.mark.parametrize("n_gas,n_col,n_lev,n_row", SPECTRA_CASES)
def test_spectra_route(eng, n_gas, n_col, n_lev, n_row):
    n_pts = 320                                                  # one full block plus one wave
    los, arrays, path, _ = _batch(eng, n_gas)
    a, e = coefficients(n_gas, n_pts)
    coeffs = (_t(a), _t(e))
    kw = _state_kw(n_gas, n_col, n_lev, n_row, path["alt"], a, e, n_pts)
    n_state = n_col + n_lev + n_row
    rad, jac = eng.limb_rays_state_jacobian(coeffs, los, pointing=True, **kw)
    assert jac.shape == (los.n_rays, n_state + 1, n_pts) and rad.shape == (los.n_rays, n_pts)
    jac_np, rad_np = jac.cpu().numpy(), rad.cpu().numpy()
    tau_max = max(float((a[:, arrays["seg_layer"]] * los.columns()[:, :, None]).sum(axis=0).max()), 0.0)
    # every other row and the radiance: those of the call without the pointing row, bit for bit
    without = kw if n_state else dict(par_gas=np.zeros(1, np.int32), par_w=np.ones((1, los.n_pt)))
    rad0, jac0 = eng.limb_rays_state_jacobian(coeffs, los, **without)
    assert np.array_equal(rad_np, rad0.cpu().numpy())
    if n_state:
        assert np.array_equal(jac_np[:, :n_state], jac0.cpu().numpy())
    worst = _pointing_row_units(eng, los, arrays, a, e, jac_np[:, n_state])
    limit = R.KERNEL_MARGIN * R.K_PLAIN_JAC
    print("\npointing row, %d gases, %d + %d + %d state rows, %d points, largest segment optical depth %.3g: limit %.3g units"
          % (n_gas, n_col, n_lev, n_row, n_pts, tau_max, limit))
    for zt, (u, j) in zip(P.Z_TANS, worst):
        print("  z_t %7.2f km: %8.3g units at point %d%s" % (zt, u, j, "  OVER" if not u <= limit else ""))
    assert np.all(np.isfinite(jac_np)) and np.all(np.abs(jac_np[:, n_state]).max(axis=1) > 0)
    assert all(u <= limit for u, _ in worst), worst


def test_spectra_route_through_the_level_factored_set(eng):
    """Two level-factored gases (the several-gases instances) with the pointing row: the other rows bitwise those of the
    call without, the pointing row against the reference."""
    n_pts, n_gas = 320, 2
    los, arrays, path, _ = _batch(eng, n_gas)
    a, e = coefficients(n_gas, n_pts, seed=1)
    coeffs = (_t(a), _t(e))
    rng = np.random.default_rng([SEED, 77])
    gases = []
    for g in range(2):
        tab = 10.0 ** rng.uniform(-21.0, -18.0, (N_LEVELS, 2, N_TAB_ROWS, n_pts))
        tab[:, 1] *= rng.uniform(1e-8, 1e-7, tab[:, 1].shape)
        gases.append((g, _t(tab), ((np.arange(N_LAYERS) + g) // 2).astype(np.int32)))
    kw = dict(level_gases=gases, par_lgas=np.array([0, 1, 1, 0], np.int32), par_level=np.array([1, 0, 3, 2], np.int32),
              par_c=rng.uniform(0.2, 1.0, (4, N_LAYERS)), par_gas=np.array([1, 0], np.int32),
              par_w=np.array([np.clip(1.0 - np.abs(path["alt"] - q) / 150.0, 0.0, None) + 0.05 for q in (150.0, 400.0)]))
    rad, jac = eng.limb_rays_state_jacobian(coeffs, los, pointing=True, **kw)
    rad0, jac0 = eng.limb_rays_state_jacobian(coeffs, los, **kw)
    assert jac.shape == (los.n_rays, 7, n_pts)
    assert np.array_equal(rad.cpu().numpy(), rad0.cpu().numpy()) and np.array_equal(jac[:, :6].cpu().numpy(), jac0.cpu().numpy())
    worst = _pointing_row_units(eng, los, arrays, a, e, jac[:, 6].cpu().numpy())
    limit = R.KERNEL_MARGIN * R.K_PLAIN_JAC
    print("\npointing row beside two level gases: %s units, limit %.3g" % ([round(u, 2) for u, _ in worst], limit))
    assert all(u <= limit for u, _ in worst), worst


# ------------------------------------------------------------------------------------------------------------------
# 3. the bands route
# ------------------------------------------------------------------------------------------------------------------
BAND_Z_TANS = P.Z_TANS + (410.5,)          # two pixels of three rays


@pytest.mark.parametrize("instrument", [False, True])
@pytest.mark.parametrize("with_fov", [False, True])
def test_bands_route(eng, with_fov, instrument):
    from spectrobot_amd import spect_main_module as smm
    n_pts, n_bands, n_gas, kinds = 330, 17, 2, (3, 4, 2)      # a partial last wave; two band tiles
    pan = B.panel(2975.0, 5e-4, n_pts, n_bands, SEED)
    grid, centers, widths, n_sigma = pan["grid"], pan["centers"], pan["widths"], pan["n_sigma"]
    assert len(centers) == n_bands
    los, arrays, path, _ = _batch(eng, n_gas, BAND_Z_TANS)
    a, e = coefficients(n_gas, n_pts, seed=2)
    coeffs = (_t(a), _t(e))
    kw = _state_kw(n_gas, *kinds, path["alt"], a, e, n_pts)
    n_state = sum(kinds)
    factors = eng.fov_factors(ROTS) if with_fov else None
    band_kw = dict(fov=factors, instrument=instrument, n_sigma=n_sigma)
    got = eng.limb_rays_state_bands(coeffs, los, grid, centers, widths, pointing=True, **band_kw, **kw)
    old = eng.limb_rays_state_bands(coeffs, los, grid, centers, widths, **band_kw, **kw)
    n_out = 2 if with_fov else 6
    assert got.shape == (n_out, 1 + n_state + 1 + (2 if instrument else 0), n_bands)
    # the radiance, the state rows and the instrument rows: those of the fused call without pointing, bit for bit
    assert np.array_equal(got[:, :1 + n_state], old[:, :1 + n_state])
    assert np.array_equal(got[:, 2 + n_state:], old[:, 1 + n_state:])
    # the pointing row: the band integrals of the spectra route's row
    _, jac = eng.limb_rays_state_jacobian(coeffs, los, grid=grid, pointing=True, **kw)
    row = jac[:, n_state].contiguous()
    row_np = row.cpu().numpy()
    ref = B.band_reference(grid, row_np, centers, widths, n_sigma, "Wm2")
    plain = B.plain_fp64(grid, row_np, centers, widths, n_sigma, "Wm2")
    composed = eng.hires_to_lowres(row, grid, centers, widths, n_sigma=n_sigma)
    assert ref["guard"].min() >= B.GUARD_MIN
    val, A = ref["value"], ref["A"]
    if with_fov:
        val, A = B.fov_reference(val, A, factors)
        plain = smm.fov_closed_form(plain[0::3], plain[1::3], plain[2::3], ROTS)
        composed = smm.fov_closed_form(composed[0::3], composed[1::3], composed[2::3], ROTS)
    k_plain = float(B.units_raw(plain, val, A).max())
    limit = B.limit(k_plain)
    fused = B.worst(B.units_raw(got[:, 1 + n_state], val, A), band_names=pan["band_names"])
    comp = B.worst(B.units_raw(composed, val, A), band_names=pan["band_names"])
    print("\npointing row on %d bands (fov %d, instrument %d): K_PLAIN %.3g limit %.3g; fused %.3g units at %s; composed %.3g units at %s"
          % (n_bands, with_fov, instrument, k_plain, limit, fused[0], fused[1], comp[0], comp[1]))
    dead = ref["count"] < 2
    assert np.all(got[:, :, dead] == 0.0) and np.any(got[:, 1 + n_state][:, ~dead] != 0.0)
    assert fused[0] <= limit and comp[0] <= limit


# ------------------------------------------------------------------------------------------------------------------
# 4. end to end against central differences
# ------------------------------------------------------------------------------------------------------------------
def cpu_chain_distances(a, e, n_gas):
    """Per ray of the case set, the long double chain (helper geometry and columns + recursion_reference): (the distance
    of the analytic pointing row from the central difference at the ray's step -- the truncation a difference carries --,
    max |rad|, max |row|)."""
    z, nd, vmr = P.case_profiles(n_gas)
    scale = np.asarray(COL_SCALE[:n_gas], P.LD)[:, None]
    zero = np.zeros(a.shape[2])
    out = []
    for zt in P.Z_TANS:
        h = P.diff_step(zt)
        shells = P.crossed_shells(z, zt)
        G = P.geometry_ld(z, nd, vmr, zt, shells=shells)
        lay = G["k"]

        def radiance(at):
            g = P.geometry_ld(z, nd, vmr, at, shells=shells)
            u = P.columns(g["x"], g["nd"], g["vmr"]) * scale
            tau, E = R.products(a[:, lay], u, R.LD), R.products(e[:, lay], u, R.LD)
            none = np.zeros((0,) + tau.shape, R.LD)
            return R.recursion_reference(tau, E, none, none, zero, want_cond=False)["I"]

        diff = (radiance(P.LD(zt) + P.LD(h)) - radiance(P.LD(zt) - P.LD(h))) / P.LD(2 * h)
        u = P.columns(G["x"], G["nd"], G["vmr"]) * scale
        ref = R.recursion_reference(*ray_forms(a, e, lay, u, P.dcol_reference(G) * scale, R.LD), zero, want_cond=False)
        row = ref["J"].sum(axis=0)
        out.append((float(np.abs(row - diff).max() / np.abs(row).max()), float(np.abs(ref["I"]).max()), float(np.abs(row).max())))
    return out


def test_end_to_end_against_central_differences(eng):
    """The pointing row of geometry.limb_los(path=True) batches against (I(z_t + h) - I(z_t - h)) / 2h of engine.limb_rays
    on batches rebuilt by geometry.limb_los at z_t +- h, h = 1e-3 km (1e-4 km for the ray at 349.0 km), per ray in the
    largest |row|.  The limit is 10 x the same distance of the long double chain at the same h (the truncation of the
    difference, which cannot be derived) plus 2^-50 max |rad| / h.

    Measured 2026-10-19 on an MI355X (2 gases, 320 points), analytic against difference, relative to the largest |row| of
    the ray:
        z_t [km]   h [km]   long double chain   limit      this route
        127.30     1e-3     6.99e-10            7.07e-09   6.51e-10
        150.01     1e-3     2.02e-10            2.12e-09   2.00e-10
        260.00     1e-3     8.66e-11            9.31e-10   1.84e-10
        349.00     1e-4     1.21e-09            1.22e-08   3.32e-09
        470.00     1e-3     1.19e-10            1.22e-09   3.40e-10
    (where this route stands above the chain it is the fp64 rounding of the rebuilt batches' sample altitudes, a few
    1e-13 km of a 45 km scale height, divided by 2h)."""
    from spectrobot_amd import geometry
    n_gas, n_pts = 2, 320
    a, e = coefficients(n_gas, n_pts, seed=3)
    coeffs = (_t(a), _t(e))
    z, nd, vmr = P.case_profiles(n_gas)
    zt = np.array(P.Z_TANS)
    h = np.array([P.diff_step(v) for v in zt])

    def batch(z_tans, path=False):
        L = geometry.limb_los(z, nd, vmr, z_tans, R=P.R_KM, n_sub=P.N_SUB, path=path)
        return eng.LimbLOS(L["seg_off"], L["seg_layer"], L["pt_off"], L["x"], L["nd"], L["vmr"], col_scale=COL_SCALE[:n_gas],
                           path=dict(alt=L["alt"], dx=L["dx_dzt"], dalt=L["dalt_dzt"]) if path else None)

    rad, jac = eng.limb_rays_state_jacobian(coeffs, batch(zt, path=True), pointing=True)
    assert jac.shape == (5, 1, n_pts)
    row = jac[:, 0].cpu().numpy()
    up = eng.limb_rays(coeffs, batch(zt + h), resident=False).cpu().numpy()
    down = eng.limb_rays(coeffs, batch(zt - h), resident=False).cpu().numpy()
    diff = (up - down) / (2.0 * h)[:, None]
    cpu = cpu_chain_distances(a, e, n_gas)
    bad = []
    print("")
    for r in range(5):
        got = float(np.abs(row[r] - diff[r]).max() / np.abs(row[r]).max())
        limit = 10.0 * cpu[r][0] + 2.0 ** -50 * float(np.abs(rad[r].cpu().numpy()).max()) / h[r] / float(np.abs(row[r]).max())
        print("z_t %7.2f km, h %g km: long double chain %.3g, limit %.3g, this route %.3g%s"
              % (zt[r], h[r], cpu[r][0], limit, got, "  OVER" if not got <= limit else ""))
        if not got <= limit:
            bad.append((zt[r], got, limit))
    assert not bad, bad


# ------------------------------------------------------------------------------------------------------------------
# 5. refusals
# ------------------------------------------------------------------------------------------------------------------
def test_refused_calls_leave_their_outputs_untouched(eng):
    import ctypes as C
    import torch
    from spectrobot_amd import _lib
    n_gas, n_pts = 2, 64
    los, arrays, path, _ = _batch(eng, n_gas)
    a, e = coefficients(n_gas, n_pts, seed=4)
    coeffs = (_t(a), _t(e))
    pan = B.panel(2975.0, 5e-4, n_pts, 5, SEED)
    kw = _state_kw(n_gas, 2, 0, 0, path["alt"], a, e, n_pts)
    good_rad, good_jac = eng.limb_rays_state_jacobian(coeffs, los, pointing=True, **kw)
    good = eng.limb_rays_state_bands(coeffs, los, pan["grid"], pan["centers"], pan["widths"], pointing=True, **kw)

    def calls(batch, path_desc):
        """(status of the spectra entry, status of the bands entry) with sentinels in jac and out, which must survive."""
        A = eng._state_args(coeffs, batch, kw["par_gas"], kw["par_w"], None, None, None, None, 0, pan["grid"], 0, None, None,
                            may_be_empty=True, as_list=True)
        w0, step, _ = eng.grid_params(pan["grid"])
        A.desc.w0, A.desc.step = w0, step
        jac = torch.full((batch.n_rays, 2 + n_gas, n_pts), -7.25, dtype=torch.float64, device="cuda")
        out = np.full(good.shape, -7.25)
        p = None if path_desc is None else C.byref(path_desc)
        s1 = _lib.lib.sr_limb_rays_jac_state_path_dev(*A.args("sr_limb_rays_jac_state_path_dev", p, None, C.c_void_p(jac.data_ptr()), None))
        cen, wid = np.ascontiguousarray(pan["centers"]), np.ascontiguousarray(pan["widths"])
        s2 = _lib.lib.sr_limb_rays_state_bands_path_dev(*A.args("sr_limb_rays_state_bands_path_dev", cen.ctypes.data_as(_lib.dp),
                                                                wid.ctypes.data_as(_lib.dp), cen.size, 5.0, 0, None,
                                                                out.ctypes.data_as(_lib.dp), None, 0, p))
        torch.cuda.synchronize()
        return s1, s2, jac.cpu().numpy(), out

    # a NULL path, a path with a NULL array
    for bad in (None, "alt", "dx_dz", "dalt_dz"):
        desc = None
        if bad is not None:
            desc = los.path_desc()
            setattr(desc, bad, None)
        s1, s2, jac, out = calls(los, desc)
        assert (s1, s2) == (_lib.SR_ERR_ARG, _lib.SR_ERR_ARG), bad
        assert np.all(jac == -7.25) and np.all(out == -7.25), bad
    # observer order
    obs, _, _, _ = _batch(eng, n_gas, LOS_order="observer")
    s1, s2, jac, out = calls(obs, obs.path_desc())
    assert (s1, s2) == (_lib.SR_ERR_UNSUPPORTED, _lib.SR_ERR_UNSUPPORTED)
    assert np.all(jac == -7.25) and np.all(out == -7.25)
    with pytest.raises(_lib.SpectRobotHipError, match="photon order"):
        eng.los_columns_dz(obs)
    # a batch without path
    bare = eng.LimbLOS(arrays["seg_off"], arrays["seg_layer"], arrays["pt_off"], arrays["x"], arrays["nd"], arrays["vmr"])
    for call in (lambda: eng.los_columns_dz(bare), lambda: eng.limb_rays_state_jacobian(coeffs, bare, pointing=True, **kw),
                 lambda: eng.limb_rays_state_bands(coeffs, bare, pan["grid"], pan["centers"], pan["widths"], pointing=True, **kw)):
        with pytest.raises(ValueError, match="path"):
            call()
    # and the valid calls still give what they gave
    s1, s2, jac, out = calls(los, los.path_desc())
    assert (s1, s2) == (_lib.SR_OK, _lib.SR_OK)
    assert np.array_equal(jac[:, :3], good_jac.cpu().numpy()) and np.array_equal(out, good)
