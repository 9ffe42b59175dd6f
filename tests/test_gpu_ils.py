"""Tabulated instrument line shapes on the GPU (sr_set_ils -> sr_lowres_weights_tab_kernel<INSTR>; engine.ILS and the ils=
keyword) against the extended-precision reference of tests/ils_reference.py: the band values and their derivatives to the
band centre and to the logarithm of the width under a cubic Hermite interpolant of tabulated knots, through
hires_to_lowres[_instrument], the fused state call and the one-call forward model.

All three rows are held to 8 x max(K_PLAIN_ILS, 1) units of 2^-53 A + 1e-290 with the A of the helper's docstring,
K_PLAIN_ILS being what plain_fp64_ils (plain numpy, written in the helper) measures against the reference on the test's
own (spectrum, band) pairs -- never what a kernel gives.  Row 0 of the instrument call is hires_to_lowres(ils=...) bit
for bit; bands outside the grid and windows of fewer than two points are exact 0.0 in all rows; a call without ils, before,
between and after calls with one, gives what it always gave, bit for bit.  Needs a real MI355X."""
import ctypes as C

import numpy as np
import pytest

import lowres_reference as R
import ils_reference as S

pytestmark = pytest.mark.gpu
SEED = 20261018
GRID = S.GRID


@pytest.fixture(scope="module")
def eng():
    import torch
    assert torch.cuda.is_available(), "these tests need the GPU"
    from spectrobot_amd import engine
    engine.set_device(0)
    return engine


@pytest.fixture(scope="module")
def panel():
    """The 8193-point, 33-band panel (two chunk boundaries at 4096, the 64-point slots, three band tiles, one-hot probes;
    with t_lo, t_hi = -+5 its windows are the Gaussian panel's) under the 33 lobed tables and under the first of them
    shared by all bands, with the references, computed once."""
    P = R.panel(GRID[0], GRID[1], 8193, 33, SEED)
    t_lo, t_hi, phi = S.lobed_tables(33)
    assert P["n_structured"] <= 33 and S.guard_ils(P["grid"], P["centers"], P["widths"], t_lo, t_hi).min() >= R.GUARD_MIN
    P["tables"] = {"shared": (t_lo, t_hi, phi[:1]), "per band": (t_lo, t_hi, phi)}
    P["units"] = {"shared": "Wm2", "per band": "nWcm2"}
    P["ref"] = {k: S.band_reference_ils(P["grid"], P["spec"], P["centers"], P["widths"], *t, units=P["units"][k]) for k, t in P["tables"].items()}
    P["plain"] = {k: S.plain_fp64_ils(P["grid"], P["spec"], P["centers"], P["widths"], *t, units=P["units"][k]) for k, t in P["tables"].items()}
    return P


def _t(v):
    import torch
    return torch.tensor(np.ascontiguousarray(v, dtype=np.float64), device="cuda")


def _ils(eng, table):
    """The helper's table as an engine.ILS, knots as given (the reference reads the same fp64 values)."""
    t_lo, t_hi, phi = table
    ils = eng.ILS(t_lo, t_hi, phi if phi.shape[0] > 1 else phi[0], normalize=False)
    assert np.array_equal(ils.phi, phi)
    return ils


def _check(tag, got3, ref, plain, spec_names, band_names):
    """got3 [n_spec, 3, n_bands] against a band_reference_ils; every figure is printed before anything is asserted."""
    got3 = np.asarray(got3)
    assert got3.shape == ref["value"].shape
    k_plain = float(S.units_of(plain, ref).max())
    lim = R.limit(k_plain)
    u = S.units_of(got3, ref)
    rows = [(S.ROWS[k],) + R.worst(u[:, k], spec_names, band_names) for k in range(3)]
    print("\n%s: K_PLAIN_ILS %.3g limit %.3g" % (tag, k_plain, lim))
    for name, m, where in rows:
        print("  %-36s %10.3g units%s at %s" % (name, m, "  OVER" if not m <= lim else "", where))
    dead = ref["count"] < 2
    assert np.all(got3[:, :, dead] == 0.0), "a band without a trapezoid is not an exact 0.0 in every row"
    bad = [r for r in rows if not r[1] <= lim]
    assert not bad, "over 8 x max(K_PLAIN_ILS, 1) = %.3g: %s" % (lim, bad)
    return lim


def _three(eng, spec, grid, centers, widths, ils, **kw):
    dev = _t(spec)
    three = eng.hires_to_lowres_instrument(dev, grid, centers, widths, ils=ils, **kw)
    value = eng.hires_to_lowres(dev, grid, centers, widths, ils=ils, **kw)
    assert np.array_equal(three[0], value), "row 0 is not engine.hires_to_lowres(ils=...), bit for bit"
    return np.stack(three, axis=1)


@pytest.mark.parametrize("which", ["shared", "per band"])
def test_three_rows_on_the_panel(eng, panel, which):
    P = panel
    ils = _ils(eng, P["tables"][which])
    assert ils.n_shapes == (1 if which == "shared" else 33)
    got = _three(eng, P["spec"], P["grid"], P["centers"], P["widths"], ils, out_units=P["units"][which])
    ref = P["ref"][which]
    dead = ref["count"] < 2
    assert got.shape == (len(P["spec"]), 3, 33) and dead.sum() >= 3
    assert all(np.any(got[:, k][:, ~dead] != 0.0) for k in range(3))
    _check("ils %s, 8193 pts 33 bands %s" % (which, P["units"][which]), got, ref, P["plain"][which], P["spec_names"], P["band_names"])
    # the lobes are there: the value's weights of the whole-grid band change sign
    b = P["band_names"].index("whole grid")
    hot = got[2:, 0, b]
    assert hot.min() < 0 < hot.max()


def test_the_weight_cache_follows_the_binding(eng, panel):
    """Gaussian, table A, table B, Gaussian, table A on the same bands and spectra: each result is its first occurrence bit
    for bit, the Gaussian's what the call without ils gives -- also with the instrument rows (the other scratch layout), and
    A differs from B differs from the Gaussian."""
    P = panel
    rows = np.r_[0:2, 2:len(P["spec"]):11]
    dev = _t(P["spec"][rows])
    cw = (P["grid"], P["centers"], P["widths"])
    t_lo, t_hi, phi = P["tables"]["per band"]
    A, B = _ils(eng, (t_lo, t_hi, phi[:1])), _ils(eng, (t_lo, t_hi, phi[1:2]))
    gauss = eng.hires_to_lowres(dev, *cw)
    gauss3 = np.stack(eng.hires_to_lowres_instrument(dev, *cw), axis=1)
    seen = {}
    for name, ils in (("gauss", None), ("A", A), ("B", B), ("gauss", None), ("A", A), ("B", B), ("A", A)):
        low = eng.hires_to_lowres(dev, *cw, ils=ils) if ils is not None else eng.hires_to_lowres(dev, *cw)
        three = np.stack(eng.hires_to_lowres_instrument(dev, *cw, ils=ils), axis=1)
        assert np.array_equal(three[:, 0], low)
        if name in seen:
            assert np.array_equal(low, seen[name][0]) and np.array_equal(three, seen[name][1]), name
        seen[name] = (low, three)
    assert np.array_equal(seen["gauss"][0], gauss) and np.array_equal(seen["gauss"][1], gauss3)
    assert not np.array_equal(seen["A"][0], seen["B"][0]) and not np.array_equal(seen["A"][0], gauss)
    # the same table bound anew is another binding of the same numbers
    assert np.array_equal(eng.hires_to_lowres(dev, *cw, ils=_ils(eng, (t_lo, t_hi, phi[:1]))), seen["A"][0])
    assert np.array_equal(eng.hires_to_lowres(dev, *cw), gauss)


@pytest.mark.parametrize("n_pts,k", [(8193, 5000), (300, 130)])
def test_exact_window_ends_and_knots(eng, n_pts, k):
    """The three bands of ils_reference.exact_cases under the table on [-5, 3] whose ends are not small: the window's lower
    end bitwise the grid value x_k (t = t_lo there), its upper end (t = t_hi: the last knot, by the clamp), and x_k exactly
    on an interior knot.  The end point belongs to the window, its neighbour outside is an exact 0.0, and the one-hot
    spectrum at k returns p phi_knot / w."""
    g, _ = R.make_grid(GRID[0], GRID[1], n_pts)
    t_lo, t_hi, phi = S.skewed_table()
    knot = 20
    t_knot = t_lo + knot * 0.125
    centers, widths, xk = S.exact_cases(g, k, t_lo, t_hi, t_knot)
    assert centers[0] + t_lo * 0.25 == xk and centers[1] + t_hi * 0.25 == xk and (xk - centers[2]) / 0.25 == t_knot and xk == 1e7 / g[k]
    # the four ends that are NOT on a grid point keep the panel's guard
    far_ends = S.guard_ils(g, [centers[0] + t_hi * 0.25, centers[1] + t_lo * 0.25, centers[2] + t_lo * 0.25, centers[2] + t_hi * 0.25],
                           [1e-9] * 4, -1.0, 1.0)
    assert far_ends.min() >= R.GUARD_MIN, far_ends
    rng = np.random.default_rng([SEED, n_pts, k])
    spec = np.zeros((5, n_pts))
    spec[0, k] = spec[1, k - 1] = spec[2, k + 1] = 1.0
    spec[3] = rng.uniform(0.5, 1.5, n_pts)
    spec[4] = rng.choice([-1.0, 1.0], n_pts) * 10.0 ** rng.uniform(-6.0, 0.0, n_pts)
    names = ["one-hot at k", "one-hot at k - 1", "one-hot at k + 1", "positive noise", "signed"]
    ref = S.band_reference_ils(g, spec, centers, widths, t_lo, t_hi, phi)
    assert np.all(ref["count"] >= 2)
    got = _three(eng, spec, g, centers, widths, _ils(eng, (t_lo, t_hi, phi)))
    lim = _check("exact ends and knot, %d pts, k %d" % (n_pts, k), got, ref, S.plain_fp64_ils(g, spec, centers, widths, t_lo, t_hi, phi), names,
                 ["lo == x_k", "hi == x_k", "x_k on knot %d" % knot])
    assert np.all(got[0, 0] > 0)                                   # the end points are in: phi > 0 at both ends and on the knot
    assert np.all(got[2, :, 0] == 0.0) and np.all(got[1, :, 1] == 0.0)   # the neighbours outside (cm-1 k + 1 below lo, k - 1 above hi)
    x, gl = (1e7 / g).astype(R.LD), g.astype(R.LD)
    for b, kn, xl, xr in ((0, 0, x[k], x[k - 1]), (1, phi.shape[1] - 1, x[k + 1], x[k]), (2, knot, x[k + 1], x[k - 1])):
        want = R.unit_factor("Wm2") * gl[k] * gl[k] * R._ten(-7) * (xr - xl) / R.LD(2) * R.LD(phi[0, kn]) / R.LD(widths[b])
        u = float(R.units_raw(got[0, 0, b], want, ref["A"][0, 0, b]))
        print("  one-hot at k, band %d: p phi_%d / w to %.3g units" % (b, kn, u))
        assert u <= lim


def test_shards_add_up(eng, panel):
    """A split at g_lo = 4097: [0, 4098) and [4097, 8193).  Each shard's three rows against the reference's partial sums,
    their sum against the whole."""
    P = panel
    rows = np.r_[0:2, 2:len(P["spec"]):5]
    spec, names = P["spec"][rows], [P["spec_names"][r] for r in rows]
    cw = (P["centers"], P["widths"])
    table = P["tables"]["per band"]
    ils = _ils(eng, table)
    whole = S.band_reference_ils(P["grid"], spec, *cw, *table)
    got = {}
    for name, (a, b) in (("shard 0", (0, 4098)), ("shard 1", (4097, 8193))):
        got[name] = _three(eng, spec[:, a:b], P["grid"], *cw, ils, g_lo=a)
        ref = S.band_reference_ils(P["grid"], spec[:, a:b], *cw, *table, g_lo=a)
        _check("%s [%d, %d)" % (name, a, b), got[name], ref, S.plain_fp64_ils(P["grid"], spec[:, a:b], *cw, *table, g_lo=a), names,
               P["band_names"])
    total = got["shard 0"] + got["shard 1"]
    u = S.units_of(total, whole)
    lim = R.limit(S.units_of(S.plain_fp64_ils(P["grid"], spec, *cw, *table), whole).max())       # the whole's own pairs
    print("\nshard 0 + shard 1 against the whole: %s units (limit %.3g)" % ([float(u[:, k].max()) for k in range(3)], lim))
    assert got["shard 0"][:, 1:].any() and got["shard 1"][:, 1:].any() and u.max() <= lim


def test_unsorted_and_duplicated_bands(eng, panel):
    """The panel's bands reversed and then once more (66 bands: five tiles), the per-band tables permuted alike: each band's
    three rows are bitwise what the panel's order gave."""
    P = panel
    assert "duplicate of overlap a" in P["band_names"] and np.any(np.diff(P["centers"]) < 0) and np.any(np.diff(P["centers"]) > 0)
    rows = np.r_[0:2, 2:len(P["spec"]):7]
    dev = _t(P["spec"][rows])
    ils = _ils(eng, P["tables"]["per band"])
    base = np.stack(eng.hires_to_lowres_instrument(dev, P["grid"], P["centers"], P["widths"], ils=ils), axis=1)
    a, b = P["band_names"].index("overlap a"), P["band_names"].index("duplicate of overlap a")
    assert not np.array_equal(base[:, :, a], base[:, :, b])           # the same band under two tables
    order = np.concatenate([np.arange(33)[::-1], np.arange(33)])
    ils66 = ils.select(order)
    assert ils66.n_shapes == 66
    twice = np.stack(eng.hires_to_lowres_instrument(dev, P["grid"], P["centers"][order], P["widths"][order], ils=ils66), axis=1)
    assert twice.shape == (len(rows), 3, 66) and np.array_equal(twice, base[:, :, order])


# ----------------------------------------------------------------------------------------------------------------------
# the fused paths: the recursion kernels' band epilogue reads the same tables
# ----------------------------------------------------------------------------------------------------------------------
def _assemble(ref3, n_rays, n_row, instrument):
    """[n_rays (1 + n_par), 3, nb] of the rays' spectra (ray-major: the radiance, then the parameter rows) ->
    [n_rays, n_row (+ 2), nb]: the value's row of every spectrum, then the radiance's two instrument rows."""
    v = ref3.reshape((n_rays, n_row) + ref3.shape[1:])
    out = [v[:, :, 0]]
    if instrument:
        out.append(v[:, 0, 1:])
    return np.concatenate(out, axis=1)


def _hold_fused(tag, got, got_fov, spectra, P, table, units, factors, rots, instrument):
    """got [n_rays, n_row (+ 2), nb], got_fov [n_pix, ...] against the reference on spectra [n_rays, n_row, n_pts] (fp64 data:
    what the unfused route writes), the field of view through lowres_reference.fov_reference; K_PLAIN from plain_fp64_ils
    (and smm.fov_closed_form) on the same pairs: the bound of tests/test_gpu_lowres_reference.py's _fused_check and of
    tests/test_gpu_state_bands_instr.py's _hold, with the tabulated shape's reference in the Gaussian's place."""
    from spectrobot_amd import spect_main_module as smm
    n_rays, n_row, n = spectra.shape
    flat = spectra.reshape(n_rays * n_row, n)
    assert np.all(np.isfinite(flat)) and np.count_nonzero(flat) > flat.size // 4
    ref = S.band_reference_ils(P["grid"], flat, P["centers"], P["widths"], *table, units=units)
    plain = S.plain_fp64_ils(P["grid"], flat, P["centers"], P["widths"], *table, units=units)
    assert ref["guard"].min() >= R.GUARD_MIN
    val, A, pl = (_assemble(np.asarray(v), n_rays, n_row, instrument) for v in (ref["value"], ref["A"], plain))
    dead = ref["count"] < 2
    bad = []
    for kind, g, v, a, p in (("rays", got, val, A, pl),
                             ("field of view", got_fov) + R.fov_reference(val, A, factors) + (smm.fov_closed_form(pl[0::3], pl[1::3], pl[2::3], rots),)):
        lim = R.limit(float(R.units_raw(p, v, a).max()))
        u = R.units_raw(g, v, a)
        k = np.unravel_index(int(np.argmax(u)), u.shape)
        print("%s, %s: K_PLAIN %.3g limit %.3g; worst %.3g units%s at row %d | %s; instrument rows %.3g"
              % (tag, kind, lim / R.KERNEL_MARGIN, lim, u[k], "  OVER" if not u[k] <= lim else "", k[1], P["band_names"][k[2]],
                 u[:, n_row:].max() if instrument else 0.0))
        assert g.shape == v.shape and np.all(g[:, :, dead] == 0.0)
        if not u.max() <= lim:
            bad.append((kind, float(u.max()), lim))
    assert dead.any() and not bad, bad


def test_state_bands_with_a_table_per_band(eng):
    """engine.limb_rays_state_bands(ils=...) on the smallest mixed case of tests/test_gpu_state_rows.py (tests/state_rows_cases.py's
    batch: 300 points, 3 rays; 2 column + 3 level + 4 row parameters), 33 bands, instrument=True, without and with the
    field of view, one table per band -- against limb_rays_state_jacobian's spectra through the reference, and the
    composition hires_to_lowres_instrument(ils=...) held to the same reference under the same limit."""
    import state_rows_cases as SR
    import test_gpu_state_rows as TR
    from spectrobot_amd import spect_main_module as smm
    m = TR._mixed(1, 2, 3, 4)
    n, n_par, nb, rots = SR.N_PTS, 9, 33, [20.0]
    P = R.panel(GRID[0], GRID[1], n, nb, SEED)
    table = S.lobed_tables(nb)
    ils = _ils(eng, table)
    los = TR._los(eng, m)
    try:
        rad, jac = TR._state_rows(eng, m, los, grid=P["grid"])
        spectra = np.concatenate([rad.cpu().numpy()[:, None], jac.cpu().numpy()], axis=1)
        assert spectra.shape == (3, 1 + n_par, n)
        factors = eng.fov_factors(rots)
        kw = dict(par_gas=m["par_gas"], par_w=m["par_w"], tab=m["tab"], coef_row=m["coef_row"], par_level=m["par_level"], par_c=m["par_c"],
                  gas=m["gas"], dcoeffs=m["dco"], par_t=m["par_t"])
        run = lambda fov, **k: eng.limb_rays_state_bands(m["co"], los, P["grid"], P["centers"], P["widths"], fov=fov, **kw, **k)
        got, got_fov = run(None, instrument=True, ils=ils), run(factors, instrument=True, ils=ils)
        assert got.shape == (3, 1 + n_par + 2, nb) and got_fov.shape == (1, 1 + n_par + 2, nb)
        # without the instrument rows: the same value and parameter rows, bit for bit; and the Gaussian is back behind the call
        assert np.array_equal(run(None, ils=ils), got[:, :1 + n_par])
        gauss = run(None)
        assert not np.array_equal(gauss, got[:, :1 + n_par])
        _hold_fused("state_bands, 2 + 3 + 4 parameters, 33 tables", got, got_fov, spectra, P, table, "Wm2", factors, rots, True)
        # the composition
        flat = _t(spectra.reshape(3 * (1 + n_par), n))
        low = eng.hires_to_lowres(flat, P["grid"], P["centers"], P["widths"], ils=ils).reshape(3, 1 + n_par, nb)
        three = eng.hires_to_lowres_instrument(rad, P["grid"], P["centers"], P["widths"], ils=ils)
        comp = np.concatenate([low, three[1][:, None], three[2][:, None]], axis=1)
        assert np.array_equal(three[0], low[:, 0])
        comp_fov = smm.fov_closed_form(comp[0::3], comp[1::3], comp[2::3], rots)
        _hold_fused("composition", comp, comp_fov, spectra, P, table, "Wm2", factors, rots, True)
        assert np.array_equal(run(None), gauss)
    finally:
        los.close()


def test_retrieval_forward_with_a_table_per_band(eng):
    """engine.retrieval_forward(ils=...) (the band epilogue of sr_limb_fold_sens_lds_kernel: `buf` stays untouched) on the
    case of tests/test_gpu_lowres_reference.py::test_retrieval_forward_band_epilogue (3 parameters, 257 points, 6 rays),
    33 bands, one table per band, without and with the field of view -- against the spectra the same call writes into `buf`
    with band fusion off, whose own band values (hires_to_lowres's kernels under the same table) are held too."""
    import torch
    import test_gpu_state_bands as SB
    n_par, n_gas, n, nb = 3, 1, 257, 33
    c = SB._case(eng, n_par, 0, 0, n_gas, n)
    par_gas, W = c["kw"]["par_gas"], c["kw"]["par_w"]
    x = c["rng"].uniform(0.5, 1.5, n_par) * np.array([[1.2e-2, 2e-3, 3e-4][g] for g in par_gas])
    factors = eng.fov_factors(SB.ROTS)
    los = SB._los(eng, c)
    P = R.panel(GRID[0], GRID[1], n, nb, SEED)
    assert np.array_equal(P["grid"], c["grid"])
    table = S.lobed_tables(nb)
    ils = _ils(eng, table)
    call = lambda fov, buf, **k: eng.retrieval_forward(c["coeffs"], los, par_gas, W, x, c["grid"], P["centers"], P["widths"],
                                                     out_units="nWcm2", fov=fov, buf=buf, **k)
    try:
        eng.set_band_fusion(0)
        unfused, buf = call(None, None, ils=ils)
        spectra = buf.cpu().numpy()
        spectra = np.concatenate([spectra[:6, None], spectra[6:].reshape(6, n_par, n)], axis=1)
        unfused_fov = call(factors, buf, ils=ils)[0]
        eng.set_band_fusion(1)
        mark = torch.full_like(buf, -7.0)
        fused, fused_fov = call(None, mark, ils=ils)[0], call(factors, mark, ils=ils)[0]
        gauss = call(None, mark)[0]
        assert bool((mark == -7.0).all()), "the fused route was not taken"
    finally:
        eng.set_band_fusion(1)
    assert fused.shape == (6, 1 + n_par, nb) and fused_fov.shape == (2, 1 + n_par, nb) and not np.array_equal(gauss, fused)
    _hold_fused("retrieval_forward fused, 3 parameters, 33 tables", fused, fused_fov, spectra, P, table, "nWcm2", factors, SB.ROTS, False)
    _hold_fused("retrieval_forward unfused", unfused, unfused_fov, spectra, P, table, "nWcm2", factors, SB.ROTS, False)


# ----------------------------------------------------------------------------------------------------------------------
# refusals
# ----------------------------------------------------------------------------------------------------------------------
def test_a_mismatched_table_count_is_refused_and_leaves_out_untouched(eng, panel):
    from spectrobot_amd import _lib
    P = panel
    dev = _t(P["spec"][:3])
    cw = (P["grid"], P["centers"], P["widths"])
    t_lo, t_hi, phi = P["tables"]["per band"]
    gauss = eng.hires_to_lowres(dev, *cw)
    five = _ils(eng, (t_lo, t_hi, phi[:5]))
    w0, step, _ = eng.grid_params(P["grid"])
    cen, wid = np.ascontiguousarray(P["centers"]), np.ascontiguousarray(P["widths"])
    out = np.full((3, 3, 33), -7.25)
    args = (C.c_void_p(dev.data_ptr()), 3, 8193, 0, w0, step, cen.ctypes.data_as(_lib.dp), wid.ctypes.data_as(_lib.dp), 33, 5.0, 0,
            out.ctypes.data_as(_lib.dp), None)
    try:
        assert _lib.lib.sr_set_ils(C.byref(five.desc)) == _lib.SR_OK
        assert _lib.lib.sr_hires_to_lowres_shard_dev(*args) == _lib.SR_ERR_ARG
        assert _lib.lib.sr_hires_to_lowres_instr_shard_dev(*args) == _lib.SR_ERR_ARG
        assert np.all(out == -7.25)
        # five bands: the binding fits
        args5 = args[:8] + (5,) + args[9:]
        assert _lib.lib.sr_hires_to_lowres_instr_shard_dev(*args5) == _lib.SR_OK
        want = np.stack(eng.hires_to_lowres_instrument(dev, P["grid"], cen[:5], wid[:5], ils=five), axis=1)
        assert np.array_equal(out.reshape(-1)[:3 * 3 * 5].reshape(3, 3, 5), want)
    finally:
        _lib.lib.sr_set_ils(None)
    # through the wrapper: the status comes up, the Gaussian is bound again behind the failed call
    with pytest.raises(_lib.SpectRobotHipError) as e:
        eng.hires_to_lowres(dev, *cw, ils=five)
    assert e.value.status == _lib.SR_ERR_ARG
    assert np.array_equal(eng.hires_to_lowres(dev, *cw), gauss)
