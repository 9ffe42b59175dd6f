"""The two instrument rows of the fused state call (sr_limb_rays_state_bands_instr[_gases]_dev: the INSTR = true instances
of sr_limb_jac_state_kernel, engine.limb_rays_state_bands(instrument=True), LevelFactored[Set].state_bands): the
derivatives of the radiance's bands to the band centre and to the logarithm of the ILS width, from the band epilogue of
the recursion kernel, on the case builder's shapes of tests/test_gpu_state_bands.py (22 layers, 6 rays).

Per case, without and with the field of view:
  rows 0 .. n_par of the call with the instrument rows are BITWISE those of the call without them;
  the two instrument rows are within 8 x max(K_PLAIN_INSTR, 1) units of the extended-precision reference
    (tests/lowres_instr_reference.py) evaluated on the hi-res radiance limb_rays_state_jacobian returns on the same inputs
    (the same recursion, operation for operation: fp64 data), through lowres_reference.fov_reference with the field of view;
    K_PLAIN_INSTR is plain_fp64_instr's distance (with smm.fov_closed_form) on the same pairs, never a kernel's;
  the composed route, engine.hires_to_lowres_instrument on that radiance (+ smm.fov_closed_form), is held to the same
    reference under the same limit -- there is no fused-against-composed constant;
  a band outside the grid (and every window of fewer than two points) is an exact 0.0 in every row.
Needs a real MI355X."""
import ctypes as C

import numpy as np
import pytest

import lowres_reference as R
import lowres_instr_reference as I

pytestmark = pytest.mark.gpu
SEED = 20261018


@pytest.fixture(scope="module")
def eng():
    import torch
    assert torch.cuda.is_available(), "these tests need the GPU"
    from spectrobot_amd import engine
    engine.set_device(0)
    return engine


def _hold(tag, rows, rad, P, units, factors, rots):
    """rows: {name: [n_rays | n_pix, 2, n_bands]} (d / d centre, d / d ln width) of the routes under test, against the
    reference on rad [n_rays, n_pts]; every figure is printed before anything is asserted."""
    from spectrobot_amd import spect_main_module as smm
    ref = I.band_reference_instr(P["grid"], rad, P["centers"], P["widths"], P["n_sigma"], units)
    plain = I.plain_fp64_instr(P["grid"], rad, P["centers"], P["widths"], P["n_sigma"], units)
    assert ref["guard"].min() >= R.GUARD_MIN
    val, A = ref["value"][:, 1:], ref["A"][:, 1:]
    pl = plain[:, 1:]
    if factors is not None:
        val, A = R.fov_reference(val, A, factors)
        pl = smm.fov_closed_form(pl[0::3], pl[1::3], pl[2::3], rots)
    k_plain = float(R.units_raw(pl, val, A).max())
    lim = R.limit(k_plain)
    dead = ref["count"] < 2
    print("\n%s: K_PLAIN_INSTR %.3g limit %.3g" % (tag, k_plain, lim))
    bad = []
    for name, got in rows.items():
        u = R.units_raw(got, val, A)
        for k in range(2):
            m, where = R.worst(u[:, k], band_names=P["band_names"])
            print("  %-10s %-16s %10.3g units%s at %s" % (name, I.ROWS[1 + k], m, "  OVER" if not m <= lim else "", where))
            if not m <= lim:
                bad.append((name, I.ROWS[1 + k], m, where))
        assert np.all(got[:, :, dead] == 0.0), name
        assert np.any(got[:, 0, ~dead] != 0.0) and np.any(got[:, 1, ~dead] != 0.0), name
    assert not bad, "over 8 x max(K_PLAIN_INSTR, 1) = %.3g: %s" % (lim, bad)


# (n_col, n_lev, n_row), n_gas, n_pts, bands, units
CASES = [((3, 0, 0), 1, 63, 17, "Wm2"),
         ((0, 8, 0), 1, 257, 33, "ergscm2"),      # nine value rows in one tile
         ((0, 16, 0), 3, 257, 17, "Wm2"),         # the radiance in the second row tile
         ((0, 17, 0), 1, 257, 17, "nWcm2"),       # two parameter blocks: the instrument rows come from block 0 only
         ((5, 12, 3), 3, 700, 37, "Wm2"),
         ((0, 0, 0), 1, 257, 17, "Wm2")]          # no parameter: the radiance and the instrument rows alone


@pytest.mark.parametrize("kinds,n_gas,n,n_bands,units", CASES)
def test_instrument_rows_of_the_fused_call(eng, kinds, n_gas, n, n_bands, units):
    import test_gpu_state_bands as SB
    c = SB._case(eng, *kinds, n_gas, n)
    n_par = c["n_par"]
    P = R.panel(2975.0, 5e-4, n, n_bands, SEED)
    assert np.array_equal(P["grid"], c["grid"]) and len(P["centers"]) == n_bands
    assert "below the grid" in P["band_names"] or "above the grid" in P["band_names"]
    los = SB._los(eng, c)
    kw = c["kw"]
    if n_par:
        rad, _ = eng.limb_rays_state_jacobian(c["coeffs"], los, grid=c["grid"], **kw)
        kw_plain = kw
    else:    # no state call without a parameter: the radiance of a call with one column parameter (the same recursion)
        kw_plain = dict(par_gas=np.zeros(1, np.int32), par_w=np.ones((1, los.n_pt)), gas=0)
        rad, _ = eng.limb_rays_state_jacobian(c["coeffs"], los, grid=c["grid"], **kw_plain)
    rad_np = rad.cpu().numpy()
    assert np.all(np.isfinite(rad_np)) and np.count_nonzero(rad_np) > rad_np.size // 2
    factors = eng.fov_factors(SB.ROTS)
    for fov in (None, factors):
        band_kw = dict(out_units=units, fov=fov)
        got = eng.limb_rays_state_bands(c["coeffs"], los, c["grid"], P["centers"], P["widths"], instrument=True, **band_kw, **kw)
        n_out = 6 if fov is None else 2
        assert got.shape == (n_out, 1 + n_par + 2, n_bands)
        old = eng.limb_rays_state_bands(c["coeffs"], los, c["grid"], P["centers"], P["widths"], **band_kw, **kw_plain)
        if n_par:
            assert np.array_equal(got[:, :1 + n_par], old), "rows 0 .. n_par are not those of the call without the instrument rows"
        else:
            assert np.array_equal(got[:, 0], old[:, 0])
        again = eng.limb_rays_state_bands(c["coeffs"], los, c["grid"], P["centers"], P["widths"], instrument=True, **band_kw, **kw)
        assert np.array_equal(again, got)                       # (after a call with the other scratch layout in between)
        three = eng.hires_to_lowres_instrument(rad, c["grid"], P["centers"], P["widths"], out_units=units)
        comp = np.stack(three[1:], axis=1)
        if fov is not None:
            from spectrobot_amd import spect_main_module as smm
            comp = smm.fov_closed_form(comp[0::3], comp[1::3], comp[2::3], SB.ROTS)
        dead = R.band_reference(P["grid"], rad_np[:1], P["centers"], P["widths"])["count"] < 2
        assert dead.any() and np.all(got[:, :, dead] == 0.0)      # no trapezoid: an exact zero in EVERY row
        _hold("state bands instr %s n_gas %d n_pts %d %d bands %s fov %d" % (kinds, n_gas, n, n_bands, units, fov is not None),
              dict(fused=got[:, 1 + n_par:], composed=comp), rad_np, P, units, fov, SB.ROTS)


def test_two_level_gases_through_the_set(eng):
    """LevelFactoredSet.state_bands(instrument=True) on a scene with two LevelGas (HCN and CH4 on the level-factored
    route), Tvib nodes of both and VMR nodes: the rows of the call without the instrument rows bit for bit, the two
    instrument rows against the reference on LevelFactoredSet.state_jacobian's radiance, without and with the field of view."""
    import test_gpu_state_gases as SG
    from spectrobot_amd import retrieval, spect_main_module as smm
    n = 700
    scene, pixels = SG._scene(eng, n_grid=n, n_layers=22)
    pixels = pixels[:2]
    z = scene.z
    hcn_nodes, tv_nodes = SG._nodes(z)
    bs = smm.BayesSet()
    bs.add_set(retrieval.TvibProfile("CH4", 5, z, tv_nodes, np.full(4, 4.0), first_guess=np.array([1.0, -0.5, 0.7, 0.2])))
    bs.add_set(smm.LinearProfile_1D_new("HCN", z, hcn_nodes, np.full(3, 2.2e-6), np.full(3, 1.1e-6)))
    bs.add_set(retrieval.TvibProfile("HCN", 1, z, tv_nodes[:3], np.full(3, 4.0), first_guess=np.array([0.5, -1.0, 0.3])))
    retrieval._state_into_gases(scene, bs)
    alts = [a for p in pixels for a in p.los_alts()]
    rots = [p.pixel_rot for p in pixels]
    coeffs = scene.coefficient_stack()
    los, alt = scene.los(alts)
    w = scene.state_weights(bs, alt, several_level_gases=True)
    assert len(w.level_gases) == 2
    lfs = eng.LevelFactoredSet([(g.lf, i, g.rows, g.tvib) for g, i in zip(w.level_gases, w.gases)])
    P = R.panel(3290.0, 5e-4, n, 17, SEED)
    assert np.array_equal(P["grid"], scene.grid)
    args = (coeffs, los, w.par_lgas, w.par_level, w.par_w_lev)
    col = dict(par_gas=w.par_gas, par_w_col=w.par_w_col)
    rad, _ = lfs.state_jacobian(*args, **col)
    rad_np = rad.cpu().numpy()
    for fov in (None, eng.fov_factors(rots)):
        old = lfs.state_bands(*args, scene.grid, P["centers"], P["widths"], fov=fov, **col)
        got = lfs.state_bands(*args, scene.grid, P["centers"], P["widths"], fov=fov, instrument=True, **col)
        assert got.shape == ((6 if fov is None else 2), 1 + 10 + 2, 17) and np.array_equal(got[:, :11], old)
        comp = np.stack(eng.hires_to_lowres_instrument(rad, scene.grid, P["centers"], P["widths"])[1:], axis=1)
        if fov is not None:
            comp = smm.fov_closed_form(comp[0::3], comp[1::3], comp[2::3], rots)
        dead = R.band_reference(P["grid"], rad_np[:1], P["centers"], P["widths"])["count"] < 2
        assert dead.any() and np.all(got[:, :, dead] == 0.0)
        _hold("two level gases, 700 pts, 17 bands, fov %d" % (fov is not None), dict(fused=got[:, 11:], composed=comp), rad_np, P, "Wm2",
              fov, rots)


def test_a_refused_call_leaves_out_untouched(eng):
    """The library's refusals of the band arguments, after a valid call has put the scratch and the weight cache in place:
    status SR_ERR_ARG and `out` keeps its sentinel."""
    import test_gpu_state_bands as SB
    from spectrobot_amd import _lib
    c = SB._case(eng, 2, 3, 0, 1, 257)
    P = R.panel(2975.0, 5e-4, 257, 17, SEED)
    los = SB._los(eng, c)
    good = eng.limb_rays_state_bands(c["coeffs"], los, c["grid"], P["centers"], P["widths"], instrument=True, **c["kw"])
    kw = c["kw"]
    A = eng._state_args(c["coeffs"], los, kw["par_gas"], kw["par_w"], kw["tab"], kw["coef_row"], kw["par_level"], kw["par_c"], kw["gas"],
                        c["grid"], 0, None, None)
    w0, step, _ = eng.grid_params(c["grid"])
    A.desc.w0, A.desc.step = w0, step
    out = np.full(good.shape, -7.25)
    cen = np.ascontiguousarray(P["centers"])

    def call(widths=P["widths"], n_bands=17, n_sigma=5.0, units=0, o=out):
        wid = np.ascontiguousarray(widths, dtype=np.float64)
        return _lib.lib.sr_limb_rays_state_bands_instr_dev(*A.args("sr_limb_rays_state_bands_instr_dev", cen.ctypes.data_as(_lib.dp),
                                                                   wid.ctypes.data_as(_lib.dp), n_bands, n_sigma, units, None,
                                                                   None if o is None else o.ctypes.data_as(_lib.dp), None))

    bad_w = P["widths"].copy()
    bad_w[5] = 0.0
    for kw_bad in (dict(widths=bad_w), dict(n_bands=0), dict(n_sigma=-5.0), dict(units=3), dict(o=None)):
        assert call(**kw_bad) == _lib.SR_ERR_ARG, kw_bad
    assert np.all(out == -7.25)
    assert call() == _lib.SR_OK and np.array_equal(out, good)
