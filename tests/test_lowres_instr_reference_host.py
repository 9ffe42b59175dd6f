"""The instrument derivatives of the band integrals (band centre, ILS width) checked on the host, no GPU: the
extended-precision reference of tests/lowres_instr_reference.py against long-double central differences of the value's
reference, its plain-fp64 yardstick K_PLAIN_INSTR recorded and respected, exact zeros where there is no trapezoid, seeded
defects beyond the kernels' limit, the ABI surface and the host-side refusals of the three new entry points, the chain rule
and the band arithmetic of retrieval.BandCalibration, and the refusal of the "instr" set by the loops that do not take it."""
import ctypes as C

import numpy as np
import pytest

import lowres_reference as R
import lowres_instr_reference as I


@pytest.fixture(scope="module")
def problem():
    P = R.panel(*I.K_PLAIN_INSTR_PANEL)
    P["ref"] = I.band_reference_instr(P["grid"], P["spec"], P["centers"], P["widths"])
    P["plain"] = I.plain_fp64_instr(P["grid"], P["spec"], P["centers"], P["widths"])
    return P


def test_k_plain_instr_is_recorded_and_respected(problem):
    k, where = I.measure_k_plain_instr(problem)
    print("K_PLAIN_INSTR: live %.3g at %s; recorded %.3g (measured %.3g)" % (k, where, I.K_PLAIN_INSTR, I.K_PLAIN_INSTR_MEASURED))
    assert k <= I.K_PLAIN_INSTR
    assert I.K_PLAIN_INSTR <= 2.0 * I.K_PLAIN_INSTR_MEASURED
    assert abs(I.K_PLAIN_INSTR - 1.5 * I.K_PLAIN_INSTR_MEASURED) < 1e-12
    # row 0 of the three-row reference is the value's reference itself
    ref0 = R.band_reference(problem["grid"], problem["spec"][:2], problem["centers"], problem["widths"])
    assert np.array_equal(problem["ref"]["value"][:2, 0], ref0["value"]) and np.array_equal(problem["ref"]["A"][:2, 0], ref0["A"])


def test_derivatives_equal_central_differences_of_the_value(problem):
    """Long-double central differences of band_reference in delta (f -> f + delta) and eta (w -> w e^eta) over the panel's
    bands whose guard is >= 1e-2, to 1e-9 of the derivative's own A.  Per band the outermost point of the stencil moves no
    window end by more than a quarter of its guard (in units of the smallest grid spacing: asserted from guard(), and the
    windows' counts are compared), so every evaluation sums the same points.
    The differences are the five-point central ones, (-v(2h) + 8 v(h) - 8 v(-h) + v(-2h)) / (12 h) with the weights
    taken for the nodes actually reached, h <= 2^-10 w (delta) or 2^-12 (eta).  The three-point difference cannot meet the bound on this panel: the one-hot probe in the middle of the
    3-point window has |t| = 8e-7, its A (proportional to |t|) is that small, and the long-double rounding of the
    difference, 2^-64 |W| / h, is 4e-9 of it at h = 2^-18 w and grows as h shrinks, while the step^2 truncation,
    (h / w)^2 / 4, forbids h > 2^-15 w.  With the h^4 truncation -- a ratio of Hermite polynomials (<= 25 for delta,
    <= 1.5e4 for eta at |t| = 5) times h^4 / 30: 1e-12 and 2e-12 -- the step may be large enough for the rounding to fall to
    4e-11 of A (measured: 3.5e-11, 4e-13)."""
    P = problem
    grid, cen, wid, ns = P["grid"], P["centers"], P["widths"], P["n_sigma"]
    ref = P["ref"]
    ok = (ref["guard"] >= 1e-2) & (ref["count"] >= 2)
    assert ok.sum() >= 20
    x = 1e7 / grid[::-1]
    sp_min = np.diff(x).min()
    move = 0.25 * ref["guard"] * sp_min                     # what a window end may move, nm
    LD = R.LD
    for which, row in (("centre", 1), ("width", 2)):
        if which == "centre":
            h = 2.0 ** np.floor(np.log2(np.minimum(wid * 2.0 ** -10, move / 2.0)))   # a power of two: f + m h is exact
            at = lambda m: (cen + m * h, wid)
            coord = lambda c, w: c.astype(LD)               # the coordinate actually reached, nm
            end_move = 2.0 * h
        else:
            h = np.minimum(2.0 ** -12, np.log1p(move / (ns * wid)) / 2.0)
            at = lambda m: (cen, wid * np.exp(m * h))
            coord = lambda c, w: np.log(w.astype(LD))
            end_move = ns * wid * np.expm1(2.0 * h)
        # no window end crosses a grid point: from guard(), and seen in the counts
        assert np.all(end_move[ok] <= 0.26 * ref["guard"][ok] * sp_min)
        val, pos = {}, {}
        for m in (-2, -1, 1, 2):
            c, w = at(m)
            assert np.all(R.guard(grid, c, w, ns)[ok] >= 0.7 * ref["guard"][ok])
            got = R.band_reference(grid, P["spec"], c, w, ns)
            assert np.array_equal(got["count"][ok], ref["count"][ok])
            val[m], pos[m] = got["value"], coord(c, w)
        # the stencil's weights for the nodes actually reached (fp64 centres and widths: f + m h is exact, w e^(m h) is
        # rounded), about the band's own coordinate: Lagrange's, c_m = sum_(j != m) prod_(k != m, j) (-z_k) / prod_(k != m) (z_m - z_k)
        z = dict((m, pos[m] - coord(cen, wid)) for m in pos)
        fd = np.zeros_like(val[1])
        for m in z:
            others = [k for k in z if k != m]
            num = sum(np.prod([-z[k] for k in others if k != j], axis=0) for j in others)
            fd = fd + val[m] * (num / np.prod([z[m] - z[k] for k in others], axis=0))[None, :]
        with np.errstate(under="ignore"):
            err = np.abs(fd - ref["value"][:, row]) / (ref["A"][:, row] + LD(R.FLOOR) / LD(R.EPS53))
        worst = float(err[:, ok].max())
        print("central differences, %s: worst %.3g of A" % (which, worst))
        assert worst <= 1e-9


def test_no_trapezoid_no_derivative(problem):
    """A window of fewer than two points and a band that misses the grid are exact zeros in all three rows, in the
    reference and in the plain evaluation."""
    P = problem
    none = P["ref"]["count"] < 2
    names = [n for n, z in zip(P["band_names"], none) if z]
    assert "below the grid" in names and "above the grid" in names and "1-point window" in names
    for got in (P["ref"]["value"], P["plain"]):
        assert np.all(np.asarray(got[:, :, none], np.float64) == 0.0)
    # and a shard that a band misses: partial sums of exact zeros
    lo = I.band_reference_instr(P["grid"], P["spec"][:2, :64], P["centers"], P["widths"], g_lo=0)
    assert np.all(np.asarray(lo["value"][:, :, lo["count"] < 2], np.float64) == 0.0) and (lo["count"] < 2).sum() > none.sum()


def test_shard_partials_add_up(problem):
    """The rows are partial sums over a shard's own trapezoids: two shards that share point 4097 add up to the whole to
    2^-5 units (long-double roundings)."""
    P = problem
    spec = P["spec"][:2]
    a = I.band_reference_instr(P["grid"], spec[:, :4098], P["centers"], P["widths"], g_lo=0)
    b = I.band_reference_instr(P["grid"], spec[:, 4097:], P["centers"], P["widths"], g_lo=4097)
    u = R.units_raw(np.asarray(a["value"] + b["value"]), P["ref"]["value"][:2], P["ref"]["A"][:2])
    # (only bands whose window lies wholly on one side or spans the cut with both ends inside a shard are sums of the
    # same trapezoids; a window END inside the other shard changes nothing either: the ends are on the fp64 grid values)
    assert u.max() <= 2.0 ** -5


@pytest.mark.parametrize("defect", I.DEFECTS)
def test_seeded_defects_exceed_the_limit(problem, defect):
    P = problem
    k_plain = I.units_of(P["plain"], P["ref"])[:, 1:].max()
    lim = R.limit(k_plain)
    u = I.units_of(I.plain_fp64_instr(P["grid"], P["spec"], P["centers"], P["widths"], defect=defect), P["ref"])
    print("%s: limit %.3g, centre %.3g, width %.3g units" % (defect, lim, u[:, 1].max(), u[:, 2].max()))
    assert I.units_of(P["plain"], P["ref"]).max() <= lim
    assert max(u[:, 1].max(), u[:, 2].max()) > lim
    if defect in ("t_sign", "missing_inverse_width"):
        assert u[:, 1].max() > lim and u[:, 2].max() <= lim
    if defect == "t2_without_minus_one":
        assert u[:, 2].max() > lim and u[:, 1].max() <= lim


# ----------------------------------------------------------------------------------------------------------------------
# the library's surface
# ----------------------------------------------------------------------------------------------------------------------
def test_abi_surface_of_the_three_entry_points():
    from spectrobot_amd import _lib
    S = _lib.SYMBOLS
    assert S["sr_hires_to_lowres_instr_shard_dev"] == S["sr_hires_to_lowres_shard_dev"]
    assert S["sr_limb_rays_state_bands_instr_dev"] == S["sr_limb_rays_state_bands_dev"]
    assert S["sr_limb_rays_state_bands_instr_gases_dev"] == S["sr_limb_rays_state_bands_gases_dev"]
    for name in ("sr_hires_to_lowres_instr_shard_dev", "sr_limb_rays_state_bands_instr_dev", "sr_limb_rays_state_bands_instr_gases_dev"):
        assert hasattr(_lib.lib, name) and S[name][0] is C.c_int
    assert _lib.lib.sr_abi_version() == 1
    text = open(_lib.__file__.replace("spectrobot_amd/_lib.py", "include/spectrobot_hip.h")).read()
    for name in ("sr_hires_to_lowres_instr_shard_dev(", "sr_limb_rays_state_bands_instr_dev(", "sr_limb_rays_state_bands_instr_gases_dev("):
        assert text.count("int " + name) == 1


def test_refused_arguments_of_the_instrument_step_leave_out_untouched():
    """sr_hires_to_lowres_instr_shard_dev refuses what sr_hires_to_lowres_shard_dev refuses, with its status codes, before
    any device call (the spectrum below is no device memory), and `out` keeps its sentinel."""
    from spectrobot_amd import _lib
    dp = _lib.dp
    cen, wid = np.array([3331.0, 3332.0]), np.array([0.5, 0.5])
    out = np.full((3, 3, 2), -7.25)
    fake = C.c_void_p(4096)

    def call(fn, rad=fake, n_rays=3, n_pts=10, g_lo=0, w0=3000.0, step=5e-4, c=cen, w=wid, n_bands=2, n_sigma=5.0, units=0, o=out):
        w = None if w is None else np.ascontiguousarray(w, dtype=np.float64)
        return fn(rad, n_rays, n_pts, g_lo, w0, step, None if c is None else c.ctypes.data_as(dp),
                  None if w is None else w.ctypes.data_as(dp), n_bands, n_sigma, units, None if o is None else o.ctypes.data_as(dp), None)

    refused = [dict(rad=None), dict(o=None), dict(c=None), dict(w=None), dict(n_rays=0), dict(n_rays=-1), dict(n_pts=1), dict(n_bands=0),
               dict(g_lo=-1), dict(step=0.0), dict(step=-5e-4), dict(w0=0.0), dict(n_sigma=0.0), dict(units=-1), dict(units=3),
               dict(w=[0.5, 0.0]), dict(w=[np.nan, 0.5])]
    for fn in (_lib.lib.sr_hires_to_lowres_instr_shard_dev, _lib.lib.sr_hires_to_lowres_shard_dev):
        for kw in refused:
            assert call(fn, **kw) == _lib.SR_ERR_ARG, kw
        assert call(fn, n_pts=2000001) == _lib.SR_ERR_LIMIT
        assert call(fn, g_lo=1999995) == _lib.SR_ERR_LIMIT
    assert np.all(out == -7.25)


def test_refused_arguments_of_the_fused_call_and_no_parameter_at_all():
    """sr_limb_rays_state_bands_instr_dev makes sr_limb_rays_state_bands_dev's checks before any device call -- except that
    no parameter at all is no refusal there: with n_col = n_lev = n_row = 0 the next check answers."""
    from spectrobot_amd import _lib
    ip, dp = _lib.ip, _lib.dp
    n_layers, n_pts, n_bands = 4, 10, 3
    so, sl, po = np.array([0, 2, 4, 6], np.int32), np.array([1, 3, 1, 3, 2, 3], np.int32), np.arange(0, 13, 2, dtype=np.int32)
    xx, one = np.tile([0.0, 1.0], 6), np.ones(24)
    d = _lib.LosDesc()
    d.n_rays, d.n_gas = 3, 2
    d.seg_off, d.seg_layer, d.pt_off = (a.ctypes.data_as(ip) for a in (so, sl, po))
    d.x, d.nd, d.vmr = xx.ctypes.data_as(dp), one.ctypes.data_as(dp), one.ctypes.data_as(dp)
    d.w0, d.step, d.g_lo, d.init_mode = 3000.0, 5e-4, 0, 0
    fake = C.c_void_p(4096)
    cen, wid = np.array([3331.0, 3332.0, 3333.0]), np.array([0.5, 0.5, 0.5])
    out = np.full((3, 3, n_bands), -7.25)

    def call(fn, n_bands=n_bands, n_pts=n_pts, widths=wid, units=0):
        w = np.ascontiguousarray(widths, dtype=np.float64)
        return fn(fake, fake, n_layers, n_pts, C.byref(d), 0, None, None, 0, None, 1, 1, None, 0, None, None, None, None, 0, None,
                  cen.ctypes.data_as(dp), w.ctypes.data_as(dp), n_bands, 5.0, units, None, out.ctypes.data_as(dp), None)

    plain, instr = _lib.lib.sr_limb_rays_state_bands_dev, _lib.lib.sr_limb_rays_state_bands_instr_dev
    assert call(plain) == _lib.SR_ERR_ARG                                   # no parameters: refused as ever
    assert call(plain, n_pts=2000001) == _lib.SR_ERR_ARG
    assert call(instr, n_pts=2000001) == _lib.SR_ERR_LIMIT                  # ... not here: the next check answers
    for kw in (dict(n_bands=0), dict(widths=[0.5, 0.0, 0.5]), dict(units=3), dict(n_pts=1)):
        assert call(instr, **kw) == _lib.SR_ERR_ARG, kw
    assert np.all(out == -7.25)


# ----------------------------------------------------------------------------------------------------------------------
# the retrieval set
# ----------------------------------------------------------------------------------------------------------------------
def _scene(bands, widths):
    from spectrobot_amd import retrieval as rt
    sc = object.__new__(rt.LimbScene)
    sc.gases = []
    sc.bands_nm, sc.widths_nm = np.array(bands, float), np.array(widths, float)
    sc.bands_nm0, sc.widths_nm0 = sc.bands_nm.copy(), sc.widths_nm.copy()
    return sc


def test_band_calibration_arithmetic_and_chain_rule():
    from spectrobot_amd import retrieval as rt, spect_main_module as smm
    b0, w0 = np.array([3300.0, 3316.5, 3333.0, 3351.0]), np.array([6.0, 6.5, 7.0, 7.5])
    bc = rt.BandCalibration(shift=(0.0, 2.0, 0.75), slope=(0.0, 0.01, -0.002), ln_width=(0.0, 0.05, 0.03))
    assert bc.name == "instr" == rt.INSTR_SET and [p.key for p in bc.set] == ["shift", "slope", "ln_width"] and bc.n_par == 3
    assert not any(p.constrain_positive for p in bc.set) and [p.apriori_err for p in bc.set] == [2.0, 0.01, 0.05]
    bs = smm.BayesSet()
    bs.add_set(bc)
    sc = _scene(b0, w0)
    rt._state_into_gases(sc, bs)
    assert np.array_equal(sc.bands_nm, b0 + 0.75 + (-0.002) * (b0 - b0.mean()))
    assert np.array_equal(sc.widths_nm, w0 * np.exp(0.03))
    assert np.array_equal(sc.bands_nm0, b0) and np.array_equal(sc.widths_nm0, w0)
    # a second call starts from the nominal bands again, not from the moved ones
    rt._state_into_gases(sc, bs)
    assert np.array_equal(sc.bands_nm, b0 + 0.75 + (-0.002) * (b0 - b0.mean()))
    # any subset; what is off stands at zero
    only = rt.BandCalibration(ln_width=(0.0, 0.05, 0.1))
    assert [p.key for p in only.set] == ["ln_width"] and only.value("shift") == 0.0
    f, w = only.bands(b0, w0)
    assert np.array_equal(f, b0) and np.array_equal(w, w0 * np.exp(0.1))
    with pytest.raises(ValueError):
        rt.BandCalibration()
    # the chain rule against central differences of a smooth band model through bands()
    model = lambda f, w: np.sin(f / 50.0) * w ** 2 + 0.1 * f
    st = bs.sets["instr"]
    f, w = st.bands(b0, w0)
    d_centre = np.cos(f / 50.0) / 50.0 * w ** 2 + 0.1
    d_lnw = 2.0 * np.sin(f / 50.0) * w ** 2
    rows = st.jacobian_rows(b0, np.stack([d_centre, 2 * d_centre]), np.stack([d_lnw, 2 * d_lnw]))
    assert rows.shape == (2, 3, 4) and np.array_equal(rows[1], 2 * rows[0])
    for k, (par, h) in enumerate(zip(st.set, (1e-4, 1e-7, 1e-6))):
        v = par.value
        par.value = v + h
        up = model(*st.bands(b0, w0))
        par.value = v - h
        dn = model(*st.bands(b0, w0))
        par.value = v
        fd = (up - dn) / (2 * h)
        assert np.allclose(rows[0, k], fd, rtol=1e-7, atol=1e-7 * np.abs(fd).max()), par.key
    # two of three, in the set's order
    two = rt.BandCalibration(shift=(0.0, 1.0), ln_width=(0.0, 0.1))
    r2 = two.jacobian_rows(b0, d_centre, d_lnw)
    assert r2.shape == (2, 4) and np.array_equal(r2[0], d_centre) and np.array_equal(r2[1], d_lnw)


def test_state_weights_accepts_the_name():
    from spectrobot_amd import retrieval as rt, spect_main_module as smm
    sc = _scene([3300.0, 3333.0], [6.0, 7.0])
    sc.z = np.array([0.0, 50.0, 100.0])
    bs = smm.BayesSet()
    bs.add_set(rt.BandCalibration(shift=(0.0, 1.0), ln_width=(0.0, 0.1)))
    w = sc.state_weights(bs, np.zeros(1), several_level_gases=True)
    assert len(w.perm) == 0 and w.par_gas.size == 0 and w.par_level.size == 0 and w.par_w_temp.shape[0] == 0
    other = smm.BayesSet()
    other.add_set(smm.RetSet("instrument", []))
    with pytest.raises(ValueError, match="names neither a gas"):
        sc.state_weights(other, np.zeros(1))


def test_the_unextended_loops_refuse_the_set_by_name():
    from spectrobot_amd import retrieval as rt, spect_main_module as smm
    bs = smm.BayesSet()
    bs.add_set(rt.BandCalibration(shift=(0.0, 1.0)))
    for who, call in (("inversion_fast_limb", lambda: rt.inversion_fast_limb(None, bs, [])),
                      ("inversion", lambda: rt.inversion(None, bs, [])),
                      ("sr_retrieval_forward_dev", lambda: rt.simulate(None, [], bayes_set=bs, arrays=True))):
        with pytest.raises(ValueError, match="'instr'") as e:
            call()
        assert who in str(e.value)
    import inspect
    for fn in (rt.inversion_state,):
        assert "instr" in inspect.getdoc(fn)
    for name in ("instrument",):
        from spectrobot_amd import engine
        assert inspect.signature(engine.limb_rays_state_bands).parameters[name].default is False
        assert inspect.signature(engine.LevelFactored.state_bands).parameters[name].default is False
        assert inspect.signature(engine.LevelFactoredSet.state_bands).parameters[name].default is False
