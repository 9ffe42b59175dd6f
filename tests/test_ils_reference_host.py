"""Tabulated instrument line shapes checked on the host, no GPU: the extended-precision reference of tests/ils_reference.py
-- its plain-fp64 yardstick K_PLAIN_ILS recorded and respected, seeded defects beyond the kernels' limit, the Gaussian as a
table against the closed-form Gaussian's reference, the two derivative rows against long-double central differences of the
value --, engine.ILS (normalisation, per-band tables, refusals), the ABI surface and the refusals of sr_set_ils and
sr_ils_area, the ils= keyword of every band call, and the host build of the weights kernel under the sanitizers."""
import ctypes as C
import inspect
import os
import subprocess

import numpy as np
import pytest

import lowres_reference as R
import ils_reference as S


@pytest.fixture(scope="module")
def problem():
    """The panel under one lobed table per band."""
    P = R.panel(*S.K_PLAIN_ILS_PANEL)
    P["ils"] = S.lobed_tables(len(P["centers"]))
    P["ref"] = S.band_reference_ils(P["grid"], P["spec"], P["centers"], P["widths"], *P["ils"])
    P["plain"] = S.plain_fp64_ils(P["grid"], P["spec"], P["centers"], P["widths"], *P["ils"])
    return P


@pytest.fixture(scope="module")
def ends():
    """The three exact bands (window end on a grid point, twice; a grid point on a knot) under the skewed table on
    [-5, 3], whose ends are not small."""
    n_pts, k = 300, 130
    g, _ = R.make_grid(S.GRID[0], S.GRID[1], n_pts)
    t_lo, t_hi, phi = S.skewed_table()
    t_knot = t_lo + 20 * 0.125
    centers, widths, xk = S.exact_cases(g, k, t_lo, t_hi, t_knot)
    rng = np.random.default_rng([20261019, n_pts, k])
    spec = np.zeros((5, n_pts))
    spec[0, k] = spec[1, k - 1] = spec[2, k + 1] = 1.0
    spec[3] = rng.uniform(0.5, 1.5, n_pts)
    spec[4] = rng.choice([-1.0, 1.0], n_pts) * 10.0 ** rng.uniform(-6.0, 0.0, n_pts)
    E = dict(grid=g, centers=centers, widths=widths, xk=xk, k=k, spec=spec, ils=(t_lo, t_hi, phi), t_knot=t_knot)
    E["ref"] = S.band_reference_ils(g, spec, centers, widths, t_lo, t_hi, phi)
    E["plain"] = S.plain_fp64_ils(g, spec, centers, widths, t_lo, t_hi, phi)
    return E


def test_k_plain_ils_is_recorded_and_respected(problem):
    k, where = S.measure_k_plain_ils(problem)
    print("K_PLAIN_ILS: live %.4g at %s; recorded %.4g (measured %.4g)" % (k, where, S.K_PLAIN_ILS, S.K_PLAIN_ILS_MEASURED))
    assert k <= S.K_PLAIN_ILS
    assert S.K_PLAIN_ILS <= 2.0 * S.K_PLAIN_ILS_MEASURED
    assert abs(S.K_PLAIN_ILS - 1.5 * S.K_PLAIN_ILS_MEASURED) < 1e-9
    # dead bands: exact zeros in all three rows, in the reference and in the plain evaluation
    none = problem["ref"]["count"] < 2
    names = [n for n, z in zip(problem["band_names"], none) if z]
    assert "below the grid" in names and "above the grid" in names and "1-point window" in names
    for got in (problem["ref"]["value"], problem["plain"]):
        assert np.all(np.asarray(got[:, :, none], np.float64) == 0.0)
    # with t_lo, t_hi = -+5 the windows are those of the Gaussian's panel
    assert np.array_equal(problem["ref"]["count"], R.band_reference(problem["grid"], problem["spec"][:1], problem["centers"],
                                                                    problem["widths"])["count"])


def test_exact_ends_and_knots_in_the_reference(ends):
    """The end point belongs to the window, its neighbour outside does not; at t = t_lo, t = t_hi and on an interior knot
    the value's weight is p phi_k / w: the reference says so to long-double precision, the plain evaluation to its limit."""
    E = ends
    t_lo, t_hi, phi = E["ils"]
    c, w, xk = E["centers"], E["widths"], E["xk"]
    assert c[0] + t_lo * w[0] == xk and c[1] + t_hi * w[1] == xk and (xk - c[2]) / w[2] == E["t_knot"] and xk == 1e7 / E["grid"][E["k"]]
    ref = E["ref"]
    v = np.asarray(ref["value"], np.float64)
    assert np.all(ref["count"] >= 2)
    # one-hot at k + 1 has the smaller x (cm-1 index up, nm down): outside band 0's window; k - 1 outside band 1's
    assert np.all(v[2, :, 0] == 0.0) and np.all(v[1, :, 1] == 0.0) and v[0, 0, 0] != 0.0 and v[0, 0, 1] != 0.0
    x = (1e7 / E["grid"]).astype(R.LD)
    g = E["grid"].astype(R.LD)
    k = E["k"]
    kf = R.unit_factor("Wm2")
    for b, knot, xl, xr in ((0, 0, x[k], x[k - 1]), (1, phi.shape[1] - 1, x[k + 1], x[k]), (2, 20, x[k + 1], x[k - 1])):
        want = kf * g[k] * g[k] * R._ten(-7) * (xr - xl) / R.LD(2) * R.LD(phi[0, knot]) / R.LD(w[b])
        assert abs(ref["value"][0, 0, b] - want) <= 1e-17 * abs(want), (b, knot)
    lim = R.limit(S.units_of(E["plain"], ref).max())
    print("exact ends: plain fp64 %.3g units, limit %.3g" % (S.units_of(E["plain"], ref).max(), lim))
    assert S.units_of(E["plain"], ref).max() <= S.K_PLAIN_ILS


@pytest.mark.parametrize("defect", S.DEFECTS)
def test_seeded_defects_exceed_the_limit(problem, ends, defect):
    """Every defect is beyond 8 x max(K_PLAIN_ILS over the pairs, 1) on the problem that can show it: the table's end and the
    window's ends need the table whose ends are not small and the bands whose ends sit on grid points."""
    on_ends = defect in ("unclamped_last_knot", "window_from_n_sigma")
    Q = ends if on_ends else problem
    lim = R.limit(S.units_of(Q["plain"], Q["ref"]).max())
    u = S.units_of(S.plain_fp64_ils(Q["grid"], Q["spec"], Q["centers"], Q["widths"], *Q["ils"], defect=defect), Q["ref"])
    print("%s: limit %.3g, value %.3g, centre %.3g, width %.3g units" % (defect, lim, u[:, 0].max(), u[:, 1].max(), u[:, 2].max()))
    assert S.units_of(Q["plain"], Q["ref"]).max() <= lim
    assert u.max() > lim
    if defect in ("centre_row_sign", "missing_inverse_width"):
        assert u[:, 1].max() > lim and u[:, 0].max() <= lim and u[:, 2].max() <= lim
    if defect == "width_row_without_t_dphi":
        assert u[:, 2].max() > lim and u[:, 0].max() <= lim and u[:, 1].max() <= lim
    if defect in ("one_sided_slopes_everywhere", "band_b_gets_table_0", "window_from_n_sigma", "unclamped_last_knot"):
        assert u[:, 0].max() > lim
    if defect == "unclamped_last_knot":       # the one-hot spectrum at t = t_hi exactly, under the band whose upper end it is
        assert u[0, 0, 1] > lim


def test_gaussian_table_against_the_closed_form():
    rel = S.gaussian_agreement()
    print("gaussian table n_tab %d: value %.3g (floor %.3g), centre %.3g, width %.3g of the row's maximum; recorded %s"
          % (S.GAUSS_TAB[0], rel[0], S.GAUSS_VALUE_FLOOR, rel[1], rel[2], S.GAUSS_ROW_MEASURED))
    import math
    assert abs(S.GAUSS_VALUE_FLOOR - math.erfc(5.0 / math.sqrt(2.0))) < 1e-18
    assert rel[0] <= S.GAUSS_VALUE_FLOOR
    assert rel[1] <= 2.0 * S.GAUSS_ROW_MEASURED[0] and rel[2] <= 2.0 * S.GAUSS_ROW_MEASURED[1]
    coarse = S.gaussian_agreement(161)
    assert np.all(coarse[1:] > 2.0 * rel[1:])                 # the derivative rows converge with n_tab


def test_derivative_rows_equal_central_differences_of_the_value():
    out = S.fd_check()
    for name, (excess, miss) in zip(("centre", "width"), out):
        print("central differences, %s: |row - FD(h/2)| %.3g, over 2 |FD(h) - FD(h/2)| by %.3g of max|row| (eps %.3g)" % (name, miss, excess, S.FD_EPS))
        assert excess <= S.FD_EPS
    assert S.FD_EPS == 2.0 * S.FD_EPS_MEASURED


def test_shard_partials_add_up(problem):
    P = problem
    spec = P["spec"][:2]
    a = S.band_reference_ils(P["grid"], spec[:, :4098], P["centers"], P["widths"], *P["ils"], g_lo=0)
    b = S.band_reference_ils(P["grid"], spec[:, 4097:], P["centers"], P["widths"], *P["ils"], g_lo=4097)
    u = R.units_raw(np.asarray(a["value"] + b["value"]), P["ref"]["value"][:2], P["ref"]["A"][:2])
    assert u.max() <= 2.0 ** -5


# ----------------------------------------------------------------------------------------------------------------------
# engine.ILS and the library's surface
# ----------------------------------------------------------------------------------------------------------------------
def test_engine_ils_normalises_and_keeps_per_band_tables():
    from spectrobot_amd import engine
    t = np.linspace(-5.0, 3.0, 65)
    raw = np.exp(-0.5 * t * t) * (1.0 + 0.3 * np.tanh(t))
    one = engine.ILS(-5.0, 3.0, raw)
    assert (one.n_shapes, one.n_tab, one.per_band) == (1, 65, False) and one.phi.shape == (1, 65)
    assert abs(one.area()[0] - 1.0) <= 4 * np.finfo(float).eps and abs(engine.ILS(-5.0, 3.0, 7.5 * raw).area()[0] - 1.0) <= 4 * np.finfo(float).eps
    assert np.array_equal(one.phi, S.skewed_table()[2])       # the helper's normalisation, written on its own
    many = engine.ILS(-5.0, 3.0, np.stack([raw, 2.0 * raw + 0.1, raw[::-1]]))
    assert (many.n_shapes, many.per_band) == (3, True) and np.all(np.abs(many.area() - 1.0) <= 4 * np.finfo(float).eps)
    assert np.array_equal(many.phi[0], one.phi[0]) and not np.array_equal(many.phi[1], many.phi[0])
    assert np.array_equal(many.select([2, 0, 0, 1]).phi, many.phi[[2, 0, 0, 1]]) and one.select([3, 1]) is one
    asis = engine.ILS(-5.0, 3.0, raw, normalize=False)
    assert np.array_equal(asis.phi[0], raw)
    area = asis.area()[0]
    assert abs(area - float(engine.ILS.interpolant_area(-5.0, 3.0, raw)[0])) <= 4 * np.finfo(float).eps * area
    # the interpolant reproduces a straight line (the central and the one-sided differences are its slope): area 2 + 2
    line = engine.ILS(0.0, 2.0, 1.0 + np.linspace(0.0, 2.0, 9), normalize=False)
    assert abs(line.area()[0] - 4.0) <= 1e-15
    # the constructors
    g = engine.ILS.gaussian()
    assert (g.n_tab, g.t_lo, g.t_hi) == (641, -5.0, 5.0) and np.array_equal(g.phi, S.gaussian_table()[2])
    assert abs(g.area()[0] - (1.0 - S.GAUSS_VALUE_FLOOR)) < 1e-9
    sc = engine.ILS.sinc(4, 129)
    assert (sc.t_lo, sc.t_hi) == (-4.0, 4.0) and sc.phi.min() < 0 and abs(sc.area()[0] - 1.0) <= 4 * np.finfo(float).eps
    ap = engine.ILS.sinc(4, 129, apodisation=lambda u: 1.0 - np.abs(u))
    assert abs(ap.phi.min()) < abs(sc.phi.min()) and abs(ap.area()[0] - 1.0) <= 4 * np.finfo(float).eps
    fn = engine.ILS.from_function(lambda tt: np.exp(-np.abs(tt)), -6.0, 6.0, 97)
    assert fn.n_tab == 97 and abs(fn.area()[0] - 1.0) <= 4 * np.finfo(float).eps


def test_engine_ils_refusals():
    from spectrobot_amd import engine
    ok = np.array([0.0, 1.0, 2.0, 1.0, 0.0])
    for bad in (dict(phi=ok[:3]), dict(phi=np.zeros((2, 2, 5))), dict(t_lo=1.0, t_hi=1.0), dict(t_lo=2.0, t_hi=1.0),
                dict(t_hi=np.inf), dict(phi=[0.0, 1.0, np.nan, 1.0, 0.0]), dict(phi=-ok), dict(phi=[1.0, -1.0, 0.0, -1.0, 1.0]),
                dict(phi=np.zeros(_max_tab() + 1) + 1.0)):
        kw = dict(t_lo=-1.0, t_hi=1.0, phi=ok)
        kw.update(bad)
        with pytest.raises(ValueError):
            engine.ILS(**kw)
    engine.ILS(-1.0, 1.0, -ok, normalize=False)               # as given: the sign is the caller's
    with pytest.raises(TypeError):
        engine._IlsBound((-1.0, 1.0, ok))


def _max_tab():
    from spectrobot_amd import _lib
    return _lib.SR_MAX_ILS_TAB


def _probe():
    """What a band call says to n_pts beyond the limit with 2 bands: SR_ERR_LIMIT under the Gaussian or a table that fits,
    SR_ERR_ARG under a table for another number of bands.  Refused before any device call either way."""
    from spectrobot_amd import _lib
    cen, wid, out = np.array([3331.0, 3332.0]), np.array([0.5, 0.5]), np.full((3, 2), -7.25)
    rc = _lib.lib.sr_hires_to_lowres_shard_dev(C.c_void_p(4096), 3, 2000001, 0, 3000.0, 5e-4, cen.ctypes.data_as(_lib.dp),
                                               wid.ctypes.data_as(_lib.dp), 2, 5.0, 0, out.ctypes.data_as(_lib.dp), None)
    assert np.all(out == -7.25)
    return rc


def test_set_ils_surface_refusals_and_binding():
    from spectrobot_amd import _lib
    lib, dp = _lib.lib, _lib.dp
    assert _lib.SYMBOLS["sr_set_ils"] == (C.c_int, [C.POINTER(_lib.IlsDesc)])
    assert _lib.SYMBOLS["sr_ils_area"] == (C.c_int, [C.POINTER(_lib.IlsDesc), dp])
    assert hasattr(lib, "sr_set_ils") and hasattr(lib, "sr_ils_area") and lib.sr_abi_version() == 1
    text = open(_lib.__file__.replace("spectrobot_amd/_lib.py", "include/spectrobot_hip.h")).read()
    assert text.count("int sr_set_ils(") == 1 and text.count("int sr_ils_area(") == 1 and text.count("} sr_ils_desc;") == 1
    assert "#define SR_MAX_ILS_TAB %d" % _lib.SR_MAX_ILS_TAB in text
    phi = np.linspace(0.0, 1.0, 5 * 6).reshape(5, 6) + 0.5
    big = np.ones(_lib.SR_MAX_ILS_TAB + 1)

    def desc(n_shapes=5, n_tab=6, t_lo=-2.0, t_hi=2.0, p=phi):
        return _lib.IlsDesc(n_shapes, n_tab, t_lo, t_hi, None if p is None else p.ctypes.data_as(dp))

    nan = phi.copy()
    nan[4, 5] = np.nan
    inf = phi.copy()
    inf[0, 0] = -np.inf
    refused = [(dict(p=None), _lib.SR_ERR_ARG), (dict(n_tab=3), _lib.SR_ERR_ARG), (dict(n_tab=0), _lib.SR_ERR_ARG),
               (dict(p=nan), _lib.SR_ERR_ARG), (dict(p=inf), _lib.SR_ERR_ARG), (dict(t_lo=2.0), _lib.SR_ERR_ARG),
               (dict(t_lo=3.0), _lib.SR_ERR_ARG), (dict(t_hi=np.inf), _lib.SR_ERR_ARG), (dict(t_lo=np.nan), _lib.SR_ERR_ARG),
               (dict(n_shapes=0), _lib.SR_ERR_ARG), (dict(n_shapes=-1), _lib.SR_ERR_ARG),
               (dict(n_shapes=1, n_tab=big.size, p=big), _lib.SR_ERR_LIMIT)]
    area = np.full(5, -7.25)
    try:
        assert lib.sr_set_ils(None) == _lib.SR_OK and _probe() == _lib.SR_ERR_LIMIT
        for kw, status in refused:                           # refused with the Gaussian bound: the Gaussian stays
            assert lib.sr_set_ils(C.byref(desc(**kw))) == status, kw
            assert _probe() == _lib.SR_ERR_LIMIT, kw
            assert lib.sr_ils_area(C.byref(desc(**kw)), area.ctypes.data_as(dp)) == status, kw
        assert np.all(area == -7.25)
        assert lib.sr_ils_area(None, area.ctypes.data_as(dp)) == _lib.SR_ERR_ARG and lib.sr_ils_area(C.byref(desc()), None) == _lib.SR_ERR_ARG
        # five tables, a call with two bands: refused with SR_ERR_ARG before the size limit is looked at
        assert lib.sr_set_ils(C.byref(desc())) == _lib.SR_OK and _probe() == _lib.SR_ERR_ARG
        for kw, status in refused:                           # refused with a table bound: that table stays
            assert lib.sr_set_ils(C.byref(desc(**kw))) == status, kw
            assert _probe() == _lib.SR_ERR_ARG, kw
        # one table, or one per band of the call: the binding fits and the next check answers
        assert lib.sr_set_ils(C.byref(desc(n_shapes=1))) == _lib.SR_OK and _probe() == _lib.SR_ERR_LIMIT
        assert lib.sr_set_ils(C.byref(desc(n_shapes=2))) == _lib.SR_OK and _probe() == _lib.SR_ERR_LIMIT
        assert lib.sr_set_ils(C.byref(desc())) == _lib.SR_OK and _probe() == _lib.SR_ERR_ARG
        assert lib.sr_set_ils(None) == _lib.SR_OK and _probe() == _lib.SR_ERR_LIMIT
        # the area: the call copies nothing and changes no binding
        assert lib.sr_ils_area(C.byref(desc()), area.ctypes.data_as(dp)) == _lib.SR_OK and _probe() == _lib.SR_ERR_LIMIT
        h = 4.0 / 5
        want = [h * (p.sum() - (p[0] + p[-1]) / 2 + ((p[1] - p[0]) - (p[-1] - p[-2])) / 12) for p in phi]
        assert np.allclose(area, want, rtol=4e-16, atol=0)
    finally:
        lib.sr_set_ils(None)


def test_the_binding_is_per_thread():
    import threading
    from spectrobot_amd import _lib
    phi = np.ones((5, 6))
    d = _lib.IlsDesc(5, 6, -2.0, 2.0, phi.ctypes.data_as(_lib.dp))
    seen = {}
    try:
        assert _lib.lib.sr_set_ils(C.byref(d)) == _lib.SR_OK and _probe() == _lib.SR_ERR_ARG
        th = threading.Thread(target=lambda: seen.update(other=_probe()))
        th.start()
        th.join()
        assert seen["other"] == _lib.SR_ERR_LIMIT and _probe() == _lib.SR_ERR_ARG
    finally:
        _lib.lib.sr_set_ils(None)


def test_every_band_call_takes_the_keyword_and_unbinds(monkeypatch):
    from spectrobot_amd import engine, retrieval, spect_classes, _lib
    for fn in (engine.hires_to_lowres, engine.hires_to_lowres_instrument, engine.retrieval_forward, engine.retrieval_step,
               engine.retrieval_loop, engine.limb_rays_state_bands, engine.LevelFactored.state_bands,
               engine.LevelFactoredSet.state_bands, retrieval.LimbScene.__init__, spect_classes.SpectralIntensity.hires_to_lowres):
        assert inspect.signature(fn).parameters["ils"].default is None, fn
    # bound for the call, the Gaussian again behind it -- also when the call raises; without ils the binding is not touched
    ils = engine.ILS(-2.0, 2.0, np.ones((5, 6)))
    try:
        with pytest.raises(_lib.SpectRobotHipError) as e:
            with engine._IlsBound(ils):
                assert _probe() == _lib.SR_ERR_ARG
                _lib.check(_probe(), "probe")
        assert e.value.status == _lib.SR_ERR_ARG and _probe() == _lib.SR_ERR_LIMIT
        calls = []
        monkeypatch.setattr(engine.lib, "sr_set_ils", lambda *a: calls.append(a) or 0, raising=False)
        with engine._IlsBound(None):
            pass
        assert calls == []
    finally:
        monkeypatch.undo()
        _lib.lib.sr_set_ils(None)


def test_the_host_build_of_the_weights_kernel_runs_clean():
    """tools/host_sim/run.sh ils_host: sr_lowres_weights_tab_kernel's own text as a stand-alone program under AddressSanitizer and
    UBSan, against plain loops (see its main.cpp)."""
    here = os.path.dirname(os.path.abspath(__file__))
    tool = os.path.join(here, "..", "tools", "host_sim", "run.sh")
    r = subprocess.run(["bash", tool, "ils_host"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True, timeout=600)
    print(r.stdout[-3000:])
    assert r.returncode == 0 and "all cases ok" in r.stdout and "FAILED" not in r.stdout and "runtime error" not in r.stdout
