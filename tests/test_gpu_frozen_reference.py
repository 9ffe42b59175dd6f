"""Frozen region boundaries (sr_lineset_set_bounds_temps), linearised weights (sr_lineset_set_linear_weights) and the
temperature derivative built on them, at boundary temperatures OTHER than the call's own, against
tests/frozen_reference.py -- the oracle's primitives composed as oracle/sr_oracle.c::layer_run with the boundaries placed
by oracle.humliv_bb_bounds (pinned to the oracle where T_b = T by tests/test_frozen_reference_host.py).  Every tolerance
is the one the unfrozen comparison of the same kind holds; its source is named where it is used."""
import numpy as np
import pytest

from conftest import relerr, far_tol

import frozen_reference as FR

pytestmark = pytest.mark.gpu

TOL = 1e-10          # tests/test_gpu_parity.py: pointwise against the oracle (one line in the wrong region at one point shows)
TOL_ONE_LINE = 2e-10  # tests/test_gpu_parity.py::test_single_line_regions_vs_oracle
TOL_ROUTES = 2e-12   # tests/test_gpu_glevel.py: the two level routes, of a spectrum's largest value
OFFSETS = (3.0, -3.0, 0.05, -0.05)


@pytest.fixture(scope="module")
def eng():
    import torch
    assert torch.cuda.is_available(), "these tests need the GPU"
    from spectrobot_amd import engine
    engine.set_device(0)
    return engine


def _np(t):
    return t.cpu().numpy()


def _plane_err(a, b):
    """max |a - b| relative to the largest |b| of each spectrum (last axis): tests/test_gpu_glevel.py's measure."""
    a, b = np.asarray(a, float), np.asarray(b, float)
    s = np.maximum(np.max(np.abs(b), axis=-1, keepdims=True), 1e-300)
    return float(np.max(np.abs(a - b) / s))


class _Refs(object):
    """The references of the many-lines case, each computed once on first use and left unchanged."""

    def __init__(self, c):
        self.c, self._memo = c, {}

    def _get(self, key, make):
        if key not in self._memo:
            v = make()
            for a in (v if isinstance(v, tuple) else (v,)):
                a.setflags(write=False)
            self._memo[key] = v
        return self._memo[key]

    def folded(self, d_call=0.0, d_bounds=None, linear=False, shift=False):
        """(abs, emi) of a call at T + d_call with the boundaries at T + d_bounds (None: the call's own)."""
        c = self.c
        kw = dict(p_shift=c["p_shift"], self_broad=c["self_broad"], p_self=c["p_self"]) if shift else {}
        t = c["temps"] + d_call
        return self._get(("folded", d_call, d_bounds, linear, shift), lambda: FR.abscoeff_layers(
            c["L"], c["mm"], c["e_lev"], t, c["press"], c["q_of_T"](t), c["tvib"], c["grid"],
            temps_b=None if d_bounds is None else c["temps"] + d_bounds, linear_weights=linear, **kw))

    def pairs(self, d_call=0.0, d_bounds=None, linear=False):
        c = self.c
        return self._get(("pairs", d_call, d_bounds, linear), lambda: FR.level_pairs(
            c["L"], c["mm"], c["e_lev"], c["temps"] + d_call, c["press"], c["grid"],
            temps_b=None if d_bounds is None else c["temps"] + d_bounds, linear_weights=linear))

    def quotient(self, scheme, h):
        c = self.c
        return self._get(("fd", scheme, h), lambda: FR.fd_quotient(c["L"], c["mm"], c["e_lev"], c["temps"], c["press"], c["q_of_T"],
                                                                  c["tvib"], c["grid"], h, scheme))

    def smooth(self):
        c = self.c
        return self._get("smooth", lambda: FR.dcoeff_dT_smooth(c["L"], c["mm"], c["e_lev"], c["temps"], c["press"], c["q_of_T"],
                                                             c["tvib"], c["grid"]))


@pytest.fixture(scope="module")
def big(oracle):
    """The many-lines case (frozen_reference.many_lines_case) and, from frozen_reference.bounds ALONE and before any GPU
    call, the conditions that keep the comparisons honest: the boundary temperatures used below move the indices."""
    c = FR.many_lines_case(oracle)
    L, mm, E, T, P, grid = (c[k] for k in ("L", "mm", "e_lev", "temps", "press", "grid"))
    b0 = FR.bounds(L, mm, T, P, grid, e_lev=E)
    for d in OFFSETS:
        frac, n3 = FR.exercise(b0, FR.bounds(L, mm, T + d, P, grid, e_lev=E))
        print("T_b = T%+.2f K: %.1f %% of the (line, layer) pairs with other indices, %d with another region-3 interval" % (d, 100 * frac, n3))
        assert frac >= (0.9 if abs(d) == 3.0 else 0.02), (d, frac)
        assert n3 >= 20, (d, n3)
    kw = dict(p_shift=c["p_shift"], self_broad=c["self_broad"], p_self=c["p_self"])
    frac, n3 = FR.exercise(FR.bounds(L, mm, T, P, grid, e_lev=E, **kw), FR.bounds(L, mm, T + 3.0, P, grid, e_lev=E, **kw))
    assert frac >= 0.9 and n3 >= 20, (frac, n3)
    c["ref"] = _Refs(c)
    return c


@pytest.fixture(scope="module")
def ls(eng, big):
    h = eng.LineSet(big["L"], big["grid"], 6, 1, big["mm"], big["e_lev"])
    yield h
    h.set_bounds_temps(None)
    h.close()


def test_one_line_at_a_time(eng):
    """Every Humlicek region and seam of ONE line whose boundaries sit at T_b = T + (-3, -0.05, +0.05, +3) K, from Doppler-
    to Lorentz-dominated, the centre half a step to either side of a grid point: the exact mode pointwise against the
    reference, with exact and with linearised weights.  The indices differ from the call's own (asserted per pressure
    for +-3 K), so a running x started with the wrong width or a value left at the boundary's shows at every seam."""
    from spectrobot_amd import synthetic as syn
    grid = syn.make_grid(2990.0, 5e-4, 14000)
    rng = np.random.default_rng(7)
    q = np.array([100.0])
    worst = 0.0
    eng.set_far_field(0)
    try:
        for P in (1e-6, 1e-3, 0.3, 5.0, 80.0, 1013.0):
            for off in (-0.5, 0.5):
                L = syn.make_lines(1, grid, seed=int(P * 1e6) % 9973 + 1, n_levels=0)
                L["freq"][0] = grid[7000] + off * 5e-4
                T = np.array([rng.uniform(90, 200)])
                b0 = FR.bounds(L, syn.CH4_MM, T, [P], grid)
                ls = eng.LineSet(L, grid, 6, 1, syn.CH4_MM)
                try:
                    for d in (-3.0, -0.05, 0.05, 3.0):
                        if abs(d) == 3.0:
                            assert np.any(FR.bounds(L, syn.CH4_MM, T + d, [P], grid)[0, 0, :4] != b0[0, 0, :4]), (P, d)
                        for linear in (False, True):
                            ls.set_bounds_temps(T + d, linear_weights=linear)
                            ab, em = ls.abscoeff_layers(T, [P], q_part=q)
                            abo, emo = FR.abscoeff_layers(L, syn.CH4_MM, [], T, [P], q, None, grid, temps_b=T + d, linear_weights=linear)
                            e = max(relerr(_np(ab), abo), relerr(_np(em), emo))
                            worst = max(worst, e)
                            assert e < TOL_ONE_LINE, (P, off, d, linear, e)
                finally:
                    ls.set_bounds_temps(None)
                    ls.close()
    finally:
        eng.set_far_field(eng.FAR_FIELD_DEFAULT)
    print("one line at a time, frozen at other temperatures: worst %.2e" % worst)


@pytest.mark.parametrize("d", OFFSETS)
def test_many_lines_every_mode_and_a_shard(eng, big, ls, d):
    """600 lines x 20 000 points x 4 layers (1e-3 to 1013 hPa), outer lines and lines centred beyond the ends among them,
    boundaries at T + d: far-field modes 3 and 2 and the exact mode pointwise against the reference (TOL, as
    tests/test_gpu_parity.py and tests/test_gpu_lineshape.py hold the far-field and the exact mode to), the far-field
    modes against the exact one and a spectral shard against the whole grid (far_tol(1e-12), as there)."""
    T, P, tv = big["temps"], big["press"], big["tvib"]
    abo, emo = big["ref"].folded(0.0, d)
    ls.set_bounds_temps(T + d)
    res = {}
    try:
        for mode in (3, 2, 0):
            eng.set_far_field(mode)
            res[mode] = tuple(_np(t) for t in ls.abscoeff_layers(T, P, tvib=tv))
        eng.set_far_field(eng.FAR_FIELD_DEFAULT)
        lo, hi = 7777, 13000
        shard = tuple(_np(t) for t in ls.abscoeff_layers(T, P, tvib=tv, g_lo=lo, g_hi=hi))
    finally:
        eng.set_far_field(eng.FAR_FIELD_DEFAULT)
        ls.set_bounds_temps(None)
    e_ref = {m: (relerr(res[m][0], abo), relerr(res[m][1], emo)) for m in res}
    e_modes = {m: (relerr(res[m][0], res[0][0]), relerr(res[m][1], res[0][1])) for m in (3, 2)}
    e_shard = (relerr(shard[0], res[3][0][:, lo:hi]), relerr(shard[1], res[3][1][:, lo:hi]))
    print("T_b = T%+.2f: against the reference %s, far-field against exact %s, shard %.2e %.2e" % (
        d, {m: "%.2e %.2e" % e_ref[m] for m in e_ref}, {m: "%.2e %.2e" % e_modes[m] for m in e_modes}, e_shard[0], e_shard[1]))
    # what the boundary temperature changes is far above the tolerance: the plain oracle is another function
    plain = big["ref"].folded(0.0, None)
    assert relerr(abo, plain[0]) > 1e-7 and relerr(emo, plain[1]) > 1e-7
    for m in res:
        assert max(e_ref[m]) < TOL, (d, m, e_ref[m])
    for m in e_modes:
        assert max(e_modes[m]) < far_tol(1e-12), (d, m, e_modes[m])
    assert max(e_shard) < far_tol(1e-12), (d, e_shard)


@pytest.mark.parametrize("linear", [False, True])
def test_many_lines_at_another_call_temperature(eng, big, ls, linear):
    """The derivative's own configuration: boundaries at T, the call at T + 0.05 K (and, linear, the weights continued
    from T) -- far-field and exact mode against the reference."""
    T, P, tv = big["temps"], big["press"], big["tvib"]
    abo, emo = big["ref"].folded(0.05, 0.0, linear)
    q = big["q_of_T"](T + 0.05)
    ls.set_bounds_temps(T, linear_weights=linear)
    try:
        ab, em = ls.abscoeff_layers(T + 0.05, P, tvib=tv, q_part=q)
        eng.set_far_field(0)
        ab_x, em_x = ls.abscoeff_layers(T + 0.05, P, tvib=tv, q_part=q)
    finally:
        eng.set_far_field(eng.FAR_FIELD_DEFAULT)
        ls.set_bounds_temps(None)
    e = (relerr(_np(ab), abo), relerr(_np(em), emo), relerr(_np(ab_x), abo), relerr(_np(em_x), emo))
    print("call at T + 0.05, boundaries at T, linear=%s: far-field %.2e %.2e exact %.2e %.2e" % ((linear,) + e))
    assert max(e) < TOL


def test_level_tables_on_both_routes(eng, big, ls):
    """glevel_pairs under set_bounds_temps(T, linear_weights=True) at T + 0.05 K, by the multi-channel pass and by one
    coefficient op per level: against each other (TOL_ROUTES of a spectrum's largest value) and against
    frozen_reference.level_pairs (TOL: of a spectrum's largest value for A_L = Gabs_L - Gind_L, whose parts cancel;
    pointwise for E_L = Gsp_L)."""
    T, P = big["temps"], big["press"]
    ref = big["ref"].pairs(0.05, 0.0, True)
    tabs = {}
    ls.set_bounds_temps(T, linear_weights=True)
    try:
        for route in (1, 0):
            eng.set_level_route(route)
            tabs[route] = _np(ls.glevel_pairs(T + 0.05, P))
    finally:
        eng.set_level_route(1)
        ls.set_bounds_temps(None)
    e_routes = _plane_err(tabs[1], tabs[0])
    e_ref = {r: (_plane_err(tabs[r], ref), relerr(tabs[r][:, 1], ref[:, 1])) for r in tabs}
    print("level tables, frozen + linearised at T + 0.05: routes %.2e, against the reference %s" % (e_routes, e_ref))
    assert np.all(np.max(np.abs(ref[1:, 1]), axis=(1, 2)) > 0.0)      # every excited level has lines
    assert e_routes < TOL_ROUTES
    for r in tabs:
        assert max(e_ref[r]) < TOL, (r, e_ref[r])


def _deriv_bound(tol, c_ref, d_ref, dT, scheme):
    """Values within tol of the reference at both ends of a quotient put the quotient within 2 tol max|c| / (2 dT)
    (central; / dT forward) of the reference's: per layer, relative to the layer's largest reference derivative."""
    span = 2.0 * dT if scheme == "central" else dT
    return 2.0 * tol * np.max(np.abs(c_ref), axis=-1) / span / np.max(np.abs(d_ref), axis=-1)


def test_level_factored_steps_with_derivative(eng, big, ls):
    """LevelFactored(dT=0.05).steps(row, tvib, derivative=True), 3 rows x 8 steps x 12 levels, against the numpy combine
    (frozen_reference.combine: the header's formula for sr_glevel_combine_dev) of the REFERENCE's tables and the
    product's host-side populations.  Coefficients: TOL of a spectrum's largest value.  Derivatives: tables within TOL of
    their largest value put step s within sum_L (|dpop_L| + 2 pop_L / dT) TOL max|table_L| of the reference's combine."""
    T, P, tv = big["temps"], big["press"], big["tvib"]
    rows = np.array([1, 2, 3])
    step_row = np.array([0, 1, 2, 2, 1, 0, 1, 2], dtype=np.int32)
    rng = np.random.default_rng(5)
    tvib = np.ascontiguousarray(tv[:, rows][:, step_row] + rng.uniform(-4.0, 4.0, (12, 8)))
    tab, tab_dT = big["ref"].pairs(0.0, None)[:, :, rows], big["ref"].pairs(0.05, 0.0, True)[:, :, rows]
    lf = eng.LevelFactored(ls, T[rows], P[rows], dT=0.05)
    (ab, em), (dab, dem) = lf.steps(step_row, tvib=tvib, derivative=True)
    pop, dpop = ls.level_populations(T[rows][step_row], tvib=tvib, derivative=True)
    (abo, emo), (dabo, demo) = FR.combine(tab, step_row, pop, tab_dT=tab_dT, dpop=dpop, dT=0.05)
    e_c = (_plane_err(_np(ab), abo), _plane_err(_np(em), emo))
    big_t = np.max(np.abs(tab), axis=-1)[:, :, step_row]                               # [L, 2, s]
    bound = np.einsum("sl,lcs->cs", np.abs(dpop) + 2.0 * pop / 0.05, big_t) * TOL
    e_d = np.stack([np.max(np.abs(_np(dab) - dabo), axis=-1), np.max(np.abs(_np(dem) - demo), axis=-1)])
    print("LevelFactored.steps: coefficients %.2e %.2e; derivatives, worst share of the bound %.3f" % (e_c + (float(np.max(e_d / bound)),)))
    assert max(e_c) < TOL
    assert np.all(e_d <= bound)


@pytest.mark.parametrize("scheme,dT", [("central", 0.05), ("forward", 0.002)])
def test_coefficients_dT_against_the_reference_quotient_and_the_smooth_derivative(eng, big, ls, scheme, dT):
    """engine.coefficients_dT against (i) the reference's quotient of the same scheme and step -- within the bound that
    TOL at either end of the quotient allows (_deriv_bound), relative to the layer's largest reference derivative -- and
    (ii) the smooth extrapolated derivative (frozen_reference.dcoeff_dT_smooth): the GPU's error may exceed the
    reference quotient's own scheme error by that bound and no more."""
    T, P, tv = big["temps"], big["press"], big["tvib"]
    _, (da, de) = eng.coefficients_dT(ls, T, P, tvib=tv, scheme=scheme, dT=dT)
    q_ref, smooth, c_ref = big["ref"].quotient(scheme, dT), big["ref"].smooth(), big["ref"].folded(0.0, None)
    for name, got, qr, sm, cr in (("abs", _np(da), q_ref[0], smooth[0], c_ref[0]), ("emi", _np(de), q_ref[1], smooth[1], c_ref[1])):
        bound = _deriv_bound(TOL, cr, sm, dT, scheme)
        e_q = np.max(np.abs(got - qr), axis=-1) / np.max(np.abs(sm), axis=-1)
        e_s, scheme_err = FR.layer_rel(got, sm), FR.layer_rel(qr, sm)
        print("coefficients_dT %s %s per layer: against the reference quotient %s (bound %s); against the smooth derivative %s "
              "(the reference quotient's %s)" % (scheme, name, e_q, bound, e_s, scheme_err))
        assert np.all(e_q <= bound), (scheme, name)
        assert np.all(e_s <= scheme_err + bound), (scheme, name)


@pytest.mark.parametrize("linear", [True, False])
def test_level_factored_derivative_against_the_smooth_derivative(eng, big, ls, linear):
    """LevelFactored(dT=0.05, linear_weights=...).steps(derivative=True), one step per layer at the case's own vibrational
    temperatures (the partition sum following T), against the same combine of the reference's tables and against the
    smooth derivative: no farther from it than the reference combine's own scheme error plus what TOL in the tables allows."""
    T, P, tv = big["temps"], big["press"], big["tvib"]
    rows = np.arange(4, dtype=np.int32)
    lf = eng.LevelFactored(ls, T, P, dT=0.05, linear_weights=linear)
    _, (dab, dem) = lf.steps(rows, tvib=tv, derivative=True)
    Q = big["q_of_T"](T)
    pop = np.array(FR.populations(big["e_lev"], T, Q, tv))
    dpop = pop * (-(FR.partition_sum_dT(6, 1, T) / Q)[:, None])
    tab, tab_dT = big["ref"].pairs(0.0, None), big["ref"].pairs(0.05, 0.0, linear)
    _, ref_q = FR.combine(tab, rows, pop, tab_dT=tab_dT, dpop=dpop, dT=0.05)
    smooth = big["ref"].smooth()
    big_t = np.max(np.abs(tab), axis=-1)[:, :, rows]
    bound_abs = np.einsum("sl,lcs->cs", np.abs(dpop) + 2.0 * pop / 0.05, big_t) * TOL
    for c, name, got in ((0, "abs", _np(dab)), (1, "emi", _np(dem))):
        top = np.max(np.abs(smooth[c]), axis=-1)
        bound = bound_abs[c] / top
        e_q = np.max(np.abs(got - ref_q[c]), axis=-1) / top
        e_s, scheme_err = FR.layer_rel(got, smooth[c]), FR.layer_rel(ref_q[c], smooth[c])
        print("LevelFactored derivative, linear=%s, %s per layer: against the reference combine %s (bound %s); against the smooth "
              "derivative %s (the reference combine's %s)" % (linear, name, e_q, bound, e_s, scheme_err))
        assert np.all(e_q <= bound), (linear, name)
        assert np.all(e_s <= scheme_err + bound), (linear, name)


def test_pressure_shift_and_self_broadening_under_frozen_boundaries(eng, big, ls):
    """The many-lines case with shifted centres and self-broadening in place and the boundaries at T + 3 K: the frozen
    indices are placed with the SHIFTED centre and lw at the boundary temperature -- far-field and exact mode against
    the reference, and against each other."""
    T, P, tv = big["temps"], big["press"], big["tvib"]
    abo, emo = big["ref"].folded(0.0, 3.0, False, True)
    ls.set_line_shape(big["p_shift"], big["self_broad"])
    ls.set_self_pressure(big["p_self"])
    ls.set_bounds_temps(T + 3.0)
    try:
        ab, em = ls.abscoeff_layers(T, P, tvib=tv)
        eng.set_far_field(0)
        ab_x, em_x = ls.abscoeff_layers(T, P, tvib=tv)
    finally:
        eng.set_far_field(eng.FAR_FIELD_DEFAULT)
        ls.set_bounds_temps(None)
        ls.set_line_shape(None, None)
        ls.set_self_pressure(None)
    e = (relerr(_np(ab), abo), relerr(_np(em), emo), relerr(_np(ab_x), abo), relerr(_np(em_x), emo))
    e_modes = (relerr(_np(ab), _np(ab_x)), relerr(_np(em), _np(em_x)))
    print("shift + self-broadening, T_b = T + 3: far-field %.2e %.2e exact %.2e %.2e, modes %.2e %.2e" % (e + e_modes))
    unshifted = big["ref"].folded(0.0, 3.0)
    assert np.all(FR.layer_rel(abo, unshifted[0])[1:] > 1e-3)          # the layers of 10 hPa and more
    assert max(e) < TOL
    assert max(e_modes) < far_tol(1e-12)
