"""Pressure shift of the line centres and self-broadening in the coefficient op (sr_lineset_set_line_shape,
sr_lineset_set_self_pressure) against tests/lineshape_reference.py -- the oracle's primitives composed as
oracle/sr_oracle.c::layer_run, with the shifted centre handed to make_shape and the self term in the Lorentz width
(pinned to the oracle without the data by tests/test_lineshape_reference_host.py)."""
import numpy as np
import pytest

from conftest import relerr, far_tol

import lineshape_reference as R

pytestmark = pytest.mark.gpu

TOL = 1e-10          # tests/test_gpu_parity.py: one line in the wrong Humlicek region at one point shows
HPA_TO_ATM = 0.00098692326671601
HALF_WINDOW = 6505   # grid points from a line's window centre to the window's first point


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
    """max |a - b| relative to the largest |b| of each spectrum (last axis)."""
    s = b.abs().amax(dim=-1, keepdim=True).clamp_min(1e-300)
    return float(((a - b).abs() / s).max())


@pytest.fixture(scope="module")
def big(eng, oracle):
    """3000 lines x 30 000 points x 6 layers down to 1450 hPa, where the centres move by up to 86 grid points: line
    set with the data in place and the reference, computed once."""
    from spectrobot_amd import synthetic as syn
    grid = syn.make_grid(2975.0, 5e-4, 30000)
    L = syn.make_lines(3000, grid, config_id=7, n_levels=12)
    atm = syn.make_atmosphere(6, 12)
    press = np.array([1450.0, 600.0, 100.0, 10.0, 0.5, 0.01])
    rng = np.random.default_rng(2026)
    n = len(L["freq"])
    p_shift, self_broad = rng.uniform(-0.03, 0.01, n), rng.uniform(0.05, 0.12, n)
    p_self = 0.05 * press
    q = oracle.partition_sums(6, 1, atm["temps"])
    ref = R.abscoeff_layers(L, syn.CH4_MM, syn.CH4_LEVEL_ENERGIES, atm["temps"], press, q, atm["tvib"], grid,
                            p_shift=p_shift, self_broad=self_broad, p_self=p_self)
    ls = eng.LineSet(L, grid, 6, 1, syn.CH4_MM, syn.CH4_LEVEL_ENERGIES)
    ls.set_line_shape(p_shift, self_broad)
    ls.set_self_pressure(p_self)
    assert np.max(np.abs(p_shift)) * press[0] * HPA_TO_ATM / 5e-4 > 80.0
    yield dict(grid=grid, L=L, temps=atm["temps"], press=press, tvib=atm["tvib"], q=q, p_shift=p_shift, self_broad=self_broad,
               p_self=p_self, ref=ref, ls=ls)
    ls.close()


def test_one_line_at_a_time(eng):
    """Every Humlicek region and seam of ONE shifted line, from Doppler- to Lorentz-dominated, the centre half a step to
    either side of a grid point; then the same with self-broadening at p_self = 0.05 P and P."""
    from spectrobot_amd import synthetic as syn
    grid = syn.make_grid(2990.0, 5e-4, 14000)
    rng = np.random.default_rng(7)
    q = np.array([100.0])
    worst = 0.0
    for P in (1e-3, 0.3, 5.0, 80.0, 1013.0, 1450.0):
        for delta in (-0.03, 0.01):
            for off in (-0.5, 0.5):
                L = syn.make_lines(1, grid, seed=int(P * 1e6) % 9973 + 1, n_levels=0)
                L["freq"][0] = grid[7000] + off * 5e-4
                T = np.array([rng.uniform(90, 200)])
                ls = eng.LineSet(L, grid, 6, 1, syn.CH4_MM)
                for g_self, f_self in ((None, None), (0.09, 0.05), (0.09, 1.0)):
                    ps = np.array([delta])
                    sb = None if g_self is None else np.array([g_self])
                    p_self = None if g_self is None else np.array([f_self * P])
                    ls.set_line_shape(ps, sb)
                    ls.set_self_pressure(p_self)
                    ab, em = ls.abscoeff_layers(T, [P], q_part=q)
                    abo, emo = R.abscoeff_layers(L, syn.CH4_MM, [], T, [P], q, None, grid, p_shift=ps, self_broad=sb, p_self=p_self)
                    e = max(relerr(_np(ab), abo), relerr(_np(em), emo))
                    worst = max(worst, e)
                    assert e < 2e-10, (P, delta, off, g_self, f_self, e)
                ls.close()
    print("one line at a time: worst %.2e" % worst)


def test_many_lines_far_field_exact_and_shard(eng, big):
    """The three host bounds (pole margin, source pole radius, widest zone) with centres up to 86 points from their
    window centres: far-field mode and exact mode against the reference, against each other, and a shard whose boxes
    start elsewhere against the whole grid."""
    ls, T, P, tv = big["ls"], big["temps"], big["press"], big["tvib"]
    abo, emo = big["ref"]
    ab, em = ls.abscoeff_layers(T, P, tvib=tv)
    e_far = (relerr(_np(ab), abo), relerr(_np(em), emo))
    eng.set_far_field(0)
    try:
        ab_x, em_x = ls.abscoeff_layers(T, P, tvib=tv)
    finally:
        eng.set_far_field(eng.FAR_FIELD_DEFAULT)
    e_exact = (relerr(_np(ab_x), abo), relerr(_np(em_x), emo))
    e_modes = (relerr(_np(ab), _np(ab_x)), relerr(_np(em), _np(em_x)))
    lo, hi = 11111, 19000
    ab_s, em_s = ls.abscoeff_layers(T, P, tvib=tv, g_lo=lo, g_hi=hi)
    e_shard = (relerr(_np(ab_s), _np(ab)[:, lo:hi]), relerr(_np(em_s), _np(em)[:, lo:hi]))
    print("far-field %.2e %.2e, exact %.2e %.2e, modes %.2e %.2e, shard %.2e %.2e" % (e_far + e_exact + e_modes + e_shard))
    assert max(e_far) < TOL and max(e_exact) < TOL
    assert max(e_modes) < far_tol(1e-12) and max(e_shard) < far_tol(1e-12)
    # and the inputs tell the feature from its absence: the unshifted oracle is far away
    ls.set_line_shape(None, None)
    try:
        ab_0, _ = ls.abscoeff_layers(T, P, tvib=tv)
    finally:
        ls.set_line_shape(big["p_shift"], big["self_broad"])
    assert np.all(R.effect(_np(ab_0), abo)[:4] > 1e-3)      # the layers of 10 hPa and more


@pytest.mark.parametrize("far", [3, 2, 0])
def test_shifts_near_the_limit(eng, oracle, far):
    """Centres up to 945 grid points from their window centres (0.33 cm-1/atm at 1450 hPa; the limit is 1024): the bounds
    at the far end of what the header allows -- per-line expansions (far=3: a sparse set), box pairs (2) and the exact
    mode (0) against the reference."""
    from spectrobot_amd import synthetic as syn
    grid = syn.make_grid(2975.0, 5e-4, 30000)
    L = syn.make_lines(600, grid, config_id=19, n_levels=12)
    rng = np.random.default_rng(77)
    p_shift = rng.uniform(-0.33, 0.33, 600)
    p_shift[:2] = (-0.33, 0.33)
    atm = syn.make_atmosphere(2, 12)
    press = np.array([1450.0, 100.0])
    q = oracle.partition_sums(6, 1, atm["temps"])
    abo, emo = R.abscoeff_layers(L, syn.CH4_MM, syn.CH4_LEVEL_ENERGIES, atm["temps"], press, q, atm["tvib"], grid, p_shift=p_shift)
    eng.set_far_field(far)
    try:
        ls = eng.LineSet(L, grid, 6, 1, syn.CH4_MM, syn.CH4_LEVEL_ENERGIES)
        ls.set_line_shape(p_shift, None)
        ab, em = ls.abscoeff_layers(atm["temps"], press, tvib=atm["tvib"])
        ls.close()
    finally:
        eng.set_far_field(eng.FAR_FIELD_DEFAULT)
    e = (relerr(_np(ab), abo), relerr(_np(em), emo))
    print("shifts to 945 points, far=%d: %.2e %.2e" % ((far,) + e))
    assert max(e) < TOL


def _window_side(grid, freq):
    """-1 / 0 / +1: the centre lies below / strictly inside / above the 13010-point window of closest_grid(freq)."""
    step = grid[1] - grid[0]
    ic = np.clip(np.rint((freq - grid[0]) / step), 0, grid.size - 1)
    first, last = grid[0] + (ic - HALF_WINDOW) * step, grid[0] + (ic + HALF_WINDOW - 1) * step
    return np.where(freq <= first + 2 * step, -1, np.where(freq >= last - 2 * step, 1, 0))


def _ends_case(eng, oracle):
    from spectrobot_amd import synthetic as syn
    grid = syn.make_grid(2975.0, 5e-4, 20000)
    rng = np.random.default_rng(31)
    L = syn.make_lines(86, grid, config_id=13, n_levels=12)
    f = np.concatenate([grid[0] + rng.uniform(-3.3, 3.3, 40), grid[-1] + rng.uniform(-3.3, 3.3, 40),
                        grid[0] - np.array([3.3, 4.0, 6.0]), grid[-1] + np.array([3.3, 4.0, 6.0])])
    p_shift = rng.uniform(-0.03, 0.01, f.size)
    press = np.array([1450.0, 100.0, 1.0])
    # a line whose shifted centre would change humliv_bb's branch in some layer is the REFUSED case (tested below): left out
    side0 = _window_side(grid, f)
    keep = np.ones(f.size, bool)
    for P in press:
        keep &= _window_side(grid, f + p_shift * P * HPA_TO_ATM) == side0
    assert keep[-6:].all() and keep.sum() >= 70 and (side0[keep] != 0).sum() >= 6
    order = np.argsort(f[keep], kind="stable")
    L = {k: np.ascontiguousarray(v[keep][order]) for k, v in L.items()}
    L["freq"] = np.ascontiguousarray(f[keep][order])
    atm = syn.make_atmosphere(3, 12)
    return dict(grid=grid, L=L, p_shift=p_shift[keep][order], press=press, temps=atm["temps"], tvib=atm["tvib"],
                q=oracle.partition_sums(6, 1, atm["temps"]))


@pytest.mark.parametrize("far", [3, 0])
def test_grid_ends_and_outer_lines(eng, oracle, far):
    """Lines around both grid ends -- clipped windows, main lines centred beyond an end, outer lines 3.3, 4 and 6 cm-1
    out (humliv_bb's sequential branches with the shifted centre) -- against the reference."""
    from spectrobot_amd import synthetic as syn
    c = _ends_case(eng, oracle)
    abo, emo = R.abscoeff_layers(c["L"], syn.CH4_MM, syn.CH4_LEVEL_ENERGIES, c["temps"], c["press"], c["q"], c["tvib"], c["grid"],
                                 p_shift=c["p_shift"])
    eng.set_far_field(far)
    try:
        ls = eng.LineSet(c["L"], c["grid"], 6, 1, syn.CH4_MM, syn.CH4_LEVEL_ENERGIES)
        ls.set_line_shape(c["p_shift"], None)
        ab, em = ls.abscoeff_layers(c["temps"], c["press"], tvib=c["tvib"])
        ls.close()
    finally:
        eng.set_far_field(eng.FAR_FIELD_DEFAULT)
    e = (relerr(_np(ab), abo), relerr(_np(em), emo))
    print("grid ends, far=%d: %.2e %.2e" % ((far,) + e))
    assert max(e) < TOL


def test_straddling_outer_line_is_refused(eng, oracle):
    """An outer line 40 points beyond its window with -0.03 cm-1/atm: at 1450 hPa its centre enters the window (86
    points) -- SR_ERR_UNSUPPORTED, outputs untouched; at 100 hPa (6 points) it stays outside and is computed."""
    import torch
    from spectrobot_amd import synthetic as syn
    from spectrobot_amd._lib import SR_ERR_UNSUPPORTED, SpectRobotHipError
    grid = syn.make_grid(2975.0, 5e-4, 20000)
    L = syn.make_lines(30, grid, config_id=17, n_levels=0)
    L["freq"][-1] = grid[-1] + (HALF_WINDOW + 40) * 5e-4
    p_shift = np.zeros(30)
    p_shift[-1] = -0.03
    T, q = np.array([150.0]), np.array([100.0])
    ls = eng.LineSet(L, grid, 6, 1, syn.CH4_MM)
    ls.set_line_shape(p_shift, None)
    out = (torch.full((1, 20000), 7.0, dtype=torch.float64, device="cuda"), torch.full((1, 20000), 7.0, dtype=torch.float64, device="cuda"))
    with pytest.raises(SpectRobotHipError) as ei:
        ls.abscoeff_layers(T, [1450.0], q_part=q, out=out)
    assert ei.value.status == SR_ERR_UNSUPPORTED
    torch.cuda.synchronize()
    assert bool((out[0] == 7.0).all()) and bool((out[1] == 7.0).all())
    ab, em = ls.abscoeff_layers(T, [100.0], q_part=q, out=out)
    abo, emo = R.abscoeff_layers(L, syn.CH4_MM, [], T, [100.0], q, None, grid, p_shift=p_shift)
    assert relerr(_np(ab), abo) < TOL and relerr(_np(em), emo) < TOL
    ls.close()


def test_defaults_are_bit_for_bit(eng, big):
    """Never set, zero arrays, set then reset: the coefficient op's outputs are equal bit for bit, in the far-field and the
    exact mode.  The level tables of the multi-channel pass are not reproducible to the bit from one call to the next as
    it is (several waves add into one LDS image in the order they arrive; two plain calls measured 5.7e-16 of a spectrum's
    largest value apart): they are held to that route's own 2e-12, and what two plain calls differ by is printed beside it."""
    import torch
    from spectrobot_amd import synthetic as syn
    L, grid, T, P, tv = big["L"], big["grid"], big["temps"], big["press"], big["tvib"]
    n = len(L["freq"])
    ls = eng.LineSet(L, grid, 6, 1, syn.CH4_MM, syn.CH4_LEVEL_ENERGIES)

    def both_modes():
        out = list(ls.abscoeff_layers(T, P, tvib=tv))
        eng.set_far_field(0)
        try:
            out += list(ls.abscoeff_layers(T, P, tvib=tv))
        finally:
            eng.set_far_field(eng.FAR_FIELD_DEFAULT)
        return out
    c0 = both_modes()
    t0, t0b = ls.glevel_pairs(T[:2], P[:2]), ls.glevel_pairs(T[:2], P[:2])
    ls.set_line_shape(np.zeros(n), np.zeros(n))
    c1 = both_modes()
    t1 = ls.glevel_pairs(T[:2], P[:2])
    assert all(torch.equal(x, y) for x, y in zip(c1, c0))
    ls.set_line_shape(big["p_shift"], big["self_broad"])
    ls.set_self_pressure(big["p_self"])
    a2, _ = ls.abscoeff_layers(T, P, tvib=tv)
    assert not torch.equal(a2, c0[0])
    ls.set_line_shape(None, None)
    ls.set_self_pressure(None)
    c3 = both_modes()
    t3 = ls.glevel_pairs(T[:2], P[:2])
    assert all(torch.equal(x, y) for x, y in zip(c3, c0))
    print("level tables: two plain calls %.1e (equal: %s), zero arrays %.1e, set then reset %.1e"
          % (_plane_err(t0b, t0), torch.equal(t0b, t0), _plane_err(t1, t0), _plane_err(t3, t0)))
    assert _plane_err(t1, t0) < 2e-12 and _plane_err(t3, t0) < 2e-12
    ls.close()


def test_level_routes_with_the_data(eng, big):
    """The multi-channel pass and one coefficient op per level agree with shifts on as they do without
    (tests/test_gpu_glevel.py: 2e-12 of a spectrum's largest value), pair tables and the three ctypes; the layer
    batches of a small table budget see their slice of the self pressure; LevelFactored.steps recombines to the folded op."""
    import torch
    ls, T, P, tv = big["ls"], big["temps"], big["press"], big["tvib"]
    tab = ls.glevel_pairs(T, P)
    g3 = ls.gcoeff_levels(T, P)
    eng.set_level_route(0)
    try:
        tab0 = ls.glevel_pairs(T, P)
        g30 = ls.gcoeff_levels(T, P)
    finally:
        eng.set_level_route(1)
    e = (_plane_err(tab, tab0), _plane_err(g3, g30))
    print("level routes with shifts: %.2e %.2e" % e)
    assert max(e) < 2e-12
    eng.set_table_budget(2 * ls.n_kept * 208)
    try:
        tab_b = ls.glevel_pairs(T, P)
        a_b, e_b = ls.abscoeff_layers(T, P, tvib=tv)
    finally:
        eng.set_table_budget(48 << 30)
    a_u, e_u = ls.abscoeff_layers(T, P, tvib=tv)
    assert torch.equal(a_b, a_u) and torch.equal(e_b, e_u) and _plane_err(tab_b, tab) < 2e-12
    rows = np.arange(len(T), dtype=np.int32)
    ab, em = eng.LevelFactored(ls, T, P).steps(rows, tvib=tv)
    sa, se = a_u.abs().amax(dim=1, keepdim=True), e_u.abs().amax(dim=1, keepdim=True)
    assert float(((ab - a_u).abs() / sa).max()) < 1e-12 and float(((em - e_u).abs() / se).max()) < 1e-12


def test_strength_route_and_temperature_derivative_with_the_data(eng, big):
    """The LTE check of tests/test_gpu_strengths.py (intensities made from the A: the strength route's abs is the G
    route's, 1e-12 per layer) and the agreement of coefficients_dT's schemes (tests/test_gpu_configs.py,
    test_temperature_derivative_schemes: frozen central 0.05 K within 1e-4, frozen forward within 2e-3 of the frozen
    central difference of 0.01 K), both with shifts and self-broadening on -- frozen boundaries place their indices with
    the shifted centre."""
    from spectrobot_amd import spect_classes as sc
    from spectrobot_amd import synthetic as syn
    ls, L, T, P, tv = big["ls"], big["L"], big["temps"], big["press"], big["tvib"]
    q296 = sc.CalcPartitionSum(6, 1, temp=296.0)
    ls.set_strengths(sc.Einstein_A_to_LineStrength_hitran(L["a_coeff"], L["freq"], 296.0, q296, L["g_up"], L["e_lower"],
                                                          syn.CH4_ISO_RATIO), iso_ab=syn.CH4_ISO_RATIO)
    ab_g, _ = ls.abscoeff_layers(T, P, tvib=tv)
    ab_s, _ = ls.abscoeff_layers_from_strengths(T, P, tvib=tv)
    a, b = _np(ab_s), _np(ab_g)
    assert float(np.max(np.max(np.abs(a - b), axis=1) / np.max(np.abs(b), axis=1))) <= 1e-12
    assert relerr(b, big["ref"][0]) < TOL     # (and both are the reference's)
    co, (da_ref, de_ref) = eng.coefficients_dT(ls, T, P, tvib=tv, scheme="central", dT=0.01)
    _, (da_c, de_c) = eng.coefficients_dT(ls, T, P, tvib=tv, coeffs=co, scheme="central")
    _, (da_f, de_f) = eng.coefficients_dT(ls, T, P, tvib=tv, coeffs=co, scheme="forward")

    def rel(x, y):
        return float(((x - y).abs().amax(dim=1) / y.abs().amax(dim=1)).max())
    print("dT schemes with shifts: central %.1e %.1e forward %.1e %.1e" % (rel(da_c, da_ref), rel(de_c, de_ref), rel(da_f, da_ref),
                                                                         rel(de_f, de_ref)))
    assert rel(da_c, da_ref) < 1e-4 and rel(de_c, de_ref) < 1e-4
    assert rel(da_f, da_ref) < 2e-3 and rel(de_f, de_ref) < 2e-3


def test_refusals_leave_the_outputs_untouched(eng, big):
    """Every refusal of the two setters and of a call with the data in place, before anything is copied or launched.
    (The handle of a per-level sub-lineset, which the setters refuse too, never leaves the library: no entry point returns
    one, so that refusal cannot be reached from here.)"""
    import ctypes as C
    import torch
    from spectrobot_amd import synthetic as syn
    from spectrobot_amd import _lib
    from spectrobot_amd._lib import lib, dp, SpectRobotHipError
    L, grid, T, P, tv = big["L"], big["grid"], big["temps"][:3], big["press"][:3], big["tvib"][:, :3]
    n = len(L["freq"])
    ls = eng.LineSet(L, grid, 6, 1, syn.CH4_MM, syn.CH4_LEVEL_ENERGIES)
    ls.set_line_shape(big["p_shift"], big["self_broad"])
    ls.set_self_pressure(0.05 * P)
    good = ls.abscoeff_layers(T, P, tvib=tv)

    def ptr(a):
        return a.ctypes.data_as(dp)
    ok = np.zeros(n)
    # the setters: wrong length, non-finite values, a negative self-broadening coefficient, negative / non-finite self pressure
    assert lib.sr_lineset_set_line_shape(ls._h, ptr(ok), None, n - 1) == _lib.SR_ERR_ARG
    assert lib.sr_lineset_set_line_shape(ls._h, None, ptr(ok), n + 1) == _lib.SR_ERR_ARG
    for bad in (np.nan, np.inf):
        v = ok.copy()
        v[n // 2] = bad
        assert lib.sr_lineset_set_line_shape(ls._h, ptr(v), None, n) == _lib.SR_ERR_ARG
        assert lib.sr_lineset_set_line_shape(ls._h, None, ptr(v), n) == _lib.SR_ERR_ARG
    v = ok.copy()
    v[3] = -1e-3
    assert lib.sr_lineset_set_line_shape(ls._h, None, ptr(v), n) == _lib.SR_ERR_ARG
    assert lib.sr_lineset_set_line_shape(None, ptr(ok), None, n) == _lib.SR_ERR_ARG
    for bad in (-1.0, np.nan, np.inf):
        v = np.array([1.0, bad, 1.0])
        assert lib.sr_lineset_set_self_pressure(ls._h, ptr(v), 3) == _lib.SR_ERR_ARG
    assert lib.sr_lineset_set_self_pressure(ls._h, ptr(ok), -1) == _lib.SR_ERR_ARG
    with pytest.raises(ValueError):
        ls.set_line_shape(ok[:-1], None)
    # none of them changed the data in place
    again = ls.abscoeff_layers(T, P, tvib=tv)
    assert torch.equal(again[0], good[0]) and torch.equal(again[1], good[1])

    out = tuple(torch.full((3, 30000), 7.0, dtype=torch.float64, device="cuda") for _ in range(2))
    tabs = torch.full((12, 2, 3, 30000), 7.0, dtype=torch.float64, device="cuda")

    def refused(status, call):
        with pytest.raises(SpectRobotHipError) as ei:
            call()
        assert ei.value.status == status
        torch.cuda.synchronize()
        assert bool((out[0] == 7.0).all()) and bool((out[1] == 7.0).all()) and bool((tabs == 7.0).all())
    # a call with another layer count than the self pressure's; a self pressure above the layer's pressure
    refused(_lib.SR_ERR_ARG, lambda: ls.abscoeff_layers(T[:2], P[:2], tvib=tv[:, :2], out=(out[0][:2], out[1][:2])))
    refused(_lib.SR_ERR_ARG, lambda: ls.glevel_pairs(T[:2], P[:2], out=tabs[:, :, :2].contiguous()))
    ls.set_self_pressure(np.array([1.0, 1.0, 1.0001]) * P)
    refused(_lib.SR_ERR_ARG, lambda: ls.abscoeff_layers(T, P, tvib=tv, out=out))
    refused(_lib.SR_ERR_ARG, lambda: ls.glevel_pairs(T, P, out=tabs))
    ls.set_self_pressure(P)        # p_self = P is allowed
    ls.abscoeff_layers(T, P, tvib=tv)
    ls.set_self_pressure(0.05 * P)
    # a shift beyond the limit of 1024 grid steps (0.4 cm-1/atm at 1.43 atm: 1145): both routes, every level route
    far_shift = np.full(n, 0.4)
    ls.set_line_shape(far_shift, big["self_broad"])
    refused(_lib.SR_ERR_LIMIT, lambda: ls.abscoeff_layers(T, P, tvib=tv, out=out))
    refused(_lib.SR_ERR_LIMIT, lambda: ls.glevel_pairs(T, P, out=tabs))
    eng.set_level_route(0)
    try:
        refused(_lib.SR_ERR_LIMIT, lambda: ls.glevel_pairs(T, P, out=tabs))
    finally:
        eng.set_level_route(1)
    ok_p = np.array([600.0, 100.0, 10.0])      # the same data where the pressure keeps it under the limit
    ls.set_self_pressure(None)
    ls.abscoeff_layers(T, ok_p, tvib=tv, out=out)
    assert bool(torch.isfinite(out[0]).all()) and not bool((out[0] == 7.0).any())
    # back to the accepted data: the handle still computes what it did
    ls.set_line_shape(big["p_shift"], big["self_broad"])
    ls.set_self_pressure(0.05 * P)
    again = ls.abscoeff_layers(T, P, tvib=tv)
    assert torch.equal(again[0], good[0]) and torch.equal(again[1], good[1])
    ls.close()


def test_make_abscoeff_isomolec_options(eng, golden):
    """smm.make_abscoeff_isomolec(pressure_shift=True, self_vmr=...) with SpectLine objects in: the line set's call with
    line_shape_of(lines) and p_self = self_vmr x Press; the defaults stay the reference's run (the golden fixture)."""
    import torch
    from spectrobot_amd import spect_classes as spcl, spect_base_module as sbm, spect_main_module as smm
    g = golden("e2e_ch4_levels")
    rng = np.random.default_rng(9)
    iso = sbm.IsoMolec(6, 1, float(g["mm"]))
    for i, e in enumerate(g["e_lev"]):
        iso.add_level("L%02d" % i, e, local_vibtemp=g["tvib"][i])
    lines = []
    for i in range(len(g["line_freq"])):
        up = "L%02d" % g["line_lev_up"][i] if g["line_lev_up"][i] >= 0 else "??"
        lo = "L%02d" % g["line_lev_lo"][i] if g["line_lev_lo"][i] >= 0 else "??"
        lines.append(spcl.SpectLine([6, 1, g["line_freq"][i], 0.0, g["line_a_coeff"][i], g["line_air_broad"][i],
                                     rng.uniform(0.05, 0.12), g["line_e_lower"][i], g["line_t_dep_broad"][i],
                                     rng.uniform(-0.012, 0.002), up, lo, "", "", "", g["line_g_up"][i], g["line_g_lo"][i]],
                                    nomi=spcl.cose_hit))
    grid = float(g["grid_w0"]) + float(g["grid_step"]) * np.arange(int(g["grid_n"]))
    T, P = np.asarray(g["temps"], float), np.asarray(g["press"], float)
    wn = [grid[0], grid[-1]]
    ab, em = smm.make_abscoeff_isomolec(wn, iso, T, P, LTE=False, lines=lines)
    assert relerr(_np(ab.device), g["abs"]) < TOL and relerr(_np(em.device), g["emi"]) < TOL
    p_shift, self_broad = spcl.line_shape_of(lines)
    ls = eng.LineSet(spcl.lines_to_soa(lines, iso), grid, 6, 1, float(g["mm"]), g["e_lev"])
    for shift, vmr in ((True, None), (False, 0.05), (True, np.linspace(0.02, 0.06, len(T)))):
        ab, em = smm.make_abscoeff_isomolec(wn, iso, T, P, LTE=False, lines=lines, pressure_shift=shift, self_vmr=vmr, to_host=False)
        ls.set_line_shape(p_shift if shift else None, self_broad if vmr is not None else None)
        ls.set_self_pressure(None if vmr is None else vmr * P)
        ab_d, em_d = ls.abscoeff_layers(T, P, tvib=g["tvib"])
        assert torch.equal(ab.device, ab_d) and torch.equal(em.device, em_d), (shift, vmr)
        assert R.effect(_np(ab_d), g["abs"]).max() > 1e-6
    with pytest.raises(ValueError):
        smm.make_abscoeff_isomolec(wn, iso, T, P, LTE=False, lineset=ls, pressure_shift=True)
    ls.close()


def test_scene_gas_with_self_broadening(eng, big):
    """retrieval.Gas(self_broadening=True): the scene hands the line set vmr x press before it builds the coefficients."""
    import torch
    from spectrobot_amd import retrieval as rt
    from spectrobot_amd import synthetic as syn
    L, grid, T, P = big["L"], big["grid"], big["temps"], big["press"]
    vmr = np.array([0.05, 0.04, 0.03, 0.02, 0.015, 0.01])
    ls = eng.LineSet(L, grid, 6, 1, syn.CH4_MM, syn.CH4_LEVEL_ENERGIES)
    ls.set_line_shape(big["p_shift"], big["self_broad"])
    z = np.linspace(0.0, 500.0, 6)
    scene = rt.LimbScene(grid, z, T, P, [rt.Gas("CH4", ls, vmr, iso_ratio=syn.CH4_ISO_RATIO, self_broadening=True)],
                         [3340.0], [2.0])
    (ab, em), = scene.coefficients()
    ls.set_self_pressure(vmr * P)
    ab_d, em_d = ls.abscoeff_layers(T, P)
    assert torch.equal(ab, ab_d) and torch.equal(em, em_d)
    ls.set_self_pressure(None)
    ab_n, _ = ls.abscoeff_layers(T, P)
    assert not torch.equal(ab_n, ab_d)
    # a new VMR profile reaches the next refresh
    scene.gas("CH4").add_clim(0.5 * vmr)
    (ab2, _), = scene.coefficients(refresh=True)
    ls.set_self_pressure(0.5 * vmr * P)
    assert torch.equal(ab2, ls.abscoeff_layers(T, P)[0])
    ls.close()
