"""tests/level_tables_reference.py on the CPU: the long-double planes against two independent fp64 paths (the oracle's C
layer_run in mode 0, frozen_reference.level_pairs), the conditions that make the exposed scene expose a single line,
seeded defects that the new unit (2e-10 of the sum of the lines' absolute contributions AT the point) catches and the
old one (2e-12 of a spectrum's largest value) does not, and the derived limits of the combine against plain numpy.
No GPU."""
import numpy as np
import pytest

import frozen_reference as FR
import level_tables_reference as LT

LD = LT.LD


@pytest.fixture(scope="module")
def exposed13():
    sc = LT.exposed_scene(13)
    S, A = LT.scene_planes(sc)
    for a in (S, A):
        a.setflags(write=False)
    return sc, S, A


def _scene(name):
    return LT.medium_scene() if name == "medium" else LT.exposed_scene(int(name))


@pytest.mark.parametrize("name", ["13", "40", "medium"])
def test_planes_equal_two_independent_fp64_paths(oracle, name):
    """S rounded to fp64 against oracle.gcoeff_layers (C: one rounded product and one rounded addition per line, so within
    gamma(m + 1) A for the m lines of the list, the + 1 for the reference's own rounding to fp64) and its pair tables
    against frozen_reference.level_pairs (up to 2 m terms in a pair plane: gamma(2 m + 1) of A_abs + A_ind); where A = 0
    both are exactly 0."""
    sc = _scene(name)
    m = len(sc["L"]["freq"])
    S, A = LT.scene_planes(sc)
    _, _, G = oracle.gcoeff_layers(sc["L"], sc["mm"], sc["e_lev"], sc["temps"], sc["press"], np.ones(sc["temps"].size), None,
                                   sc["grid"], n_threads=4)
    s_c = LT.share(np.ascontiguousarray(G.transpose(1, 2, 0, 3)), S, A, tol=LT.gamma(m + 1))
    P, U = LT.pairs_of(S, A)
    s_p = LT.share(FR.level_pairs(sc["L"], sc["mm"], sc["e_lev"], sc["temps"], sc["press"], sc["grid"]), P, U, tol=LT.gamma(2 * m + 1))
    print("scene %s, %d lines: the C path at %.3f of gamma(m + 1) A, level_pairs at %.3f of gamma(2 m + 1) A" % (name, m, s_c, s_p))
    assert s_c <= 1.0 and s_p <= 1.0
    assert float(np.max(A)) > 0


@pytest.mark.parametrize("n_lev,outer", [(2, False), (13, False), (40, False), (49, False), (13, True), (40, True)])
def test_exposed_scene_conditions(n_lev, outer):
    """From the reference alone: at most one line per (upper level, G_sp | G_ind) plane; a level without any line (from
    six levels on; with two levels the ground state's G_sp and G_ind planes are the empty ones); a dynamic range of 1e9 or
    more inside a plane; no contribution near the subnormals (> 1e-200: the limits need no absolute floor)."""
    sc = LT.exposed_scene(n_lev, outer)
    L = sc["L"]
    assert len(set(L["lev_up"].tolist())) == len(L["lev_up"]) and np.all(L["lev_up"] != L["lev_lo"]) and np.all(L["lev_up"] >= 1)
    assert np.all(L["lev_lo"] <= 3) and (n_lev <= 4 or np.any(L["lev_lo"] > 0))
    S, A = LT.scene_planes(sc)
    assert S.shape == (n_lev, 3, 3, LT.N_GRID)
    empty = [lv for lv in range(n_lev) if not A[lv].any()]
    assert empty if n_lev >= 6 else (not A[0, 0].any() and not A[0, 1].any())
    live = A > 0
    assert float(A[live].min()) > 1e-200
    # one line per plane: S and A agree to the reference's own rounding wherever a G_sp / G_ind plane is not empty
    up = A[:, :2]
    assert np.all(np.abs(np.abs(S[:, :2]) - up) <= LD(2.0 ** -60) * up)
    span = 0.0
    for lv in range(n_lev):
        for c in range(3):
            for k in range(3):
                a = A[lv, c, k][live[lv, c, k]]
                if a.size:
                    span = max(span, float(a.max() / a.min()))
    below = float(np.mean((A < LD(1e-6) * A.max(axis=-1, keepdims=True))[live]))
    print("n_lev %d outer %s: %d lines, empty levels %s, smallest contribution %.1e, in-plane range %.1e, %.0f %% of the points "
          "below 1e-6 of their plane's maximum" % (n_lev, outer, len(L["freq"]), empty, float(A[live].min()), span, 100 * below))
    assert span >= 1e9
    if not outer:
        assert np.all(sc["point"] >= 700 - 1) and np.all(np.abs(sc["point"][sc["cluster"]] - LT.IC) <= 3 * 32)


def test_seeded_defects_exceed_the_new_limit_and_most_pass_the_old_one(oracle, exposed13):
    """Six defects applied to a copy of the reference's planes (rounded to fp64, which itself sits at 1e-6 of the limit).
    Every one exceeds the new limit somewhere (2e-10 A, or a value where A = 0: printed as inf); those that are SMALL
    AGAINST THE LARGEST VALUE of their spectrum -- a weak line in a strong line's plane, a wing, a far box -- pass 2e-12 of
    the plane's maximum, the measure the level tables were held to before."""
    sc, S, A = exposed13
    L, grid = sc["L"], sc["grid"]
    clean = S.astype(np.float64)
    assert LT.share(clean, S, A) < 1e-5 and LT.old_measure(clean, S) < 1e-15
    weak, strong = int(np.flatnonzero(L["lev_up"] == 1)[0]), int(np.flatnonzero(L["lev_up"] == 2)[0])
    assert sc["cluster"][weak] and sc["cluster"][strong] and abs(sc["point"][weak] - sc["point"][strong]) == 3
    assert L["a_coeff"][strong] / L["a_coeff"][weak] == 1e12
    ps = int(sc["point"][strong])
    il2 = int(FR.bounds(L, sc["mm"], sc["temps"], sc["press"], grid, e_lev=sc["e_lev"])[strong, 0, 2])
    seam = oracle.closest_grid(grid, float(L["freq"][strong])) - FR.IMXSIG // 2 + il2 - 1
    assert 0 < ps - seam < 200 and clean[2, 0, 0, seam] != 0

    def d_wrong_plane(t):       # the weak line's G_ind lands in the neighbouring level's plane
        t[2, 1] += clean[1, 1]

    def d_wing(t):              # a region-1 wing dropped beyond +4096 points, Doppler row
        t[2, 0, 0, ps + 4096:] = 0.0

    def d_seam(t):              # one point doubled at the line's il2 seam
        t[2, 0, 0, seam] *= 2.0

    def d_scale(t):             # the weak line, three points from one 1e12 stronger, scaled by 1 + 1e-6
        t[1, 0] *= 1.0 + 1e-6
        t[1, 1] *= 1.0 + 1e-6

    def d_leak(t):              # 1e-9 of the strongest core leaks into another one-line plane
        t[1, 0] += 1e-9 * clean[2, 0]

    def d_far_box(t):           # one 1024-point far box of a Lorentz wing off by 1e-9 of the line's own value
        t[2, 0, 2, ps + 4096: ps + 5120] *= 1.0 + 1e-9

    def new_measure(t, S_, A_):
        try:
            return LT.share(t, S_, A_)
        except AssertionError:    # a value where no line contributes (the weak line's window ends 3 points past the strong one's)
            return np.inf

    res = {}
    for f in (d_wrong_plane, d_wing, d_seam, d_scale, d_leak, d_far_box):
        t = clean.copy()
        f(t)
        res[f.__name__] = (new_measure(t, S, A), LT.old_measure(t, S))
        print("%-14s new measure: %.3g of the limit; old measure: %.3g (limit %.0e)%s" % (
            f.__name__, res[f.__name__][0], res[f.__name__][1], LT.TOL_OLD, "  PASSES the old one" if res[f.__name__][1] < LT.TOL_OLD else ""))
    assert all(v[0] > 1.0 for v in res.values()), res
    missed = sorted(k for k, v in res.items() if v[1] < LT.TOL_OLD)
    # (the doubled seam point is 3.8e-9 of its spectrum's maximum, the scaled line 1e-6 and the leak far more: those the
    # old measure sees too)
    assert missed == ["d_far_box", "d_wing", "d_wrong_plane"], missed
    # the same defect in the PAIR tables, as glevel_pairs holds them
    t = clean.copy()
    d_wrong_plane(t)
    P, U = LT.pairs_of(S, A)
    tp = np.stack([t[:, 2] - t[:, 1], t[:, 0]], axis=1)
    assert new_measure(tp, P, U) > 1.0 and LT.old_measure(tp, P) < LT.TOL_OLD


def test_share_insists_on_exact_zeros(exposed13):
    sc, S, A = exposed13
    t = S.astype(np.float64)
    t[5, 0, 1, 100] = 1e-300          # level 5 owns no line
    with pytest.raises(AssertionError):
        LT.share(t, S, A)


@pytest.mark.parametrize("n_levels", [1, 2, 4, 5, 8, 9, 12, 13, 16, 17, 40, 64])
def test_plain_numpy_combine_holds_the_derived_bounds(n_levels):
    """frozen_reference.combine (numpy fp64, any summation order: n rounded products and at most n - 1 rounded additions
    per term; for the derivative the two roundings of (tab' - tab) / dT, a product, and at most n additions of the two
    sums) against the long-double combine: gamma(n) U and gamma(2 n + 2) dU."""
    worst = [0.0, 0.0]
    for n_pts in (1, 257):
        tab, tab_dT, step_row, pop, dpop, inv_dT = LT.combine_inputs(n_levels, n_pts, seed=100 * n_levels + n_pts)
        val, U, dval, dU = LT.combine_reference(tab, step_row, pop, tab_dT, dpop, inv_dT)
        if n_pts == 257:
            assert np.abs(tab).max() / np.abs(tab).min() > 1e55 and np.any(tab < 0) and np.any(tab > 0)
        if n_levels >= 8:
            assert pop.min() < 1e-35
        (ab, em), (dab, dem) = FR.combine(tab, step_row, pop, tab_dT=tab_dT, dpop=dpop, dT=0.05)
        assert np.all(U > 0) and np.all(dU > 0)
        worst[0] = max(worst[0], float(np.max(np.abs(np.stack([ab, em]).astype(LD) - val) / (LT.gamma(n_levels) * U))))
        worst[1] = max(worst[1], float(np.max(np.abs(np.stack([dab, dem]).astype(LD) - dval) / (LT.gamma(2 * n_levels + 2) * dU))))
    print("n_levels %d: plain numpy at %.3f of gamma(n) U and %.3f of gamma(2 n + 2) dU" % (n_levels, worst[0], worst[1]))
    assert worst[0] <= 1.0 and worst[1] <= 1.0
