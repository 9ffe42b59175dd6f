"""The level tables (sr_glevel_pairs_dev, sr_gcoeff_levels_dev: sr_zones_mc_kernel, sr_wings_mc_kernel, the far-only
passes; the per-level fallback) and their combine (sr_glevel_combine_dev) held POINTWISE to each line's own contribution:
against tests/level_tables_reference.py, the long-double sum S of shape * G per (level, ctype, row, point) and the sum A of
the absolute contributions at that point.

Limits (constants of the reference module, none measured here):
    tables     |table - S| <= 2e-10 A at every point (TOL_ONE_LINE), exactly 0 where A = 0;
               pair tables [L, 0] = S_abs - S_ind in units of A_abs + A_ind, [L, 1] = S_sp in units of A_sp
    combine    gamma(n) U for the values, gamma(2 n + 2) dU for the derivatives (n = n_levels, u = 2^-53)
    steps      the two together: sum_L |pop_L| 2e-10 A_L + gamma(n) U, and
               sum_L |dpop_L| 2e-10 A_L + |pop_L| 2e-10 (A_L + A'_L) / dT + gamma(2 n + 2) dU

Every test prints its worst share of the limit per entry point.

Measured on an MI355X, 2026-10-19: worst share of the limit.  Tables, |table - S| / (2e-10 A); glevel_pairs and
gcoeff_levels gave the same figure to four digits in every case, and so did the multi-channel route (route 1), the
per-level route (route 0) and, where run, route 0 in the exact mode -- the worst point lies in the near field, which all
of them evaluate alike; the far field's truncation stays below it:

    exposed scene, n_lev        2       10      11      15      16      47      48      64
                                0.049   0.084   0.084   0.099   0.099   0.098   0.098   0.096
    multi-channel pass          pairs: ran at every n_lev; three ctypes: ran up to 47, fell back at 48 and 64

    exposed scene, further conditions           13 levels   40 levels
    far field 1 / far field 2                   0.099       0.095
    shard (3001, 13333)                         0.099       0.095
    shard (8190, 16384)                         0.078       0.091
    shard (8200, 8231)                          0.0031      0.013
    one row per batch                           0.099       0.095
    frozen + linearised, call at T + 0.05       0.097       0.095
    pressure shift + self-broadening            0.099       0.095
    outer lines                                 0.084       0.098

    medium scene (3000 lines, 12 levels)        0.090, pair planes included, both routes

Combine alone, share of gamma(n) U | gamma(2 n + 2) dU (the values of the plain call and of the derivative call agree):

    n_levels     1      2      4      5      8      9      12     13     16     17     40     64
    values       0.988  0.930  0.569  0.636  0.385  0.298  0.298  0.261  0.271  0.208  0.107  0.073
    derivatives  0.396  0.412  0.324  0.317  0.207  0.178  0.135  0.193  0.138  0.122  0.082  0.078

LevelFactored(dT=0.05).steps(derivative=True): values 0.069 (13 levels) and 0.091 (40), derivatives 0.067 and 0.048.

With G_ind routed to the lower level in the reference, every table test and both steps tests above fail (29 of 41; the
twelve combine tests use no line data).
"""
import functools

import numpy as np
import pytest

import level_tables_reference as LT

pytestmark = pytest.mark.gpu

LD = LT.LD
ENTRIES = ("glevel_pairs", "gcoeff_levels")

# Whether the multi-channel pass takes (pair tables, three ctypes) of n_lev levels, or returns without a word and leaves one
# coefficient op per level to the caller.  zones_mc_image (spectrobot_amd/csrc/sr_kernels.hip): an image of n_ch planes
# takes 8 n_ch (w + 2) + 16384 bytes of the 160 KB of LDS; two images of w = 256 points fit up to 31 planes, one of
# w = 128 up to 141; n_ch = 2 n_lev | 3 n_lev.  So 256-point images up to 15 | 10 levels, 128-point images up to 64 | 47
# (SR_MAX_LEVELS is 64), and the three ctypes of 48 levels and more fall back.
MC_RAN = {2: (True, True), 10: (True, True), 11: (True, True), 12: (True, True), 13: (True, True), 15: (True, True), 16: (True, True),
          40: (True, True), 47: (True, True), 48: (True, False), 64: (True, False)}


@pytest.fixture(scope="module")
def eng():
    import torch
    assert torch.cuda.is_available(), "these tests need the GPU"
    from spectrobot_amd import engine
    engine.set_device(0)
    engine.set_timing(1)          # (the default) last_level_tables_ms answers after a multi-channel pass
    return engine


@functools.lru_cache(maxsize=2)
def _ref(name, variant="plain"):
    """(scene, {entry: (want, unit)}) of a scene and a variant, computed once and left unchanged; the units in fp64 (they
    are units: 64 levels x 3 x 3 x 16 384 long doubles are 150 MB an array)."""
    outer = variant == "outer"
    sc = LT.medium_scene() if name == "medium" else LT.exposed_scene(int(name), outer=outer)
    S, A = LT.scene_planes(sc, d_call=0.05 if variant == "frozen_linear" else 0.0, frozen_linear=variant == "frozen_linear",
                           shape=variant == "shape")
    P, U = LT.pairs_of(S, A)
    out = {"glevel_pairs": (P, U.astype(np.float64)), "gcoeff_levels": (S, A.astype(np.float64))}
    for pair in out.values():
        for a in pair:
            a.setflags(write=False)
    return sc, out


def _tables(eng, sc, entry, route, far, temps, lo=0, hi=None, setup=None):
    """(table as numpy, whether the multi-channel pass ran) of one entry point on a FRESH handle: no earlier pass's
    events on it, so last_level_tables_ms answers only if this call's pass ran to its end
    (tests/test_gpu_farfield_lines.py::test_level_tables_far_only_passes_hold_the_bound)."""
    import torch
    from spectrobot_amd._lib import SpectRobotHipError
    ls = eng.LineSet(sc["L"], sc["grid"], 6, 1, sc["mm"], sc["e_lev"])
    try:
        if setup is not None:
            setup(ls)
        eng.set_level_route(route)
        eng.set_far_field(far)
        out = getattr(ls, entry)(temps, sc["press"], g_lo=lo, g_hi=hi)
        torch.cuda.synchronize()
        try:
            ms = ls.last_level_tables_ms()
            ran = all(np.isfinite(ms)) and max(ms) > 0.0
        except SpectRobotHipError:
            ran = False
        return out.cpu().numpy(), ran
    finally:
        eng.set_level_route(1)
        eng.set_far_field(eng.FAR_FIELD_DEFAULT)
        ls.close()


def _hold(eng, name, configs, variant="plain", d_call=0.0, lo=0, hi=None, setup=None, title=""):
    """Both entry points under every (label, route, far-field mode) of `configs` against the reference; prints the worst
    share per entry point and configuration, then asserts all of them and the expected ran / fell-back pattern."""
    sc, ref = _ref(name, variant)
    n_lev = sc["n_lev"]
    shares, pattern = {}, {}
    for ie, entry in enumerate(ENTRIES):
        want, unit = ref[entry]
        for label, route, far in configs:
            got, ran = _tables(eng, sc, entry, route, far, sc["temps"] + d_call, lo, hi, setup)
            assert got.shape == want[..., lo:hi].shape
            shares[(entry, label)] = LT.share(got, want[..., lo:hi], unit[..., lo:hi])
            pattern[(entry, label)] = (ran, route == 1 and far != 0 and MC_RAN[n_lev][ie])
    print("\n%s, %d levels%s: worst |table - S| / (2e-10 A)" % (name, n_lev, title))
    for key in shares:
        print("  %-14s %-22s %.4g%s   multi-channel pass %s" % (key + (shares[key], "  OVER" if shares[key] > 1.0 else "",
                                                                    "ran" if pattern[key][0] else "did not run")))
    wrong = {k: v for k, v in pattern.items() if v[0] != v[1]}
    assert not wrong, "ran / fell back otherwise than MC_RAN says: %s" % wrong
    over = {k: v for k, v in shares.items() if not v <= 1.0}
    assert not over, over
    return shares


def _default(eng):
    return (("route 1", 1, eng.FAR_FIELD_DEFAULT), ("route 0", 0, eng.FAR_FIELD_DEFAULT))


@pytest.mark.parametrize("n_lev", [2, 10, 11, 15, 16, 47, 48, 64])
def test_tables_on_the_exposed_scene_at_every_switch(eng, n_lev):
    """Either side of every switch of the zones kernel's image width and of the fall-back (15 | 16 levels for the pair
    tables, 10 | 11 and 47 | 48 for the three ctypes), the smallest and the largest molecule: the multi-channel route, the
    per-level route, and the per-level route in the exact mode, each against the reference."""
    _hold(eng, str(n_lev), _default(eng) + (("route 0, exact mode", 0, 0),))


@pytest.mark.parametrize("n_lev", [13, 40])
@pytest.mark.parametrize("far", [1, 2])
def test_tables_under_forced_far_field_modes(eng, n_lev, far):
    """sr_set_far_field(1) / (2): per-line expansions / the box-pair chain for every sub-lineset, on both routes."""
    _hold(eng, str(n_lev), (("route 1", 1, far), ("route 0", 0, far)), title=", far field %d" % far)


@pytest.mark.parametrize("n_lev", [13, 40])
@pytest.mark.parametrize("shard", [(3001, 13333), (8190, 16384), (8200, 8231)])
def test_tables_on_shards(eng, n_lev, shard):
    """Spectral shards (their boxes and images start at g_lo): two wide ones and 31 points inside the cluster."""
    _hold(eng, str(n_lev), _default(eng), lo=shard[0], hi=shard[1], title=", shard %s" % (shard,))


@pytest.mark.parametrize("n_lev", [13, 40])
def test_tables_one_row_per_batch(eng, n_lev):
    """A table budget below one row's share (mc_bytes_per_row, sr_api.hip, starts with four record tables of 112 bytes
    per line; tests/test_gpu_glevel.py::test_multichannel_route_in_row_batches_and_after_other_calls takes three rows
    of them plus scratch for "a few rows"): rows_max = max(1, budget / bytes per row) = 1, every row a batch of its own."""
    n_lines = len(_ref(str(n_lev))[0]["L"]["freq"])
    try:
        eng.set_table_budget(n_lines * 112 * 4)
        _hold(eng, str(n_lev), _default(eng), title=", one row per batch")
    finally:
        eng.set_table_budget(48 << 30)


@pytest.mark.parametrize("n_lev", [13, 40])
def test_tables_frozen_and_linearised(eng, n_lev):
    """set_bounds_temps(T, linear_weights=True), the call at T + 0.05 K: the T + dT build of LevelFactored."""
    T = LT.ROW_TEMPS
    _hold(eng, str(n_lev), _default(eng), variant="frozen_linear", d_call=0.05,
          setup=lambda ls: ls.set_bounds_temps(T, linear_weights=True), title=", frozen + linearised at T + 0.05")


@pytest.mark.parametrize("n_lev", [13, 40])
def test_tables_with_pressure_shift_and_self_broadening(eng, n_lev):
    sc = _ref(str(n_lev), "shape")[0]

    def setup(ls):
        ls.set_line_shape(sc["p_shift"], sc["self_broad"])
        ls.set_self_pressure(sc["p_self"])
    _hold(eng, str(n_lev), _default(eng), variant="shape", setup=setup, title=", shifted and self-broadened")


@pytest.mark.parametrize("n_lev", [13, 40])
def test_tables_with_outer_lines(eng, n_lev):
    """Four lines 3.3 and 6 cm-1 beyond either grid end (centre outside its own window), each on an upper level of its
    own: their planes hold the outer branch alone."""
    sc, ref = _ref(str(n_lev), "outer")
    S, A = ref["gcoeff_levels"]
    for lv in range(n_lev - 4, n_lev):
        assert A[lv, 0, 2].max() > 0 and np.count_nonzero(A[lv, 0, 2]) < LT.N_GRID // 2      # it reaches the grid, from one end
    _hold(eng, str(n_lev), _default(eng), variant="outer", title=", outer lines")


def test_tables_on_the_medium_scene(eng):
    """3000 lines, twelve levels, two rows: many lines per plane, several chunks per image.  All planes, the pair planes
    whose parts cancel included, to 2e-10 A on both routes."""
    _hold(eng, "medium", _default(eng))


@pytest.mark.parametrize("n_levels", [1, 2, 4, 5, 8, 9, 12, 13, 16, 17, 40, 64])
def test_combine_alone(eng, n_levels):
    """sr_glevel_combine_kernel<1 | 4 | 8 | 12 | 16> on either side of every instance's limit and
    sr_glevel_combine_stream_kernel above 16 levels, on synthetic tables (random signs, 60 decades, populations down to
    1e-40; 3 table rows, one unused; 7 steps in scrambled order), at 1, 255, 256 and 257 points (a block is 256), with
    and without the derivative."""
    import torch
    worst = {}
    for n_pts in (1, 255, 256, 257):
        tab, tab_dT, step_row, pop, dpop, inv_dT = LT.combine_inputs(n_levels, n_pts, seed=1000 * n_levels + n_pts)
        val, U, dval, dU = LT.combine_reference(tab, step_row, pop, tab_dT, dpop, inv_dT)
        t0, t1 = torch.from_numpy(tab).cuda(), torch.from_numpy(tab_dT).cuda()
        plain = eng.glevel_combine(t0, step_row, pop)
        (ab, em), (dab, dem) = eng.glevel_combine(t0, step_row, pop, tab_dT=t1, dpop=dpop, dT=0.05)
        torch.cuda.synchronize()
        for key, got, want, lim in (("values", plain, val, LT.gamma(n_levels) * U), ("values (derivative call)", (ab, em), val, LT.gamma(n_levels) * U),
                                    ("derivatives", (dab, dem), dval, LT.gamma(2 * n_levels + 2) * dU)):
            s = LT.share_of_limit(np.stack([g.cpu().numpy() for g in got]), want, lim)
            worst[key] = max(worst.get(key, 0.0), s)
    print("\nglevel_combine, %d levels: worst share of gamma(n) U / gamma(2 n + 2) dU: %s" % (n_levels, {k: "%.3f" % v for k, v in worst.items()}))
    assert all(v <= 1.0 for v in worst.values()), worst


@pytest.mark.parametrize("n_lev", [13, 40])
def test_level_factored_steps_with_derivative(eng, n_lev):
    """LevelFactored(dT=0.05).steps(derivative=True) on the exposed scene: five steps on the three rows, vibrational
    temperatures of their own, populations from level_populations(derivative=True); the target is the long-double combine
    of the REFERENCE's tables at T and (frozen, linearised) at T + dT."""
    import torch
    sc, ref = _ref(str(n_lev))
    P0, U0 = ref["glevel_pairs"]
    P1, U1 = LT.pairs_of(*LT.scene_planes(sc, d_call=0.05, frozen_linear=True))
    T = sc["temps"]
    step_row = np.array([2, 0, 1, 1, 0], dtype=np.int32)
    rng = np.random.default_rng(13)
    tvib = np.ascontiguousarray(T[step_row][None, :] + rng.uniform(-10.0, 25.0, (n_lev, 5)))
    tvib[0] = T[step_row]
    ls = eng.LineSet(sc["L"], sc["grid"], 6, 1, sc["mm"], sc["e_lev"])
    try:
        lf = eng.LevelFactored(ls, T, sc["press"], dT=0.05)
        (ab, em), (dab, dem) = lf.steps(step_row, tvib=tvib, derivative=True)
        torch.cuda.synchronize()
        pop, dpop = ls.level_populations(T[step_row], tvib=tvib, derivative=True)
        got, dgot = np.stack([ab.cpu().numpy(), em.cpu().numpy()]), np.stack([dab.cpu().numpy(), dem.cpu().numpy()])
    finally:
        ls.close()
    inv_dT = 1.0 / 0.05
    val, U, dval, dU = LT.combine_reference(P0, step_row, pop, P1, dpop, inv_dT)
    tol = LD(LT.TOL_ONE_LINE)
    unit_v = LT.combine_reference(U0, step_row, np.abs(pop))[0]
    unit_d = LT.combine_reference(U0, step_row, np.abs(dpop))[0] + LT.combine_reference(U0 + U1.astype(np.float64), step_row, np.abs(pop))[0] * LD(inv_dT)
    s_v = LT.share_of_limit(got, val, tol * unit_v + LT.gamma(n_lev) * U)
    s_d = LT.share_of_limit(dgot, dval, tol * unit_d + LT.gamma(2 * n_lev + 2) * dU)
    print("\nLevelFactored.steps, %d levels: values at %.4g of their limit, derivatives at %.4g" % (n_lev, s_v, s_d))
    assert np.all(U > 0) and s_v <= 1.0 and s_d <= 1.0
