"""The far field held to ONE LINE'S OWN contribution, level by level (sr_far_field_truncation_bound: "of a line's own
contribution").  One line per LineSet and nothing else in the spectrum: every point's value is that line's, and
|far - exact| / |exact| is the quantity the bound speaks of -- no near lines dilute it, as they do on the dense line lists
of every other far-versus-exact comparison of the suite.

Shapes.  16384 grid points (16 top-level boxes), the line at index 8192 (both window ends, +-6505, and admissible boxes of
every level on the grid), n_levels = 0 with a given q_part, three layers per call -- Doppler-dominated (1e-5 hPa), ry = 0.5,
Lorentz-dominated (900 hPa) --, two grids: step 5e-4 at 2990 cm-1 (pole margin 5 at 70 K) and step 2e-3 (pole margin 2: the
box at its sharpest against the pole).  A shard's boxes start at its g_lo, so g_lo is swept, not the line: for every level
0-4 and each wing twelve consecutive g_lo around the one that puts a box of the level at sr_far_field_min_distance (the
kernels' own expression, through the engine) from the line's centre index, the centre on its grid point and 0.3 step off.
The sweep of level l + 1 is at once the HAND-OVER sweep of level l: below the threshold the two children own the line,
above it the parent -- a (line, box) pair dropped or doubled there is an error of 1.0.  Every sweep proves that it sits on
the threshold: where the library's distance says "not admissible" the box agrees with the exact mode to rounding
(8 K_PLAIN_FAR 2^-53: it is evaluated point by point, or by narrower boxes 7 half-widths away), where it says "admissible"
the box carries at least a quarter of the truncation the long-double model (tests/farfield_reference.py) predicts for it.
(The quiet side is not bit-equal to the exact mode: the near-wings kernel takes one reciprocal per point, the exact
kernels one per four.)

Routes: sr_set_far_field(1) (sr_farfield_kernel on every level), (3) (a single line is a sparse set:
sr_farfield_rows_kernel), (2) (box pairs, the line on the first / last point of its source box of every level), and the
multi-channel level tables (glevel_pairs / gcoeff_levels of a two-level molecule, sr_farfield_rows_batch_kernel +
sr_l2l_kernel) against the per-level route in the exact mode.

Limit: bound + 8 K_PLAIN_FAR 2^-53 (farfield_reference.K_PLAIN_FAR: the plain fp64 restatement of the expansion against
long double, in units of 2^-53 of the line's value).

Measured on an MI355X, 2026-10-18: worst |far - exact| / |exact| per route and level, in units of 1e-11 (the bound is
1.637, the limit 1.638), before -- the admissible distance 4 h + pm on every level, the box pairs' separation ratio 0.27 --
and as built now (sr_kernels.hpp ff_thr2: levels >= 1 carry a margin of 0.0735 h; sr_kernels.hip m2l_separated: 0.21):

    route                       level 0   level 1   level 2   level 3   level 4
    far field 1, before          1.236     1.704     2.005     2.177     2.269
    far field 3, before          1.236     1.704     2.005     2.177     2.269
    level tables, before         1.236     1.704     2.006     2.177     2.269
    far field 1, now             1.236     1.157     1.413     1.503     1.566
    far field 3, now             1.236     1.157     1.413     1.503     1.566
    level tables, now            1.236     1.157     1.413     1.503     1.566

    box pairs (far field 2)     step 5e-4: before 1.896 (192 points from the line: the nearest point of the first valid
                                target box, the line on the last point of its source box), now 0.645; step 2e-3: 0.587, 0.587
    window ends                 0.009 at the ends; 0.032 (per line) and 0.31 (box pairs) anywhere in those spectra

(all worst cases of the per-line routes: the Doppler-dominated layer, the centre 0.3 step towards the box, the box's
outermost point away from the line; level 1 was inside the bound on the fine grid, 1.416, and outside on the coarse one.)
The exact mode against the long-double rational: 5.3e-14 at worst, the plain fp64 restatement 5.2e-14, limit 4.2e-13.
"""
import signal

import numpy as np
import pytest

import farfield_reference as F

pytestmark = pytest.mark.gpu

N_GRID, IC = 16384, 8192
W0 = 2990.0
STEPS = (5e-4, 2e-3)
OFFS = (0.0, 0.3)
TEMPS = np.array([70.0, 68.0, 72.0])
Q_PART = np.array([90.0, 88.0, 93.0])
GAMMA, NDEP = 0.06, 0.7
SWEEP = range(-8, 4)          # g_lo - (the g_lo that puts the box AT the smallest admissible half-odd distance)
HALF = 6505


@pytest.fixture(autouse=True)
def _time_limit():
    """Each test under its own limit (they take seconds).  The alarm's handler runs between Python instructions: it ends a
    test that is slow, or that loops on the host; a call that never returns from the HIP runtime (a hung kernel under a
    synchronise or a copy) is not interrupted by it -- that is the limit of the command the suite runs under."""
    def _over(signum, frame):
        raise TimeoutError("test_gpu_farfield_lines: over its 150 s limit")
    old = signal.signal(signal.SIGALRM, _over)
    signal.alarm(150)
    try:
        yield
    finally:
        signal.alarm(0)
        signal.signal(signal.SIGALRM, old)


@pytest.fixture(scope="module")
def eng():
    import torch
    assert torch.cuda.is_available(), "these tests need the GPU"
    from spectrobot_amd import engine
    engine.set_device(0)
    return engine


def _line(freq, n=1, two_levels=False):
    one = np.ones(n)
    return dict(freq=np.atleast_1d(np.asarray(freq, float)), a_coeff=2.0 * one, e_lower=100.0 * one, g_up=9.0 * one,
                g_lo=7.0 * one, air_broad=GAMMA * one, t_dep_broad=NDEP * one,
                lev_up=np.full(n, 1 if two_levels else 0, np.int32), lev_lo=np.zeros(n, np.int32))


class Scene(object):
    """One grid, one line `off` steps beyond index IC, the three layers; the line's widths per layer from the reference's
    own formulas (spect_classes), the pole margins as the host sets them."""

    def __init__(self, eng, step, off, two_levels=False):
        from spectrobot_amd import synthetic as syn, spect_classes as spcl
        self.step, self.off = step, off
        self.grid = syn.make_grid(W0, step, N_GRID)
        self.x0 = float(self.grid[IC] + off * step)
        assert int(np.argmin(np.abs(self.grid - self.x0))) == IC
        self.dwp = np.array([spcl.Doppler_width(T, syn.CH4_MM, self.x0) for T in TEMPS]) / np.sqrt(np.log(2.0))
        # pressures: Doppler-dominated, ry = 0.5, Lorentz-dominated
        p_half = 0.5 * self.dwp[1] / float(spcl.Lorenz_width(TEMPS[1], spcl.convert_to_atm(1.0), NDEP, GAMMA))
        self.press = np.array([1e-5, p_half, 900.0])
        self.lw = np.array([spcl.Lorenz_width(T, spcl.convert_to_atm(P), NDEP, GAMMA) for T, P in zip(TEMPS, self.press)])
        self.ry = self.lw / self.dwp
        assert abs(self.ry[1] - 0.5) < 1e-6 and self.ry[0] < 1e-6 and self.ry[2] > 20
        # (np.arange's spacing, which the library takes from the grid, is not the nominal step to the last bit: 2e-10 off)
        self.xstep = float(self.grid[1] - self.grid[0]) / self.dwp
        self.pm = [F.pole_margin(xs) for xs in self.xstep]
        self.zone = np.ceil((self.lw + 15.0 * self.dwp) / step) + 2      # region 1 starts beyond this many points
        e_lev = [0.0, 1500.0] if two_levels else ()
        self.ls = eng.LineSet(_line(self.x0, two_levels=two_levels), self.grid, 6, 1, syn.CH4_MM, e_lev)
        self._exact = {}

    def coeffs(self, g_lo):
        a, e = self.ls.abscoeff_layers(TEMPS, self.press, q_part=Q_PART, g_lo=g_lo)
        return np.stack([a.cpu().numpy(), e.cpu().numpy()])           # [2, layer, point]


def _relerr(far, exact):
    nz = exact != 0
    assert np.array_equal(far != 0, nz)
    out = np.zeros(exact.shape)
    out[nz] = np.abs(far[nz] - exact[nz]) / np.abs(exact[nz])
    return out


def _box_lo(level, side, delta, pm):
    """First point of the level's box whose centre is the smallest admissible half-odd distance + delta from IC, right
    (side +1) or left (-1) of the line; and that distance."""
    W = 64 << level
    dmin = F.min_distance_pm(level, pm)
    d0 = np.floor(dmin) + 0.5                                          # centres sit on half points; dmin is a multiple of 1/2
    d = d0 + delta
    centre = IC + side * d
    return int(round(centre - (W - 1) / 2.0)), d, dmin


class Worst(object):
    def __init__(self):
        self.t = {}

    def add(self, key, val, where):
        if val > self.t.get(key, (-1.0, None))[0]:
            self.t[key] = (val, where)

    def show(self, title, limit):
        print("\n%s (limit %.4g)" % (title, limit))
        for key in sorted(self.t):
            v, where = self.t[key]
            print("  %-28s %.4g%s  at %s" % (key, v, "  OVER" if v > limit else "", where))

    def over(self, limit):
        return {k: v for k, v in self.t.items() if v[0] > limit}


def _limit(eng):
    return eng.far_field_truncation_bound() + F.KERNEL_MARGIN * F.K_PLAIN_FAR * F.EPS53


def _sweep_route(eng, route_name, far_call, exact_call):
    """The threshold sweeps of every level, wing, grid and centre offset for one route.  far_call / exact_call (scene, g_lo)
    -> array [plane, layer, point] over the shard [g_lo, N_GRID)."""
    degree = eng.far_field_degree()
    limit, quiet_limit = _limit(eng), F.KERNEL_MARGIN * F.K_PLAIN_FAR * F.EPS53
    worst, everywhere = Worst(), Worst()
    flips_missing, quiet_bad, loud_bad = [], [], []
    for step in STEPS:
        for off in OFFS:
            sc = Scene(eng, step, off, two_levels=(route_name == "level tables"))
            for level in F.LEVELS:
                W = 64 << level
                for side in (+1, -1):
                    seen = {k: [False, False] for k in range(3)}       # per layer: a quiet and a loud position seen
                    for delta in SWEEP:
                        blo, _, _ = _box_lo(level, side, delta, sc.pm[0])
                        g_lo = blo % W
                        far, exact = far_call(sc, g_lo), exact_call(sc, g_lo)
                        err = _relerr(far, exact)                       # [plane, layer, point]
                        everywhere.add("step %g level %d" % (step, level), float(err.max()),
                                       "off %g side %+d g_lo %d point %d" % (off, side, g_lo, g_lo + int(np.argmax(err.max(axis=(0, 1))))))
                        box = err[:, :, blo - g_lo: blo - g_lo + W]
                        for k in range(3):
                            d = abs(blo + (W - 1) / 2.0 - IC)
                            e_box = float(box[:, k].max())
                            worst.add("level %d step %g layer %d" % (level, step, k), e_box,
                                      "off %g side %+d g_lo %d distance %.1f" % (off, side, g_lo, d))
                            if d - W / 2.0 < sc.zone[k]:
                                continue                                # the box meets the line's zone: never admissible
                            admissible = d >= F.min_distance_pm(level, sc.pm[k])
                            # the line's centre lies off * step beyond IC: towards a box on the right, away from one on the left
                            model = F.truncation(level, sc.xstep[k], sc.ry[k], d, degree, -side * off)
                            tag = (step, off, level, side, delta, k, e_box, model)
                            if not admissible:
                                seen[k][0] = True
                                if e_box > quiet_limit:
                                    quiet_bad.append(tag)
                            elif model >= 20 * quiet_limit:
                                seen[k][1] = True
                                if e_box < 0.25 * model:
                                    loud_bad.append(tag)
                    # The Doppler layer and the ry = 0.5 layer: their zones (83 / 85 points on the fine grid, 23 on the
                    # coarse one) end inside 4 h + pm - h of every level, so every position of every sweep is judged and
                    # both sides must be seen.  The Lorentz layer cannot be held to that: its zone (371 / 95 points) reaches
                    # past the threshold boxes of levels 0-1 on the fine grid, which are then never admissible; where its
                    # boxes are judged the same quiet / loud checks apply to them.
                    if not (all(seen[0]) and all(seen[1])):
                        flips_missing.append((step, off, level, side, seen))
    worst.show("%s: worst |far - exact| / |exact| over the targeted boxes" % route_name, limit)
    everywhere.show("%s: the same over every point of the sweeps' shards" % route_name, limit)
    print("flip: %d quiet boxes over %.3g, %d admissible boxes under a quarter of the model" % (len(quiet_bad), quiet_limit, len(loud_bad)))
    for tag in (quiet_bad + loud_bad)[:12]:
        print("   step %g off %g level %d side %+d delta %d layer %d: box %.3g model %.3g" % tag)
    assert not flips_missing, "a sweep that does not straddle the threshold: %s" % flips_missing[:4]
    assert not quiet_bad and not loud_bad, "the sweep does not sit on the library's threshold (printed above)"
    over = dict(worst.over(limit), **everywhere.over(limit))
    assert not over, "over bound + 8 K_PLAIN_FAR 2^-53 = %.4g: %s" % (limit, over)


def _mode_calls(eng, mode):
    def far_call(sc, g_lo):
        eng.set_far_field(mode)
        try:
            return sc.coeffs(g_lo)
        finally:
            eng.set_far_field(eng.FAR_FIELD_DEFAULT)

    def exact_call(sc, g_lo):
        eng.set_far_field(0)
        try:
            return sc.coeffs(g_lo)
        finally:
            eng.set_far_field(eng.FAR_FIELD_DEFAULT)
    return far_call, exact_call


def _counts(eng, mode, sc, g_lo):
    eng.set_counting(1)
    eng.set_far_field(mode)
    try:
        sc.coeffs(g_lo)
        return sc.ls.last_eval_counts()
    finally:
        eng.set_far_field(eng.FAR_FIELD_DEFAULT)
        eng.set_counting(0)


@pytest.mark.parametrize("mode", [1, 3])
def test_per_line_expansions_hold_the_bound_at_every_level(eng, mode):
    """sr_set_far_field(1): sr_farfield_kernel; (3): one line is a sparse set -- sr_farfield_rows_kernel."""
    c = _counts(eng, mode, Scene(eng, STEPS[0], 0.0), 0)
    assert c["farfield_expansions"] > 0 and c["box_pair_translations"] == 0
    far_call, exact_call = _mode_calls(eng, mode)
    _sweep_route(eng, "far field %d" % mode, far_call, exact_call)


def test_box_pairs_hold_the_bound(eng):
    """sr_set_far_field(2): box pairs forced.  Source and target boxes share the frame that starts at g_lo: with
    g_lo = IC + 1 (mod 1024) the line sits on the LAST point of its source box at every level, facing the first valid
    target offset to its right; with g_lo = IC (mod 1024) on the first point, facing the left.  Eight g_lo around each.
    (What is measured here is mostly the MULTIPOLE series' truncation, which stops at the expansion degree too: with the
    separation ratio 0.27 of degree 22 this test read 1.896e-11 on the fine grid; m2l_separated has the derivation.)"""
    limit = _limit(eng)
    worst = Worst()
    far_call, exact_call = _mode_calls(eng, 2)
    c = _counts(eng, 2, Scene(eng, STEPS[0], 0.0), (IC + 1) % 1024)
    assert c["farfield_expansions"] > 0 and c["box_pair_translations"] > 0 and c["multipole_line_sides"] > 0
    for step in STEPS:
        for off in OFFS:
            sc = Scene(eng, step, off)
            for g_lo in sorted(set((IC + 1 + s) % 1024 for s in range(-4, 4)) | set((IC + 1 + s) % 64 for s in range(-4, 4))):
                err = _relerr(far_call(sc, g_lo), exact_call(sc, g_lo))
                k = int(np.argmax(err.max(axis=(0, 1))))
                worst.add("step %g off %g" % (step, off), float(err.max()),
                          "g_lo %d point %d (%+d from the line)" % (g_lo, g_lo + k, g_lo + k - IC))
    worst.show("far field 2 (box pairs): worst |far - exact| / |exact|", limit)
    assert not worst.over(limit), worst.over(limit)


def test_level_tables_far_only_passes_hold_the_bound(eng):
    """glevel_pairs and gcoeff_levels of a two-level molecule (the line: level 1 -> level 0) by the multi-channel route --
    far-only passes of the level sub-linesets, sr_farfield_rows_batch_kernel + sr_l2l_kernel -- against the per-level
    route in the exact mode.  Every non-zero plane is the one line times a weight.
    That the multi-channel pass RAN is shown first, once per entry point: where it does not apply it returns without a word
    and the callers fall back to one coefficient op per level -- with one line that is far field 3's rows kernel, which
    would pass every check below.  Counting cannot show it (a counting pass is itself a reason to fall back); the pass's
    timing events can: last_level_tables_ms answers only after a pass that ran to its end on that handle."""
    import torch
    from spectrobot_amd._lib import SpectRobotHipError

    eng.set_timing(1)                                                  # (the default)
    for entry in ("glevel_pairs", "gcoeff_levels"):
        for route, ran in ((0, False), (1, True)):
            sc = Scene(eng, STEPS[0], 0.0, two_levels=True)            # a fresh handle: no earlier pass's events on it
            eng.set_level_route(route)
            try:
                getattr(sc.ls, entry)(TEMPS, sc.press, g_lo=3)
                torch.cuda.synchronize()
            finally:
                eng.set_level_route(1)
            if ran:
                ms = sc.ls.last_level_tables_ms()
                assert len(ms) == 4 and all(np.isfinite(ms)) and min(ms) >= 0.0 and max(ms) > 0.0, (entry, ms)
            else:
                with pytest.raises(SpectRobotHipError):
                    sc.ls.last_level_tables_ms()

    def tables(sc, g_lo):
        p = sc.ls.glevel_pairs(TEMPS, sc.press, g_lo=g_lo)            # [level, 2, row, point]
        g = sc.ls.gcoeff_levels(TEMPS, sc.press, g_lo=g_lo)           # [level, 3, row, point]
        torch.cuda.synchronize()
        return np.concatenate([p.cpu().numpy().reshape(4, 3, -1), g.cpu().numpy().reshape(6, 3, -1)])

    def far_call(sc, g_lo):
        eng.set_level_route(1)
        eng.set_far_field(eng.FAR_FIELD_DEFAULT)
        out = tables(sc, g_lo)
        sc.ls.last_level_tables_ms()                                   # raises unless this handle's passes ran
        return out

    def exact_call(sc, g_lo):
        eng.set_level_route(0)
        eng.set_far_field(0)
        try:
            out = tables(sc, g_lo)
        finally:
            eng.set_far_field(eng.FAR_FIELD_DEFAULT)
            eng.set_level_route(1)
        assert sum(bool(np.any(pl != 0)) for pl in out) >= 6          # Gabs, -Gind, Gsp of the pairs; the three ctypes
        return out
    _sweep_route(eng, "level tables", far_call, exact_call)


def _plain_x(sc, k, j):
    """x of grid points j in layer k as a plain fp64 program following the reference's definitions has it: the window
    x(m) = (lin_start + (m - 1) lin_delta) + grid[IC] of the 13010 points about the centre index (spect_classes.py:1446),
    xstep = (x(2) - x(1)) / dw' (lineshape.f:265-266), the left wing counted from x(1) (lineshape.f:462), the right wing
    from the window point where it starts (:471) -- and then ONE fma per point, no running additions."""
    LD = F.LD
    gstep = float(sc.grid[1] - sc.grid[0])
    lin_start = -13010 * gstep / 2
    lin_delta = (lin_start + gstep) - lin_start                        # numpy.arange's spacing
    xw = lambda m: (lin_start + (m - 1) * lin_delta) + float(sc.grid[IC])
    dwp = float(sc.dwp[k])
    xstep = (xw(2) - xw(1)) / dwp
    m = j - (IC - HALF) + 1                                            # window index of grid point j
    m_r = HALF + 1 + int(sc.zone[k]) + 2
    fma = lambda n, a, c: np.asarray(LD(a) * n.astype(LD) + LD(c), np.float64)
    x_l = fma(m - 1, xstep, -((sc.x0 - xw(1)) / dwp))
    x_r = fma(m - m_r, xstep, (xw(m_r) - sc.x0) / dwp)
    return np.where(j < IC, x_l, x_r)


def test_exact_mode_against_the_long_double_rational(eng):
    """The yardstick's yardstick: the exact mode's region-1 values against w(x, ry) in long double.  Each spectrum is
    normalised at one far point k* (the weight drops out: weights are pinned elsewhere); y(k) / y(k*) against
    w(x_k) / w(x_k*) with x_k = (grid[k] - x0) / dw' in long double from the fp64 inputs, over the points safely inside
    region 1 and the window.  Limit: 8 x the distance of a plain numpy fp64 restatement (_plain_x: the reference's window
    and xstep, one fma per point; the rational with IEEE division) from that reference on the same inputs.  What that
    distance is made of: xstep is the difference of two window values rounded at 2990 cm-1, 4.5e-13 / 5e-4 of itself at
    worst -- the reference's definition, which the kernels reproduce; not the oracle's running additions, whose drift is
    larger than what is measured here.  So the plain distance is 0.8e-15 ... 5.2e-14, nearly all of it that definition and
    not rounding (the "fma" is one rounding of a long-double product and sum), and the limit 6e-15 ... 4.2e-13: this test
    catches an error of the exact mode's region 1 above about 4e-13 of a value (6e-15 on the Lorentz layer of the fine
    grid), and nothing smaller."""
    LD = F.LD
    _, exact_call = _mode_calls(eng, 1)
    for step in STEPS:
        for off in OFFS:
            sc = Scene(eng, step, off)
            y = exact_call(sc, 0)                                       # [2, layer, point]
            j = np.arange(N_GRID)
            kstar = IC + 3000
            for k in range(3):
                x_ld = (sc.grid.astype(LD) - LD(sc.x0)) / LD(sc.dwp[k])
                w_ld = F.rational(x_ld, sc.ry[k])
                w_64 = F.rational(_plain_x(sc, k, j), sc.ry[k], np.float64)
                sel = (np.abs(j - IC) >= sc.zone[k] + 2) & (j >= IC - HALF + 2) & (j <= IC + HALF - 3)
                assert sel.sum() > 10000 and sel[kstar]
                want = np.asarray(w_ld / w_ld[kstar], LD)
                plain = float(np.max(np.abs(w_64.astype(LD) / LD(w_64[kstar]) - want)[sel] / want[sel]))
                for plane, name in ((0, "abs"), (1, "emi")):
                    got = y[plane, k]
                    assert np.all(got[sel] != 0)
                    dist = float(np.max(np.abs(got.astype(LD) / LD(got[kstar]) - want)[sel] / want[sel]))
                    print("step %g off %g layer %d %s: exact mode %.3g, plain fp64 %.3g, limit %.3g%s"
                          % (step, off, k, name, dist, plain, 8 * plain, "  OVER" if dist > 8 * plain else ""))
                    assert dist <= 8 * plain, (step, off, k, name, dist, plain)


def test_window_ends_hold_the_bound(eng):
    """Forty lines whose centres lie within 20 points of each other: their window ends fall into the same 64-point slots
    and are taken by the per-line window-end expansions (a slot needs twelve of them).  Far field against the exact mode
    relative to the SUM (all weights are positive), same limit."""
    from spectrobot_amd import synthetic as syn
    limit = _limit(eng)
    rng = np.random.default_rng(20261018)
    for step in STEPS:
        grid = syn.make_grid(W0, step, N_GRID)
        freq = np.sort(grid[IC] + step * rng.uniform(-10.0, 10.0, 40))
        ls = eng.LineSet(_line(freq, 40), grid, 6, 1, syn.CH4_MM)
        press = np.array([1e-5, 8.0, 900.0])
        res = {}
        try:
            for far in (0, 1, 3, 2):
                eng.set_far_field(far)
                eng.set_counting(1 if far else 0)
                a, e = ls.abscoeff_layers(TEMPS, press, q_part=Q_PART)
                res[far] = np.stack([a.cpu().numpy(), e.cpu().numpy()])
                if far:
                    assert ls.last_eval_counts()["window_end_expansions"] > 0, far
        finally:
            eng.set_counting(0)
            eng.set_far_field(eng.FAR_FIELD_DEFAULT)
        assert np.all(res[0] >= 0)
        for far in (1, 3, 2):
            err = _relerr(res[far], res[0])
            ends = np.r_[IC - HALF - 40: IC - HALF + 90, IC + HALF - 90: IC + HALF + 40]
            print("window ends, step %g far field %d: %.4g at the ends, %.4g everywhere (limit %.4g)"
                  % (step, far, float(err[:, :, ends].max()), float(err.max()), limit))
            assert float(err.max()) <= limit, (step, far, float(err.max()))
