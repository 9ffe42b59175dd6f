"""Reference of the LEVEL TABLES (sr_glevel_pairs_dev, sr_gcoeff_levels_dev) and of their combine
(sr_glevel_combine_dev) that keeps every line's own contribution visible: for every (level, ctype, row, point) the sum
S of the per-line contributions shape * G[c] AND the sum A of their absolute values, both in numpy.longdouble, built on
frozen_reference._walk (the oracle's primitives in layer_run's order).  G_sp and G_ind go to the line's upper level,
G_abs to its lower level (oracle/sr_oracle.c::layer_run, mode 0; spect_classes.py:1304-1327).

A is the UNIT of every comparison made with this reference: a table value may differ from S by 2e-10 A at THAT point
(TOL_ONE_LINE, the suite's one-line limit against the oracle), and must be exactly 0 where A is 0 -- a level without
lines, a point beyond every window.  A measure "of a spectrum's largest value" cannot see a weak line beside a strong
one, a wing, or a contribution sent to the wrong plane; this one sees one line at one point.

The combine's limits are derived, not measured: gamma(k) = k u / (1 - k u), u = 2^-53, is the forward-error bound of a
chain of k roundings (Higham, Accuracy and Stability of Numerical Algorithms, 2nd ed., lemma 3.1): n fma for the values of
n levels, 2 n fma plus the two roundings of (tab' - tab) * inv_dT for the derivative.

TEST INFRASTRUCTURE ONLY; no GPU, no fixture."""
import numpy as np

import frozen_reference as FR
from test_gpu_frozen_reference import TOL_ONE_LINE      # 2e-10: tests/test_gpu_parity.py::test_single_line_regions_vs_oracle

LD = np.longdouble
U53 = 2.0 ** -53
TOL_OLD = 2e-12        # tests/test_gpu_glevel.py: of a spectrum's largest value (what this reference replaces)
N_GRID, IC = 16384, 8192
ROW_TEMPS = np.array([131.0, 150.0, 173.0])
ROW_PRESS = np.array([1e-5, 0.3, 200.0])       # Doppler-dominated, mixed, Lorentz-dominated
OFFS = (0.0, 0.3, 0.5, -0.5)                   # centre: steps off its grid point


def gamma(k):
    return k * U53 / (1.0 - k * U53)


def planes_by_row(lines, mm, e_lev, temps, press, grid, temps_b=None, linear_weights=False, p_shift=None, self_broad=None,
                  p_self=None):
    """Yields (k, S, A) per row k: S, A [max(n_levels, 1), 3, n_grid] in long double (64 levels x 3 ctypes x 16 384 points
    are 50 MB each: never all rows at once unless the caller keeps them), ctype 0 sp_emission | 1 ind_emission |
    2 absorption as sr_gcoeff_levels_dev orders them."""
    temps, press = np.atleast_1d(np.asarray(temps, float)), np.atleast_1d(np.asarray(press, float))
    tb = None if temps_b is None else np.atleast_1d(np.asarray(temps_b, float))
    nlev = len(e_lev) if e_lev is not None else 0
    for k in range(temps.size):
        S = np.zeros((max(nlev, 1), 3, len(grid)), dtype=LD)
        A = np.zeros_like(S)
        for _, i, lu, ll, lo, hi, shape, G in FR._walk(
                lines, mm, e_lev, temps[k:k + 1], press[k:k + 1], grid, None if tb is None else tb[k:k + 1], linear_weights, False,
                p_shift, self_broad, None if p_self is None else np.atleast_1d(np.asarray(p_self, float))[k:k + 1]):
            sh = shape.astype(LD)
            ash = np.abs(sh)
            for c, lev in ((0, lu), (1, lu), (2, ll)):
                g = LD(G[c])
                S[lev, c, lo:hi] += sh * g
                A[lev, c, lo:hi] += ash * abs(g)
        yield k, S, A


def planes(lines, mm, e_lev, temps, press, grid, **opts):
    """(S, A) [max(n_levels, 1), 3, n_rows, n_grid] in long double: sr_gcoeff_levels_dev's layout."""
    rows = [(S, A) for _, S, A in planes_by_row(lines, mm, e_lev, temps, press, grid, **opts)]
    return np.stack([r[0] for r in rows], axis=2), np.stack([r[1] for r in rows], axis=2)


def pairs_of(S, A):
    """The pair tables and their units from the planes (ctype axis 1): [L, 0] = S_abs - S_ind with unit A_abs + A_ind,
    [L, 1] = S_sp with unit A_sp -- sr_glevel_pairs_dev's layout."""
    return np.stack([S[:, 2] - S[:, 1], S[:, 0]], axis=1), np.stack([A[:, 2] + A[:, 1], A[:, 0]], axis=1)


def share_of_limit(got, want, limit):
    """The worst |got - want| / limit over the points with limit > 0; where the limit is 0 `got` must be exactly 0
    (AssertionError names the first offender).  No point is left out."""
    got = np.asarray(got)
    assert got.shape == want.shape == limit.shape, (got.shape, want.shape, limit.shape)
    assert np.all(np.isfinite(got))
    dead = limit == 0
    bad = dead & (got != 0)
    assert not bad.any(), "non-zero where no line contributes: first at %s" % (tuple(int(v) for v in np.argwhere(bad)[0]),)
    live = ~dead
    if not live.any():
        return 0.0
    return float(np.max(np.abs(got[live].astype(LD) - want[live]) / limit[live]))


def share(got, S, A, tol=TOL_ONE_LINE):
    """The worst |got - S| / (tol A) over the points with A > 0; exactly 0 where A = 0."""
    return share_of_limit(got, S, LD(tol) * A)


def old_measure(got, S):
    """max |got - S| over the largest |S| of each spectrum (last axis): tests/test_gpu_glevel.py::_plane_err."""
    s = np.maximum(np.max(np.abs(S), axis=-1, keepdims=True), LD(1e-300))
    return float(np.max(np.abs(np.asarray(got).astype(LD) - S) / s))


def exposed_scene(n_lev, outer=False):
    """A deterministic scene in which one line's contribution is visible from its core to its window ends and beyond:
    16 384 points of step 5e-4 at 2990 cm-1 (16 top-level far boxes; a +-6505-point window fits), the three rows above,
    levels [0, linspace(1300, 6000, n_lev - 1)].  Every upper level owns AT MOST ONE line (the levels L with L % 6 == 5
    own none: from six levels on there is a level without any line), so every G_sp and G_ind plane is one line or empty.
    Lines i with i % 4 < 2 sit 3 points apart around point 8192 (one chunk, colliding LDS adds; i and i + 1 own
    neighbouring levels, i.e. neighbouring planes), the others are spread over points 700 ... 15 700.  a_coeff = 10^((12 i
    mod 13) - 8): thirteen decades, lines 0 and 1 -- cluster neighbours, levels 1 and 2 -- 1e12 apart.  e_lower cycles over
    0 ... 2000 cm-1 (the weak line 0 at 2000, the strong line 1 at 0: their Boltzmann factors widen the gap).  Every fifth line has its lower level in 1 ... 3 (never its upper level), the others level 0.
    outer: the last four levels own one line each 3.3 and 6 cm-1 beyond either grid end (centre outside its own window:
    humliv_bb's sequential branches; the 200 hPa row reaches the grid).
    Returns a dict: grid, L (sorted by wavenumber), mm, e_lev, temps, press, p_shift, self_broad (per line, for
    set_line_shape), p_self (per row), point (centre grid point per line, -1 outer), cluster (bool per line)."""
    from spectrobot_amd import synthetic as syn
    step = 5e-4
    grid = syn.make_grid(2990.0, step, N_GRID)
    e_lev = np.concatenate([[0.0], np.linspace(1300.0, 6000.0, n_lev - 1)])
    top = n_lev - (4 if outer else 0)
    owners = np.array([lv for lv in range(1, top) if lv % 6 != 5], dtype=np.int32)
    n = owners.size
    i = np.arange(n)
    cluster = (i % 4) < 2
    nc = int(cluster.sum())
    point = np.zeros(n, dtype=np.int64)
    point[cluster] = IC + 3 * (np.arange(nc) - nc // 2)
    point[~cluster] = np.rint(np.linspace(700.0, 15700.0, n - nc)).astype(np.int64)
    freq = grid[point] + step * np.array(OFFS)[(i + i // 4) % 4]
    lev_lo = np.zeros(n, dtype=np.int32)
    if n_lev > 4:
        fifth = i % 5 == 4
        alt = 1 + (i // 5) % 3
        alt = np.where(alt == owners, alt % 3 + 1, alt)
        lev_lo[fifth] = alt[fifth]
    L = dict(freq=freq, a_coeff=10.0 ** ((12 * i) % 13 - 8.0), e_lower=250.0 * ((i + 8) % 9), g_up=2.0 * (i % 7) + 3.0,
             g_lo=2.0 * (i % 5) + 1.0, air_broad=0.04 + 0.004 * (i % 11), t_dep_broad=0.55 + 0.03 * (i % 10), lev_up=owners,
             lev_lo=lev_lo)
    if outer:
        o = np.arange(4)
        Lo = dict(freq=np.array([grid[0] - 3.3, grid[0] - 6.0, grid[-1] + 3.3, grid[-1] + 6.0]), a_coeff=10.0 ** (o - 1.0),
                  e_lower=100.0 * o, g_up=9.0 + 0 * o, g_lo=7.0 + 0 * o, air_broad=0.08 - 0.005 * o, t_dep_broad=0.6 + 0.05 * o,
                  lev_up=(top + o).astype(np.int32), lev_lo=np.zeros(4, np.int32))
        L = {k: np.concatenate([L[k], Lo[k]]).astype(L[k].dtype) for k in L}
        point, cluster = np.concatenate([point, np.full(4, -1)]), np.concatenate([cluster, np.zeros(4, bool)])
    order = np.argsort(L["freq"], kind="stable")
    L = {k: np.ascontiguousarray(v[order]) for k, v in L.items()}
    m = np.arange(order.size)
    return dict(grid=grid, L=L, mm=syn.CH4_MM, e_lev=e_lev, temps=ROW_TEMPS.copy(), press=ROW_PRESS.copy(),
                p_shift=-0.02 + 0.003 * (m % 11), self_broad=0.05 + 0.006 * (m % 12), p_self=0.05 * ROW_PRESS,
                point=point[order], cluster=cluster[order], n_lev=n_lev)


def medium_scene():
    """Many lines per plane, several chunks per image: 3000 random lines on 20 000 points, twelve levels, two rows (a
    Doppler-dominated and a Lorentz-dominated one)."""
    from spectrobot_amd import synthetic as syn
    grid = syn.make_grid(2985.0, 5e-4, 20000)
    return dict(grid=grid, L=syn.make_lines(3000, grid, n_levels=12), mm=syn.CH4_MM, e_lev=syn.CH4_LEVEL_ENERGIES,
                temps=np.array([140.0, 168.0]), press=np.array([1e-3, 30.0]), n_lev=12)


def scene_planes(sc, d_call=0.0, frozen_linear=False, shape=False):
    """planes() of a scene dict; frozen_linear: boundaries and linearised weights at the scene's T, the call at
    T + d_call; shape: with the scene's pressure shift, self-broadening and self pressure."""
    kw = {}
    if frozen_linear:
        kw.update(temps_b=sc["temps"], linear_weights=True)
    if shape:
        kw.update(p_shift=sc["p_shift"], self_broad=sc["self_broad"], p_self=sc["p_self"])
    return planes(sc["L"], sc["mm"], sc["e_lev"], sc["temps"] + d_call, sc["press"], sc["grid"], **kw)


def combine_reference(tab, step_row, pop, tab_dT=None, dpop=None, inv_dT=None):
    """sr_glevel_combine_dev's formula (include/spectrobot_hip.h; frozen_reference.combine) in long double, the fp64
    inputs and the fp64 inv_dT the library receives taken as exact:
        val[c, s] = sum_L pop[s, L] tab[L, c, row[s]]                          U  = sum_L |pop| |tab_L|
        dval[c, s] = sum_L dpop[s, L] tab_L + pop[s, L] (tab'_L - tab_L) inv_dT     dU = sum_L |dpop| |tab_L| + |pop| |tab'_L - tab_L| inv_dT
    Returns (val, U) or (val, U, dval, dU), each [2, n_steps, n_pts] (abs | emi).  Limits: gamma(n) U, gamma(2 n + 2) dU."""
    step_row = np.asarray(step_row, int)
    pop = np.asarray(pop).astype(LD)
    nl = tab.shape[0]
    shape = (2, step_row.size, tab.shape[3])
    val, U = np.zeros(shape, LD), np.zeros(shape, LD)
    want = tab_dT is not None
    if want:
        dpop, inv = np.asarray(dpop).astype(LD), LD(inv_dT)
        dval, dU = np.zeros(shape, LD), np.zeros(shape, LD)
    for lv in range(nl):
        t = np.asarray(tab[lv][:, step_row, :]).astype(LD)              # [2, s, n]
        p = pop[None, :, lv, None]
        val += p * t
        U += np.abs(p) * np.abs(t)
        if want:
            d = (np.asarray(tab_dT[lv][:, step_row, :]).astype(LD) - t) * inv
            q = dpop[None, :, lv, None]
            dval += q * t + p * d
            dU += np.abs(q) * np.abs(t) + np.abs(p) * np.abs(d)
    return (val, U, dval, dU) if want else (val, U)


def combine_inputs(n_levels, n_pts, seed):
    """Synthetic inputs of the combine alone: tables of 3 rows (row 1 unused) with random signs and 60 decades of
    magnitude, T + dT tables a few 1e-3 away, populations down to 1e-40 (signed derivatives), 7 steps in scrambled order."""
    rng = np.random.default_rng(seed)
    shp = (n_levels, 2, 3, n_pts)
    tab = rng.choice([-1.0, 1.0], shp) * 10.0 ** rng.uniform(-30.0, 30.0, shp)
    tab_dT = tab * (1.0 + 3e-3 * rng.standard_normal(shp))
    step_row = np.array([2, 0, 0, 2, 2, 0, 2], dtype=np.int32)
    pop = 10.0 ** rng.uniform(-40.0, 0.0, (7, n_levels))
    dpop = pop * rng.uniform(-0.2, 0.2, (7, n_levels))
    return tab, tab_dT, step_row, pop, dpop, 1.0 / 0.05
