"""The extended-precision reference of the instrument step (tests/lowres_reference.py) checked on the host: it reproduces
the reference program's recorded run (tests/golden/lowres_ils.npz) in all three units, the plain-fp64 yardstick K_PLAIN is
recorded and respected, shard partials add up to the whole, the panel keeps its guard and holds the windows it promises,
the exact-end cases meet their bitwise preconditions, and five seeded defects of a plain restatement each land beyond the
kernels' limit on at least one probe.  No GPU."""
import numpy as np
import pytest

import lowres_reference as R


@pytest.fixture(scope="module")
def problem():
    P = R.panel(*R.K_PLAIN_PANEL)
    P["ref"] = R.band_reference(P["grid"], P["spec"], P["centers"], P["widths"])
    P["plain"] = R.oracle_plain(P["grid"], P["spec"], P["centers"], P["widths"])
    # the two exact-end bands on the same grid, probed by a one-hot spectrum at their shared end point and by noise
    k = 5000
    ec, ew, xk = R.exact_end_cases(P["grid"], k)
    spec = np.zeros((2, P["grid"].size))
    spec[0, k] = 1.0
    spec[1] = P["spec"][0]
    P["exact"] = dict(k=k, centers=ec, widths=ew, xk=xk, spec=spec, ref=R.band_reference(P["grid"], spec, ec, ew))
    return P


def test_reference_reproduces_the_recorded_run(golden):
    """lowres_ils.npz (the reference program's own numpy run: 7 bands, 24 000 points, one positive spectrum) in 'Wm2',
    'ergscm2' and 'nWcm2' within the kernels' limit of the fixture's own K_PLAIN."""
    g = golden("lowres_ils")
    grid, step = R.make_grid(float(g["grid_w0"]), float(g["grid_step"]), int(g["grid_n"]))
    assert step == float(g["grid_step"])
    for u in R.UNITS:
        ref = R.band_reference(grid, g["spectrum"], g["centers_nm"], g["widths_nm"], units=u)
        k_plain = R.units_of(R.oracle_plain(grid, g["spectrum"], g["centers_nm"], g["widths_nm"], units=u), ref).max()
        got = R.units_of(g["low_" + u][None, :], ref)
        print("lowres_ils %s: K_PLAIN %.3g, limit %.3g, recorded run %.3g units (guard %.3g, counts %s)"
              % (u, k_plain, R.limit(k_plain), got.max(), ref["guard"].min(), ref["count"]))
        assert np.all(ref["count"] >= 2) and got.max() <= R.limit(k_plain)


def test_long_double_against_60_digits():
    """A 257-point panel of 17 bands in mpmath at 60 digits -- the same fp64 data, the same fp64 window selection, exact
    powers of ten -- under the two dense spectra and every eighth one-hot probe, compared in long double: the reference is
    within 2^-5 units (a dozen roundings of a term at 2^-64 = 2^-11 units each, as in test_shard_partials_add_up)."""
    from mpmath import mp          # (sympy, which torch needs, brings it)
    mp.dps = 60
    P = R.panel(2975.0, 5e-4, 257, 17, 20261018)
    rows = np.r_[0:2, 2:len(P["spec"]):8]
    spec = P["spec"][rows]
    ref = R.band_reference(P["grid"], spec, P["centers"], P["widths"], units="nWcm2")
    g = P["grid"][::-1]
    x = 1e7 / g
    val = np.zeros((len(rows), len(P["centers"])), R.LD)
    for b, (f, w) in enumerate(zip(P["centers"], P["widths"])):
        sel = np.flatnonzero((x >= f - 5.0 * w) & (x <= f + 5.0 * w))
        if sel.size < 2:
            continue
        xs = [mp.mpf(float(x[i])) for i in sel]
        fm, wm = mp.mpf(float(f)), mp.mpf(float(w))
        y = [[mp.mpf(float(s[::-1][i])) * mp.mpf(float(g[i])) ** 2 / mp.mpf(10) ** 7
              * mp.exp(-((xi - fm) / wm) ** 2 / 2) / (wm * mp.sqrt(2 * mp.pi)) for i, xi in zip(sel, xs)] for s in spec]
        for r in range(len(rows)):         # the trapezoid rule as the definition states it
            acc = mp.mpf(0)
            for k in range(1, len(xs)):
                acc += (xs[k] - xs[k - 1]) * (y[r][k] + y[r][k - 1]) / 2
            val[r, b] = R.LD(mp.nstr(acc * 100, 30))   # 'ergscm2' -> 'nWcm2': 1e-3 x 1e5
    u = R.units_raw(ref["value"], val, ref["A"])
    print("long double vs 60 digits: %.3g units at %s" % R.worst(u, [P["spec_names"][r] for r in rows], P["band_names"]))
    assert u.max() <= 2.0 ** -5 and np.count_nonzero(val) > val.size // 8


def test_panel_holds_what_it_promises(problem):
    P, ref = problem, problem["ref"]
    count = dict(zip(P["band_names"], ref["count"]))
    print("panel: guard %.3g; %s" % (ref["guard"].min(), count))
    assert ref["guard"].min() >= R.GUARD_MIN
    assert P["n_structured"] <= len(P["centers"]) == 33            # nothing structured was cut
    assert count["below the grid"] == 0 and count["above the grid"] == 0 and count["whole grid"] == P["grid"].size
    assert [count["%d-point window" % m] for m in (1, 2, 3)] == [1, 2, 3]
    assert count["duplicate of overlap a"] == count["overlap a"] > 2
    assert list(P["band_names"]) != sorted(P["band_names"], key=lambda n: P["centers"][P["band_names"].index(n)])   # unsorted
    n = P["grid"].size
    W, _, _ = R.weights(P["grid"], P["centers"], P["widths"])
    rng_of = lambda name: np.flatnonzero(W[P["band_names"].index(name)] != 0)[[0, -1]]
    assert tuple(rng_of("range [64, 128)")) == (64, 127) and tuple(rng_of("range [64, 256)")) == (64, 255)
    assert tuple(rng_of("chunk 4096: one point below")) == (4095, 4135) and tuple(rng_of("chunk 4096: one point above")) == (4056, 4096)
    assert tuple(rng_of("chunk 8192: one point below")) == (8191, 8192) and tuple(rng_of("chunk 8192: one point above")) == (8152, 8192)
    lo, hi = rng_of("inside chunk 1")
    assert lo // R.CHUNK == hi // R.CHUNK == 1
    # exact zeros: outside the grid, the 1-point window, and every one-hot probe outside a window
    for name in ("below the grid", "above the grid", "1-point window"):
        b = P["band_names"].index(name)
        assert not ref["value"][:, b].any() and not ref["A"][:, b].any()
    # a one-hot probe returns the single weight (in 'Wm2': x 1e-3)
    hot0 = 2 + int(np.flatnonzero(P["hot"] == 0)[0])
    assert np.array_equal(ref["value"][hot0], W[:, 0] * R.unit_factor("Wm2")) and {0, n - 1, 63, 64, 4095, 4096, 8191, 8192} <= set(P["hot"])


def test_k_plain_recorded_and_respected(problem):
    u = R.units_of(problem["plain"], problem["ref"])
    print("K_PLAIN live: %.3g at %s; dense spectra %s; one-hot probes %.3g"
          % (R.worst(u, problem["spec_names"], problem["band_names"]) + (u[:2].max(axis=1), u[2:].max())))
    assert u.max() <= R.K_PLAIN
    assert R.K_PLAIN <= 2.0 * R.K_PLAIN_MEASURED      # the constant is a record, not a budget


@pytest.mark.parametrize("k", [4096, 4097, 130, 5000])
def test_shard_partials_add_up(problem, k):
    """[0, k + 1) and [k, n): a shard plus the next shard's first point; the trapezoids of the two are those of the whole.
    In long double the two evaluations differ by their own roundings alone: a term W_i s_i is rounded about a dozen times
    (t, its square, exp -- whose argument error the (1 + t^2) of the unit covers --, five products, the interval, the sum)
    at 2^-64 = 2^-11 units each, in the whole and in the shard: 24 x 2^-11 = 0.012 units; held to 2^-5."""
    P = problem
    rows = np.r_[0:2, 2:len(P["spec"]):7]
    spec = P["spec"][rows]
    n = P["grid"].size
    a = R.band_reference(P["grid"], spec[:, :k + 1], P["centers"], P["widths"], g_lo=0)
    b = R.band_reference(P["grid"], spec[:, k:], P["centers"], P["widths"], g_lo=k)
    whole = {"value": P["ref"]["value"][rows], "A": P["ref"]["A"][rows]}
    u = R.units_of(a["value"] + b["value"], whole)
    print("shards cut at %d: %.3g units (whole guard %.3g, shard guards %.3g %.3g)" % (k, u.max(), P["ref"]["guard"].min(),
                                                                                       a["guard"].min(), b["guard"].min()))
    assert u.max() <= 2.0 ** -5 and a["value"].any() and b["value"].any()
    # ... and the plain evaluation of a shard is the oracle on the grid slice: within its own K_PLAIN of the partial
    pa = R.units_of(R.oracle_plain(P["grid"], spec[:, k:], P["centers"], P["widths"], g_lo=k), b)
    assert pa.max() <= R.K_PLAIN


def test_exact_end_cases(problem):
    """f -+ 5 w is bitwise the grid value x_k: the end point belongs to the window, and a one-hot spectrum there returns its
    (half-interval) weight, not 0."""
    P, E = problem, problem["exact"]
    (f_lo, f_hi), w, xk, k = E["centers"], 0.25, E["xk"], E["k"]
    assert f_lo - 5.0 * w == xk and f_hi + 5.0 * w == xk and xk == 1e7 / P["grid"][k]
    far = R.guard(P["grid"], [f_lo + 2.5, f_hi - 2.5], [1e-9, 1e-9], 5.0)      # the two far ends (or the grid's end)
    assert far.min() >= R.GUARD_MIN
    ref = E["ref"]
    assert np.all(ref["count"] >= 3) and np.all(ref["value"][0] > 0) and np.all(ref["value"][1] > 0)
    W, _, _ = R.weights(P["grid"], E["centers"], E["widths"])
    n = P["grid"].size
    assert W[0, k] != 0 and W[1, k] != 0 and W[0, k + 1] == 0 and W[1, k - 1] == 0     # x_k is the first / the last point (nm order)
    u = R.units_of(R.oracle_plain(P["grid"], E["spec"], E["centers"], E["widths"]), ref)
    print("exact ends: plain %.3g units" % u.max())
    assert u.max() <= R.K_PLAIN


@pytest.mark.parametrize("defect", R.DEFECTS)
def test_seeded_defects_are_over_the_limit(problem, defect):
    """The teeth of the bound: each defect alone puts the plain restatement beyond the kernels' limit 8 x max(K_PLAIN, 1)
    on at least one probe of the panel (with its two exact-end bands); without a defect it stays inside."""
    P, E = problem, problem["exact"]
    k_plain = max(R.units_of(P["plain"], P["ref"]).max(),
                  R.units_of(R.oracle_plain(P["grid"], E["spec"], E["centers"], E["widths"]), E["ref"]).max())
    lim = R.limit(k_plain)
    run = lambda d: (R.units_of(R.plain_fp64(P["grid"], P["spec"], P["centers"], P["widths"], defect=d), P["ref"]),
                     R.units_of(R.plain_fp64(P["grid"], E["spec"], E["centers"], E["widths"], defect=d), E["ref"]))
    clean, bad = run(None), run(defect)
    n_over = int((bad[0] > lim).sum() + (bad[1] > lim).sum())
    print("%s: panel %.3g units at %s; exact ends %.3g; %d probes over the limit %.3g (no defect: %.3g, %.3g)"
          % ((defect,) + R.worst(bad[0], P["spec_names"], P["band_names"]) + (bad[1].max(), n_over, lim, clean[0].max(), clean[1].max())))
    assert clean[0].max() <= lim and clean[1].max() <= lim
    assert max(bad[0].max(), bad[1].max()) > lim
    # a defect must show where the result is NOT an exact zero too (a wrong zero / non-zero is the easy catch)
    live = [(b > lim) & (np.asarray(r["A"], np.float64) > 0) for b, r in zip(bad, (P["ref"], E["ref"]))]
    assert live[0].any() or live[1].any()


def test_fov_reference_is_the_closed_form():
    """fov_reference on exact small integers reproduces smm.fov_closed_form to fp64 rounding, with and without an edge."""
    from spectrobot_amd import engine, spect_main_module as smm
    rng = np.random.default_rng(5)
    s = rng.integers(-9, 10, (6, 3, 4)).astype(float)
    rots = [0.0, 20.0]
    val, A = R.fov_reference(s, np.abs(s), engine.fov_factors(rots))
    plain = smm.fov_closed_form(s[0::3], s[1::3], s[2::3], rots)
    u = R.units_raw(plain, val, A)
    print("fov closed form against its long-double expression: %.3g units" % u.max())
    assert val.shape == plain.shape == (2, 3, 4) and u.max() <= 8.0 and np.all(A >= np.abs(val))
