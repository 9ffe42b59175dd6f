"""engine.hires_to_lowres_instrument (sr_hires_to_lowres_instr_shard_dev: sr_lowres_weights_kernel<true>,
sr_lowres_apply_kernel<3>, sr_lowres_sum_kernel) against the extended-precision reference of
tests/lowres_instr_reference.py: the band values with their derivatives to the band centre and to the logarithm of the ILS
width, the windows' membership held fixed.

Row 0 must be engine.hires_to_lowres itself, bit for bit.  Rows 1 and 2 are held to 8 x max(K_PLAIN_INSTR, 1) units of
2^-53 A + 1e-290 with the A of the helper's docstring, K_PLAIN_INSTR being what plain_fp64_instr (plain numpy, written in
the helper) measures against the reference on the test's own (spectrum, band) pairs -- never what a kernel gives.  Bands
outside the grid and windows of fewer than two points must be exact 0.0 in all three rows.  Needs a real MI355X."""
import numpy as np
import pytest

import lowres_reference as R
import lowres_instr_reference as I

pytestmark = pytest.mark.gpu
SEED = 20261018
GRID = (2975.0, 5e-4)


@pytest.fixture(scope="module")
def eng():
    import torch
    assert torch.cuda.is_available(), "these tests need the GPU"
    from spectrobot_amd import engine
    engine.set_device(0)
    return engine


@pytest.fixture(scope="module")
def panel():
    """The 8193-point, 33-band panel (two chunk boundaries at 4096, the 64-point slots, three band tiles, one-hot probes)
    with its references in the three units, computed once."""
    P = R.panel(GRID[0], GRID[1], 8193, 33, SEED)
    assert P["n_structured"] <= 33 and R.guard(P["grid"], P["centers"], P["widths"]).min() >= R.GUARD_MIN
    P["ref"] = {u: I.band_reference_instr(P["grid"], P["spec"], P["centers"], P["widths"], units=u) for u in R.UNITS}
    P["plain"] = {u: I.plain_fp64_instr(P["grid"], P["spec"], P["centers"], P["widths"], units=u) for u in R.UNITS}
    return P


def _t(v):
    import torch
    return torch.tensor(np.ascontiguousarray(v, dtype=np.float64), device="cuda")


def _check(tag, got3, ref, plain, spec_names, band_names, extra=()):
    """got3 [n_spec, 3, n_bands] against a band_reference_instr; every figure is printed before anything is asserted."""
    got3 = np.asarray(got3)
    assert got3.shape == ref["value"].shape
    k_plain = float(I.units_of(plain, ref)[:, 1:].max())
    lim = R.limit(k_plain)
    u = I.units_of(got3, ref)
    rows = [(I.ROWS[k],) + R.worst(u[:, k], spec_names, band_names) for k in range(3)] + list(extra)
    print("\n%s: K_PLAIN_INSTR %.3g limit %.3g" % (tag, k_plain, lim))
    for name, m, where in rows:
        print("  %-36s %10.3g units%s at %s" % (name, m, "  OVER" if not m <= lim else "", where))
    dead = ref["count"] < 2
    assert np.all(got3[:, :, dead] == 0.0), "a band without a trapezoid is not an exact 0.0 in every row"
    bad = [r for r in rows if not r[1] <= lim]
    assert not bad, "over 8 x max(K_PLAIN_INSTR, 1) = %.3g: %s" % (lim, bad)
    return lim


@pytest.mark.parametrize("units", R.UNITS)
def test_instrument_rows_on_the_panel(eng, panel, units):
    P = panel
    dev = _t(P["spec"])
    low, dc, dw = eng.hires_to_lowres_instrument(dev, P["grid"], P["centers"], P["widths"], out_units=units)
    value = eng.hires_to_lowres(dev, P["grid"], P["centers"], P["widths"], out_units=units)
    assert low.shape == dc.shape == dw.shape == value.shape == (len(P["spec"]), 33)
    assert np.array_equal(low, value), "row 0 is not engine.hires_to_lowres, bit for bit"
    assert np.array_equal(eng.hires_to_lowres(dev, P["grid"], P["centers"], P["widths"], out_units=units), value)   # (the cache, both ways)
    dead = P["ref"][units]["count"] < 2
    assert dead.sum() >= 3 and np.any(dc[:, ~dead] != 0.0) and np.any(dw[:, ~dead] != 0.0)
    _check("hires_to_lowres_instrument 8193 pts 33 bands %s" % units, np.stack([low, dc, dw], axis=1), P["ref"][units],
           P["plain"][units], P["spec_names"], P["band_names"])


@pytest.mark.parametrize("n_pts,k", [(8193, 5000), (300, 130)])
def test_exact_window_ends(eng, n_pts, k):
    """The two bands of exact_end_cases: the window's end is bitwise the grid value x_k, the end point belongs to the
    window, and it has t = -+n_sigma exactly: its weights in the derivative rows are W (-+5 / w) and 24 W."""
    g, _ = R.make_grid(GRID[0], GRID[1], n_pts)
    centers, widths, xk = R.exact_end_cases(g, k)
    assert centers[0] - 5.0 * 0.25 == xk and centers[1] + 5.0 * 0.25 == xk and xk == 1e7 / g[k] and np.all(widths == 0.25)
    far = R.guard(g, [centers[0] + 2.5, centers[1] - 2.5], [1e-9, 1e-9], 5.0)
    assert far.min() >= R.GUARD_MIN, far
    rng = np.random.default_rng([SEED, n_pts, k])
    spec = np.zeros((5, n_pts))
    spec[0, k] = spec[1, k - 1] = spec[2, k + 1] = 1.0
    spec[3] = rng.uniform(0.5, 1.5, n_pts)
    spec[4] = rng.choice([-1.0, 1.0], n_pts) * 10.0 ** rng.uniform(-6.0, 0.0, n_pts)
    names = ["one-hot at k", "one-hot at k - 1", "one-hot at k + 1", "positive noise", "signed"]
    ref = I.band_reference_instr(g, spec, centers, widths)
    assert np.all(ref["count"] >= 2)
    got = np.stack(eng.hires_to_lowres_instrument(_t(spec), g, centers, widths), axis=1)
    assert np.array_equal(got[:, 0], eng.hires_to_lowres(_t(spec), g, centers, widths))
    _check("exact ends, %d pts, k %d" % (n_pts, k), got, ref, I.plain_fp64_instr(g, spec, centers, widths), names, ["lo == x_k", "hi == x_k"])
    # the end point: t = -5 under band 0 (x_k = f - 5 w), +5 under band 1
    assert np.all(got[0, 0] > 0) and got[0, 1, 0] < 0 < got[0, 1, 1] and np.all(got[0, 2] > 0)
    assert got[2, 1, 0] == 0.0 and got[1, 1, 1] == 0.0 and got[2, 2, 0] == 0.0 and got[1, 2, 1] == 0.0   # the neighbours outside


def test_shards_add_up(eng, panel):
    """A split at g_lo = 4097: [0, 4098) and [4097, 8193), a shard plus the next shard's first point.  Each shard's three
    rows against the reference's partial sums, their sum against the whole."""
    P = panel
    rows = np.r_[0:2, 2:len(P["spec"]):5]
    spec, names = P["spec"][rows], [P["spec_names"][r] for r in rows]
    cw = (P["centers"], P["widths"])
    whole_ref = dict((key, v[rows] if key in ("value", "A") else v) for key, v in P["ref"]["Wm2"].items())
    got = {}
    for name, (a, b) in (("shard 0", (0, 4098)), ("shard 1", (4097, 8193))):
        three = eng.hires_to_lowres_instrument(_t(spec[:, a:b]), P["grid"], *cw, g_lo=a)
        got[name] = np.stack(three, axis=1)
        assert np.array_equal(three[0], eng.hires_to_lowres(_t(spec[:, a:b]), P["grid"], *cw, g_lo=a))
        ref = I.band_reference_instr(P["grid"], spec[:, a:b], *cw, g_lo=a)
        _check("%s [%d, %d)" % (name, a, b), got[name], ref, I.plain_fp64_instr(P["grid"], spec[:, a:b], *cw, g_lo=a), names,
               P["band_names"])
    total = got["shard 0"] + got["shard 1"]
    u = I.units_of(total, whole_ref)
    lim = R.limit(I.units_of(P["plain"]["Wm2"][rows], whole_ref)[:, 1:].max())       # the whole's own pairs
    print("\nshard 0 + shard 1 against the whole: %s units (limit %.3g)" % ([float(u[:, k].max()) for k in range(3)], lim))
    assert got["shard 0"][:, 1:].any() and got["shard 1"][:, 1:].any() and u.max() <= lim


def test_unsorted_and_duplicated_bands(eng, panel):
    """The panel's bands are shuffled and hold a duplicate; reversed, and with every band given twice (66 bands: five
    tiles), each band's three rows are bitwise what the panel's order gave."""
    P = panel
    assert "duplicate of overlap a" in P["band_names"] and np.any(np.diff(P["centers"]) < 0) and np.any(np.diff(P["centers"]) > 0)
    rows = np.r_[0:2, 2:len(P["spec"]):7]
    dev = _t(P["spec"][rows])
    base = np.stack(eng.hires_to_lowres_instrument(dev, P["grid"], P["centers"], P["widths"]), axis=1)
    a, b = P["band_names"].index("overlap a"), P["band_names"].index("duplicate of overlap a")
    assert np.array_equal(base[:, :, a], base[:, :, b]) and base[:, 1:, a].any()
    order = np.concatenate([np.arange(33)[::-1], np.arange(33)])
    twice = np.stack(eng.hires_to_lowres_instrument(dev, P["grid"], P["centers"][order], P["widths"][order]), axis=1)
    assert twice.shape == (len(rows), 3, 66) and np.array_equal(twice, base[:, :, order])
