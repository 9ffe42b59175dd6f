"""Tabulated absorbers (engine.AbsorberTable, retrieval.TableGas, sr_abs_table_*) checked on the host, no GPU: the ABI
surface, the rows' plan against the long-double statement of the policy, the two file readers on the synthetic fixtures,
the reference's temperature derivatives against its own central differences, the honesty of its bounds (a plain fp64
evaluation stays inside half of each), TableGas's cache key, and what the line-list call sites do with a TableGas."""
import os
import re
import sys

import numpy as np
import pytest

import absorber_table_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
NAMES = ("sr_abs_table_create", "sr_abs_table_destroy", "sr_abs_table_layers_dev")


def test_abi_surface():
    from spectrobot_amd import _lib
    header = open(os.path.join(ROOT, "include", "spectrobot_hip.h")).read()
    for name in NAMES:
        assert re.search(r"^int %s\(" % name, header, re.M), name
        assert name in _lib.SYMBOLS and hasattr(_lib.lib, name)
    assert _lib.lib.sr_abi_version() == 1
    for macro, value in (("SR_MAX_ABS_SETS", _lib.SR_MAX_ABS_SETS), ("SR_MAX_ABS_VALUES", _lib.SR_MAX_ABS_VALUES),
                         ("SR_MAX_ABS_ROWS", _lib.SR_MAX_ABS_ROWS)):
        assert int(re.search(r"#define %s (\d+)" % macro, header)[1]) == value


def _table(labels):
    from spectrobot_amd import engine
    return engine.AbsorberTable(R.panel_sets(0, labels=labels))


@pytest.mark.parametrize("labels", [False, True])
def test_plan_against_the_policy(labels):
    tab = _table(labels)
    # below, at (coldest, inner, hottest), between and above the set temperatures
    temps = np.array([140.0, 150.0, 170.0, 187.3, 200.0, 230.0, 250.0, 299.0, 300.0, 310.0])
    # pressure groups at 1 and 20 hPa: sqrt(20) is the tie in ln P (the lower group wins), its neighbours fall either side
    tie = float(np.sqrt(20.0))
    press = np.array([0.1, 1.0, tie, tie * (1 - 1e-12), tie * (1 + 1e-12), 20.0, 50.0, tie, 3.0, 8.0]) if labels else None
    set2, w2, dw2 = tab.plan(temps, press)
    r2, rw, rdw = R.plan(tab.set_temp, tab.set_press, temps, press)
    assert np.array_equal(set2, r2)
    assert np.max(np.abs(w2 - rw)) <= 2.0 ** -52 and np.max(np.abs(dw2 - rdw) / np.maximum(np.abs(rdw), 1e-300)) <= 2.0 ** -52
    assert np.all(w2[:, 0] + w2[:, 1] == 1.0) and np.all(dw2[:, 0] + dw2[:, 1] == 0.0)   # exactly
    if labels:
        # (whether sqrt(20) is a tie in the doubles of ln P or not, the reference decides it the same way; its two
        # neighbours fall to either side; rows 7 .. 9 use the group their pressure is nearer to)
        low = {0, 1}
        assert set(set2[3]) <= low and not set(set2[4]) <= low and set(set2[0]) <= low and not set(set2[6]) <= low
    else:
        # exactly at a set: that set with weight 1 and the derivative of the interval above; the hottest: none above
        assert tuple(set2[1]) == (0, 1) and tuple(w2[1]) == (1.0, 0.0) and dw2[1, 1] == 1.0 / 50.0
        assert tuple(set2[4]) == (1, 2) and tuple(w2[4]) == (1.0, 0.0) and dw2[4, 0] == -1.0 / 50.0
        assert tuple(set2[8]) == (3, 3) and tuple(w2[8]) == (1.0, 0.0) and tuple(dw2[8]) == (0.0, 0.0)
        assert tuple(set2[0]) == (0, 0) and tuple(dw2[0]) == (0.0, 0.0) and tuple(set2[9]) == (3, 3)
    # labels without row pressures: every set
    if labels:
        s_all, _, _ = tab.plan(temps)
        assert np.array_equal(s_all, _table(False).plan(temps)[0])


def test_plan_refuses_two_sets_at_one_temperature():
    from spectrobot_amd import engine
    s = R.panel_sets(0)
    with pytest.raises(ValueError):
        engine.AbsorberTable([s[0], (s[0][0],) + s[1][1:]])


def _fixtures():
    sys.path.insert(0, GOLDEN)
    try:
        import make_absorber_fixtures as M
    finally:
        sys.path.remove(GOLDEN)
    return M


def test_read_xsc():
    from spectrobot_amd import spect_classes as spcl
    want = _fixtures().xsc_sets()
    got = spcl.read_xsc(os.path.join(GOLDEN, "absorber_sample.xsc"))
    assert len(got) == len(want) == 4
    for g, w in zip(got, want):
        assert g[0] == w[0] and g[1] == w[1] and g[2] == w[2] and np.array_equal(g[3], w[3])
        assert abs(g[4] - w[4]) <= 1e-12 * w[4]
    assert abs(got[0][4] - 20.0 * 1.333224) < 1e-12 and spcl.TORR_TO_HPA == 1.333224


def test_read_cia():
    from spectrobot_amd import spect_classes as spcl
    want = _fixtures().cia_sets()
    got = spcl.read_cia(os.path.join(GOLDEN, "absorber_sample.cia"))
    assert len(got) == len(want) == 3
    for g, w in zip(got, want):
        assert len(g) == 4 and g[0] == w[0] and g[1] == w[1] and abs(g[2] - w[2]) <= 1e-12 * w[2] and np.array_equal(g[3], w[3])
    assert min(v.min() for _, _, _, v in got) < 0          # negative values are kept as given
    with pytest.raises(ValueError, match="irregular"):
        spcl.read_cia(os.path.join(GOLDEN, "absorber_irregular.cia"))


def _random_case(rng):
    sets = []
    for k in range(3):
        n = int(rng.integers(2, 400))
        sets.append((150.0 + 40 * k, 2900 + rng.uniform(-5, 5), 10 ** rng.uniform(-3, 0), rng.normal(size=n) * 10 ** rng.uniform(-25, -18)))
    nr = 4
    w, d = rng.uniform(0, 1, nr), rng.uniform(0.01, 0.1, nr)
    return (sets, rng.integers(0, 3, (nr, 2)), np.stack([1 - w, w], 1), np.stack([-d, d], 1), rng.uniform(100, 300, nr),
            10 ** rng.uniform(0, 18, nr), 2895.0 + rng.uniform(0, 5), 10 ** rng.uniform(-4, -2), int(rng.integers(0, 5000)), 64)


def test_bounds_are_honest():
    """A plain fp64 evaluation of 200 random cases (windows with c2 nu / T >= 13) stays inside HALF of each bound."""
    rng = np.random.default_rng(20261020)
    worst = dict(abs=0.0, emi=0.0, dabs=0.0, demi=0.0)
    for _ in range(200):
        a = _random_case(rng)
        L, D = R.evaluate(*a), R.evaluate(*a, dtype=np.float64)
        for k in worst:
            b, err = L["b_" + k], np.abs(D[k].astype(R.LD) - L[k])
            assert np.all(err[b == 0] == 0)
            if np.any(b > 0):
                worst[k] = max(worst[k], float(np.max(err[b > 0] / b[b > 0])))
    print("plain fp64 / bound:", worst)
    assert all(v <= 0.5 for v in worst.values()), worst


def test_reference_derivatives_against_its_own_differences():
    """dabs, demi of the reference against long-double central differences in T of abs, emi, the plan's weights moved
    along their own derivatives (they are linear in T) and the scale held fixed."""
    sets = R.panel_sets(0)
    n = len(R.ROW_TEMPS)
    set2 = np.array([[0, 0], [1, 2], [0, 1], [1, 2], [3, 3]])
    w2 = np.array([[1, 0], [1, 0], [0.6, 0.4], [0.4, 0.6], [1, 0]], dtype=float)
    dw2 = np.array([[0, 0], [-0.02, 0.02], [-0.02, 0.02], [-0.02, 0.02], [0, 0]], dtype=float)
    w0, step, n_pts = R.GRID
    L = R.evaluate(sets, set2, w2, dw2, R.ROW_TEMPS, R.ROW_SCALE, w0, step, 0, n_pts)
    h = 2.0 ** -10        # exactly representable moves: T +- h and w +- h dw are the doubles the formulas take
    up = R.evaluate(sets, set2, w2 + h * dw2, None, R.ROW_TEMPS + h, R.ROW_SCALE, w0, step, 0, n_pts)
    dn = R.evaluate(sets, set2, w2 - h * dw2, None, R.ROW_TEMPS - h, R.ROW_SCALE, w0, step, 0, n_pts)
    for k in ("abs", "emi"):
        fd = (up[k] - dn[k]) / (2 * R.LD(h))
        big = np.maximum(np.max(np.abs(L["d" + k]), axis=1, keepdims=True), np.max(np.abs(L[k]), axis=1, keepdims=True) / 100.0)   # (rows with dw = 0 have dabs = 0)
        # abs is linear in T (exact up to the roundings of w +- h dw: 2^-53 / h); emi's third derivative gives h^2 x'''
        assert np.max(np.abs(fd - L["d" + k]) / big) < 1e-6, k
    assert np.any(L["dabs"][1] != 0) and np.all(L["dabs"][0] == 0) and np.any(L["demi"][0] != 0)


class _Scene(object):
    def __init__(self, n=6):
        self.temps, self.press = np.linspace(150.0, 180.0, n), np.geomspace(10.0, 0.1, n)
        self.nd = self.press / self.temps
        self.grid = R.grid_nu(2900.0, 0.01, 0, 300)


def test_table_gas_cache_key_is_by_content():
    from spectrobot_amd import engine, retrieval as rt
    tab = engine.AbsorberTable(R.panel_sets(0))
    sc = _Scene()
    g = rt.TableGas("haze", tab, np.ones(6), scale=lambda s: s.nd * 0.98)
    k0 = g.cache_key(sc, 0, 300)
    sc.temps, sc.press, sc.nd = sc.temps.copy(), sc.press.copy(), sc.nd.copy()        # new objects, same content
    assert g.cache_key(sc, 0, 300) == k0
    for attr in ("temps", "press", "nd"):
        moved = _Scene()
        getattr(moved, attr)[2] *= 1.0 + 1e-15 * 4
        assert g.cache_key(moved, 0, 300) != k0, attr
    assert g.cache_key(sc, 0, 200) != k0 and g.cache_key(sc, 10, 300) != k0
    fixed = rt.TableGas("haze", tab, np.ones(6), scale=np.full(6, 2.0))
    assert fixed.cache_key(sc, 0, 300) == rt.TableGas("x", tab, np.ones(6), scale=np.full(6, 2.0)).cache_key(sc, 0, 300)
    assert fixed.cache_key(sc, 0, 300) != rt.TableGas("x", tab, np.ones(6)).cache_key(sc, 0, 300)
    assert g.lineset is None and g.accumulate_into is None and g.source


def test_line_list_call_sites_accept_or_refuse_a_table_gas():
    from spectrobot_amd import engine, retrieval as rt
    tab = engine.AbsorberTable(R.panel_sets(0))
    haze = rt.TableGas("haze", tab, np.ones(4))
    # single_rad_keys: a ('gas', g) part under 'iso_0'; a tracked level of it is refused by name
    assert rt.single_rad_keys([haze]) == [(("haze", "iso_0"), 0, None)]
    with pytest.raises(ValueError, match="not a level of gas haze"):
        rt.single_rad_keys([haze], {("haze", "iso_0"): [0]})
    z = np.arange(4) * 50.0 + 100.0
    scene = rt.LimbScene(R.grid_nu(2900.0, 0.01, 0, 300), z, np.full(4, 160.0), np.geomspace(5.0, 0.05, 4), [haze], [3447.0], [1.0])
    with pytest.raises(ValueError, match="TableGas"):
        rt.lut_coefficients(scene)
    with pytest.raises(ValueError, match="TableGas"):
        rt._refuse_table_gas(haze, "the level-factored route of the radiance budget")
    # accumulate_into names a plain line gas of the scene, or the scene is refused
    with pytest.raises(ValueError, match="accumulate_into"):
        rt.LimbScene(scene.grid, z, scene.temps, scene.press, [rt.TableGas("cont", tab, np.ones(4), accumulate_into="CH4")], [3447.0], [1.0])
    with pytest.raises(ValueError, match="accumulate_into"):
        rt.LimbScene(scene.grid, z, scene.temps, scene.press, [haze, rt.TableGas("cont", tab, np.ones(4), accumulate_into="haze")],
                     [3447.0], [1.0])
