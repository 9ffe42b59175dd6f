"""The look-up-table route on the CPU: LutSet.interp_plan against the planner of tests/lut_reference.py on lattices and
queries that include every tie, the reference module held to its own bounds (a plain fp64 restatement of the kernel's
formula passes, six seeded defects do not), and the refusals of sr_lut_interp_dev, which all come before anything is
staged.  No GPU."""
import ctypes as C

import numpy as np
import pytest

import lut_reference as LR

LD = LR.LD


# ----------------------------------------------------------------------------------------------------------------------
# the planner
# ----------------------------------------------------------------------------------------------------------------------
def _log_pressures(n, step):
    """The pressure lattice retrieval.lut_coefficients builds for layers between 1 hPa and p_max, restated."""
    p_min, p_max = 1.0, (1.0 if n == 1 else float(np.exp((n - 1.25) * step)))
    Ps = np.exp(np.arange(np.floor(np.log(p_min)), np.log(p_max) + step, step))
    assert Ps.size == n
    return Ps


def _lattice(n_t, n_p, kind):
    if kind == "T 5 K, ln P 1.0":
        return 100.0 + 5.0 * np.arange(n_t), _log_pressures(n_p, 1.0)
    if kind == "T 2.5 K, ln P 0.5":
        return 117.5 + 2.5 * np.arange(n_t), _log_pressures(n_p, 0.5)
    assert kind == "T geometric, P linear"
    return 90.0 * 1.03 ** np.arange(n_t), 0.5 + 1.5 * np.arange(n_p)


def _lutset(Ps, Ts):
    from spectrobot_amd import spect_main_module as smm
    lut = smm.LutSet(6, 1, 16.0)
    assert lut.device is None
    lut.PTcouples = [[float(P), float(T)] for P in Ps for T in Ts]
    return lut


def _queries(Ps, Ts, rng):
    """[(P, T, raises)]: every temperature query at a few pressures, every pressure query at a few temperatures."""
    mid_t = 0.5 * (Ts[:-1] + Ts[1:])
    t_q = np.concatenate([Ts, mid_t, rng.uniform(Ts[:-1], Ts[1:]), [Ts[0] - 7.3, Ts[0] - 2.5, Ts[-1] + 0.1, Ts[-1] + 11.0]])
    t_few = [float(Ts[0]), float(mid_t[0]), float(mid_t[-1]), float(rng.uniform(Ts[0], Ts[-1]))]
    p_q = [0.5 * Ps[0], Ps[0], np.nextafter(Ps[0], np.inf), Ps[-1]] + list(Ps)
    if Ps.size > 1:
        p_q += list(0.5 * (Ps[:-1] + Ps[1:])) + list(rng.uniform(Ps[:-1], Ps[1:]))
    p_few = p_q[:2] + ([float(Ps[Ps.size // 2]), float(0.5 * (Ps[0] + Ps[1])), float(rng.uniform(Ps[0], Ps[-1]))] if Ps.size > 1 else [])
    p_q.append(np.nextafter(Ps[-1], np.inf))          # one ulp above the highest pressure: raises
    return [(float(P), float(T), bool(P > Ps[-1])) for T in t_q for P in p_few] + [(float(P), float(T), bool(P > Ps[-1])) for P in p_q for T in t_few]


def _ulps(a, b):
    return abs(a - b) / np.spacing(abs(np.float64(b)))


def _sums_to_one(w1, w2):
    """w1 + w2 == 1 within one ulp of the largest of 1, |w1|, |w2|: w1 = fl(1 - w2) is off by half an ulp of its own, the
    sum rounds once more.  Between the nodes (weights in [0, 1]) that is an ulp of 1; an extrapolated pair such as
    (4.96, -3.96) cannot do better than an ulp of 4."""
    return abs((w1 + w2) - 1.0) <= np.spacing(max(1.0, abs(w1), abs(w2)))


@pytest.mark.parametrize("kind", ["T 5 K, ln P 1.0", "T 2.5 K, ln P 0.5", "T geometric, P linear"])
@pytest.mark.parametrize("n_p", [1, 2, 7])
@pytest.mark.parametrize("n_t", [2, 3, 8, 17, 40])
def test_interp_plan_equals_the_reference_rule(n_t, n_p, kind):
    """Rows equal, weights equal to 2 ulp and finite, T1 != T2, P1 != P2, each weight pair sums to 1 within an ulp (_sums_to_one):
    at every node, every temperature and pressure midpoint (the ties), random points between the nodes, temperatures
    outside the lattice, P below, at and just above the lowest pressure and at the highest; one ulp above the highest
    pressure both raise."""
    Ts, Ps = _lattice(n_t, n_p, kind)
    lut = _lutset(Ps, Ts)
    PT = lut.PTcouples
    rng = np.random.default_rng([n_t, n_p, len(kind)])
    n_tie = 0
    for P, T, raises in _queries(Ps, Ts, rng):
        if raises:
            with pytest.raises(ValueError):
                LR.plan(PT, P, T)
            with pytest.raises(ValueError):
                lut.interp_plan(P, T)
            continue
        want_i, want_w = LR.plan(PT, P, T)
        got_i, got_w = lut.interp_plan(P, T)
        where = (P, T, got_i, got_w, want_i, want_w)
        assert [int(i) for i in got_i] == want_i, where
        assert np.all(np.isfinite(got_w)), where
        assert all(_ulps(g, w) <= 2.0 for g, w in zip(got_w, want_w)), where
        i1, i2, i3, i4 = got_i
        assert PT[i1][1] != PT[i2][1] and PT[i1][0] == PT[i2][0], where
        assert _sums_to_one(got_w[2], got_w[3]), where
        if P <= Ps[0]:
            assert i3 == -1 and i4 == -1 and got_w[0] == 0.0 and got_w[1] == 0.0 and PT[i1][0] == Ps[0], where
        else:
            assert PT[i1][0] != PT[i3][0] and PT[i3][0] == PT[i4][0] and PT[i1][1] == PT[i3][1] and PT[i2][1] == PT[i4][1], where
            assert _sums_to_one(got_w[0], got_w[1]), where
        d = np.sort(np.abs(Ts - T))
        n_tie += int(d[0] == d[1])
    if kind != "T geometric, P linear":
        assert n_tie >= 2 * (n_t - 1)       # the midpoints of an even lattice are exact ties, each asked at two pressures or more


def test_interp_plan_midpoints_of_the_lattices_in_use():
    """An 8-node lattice at 5 K and the lattice of temp_step=2.5, queried at every midpoint: the two temperatures differ
    and the weights are (1/2, 1/2).  (With the reference's unstable argsort 3 of the 7 midpoints of the first lattice name
    one node twice and give weights (-inf, inf).)"""
    for Ts in (150.0 + 5.0 * np.arange(8), 120.0 + 2.5 * np.arange(30)):
        lut = _lutset([1.0, 2.0], Ts)
        for k in range(Ts.size - 1):
            idx, w = lut.interp_plan(0.5, 0.5 * (Ts[k] + Ts[k + 1]))
            assert idx == [k, k + 1, -1, -1] and w == [0.0, 0.0, 0.5, 0.5], (Ts[k], idx, w)
            idx, w = lut.interp_plan(1.5, 0.5 * (Ts[k] + Ts[k + 1]))
            assert idx == [k, k + 1, Ts.size + k, Ts.size + k + 1] and w == [0.5, 0.5, 0.5, 0.5], (Ts[k], idx, w)


def test_logarithmic_lattice_extrapolates_from_the_two_nearest_nodes():
    """THE REFERENCE'S BEHAVIOUR, kept on purpose: the two nodes are the nearest two in LINEAR pressure (LutSet.calculate,
    spect_main_module.py:1027-1030), which on a logarithmic lattice is often the pair BELOW the query.  At P = 8 hPa on
    the nodes 1, e, e^2, e^3 hPa the distances are 7, 5.28, 0.61 and 12.09: the rule takes e^2 and e, and the query is
    extrapolated from them (wP1 > 1, wP2 < 0) though e^2 and e^3 bracket it.  Not to be 'fixed' here."""
    Ps, Ts = np.exp(np.arange(4.0)), np.array([140.0, 150.0])
    lut = _lutset(Ps, Ts)
    idx, w = lut.interp_plan(8.0, 143.0)
    assert idx == [4, 5, 2, 3] and idx == LR.plan(lut.PTcouples, 8.0, 143.0)[0]
    assert lut.PTcouples[idx[0]][0] == Ps[2] < 8.0 and lut.PTcouples[idx[2]][0] == Ps[1] < 8.0
    assert w[0] > 1.0 and w[1] < 0.0 and w == LR.plan(lut.PTcouples, 8.0, 143.0)[1]
    assert w[1] == (8.0 - Ps[2]) / (Ps[1] - Ps[2]) and abs(w[2] - 0.7) < 1e-15 and abs(w[3] - 0.3) < 1e-15


def test_non_rectangular_couple_list_raises():
    lut = _lutset([1.0, 2.0], [140.0, 150.0, 160.0])
    lut.PTcouples.remove([2.0, 150.0])
    with pytest.raises(ValueError, match="couple not found"):
        lut.interp_plan(1.2, 158.0)        # needs (2 hPa, 150 K)
    with pytest.raises(ValueError, match="couple not found"):
        LR.plan(lut.PTcouples, 1.2, 158.0)
    assert lut.interp_plan(0.5, 158.0)[0] == [2, 1, -1, -1]     # the lowest pressure's row is complete


# ----------------------------------------------------------------------------------------------------------------------
# the reference checks itself
# ----------------------------------------------------------------------------------------------------------------------
def _shares(c, defect=None):
    """Worst shares of the three bounds of lut_reference.plain on a synthetic case: (interpolation at bilinear steps,
    at T-only steps, combine)."""
    val, M = LR.interpolate(c["tab"], c["idx4"], c["wgt4"])
    lim = LR.limit_interp(M, c["idx4"])
    bil = LR.bilinear_steps(c["idx4"])
    with np.errstate(invalid="ignore", over="ignore"):
        v = LR.plain(c["tab"], c["idx4"], c["wgt4"], defect=defect)
        ab, em = LR.plain(c["tab"], c["idx4"], c["wgt4"], c["pop"], c["abs0"], c["emi0"], defect=defect)
    v = np.where(np.isfinite(v), v, np.inf)      # a NaN row read by a defect: counted as infinitely far off
    ab, em = (np.where(np.isfinite(a), a, np.inf) for a in (ab, em))
    r = np.abs(v.astype(LD) - val) / lim
    (wa, we), (Ya, Ye) = LR.combine(c["tab"], c["idx4"], c["wgt4"], c["pop"], c["abs0"], c["emi0"])
    rc = max(float(np.max(np.abs(ab.astype(LD) - wa) / LR.limit_combine(Ya))), float(np.max(np.abs(em.astype(LD) - we) / LR.limit_combine(Ye))))
    return (float(r[:, bil].max()) if bil.any() else 0.0, float(r[:, ~bil].max()) if (~bil).any() else 0.0, rc)


def _cases():
    return [(n_pts, n_pt, n_steps) for n_pts in (1, 257) for n_pt in LR.N_PT for n_steps in LR.N_STEPS]


def test_synthetic_cases_are_what_they_claim():
    seen_dead = False
    for n_pts, n_pt, n_steps in _cases():
        c = LR.case(n_pts, n_pt, n_steps, combine_inputs=True)
        idx, w, tab = c["idx4"], c["wgt4"], c["tab"]
        bil = LR.bilinear_steps(idx)
        assert np.all(idx[bil] >= 0) and np.all(idx[bil] < n_pt) and np.all(idx[~bil, :2] >= 0) and np.all(idx[~bil, 2:] == -1)
        assert np.all(np.isfinite(w)) and np.all(w[~bil, :2] != 0.0)
        named = np.unique(idx[idx >= 0])
        assert np.all(np.isfinite(tab[:, named])) and np.all(np.isnan(tab[:, c["dead"]])) and named.size + c["dead"].size == n_pt
        seen_dead |= c["dead"].size > 0
        if n_steps >= 3:
            assert bil.any() and (~bil).any() and 0.0 in c["pop"] and 1e-250 in c["pop"]
        if n_steps == 70:
            assert np.any(w < 0.0) and np.any(w > 1.0) and np.any(idx[bil, 0] == idx[bil, 1]) and np.any(idx[bil, 2] == idx[bil, 3])
        if n_pts == 257:
            live = np.abs(tab[:, named])
            assert live.max() / live.min() > 1e55 and np.any(tab[:, named] < 0) and np.any(tab[:, named] > 0)
    assert seen_dead


def test_plain_fp64_restatement_holds_the_three_bounds():
    """gamma(4) M at bilinear steps, gamma(2) M at T-only steps, gamma(7) of the combine's yardstick."""
    worst = np.zeros(3)
    for n_pts, n_pt, n_steps in _cases():
        worst = np.maximum(worst, _shares(LR.case(n_pts, n_pt, n_steps, combine_inputs=True)))
    print("plain fp64: %.3f of gamma(4) M (bilinear), %.3f of gamma(2) M (T only), %.3f of gamma(7) Y (combine)" % tuple(worst))
    assert np.all(worst <= 1.0) and np.all(worst > 0.0)


@pytest.mark.parametrize("defect", LR.DEFECTS)
def test_seeded_defect_exceeds_the_bound(defect):
    """Each defect exceeds a bound by a factor of 1e3 or more at some point, on the cases the GPU tests run (the
    interpolated set for the first three, the combine for all six), and the cases that catch it are printed."""
    caught = []
    for n_pts, n_pt, n_steps in _cases():
        s = _shares(LR.case(n_pts, n_pt, n_steps, combine_inputs=True), defect)
        interp, comb = max(s[0], s[1]), s[2]
        if comb >= 1e3 and (interp >= 1e3 or defect not in LR.INTERP_DEFECTS):
            caught.append((n_pts, n_pt, n_steps))
        if defect not in LR.INTERP_DEFECTS:
            assert interp <= 1.0          # (a defect of the combine leaves the interpolated set alone)
    print("%s: caught (share >= 1e3) in %d of %d cases, e.g. (n_pts, n_pt, n_steps) = %s" % (defect, len(caught), len(_cases()), caught[:3]))
    assert (257, 40, 70) in caught and (257, 6, 3) in caught, caught


# ----------------------------------------------------------------------------------------------------------------------
# refusals of sr_lut_interp_dev
# ----------------------------------------------------------------------------------------------------------------------
FAKE = C.c_void_p(4096)     # stands for a device buffer: never dereferenced by a refused call
N_PT, N_PTS = 6, 10
_GOOD_IDX = [[0, 1, 2, 3], [4, 5, -1, -1], [5, 5, 0, 0]]
_GOOD_W = [[0.25, 0.75, 1.5, -0.5], [0.0, 0.0, 0.5, 0.5], [1.0, 0.0, 0.0, 1.0]]


def _call(idx=_GOOD_IDX, w=_GOOD_W, combine=0, pop=True, out_e=True):
    from spectrobot_amd import _lib
    idx = np.ascontiguousarray(idx, np.int32)
    w = np.ascontiguousarray(w, np.float64)
    p = np.ones(idx.shape[0])
    return _lib.lib.sr_lut_interp_dev(FAKE, N_PT, N_PTS, idx.shape[0], idx.ctypes.data_as(_lib.ip), w.ctypes.data_as(_lib.dp),
                                      p.ctypes.data_as(_lib.dp) if pop else None, combine, FAKE, FAKE if out_e else None, None)


def _with(a, s, i, v):
    a = [list(r) for r in a]
    a[s][i] = v
    return a


_REFUSED = [("row == n_pt", dict(idx=_with(_GOOD_IDX, 0, 1, N_PT))),
            ("row == n_pt in the last slot of the last step", dict(idx=_with(_GOOD_IDX, 2, 3, N_PT))),
            ("row > n_pt in a T-only step", dict(idx=_with(_GOOD_IDX, 1, 0, N_PT + 7))),
            ("negative first row", dict(idx=_with(_GOOD_IDX, 0, 0, -1))),
            ("negative second row of a bilinear step", dict(idx=_with(_GOOD_IDX, 2, 1, -1))),
            ("negative fourth row of a bilinear step", dict(idx=_with(_GOOD_IDX, 0, 3, -1))),
            ("i3 < 0 with i4 >= 0", dict(idx=_with(_GOOD_IDX, 1, 3, 2))),
            ("combine without pop", dict(combine=1, pop=False)),
            ("combine without out_e", dict(combine=1, out_e=False))]
_REFUSED += [("%s weight in slot %d of step %d%s" % (name, i, s, ", combine" if comb else ""), dict(w=_with(_GOOD_W, s, i, v), combine=comb))
             for name, v in (("NaN", np.nan), ("+inf", np.inf), ("-inf", -np.inf)) for s in range(3) for i in range(4) for comb in (0, 1)]


@pytest.mark.parametrize("what,kw", _REFUSED, ids=[r[0] for r in _REFUSED])
def test_lut_interp_refusals(what, kw):
    """SR_ERR_ARG from the argument checks, before anything is staged: the table and the outputs are placeholders that a
    call which got as far as a copy or a launch could not use.  A weight that is not finite is refused in every slot of
    every step, the pressure slots of a T-only step included (the planner's division by T2 - T1 == 0 gave (-inf, inf))."""
    from spectrobot_amd import _lib
    assert _call(**kw) == _lib.SR_ERR_ARG
