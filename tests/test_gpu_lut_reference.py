"""The look-up-table route (sr_lut_interp_dev: sr_lut_kernel<false | true>; LutSet.calculate_steps / combine_steps;
retrieval.lut_coefficients) held POINTWISE to tests/lut_reference.py: the long-double interpolation of the fp64 table
with the fp64 weights, and the sum M of the absolute addends at that point.

Limits (derived in the reference module's docstring from the kernel's operations, none measured here):
    interpolated set   gamma(4) M at bilinear steps, gamma(2) M at T-only steps
    combine            gamma(7) (|abs0| + |pop| (M_abs + M_ind)) and gamma(7) (|emi0| + |pop| M_sp)
    lut_coefficients   gamma(7) of the combine's yardstick summed over the gas's levels

(A) synthetic tables through engine.lut_interp, (B) the combining instance, two calls into the same outputs, (C) a real
table of gcoeff_levels through LutSet.calculate_steps / combine_steps, bit for bit at the tabulated couples, (D)
retrieval.lut_coefficients on a small scene whose layer temperatures include exact midpoints of the lattice, (E) refused
calls leave the outputs untouched.  A, B, C and D print the worst share of the limit they saw.

Measured on an MI355X, 2026-10-21, worst share of the limit:

    n_pts                        1       255     256     257     1031
    A, n_pt 2                    0.552   0.986   0.910   0.935   0.982
    A, n_pt 6                    0.722   0.930   0.963   0.955   0.978
    A, n_pt 40                   0.764   0.954   0.968   0.964   0.963
    B, n_pt 2                    0.324   0.482   0.545   0.510   0.566
    B, n_pt 6                    0.372   0.514   0.556   0.550   0.619
    B, n_pt 40                   0.277   0.610   0.572   0.560   0.561

    C  calculate_steps 0.919, combine_steps 0.490 (12 levels x 17 queries)
    D  0.960 (temp_step 5 K, layers at multiples of 2.5 K), 0.980 (2.5 K, 1.25 K); the table route differs from
       scene.coefficients() by 5.9e-2 and 2.8e-2 of a layer's largest value (the lattice's interpolation error)

The six seeded defects of tests/test_lut_reference_host.py compiled into sr_lut_kernel (never committed): wP1 <-> wP2, rows
i2 <-> i3 and pressure weights in the T-only form fail all 15 cases of A and all 15 of B; G_ind added, emission from the
wrong plane and the population of step s + 1 fail all 15 cases of B.
"""
import numpy as np
import pytest

import lut_reference as LR

pytestmark = pytest.mark.gpu

LD = LR.LD


@pytest.fixture(scope="module")
def eng():
    import torch
    assert torch.cuda.is_available(), "these tests need the GPU"
    from spectrobot_amd import engine
    engine.set_device(0)
    return engine


def _dev(a):
    import torch
    return torch.as_tensor(np.ascontiguousarray(a), device="cuda")


# ----------------------------------------------------------------------------------------------------------------------
# (A) the interpolated set on synthetic tables
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_pt", LR.N_PT)
@pytest.mark.parametrize("n_pts", LR.N_PTS)
def test_interp_synthetic(eng, n_pts, n_pt):
    """engine.lut_interp against lut_reference.interpolate at every point: entries of random sign over 60 decades,
    bilinear and T-only steps in one call, repeated rows, weights outside [0, 1], NaN in every row that no step names (a
    wrong row index shows as a NaN, which share() refuses)."""
    worst = 0.0
    for n_steps in LR.N_STEPS:
        c = LR.case(n_pts, n_pt, n_steps)
        got = eng.lut_interp(_dev(c["tab"]), c["idx4"], c["wgt4"]).cpu().numpy()
        assert got.shape == (3, n_steps, n_pts)
        val, M = LR.interpolate(c["tab"], c["idx4"], c["wgt4"])
        worst = max(worst, LR.share(got, val, LR.limit_interp(M, c["idx4"])))
    print("lut_interp, n_pts %d, n_pt %d: %.3f of gamma(4) M | gamma(2) M" % (n_pts, n_pt, worst))
    assert worst <= 1.0


# ----------------------------------------------------------------------------------------------------------------------
# (B) the combining instance
# ----------------------------------------------------------------------------------------------------------------------
def _combine_share(got, c, abs0, emi0):
    (wa, we), (Ya, Ye) = LR.combine(c["tab"], c["idx4"], c["wgt4"], c["pop"], abs0, emi0)
    return max(LR.share(got[0], wa, LR.limit_combine(Ya)), LR.share(got[1], we, LR.limit_combine(Ye)))


@pytest.mark.parametrize("n_pt", LR.N_PT)
@pytest.mark.parametrize("n_pts", LR.N_PTS)
def test_combine_synthetic(eng, n_pts, n_pt):
    """sr_lut_kernel<true> against lut_reference.combine: outputs pre-filled with random values of either sign, populations
    that include 0.0 and 1e-250, and a second call (another table, other rows, weights and populations) into the same
    outputs as the next level makes it -- held to the reference started from the first call's fp64 result."""
    worst = 0.0
    for n_steps in LR.N_STEPS:
        c1 = LR.case(n_pts, n_pt, n_steps, combine_inputs=True)
        c2 = LR.case(n_pts, n_pt, n_steps, seed=1, combine_inputs=True)
        ab, em = _dev(c1["abs0"]), _dev(c1["emi0"])
        assert np.all(c1["abs0"] != 0.0) and np.all(c1["emi0"] != 0.0)
        eng.lut_interp(_dev(c1["tab"]), c1["idx4"], c1["wgt4"], pops=c1["pop"], out=(ab, em))
        first = (ab.cpu().numpy(), em.cpu().numpy())
        worst = max(worst, _combine_share(first, c1, c1["abs0"], c1["emi0"]))
        eng.lut_interp(_dev(c2["tab"]), c2["idx4"], c2["wgt4"], pops=c2["pop"], out=(ab, em))
        worst = max(worst, _combine_share((ab.cpu().numpy(), em.cpu().numpy()), c2, first[0], first[1]))
        if n_steps >= 2:       # a population of 0.0 leaves its step as it was, bit for bit
            s = n_steps - 1
            assert c1["pop"][s] == 0.0 and np.array_equal(first[0][s], c1["abs0"][s]) and np.array_equal(first[1][s], c1["emi0"][s])
    print("lut combine, n_pts %d, n_pt %d: %.3f of gamma(7) Y" % (n_pts, n_pt, worst))
    assert worst <= 1.0


# ----------------------------------------------------------------------------------------------------------------------
# (C) a real table
# ----------------------------------------------------------------------------------------------------------------------
C_PS, C_TS = (0.01, 0.1, 1.0), (140.0, 150.0, 160.0, 170.0)


@pytest.fixture(scope="module")
def real_table(eng):
    """gcoeff_levels of 300 CH4-like lines (12 levels) on 3000 points at the 3 x 4 lattice C_PS x C_TS, one LutSet per
    level filled by _append; the tables on the host, left unchanged."""
    from spectrobot_amd import spect_main_module as smm, synthetic as syn
    grid = syn.make_grid(2975.0, 5e-4, 3000)
    ls = eng.LineSet(syn.make_lines(300, grid, seed=9, n_levels=12), grid, 6, 1, syn.CH4_MM, syn.CH4_LEVEL_ENERGIES)
    PT = [[P, T] for P in C_PS for T in C_TS]
    g_all = ls.gcoeff_levels([pt[1] for pt in PT], [pt[0] for pt in PT])
    luts = []
    for lev in range(12):
        lut = smm.LutSet(ls.mol, ls.iso, ls.mm, level=None, level_index=lev)
        lut._append(g_all[lev], PT)
        luts.append(lut)
    host = g_all.cpu().numpy()
    host.setflags(write=False)
    assert host.shape == (12, 3, 12, 3000) and np.all(np.isfinite(host)) and np.count_nonzero(host) > host.size // 2
    return luts, host, PT


def _real_queries():
    rng = np.random.default_rng(20261021)
    P = [0.03, 0.055, 0.5, 0.55, 1.0, 0.1, 0.004, 0.01, 0.010000000000000002, 0.07, 0.3]
    T = [145.0, 155.0, 165.0, 147.3, 168.9, 152.5, 155.0, 141.0, 150.0, 133.0, 176.5]
    return np.array(P + list(rng.uniform(0.005, 1.0, 6))), np.array(T + list(rng.uniform(138.0, 172.0, 6)))


def test_real_table_interpolation_and_combine(eng, real_table):
    """LutSet.calculate_steps and combine_steps of every level against the reference's planner + interpolation applied to
    the table copied to the host: midpoints in T and in P, points between the nodes, below the lowest pressure (T only),
    temperatures outside the lattice."""
    luts, host, PT = real_table
    Pq, Tq = _real_queries()
    idx, w = LR.plan_steps(PT, Pq, Tq)
    bil = LR.bilinear_steps(idx)
    assert bil.any() and (~bil).any() and np.any(w == 0.5) and np.any(w < 0.0)
    rng = np.random.default_rng(5)
    worst = [0.0, 0.0]
    for lev, lut in enumerate(luts):
        got = lut.calculate_steps(Pq, Tq).cpu().numpy()
        val, M = LR.interpolate(host[lev], idx, w)
        worst[0] = max(worst[0], LR.share(got, val, LR.limit_interp(M, idx)))
        pop = 10.0 ** rng.uniform(-6.0, 0.0, Pq.size)
        abs0, emi0 = (rng.choice([-1.0, 1.0], got[0].shape) * np.abs(got[k]).max() * rng.uniform(0.0, 1e-3, got[0].shape) for k in (2, 0))
        ab, em = _dev(abs0), _dev(emi0)
        lut.combine_steps(Pq, Tq, pop, ab, em)
        (wa, we), (Ya, Ye) = LR.combine(host[lev], idx, w, pop, abs0, emi0)
        worst[1] = max(worst[1], LR.share(ab.cpu().numpy(), wa, LR.limit_combine(Ya)), LR.share(em.cpu().numpy(), we, LR.limit_combine(Ye)))
    print("real table, 12 levels x %d queries: calculate_steps %.3f of gamma(4) M | gamma(2) M, combine_steps %.3f of gamma(7) Y"
          % (Pq.size, worst[0], worst[1]))
    assert worst[0] <= 1.0 and worst[1] <= 1.0


def test_real_table_rows_at_the_tabulated_couples(eng, real_table):
    """At a tabulated couple the weights are exactly 1 and 0 and the interpolated set is the table's row, bit for bit --
    at the lowest pressure through the T-only form, above it through the bilinear one."""
    luts, host, PT = real_table
    Pq, Tq = np.array([pt[0] for pt in PT]), np.array([pt[1] for pt in PT])
    for lev in (0, 1, 7, 11):
        got = luts[lev].calculate_steps(Pq, Tq).cpu().numpy()
        assert np.array_equal(got, host[lev]), lev


# ----------------------------------------------------------------------------------------------------------------------
# (D) retrieval.lut_coefficients
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("temp_step,quantum", [(5.0, 2.5), (2.5, 1.25)])
def test_lut_coefficients_on_a_scene_with_midpoint_temperatures(eng, temp_step, quantum):
    """retrieval.lut_coefficients on bench_configs.two_gas_scene at its smallest working size (the bands need a window of
    2.4 nm: 6000 points), the layer temperatures rounded to multiples of `quantum` so that some lie exactly halfway between
    two nodes of the lattice of `temp_step` and some on a node.  Every output is finite and equals, within gamma(7) of the
    combine's yardstick summed over the levels, the reference's planner + combine applied to the scene's own tables with
    the populations restated here.

    Before the planner's second node was taken from the REMAINING nodes this case returned NaN: at a midpoint the
    unstable argsort named the nearest temperature twice, the weights came out as (-inf, inf), and the layer's spectra
    were NaN with no error raised.

    The limit is not a worst-case count for a gas of L levels: the outputs are updated twice per level, so an addend of
    level l passes up to 5 + 2 (L - l) roundings (28 for the ground state of 12 levels, which carries nearly all of Y).  It
    holds because rounding errors do not line up -- measured 0.960 (5 K) and 0.980 (2.5 K) of it, 34 of 42 000 points above
    0.8, the tables and the outputs the same bit for bit from run to run.

    Printed, not asserted: the largest difference between the table route and scene.coefficients(), per layer relative to
    the layer's largest value -- the interpolation error of the lattice, a property of the table and not of the code."""
    import torch
    import bench_configs as bc
    from spectrobot_amd import retrieval, spect_classes as spcl, synthetic as syn
    scene = bc.two_gas_scene(600, 150, 6000, 7)
    temps = quantum * np.round(scene.temps / quantum)
    scene.temps, scene.nd = temps, syn.number_density(scene.press, temps)
    frac = np.mod(temps, temp_step)
    assert np.sum(frac == 0.5 * temp_step) >= 2 and np.sum(frac == 0.0) >= 1, temps
    out = retrieval.lut_coefficients(scene, temp_step=temp_step, pres_step_log=1.0)
    direct = scene.coefficients()
    worst, interp_err = 0.0, 0.0
    for g, (ab, em), (ab_d, em_d) in zip(scene.gases, out, direct):
        ls = g.lineset
        PT = g.luts[0].PTcouples
        idx, w = LR.plan_steps(PT, scene.press, temps)
        assert np.any(w[:, 2:] == 0.5) and np.all(np.isfinite(w))
        rows = np.unique(idx[idx >= 0])                       # (only the rows in use travel to the host)
        local = np.where(idx >= 0, np.searchsorted(rows, idx), -1).astype(np.int32)
        q = np.atleast_1d(spcl.CalcPartitionSum(ls.mol, ls.iso, temps))
        n_lev = ls.level_energies.size
        assert len(g.luts) == max(n_lev, 1) and all(lut.PTcouples == PT for lut in g.luts)
        want = [np.zeros((temps.size, ls.n_grid), LD) for _ in range(2)]
        Y = [np.zeros((temps.size, ls.n_grid), LD) for _ in range(2)]
        for lev, lut in enumerate(g.luts):
            tab = lut.device[:, torch.as_tensor(rows, device="cuda")].cpu().numpy()
            tv = temps if g.tvib is None else np.asarray(g.tvib)[lev]
            pop = np.exp(-spcl.c2 * ls.level_energies[lev] / tv) / q if n_lev else 1.0 / q
            (a_l, e_l), (Ya_l, Ye_l) = LR.combine(tab, local, w, pop, 0.0 * Y[0], 0.0 * Y[1])
            want[0] += a_l
            want[1] += e_l
            Y[0] += Ya_l
            Y[1] += Ye_l
        for k, (got, ref) in enumerate(((ab, ab_d), (em, em_d))):
            got, ref = got.cpu().numpy(), ref.cpu().numpy()
            assert np.all(np.isfinite(got)), (g.name, k, np.argwhere(~np.isfinite(got))[:3])
            worst = max(worst, LR.share(got, want[k], LR.limit_combine(Y[k])))
            interp_err = max(interp_err, float(np.max(np.abs(got - ref).max(axis=1) / np.abs(ref).max(axis=1))))
    print("lut_coefficients, temp_step %.2f K, layers at multiples of %.2f K: %.3f of gamma(7) sum_levels Y; the table route differs "
          "from scene.coefficients() by %.2e of a layer's largest value (the lattice's interpolation error)" % (temp_step, quantum, worst, interp_err))
    assert worst <= 1.0


# ----------------------------------------------------------------------------------------------------------------------
# (E) refusals leave the outputs untouched
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("what", ["row == n_pt", "negative row", "NaN weight", "infinite weight in a T-only step's pressure slot"])
def test_refused_calls_write_nothing(eng, what):
    import ctypes as C
    import torch
    from spectrobot_amd import _lib
    n_pts, n_pt, n_steps = 257, 6, 3
    c = LR.case(n_pts, n_pt, n_steps, combine_inputs=True)
    idx, w = c["idx4"].copy(), c["wgt4"].copy()
    t_only = int(np.flatnonzero(~LR.bilinear_steps(idx))[0])
    if what == "row == n_pt":
        idx[n_steps - 1, 1] = n_pt
    elif what == "negative row":
        idx[0, 0] = -1
    elif what == "NaN weight":
        w[n_steps - 1, 3] = np.nan
    else:
        w[t_only, 0] = np.inf
    tab = _dev(np.nan_to_num(c["tab"]))
    sentinel = -7.25
    ab, em = (torch.full((n_steps, n_pts), sentinel, dtype=torch.float64, device="cuda") for _ in range(2))
    with pytest.raises(_lib.SpectRobotHipError) as e:
        eng.lut_interp(tab, idx, w, pops=c["pop"], out=(ab, em))
    assert e.value.status == _lib.SR_ERR_ARG
    g = torch.full((3, n_steps, n_pts), sentinel, dtype=torch.float64, device="cuda")
    rc = _lib.lib.sr_lut_interp_dev(C.c_void_p(tab.data_ptr()), n_pt, n_pts, n_steps, idx.ctypes.data_as(_lib.ip), w.ctypes.data_as(_lib.dp),
                                    None, 0, C.c_void_p(g.data_ptr()), None, None)
    assert rc == _lib.SR_ERR_ARG
    torch.cuda.synchronize()
    assert bool((ab == sentinel).all()) and bool((em == sentinel).all()) and bool((g == sentinel).all())
