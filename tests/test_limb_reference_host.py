"""The extended-precision reference of the limb recursion (tests/limb_reference.py) checked on the host: long double
against 60-digit arithmetic, the plain-fp64 yardstick K_PLAIN recorded and respected, four seeded defects each far
over the kernels' limit, the cost of the thin rule -- and the ceiling of the far field's truncation bound that
conftest.far_tol takes its tolerances from.  No GPU."""
import numpy as np
import pytest

import limb_reference as R

SEED, N_SEG, N_GAS, N_PAR = 20261017, 41, 2, 3     # the shapes K_PLAIN_* were recorded at


@pytest.fixture(scope="module")
def problem():
    pan = R.panel_problem(N_SEG, N_GAS, N_PAR, SEED)
    args = (pan["coef_a"], pan["coef_e"], pan["col"], pan["par_gas"], pan["dcol"])
    pan["ld"] = R.forms(*args, R.LD)
    pan["f64"] = R.forms(*args, np.float64)
    pan["ref"] = R.recursion_reference(*pan["ld"], pan["I0"], thin_ulps=N_GAS + 1)
    return pan


def _plain_units(pan, defect=None):
    ref = pan["ref"]
    I, J = R.plain_fp64(*pan["f64"], pan["I0"], defect=defect)
    return (R.units(I, ref["I"], ref["A_I"], ref["C_I"], N_GAS), R.units(J, ref["J"], ref["A"], ref["C"], N_GAS))


def test_long_double_against_60_digits(problem):
    """Every third panel column in mpmath at 60 digits, thin_rule=False on both sides, the fp64 forms of tau, E, dtau,
    dE taken as exact: the long-double reference, rounded to double, is within 2 units of A alone (C left out)."""
    from mpmath import mp          # (sympy, which torch needs, brings it)
    mp.dps = 60
    tau, E, dtau, dE = problem["f64"]
    cols = np.arange(0, tau.shape[1], 3)
    ref = R.recursion_reference(tau[:, cols], E[:, cols], dtau[:, :, cols], dE[:, :, cols], problem["I0"][cols],
                                thin_rule=False, want_cond=False)
    I_mp = np.zeros(cols.size)
    J_mp = np.zeros((N_PAR, cols.size))
    for k, j in enumerate(cols):
        I = mp.mpf(float(problem["I0"][j]))
        J = [mp.mpf(0)] * N_PAR
        for s in range(N_SEG):
            x, e = mp.mpf(float(tau[s, j])), mp.mpf(float(E[s, j]))
            t = mp.exp(-x)
            if x == 0:
                f, fp = mp.mpf(1), mp.mpf(-1) / 2
            else:
                f = -mp.expm1(-x) / x
                # (tau t - (1 - t)) / tau^2 cancels ~ 2 log10(1/tau) digits: evaluated with that many digits to spare
                with mp.workdps(60 + 2 * max(0, int(-mp.log10(abs(x)))) + 10):
                    fp = (x * mp.exp(-x) + mp.expm1(-x)) / (x * x)
            for p in range(N_PAR):
                dt, de = mp.mpf(float(dtau[p, s, j])), mp.mpf(float(dE[p, s, j]))
                J[p] = J[p] * t + (-I * t * dt + de * f + e * fp * dt)
            I = I * t + e * f
        I_mp[k] = float(I)
        J_mp[:, k] = [float(v) for v in J]
    uI = R.units(np.asarray(ref["I"], np.float64), I_mp, ref["A_I"], 0.0, N_GAS)
    uJ = R.units(np.asarray(ref["J"], np.float64), J_mp, ref["A"], 0.0, N_GAS)
    names = problem["names"]
    print("long double vs 60 digits: rad %.3g units at %s, jac %.3g units at %s"
          % (R.worst(uI, names, cols) + R.worst(uJ, names, cols)))
    assert uI.max() <= 2.0 and uJ.max() <= 2.0


def test_k_plain_recorded_and_respected(problem):
    uI, uJ = _plain_units(problem)
    ref = problem["ref"]
    I, J = R.plain_fp64(*problem["f64"], problem["I0"])
    no_c = R.units(J, ref["J"], ref["A"], 0.0, N_GAS).max()
    names = problem["names"]
    print("K_PLAIN live: rad %.3g at %s; jac %.3g at %s; jac with C left out %.3g"
          % (R.worst(uI, names) + R.worst(uJ, names) + (no_c,)))
    assert uI.max() <= R.K_PLAIN_RAD and uJ.max() <= R.K_PLAIN_JAC
    # the constants are a record, not a budget: at most 2 x what was measured when they were written
    assert R.K_PLAIN_RAD <= 2.0 * R.K_PLAIN_RAD_MEASURED and R.K_PLAIN_JAC <= 2.0 * R.K_PLAIN_JAC_MEASURED


@pytest.mark.parametrize("defect", R.DEFECTS)
def test_seeded_defects_are_far_over_the_limit(problem, defect):
    """The teeth of the bound: each defect alone puts plain_fp64 at least 10 x over the kernels' limit 8 x K_PLAIN."""
    uI0, uJ0 = _plain_units(problem)
    limit = R.KERNEL_MARGIN * max(uI0.max(), uJ0.max())
    uI, uJ = _plain_units(problem, defect)
    names = problem["names"]
    print("%s: rad %.3g units at %s; jac %.3g units at %s; limit %.3g" % ((defect,) + R.worst(uI, names) + R.worst(uJ, names) + (limit,)))
    assert max(uI.max(), uJ.max()) >= 10.0 * limit


def test_thin_rule_cost_is_reported(problem):
    """The distance between the build's definition (f = 1, f' = -1/2 where |tau| <= 1e-12) and the limit-free
    functions: reported, not asserted beyond its derivation (f = 1 - tau/2 + ...: at most 5e-13 of each term)."""
    a = problem["ref"]
    b = R.recursion_reference(*problem["ld"], problem["I0"], thin_rule=False, want_cond=False)
    with np.errstate(all="ignore"):
        dI = np.asarray(np.abs(a["I"] - b["I"]) / np.maximum(a["A_I"], R.LD(R.FLOOR)), np.float64)
        dJ = np.asarray(np.abs(a["J"] - b["J"]) / np.maximum(a["A"], R.LD(R.FLOOR)), np.float64)
    names = problem["names"]
    print("thin rule against the limit-free functions: rad %.3g of A_I at %s; jac %.3g of A at %s"
          % (R.worst(dI, names) + R.worst(dJ, names)))
    assert dI.max() <= 5.1e-13 and dJ.max() <= 5.1e-13


def test_reference_limits():
    """Closed forms of one segment: a saturated segment returns E / tau, an exactly empty one E, and J of a lone thin
    segment is dE - I0 dtau - E dtau / 2."""
    tau = np.array([[1e6, 0.0, 1e-13]])
    E = np.array([[3.0, 2.0, 4.0]])
    dtau = np.array([[[0.0, 0.5, 0.25]]])
    dE = np.array([[[0.0, 7.0, 1.0]]])
    r = R.recursion_reference(tau, E, dtau, dE, np.array([5.0, 1.0, 2.0]))
    assert float(abs(r["I"][0] - R.LD(3) / R.LD(10) ** 6)) < 1e-24 and float(r["I"][1]) == 3.0
    assert float(r["J"][0, 1]) == 7.0 - 1.0 * 0.5 - 2.0 * 0.5 * 0.5
    assert abs(float(r["J"][0, 2]) - (1.0 - 2.0 * 0.25 - 4.0 * 0.5 * 0.25)) < 1e-12


def test_far_field_truncation_bound_has_a_ceiling():
    """conftest.far_tol widens seventeen assertions to this bound: a build with a larger one must not loosen them
    silently.  18 theta^-(degree + 1) at theta 4, degree 19 (include/spectrobot_hip.h)."""
    from spectrobot_amd import engine
    b = engine.far_field_truncation_bound()
    assert 0.0 < b <= 18 * 4.0 ** -20 * (1 + 1e-12)
