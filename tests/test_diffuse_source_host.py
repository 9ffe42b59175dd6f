"""The two-stream diffuse source (engine.diffuse_source, geometry.vertical_columns, retrieval.Sun(multiple=),
sr_diffuse_source_rows_dev) checked on the host, no GPU: the ABI surface, the reference's two statements against each
other, the fp64 restatement of the kernel's formulas against the reference, exact zeros, conservation, empty layers, the
vertical columns against slant_los, the sun's key and the refusals of the host layers."""
import os
import re

import numpy as np
import pytest

import columns_reference as CR
import diffuse_source_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LD = np.longdouble


def test_abi_surface():
    from spectrobot_amd import _lib
    header = open(os.path.join(ROOT, "include", "spectrobot_hip.h")).read()
    assert re.search(r"^int sr_diffuse_source_rows_dev\(const sr_diffuse_desc \*desc,", header, re.M)
    assert re.search(r"\} sr_diffuse_desc;", header)
    assert "sr_diffuse_source_rows_dev" in _lib.SYMBOLS and hasattr(_lib.lib, "sr_diffuse_source_rows_dev")
    names = [n for n, _ in _lib.DiffuseDesc._fields_]
    assert names == ["n_gas", "n_layers", "v", "ssa", "asym", "mu0", "surface_albedo"]
    assert _lib.lib.sr_abi_version() == 1


def test_adding_form_against_the_interface_system():
    """`reference` (closed-form layer operators, added) against `reference_bvp` (the 2N x 2N system in the exponential
    basis), both in long double, on columns with co >= 1e-3.  Units: b at long double's precision, b 2^-11, times the
    basis form's own conditioning: 1 / co for its particular solution (divided by k^2 ~ co), and 1 / min(k dtau', 1) for
    its two exponentials, which become linearly dependent in a thin layer.  Gaussian elimination is stable in the norm
    of the column's solution, not interface by interface, so |ref| of b is the column's largest value of that output
    (the fluxes fall by up to e^-30 along a column)."""
    rng = np.random.default_rng(20261021)
    worst = 0.0
    for case in range(40):
        n_layers = (1, 2, 3, 7, 17)[case % 5]
        c = R.bvp_case(rng, n_layers, empty=0.2 if case % 4 == 3 else 0.0)
        co, dt = R.min_co(*R.args(c)[:4]), R.min_dtau(*R.args(c)[:4])
        if not np.isfinite(dt):
            continue
        assert co >= 1e-3
        ref, bvp = R.reference(*R.args(c)), R.reference_bvp(*R.args(c))
        k_dtau = np.sqrt(3.0 * co) * dt
        allow = 2.0 ** -11 / (co * min(k_dtau, 1.0))
        for key in ("J", "flux", "emi"):
            top = np.max(np.abs(ref[key]).reshape(-1, ref[key].shape[-1]), axis=0)     # per point: the column's largest
            b = R.bound(np.broadcast_to(top, ref[key].shape), 2, n_layers) * LD(allow)
            assert np.all(b > 0)
            worst = max(worst, float(np.max(np.abs(bvp[key] - ref[key]) / b)))
    print("adding form against the interface system, in units of b 2^-11 / (co min(k dtau, 1)): %.3f" % worst)
    assert worst <= 1.0


def test_fp64_restatement_against_the_reference():
    """plain64 (the kernel's formulas in fp64) stays at <= 0.5 of b over the GPU panel and 300 random columns: what fixes
    C_LAYER."""
    worst = dict(emi=0.0, J=0.0, flux=0.0)
    cases = [R.panel_case(n, g, p) for n in R.N_LAYERS for g in R.N_GAS for p in R.N_PTS] + list(R.random_columns())
    seen_zero_co = seen_empty = False
    for c in cases:
        n_gas, n_layers = c["A"].shape[:2]
        seen_zero_co |= R.min_co(*R.args(c)[:4]) == 0.0
        seen_empty |= bool(np.any(c["V"].sum(axis=0) == 0.0))
        ref, p64 = R.reference(*R.args(c)), R.plain64(*R.args(c))
        for key in worst:
            assert np.all(ref[key] >= 0) and np.all(p64[key] >= 0), key
            worst[key] = max(worst[key], R.ratio(p64[key], ref[key], R.bound(ref[key], n_gas, n_layers)))
    assert seen_zero_co and seen_empty
    print("plain fp64 against the reference, in units of b (C_LAYER = %d): emi %.3f J %.3f flux %.3f"
          % (R.C_LAYER, worst["emi"], worst["J"], worst["flux"]))
    assert max(worst.values()) <= 0.5


def test_exact_zeros():
    c = R.panel_case(3, 3, 5)
    for fn in (R.reference, R.plain64):
        # no scatterer and nothing below that reflects: no diffuse light at all
        o = fn(c["A"], c["V"], np.zeros(3), c["asym"], c["beam"], c["sun"], c["mu0"], 0.0)
        assert all(np.all(o[k] == 0) for k in ("emi", "J", "flux"))
        # no scatterer above a reflecting ground: the ground's light, but no rows
        o = fn(c["A"], c["V"], np.zeros(3), c["asym"], c["beam"], c["sun"], 0.8, 0.5)
        assert np.all(o["emi"] == 0) and np.all(o["flux"][0] > 0)
        # no sunlight anywhere and a black ground
        o = fn(c["A"], c["V"], c["ssa"], c["asym"], np.zeros_like(c["beam"]), c["sun"], c["mu0"], 0.0)
        assert all(np.all(o[k] == 0) for k in ("emi", "J", "flux"))
        o = fn(c["A"], c["V"], c["ssa"], c["asym"], c["beam"], np.zeros_like(c["sun"]), c["mu0"], 0.7)
        assert all(np.all(o[k] == 0) for k in ("emi", "J", "flux"))


@pytest.mark.parametrize("n_layers", [1, 3, 17, 80])
def test_conservation(n_layers):
    """ssa = 1, no absorber, a black lower boundary: what leaves through the two boundaries is what the beam put in,
    F+_N + F-_0 = sum_l dtau'_l D_l, to b (the floor co >= 2^-52 absorbs less than that in these columns of optical depth
    below 2, in either precision: R.conservation_case)."""
    c = R.conservation_case(n_layers, 4)
    want = R.absorbed_input(c)
    for fn, slack in ((R.reference, 1.0), (R.plain64, 1.0)):
        F = fn(*R.args(c))["flux"]
        out = np.asarray(F[0, -1], LD) + np.asarray(F[1, 0], LD)
        assert np.all(np.abs(out - want) <= R.bound(want, 1, n_layers) * LD(slack)), fn.__name__


def test_an_empty_layer_changes_nothing_but_the_index():
    c = R.panel_case(3, 3, 5)
    c["V"][:, :] = np.maximum(c["V"], 1e-3)
    ins = lambda a, axis: np.insert(a, 1, 0.0, axis=axis)
    A2 = np.insert(c["A"], 1, 0.7, axis=1)
    V2 = ins(c["V"], 1)
    beam2 = np.insert(c["beam"], 1, 0.5 * (c["beam"][0] + c["beam"][1]), axis=0)
    for fn in (R.reference, R.plain64):
        a = fn(*R.args(c))
        b = fn(A2, V2, c["ssa"], c["asym"], beam2, c["sun"], c["mu0"], c["albedo"])
        assert np.all(np.delete(b["flux"], 1, axis=1) == a["flux"]) and np.all(b["flux"][:, 1] == b["flux"][:, 2])
        assert np.all(np.delete(b["emi"], 1, axis=0) == a["emi"])
        assert np.all(np.delete(b["J"], 1, axis=0) == a["J"])


def _plain_columns(L, col_scale):
    col, _ = CR.columns(2, L["x"], L["nd"], L["vmr"], pt_off=L["pt_off"], dtype=np.float64, scale=col_scale)
    return np.asarray(col, float)


def test_vertical_columns_equal_slant_los_at_zenith():
    """Layer by layer, with the tolerance of the solar geometry's own test: 64 eps of the column sum per gas."""
    from spectrobot_amd import geometry as G
    z = np.linspace(100.0, 690.0, 60) + np.where(np.arange(60) % 2, 1.5, 0.0)
    nd = 3e17 * np.exp(-(z - 100.0) / 63.0)
    vmr = np.array([0.0148 * (1.0 + (z - 100.0) / 900.0), 4e-5 * np.exp(-(z - 100.0) / 300.0), np.full(z.size, 1.0)])
    cs = np.array([0.98827, 1.0, 0.5])
    V = G._vertical_columns(z, nd, vmr, G.TITAN_RADIUS_KM, 3, cs, _plain_columns)
    S = G.slant_los(z, nd, vmr, [0.0])
    col = _plain_columns(S, cs)
    want = np.zeros((3, z.size))
    for g in range(3):
        np.add.at(want[g], S["seg_layer"][S["seg_off"][0]:S["seg_off"][1]], col[g, S["seg_off"][0]:S["seg_off"][1]])
    assert V.shape == (3, z.size) and np.all(V > 0)
    tol = 64 * 2.0 ** -53 * want.sum(axis=1, keepdims=True)
    assert np.all(np.abs(V - want) <= tol), float(np.max(np.abs(V - want) / tol))


def test_sun_key_and_value_errors():
    from spectrobot_amd import retrieval as rt
    irr = np.ones(8)
    plain = rt.Sun(60.0, 30.0, irr)
    assert len(plain.key()) == 3 and plain.multiple is False
    assert rt.Sun(60.0, 30.0, irr, multiple=False, surface_albedo=0.3).key() == plain.key()
    multi = rt.Sun(60.0, 30.0, irr, multiple=True, surface_albedo=0.3)
    assert multi.key()[:3] == plain.key() and multi.key()[3:] == (True, 0.3)
    assert rt.Sun(60.0, 30.0, irr, multiple=True).key() != multi.key()
    for bad in (-0.1, 1.1, float("nan")):
        with pytest.raises(ValueError):
            rt.Sun(60.0, 30.0, irr, multiple=True, surface_albedo=bad)
    grid = 2950.0 + 0.01 * np.arange(8)
    z = np.linspace(100.0, 400.0, 4)
    back = rt.TableGas("haze", None, np.ones(4), solar=dict(albedo=0.9, g=-0.7))
    scene = lambda sun: rt.LimbScene(grid, z, np.full(4, 150.0), np.full(4, 1.0), [back], [3389.0], [5.0], sun=sun)
    scene(plain)                                    # single scattering takes any |g| < 1
    with pytest.raises(ValueError):
        scene(multi)


def test_engine_refusals_need_no_gpu():
    """The Python entry looks at its tensors first: host arrays are refused before any device call."""
    from spectrobot_amd import engine
    with pytest.raises(ValueError):
        engine.diffuse_source(np.ones((1, 2, 3)), np.ones((1, 2)), [0.5], [0.1], np.ones((3, 3)), np.ones(3), 0.5, out_gas=0)
