"""The diffuse field for several columns of illumination (engine.diffuse_source_columns, geometry.sza_columns,
sr_diffuse_source_columns_dev) checked on the host, no GPU: the ABI surface, the fp64 restatement of the kernel's formulas
against the extended-precision reference, the interpolation weights, exact zeros of the reference pair and the refusals of
the Python entry."""
import os
import re

import numpy as np
import pytest

import diffuse_columns_reference as DC
import diffuse_source_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LD = np.longdouble


def test_abi_surface():
    from spectrobot_amd import _lib
    header = open(os.path.join(ROOT, "include", "spectrobot_hip.h")).read()
    assert re.search(r"^int sr_diffuse_source_columns_dev\(const sr_diffuse_desc \*desc, const sr_diffuse_columns_desc \*cols,", header, re.M)
    assert re.search(r"\} sr_diffuse_columns_desc;", header)
    assert re.search(r"^#define SR_MAX_DIFFUSE_COLUMNS 8$", header, re.M) and _lib.SR_MAX_DIFFUSE_COLUMNS == 8
    assert "sr_diffuse_source_columns_dev" in _lib.SYMBOLS and hasattr(_lib.lib, "sr_diffuse_source_columns_dev")
    names = [n for n, _ in _lib.DiffuseColumnsDesc._fields_]
    assert names == ["n_col", "n_rows", "mu0", "col_w", "row_layer", "src_row"]
    assert _lib.lib.sr_abi_version() == 1


@pytest.mark.parametrize("C", [1, 3, 8])
def test_fp64_restatement_against_the_reference(C):
    """plain64_columns (the kernel's formulas as built, the sources factored) stays at <= 0.5 of b over the GPU panel and
    the 300 random columns, for J, the fluxes and the rows."""
    worst = dict(J=0.0, flux=0.0, rows=0.0)
    rng = np.random.default_rng([20261021, C])
    for c in DC.host_cases():
        n_gas, n_layers = c["A"].shape[:2]
        mu0s, beams = DC.columns_of(c, C)
        w, layer, _ = DC.rows_of(rng, n_layers, C)
        ref = DC.reference(c, mu0s, beams, w, layer)
        p64 = DC.plain64_columns(c, mu0s, beams, w, layer)
        b = DC.bounds(ref, n_gas, n_layers, C)
        for key in worst:
            assert np.all(ref[key] >= 0) and np.all(p64[key] >= 0), key
            worst[key] = max(worst[key], R.ratio(p64[key], ref[key], b[key]))
    print("plain fp64 columns against the reference, C = %d, in units of b: J %.3f flux %.3f rows %.3f"
          % (C, worst["J"], worst["flux"], worst["rows"]))
    assert max(worst.values()) <= 0.5


def test_one_column_is_the_single_source():
    """With one column the reference is diffuse_source_reference's own, and the rows with row_layer = arange its emi."""
    c = R.panel_case(17, 3, 5)
    mu0s, beams = DC.columns_of(c, 1)
    ref = DC.reference(c, mu0s, beams, np.ones((17, 1)), np.arange(17))
    one = R.reference(*R.args(c))
    assert np.array_equal(ref["J"][0], one["J"]) and np.array_equal(ref["flux"][0], one["flux"])
    assert np.array_equal(ref["rows"], one["emi"])


def test_sza_columns():
    from spectrobot_amd import geometry as G
    rng = np.random.default_rng(20261021)
    eps = 2.0 ** -52
    for n_col in (2, 3, 4, 8):
        mu = rng.uniform(-0.3, 0.9, 200)
        nodes, w = G.sza_columns(mu, n_col)
        assert nodes.shape == (n_col,) and w.shape == (200, n_col)
        assert nodes[0] == mu.min() and nodes[-1] == mu.max() and np.all(np.diff(nodes) > 0)
        assert np.all(w >= 0) and np.all(np.abs(w.sum(axis=1) - 1.0) <= eps)       # (1 - f) + f: two roundings
        for row in w:
            nz = np.flatnonzero(row)
            assert 1 <= nz.size <= 2 and (nz.size == 1 or nz[1] == nz[0] + 1)
        # (1 - f) n_k + f n_k+1 with f = (mu - n_k) / h: the quotient, 1 - f, two products and the sum, half an ulp of
        # a number <= 1 each -- below 3 eps, asserted at 4
        assert np.all(np.abs(w @ nodes - mu) <= 4 * eps)
    # the ends and the nodes themselves
    nodes, w = G.sza_columns([0.25, 0.75, 0.5, 0.375], 3)
    assert np.array_equal(nodes, [0.25, 0.5, 0.75]) and np.array_equal(w[3], [0.5, 0.5, 0]) and np.array_equal(w[0], [1, 0, 0]) and np.array_equal(w[1], [0, 0, 1])
    assert np.array_equal(w[2], [0, 1, 0])
    # a degenerate range and n_col = 1: one node at the mean, weights of 1
    for mu, n_col in (([0.4, 0.4 + 1e-13, 0.4], 4), ([0.1, 0.7, 0.3], 1)):
        nodes, w = G.sza_columns(mu, n_col)
        assert nodes.shape == (1,) and nodes[0] == np.mean(mu) and np.array_equal(w, np.ones((3, 1)))
    with pytest.raises(ValueError):
        G.sza_columns([0.1, 0.2], 0)
    with pytest.raises(ValueError):
        G.sza_columns([0.1, 1.2], 2)


def test_exact_zeros():
    c = R.panel_case(3, 3, 5)
    mu0s, beams = DC.columns_of(c, 3)
    rng = np.random.default_rng(5)
    w, layer, _ = DC.rows_of(rng, 3, 3)
    dark = np.flatnonzero(~w.any(axis=1))
    assert dark.size == 1
    for fn in (DC.reference, DC.plain64_columns):
        o = fn(c, mu0s, beams, w, layer)
        assert np.all(o["rows"][dark] == 0) and np.all(np.delete(o["rows"], dark, axis=0) >= 0)
        # no scatterer and a black ground; no beam and a black ground
        for change in (dict(ssa=np.zeros(3)), dict(beams=np.zeros_like(beams))):
            cc = dict(c, albedo=0.0, **{k: v for k, v in change.items() if k != "beams"})
            o = fn(cc, mu0s, change.get("beams", beams), w, layer)
            assert all(np.all(o[k] == 0) for k in ("rows", "J", "flux"))
        # a gas that scatters nothing has rows of zero above a bright ground
        o = fn(dict(c, ssa=np.zeros(3), albedo=0.5), np.full(3, 0.8), beams, w, layer)
        assert np.all(o["rows"] == 0) and np.all(o["flux"][:, 0] > 0)


def test_engine_refusals_need_no_gpu():
    """The Python entry looks at its tensors first: host arrays are refused before any device call."""
    from spectrobot_amd import engine
    A, V, beams, sun = np.ones((1, 2, 3)), np.ones((1, 2)), np.ones((2, 3, 3)), np.ones(3)
    with pytest.raises(ValueError):
        engine.diffuse_source_columns(A, V, [0.5], [0.1], beams, sun, [0.2, 0.6], np.ones((2, 2)), [0, 1], out_gas=0)
    with pytest.raises(ValueError):
        engine.diffuse_source_columns(A, V, [0.5], [0.1], beams, sun, [0.2, 0.6], None, None, mean_intensity=True)
