"""The table preparation layer by layer, and region 4's exponential at the accuracy the spectrum is held to.

sr_prep_kernel / sr_prep_batch_kernel prepare every (line, layer) on its own.  A preparation that keeps a wave on its
64 lines and loops over a block of layers (the line data read once per block instead of once per layer) was built and
measured with this file and taken out again: it was slower (profiles/bytes_and_digits_ab.txt).  Its tests stay as the
property any such variant has to keep: row k of a call over n layers is the one-layer call on layer k bit for bit, for
layer counts around one and two blocks of 8 or 16 (1, 7, 8, 9, 15, 16, 17, 35), with vibrational temperatures, with
frozen boundaries and linearised weights, per level, and on a shard whose last line chunk is partial and has a wave
that writes no cold record; and the level tables of the multi-channel route (sr_prep_batch_kernel) against the
per-level route's.

Region 4 (exp_core, sr_device.hpp: a polynomial of total degree 9, <= 1.8e-14 relative by its derivation) through the
humliv_bb shim against the oracle, one line at a time: <= 1e-12 relative at every region-4 point, out to the core's
outer seam at rx = 5.5 + ry.  A wrong coefficient
shows at 1e-9 or more; a correct exp_core leaves the comparison where exp_bounded had it (2.5e-14 .. 3.3e-14: the
rational part's rounding)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

LAYER_COUNTS = [1, 7, 8, 9, 15, 16, 17, 35]
N_MAX = max(LAYER_COUNTS)


@pytest.fixture(scope="module")
def eng():
    import torch
    assert torch.cuda.is_available(), "these tests need the GPU"
    from spectrobot_amd import engine
    engine.set_device(0)
    return engine


@pytest.fixture(scope="module")
def case(eng):
    """400 lines on 3000 points, 35 layers, and the one-layer calls on every layer (computed once, shared)."""
    from spectrobot_amd import synthetic as syn
    grid = syn.make_grid(2975.0, 5e-4, 3000)
    L = syn.make_lines(400, grid, seed=5201, n_levels=12)
    atm = syn.make_atmosphere(N_MAX, 12)
    T, P, tv = atm["temps"], atm["press"], atm["tvib"]
    ls = eng.LineSet(L, grid, 6, 1, syn.CH4_MM, syn.CH4_LEVEL_ENERGIES)
    one = [ls.abscoeff_layers(T[k:k + 1], P[k:k + 1], tvib=tv[:, k:k + 1]) for k in range(N_MAX)]
    return dict(ls=ls, T=T, P=P, tv=tv, one=one, grid=grid)


@pytest.mark.parametrize("n_layers", LAYER_COUNTS)
def test_layer_blocks_are_invisible(case, n_layers):
    import torch
    ls, T, P, tv = case["ls"], case["T"], case["P"], case["tv"]
    n = n_layers
    a, e = ls.abscoeff_layers(T[:n], P[:n], tvib=tv[:, :n])
    assert float(a.abs().max()) > 0 and float(e.abs().max()) > 0
    for k in range(n):
        a1, e1 = case["one"][k]
        assert torch.equal(a[k], a1[0]) and torch.equal(e[k], e1[0]), "layer %d of %d" % (k, n)


def test_layer_blocks_frozen_boundaries_linear_weights(case):
    """17 layers (a short last block for a block size of 8 or 16) with the boundaries frozen at T and the weights
    linearised about T, called at T + 0.05 K."""
    import torch
    ls, T, P, tv = case["ls"], case["T"][:17], case["P"][:17], case["tv"][:, :17]
    try:
        ls.set_bounds_temps(T, linear_weights=True)
        a, e = ls.abscoeff_layers(T + 0.05, P, tvib=tv)
        for k in range(17):
            ls.set_bounds_temps(T[k:k + 1], linear_weights=True)
            a1, e1 = ls.abscoeff_layers(T[k:k + 1] + 0.05, P[k:k + 1], tvib=tv[:, k:k + 1])
            assert torch.equal(a[k], a1[0]) and torch.equal(e[k], e1[0]), "layer %d" % k
    finally:
        ls.set_bounds_temps(None)
    # (not the unfrozen result: the linearised weights differ from the exact ones at T + 0.05 K)
    a0, _ = ls.abscoeff_layers(T + 0.05, P, tvib=tv)
    assert not torch.equal(a, a0)


def test_layer_blocks_per_level(case):
    """gcoeff_layers(level=3): the per-level weight modes, 17 layers against one at a time."""
    import torch
    ls, T, P = case["ls"], case["T"][:17], case["P"][:17]
    g = ls.gcoeff_layers(T, P, level=3)                       # [3, k, n]
    assert float(g.abs().max()) > 0
    for k in range(17):
        g1 = ls.gcoeff_layers(T[k:k + 1], P[k:k + 1], level=3)
        assert torch.equal(g[:, k], g1[:, 0]), "layer %d" % k


def test_layer_blocks_on_a_shard_with_a_partial_line_chunk(eng):
    """130 lines (two whole waves and one of two lines) on the shard [137, 137 + 2651): the last wave's two lines lie
    beyond the shard with their whole zones, so that wave writes no cold record in any layer."""
    import torch
    from spectrobot_amd import synthetic as syn, spect_classes as spcl
    grid = syn.make_grid(2975.0, 5e-4, 3000)
    L = syn.make_lines(130, grid, seed=5202, n_levels=12)
    L["freq"][-2:] = [grid[2960] + 1e-4, grid[2990] + 2e-4]
    o = np.argsort(L["freq"], kind="stable")
    L = {k: np.ascontiguousarray(v[o]) for k, v in L.items()}
    lo, hi = 137, 137 + 2651
    atm = syn.make_atmosphere(17, 12)
    T, P, tv = atm["temps"], atm["press"], atm["tvib"]
    for k in range(17):   # half a zone, (15 dw' + lw) / step points (lineshape.f:447-454), stays right of the shard
        for j in (-2, -1):
            lw = spcl.Lorenz_width(T[k], spcl.convert_to_atm(P[k]), L["t_dep_broad"][j], L["air_broad"][j])
            dwp = spcl.Doppler_width(T[k], syn.CH4_MM, L["freq"][j]) / np.sqrt(np.log(2.0))
            assert (L["freq"][j] - grid[hi - 1]) / 5e-4 > (15.0 * dwp + lw) / 5e-4 + 2
    ls = eng.LineSet(L, grid, 6, 1, syn.CH4_MM, syn.CH4_LEVEL_ENERGIES)
    a, e = ls.abscoeff_layers(T, P, tvib=tv, g_lo=lo, g_hi=hi)
    assert a.shape == (17, hi - lo) and float(a.abs().max()) > 0
    for k in range(17):
        a1, e1 = ls.abscoeff_layers(T[k:k + 1], P[k:k + 1], tvib=tv[:, k:k + 1], g_lo=lo, g_hi=hi)
        assert torch.equal(a[k], a1[0]) and torch.equal(e[k], e1[0]), "layer %d" % k


def _plane_err(a, b):
    """test_gpu_glevel._plane_err: max |a - b| relative to the largest |b| of each (level, channel, row) spectrum."""
    s = b.abs().amax(dim=-1, keepdim=True).clamp_min(1e-300)
    return float(((a - b).abs() / s).max())


def test_level_table_build_agrees_with_itself(eng):
    """The multi-channel route (its sparse far-only passes are prepared by sr_prep_batch_kernel) against one coefficient
    op per level, 3 layers and 12 levels: the two routes differ by the order of summation only, <= 2e-12 of a
    spectrum's largest value (test_multichannel_route_equals_the_per_level_route)."""
    import torch
    from spectrobot_amd import synthetic as syn
    grid = syn.make_grid(2975.0, 5e-4, 3000)
    L = syn.make_lines(400, grid, seed=5203, n_levels=12)
    atm = syn.make_atmosphere(3, 12)
    T, P = atm["temps"], atm["press"]
    ls = eng.LineSet(L, grid, 6, 1, syn.CH4_MM, syn.CH4_LEVEL_ENERGIES)
    res = {}
    try:
        for route in (1, 0):
            eng.set_level_route(route)
            res[route] = (ls.glevel_pairs(T, P), ls.gcoeff_levels(T, P))
            torch.cuda.synchronize()
    finally:
        eng.set_level_route(1)
    assert float(res[0][0].abs().max()) > 0 and float(res[0][1].abs().max()) > 0
    err = (_plane_err(res[1][0], res[0][0]), _plane_err(res[1][1], res[0][1]))
    print("multi-channel against per-level route: pairs %.2e ctypes %.2e" % err)
    assert err[0] < 2e-12 and err[1] < 2e-12


# ---- region 4 against the oracle ------------------------------------------------------------------------------------
# The reference's middle branch places the seam between region 2 and the core by index at rx - ry = 5.5
# (lineshape.f:483-490: il2 = il + nint((rx - ry - 5.5) / xstep), rx = |x - x0| / dw), and takes a core point to region 4
# where ry < 0.195 rx - 0.176 (:528-530): region 4 is rx in ((ry + 0.176) / 0.195, 5.5 + ry), which exists up to
# ry = 1.1137.  Re c1 = ry^2 - rx^2 is most negative at the outer seam: -32.4 at ry = 0.15, -39.0 at 0.8, -41.3 at 1.0
# (-42.5 at the largest ry): the arguments at which exp_core's dropped low word of ln2 weighs most.  ry = 1.0 is added
# to the six values for that reason.
RY_REGION4 = [1e-9, 1e-5, 6e-4, 0.05, 0.15, 0.8, 1.0]
DW = 0.2            # dw / step = 400: region 4 of ry = 1.0 holds 2 x 188 points, of ry = 0.8 2 x 518
STEP = 5e-4


def _region4_formula(rx, ry):
    """Region 4 as the reference writes it (lineshape.f:530-546) at c2 = (single(ry), single(-rx)), in numpy."""
    c2 = np.float64(np.float32(ry)) + 1j * np.float32(-rx).astype(np.float64)
    c1 = c2 * c2
    f = lambda v: float(np.float32(v))   # the literals are default-kind reals
    p = f(36183.31) - c1 * (f(3321.9905) - c1 * (f(1540.787) - c1 * (f(219.0313) - c1 * (f(35.76683) - c1 * (
        f(1.320522) - c1 * f(.56419))))))
    q = f(32066.6) - c1 * (f(24322.84) - c1 * (f(9022.228) - c1 * (f(2186.181) - c1 * (f(364.2191) - c1 * (
        f(61.57037) - c1 * (f(1.841439) - c1))))))
    return np.exp(c1.real) * np.cos(c1.imag) - (c2 * p / q).real


def _window(oracle, ry):
    """One 13010-point window with the line 0.3 steps off its centre point, the oracle's values and the mask of region
    4: two points inside the index-placed seam at rx - ry = 5.5, 1e-6 inside the per-point seam to region 3."""
    x = 3000.0 + STEP * np.arange(13010)
    x0 = x[6505] + 0.3 * STEP
    lw = ry * DW
    yo = oracle.humliv_bb(x, 1, 13010, x0, lw, DW)
    rx = np.abs(x - x0) / DW
    r = lw / DW
    reg4 = (rx - r < 5.5 - 2 * STEP / DW) & (r < 0.195 * rx - 0.176 - 1e-6)
    return x, x0, lw, yo, rx, reg4


@pytest.mark.parametrize("ry", RY_REGION4)
def test_region4_against_the_oracle(eng, oracle, ry):
    from spectrobot_amd.compat import lineshape
    x, x0, lw, yo, rx, reg4 = _window(oracle, ry)
    # the oracle alone: at least 200 points, out to the seam at 5.5 + ry, and it evaluates them by the region-4 formula
    # (region 3's rational function differs from it by ~1e-4 there, region 2's by more)
    assert reg4.sum() >= 200, "the window must put 200 points into region 4"
    assert rx[reg4].max() > 5.5 + ry - 4 * STEP / DW
    assert np.all(yo[reg4] > 0)
    f4 = _region4_formula(rx[reg4], ry)
    assert float(np.max(np.abs(yo[reg4] - f4) / np.abs(f4))) < 1e-12
    y = lineshape.humliv_bb(x, 1, 13010, x0, lw, DW)
    err = float(np.max(np.abs(y[reg4] - yo[reg4]) / np.abs(yo[reg4])))
    u_min = float(np.float32(ry)) ** 2 - float(rx[reg4].max()) ** 2
    print("ry %.1e: %d region-4 points, Re c1 down to %.1f, max rel err %.2e" % (ry, reg4.sum(), u_min, err))
    assert err <= 1e-12
