"""Every route to the instrument's band integrals against the extended-precision CPU reference of
tests/lowres_reference.py: engine.hires_to_lowres (sr_lowres_weights_kernel, sr_lowres_apply_kernel, sr_lowres_sum_kernel),
its shards through g_lo and the weight cache's key, and the band epilogues of the recursion kernels
(sr_limb_fold_sens_lds_kernel<., true> through engine.retrieval_forward, sr_limb_jac_state_kernel<..., BANDS = true>
through engine.limb_rays_state_bands, both with sr_lowres_sum_blocks_kernel), without and with the field of view.

The limit of every comparison is 8 x max(K_PLAIN, 1) units of  2^-53 sum_i |s_i W_i| (1 + t_i^2) + 1e-290,  K_PLAIN being
what the plain fp64 evaluation (oracle.hires_to_lowres; smm.fov_closed_form on its band values) measures against the
reference on the test's own (spectrum, band) pairs -- never what a kernel gives.  Bands outside the grid and windows of
fewer than two points must be exact 0.0; every band keeps a guard of 1e-6 of the grid spacing (asserted on the CPU), the
two exact-end cases apart, whose bitwise preconditions are asserted instead.

The fused routes never write the hi-res spectra they integrate.  Those come from the unfused instance of the same kernel on
the same inputs (limb_jac_los, the resident entry of limb_rays_jacobian, which sr_retrieval_forward_dev itself runs into
`buf` under sr_set_band_fusion(0); limb_rays_state_jacobian): "the same recursion, operation for operation", built with
contraction off -- and are the reference's fp64 input data.  The recursion is pinned by tests/test_gpu_limb_reference.py.
The epilogue is one v_mfma_f64_16x16x4 chain of 16 fused multiply-adds over a wave's 64 points, then at most 16 + 16 slot
partials added by sr_lowres_sum_blocks_kernel: fewer roundings than the 256-thread strided sums, five shuffles and chunk
partials that KERNEL_MARGIN = 8 was written for, so the margin stays 8.  Needs a real MI355X."""
import functools

import numpy as np
import pytest

import lowres_reference as R

pytestmark = pytest.mark.gpu
SEED = 20261018
GRID_A = (2975.0, 5e-4)       # the grid of the sibling tests
GRID_B = (1234.5, 1e-2)       # another w0 and step: 8100 nm, spacing 0.066 nm
ROTS = [0.0, 20.0]            # the two pixels' rotations (the first has no edge term)


@pytest.fixture(scope="module")
def eng():
    import torch
    assert torch.cuda.is_available(), "these tests need the GPU"
    from spectrobot_amd import engine
    engine.set_device(0)
    return engine


def _t(v):
    import torch
    return torch.tensor(np.ascontiguousarray(v, dtype=np.float64), device="cuda")


class Tally(object):
    """The comparisons of one test: every figure is printed before anything is asserted.  K_PLAIN per kind ('band': band
    values; 'fov': after the field-of-view integral), each row held to 8 x max(its kind's K_PLAIN, 1)."""

    def __init__(self):
        self.k, self.rows, self.zeros, self.guard = {}, [], [], np.inf

    def plain(self, kind, u):
        self.k[kind] = max(self.k.get(kind, 0.0), float(np.max(u)) if np.size(u) else 0.0)

    def add(self, kind, tag, u, where="-"):
        self.rows.append((kind, tag, float(u), where))

    def band(self, tag, got, ref, spec_names=None, band_names=None):
        """got [n_spec, n_bands] against a band_reference; bands of fewer than two points must be exact zeros."""
        got = np.asarray(got)
        assert got.shape == ref["value"].shape, (got.shape, ref["value"].shape)
        self.guard = min(self.guard, float(ref["guard"].min()))
        dead = ref["count"] < 2
        if dead.any():
            self.zeros.append((tag, bool(np.all(got[:, dead] == 0.0))))
        self.add("band", tag, *R.worst(R.units_of(got, ref), spec_names, band_names))

    def finish(self, min_guard=R.GUARD_MIN):
        lim = {kind: R.limit(k) for kind, k in self.k.items()}
        print("\n" + "  ".join("K_PLAIN %s %.3g limit %.3g" % (kind, self.k[kind], lim[kind]) for kind in sorted(lim))
              + "  guard %.3g" % self.guard)
        for kind, tag, u, where in self.rows:
            print("  %-58s %10.3g units%s at %s" % (tag, u, "  OVER" if not u <= lim[kind] else "", where))
        for tag, ok in self.zeros:
            if not ok:
                print("  %s: a band without a trapezoid is not an exact 0.0" % tag)
        assert self.guard >= min_guard, "a window end within %.1e of the spacing of a grid point: %.3g" % (min_guard, self.guard)
        assert all(ok for _, ok in self.zeros), [tag for tag, ok in self.zeros if not ok]
        bad = [r for r in self.rows if not r[2] <= lim[r[0]]]
        assert not bad, "over 8 x max(K_PLAIN, 1) (%s): %s" % (lim, bad)


# ------------------------------------------------------------------------------------------------------------------
# engine.hires_to_lowres
# ------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=4)
def _panel(grid, n_pts, n_bands, n_sigma):
    return R.panel(grid[0], grid[1], n_pts, n_bands, SEED, n_sigma)


N_PTS = [2, 63, 64, 65, 257, 4095, 4096, 4097, 8193]
CONFIGS = [(1, "Wm2", 5.0), (15, "Wm2", 5.0), (16, "Wm2", 5.0), (17, "Wm2", 5.0), (33, "Wm2", 5.0), (33, "ergscm2", 5.0),
           (33, "nWcm2", 5.0), (33, "Wm2", 3.0), (33, "Wm2", 0.5), (17, "nWcm2", 0.5)]


def _run_panel(eng, T, P, units, tag):
    n_sigma = P["n_sigma"]
    ref = R.band_reference(P["grid"], P["spec"], P["centers"], P["widths"], n_sigma, units)
    T.plain("band", R.units_of(R.oracle_plain(P["grid"], P["spec"], P["centers"], P["widths"], n_sigma, units), ref))
    got = eng.hires_to_lowres(_t(P["spec"]), P["grid"], P["centers"], P["widths"], out_units=units, n_sigma=n_sigma)
    T.band(tag, got, ref, P["spec_names"], P["band_names"])
    return got, ref


@pytest.mark.parametrize("n_bands,units,n_sigma", CONFIGS)
@pytest.mark.parametrize("n_pts", N_PTS)
def test_hires_to_lowres(eng, n_pts, n_bands, units, n_sigma):
    """The panel's spectra as the rays of one call: grids on both sides of a wave, a 256-point block and the 4096-point
    chunk, band counts on both sides of the tiles of 16, the three units, three window widths."""
    P = _panel(GRID_A, n_pts, n_bands, n_sigma)
    assert len(P["centers"]) == n_bands and (n_bands < 33 or P["n_structured"] <= n_bands)
    T = Tally()
    _run_panel(eng, T, P, units, "hires_to_lowres %d pts %d bands %s n_sigma %g (%d spectra)" % (n_pts, n_bands, units, n_sigma, len(P["spec"])))
    T.finish()


@pytest.mark.parametrize("n_pts", [65, 4097])
def test_hires_to_lowres_on_another_grid(eng, n_pts):
    P = _panel(GRID_B, n_pts, 33, 5.0)
    T = Tally()
    _run_panel(eng, T, P, "Wm2", "hires_to_lowres grid w0 %g step %g, %d pts" % (GRID_B + (n_pts,)))
    T.finish()


@pytest.mark.parametrize("grid,n_pts,k", [(GRID_A, 8193, 5000), (GRID_A, 300, 130), (GRID_B, 4097, 4095)])
def test_exact_window_ends(eng, grid, n_pts, k):
    """w = 2^-2, n_sigma = 5, f = x_k +- 1.25: the window's end is bitwise the grid value x_k.  The end point belongs to
    the window (>=, <=): a one-hot spectrum at x_k returns the weight of its half interval, not 0."""
    g, _ = R.make_grid(grid[0], grid[1], n_pts)
    centers, widths, xk = R.exact_end_cases(g, k)
    assert centers[0] - 5.0 * 0.25 == xk and centers[1] + 5.0 * 0.25 == xk and xk == 1e7 / g[k] and np.all(widths == 0.25)
    far = R.guard(g, [centers[0] + 2.5, centers[1] - 2.5], [1e-9, 1e-9], 5.0)    # the far ends keep the guard
    assert far.min() >= R.GUARD_MIN, far
    rng = np.random.default_rng([SEED, n_pts, k])
    spec = np.zeros((5, n_pts))
    spec[0, k] = spec[1, k - 1] = spec[2, k + 1] = 1.0
    spec[3] = rng.uniform(0.5, 1.5, n_pts)
    spec[4] = rng.choice([-1.0, 1.0], n_pts) * 10.0 ** rng.uniform(-6.0, 0.0, n_pts)
    names = ["one-hot at k", "one-hot at k - 1", "one-hot at k + 1", "positive noise", "signed"]
    ref = R.band_reference(g, spec, centers, widths)
    assert np.all(ref["count"] >= 2) and np.all(ref["value"][0] > 0)
    # x_k is the first point of band 0 in nm order (cm-1 neighbour k + 1 lies outside) and the last of band 1
    assert ref["value"][2, 0] == 0 and ref["value"][1, 0] > 0 and ref["value"][1, 1] == 0 and ref["value"][2, 1] > 0
    T = Tally()
    T.plain("band", R.units_of(R.oracle_plain(g, spec, centers, widths), ref))
    got = eng.hires_to_lowres(_t(spec), g, centers, widths)
    T.band("exact ends, %d pts, k %d" % (n_pts, k), got, ref, names, ["lo == x_k", "hi == x_k"])
    print("\n  one-hot at x_k: kernel %s reference %s" % (got[0], np.asarray(ref["value"][0], np.float64)))
    T.finish(min_guard=0.0)     # (the guard is what these two bands give up; their far ends are asserted above)
    assert np.all(got[0] > 0) and got[2, 0] == 0.0 and got[1, 1] == 0.0


@pytest.mark.parametrize("n_pts,k", [(300, 130), (8193, 4096), (8193, 4097)])
def test_shards_and_the_weight_cache(eng, n_pts, k):
    """[0, k + 1) at g_lo = 0 and [k, n) at g_lo = k -- a shard plus the next shard's first point -- each against the
    reference's partial integral, their sum against the whole; then whole, shard, shard, whole, shard in a row: each
    bitwise what the same call gives right after an unrelated instrument step has replaced the cached weight table (cut at
    4096 of 8193 both shards have 4097 points: their keys differ in g_lo alone)."""
    P = _panel(GRID_A, n_pts, 33, 5.0)
    rows = np.r_[0:2, 2:len(P["spec"]):5]
    spec, names = P["spec"][rows], [P["spec_names"][r] for r in rows]
    grid, cw = P["grid"], (P["centers"], P["widths"])
    cuts = {"whole": (0, n_pts), "shard 0": (0, k + 1), "shard 1": (k, n_pts)}
    dev = {name: _t(spec[:, a:b]) for name, (a, b) in cuts.items()}
    other_grid, _ = R.make_grid(2975.0, 5e-4, 400)
    other = _t(np.random.default_rng(1).uniform(0, 1, (3, 400)))

    def call(name):
        return eng.hires_to_lowres(dev[name], grid, *cw, g_lo=cuts[name][0] if name != "whole" else None)

    def first(name):
        eng.hires_to_lowres(other, other_grid, [1e7 / other_grid[200]], [0.02])
        return call(name)

    T = Tally()
    fresh, refs = {}, {}
    for name, (a, b) in cuts.items():
        fresh[name] = first(name)
        refs[name] = R.band_reference(grid, spec[:, a:b], *cw, g_lo=a)
        T.plain("band", R.units_of(R.oracle_plain(grid, spec[:, a:b], *cw, g_lo=a), refs[name]))
        T.band("%s [%d, %d) of %d" % (name, a, b, n_pts), fresh[name], refs[name], names, P["band_names"])
    T.add("band", "shard 0 + shard 1 against the whole", *R.worst(R.units_of(fresh["shard 0"] + fresh["shard 1"], refs["whole"]),
                                                                  names, P["band_names"]))
    seq = ["whole", "shard 0", "shard 1", "whole", "shard 1", "shard 0", "whole"]
    same = [(name, bool(np.array_equal(call(name), fresh[name]))) for name in seq]
    print("\n  in a row, bitwise equal to a first call: %s" % same)
    T.finish()
    assert all(ok for _, ok in same), same
    assert fresh["shard 0"].any() and fresh["shard 1"].any() and not np.array_equal(fresh["shard 0"], fresh["whole"])


# ------------------------------------------------------------------------------------------------------------------
# the band epilogues of the recursion kernels
# ------------------------------------------------------------------------------------------------------------------
def _probe_masks(P, n):
    """Point masks of the coefficient tables: everything; the first and last point of every window; 63 | 64 and the two
    ends of the grid; n - 1 alone, where the clamped lanes of the last wave read."""
    W, _, count = R.weights(P["grid"], P["centers"], P["widths"], P["n_sigma"])
    ends = set()
    for b in np.flatnonzero(count >= 2):
        nz = np.flatnonzero(W[b] != 0)
        ends.update((int(nz[0]), int(nz[-1])))
    out = [("dense", np.ones(n))]
    for tag, pts in (("window ends", ends), ("63 | 64, 0, n - 1", {0, 63, 64, n - 1}), ("n - 1", {n - 1})):
        m = np.zeros(n)
        m[[p for p in pts if 0 <= p < n]] = 1.0
        out.append((tag, m))
    return out


def _fused_check(T, tag, P, spectra, unfused, fused, fused_fov, units, factors):
    """spectra [n_rays, n_row, n_pts] (the unfused instance's: the reference's input); unfused / fused [n_rays, n_row, n_bands]
    or None; fused_fov [n_pix, n_row, n_bands]."""
    from spectrobot_amd import spect_main_module as smm
    n_rays, n_row, n = spectra.shape
    nb = len(P["centers"])
    flat = spectra.reshape(n_rays * n_row, n)
    assert np.all(np.isfinite(flat))
    ref = R.band_reference(P["grid"], flat, P["centers"], P["widths"], P["n_sigma"], units)
    plain = R.oracle_plain(P["grid"], flat, P["centers"], P["widths"], P["n_sigma"], units)
    T.plain("band", R.units_of(plain, ref))
    names = ["ray %d row %d" % (r, q) for r in range(n_rays) for q in range(n_row)]
    for what, got in (("unfused", unfused), ("fused", fused)):
        if got is not None:
            T.band("%s %s" % (tag, what), got.reshape(n_rays * n_row, nb), ref, names, P["band_names"])
    if fused_fov is not None:
        shape = (n_rays, n_row, nb)
        val, A = R.fov_reference(ref["value"].reshape(shape), ref["A"].reshape(shape), factors)
        pl = plain.reshape(shape)
        T.plain("fov", R.units_raw(smm.fov_closed_form(pl[0::3], pl[1::3], pl[2::3], ROTS), val, A))
        u = R.units_raw(fused_fov, val, A)
        k = np.unravel_index(int(np.argmax(u)), u.shape)
        T.add("fov", "%s fused, field of view" % tag, u[k], "pixel %d row %d | %s" % (k[0], k[1], P["band_names"][k[2]]))
        dead = ref["count"] < 2
        T.zeros.append((tag + " fov", bool(np.all(fused_fov[..., dead] == 0.0))))
    return ref


FUSED_N = [63, 64, 65, 257, 321]


@pytest.mark.parametrize("n_par,n_gas", [(3, 1), (8, 3)])
@pytest.mark.parametrize("n_pts", FUSED_N)
def test_retrieval_forward_band_epilogue(eng, n_pts, n_par, n_gas):
    """sr_limb_fold_sens_lds_kernel<., true> + sr_lowres_sum_blocks_kernel (engine.retrieval_forward, <= 8 parameters, band
    fusion on: `buf` stays untouched) on 17 and 33 bands, without and with the field of view; the spectra it integrates are
    those the same call writes into `buf` with band fusion off, whose own band values (the apply kernel) are held too."""
    import torch
    import test_gpu_state_bands as SB
    c = SB._case(eng, n_par, 0, 0, n_gas, n_pts)
    par_gas, W = c["kw"]["par_gas"], c["kw"]["par_w"]
    x = c["rng"].uniform(0.5, 1.5, n_par) * np.array([[1.2e-2, 2e-3, 3e-4][g] for g in par_gas])
    factors = eng.fov_factors(ROTS)
    los = SB._los(eng, c)
    T = Tally()
    try:
        for n_bands, units in ((17, "Wm2"), (33, "nWcm2")):
            P = _panel(GRID_A, n_pts, n_bands, 5.0)
            assert np.array_equal(P["grid"], c["grid"])
            for mtag, m in _probe_masks(P, n_pts):
                coeffs = (_t(c["a"] * m), _t(c["e"] * m))
                call = lambda fov, buf: eng.retrieval_forward(coeffs, los, par_gas, W, x, c["grid"], P["centers"], P["widths"],
                                                              out_units=units, fov=fov, buf=buf)
                eng.set_band_fusion(0)
                unfused, buf = call(None, None)
                spectra = buf.cpu().numpy()
                spectra = np.concatenate([spectra[:6, None], spectra[6:].reshape(6, n_par, n_pts)], axis=1)
                eng.set_band_fusion(1)
                mark = torch.full_like(buf, -7.0)
                fused, fused_fov = call(None, mark)[0], call(factors, mark)[0]
                assert bool((mark == -7.0).all()), "the fused route was not taken"
                assert mtag != "dense" or np.count_nonzero(spectra) > spectra.size // 2
                assert mtag == "dense" or (np.count_nonzero(spectra.any(axis=(0, 1))) == int(m.sum()) and spectra[:, 0].any())
                _fused_check(T, "retrieval_forward %d par %d bands, %s:" % (n_par, n_bands, mtag), P, spectra, unfused, fused, fused_fov,
                             units, factors)
    finally:
        eng.set_band_fusion(1)
    T.finish()


@pytest.mark.parametrize("kinds,n_gas", [((0, 8, 0), 1), ((0, 16, 0), 3), ((5, 12, 3), 3)])
@pytest.mark.parametrize("n_pts", FUSED_N)
def test_state_bands_epilogue(eng, n_pts, kinds, n_gas):
    """sr_limb_jac_state_kernel<..., BANDS = true> + sr_lowres_sum_blocks_kernel (engine.limb_rays_state_bands) at NP 8, NP 16
    (the second row tile) and two parameter blocks, 17 and 33 bands, without and with the field of view; the spectra it
    integrates are limb_rays_state_jacobian's on the same inputs."""
    import test_gpu_state_bands as SB
    c = SB._case(eng, *kinds, n_gas, n_pts)
    factors = eng.fov_factors(ROTS)
    los = SB._los(eng, c)
    n_par = c["n_par"]
    T = Tally()
    for n_bands, units in ((17, "ergscm2"), (33, "Wm2")):
        P = _panel(GRID_A, n_pts, n_bands, 5.0)
        assert np.array_equal(P["grid"], c["grid"])
        for mtag, m in _probe_masks(P, n_pts):
            coeffs = (_t(c["a"] * m), _t(c["e"] * m))
            kw = dict(c["kw"])
            if "tab" in kw:
                kw["tab"] = _t(c["tab_np"] * m)
            if "dcoeffs" in kw:
                kw["dcoeffs"] = (_t(c["da"] * m), _t(c["de"] * m))
            rad, jac = eng.limb_rays_state_jacobian(coeffs, los, grid=c["grid"], **kw)
            spectra = np.concatenate([rad.cpu().numpy()[:, None], jac.cpu().numpy()], axis=1)
            run = lambda fov: eng.limb_rays_state_bands(coeffs, los, c["grid"], P["centers"], P["widths"], out_units=units, fov=fov, **kw)
            fused, fused_fov = run(None), run(factors)
            assert fused.shape == (6, 1 + n_par, n_bands) and fused_fov.shape == (2, 1 + n_par, n_bands)
            assert mtag != "dense" or np.count_nonzero(spectra) > spectra.size // 4
            assert mtag == "dense" or (np.count_nonzero(spectra.any(axis=(0, 1))) == int(m.sum()) and spectra[:, 1:].any())
            _fused_check(T, "state_bands %s %d bands, %s:" % (kinds, n_bands, mtag), P, spectra, None, fused, fused_fov, units, factors)
    T.finish()
