"""The radiance budget of limb rays in one pass (sr_limb_rays_parts_dev, engine.limb_rays_parts,
LevelFactored.level_radiances, retrieval.radtrans(track_levels=...)).  The reference's single_rads come from the absent
spect_base_module: the definition is the build's, checked (A) against a composition of existing ops that is the same
linear functional, (B) for closure, (C) against the CPU oracle's recursion, (D) for its argument checks, (E) on the
public route.  Scene and cases of tests/test_gpu_tvib_jacobian.py."""
import ctypes as C

import numpy as np
import pytest

from conftest import far_tol, relerr

pytestmark = pytest.mark.gpu

N_GRID = 24000
Z_TANS = [130.0, 300.0, 480.0, 650.0]
BANDS = [(-np.inf, 300.0), (300.0, 600.0), (600.0, np.inf)]          # km: three altitude bands


@pytest.fixture(scope="module")
def eng():
    import torch
    assert torch.cuda.is_available(), "these tests need the GPU"
    from spectrobot_amd import engine
    engine.set_device(0)
    return engine


@pytest.fixture(scope="module")
def scene(eng):
    from spectrobot_amd import synthetic as syn
    grid = syn.make_grid(2990.0, 5e-4, N_GRID)
    L = syn.make_lines(9000, grid, seed=21, n_levels=12, config_id=2)
    atm = syn.make_atmosphere(7, 12)
    atm["nd"] = syn.number_density(atm["press"], atm["temps"])
    ls = eng.LineSet(L, grid, 6, 1, syn.CH4_MM, syn.CH4_LEVEL_ENERGIES)
    Lc = syn.make_lines(700, grid, seed=3, n_levels=0, co_like=True)
    lc = eng.LineSet(Lc, grid, 5, 1, syn.CO_MM, [])
    return dict(grid=grid, atm=atm, ls=ls, lc=lc)


def _build(eng, scene, case):
    """The LOS batch (and its twin without an initial intensity), the level-factored gas's tables and coefficients and
    the parts of one case: part_gas, part_level, part_c [n_part, n_rows]."""
    import torch
    from spectrobot_amd import synthetic as syn
    atm, ls, grid = scene["atm"], scene["ls"], scene["grid"]
    z = atm["z"]
    vm = np.full(7, 0.0148)
    opts = {}
    if case == "observer":
        opts["LOS_order"] = "observer"
    if case == "solo":
        opts["solo_absorption"] = True
    init = 180.0 if case in ("planck", "shard", "solo") else None
    g_lo, g_hi = (5000, 17000) if case == "shard" else (0, N_GRID)
    two = case == "two_gas"
    vmrs = [np.full(7, 3e-4), vm] if two else [vm]
    scale = [1.0, syn.CH4_ISO_RATIO] if two else [syn.CH4_ISO_RATIO]
    if case == "3d":
        Lr = syn.limb_los_3d(z, atm["nd"], vmrs, Z_TANS[:3], 50.0, 30.0)
        step_row = Lr["seg_alt_layer"].astype(np.int32)        # a coefficient row per LOS step, seven table rows
        po = Lr["pt_off"]
        alt_rows = np.array([Lr["alt"][a:b].mean() for a, b in zip(po[:-1], po[1:])])
        exc = (atm["tvib"] - atm["temps"][None, :])[:, step_row]
        tvib = atm["temps"][step_row][None, :] + exc * (0.4 + 1.2 * np.clip(Lr["seg_mu"], 0.0, 1.0))[None, :]
    else:
        Lr = syn.limb_los(z, atm["nd"], vmrs, Z_TANS)
        step_row = np.arange(7, dtype=np.int32)
        alt_rows = z
        tvib = atm["tvib"].copy()
    mk = lambda **kw: eng.LimbLOS(Lr["seg_off"], Lr["seg_layer"], Lr["pt_off"], Lr["x"], Lr["nd"], Lr["vmr"], col_scale=scale, **kw)
    los = mk(initial_temperature=init, **opts)
    los0 = mk(**opts) if init is not None else los
    lf = eng.LevelFactored(ls, atm["temps"], atm["press"], g_lo=g_lo, g_hi=g_hi)
    co = lf.steps(step_row, tvib=tvib)
    gas, n_gas = 0, 1
    if two:
        gas, n_gas = 1, 2
        c0 = scene["lc"].abscoeff_layers(atm["temps"], atm["press"])
        co = (torch.stack([c0[0], co[0]]).contiguous(), torch.stack([c0[1], co[1]]).contiguous())
    pop = ls.level_populations(atm["temps"][step_row], tvib=tvib).T          # [n_levels, n_rows]
    n_rows = len(step_row)
    if case == "np_small":      # 5 parts + the background: the kernel's other block size; one part without coefficients
        lev = [1, 5, 5, 8]
        pc = [pop[1], pop[5], np.zeros(n_rows), pop[8]]
    elif case == "banded":      # 12 levels x 3 altitude bands + the gas part: 37 parts + the background, three blocks
        lev = [L for L in range(12) for _ in BANDS]
        pc = [pop[L] * ((alt_rows >= lo) & (alt_rows < hi)) for L in range(12) for lo, hi in BANDS]
    else:
        lev = list(range(12))
        pc = [pop[L] for L in range(12)]
    part_gas = np.array([gas] * len(lev) + list(range(n_gas)), np.int32)
    part_level = np.array(lev + [-1] * n_gas, np.int32)
    part_c = np.array(pc + [np.zeros(n_rows)] * n_gas)
    return dict(los=los, los0=los0, lf=lf, co=co, gas=gas, n_gas=n_gas, step_row=step_row, tvib=tvib, pop=pop, g_lo=g_lo,
                grid=grid, part_gas=part_gas, part_level=part_level, part_c=part_c, init=init)


def _emission_rows(eng, b, k):
    """[n_gas, n_rows, n_pts]: the emission share of part k from existing ops, zeros for the other gases."""
    import torch
    a, e = eng._gas_stack(b["co"])
    out = torch.zeros_like(e)
    g = int(b["part_gas"][k])
    if b["part_level"][k] < 0:
        out[g] = e[g]
    else:
        oh = np.zeros((len(b["step_row"]), b["lf"].tab.shape[0]))
        oh[:, b["part_level"][k]] = b["part_c"][k]
        out[g] = eng.glevel_combine(b["lf"].tab, b["step_row"], oh)[1]
    return out


def _composition(eng, b):
    """ref [n_rays, n_part + 1, n_pts]: every part by limb_rays((abs_total, its emission share), the paths without an
    initial intensity), the background by limb_rays of the batch itself with zero emission."""
    import torch
    a, e = eng._gas_stack(b["co"])
    n_part = len(b["part_level"])
    ref = torch.empty((b["los"].n_rays, n_part + 1, a.shape[2]), dtype=torch.float64, device="cuda")
    for k in range(n_part):
        ref[:, k] = eng.limb_rays((a, _emission_rows(eng, b, k)), b["los0"], grid=b["grid"], g_lo=b["g_lo"])
    ref[:, n_part] = eng.limb_rays((a, torch.zeros_like(e)), b["los"], grid=b["grid"], g_lo=b["g_lo"])
    return ref


def _row_err(a, ref):
    """max |a - ref| of every (ray, part) row, scaled by the row's largest |ref| (rows of zeros: absolute)."""
    s = ref.abs().amax(dim=-1)
    s = s.masked_fill(s == 0, 1.0)
    return (a - ref).abs().amax(dim=-1) / s


def _call(eng, b, **kw):
    return eng.limb_rays_parts(b["co"], b["los"], b["part_gas"], b["part_level"], part_c=b["part_c"], tab=b["lf"].tab,
                               coef_row=b["step_row"], gas=b["gas"], grid=b["grid"], g_lo=b["g_lo"], **kw)


CASES = ["1d", "3d", "observer", "solo", "planck", "two_gas", "shard", "np_small", "banded"]


@pytest.mark.parametrize("case", CASES)
def test_equals_the_composition_and_closes(eng, scene, case):
    """A.  Every part against glevel_combine (one-hot part_c: the part's emission rows) -> limb_rays with the total
    absorption and no initial intensity; the background against limb_rays of the batch with zero emission; rad against
    limb_rays.  Per (ray, part) row, scaled by the row's largest reference value: at most 1e-12.  Rows that must be zero
    (level 0, a part without coefficients, every part under solo) are exactly 0.0.
    B.  Closure, per ray: |gas parts + B - rad| <= 1e-12 max|rad|; the level parts of the gas sum to its gas part and the
    three bands of a level to the level's part (the `1d` call of the same paths) at 1e-12 of that part's maximum.
    Not vacuous: at least 10 of the 12 level parts reach 1e-3 max|rad| on every ray, judged on the composition.
    Measured on the MI355X, largest row error against the composition / rad against limb_rays: 1d 5.0e-16 / 7.8e-16, 3d
    3.6e-16 / 6.5e-16, observer 3.7e-16 / 6.5e-16, solo 4.5e-16 (the background) / 8.6e-16, planck 5.0e-16 / 6.2e-16, two_gas
    4.6e-16 / 6.4e-16, shard 4.9e-16 / 6.5e-16, np_small 5.0e-16 / 7.8e-16, banded 4.1e-16 / 7.8e-16.  Closure: gas parts + B -
    rad 0 ... 3.7e-16, level parts - gas part 3.7e-16 ... 5.5e-16, bands - level part 5.0e-16.  11 of the 12 level parts reach
    1e-3 max|rad| on every ray of 1d, 3d, observer, planck, two_gas and shard (smallest non-zero share 1.7e-2, 3d 3.8e-3;
    the Planck background is 5.5e-3 of max|rad|)."""
    import torch
    b = _build(eng, scene, case)
    los, lf = b["los"], b["lf"]
    n_part = len(b["part_level"])
    ref = _composition(eng, b)
    rad, parts = _call(eng, b)
    assert tuple(parts.shape) == (los.n_rays, n_part + 1, lf.tab.shape[3]) and torch.isfinite(parts).all()
    r0 = eng.limb_rays(b["co"], los, grid=b["grid"], g_lo=b["g_lo"])
    is_gas = torch.as_tensor(b["part_level"] < 0, device="cuda")
    is_lev = ~is_gas
    err = _row_err(parts, ref)
    rmax = r0.abs().amax(dim=-1)                                        # [n_rays]
    rmax = rmax.masked_fill(rmax == 0, 1.0)                             # (solo: the lowest ray is absorbed entirely)
    share = ref.abs().amax(dim=-1) / rmax[:, None]                     # [n_rays, n_part + 1], from the composition
    print("parts [%s]: %d parts + background, %d coefficient rows; new kernel vs the composition, largest row error %.2e "
          "(level parts %.2e, gas parts %.2e, background %.2e); rad vs limb_rays %.2e"
          % (case, n_part, len(b["step_row"]), float(err.max()), float(err[:, :n_part][:, is_lev].max()),
             float(err[:, :n_part][:, is_gas].max()), float(err[:, n_part].max()),
             relerr(rad.cpu().numpy(), r0.cpu().numpy())))
    assert float(err.max()) <= 1e-12
    assert relerr(rad.cpu().numpy(), r0.cpu().numpy()) < 1e-13
    # rows of exact zeros
    zero = ref.abs().amax(dim=-1) == 0
    assert bool((parts.abs().amax(dim=-1)[zero] == 0).all())
    lev0 = torch.as_tensor(b["part_level"] == 0, device="cuda")
    assert bool(zero[:, :n_part][:, lev0].all())
    if case == "np_small":
        assert bool(zero[:, 2].all()) and not bool(zero[:, 1].any())
    if case == "solo":
        assert bool(zero[:, :n_part].all()) and torch.equal(parts[:, n_part], rad)
    if b["init"] is None:
        assert bool(zero[:, n_part].all())
    else:
        assert float(ref[:, n_part].abs().max()) > 0
    # B: closure
    tot = parts[:, :n_part][:, is_gas].sum(dim=1) + parts[:, n_part]
    clo = (tot - rad).abs().amax(dim=-1) / rmax
    gp = parts[:, n_part - b["n_gas"] + b["gas"]]                       # the gas part of the level-factored gas
    gmax = gp.abs().amax(dim=-1)
    gmax = gmax.masked_fill(gmax == 0, 1.0)
    print("parts [%s]: closure gas parts + B - rad %.2e of max|rad|" % (case, float(clo.max())))
    assert float(clo.max()) <= 1e-12
    if case != "np_small":
        clo_lev = (parts[:, :n_part][:, is_lev].sum(dim=1) - gp).abs().amax(dim=-1) / gmax
        print("parts [%s]: closure level parts - gas part %.2e of the gas part's maximum" % (case, float(clo_lev.max())))
        assert float(clo_lev.max()) <= 1e-12
    if case == "banded":
        b1 = _build(eng, scene, "1d")
        p1 = _call(eng, b1, want_rad=False)[1]
        three = parts[:, :36].reshape(los.n_rays, 12, 3, -1).sum(dim=2)
        s = p1[:, :12].abs().amax(dim=-1)
        s = s.masked_fill(s == 0, 1.0)
        clo_band = ((three - p1[:, :12]).abs().amax(dim=-1) / s)
        print("parts [banded]: closure bands - level part %.2e of the level part's maximum; bands that see nothing: %d of %d rows"
              % (float(clo_band.max()), int(zero[:, :36].sum()), zero[:, :36].numel()))
        assert float(clo_band.max()) <= 1e-12
        assert bool((three[:, 0] == 0).all())
    # not vacuous: judged on the composition's values
    if case not in ("solo", "np_small", "banded"):
        seen = (share[:, :12] >= 1e-3).sum(dim=1)
        pos = share[:, :12][share[:, :12] > 0]
        print("parts [%s]: level parts that reach 1e-3 max|rad| per ray %s, smallest non-zero share %.2e, background share %.2e"
              % (case, seen.cpu().tolist(), float(pos.min()), float(share[:, n_part].max())))
        assert int(seen.min()) >= 10
    if case == "1d":
        # the object's route: populations from level_populations, every level, a gas part per gas
        rad2, parts2, labels = lf.level_radiances(b["co"], los, b["step_row"], b["tvib"])
        assert labels == [("level", L) for L in range(12)] + [("gas", 0), ("background",)]
        assert torch.equal(parts2, parts) and torch.equal(rad2, rad)
        alt = scene["atm"]["z"]
        w = np.array([(alt >= lo) & (alt < hi) for lo, hi in BANDS], float)
        _, p3, lab3 = lf.level_radiances(b["co"], los, b["step_row"], b["tvib"], levels=[5, 5, 5], weights=w, gas_parts=False)
        assert lab3 == [("level", 5)] * 3 + [("background",)] and tuple(p3.shape)[1] == 4
        s5 = float(parts[:, 5].abs().max())
        assert float((p3[:, :3].sum(dim=1) - parts[:, 5]).abs().max()) <= 1e-12 * s5
        # gas parts alone need no tables
        rad4, p4 = eng.limb_rays_parts(b["co"], los, [0], [-1])
        assert torch.equal(p4[:, 0], parts[:, 12]) and torch.equal(rad4, rad)


@pytest.mark.parametrize("case", ["1d", "two_gas"])
def test_against_the_cpu_oracle_recursion(eng, scene, oracle, case):
    """C.  Every part of every ray against the CPU oracle's recursion on effective rows: coefficients and emission shares
    copied to the host, per segment abs_eff[s] = sum_g abs_g u_g, emi_eff[s] = e_k u_g(k), radiance_ray(abs_eff, emi_eff,
    arange, ones).  Row-scaled error at most 1e-12 (the recursion tests hold 1e-13 pointwise against this oracle; the
    factor 10 is for the product abs u formed on the host); the pointwise figure is printed.
    Measured on the MI355X: 1d row-scaled 4.9e-16, pointwise 7.6e-16; two_gas 5.5e-16, 7.4e-16."""
    b = _build(eng, scene, case)
    los = b["los"]
    a, e = eng._gas_stack(b["co"])
    a_h = a.cpu().numpy()
    col = los.columns()                                                # [n_gas, n_seg]
    n_part = len(b["part_level"])
    _, parts = _call(eng, b, want_rad=False)
    parts = parts.cpu().numpy()
    worst_row = worst_pt = 0.0
    for k in range(n_part):
        g = int(b["part_gas"][k])
        e_h = _emission_rows(eng, b, k)[g].cpu().numpy()
        for r in range(los.n_rays):
            s = np.arange(los.seg_off[r], los.seg_off[r + 1])
            lay = los.seg_layer[s]
            abs_eff = sum(a_h[gg][lay] * col[gg, s][:, None] for gg in range(b["n_gas"]))
            emi_eff = e_h[lay] * col[g, s][:, None]
            want = oracle.radiance_ray(abs_eff, emi_eff, np.arange(len(s), dtype=np.int32), np.ones(len(s)))
            got = parts[r, k]
            m = np.abs(want).max()
            if m == 0:
                assert np.all(got == 0)
                continue
            worst_row = max(worst_row, float(np.abs(got - want).max() / m))
            nz = want != 0
            worst_pt = max(worst_pt, relerr(got[nz], want[nz]))
    print("parts [%s] vs the CPU oracle: largest row-scaled error %.2e, largest pointwise relative error %.2e"
          % (case, worst_row, worst_pt))
    assert worst_row <= 1e-12
    assert np.all(parts[:, n_part] == 0)                               # no initial intensity: no background


def test_refused_arguments_leave_the_outputs_untouched(eng, scene):
    """D.  Every refused argument returns its status before anything is copied or launched (rad and parts keep their
    sentinel), and a valid call afterwards on the same stream gives the result of before."""
    import torch
    from spectrobot_amd import _lib
    b = _build(eng, scene, "two_gas")
    lf, los = b["lf"], b["los"]
    a, e = eng._gas_stack(b["co"])
    n_gas, n_layers, n_pts = a.shape
    n_lev, n_rows = lf.tab.shape[0], lf.tab.shape[2]
    n_part = len(b["part_level"])
    good_rad, good = _call(eng, b)
    torch.cuda.synchronize()
    parts = torch.full((los.n_rays, n_part + 1, n_pts), 7.25, dtype=torch.float64, device="cuda")
    rad = torch.full((los.n_rays, n_pts), 7.25, dtype=torch.float64, device="cuda")
    ip_, dp_ = _lib.ip, _lib.dp
    ptr = lambda t: C.c_void_p(t.data_ptr())
    pc = np.ascontiguousarray(b["part_c"])

    def call(**kw):
        d = los.desc()
        if "init_mode" in kw:
            d.init_mode = kw["init_mode"]
        row = np.ascontiguousarray(kw.get("coef_row", b["step_row"]), dtype=np.int32)
        lev = np.ascontiguousarray(kw.get("part_level", b["part_level"]), dtype=np.int32)
        pg = np.ascontiguousarray(kw.get("part_gas", b["part_gas"]), dtype=np.int32)
        return _lib.lib.sr_limb_rays_parts_dev(
            ptr(a), ptr(e), n_layers, kw.get("n_pts", n_pts), C.byref(d), kw.get("gas", b["gas"]),
            None if kw.get("no_tab") else ptr(lf.tab), kw.get("n_levels", n_lev), n_rows, row.ctypes.data_as(ip_),
            kw.get("n_part", n_part), pg.ctypes.data_as(ip_), lev.ctypes.data_as(ip_), pc.ctypes.data_as(dp_), ptr(rad),
            None if kw.get("no_parts") else ptr(parts), eng._stream_ptr())

    def edit(arr, i, v):
        out = arr.copy()
        out[i] = v
        return out

    refused = [(dict(no_parts=True), _lib.SR_ERR_ARG), (dict(n_part=0), _lib.SR_ERR_ARG),
               (dict(part_level=edit(b["part_level"], 3, n_lev)), _lib.SR_ERR_ARG),
               (dict(part_level=edit(b["part_level"], 0, -2)), _lib.SR_ERR_ARG),
               (dict(part_gas=edit(b["part_gas"], 4, 0)), _lib.SR_ERR_ARG),          # a level part of the other gas
               (dict(gas=0), _lib.SR_ERR_ARG), (dict(no_tab=True), _lib.SR_ERR_ARG),
               (dict(part_gas=edit(b["part_gas"], n_part - 1, n_gas)), _lib.SR_ERR_ARG),
               (dict(part_gas=edit(b["part_gas"], n_part - 2, -1)), _lib.SR_ERR_ARG),
               (dict(coef_row=edit(b["step_row"], 3, -1)), _lib.SR_ERR_ARG),
               (dict(coef_row=edit(b["step_row"], 6, n_rows)), _lib.SR_ERR_ARG),
               (dict(init_mode=1), _lib.SR_ERR_ARG), (dict(n_pts=2000001), _lib.SR_ERR_LIMIT)]
    for kw, status in refused:
        assert call(**kw) == status, kw
        torch.cuda.synchronize()
        assert bool((parts == 7.25).all()) and bool((rad == 7.25).all()), kw
    assert call() == _lib.SR_OK
    torch.cuda.synchronize()
    assert torch.equal(parts, good) and torch.equal(rad, good_rad)
    # the wrappers' own checks
    with pytest.raises(ValueError):
        eng.limb_rays_parts(b["co"], los, b["part_gas"], b["part_level"], part_c=b["part_c"], tab=lf.tab, coef_row=b["step_row"][:5], gas=1)
    with pytest.raises(ValueError):
        eng.limb_rays_parts(b["co"], los, b["part_gas"], b["part_level"], part_c=b["part_c"][:4], tab=lf.tab, coef_row=b["step_row"], gas=1)
    with pytest.raises(ValueError):
        eng.limb_rays_parts(b["co"], los, b["part_gas"], b["part_level"])              # level parts without tables
    with pytest.raises(ValueError):
        lf.level_radiances(b["co"], los, b["step_row"], b["tvib"], levels=[12], gas=1)
    with pytest.raises(RuntimeError):
        eng.limb_rays_parts(b["co"], los, b["part_gas"], b["part_level"], part_c=b["part_c"], tab=lf.tab, coef_row=b["step_row"], gas=0)


@pytest.mark.parametrize("grouped", [False, True])
def test_radtrans_returns_the_budget(eng, grouped):
    """E.  retrieval.radtrans(track_levels=track_all_levels(scene)) on a small two-gas LimbScene, with and without
    group_observations: sims equal radtrans(scene, pixels) within far_tol(1e-10) (the coefficient route differs); per
    line of sight the gases' spectra add up to radtrans[tag] and a gas's levels to the gas, to 1e-12 of the band maximum;
    the band integrals of two spectral shards add up to the whole grid's, radiances and every part, within
    far_tol(1e-12) max|whole|.  With default arguments radtrans returns what simulate(scene, pixels, None)[0] does, bit
    for bit.
    Measured on the MI355X (per pixel, 18 lines of sight / grouped, 15): sims against the default route 3.6e-16 / 5.6e-16,
    gases - radtrans 3.6e-16 / 4.2e-16, levels - gas 3.1e-16 / 3.1e-16, two shards against the whole grid 3.7e-16 / 3.7e-16;
    11 of the 12 CH4 levels reach 1e-3 of the band maximum on every line of sight."""
    import bench_configs as bc
    from spectrobot_amd import retrieval, spect_main_module as smm
    sc = bc.two_gas_scene(6000, 1500, 16000, 30)
    _, pixels, _ = bc.retrieval_problem(sc)
    kw = dict(group_observations=True, alt_step_sims=40.0) if grouped else {}
    group = (40.0, None) if grouped else None
    plain = retrieval.radtrans(sc, pixels, **kw)
    again = retrieval.simulate(sc, pixels, None, group=group)[0]
    assert all(np.array_equal(p.spectrum, q.spectrum) for p, q in zip(plain, again))
    tl = smm.track_all_levels(sc)
    assert tl == {("CH4", "iso_1"): ["lev_%02d" % i for i in range(12)], ("HCN", "iso_1"): ["lev_%02d" % i for i in range(6)]}
    sims, rt, single = retrieval.radtrans(sc, pixels, track_levels=tl, **kw)
    assert len(sims) == len(pixels)
    d_sims = max(float(np.max(np.abs(s.spectrum - p.spectrum)) / np.max(np.abs(p.spectrum))) for s, p in zip(sims, plain))
    tags = sorted(rt)
    n_los = len(tags)
    assert tags == retrieval.los_tags(n_los) and (grouped or n_los == 3 * len(pixels))
    assert len(single) == 2 + 12 + 6 and all(sorted(v) == tags for v in single.values())
    clo_gas = clo_lev = 0.0
    for tag in tags:
        top = np.max(np.abs(rt[tag].spectrum))
        tot = single[("CH4", "iso_1")][tag].spectrum + single[("HCN", "iso_1")][tag].spectrum
        clo_gas = max(clo_gas, float(np.max(np.abs(tot - rt[tag].spectrum)) / top))
        for name, n_lev in (("CH4", 12), ("HCN", 6)):
            lev = sum(single[(name, "iso_1", "lev_%02d" % i)][tag].spectrum for i in range(n_lev))
            clo_lev = max(clo_lev, float(np.max(np.abs(lev - single[(name, "iso_1")][tag].spectrum)) / top))
    seen = [sum(np.max(np.abs(single[("CH4", "iso_1", "lev_%02d" % i)][tag].spectrum)) >= 1e-3 * np.max(np.abs(rt[tag].spectrum))
                for i in range(12)) for tag in tags]
    # two spectral shards: without a process group the all-reduce is the identity, so each call returns its partial sums
    n = len(sc.grid)
    halves = [retrieval.radtrans(sc, pixels, track_levels=tl, shard=sh, **kw) for sh in ((0, n // 3), (n // 3, n))]
    d_shard = 0.0
    for tag in tags:
        whole = [rt[tag].spectrum] + [single[k][tag].spectrum for k in single]
        added = [halves[0][1][tag].spectrum + halves[1][1][tag].spectrum] + \
                [halves[0][2][k][tag].spectrum + halves[1][2][k][tag].spectrum for k in single]
        top = np.max(np.abs(rt[tag].spectrum))
        d_shard = max(d_shard, max(float(np.max(np.abs(w - s))) / top for w, s in zip(whole, added)))
    print("radtrans budget [%s]: %d lines of sight, sims vs the default route %.2e, gases - radtrans %.2e, levels - gas %.2e "
          "of the band maximum, two shards vs the whole grid %.2e, CH4 levels that reach 1e-3 of the band maximum per line "
          "of sight: %d..%d" % ("grouped" if grouped else "per pixel", n_los, d_sims, clo_gas, clo_lev, d_shard, min(seen), max(seen)))
    assert d_sims <= far_tol(1e-10)
    assert clo_gas <= 1e-12 and clo_lev <= 1e-12
    assert d_shard <= far_tol(1e-12)
    assert min(seen) >= 1
    # full_output without tracked levels: the gases alone, through the same call
    s2, rt2, single2 = retrieval.radtrans(sc, pixels, full_output=True, **kw)
    assert sorted(single2) == [("CH4", "iso_1"), ("HCN", "iso_1")]
    assert all(np.max(np.abs(rt2[t].spectrum - rt[t].spectrum)) <= far_tol(1e-10) * np.max(np.abs(rt[t].spectrum)) for t in tags)
