"""Parameter blocks per ray in the mixed-state pass (sr_set_state_ray_blocks), the part that needs no GPU: the library's
surface, and the per-ray plan (ray_jac_plan in spectrobot_amd/csrc/sr_limb_plan.hpp, reached through sr_state_ray_plan)
against a brute-force restatement in numpy on the batches of tests/state_rayblocks_cases.py."""
import numpy as np
import pytest

import state_rayblocks_cases as B


@pytest.fixture(scope="module")
def eng():
    from spectrobot_amd import engine
    return engine


def test_new_symbols(eng):
    """The switch, the two getters and the plan hook are exported and bound; the switch takes 0 and 1; no call yet on this
    thread: route 0.  (sr_abi_version() stays 1: every earlier extension left it there and the suite pins it.)"""
    from spectrobot_amd import _lib
    for name in ("sr_set_state_ray_blocks", "sr_last_state_route", "sr_last_state_walks", "sr_state_ray_plan"):
        assert name in _lib.SYMBOLS and hasattr(_lib.lib, name)
    assert _lib.lib.sr_set_state_ray_blocks(1) == _lib.SR_OK and _lib.lib.sr_set_state_ray_blocks(0) == _lib.SR_OK
    assert _lib.lib.sr_abi_version() == 1
    eng.set_state_ray_blocks(True)
    eng.set_state_ray_blocks(False)
    assert eng.last_state_route()[0] in (0, 1, 2)


def _los(eng, c, **opts):
    return eng.LimbLOS(c["seg_off"], c["seg_layer"], c["pt_off"], c["x"], c["nd"], c["vmr"], **opts)


def _plan(eng, c, n_hid=0, **opts):
    los = _los(eng, c, **opts)
    try:
        return eng.state_ray_plan(los, c["n_layers"], c["par_gas"][:c["n_col"]], c["par_w"][:c["n_col"]], c["par_level"][:c["n_lev"]],
                                  c["par_c"][:c["n_lev"]], c["par_t"][:c["n_row"]] if c["n_row"] else None,
                                  c["par_lgas"][:c["n_lev"]] if c["n_lgas"] > 1 else None, n_hid=n_hid)
    finally:
        los.close()


CASES = {
    "columns": lambda: (B.main_case(37, 0, 0), 0),
    "columns + levels": lambda: (B.main_case(27, 10, 0), 0),
    "all kinds": lambda: (B.main_case(21, 10, 6), 0),
    "two level gases": lambda: (B.main_case(21, 10, 6, n_lgas=2), 0),
    "hidden slots": lambda: (B.main_case(18, 10, 6), 3),
    "eight slots": lambda: (B.small_case(), 0),
    "row per step": lambda: (B.step_rows_case(), 0),
    "observer order": lambda: (B.main_case(21, 10, 6), 0, dict(LOS_order="observer")),
}


def test_main_batch_touch_counts():
    """The main batch is what the tests say it is: ray 0 touches nothing, ray 1 sixteen parameters, ray 2 seventeen, ray 3
    at most eight, rays 4 and 5 all three kinds; 37 parameters are three dense blocks; the walks fall from 18 to 7 (ray 2 alone needs two)."""
    for split in ((37, 0, 0), (27, 10, 0), (21, 10, 6)):
        c = B.main_case(*split)
        assert tuple(B.touches(c).sum(axis=1)) == B.TARGET == (0, 16, 17, 5, 13, 14)
        assert B.walks(c) == (16, 7, 18)
    c = B.main_case(21, 10, 6)
    T = B.touches(c)
    for ray in (4, 5):
        assert T[ray, :21].any() and T[ray, 21:31].any() and T[ray, 31:].any()
    assert not T[:, 20].any()            # a parameter that touches no ray
    s = B.small_case()
    assert B.touches(s).sum(axis=1).max() == 8 and B.walks(s) == (8, 6, 6)


@pytest.mark.parametrize("name", list(CASES))
def test_plan_against_the_restatement(eng, name):
    """Ray by ray: the union of its blocks is its touched set in the plan's order (so no parameter twice, the slot kinds in
    order: column slots -- blk's count --, level slots by (level gas, level), row slots); col_row names the dcol rows of
    the column slots and blk their gases; the entries of (ray block, row) are those of the block's level and row slots
    with a non-zero coefficient on that row, slot by slot, on the rows the ray crosses and none elsewhere; unused slots
    are -1; ray_blk_off is the prefix sum, n_blocks its largest step, np the rule."""
    got = CASES[name]()
    c, n_hid, opts = got[0], got[1], (got[2] if len(got) > 2 else {})
    P = _plan(eng, c, n_hid, **opts)
    n_col, n_lev, n_row, n_layers = c["n_col"], c["n_lev"], c["n_row"], c["n_layers"]
    n_state = n_col + n_lev + n_row
    lists = B.ray_lists(c, n_hid)
    n_p, n_walks, _ = B.walks(c, n_hid)
    assert P["np"] == n_p and int(P["ray_blk_off"][-1]) == n_walks == len(P["blk"])
    counts = np.diff(P["ray_blk_off"])
    assert P["ray_blk_off"][0] == 0 and counts.min() >= 1 and P["n_blocks"] == counts.max()
    word = lambda p: int(c["par_level"][p]) | (int(c["par_lgas"][p]) << 16 if c["n_lgas"] > 1 else 0)
    for ray, lst in enumerate(lists):
        b0, b1 = P["ray_blk_off"][ray], P["ray_blk_off"][ray + 1]
        assert b1 - b0 == max(1, -(-len(lst) // n_p))
        slots = P["slot_par"][b0:b1].reshape(-1)
        assert list(slots[:len(lst)]) == lst and np.all(slots[len(lst):] == -1)
        rows_on_ray = set(c["seg_layer"][c["seg_off"][ray]:c["seg_off"][ray + 1]].tolist())
        for rb in range(b0, b1):
            mine = lst[(rb - b0) * n_p:(rb - b0 + 1) * n_p]
            is_col = [p < n_col or p >= n_state for p in mine]
            nc = sum(is_col)
            assert P["blk"][rb, 0] == nc and all(is_col[:nc])           # the column slots come first
            for q in range(nc):
                p = mine[q]
                assert P["col_row"][rb, q] == (p if p < n_col else n_col + (p - n_state))
                assert (int(P["blk"][rb, 1]) >> (2 * q)) & 3 == (c["par_gas"][p] if p < n_col else p - n_state)
            assert int(P["blk"][rb, 1]) >> (2 * nc) == 0 and np.all(P["col_row"][rb, nc:] == 0)
            kinds = [0 if k else (1 if p < n_col + n_lev else 2) for p, k in zip(mine, is_col)]
            assert kinds == sorted(kinds)
            lev_words = [word(p - n_col) for p, k in zip(mine, kinds) if k == 1]
            assert lev_words == sorted(lev_words)
            for r in range(n_layers):
                e0, e1 = P["ent_off"][rb, r], P["ent_off"][rb, r + 1]
                want = []
                if r in rows_on_ray:
                    for q, (p, k) in enumerate(zip(mine, kinds)):
                        cc = c["par_c"][p - n_col, r] if k == 1 else c["par_t"][p - n_col - n_lev, r] if k == 2 else 0.0
                        if cc != 0.0:
                            want.append((q, word(p - n_col) if k == 1 else -2, cc))
                have = list(zip(P["ent_slot"][e0:e1].tolist(), P["ent_level"][e0:e1].tolist(), P["ent_c"][e0:e1].tolist()))
                assert have == want, (ray, rb, r)
    assert P["ent_off"][-1, -1] == len(P["ent_c"]) and np.all(np.diff(P["ent_off"].reshape(-1)) >= 0)


def test_plan_refusals(eng):
    """The hook checks its arguments as the state calls do: no sizes, a gas out of range, hidden slots out of range."""
    from spectrobot_amd import _lib
    import ctypes as C
    c = B.small_case()
    los = _los(eng, c)
    d = los.desc()
    sizes = np.zeros(4, np.int32)
    pg, pw = c["par_gas"].copy(), np.ascontiguousarray(c["par_w"])
    call = lambda n_hid, s, gases: _lib.lib.sr_state_ray_plan(
        C.byref(d), c["n_layers"], c["n_col"], gases.ctypes.data_as(_lib.ip), pw.ctypes.data_as(_lib.dp), 0, None, None, None, 0, None,
        n_hid, s, None, None, None, None, None, None, None, None)
    assert call(0, None, pg) == _lib.SR_ERR_ARG and call(5, sizes.ctypes.data_as(_lib.ip), pg) == _lib.SR_ERR_ARG
    bad = pg.copy()
    bad[0] = 3
    assert call(0, sizes.ctypes.data_as(_lib.ip), bad) == _lib.SR_ERR_ARG
    assert call(0, sizes.ctypes.data_as(_lib.ip), pg) == _lib.SR_OK and sizes[0] == 8
    los.close()


# ------------------------------------------------------------------------------------------------------------------
# the geometry helpers of the latitude-box driver
# ------------------------------------------------------------------------------------------------------------------
def _box_scene(n_box=3, n_nodes=5, n_pix=6):
    """The example's scene without its line sets: levels, densities, two gases, BoxPixels heading north across the box
    boundaries, and a LinearProfile_2D set with values of its own in every (box, node)."""
    import types
    from spectrobot_amd import retrieval, spect_main_module as smm, synthetic as syn
    atm = syn.make_atmosphere(40, 12)
    z = atm["z"]
    span = z[-1] - z[0]
    gases = [types.SimpleNamespace(name="HCN", vmr=np.full(40, 2e-6)), types.SimpleNamespace(name="CH4", vmr=np.full(40, 0.0148))]
    scene = types.SimpleNamespace(z=z, nd=syn.number_density(atm["press"], atm["temps"]), gases=gases, R=2575.0, n_sub=3)
    lat_limits = [-90.0] + list(36.0 / (n_box - 1) * np.arange(n_box - 1)) + [90.0]     # (the closing limit: a start without a mask)
    pixels = [retrieval.BoxPixel(z[0] + (0.08 + 0.8 * i / n_pix) * span, tangent_lat_deg=-4.0 + 12.0 * i / (n_pix - 1), heading_deg=0.0,
                                 fov_half=0.015 * span) for i in range(n_pix)]
    nodes = [z[0] + f * span for f in np.linspace(0.08, 0.9, n_nodes)]
    atmosphere = types.SimpleNamespace(grid=types.SimpleNamespace(coords={"alt": z}))
    st = smm.LinearProfile_2D("HCN", atmosphere, nodes, lat_limits, [np.full(n_nodes, 2e-6)] * (n_box + 1),
                             [np.full(n_nodes, 1e-6)] * (n_box + 1))
    rng = np.random.default_rng(3)
    for p in st.set:
        p.value = p.apriori * rng.uniform(0.5, 1.5)
    bs = smm.BayesSet()
    bs.add_set(st)
    return scene, pixels, bs, lat_limits


def test_box_weights_times_values_are_the_box_vmr():
    """geometry.box_profile_weights of a LinearProfile_2D set times its values equals geometry.box_vmr of set.profile() at
    every sample point, to rounding: both are a0 v[k] + a1 v[k + 1] of the step's box, one with the sum over the
    parameters inside, one outside -- n_par products and sums each way, so 2 n_par ulps of the largest term bound the
    difference (measured: below 2 ulps).  The rays cross box boundaries, every box is met, and a step's sample points share
    its box."""
    from spectrobot_amd import geometry, retrieval
    scene, pixels, bs, lat_limits = _box_scene()
    B = retrieval.box_batch(scene, bs, pixels)
    st = bs.sets["HCN"]
    seg_box = B.seg_box["HCN"]
    assert np.array_equal(seg_box, geometry.lat_box_of_segments(B.L3, st.lats))
    ref_box = np.clip(np.searchsorted(np.asarray(lat_limits), B.L3["seg_lat"], side="right") - 1, 0, len(lat_limits) - 1)
    assert np.array_equal(seg_box, ref_box) and set(seg_box.tolist()) == {0, 1, 2}
    per_ray = [len(set(seg_box[a:b].tolist())) for a, b in zip(B.L3["seg_off"][:-1], B.L3["seg_off"][1:])]
    assert min(per_ray) >= 2                          # every ray crosses a box boundary
    x = bs.param_vector()
    vmr = geometry.box_vmr(B.L3, scene.z, st.profile(), seg_box)
    W = B.par_w
    assert W.shape == (20, len(B.L3["alt"])) and not W[15:].any() and np.array_equal(B.vmr(scene, bs)[0], vmr)
    scale = np.abs(W * x[:, None]).sum(axis=0)
    err = np.abs(W.T @ x - vmr)
    print("\nbox weights x values against box_vmr: largest difference %.2f ulps of the terms' sum" % float((err / (scale * 2.0 ** -52)).max()))
    assert np.all(vmr > 0) and np.all(err <= 2 * 20 * 2.0 ** -53 * scale)
    # a profile that is the same in every box is the 1-D interpolation of limb_los
    flat = np.tile(np.linspace(1e-6, 3e-6, 40), (4, 1))
    zz = np.append(scene.z, scene.z[-1] + (scene.z[-1] - scene.z[-2]))
    assert np.allclose(geometry.box_vmr(B.L3, scene.z, flat, seg_box), np.interp(B.L3["alt"], zz, np.append(flat[0], flat[0][-1])),
                       rtol=1e-14, atol=0.0)


def test_touches_against_check_involved():
    """'Touches' (BoxBatch.touches: a non-zero weight at a sample point of one of the pixel's rays) against
    LinearProfile_2D.check_involved on the pixel's coordinate range (lowest altitude of its three paths, latitude range of
    their steps), for every (pixel, parameter).  check_involved is a bounding-box test -- altitude and latitude apart --
    so it may call a parameter involved that no sample point weights: the rays meet the parameter's box only at altitudes
    outside the node's triangle, below the node before it or above the node after it (this scene has such pairs by
    construction: a ray is low near its tangent point and high where it has run far north or south).  The other way
    round never happens: whatever touches is involved.  The closing limit's parameters are neither."""
    from spectrobot_amd import retrieval
    scene, pixels, bs, _ = _box_scene()
    B = retrieval.box_batch(scene, bs, pixels)
    st = bs.sets["HCN"]
    L3 = B.L3
    involved = np.zeros_like(B.touches)
    seen_by_alt_and_box = np.zeros_like(B.touches)
    for i in range(len(pixels)):
        s0, s1 = L3["seg_off"][3 * i], L3["seg_off"][3 * i + 3]
        p0, p1 = L3["pt_off"][s0], L3["pt_off"][s1]
        rng_ = dict(alt=(L3["alt"][p0:p1].min(), L3["alt"][p0:p1].max()), lat=(L3["seg_lat"][s0:s1].min(), L3["seg_lat"][s0:s1].max()))
        for ip, par in enumerate(st.set):
            involved[i, ip] = st.check_involved(par.key, rng_)
    both, only_involved, only_touches = (involved & B.touches).sum(), (involved & ~B.touches).sum(), (~involved & B.touches).sum()
    print("\ntouches against check_involved: %d pairs both, %d involved only, %d touches only, %d neither"
          % (both, only_involved, only_touches, (~involved & ~B.touches).sum()))
    assert only_touches == 0
    assert both > 0 and (~B.touches).sum() > 0 and B.touches.sum(axis=1).max() <= 16
    assert not involved[:, 15:].any() and not B.touches[:, 15:].any()
    # the pairs that are involved only: in every one the rays meet the parameter's box only outside the node's triangle
    for i, ip in zip(*np.nonzero(involved & ~B.touches)):
        box, node = divmod(ip, len(st.alts))
        s0, s1 = L3["seg_off"][3 * i], L3["seg_off"][3 * i + 3]
        in_box = np.repeat(B.seg_box["HCN"][s0:s1] == box, np.diff(L3["pt_off"][s0:s1 + 1]))
        alts_in_box = L3["alt"][L3["pt_off"][s0]:L3["pt_off"][s1]][in_box]
        lo = st.alts[node - 1] if node > 0 else -np.inf
        hi = st.alts[node + 1] if node + 1 < len(st.alts) else np.inf
        assert not np.any((alts_in_box > lo) & (alts_in_box < hi))
