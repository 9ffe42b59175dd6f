"""Every kernel of the limb radiance recursion and its Jacobians against the extended-precision CPU reference of
tests/limb_reference.py, on the regime panel (thin switch, range-reduction boundaries, the subnormal edge of exp,
saturated, exactly zero and negative optical depths, opaque middles) at small shapes.

The limit of every comparison is 8 x K_PLAIN units of  2^-53 (A + (n_gas + 1) C [+ F]) + 1e-290,  K_PLAIN being what
the plain fp64 recursion (limb_reference.plain_fp64) measures against the reference on the same inputs -- never what a
kernel gives.  F enters only where the call reaches sr_limb_adjoint_fold_kernel (sr_set_jac_layer_mode 0, shared
shells, more than 8 parameters or layer rows, and sr_limb_rays_jacobians_dev); every other route, the dense fold
included, is held to A and C alone.  Group A: the host-column calls, one gas, columns of 1, abs_c = tau exactly.
Group B: the device LOS pipeline on synthetic limb geometry; the reference takes the device's Curtis-Godson columns as
fp64 inputs.  Their own yardstick is tests/columns_reference.py: tests/test_gpu_columns_reference.py holds the columns
of every route, those of resident batches and the parameter-mask columns included, to curgod_fort_2 in long double.
Needs a real MI355X."""
import functools

import numpy as np
import pytest

import limb_reference as R

pytestmark = pytest.mark.gpu
SEED = 20261017


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


def _np(t):
    return t.detach().cpu().numpy()


class Tally(object):
    """The comparisons of one test: every figure is printed before anything is asserted.  K_PLAIN is taken on the
    panel columns the launch holds, for radiances and for Jacobians separately; each row is held to 8 x its own."""

    def __init__(self, names, cols, n_gas):
        self.names, self.cols, self.n_gas = names, cols, n_gas
        self.k_rad, self.k_jac, self.rows, self.info = 0.0, 0.0, [], []

    def plain(self, ref, f64, I0, solo):
        """K_PLAIN of these inputs: plain fp64 against the reference on the columns of the launch."""
        c = np.unique(self.cols)
        I, J = R.plain_fp64(*f64, I0, solo=solo)
        self.k_rad = max(self.k_rad, R.units(I[c], ref["I"][c], ref["A_I"][c], ref["C_I"][c], self.n_gas).max())
        if J.size:
            self.k_jac = max(self.k_jac, R.units(J[:, c], ref["J"][:, c], ref["A"][:, c], ref["C"][:, c], self.n_gas).max())

    def rad(self, tag, got, ref):
        c = self.cols
        self.rows.append((tag + " rad",) + R.worst(R.units(got, ref["I"][c], ref["A_I"][c], ref["C_I"][c], self.n_gas), self.names, c))

    def jac(self, tag, got, ref, use_F=False, rows=None, cancels=True):
        """use_F: the call is shaped to reach sr_limb_adjoint_fold_kernel.  cancels: emission takes part, so the fold's
        cancellation residues exist (absorption alone has none)."""
        c = self.cols
        pick = (lambda a: a[:, c]) if rows is None else (lambda a: a[rows][:, c])
        u = R.units(got, pick(ref["J"]), pick(ref["A"]), pick(ref["C"]), self.n_gas, pick(ref["F"]) if use_F else None)
        self.rows.append((tag + (" jac+F" if use_F else " jac"),) + R.worst(u, self.names, c))
        if use_F and cancels:      # what the fold measures against A and C alone: reported, and it pins the route (finish)
            self.info.append((tag + " jac, F left out",) + R.worst(R.units(got, pick(ref["J"]), pick(ref["A"]), pick(ref["C"]), self.n_gas),
                                                                   self.names, c))

    def finish(self):
        lim = {"rad": R.KERNEL_MARGIN * self.k_rad, "jac": R.KERNEL_MARGIN * self.k_jac}
        kind = lambda tag: "rad" if tag.endswith(" rad") else "jac"
        print("\nK_PLAIN rad %.3g jac %.3g  limits %.3g %.3g" % (self.k_rad, self.k_jac, lim["rad"], lim["jac"]))
        for tag, u, where in self.rows:
            print("  %-44s %10.3g units%s at %s" % (tag, u, "  OVER" if not u <= lim[kind(tag)] else "", where))
        info = _worst_per_tag(self.info)
        for tag, u, where in info:
            print("  (%s: %.3g units at %s)" % (tag, u, where))
        bad = [r for r in self.rows if not r[1] <= lim[kind(r[0])]]
        assert not bad, "over 8 x K_PLAIN (rad %.3g, jac %.3g units): %s" % (lim["rad"], lim["jac"], bad)
        # F is granted on a reading of the dispatch: where the fold ran, its residues behind opaque stretches stand far
        # above A and C (1e14 units); a call that fell back to another kernel would meet A and C and F would only loosen
        # its bound unseen
        if info:
            assert min(r[1] for r in info) > 1e3 * max(lim["jac"], 1.0), "F was granted, but these figures are not the fold's: %s" % (info,)


# ------------------------------------------------------------------------------------------------------------------
# Group A: exact regimes through the host-column calls
# ------------------------------------------------------------------------------------------------------------------
RAY_SEGS = (1, 2, 3, 5, 41)     # segments per ray of one launch; fewer than four leave the split kernel's stretches empty


@functools.lru_cache(maxsize=None)
def _panel_a(n_rows, repeat=1):
    pan = R.regime_panel(n_rows, np.random.default_rng(SEED), repeat=repeat)
    pan["E"] = R.emission_of(pan["tau"], pan["source"])
    return pan


def _host_rays():
    """Ray k crosses the first RAY_SEGS[k] rows of the 41-row panel, every segment on its own row with a column of 1."""
    seg_off = np.concatenate([[0], np.cumsum(RAY_SEGS)]).astype(np.int32)
    seg_layer = np.concatenate([np.arange(k) for k in RAY_SEGS]).astype(np.int32)
    return seg_off, seg_layer, np.ones(seg_layer.size)


@functools.lru_cache(maxsize=None)
def _ref_a(n_seg, with_I0, n_par):
    """Reference and plain-fp64 forms of the ray that crosses the first n_seg panel rows; parameter p scales the column
    of segment s by dcol[s, p] (seeded per (n_seg, n_par))."""
    pan = _panel_a(41)
    tau, E = pan["tau"][:n_seg], pan["E"][:n_seg]
    rng = np.random.default_rng([SEED, n_seg, n_par])
    dcol = rng.uniform(0.0, 1.0, (n_seg, n_par)) * (rng.random((n_seg, n_par)) < 0.8)
    dtau = np.array([tau * dcol[:, p][:, None] for p in range(n_par)]).reshape(n_par, n_seg, tau.shape[1])
    dE = np.array([E * dcol[:, p][:, None] for p in range(n_par)]).reshape(n_par, n_seg, tau.shape[1])
    dtau_l = np.array([tau.astype(R.LD) * dcol[:, p].astype(R.LD)[:, None] for p in range(n_par)]).reshape(n_par, n_seg, tau.shape[1])
    dE_l = np.array([E.astype(R.LD) * dcol[:, p].astype(R.LD)[:, None] for p in range(n_par)]).reshape(n_par, n_seg, tau.shape[1])
    I0 = pan["I0"] if with_I0 else np.zeros_like(pan["I0"])
    ref = R.recursion_reference(tau, E, dtau_l, dE_l, I0)
    return ref, (tau, E, dtau, dE), I0, dcol


@pytest.mark.parametrize("with_rad0", [False, True])
@pytest.mark.parametrize("n_pts", [1, 63, 65, 257])
def test_host_column_radiances(eng, n_pts, with_rad0):
    pan = _panel_a(41)
    cols = R.tile_columns(len(pan["names"]), n_pts, np.random.default_rng(SEED + n_pts))
    seg_off, seg_layer, seg_col = _host_rays()
    rad0 = _t(np.tile(pan["I0"][cols], (len(RAY_SEGS), 1))) if with_rad0 else None
    got = _np(eng.radiance_rays(_t(pan["tau"][:, cols]), _t(pan["E"][:, cols]), seg_off, seg_layer, seg_col, rad0=rad0))
    T = Tally(pan["names"], cols, 1)
    for r, k in enumerate(RAY_SEGS):
        ref, f64, I0, _ = _ref_a(k, with_rad0, 0)
        T.plain(ref, f64, I0, False)
        T.rad("radiance_rays %d seg" % k, got[r], ref)
    T.finish()


@pytest.mark.parametrize("n_pts", [1, 63, 65, 257])
@pytest.mark.parametrize("n_par", [1, 4, 5])
def test_host_column_jacobian(eng, n_par, n_pts):
    pan = _panel_a(41)
    cols = R.tile_columns(len(pan["names"]), n_pts, np.random.default_rng(SEED + n_pts))
    seg_off, seg_layer, seg_col = _host_rays()
    refs = [_ref_a(k, False, n_par) for k in RAY_SEGS]
    dcol = np.concatenate([r[3] for r in refs], axis=0)
    rad, jac = eng.radiance_jacobian(_t(pan["tau"][:, cols]), _t(pan["E"][:, cols]), seg_off, seg_layer, seg_col, dcol)
    rad, jac = _np(rad), _np(jac)
    T = Tally(pan["names"], cols, 1)
    for r, k in enumerate(RAY_SEGS):
        ref, f64, I0, _ = refs[r]
        T.plain(ref, f64, I0, False)
        T.rad("radiance_jacobian %d seg" % k, rad[r], ref)
        T.jac("radiance_jacobian %d seg" % k, jac[r], ref)
    T.finish()


@functools.lru_cache(maxsize=None)
def _layer_case(n_layers, absorption_only):
    """Limb-like rays down to row 0 and up again (and one that turns at row 1, one of a single segment), the panel on
    n_layers rows, one parameter per row acting through the row's own coefficients; references per ray."""
    pan = _panel_a(n_layers, repeat=2)
    N = len(pan["names"])
    rng = np.random.default_rng([SEED, n_layers])
    dabs = pan["tau"] * rng.uniform(-1.0, 1.0, pan["tau"].shape)
    demi = pan["E"] * rng.uniform(-1.0, 1.0, pan["E"].shape) * (0.0 if absorption_only else 1.0)
    down = np.arange(n_layers - 1, -1, -1)
    rays = [np.concatenate([down, down[::-1][1:]]), np.concatenate([down[:-1], down[:-1][::-1]]), down[:1]]
    refs = []
    for lay in rays:
        tau, E = pan["tau"][lay], pan["E"][lay]
        hit = (lay[None, :] == np.arange(n_layers)[:, None])[:, :, None]        # [row, segment]
        f64 = (tau, E, np.where(hit, dabs[lay][None], 0.0), np.where(hit, demi[lay][None], 0.0))
        refs.append((R.recursion_reference(*f64, np.zeros(N)), f64))
    return pan, dabs, demi, rays, refs


@pytest.mark.parametrize("n_pts", [1, 63, 65, 257])
@pytest.mark.parametrize("absorption_only", [False, True])
@pytest.mark.parametrize("n_layers", [3, 9])
def test_host_layer_jacobian(eng, n_layers, absorption_only, n_pts):
    """sr_radiance_jac_layer_kernel.  absorption_only: demi = 0, so dE = 0 and, the rays starting from I = 0, a thin
    path's entries are E f' dtau and I_prev t dtau alone: f' between 1e-12 and 1e-4 on its own.  The closed form
    (tau t - (1 - t)) / tau^2 is a difference of nearly equal numbers there, good to ~2^-53 / tau of f', in
    atten_fprime() as in plain_fp64: K_PLAIN of these cases is what that costs in units of the bound."""
    pan, dabs, demi, rays, refs = _layer_case(n_layers, absorption_only)
    N = len(pan["names"])
    cols = R.tile_columns(N, n_pts, np.random.default_rng(SEED + n_layers + n_pts))
    seg_off = np.concatenate([[0], np.cumsum([len(r) for r in rays])]).astype(np.int32)
    seg_layer = np.concatenate(rays).astype(np.int32)
    got = _np(eng.radiance_layer_jacobian(_t(pan["tau"][:, cols]), _t(pan["E"][:, cols]), _t(dabs[:, cols]), _t(demi[:, cols]),
                                          seg_off, seg_layer, np.ones(seg_layer.size)))
    T = Tally(pan["names"], cols, 1)
    for r, lay in enumerate(rays):
        ref, f64 = refs[r]
        T.plain(ref, f64, np.zeros(N), False)
        T.jac("radiance_layer_jacobian ray %d (%d seg)" % (r, len(lay)), got[r], ref)
    T.finish()


# ------------------------------------------------------------------------------------------------------------------
# Group B: the device LOS pipeline
# ------------------------------------------------------------------------------------------------------------------
def _z_tans(z, n_rays):
    top = z[-1] + (z[-1] - z[-2])
    if n_rays == 1:
        return [z[0] + 5.0]
    if n_rays == 3:
        return [z[0] + 5.0, z[len(z) // 3] + 3.0, 0.5 * (z[-1] + top)]
    zt = np.linspace(z[0] + 2.0, z[-1] - 1.0, n_rays)      # ray 0 through the lowest layer
    zt[7] = zt[6]                                           # a repeated height
    zt[-1] = top - 0.05                                     # grazing the top shell
    return list(zt)


@functools.lru_cache(maxsize=None)
def _scene(n_layers, n_rays, n_gas, order="photon"):
    """Geometry, device columns and panel coefficients: abs_c[g][layer][j] = share_g target[layer][j] / u_far(layer,
    ray 0): ray 0's far-side segment of every layer meets the panel's optical depth (to rounding), every other segment a
    multiple of it."""
    from spectrobot_amd import engine, synthetic as syn
    atm = syn.make_atmosphere(n_layers, 1)
    z = atm["z"]
    nd = syn.number_density(atm["press"], atm["temps"])
    vm = [np.full(n_layers, 1.2e-2), np.linspace(2e-3, 5e-4, n_layers), 3e-4 * (1 + 0.3 * np.sin(z / 90.0)),
          np.linspace(1e-5, 4e-5, n_layers)][:n_gas]
    scale = [0.98827, 1.0, 0.5, 1.0][:n_gas]
    L = syn.limb_los(z, nd, vm, _z_tans(z, n_rays))
    los = engine.LimbLOS(L["seg_off"], L["seg_layer"], L["pt_off"], L["x"], L["nd"], L["vmr"], col_scale=scale, LOS_order=order)
    col = los.columns()
    los.close()
    rng = np.random.default_rng([SEED, n_layers, n_gas])
    pan = R.regime_panel(n_layers, rng, repeat=2)
    u_far = np.zeros((n_gas, n_layers))
    s0, s1 = int(L["seg_off"][0]), int(L["seg_off"][1])
    for s in range(s1 - 1, s0 - 1, -1):                      # (the first crossing of a layer wins)
        u_far[:, L["seg_layer"][s]] = col[:, s]
    assert np.all(u_far > 0), "ray 0 must cross every layer"
    share = rng.uniform(0.2, 1.0, n_gas)
    share /= share.sum()
    E = R.emission_of(pan["tau"], pan["source"])
    abs_c = share[:, None, None] * pan["tau"][None] / u_far[:, :, None]
    emi_c = share[:, None, None] * E[None] / u_far[:, :, None]
    return dict(z=z, L=L, col=col, scale=scale, names=pan["names"], I0=pan["I0"], abs_c=abs_c, emi_c=emi_c)


def _los(eng, sc, **opts):
    L = sc["L"]
    return eng.LimbLOS(L["seg_off"], L["seg_layer"], L["pt_off"], L["x"], L["nd"], L["vmr"], col_scale=sc["scale"], **opts)


def _segments(sc, r, order="photon"):
    a, b = int(sc["L"]["seg_off"][r]), int(sc["L"]["seg_off"][r + 1])
    s = np.arange(a, b)
    return s if order == "photon" else s[::-1]        # observer order: listed from the observer, walked backwards


def _mask_columns(eng, sc, par_gas, W, order="photon"):
    """d col / d x_p per segment: the Curtis-Godson column of the parameter's mask times the gas's col_scale."""
    L = sc["L"]
    out = []
    for p0 in range(0, len(W), 4):           # (a LOS carries at most four gases)
        Wb = W[p0:p0 + 4]
        m = eng.LimbLOS(L["seg_off"], L["seg_layer"], L["pt_off"], L["x"], L["nd"], Wb,
                        col_scale=[sc["scale"][g] for g in par_gas[p0:p0 + 4]], LOS_order=order)
        out.append(m.columns())
        m.close()
    return np.concatenate(out, axis=0)


def _box_masks(sc, n_par, n_gas):
    """Parameter p: the VMR of gas p % n_gas inside layer p // n_gas (a segment touches one parameter per gas)."""
    L = sc["L"]
    pt_layer = np.repeat(L["seg_layer"], np.diff(L["pt_off"]))
    return (np.arange(n_par) % n_gas).astype(np.int32), np.array([(pt_layer == p // n_gas) * 1.0 for p in range(n_par)])


def _broad_masks(sc, n_par, n_gas):
    """Every parameter acts on the whole path (more than four per segment)."""
    L, z = sc["L"], sc["z"]
    W = np.array([np.exp(-0.5 * ((L["alt"] - z[(3 * p) % len(z)]) / 250.0) ** 2) for p in range(n_par)])
    return (np.arange(n_par) % n_gas).astype(np.int32), W


def _ray_forms(sc, segs, dtype, par_gas=None, dcol=None, dco=None, rows=None, n_rows=0, level=None):
    """tau, E, dtau, dE of one ray in `dtype`.  Parameters, in this order: column parameters (par_gas, dcol), one per
    Jacobian row (dco = (dabs, demi) [G, n_layers, N]; rows[s]: the row a segment's sensitivity goes to), level
    parameters (level = (gas, tabA, tabE [n_lev_par, n_layers, N], par_c [n_lev_par, n_layers]))."""
    lay = sc["L"]["seg_layer"][segs]
    col = sc["col"][:, segs]
    ca, ce = sc["abs_c"][:, lay], sc["emi_c"][:, lay]
    tau, E = R.products(ca, col, dtype), R.products(ce, col, dtype)
    dtau, dE = [], []
    if par_gas is not None:
        _, _, a, b = R.forms(ca, ce, col, par_gas, dcol[:, segs], dtype)
        dtau += list(a)
        dE += list(b)
    if dco is not None:
        da, de = R.products(dco[0][:, lay], col, dtype), R.products(dco[1][:, lay], col, dtype)
        hit = (rows[segs][None, :] == np.arange(n_rows)[:, None])[:, :, None]
        dtau += list(np.where(hit, da[None], dtype(0)))
        dE += list(np.where(hit, de[None], dtype(0)))
    if level is not None:
        gas, tabA, tabE, par_c = level
        w = np.asarray(par_c[:, lay], dtype) * np.asarray(col[gas], dtype)[None, :]
        dtau += list(w[:, :, None] * np.asarray(tabA[:, lay], dtype))
        dE += list(w[:, :, None] * np.asarray(tabE[:, lay], dtype))
    N = tau.shape[1]
    P = len(dtau)
    return tau, E, np.array(dtau, dtype).reshape(P, len(segs), N), np.array(dE, dtype).reshape(P, len(segs), N)


def _ray_refs(sc, n_gas, I0, solo=False, order="photon", tally=None, **par):
    """The reference of every ray of the scene (and K_PLAIN of these inputs into the tally)."""
    refs = []
    for r in range(len(sc["L"]["seg_off"]) - 1):
        segs = _segments(sc, r, order)
        ref = R.recursion_reference(*_ray_forms(sc, segs, R.LD, **par), I0, solo=solo, thin_ulps=n_gas + 1)
        if tally is not None:
            tally.plain(ref, _ray_forms(sc, segs, np.float64, **par), I0, solo)
        refs.append(ref)
    return refs


def _coeffs(sc, cols, rows=None):
    a, e = sc["abs_c"][:, :, cols], sc["emi_c"][:, :, cols]
    if rows is not None:
        a, e = a[:, rows], e[:, rows]
    return _t(a), _t(e)


def _planck(eng, sc, los, n_pts, grid, n_layers):
    """The Planck initial intensity as the device forms it: the radiance of the batch through empty coefficients
    (tau = 0 exactly: I0 passes unchanged).  An input of these tests, not their subject."""
    import torch
    zero = torch.zeros((los.n_gas, n_layers, n_pts), dtype=torch.float64, device="cuda")
    return _np(eng.limb_rays((zero, zero), los, grid=grid, resident=False))[0]


LIMB_RAYS_CASES = {
    "split 3 rays 2 gases":        dict(n_layers=12, n_rays=3, n_gas=2, n_pts=300, route=1),
    "split 1 ray 4 gases 30 lay":  dict(n_layers=30, n_rays=1, n_gas=4, n_pts=300, route=1),
    "split rad0":                  dict(n_layers=12, n_rays=3, n_gas=1, n_pts=300, rad0=True, route=1),
    "split observer":              dict(n_layers=12, n_rays=3, n_gas=2, n_pts=300, order="observer", route=1),
    "split solo planck":           dict(n_layers=12, n_rays=3, n_gas=2, n_pts=300, solo=True, planck=250.0, route=1),
    "split planck":                dict(n_layers=12, n_rays=3, n_gas=2, n_pts=300, planck=180.0, route=1),
    "folded 33 rays 3 gases":      dict(n_layers=12, n_rays=33, n_gas=3, n_pts=4100, route=2),
    "folded rad0":                 dict(n_layers=12, n_rays=33, n_gas=2, n_pts=4100, route=2, rad0=True),
    "path order row per step":     dict(n_layers=12, n_rays=33, n_gas=2, n_pts=4100, route=1, per_step=True),
}


@pytest.mark.parametrize("case", list(LIMB_RAYS_CASES))
def test_limb_rays(eng, case):
    """sr_limb_split_kernel (small launches), sr_limb_kernel (a coefficient row per step) and the folded forward sweep
    (ceil(n_pts / 64) n_rays >= 2048 on shared shells), each through the resident batch and staged per call."""
    from spectrobot_amd import synthetic as syn
    c = dict(order="photon", solo=False, planck=None, rad0=False, route=None, per_step=False)
    c.update(LIMB_RAYS_CASES[case])
    sc = _scene(c["n_layers"], c["n_rays"], c["n_gas"], c["order"])
    N = len(sc["names"])
    cols = R.tile_columns(N, c["n_pts"], np.random.default_rng(SEED + c["n_pts"]))
    L = sc["L"]
    grid = syn.make_grid(2975.0, 5e-4, c["n_pts"]) if c["planck"] else None
    opts = dict(LOS_order=c["order"], solo_absorption=c["solo"], initial_temperature=c["planck"])
    rows = None
    if c["per_step"]:
        rows = L["seg_layer"]
        los = eng.LimbLOS(L["seg_off"], np.arange(len(rows)), L["pt_off"], L["x"], L["nd"], L["vmr"], col_scale=sc["scale"], **opts)
    else:
        los = _los(eng, sc, **opts)
    coeffs = _coeffs(sc, cols, rows)
    n_rows = coeffs[0].shape[1]
    T = Tally(sc["names"], cols, c["n_gas"])
    I0 = sc["I0"] if c["rad0"] else np.zeros(N)
    if c["planck"]:
        # one Planck value per point of the launch: the reference runs on the launch's own columns
        bb = _planck(eng, sc, los, c["n_pts"], grid, n_rows)
        assert c["n_pts"] >= N and np.all(bb > 0)
        I0 = bb[:N]            # (the first tile is the panel in its own order)
        T.cols = cols = cols[:N]
    refs = _ray_refs(sc, c["n_gas"], I0, solo=c["solo"], order=c["order"], tally=T)
    try:
        for resident in (True, False):
            rad0 = _t(np.tile(sc["I0"][cols], (c["n_rays"], 1))) if c["rad0"] else None
            got = _np(eng.limb_rays(coeffs, los, grid=grid, rad0=rad0, resident=resident))
            route = eng.last_limb_route()
            if c["route"] is not None:
                assert route == c["route"], "route %d, shaped for %d" % (route, c["route"])
            for r in range(c["n_rays"]):
                T.rad("limb_rays %s route %d ray %d" % ("resident" if resident else "staged", route, r), got[r][:len(cols)], refs[r])
    finally:
        los.close()
    T.rows = _worst_per_tag(T.rows)
    T.finish()


def _worst_per_tag(rows):
    """One line per kernel route: the worst ray of each (the tag up to ' ray ')."""
    best = {}
    for tag, u, where in rows:
        key = tag.split(" ray ")[0] + (" " + tag.rsplit(" ", 1)[1] if " ray " in tag else "")
        if key not in best or not u <= best[key][1]:
            best[key] = (tag, u, where)
    return list(best.values())


JAC_CASES = [(1, "broad"), (4, "broad"), (5, "broad"), (8, "broad"), (9, "box"), (16, "box"), (17, "box"), (33, "box")]


JAC_OPTIONS = [dict(), dict(LOS_order="observer"), dict(solo_absorption=True, initial_temperature=250.0), dict(rad0=True)]


@pytest.mark.parametrize("n_par,kind", JAC_CASES)
def test_limb_rays_jacobian(eng, n_par, kind):
    """sr_limb_rays_jac_dev: the dense fold (<= 8 parameters, mode 0), the adjoint fold (> 8, mode 0: F), the adjoint
    kernels in path order (modes 2 and 3) and the forward sensitivities (mode 1: NP 4 and 16); observer order, absorption
    alone of a Planck source and a given initial intensity on the 4- and the 9-parameter case."""
    from spectrobot_amd import synthetic as syn
    n_gas = 3
    sc = _scene(12, 3, n_gas)
    N = len(sc["names"])
    cols = R.tile_columns(N, 300, np.random.default_rng(SEED + 300))
    par_gas, W = (_broad_masks if kind == "broad" else _box_masks)(sc, n_par, n_gas)
    dcol = _mask_columns(eng, sc, par_gas, W)
    T = Tally(sc["names"], cols, n_gas)
    coeffs = _coeffs(sc, cols)
    grid = syn.make_grid(2975.0, 5e-4, 300)
    try:
        for o in (JAC_OPTIONS if n_par in (4, 9) else JAC_OPTIONS[:1]):
            opts = {k: v for k, v in o.items() if k != "rad0"}
            order, solo, planck = opts.get("LOS_order", "photon"), opts.get("solo_absorption", False), "initial_temperature" in opts
            los = _los(eng, sc, **opts)
            use_cols, I0 = cols, (sc["I0"] if o.get("rad0") else np.zeros(N))
            if planck:
                use_cols, I0 = cols[:N], _planck(eng, sc, los, 300, grid, 12)[:N]
            T.cols = use_cols
            refs = _ray_refs(sc, n_gas, I0, solo=solo, order=order, tally=T, par_gas=par_gas, dcol=dcol)
            for mode in (0, 1, 2, 3):
                eng.set_jac_layer_mode(mode)
                for resident in ((False, True) if mode == 0 else (False,)):
                    rad0 = _t(np.tile(sc["I0"][cols], (3, 1))) if o.get("rad0") else None
                    rad, jac = eng.limb_rays_jacobian(coeffs, los, par_gas, W, grid=grid if planck else None, rad0=rad0,
                                                      resident=resident)
                    rad, jac = _np(rad), _np(jac)
                    tag = "limb_rays_jacobian n_par %d mode %d%s %s" % (n_par, mode, " resident" if resident else "",
                                                                        ",".join(sorted(o)) or "-")
                    fold = mode == 0 and n_par > 8 and not resident
                    for r in range(3):
                        T.rad(tag + " ray %d" % r, rad[r][:len(use_cols)], refs[r])
                        T.jac(tag + " ray %d" % r, jac[r][:, :len(use_cols)], refs[r], use_F=fold, cancels=not solo)
            los.close()
    finally:
        eng.set_jac_layer_mode(0)
    T.rows = _worst_per_tag(T.rows)
    T.finish()


def test_limb_rays_jacobian_large_launch(eng):
    """The dense fold and the forward sensitivities on 33 rays x 4100 points, the panel tiled by permutations."""
    n_gas, n_par = 2, 4
    sc = _scene(12, 33, n_gas)
    N = len(sc["names"])
    cols = R.tile_columns(N, 4100, np.random.default_rng(SEED + 4100))
    par_gas, W = _broad_masks(sc, n_par, n_gas)
    dcol = _mask_columns(eng, sc, par_gas, W)
    T = Tally(sc["names"], cols, n_gas)
    refs = _ray_refs(sc, n_gas, np.zeros(N), tally=T, par_gas=par_gas, dcol=dcol)
    coeffs = _coeffs(sc, cols)
    los = _los(eng, sc)
    try:
        for mode in (0, 1):
            eng.set_jac_layer_mode(mode)
            rad, jac = eng.limb_rays_jacobian(coeffs, los, par_gas, W)
            rad, jac = _np(rad), _np(jac)
            for r in range(33):
                T.rad("limb_rays_jacobian 33x4100 mode %d ray %d" % (mode, r), rad[r], refs[r])
                T.jac("limb_rays_jacobian 33x4100 mode %d ray %d" % (mode, r), jac[r], refs[r])
    finally:
        eng.set_jac_layer_mode(0)
        los.close()
    T.rows = _worst_per_tag(T.rows)
    T.finish()


@pytest.mark.parametrize("n_gas,n_layers", [(1, 12), (4, 30)])
def test_limb_rays_jacobian_one_and_four_gases(eng, n_gas, n_layers):
    """The kernels' other gas counts, and the 30-layer atmosphere (60 segments on one ray): 4 broad parameters (dense
    fold, forward NP 4) and 9 layer boxes (adjoint fold with F, forward NP 16, path-order adjoint)."""
    sc = _scene(n_layers, 1, n_gas)
    N = len(sc["names"])
    cols = R.tile_columns(N, 300, np.random.default_rng(SEED + 300))
    coeffs = _coeffs(sc, cols)
    T = Tally(sc["names"], cols, n_gas)
    los = _los(eng, sc)
    try:
        for n_par, masks in ((4, _broad_masks), (9, _box_masks)):
            par_gas, W = masks(sc, n_par, n_gas)
            dcol = _mask_columns(eng, sc, par_gas, W)
            refs = _ray_refs(sc, n_gas, np.zeros(N), tally=T, par_gas=par_gas, dcol=dcol)
            for mode in (0, 1, 2):
                eng.set_jac_layer_mode(mode)
                rad, jac = eng.limb_rays_jacobian(coeffs, los, par_gas, W)
                tag = "limb_rays_jacobian %d gases %d layers n_par %d mode %d" % (n_gas, n_layers, n_par, mode)
                T.rad(tag, _np(rad)[0], refs[0])
                T.jac(tag, _np(jac)[0], refs[0], use_F=(mode == 0 and n_par > 8))
    finally:
        eng.set_jac_layer_mode(0)
        los.close()
    T.finish()


def _dcoeffs(sc, rng):
    return (sc["abs_c"] * rng.uniform(-1.0, 1.0, sc["abs_c"].shape), sc["emi_c"] * rng.uniform(-1.0, 1.0, sc["emi_c"].shape))


@pytest.mark.parametrize("n_layers", [8, 12])
def test_limb_rays_layer_jacobian(eng, n_layers):
    """sr_limb_rays_jac_layer_dev: 8 layers stay on the forward kernel, 12 take the adjoint fold in mode 0 (F); the
    options on the 12-layer case."""
    from spectrobot_amd import synthetic as syn
    n_gas = 2
    sc = _scene(n_layers, 3, n_gas)
    N = len(sc["names"])
    cols = R.tile_columns(N, 300, np.random.default_rng(SEED + 300))
    dco = _dcoeffs(sc, np.random.default_rng([SEED, n_layers, 7]))
    coeffs = _coeffs(sc, cols)
    dcoeffs = (_t(dco[0][:, :, cols]), _t(dco[1][:, :, cols]))
    grid = syn.make_grid(2975.0, 5e-4, 300)
    T = Tally(sc["names"], cols, n_gas)
    option_sets = [dict()] + ([dict(LOS_order="observer"), dict(solo_absorption=True, initial_temperature=250.0)] if n_layers == 12 else [])
    try:
        for opts in option_sets:
            order, solo = opts.get("LOS_order", "photon"), opts.get("solo_absorption", False)
            los = _los(eng, sc, **opts)
            use_cols, I0 = cols, np.zeros(N)
            if "initial_temperature" in opts:
                I0, use_cols = _planck(eng, sc, los, 300, grid, n_layers)[:N], cols[:N]
            T.cols = use_cols
            refs = _ray_refs(sc, n_gas, I0, solo=solo, order=order, tally=T, dco=dco, rows=sc["L"]["seg_layer"], n_rows=n_layers)
            for mode in (0, 1, 2):
                eng.set_jac_layer_mode(mode)
                jac = _np(eng.limb_rays_layer_jacobian(coeffs, dcoeffs, los, grid=grid if "initial_temperature" in opts else None))
                tag = "limb_rays_layer_jacobian %d layers mode %d %s" % (n_layers, mode, ",".join(sorted(opts)) or "-")
                for r in range(3):
                    T.jac(tag + " ray %d" % r, jac[r][:, :len(use_cols)], refs[r], use_F=(mode == 0 and n_layers > 8), cancels=not solo)
            los.close()
    finally:
        eng.set_jac_layer_mode(0)
    T.rows = _worst_per_tag(T.rows)
    T.finish()


@pytest.mark.parametrize("mapped", [False, True])
def test_limb_rays_jacobians_all_modes(eng, mapped):
    """sr_limb_rays_jacobians_dev, radiances + per-layer + column-parameter Jacobians in one pass, under modes 0 to 3;
    mapped: a coefficient row per LOS step with a seg_jac_row map back to the layers -- the fold again in mode 0 (its
    shells are then the Jacobian rows), path order in modes 2 and 3; the forward kernels (mode 1) refuse the map.
    Every mode sweep also in observer order and as absorption alone of a Planck source."""
    from spectrobot_amd import synthetic as syn
    n_gas, n_layers, n_par = 2, 12, 10
    sc = _scene(n_layers, 3, n_gas)
    N = len(sc["names"])
    L = sc["L"]
    cols = R.tile_columns(N, 300, np.random.default_rng(SEED + 300))
    dco = _dcoeffs(sc, np.random.default_rng([SEED, n_layers, 9]))
    par_gas, W = _box_masks(sc, n_par, n_gas)
    dcol = _mask_columns(eng, sc, par_gas, W)
    T = Tally(sc["names"], cols, n_gas)
    rows = L["seg_layer"] if mapped else None
    coeffs = _coeffs(sc, cols, rows)
    dcoeffs = (_t(dco[0][:, :, cols] if rows is None else dco[0][:, rows][:, :, cols]),
               _t(dco[1][:, :, cols] if rows is None else dco[1][:, rows][:, :, cols]))
    grid = syn.make_grid(2975.0, 5e-4, 300)
    kw = dict(seg_jac_row=L["seg_layer"], n_jac_rows=n_layers) if mapped else {}
    try:
        for opts in (dict(), dict(LOS_order="observer"), dict(solo_absorption=True, initial_temperature=250.0)):
            order, solo, planck = opts.get("LOS_order", "photon"), opts.get("solo_absorption", False), "initial_temperature" in opts
            if mapped:
                los = eng.LimbLOS(L["seg_off"], np.arange(len(rows)), L["pt_off"], L["x"], L["nd"], L["vmr"], col_scale=sc["scale"], **opts)
            else:
                los = _los(eng, sc, **opts)
            use_cols, I0 = cols, np.zeros(N)
            if planck:
                use_cols, I0 = cols[:N], _planck(eng, sc, los, 300, grid, coeffs[0].shape[1])[:N]
            T.cols = use_cols
            refs = _ray_refs(sc, n_gas, I0, solo=solo, order=order, tally=T, par_gas=par_gas, dcol=dcol, dco=dco,
                             rows=L["seg_layer"], n_rows=n_layers)
            for mode in ((0, 2, 3) if mapped else (0, 1, 2, 3)):    # (rows other than the coefficient rows: the one-pass kernels only)
                eng.set_jac_layer_mode(mode)
                rad, jl, jp = eng.limb_rays_jacobians(coeffs, los, dcoeffs=dcoeffs, par_gas=par_gas, par_w=W,
                                                      grid=grid if planck else None, **kw)
                rad, jl, jp = _np(rad), _np(jl), _np(jp)
                fold = mode == 0      # (mapped too: limb paths walk their Jacobian rows monotonically, the shells of the fold)
                tag = "limb_rays_jacobians%s mode %d %s" % (" mapped" if mapped else "", mode, ",".join(sorted(opts)) or "-")
                n = len(use_cols)
                for r in range(3):
                    T.rad(tag + " ray %d" % r, rad[r][:n], refs[r])
                    T.jac(tag + " par ray %d" % r, jp[r][:, :n], refs[r], use_F=fold, rows=slice(0, n_par), cancels=not solo)
                    T.jac(tag + " layer ray %d" % r, jl[r][:, :n], refs[r], use_F=fold, rows=slice(n_par, n_par + n_layers), cancels=not solo)
            los.close()
    finally:
        eng.set_jac_layer_mode(0)
    T.rows = _worst_per_tag(T.rows)
    T.finish()


def _tables(sc, gas, n_levels, rng):
    """Pair tables of the level-factored gas on the panel columns: level L holds a random share of the gas's own
    coefficients on a permuted table row (coef_row undoes the permutation), so that dtau follows tau into every regime."""
    n_layers = sc["abs_c"].shape[1]
    coef_row = rng.permutation(n_layers).astype(np.int32)
    tab = np.zeros((n_levels, 2, n_layers, sc["abs_c"].shape[2]))
    w = rng.uniform(0.2, 1.0, (n_levels, 2, n_layers, 1))
    tab[:, 0, coef_row] = w[:, 0] * sc["abs_c"][gas][None]
    tab[:, 1, coef_row] = w[:, 1] * sc["emi_c"][gas][None]
    return tab, coef_row


@pytest.mark.parametrize("n_lev,n_col", [(8, 0), (9, 0), (16, 0), (17, 0), (5, 3), (6, 3), (12, 5), (5, 0)])
def test_limb_rays_level_and_state_jacobian(eng, n_lev, n_col):
    """sr_limb_jac_state_kernel<NG, 8 | 16> through the level call (n_col = 0) and the state call, parameter counts on
    both sides of the block sizes 8 and 16; the last case carries the options."""
    from spectrobot_amd import synthetic as syn
    n_gas, n_layers, gas, n_levels = 2, 12, 1, 4
    sc = _scene(n_layers, 3, n_gas)
    N = len(sc["names"])
    cols = R.tile_columns(N, 300, np.random.default_rng(SEED + 300))
    rng = np.random.default_rng([SEED, n_lev, n_col])
    tab, coef_row = _tables(sc, gas, n_levels, rng)
    par_level = rng.integers(0, n_levels, n_lev).astype(np.int32)
    par_c = rng.uniform(-1.0, 1.0, (n_lev, n_layers)) * (rng.random((n_lev, n_layers)) < 0.7)
    level = (gas, tab[par_level, 0][:, coef_row], tab[par_level, 1][:, coef_row], par_c)
    par_gas = W = dcol = None
    if n_col:
        par_gas, W = _broad_masks(sc, n_col, n_gas)
        dcol = _mask_columns(eng, sc, par_gas, W)
    coeffs = _coeffs(sc, cols)
    tab_d = _t(tab[:, :, :, cols])
    grid = syn.make_grid(2975.0, 5e-4, 300)
    T = Tally(sc["names"], cols, n_gas)
    options = [dict()] + ([dict(LOS_order="observer"), dict(solo_absorption=True, initial_temperature=250.0),
                           dict(initial_temperature=180.0)] if (n_lev, n_col) == (5, 0) else [])
    for opts in options:
        order, solo = opts.get("LOS_order", "photon"), opts.get("solo_absorption", False)
        los = _los(eng, sc, **opts)
        try:
            planck = "initial_temperature" in opts
            use_cols, I0 = (cols[:N], _planck(eng, sc, los, 300, grid, n_layers)[:N]) if planck else (cols, np.zeros(N))
            T.cols = use_cols
            refs = _ray_refs(sc, n_gas, I0, solo=solo, order=order, tally=T, par_gas=par_gas, dcol=dcol, level=level)
            g = grid if planck else None
            calls = [("state", lambda: eng.limb_rays_state_jacobian(coeffs, los, par_gas, W, tab_d, coef_row, par_level, par_c, gas=gas, grid=g))]
            if not n_col:
                calls.append(("level", lambda: eng.limb_rays_level_jacobian(coeffs, los, tab_d, coef_row, par_level, par_c, gas=gas, grid=g)))
            for name, call in calls:
                rad, jac = call()
                rad, jac = _np(rad), _np(jac)
                tag = "%s jacobian %d col + %d lev %s" % (name, n_col, n_lev, ",".join(sorted(opts)) or "-")
                for r in range(3):
                    T.rad(tag + " ray %d" % r, rad[r][:len(use_cols)], refs[r])
                    T.jac(tag + " ray %d" % r, jac[r][:, :len(use_cols)], refs[r])
        finally:
            los.close()
    T.rows = _worst_per_tag(T.rows)
    T.finish()


@pytest.mark.parametrize("n_part", [3, 9])
def test_limb_rays_parts(eng, n_part):
    """sr_limb_parts_kernel: C_k <- C_k t + e_k u f is the radiance recursion with the part's emission as the only
    source, the background B <- B t the one without a source: the same reference function (n_part + 1 > 8 changes the
    block size).  A Planck background, observer order, and absorption alone (every part exactly zero, B = I)."""
    from spectrobot_amd import synthetic as syn
    n_gas, n_layers, gas, n_levels = 2, 12, 1, 4
    sc = _scene(n_layers, 3, n_gas)
    N = len(sc["names"])
    cols = np.arange(N)
    rng = np.random.default_rng([SEED, n_part])
    tab, coef_row = _tables(sc, gas, n_levels, rng)
    part_level = np.array([-1, -1] + list(rng.integers(0, n_levels, n_part - 2)), np.int32)
    part_gas = np.array([0, 1] + [gas] * (n_part - 2), np.int32)
    part_c = rng.uniform(0.0, 1.0, (n_part, n_layers))
    coeffs = _coeffs(sc, cols)
    grid = syn.make_grid(2975.0, 5e-4, N)
    T = Tally(sc["names"], cols, n_gas)
    for opts in (dict(initial_temperature=220.0), dict(LOS_order="observer"), dict(solo_absorption=True, initial_temperature=250.0)):
        order, solo, planck = opts.get("LOS_order", "photon"), opts.get("solo_absorption", False), "initial_temperature" in opts
        los = _los(eng, sc, **opts)
        try:
            I0 = _planck(eng, sc, los, N, grid, n_layers) if planck else np.zeros(N)
            rad, parts = eng.limb_rays_parts(coeffs, los, part_gas, part_level, part_c=part_c, tab=_t(tab), coef_row=coef_row,
                                             gas=gas, grid=grid if planck else None)
            rad, parts = _np(rad), _np(parts)
        finally:
            los.close()
        name = ",".join(sorted(opts))
        for r in range(3):
            segs = _segments(sc, r, order)
            lay = sc["L"]["seg_layer"][segs]
            col = sc["col"][:, segs]
            ref = R.recursion_reference(*_ray_forms(sc, segs, R.LD), I0, solo=solo, thin_ulps=n_gas + 1)
            T.plain(ref, _ray_forms(sc, segs, np.float64), I0, solo)
            T.rad("parts %s: total ray %d" % (name, r), rad[r], ref)
            if solo:
                assert not parts[r, :n_part].any() and np.array_equal(parts[r, n_part], rad[r])
                continue
            for k in range(n_part + 1):
                forms = []
                for dt in (R.LD, np.float64):
                    tau = R.products(sc["abs_c"][:, lay], col, dt)
                    if k == n_part:
                        E = np.zeros_like(tau)
                    elif part_level[k] < 0:
                        E = np.asarray(sc["emi_c"][part_gas[k]][lay], dt) * np.asarray(col[part_gas[k]], dt)[:, None]
                    else:
                        e_k = np.asarray(part_c[k][lay], dt)[:, None] * np.asarray(tab[part_level[k], 1][coef_row[lay]], dt)
                        E = e_k * np.asarray(col[gas], dt)[:, None]
                    z3 = np.zeros((0,) + tau.shape, dt)
                    forms.append((tau, E, z3, z3))
                i0 = I0 if k == n_part else np.zeros(N)
                ref = R.recursion_reference(*forms[0], i0, thin_ulps=n_gas + 1)
                T.plain(ref, forms[1], i0, False)
                T.rad("parts %s: %s ray %d" % (name, "background" if k == n_part else "part", r), parts[r, k], ref)
    T.rows = _worst_per_tag(T.rows)
    T.finish()
