"""Every compiled instance of sr_limb_jac_state_kernel on the GPU, held to the extended-precision reference.

tests/state_instances_cases.EXPECTED lists the 432 instances with the smallest call that reaches each.  A test per gas
count makes those calls; after each, engine.last_state_instance() -- the compile-time constants of the instantiation that
was launched, recorded at the launch -- must be the entry's instance: a call that lands elsewhere is a failure.
  spectra instances: radiances and every Jacobian row against limb_reference.recursion_reference, in its units, within
      KERNEL_MARGIN x K_PLAIN measured on the case's own inputs (the device's columns); the rows without weights exact
      zeros; a pointing row as many_gases_cases.pointing_row forms it;
  BANDS instances: against engine.hires_to_lowres of the spectra of their twin without BANDS (same state, itself held to
      the reference above), 1e-12 of a row's largest element; the band outside the grid exactly zero;
  INSTR instances: the two last rows against hires_to_lowres_instrument of the twin's radiances by the same rule, the
      other rows those of the BANDS twin bit for bit.
The last census test makes every call again by itself and asserts that the instances visited are the compiled set.
One more test holds a resident batch to the weights it was called with after an in-place edit of them."""
import numpy as np
import pytest

import limb_reference as R
import state_instances_cases as X

pytestmark = pytest.mark.gpu

BANDS_BOUND = 1e-12      # tests/test_gpu_state_bands.py
ENTRIES = [X.entry_dict(e) for e in X.EXPECTED]


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


def _bands_of(grid, rng, n_bands=33):
    """33 bands (three band tiles): one outside the grid, one over all of it, the rest scattered (test_gpu_many_gases)."""
    lam_lo, lam_hi = 1e7 / grid[-1], 1e7 / grid[0]
    span = lam_hi - lam_lo
    bands = np.concatenate([[lam_lo - 50 * span - 1.0, 0.5 * (lam_lo + lam_hi)], lam_lo + span * rng.uniform(0.02, 0.98, n_bands - 2)])
    widths = np.concatenate([[0.05 * span, 3.0 * span], span * rng.uniform(0.003, 0.2, n_bands - 2)])
    return bands, widths


def _band_distance(f, u):
    scale = np.max(np.abs(u), axis=(0, 2), keepdims=True)
    return float(np.max(np.abs(f - u) / np.where(scale > 0, scale, 1.0)))


class Batch(object):
    """The case of one gas count on the device: the panel on the launched points, the batches of the options, and what
    the entries share -- states, device columns, references (one per state and option)."""

    def __init__(self, eng, n_gas):
        from spectrobot_amd import synthetic as syn
        self.eng, self.n_gas = eng, n_gas
        self.c = X.panel_case(n_gas)
        self.N = len(self.c["names"])
        self.at = R.tile_columns(self.N, X.N_PTS, np.random.default_rng([X.SEED, n_gas, 21]))
        self.put = lambda a: _t(a[..., self.at])
        self.coeffs = (self.put(self.c["coef_a"]), self.put(self.c["coef_e"]))
        self.grids = {False: syn.make_grid(2975.0, 5e-4, X.N_PTS), True: syn.make_grid(2975.0, 5e-4, X.N_GRID)}
        self.bands = {k: _bands_of(g, np.random.default_rng([X.SEED, 9])) for k, g in self.grids.items()}
        self.col = self.columns(self.c["vmr"], self.c["col_scale"])
        self._los, self._states, self._dcol, self._refs, self._kw = {}, {}, {}, {}, {}

    def columns(self, profiles, scale):
        """[., n_seg] columns from the device, four profiles per batch (the column kernel every batch size runs)."""
        c, g, out = self.c, self.c["geo"], []
        for p0 in range(0, len(profiles), 4):
            los = self.eng.LimbLOS(g["seg_off"], g["seg_layer"], g["pt_off"], c["x"], c["nd"], profiles[p0:p0 + 4], col_scale=scale[p0:p0 + 4])
            out.append(los.columns())
            los.close()
        return np.concatenate(out) if out else np.zeros((0, g["n_seg"]))

    def los(self, option):
        key = option if option in ("observer", "solo", "planck", "pointing") else None
        if key not in self._los:
            self._los[key] = X.make_los(self.eng, self.c, key)
        return self._los[key]

    def grid(self, option):
        """(grid, g_lo, bands, widths) of an option: the tables are the whole grid, or points G_LO .. of a wider one."""
        wide = option == "g_lo"
        return (self.grids[wide], X.G_LO if wide else 0) + self.bands[wide]

    def state(self, e):
        key = (e["n_col"], e["levs"], e["n_row"])
        if key not in self._states:
            s = X.state(self.c, *key)
            self._states[key] = s
            self._dcol[key] = self.columns(s["par_w"], self.c["col_scale"][s["par_gas"]]) if s["n_col"] else np.zeros((0, X.N_SEG))
        return self._states[key]

    def keywords(self, e):
        """The parameter keywords of an entry's call; the tensors of a state go to the device once."""
        key = (e["n_col"], e["levs"], e["n_row"], e["call"] == "level", e["option"] == "pointing")
        if key not in self._kw:
            self._kw[key] = X.call_keywords(self.state(e), e, self.put)
        return self._kw[key]

    def initial(self, option):
        """The Planck start as the library forms it, [n_pts]: a call through empty tables."""
        import torch
        zero = torch.zeros((self.n_gas, X.N_LAYERS, X.N_PTS), dtype=torch.float64, device="cuda")
        return _np(self.eng.limb_rays((zero, zero), self.los("planck"), grid=self.grids[False], resident=False))[0]

    def refs(self, e):
        """(references per ray on the launched points' columns, hidden slots or 0): shared by the entries of a state and
        an option.  A Planck start differs from point to point: its references are made on the launched points."""
        opt = e["option"] if e["option"] != "g_lo" else None
        key = (e["n_col"], e["levs"], e["n_row"], opt)
        if key not in self._refs:
            s = self.state(e)
            _, solo, observer = X.options_of(opt)
            hidden = self.eng.los_columns_dz(self.los("pointing")) if opt == "pointing" else None
            planck = opt in ("planck", "solo")
            refs = X.references(s, self.col, self._dcol[key[:3]], self.initial(opt) if planck else None, solo=solo, hidden=hidden,
                                observer=observer, at=self.at if planck else None)
            self._refs[key] = (refs, planck)
        return self._refs[key]

    def close(self):
        for los in self._los.values():
            los.close()


def _launch(B, e):
    """The engine call of an entry: (rad, jac) tensors of a spectra entry, the numpy bands of the others; then the census."""
    eng = B.eng
    grid, g_lo, bands, widths = B.grid(e["option"])
    los, kw = B.los(e["option"]), B.keywords(e)
    if e["call"] == "level":
        eng.set_state_ray_blocks(e["ray_blocks"])
        try:
            out = eng.limb_rays_level_jacobian(B.coeffs, los, kw["tab"], kw["coef_row"], kw["par_level"], kw["par_c"], gas=kw["gas"], grid=grid,
                                               g_lo=g_lo)
        finally:
            eng.set_state_ray_blocks(False)
    elif e["call"] == "state":
        out = eng.limb_rays_state_jacobian(B.coeffs, los, grid=grid, g_lo=g_lo, ray_blocks=e["ray_blocks"], **kw)
    else:
        out = eng.limb_rays_state_bands(B.coeffs, los, grid, bands, widths, g_lo=g_lo, instrument=e["call"] == "instr",
                                        ray_blocks=e["ray_blocks"], **kw)
    got = eng.last_state_instance()
    assert got is not None and X.flags_of(got) == e["key"], "entry %s ran instance %s" % (e["key"], got)
    assert eng.last_state_route()[0] == (2 if e["ray_blocks"] else 1)
    return out


def _check_spectra(B, e, rad, jac, tally):
    """Radiances and every Jacobian row of a spectra entry against the reference, in its units."""
    n_gas, s = B.n_gas, B.state(e)
    refs, on_points = B.refs(e)
    n_state, pointing = e["n_state"], e["option"] == "pointing"
    sel = (lambda a: a) if on_points else (lambda a: a[..., B.at])
    k_rad, k_jac = X.k_plain(refs, n_gas, n_state=n_state if pointing else None)
    lim_rad, lim_jac = R.KERNEL_MARGIN * k_rad, R.KERNEL_MARGIN * k_jac
    assert tuple(jac.shape) == (3, n_state + pointing, X.N_PTS) and tuple(rad.shape) == (3, X.N_PTS)
    w_rad = w_jac = 0.0
    for r, (ref, _) in enumerate(refs):
        w_rad = max(w_rad, R.units(rad[r], sel(ref["I"]), sel(ref["A_I"]), sel(ref["C_I"]), n_gas).max())
        J, A, C = (sel(ref[k][:n_state]) for k in ("J", "A", "C"))
        w_jac = max(w_jac, R.units(jac[r, :n_state], J, A, C, n_gas).max())
        if pointing:
            _, ref_p, A_p, C_p = X.pointing_row(ref, ref["J"], n_state, n_gas)
            w_jac = max(w_jac, R.units(jac[r, n_state], sel(ref_p), sel(A_p), sel(C_p), n_gas).max())
    tally.append((e["key"], k_rad, k_jac, w_rad, w_jac))
    assert w_rad <= lim_rad and w_jac <= lim_jac, (e["key"], e["option"], "rad %.3g of %.3g, jac %.3g of %.3g" % (w_rad, lim_rad, w_jac, lim_jac))
    assert k_jac > 0 and (k_rad > 0 or e["option"] == "solo")
    for p0, n in ((0, s["n_col"]), (s["n_col"], s["n_lev"]), (s["n_col"] + s["n_lev"], s["n_row"])):
        if n > 1:
            assert not jac[:, p0 + 1].any(), (e["key"], p0 + 1)      # the parameter without weights: exact zeros
        if n:
            assert np.abs(jac[:, p0]).max() > 0
    if pointing:
        assert np.abs(jac[:, n_state]).max() > 0


def _lowres(B, e, spectra):
    grid, g_lo, bands, widths = B.grid(e["option"])
    return B.eng.hires_to_lowres(spectra.contiguous(), grid, bands, widths, g_lo=g_lo)


def _check_bands(B, e, low, twin, dists):
    """A BANDS entry against the band sums of its twin's spectra."""
    rad, jac = twin
    n_rows = jac.shape[1]
    assert low.shape == (3, 1 + n_rows, 33)
    comp = np.concatenate([_lowres(B, e, rad)[:, None, :], _lowres(B, e, jac.contiguous().view(3 * n_rows, -1)).reshape(3, n_rows, -1)], axis=1)
    dist = _band_distance(low, comp)
    dists.append(dist)
    assert np.all(low[..., 0] == 0.0), e["key"]                       # the band outside the grid
    assert np.abs(low[:, 0]).max() > 0 and dist <= BANDS_BOUND, (e["key"], dist)


def _check_instr(B, e, instr, plain, twin, dists):
    """An INSTR entry: the instrument rows against hires_to_lowres_instrument of the twin's radiances, the others the
    BANDS twin's bit for bit (without any parameter: the radiance row, which no parameter takes part in)."""
    grid, g_lo, bands, widths = B.grid(e["option"])
    _, d_c, d_w = B.eng.hires_to_lowres_instrument(twin[0].contiguous(), grid, bands, widths, g_lo=g_lo)
    if e["n_state"]:
        assert instr.shape == (3, plain.shape[1] + 2, 33) and np.array_equal(instr[:, :-2], plain), e["key"]
    else:
        assert instr.shape == (3, 3, 33) and np.array_equal(instr[:, 0], plain[:, 0]), e["key"]
    dist = _band_distance(instr[:, -2:], np.stack([d_c, d_w], axis=1))
    dists.append(dist)
    assert np.abs(instr[:, -2:]).max() > 0 and np.all(instr[..., 0] == 0.0) and dist <= BANDS_BOUND, (e["key"], dist)


@pytest.mark.parametrize("n_gas", range(1, 9))
def test_instances_against_the_reference(eng, n_gas):
    """The share of EXPECTED that runs on a batch of n_gas gases: one call per instance, each held to the reference."""
    mine = sorted((e for e in ENTRIES if e["n_gas"] == n_gas), key=lambda e: ("B" in e["flags"], "I" in e["flags"]))
    B = Batch(eng, n_gas)
    spectra, plain, tally, dists = {}, {}, [], []
    try:
        for e in mine:
            out = _launch(B, e)
            if e["call"] in ("level", "state"):
                spectra[e["key"]] = out
                _check_spectra(B, e, _np(out[0]), _np(out[1]), tally)
            elif e["call"] == "bands":
                plain[e["key"]] = out
                _check_bands(B, e, out, spectra[e["twin"]], dists)
            else:
                _check_instr(B, e, out, plain[(e["ng"], e["np"], e["flags"].replace("I", "-"))], spectra[e["twin"]], dists)
    finally:
        B.close()
    k = np.array([t[1:] for t in tally])
    print("\nstate instances, %d gases (NG %s): %d instances visited (%d spectra, %d bands, %d with instrument rows); K_PLAIN up to rad %.3g "
          "jac %.3g (recorded %.3g, %.3g); worst rad %.3g units (%.2f of its limit), jac %.3g units (%.2f of its limit); "
          "bands |fused - composed| / scale up to %.2e (bound %.0e)"
          % (n_gas, sorted({e["ng"] for e in mine}), len(mine), len(tally), len(plain), len(mine) - len(tally) - len(plain), k[:, 0].max(),
             k[:, 1].max(), R.K_PLAIN_RAD, R.K_PLAIN_JAC, k[:, 2].max(), np.max(k[:, 2] / np.maximum(R.KERNEL_MARGIN * k[:, 0], 1e-300)),
             k[:, 3].max(), np.max(k[:, 3] / (R.KERNEL_MARGIN * k[:, 1])), max(dists), BANDS_BOUND))
    assert len(mine) == len(tally) + len(dists)


def test_every_compiled_instance_was_reached_or_is_barred(eng):
    """Every entry's call once more, by this test alone: the instances the census reports are the compiled set -- no
    reachable instance is left out (X.BARRED, the instances no call can reach, is empty: nothing is refused here; the
    refusal of a call without any parameter is tests/test_state_instances_host.py's)."""
    visited, per_ng = set(), {}
    for n_gas in range(1, 9):
        B = Batch(eng, n_gas)
        try:
            for e in (e for e in ENTRIES if e["n_gas"] == n_gas):
                _launch(B, e)
                visited.add(X.flags_of(eng.last_state_instance()))
                per_ng[e["ng"]] = per_ng.get(e["ng"], 0) + 1
        finally:
            B.close()
    compiled = X.compiled_instances()
    print("\nstate instances visited per NG: %s of %d compiled; barred: %d" % (sorted(per_ng.items()), len(compiled), len(X.BARRED)))
    assert not (visited & set(X.BARRED)) and visited | set(X.BARRED) == compiled, sorted(compiled - visited)
    assert per_ng == {1: 48, 2: 96, 3: 96, 4: 96, 6: 48, 8: 48}


def test_a_resident_batch_follows_an_in_place_edit_of_its_weights(eng):
    """limb_rays_jacobian(resident=True) keys the batch it keeps on the device by the content of par_w.  Two neighbours
    of a 6 x 90 table (4320 bytes: keyed by the reductions over its words) change places in the caller's array: the second
    call must return the Jacobian of the weights as they are now -- each call against the reference of its own weights.
    (With the key that weighted position i by i | 1 the second call found the first call's batch.)"""
    n_gas = 3
    B = Batch(eng, n_gas)
    try:
        s = dict(X.state(B.c, 6, (), 0))
        par_w = np.array(s["par_w"])
        assert par_w.shape == (6, 90) and par_w.nbytes > 4096 and par_w.flags.writeable
        i = next(i for i in range(2 * 90 + 10, 3 * 90 - 1) if par_w.reshape(-1)[i] != par_w.reshape(-1)[i + 1])   # row 2: it has weights
        los = B.los(None)
        results = []
        for edit in (False, True):
            if edit:
                flat = par_w.reshape(-1)
                flat[i], flat[i + 1] = flat[i + 1], flat[i]
            s["par_w"] = par_w.copy()
            dcol = B.columns(s["par_w"], B.c["col_scale"][s["par_gas"]])
            refs = X.references(s, B.col, dcol)
            rad, jac = eng.limb_rays_jacobian(B.coeffs, los, s["par_gas"], par_w, resident=True)
            results.append((_np(jac), refs, dcol))
        assert not np.array_equal(results[0][2], results[1][2])
        for tag, (jac, refs, _) in zip(("as given", "after the edit"), results):
            k_rad, k_jac = X.k_plain(refs, n_gas)
            worst = max(R.units(jac[r], ref["J"][:, B.at], ref["A"][:, B.at], ref["C"][:, B.at], n_gas).max() for r, (ref, _) in enumerate(refs))
            print("\nresident batch, weights %s: K_PLAIN jac %.3g, limit %.3g, worst %.3g units" % (tag, k_jac, R.KERNEL_MARGIN * k_jac, worst))
            assert k_jac > 0 and worst <= R.KERNEL_MARGIN * k_jac, tag
        stale = max(R.units(results[0][0][r], ref["J"][:, B.at], ref["A"][:, B.at], ref["C"][:, B.at], n_gas).max()
                    for r, (ref, _) in enumerate(results[1][1]))
        assert stale > R.KERNEL_MARGIN * X.k_plain(results[1][1], n_gas)[1]        # (the test can tell the two apart)
    finally:
        B.close()
