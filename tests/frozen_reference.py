"""Reference of the coefficient op with FROZEN region boundaries and LINEARISED weights (include/spectrobot_hip.h,
sr_lineset_set_bounds_temps / sr_lineset_set_linear_weights) and of the temperature derivative built on them: a
plain-Python composition of the oracle's primitives in the style of tests/lineshape_reference.py, which follows
oracle/sr_oracle.c::layer_run (mode 1) line by line.  What changes against it:

    temps_b          the shape comes from oracle.make_shape_bounds with lw_b = lorentz_width(T_b, ...) and
                     dw_b = doppler_width(T_b, mm, Freq): il, ir, il2, ir2 and the region 3 / 4 choice of the core as at
                     T_b, every width, running x and value at the call's T (oracle/sr_oracle.h, sro_humliv_bb_bounds).
                     A pressure-shifted centre x0' is the same for both sets of widths.
    linear_weights   G = calc_gcoeffs(..., T_b) and fac at T_b; G_sp and G_ind times
                     1 + (T - T_b) (c2 eps_up / T_b^2 - 1 / (2 T_b)), G_abs likewise with eps_lo;
                     eps_up = E_low + Freq - E_vib_up, eps_lo = E_low - E_vib_lo.  The populations are the caller's, at
                     the call's T: never linearised.
    smooth           the oracle's "smooth" flag (cmplx(ry, -rx) left in double): for derivatives by difference.

With temps_b = None, or temps_b = temps, it equals oracle.abscoeff_layers(mode=1) bit for bit
(tests/test_frozen_reference_host.py).  TEST INFRASTRUCTURE ONLY; no GPU."""
import math

import numpy as np

from oracle import oracle as O

import lineshape_reference as R

IMXSIG = O.IMXSIG


def lin_factor(T, T_b, eps):
    """1 + (T - T_b) d ln w / d T at T_b of a weight w ~ exp(-c2 eps / T) / sqrt(T) (the Boltzmann factor of a G
    coefficient over the normalisation fac ~ dw ~ sqrt(T))."""
    return 1.0 + (T - T_b) * (O.constants()["c2"] * eps / (T_b * T_b) - 1.0 / (2.0 * T_b))


def _walk(lines, mm, e_lev, temps, press, grid, temps_b=None, linear_weights=False, smooth=False, p_shift=None,
          self_broad=None, p_self=None, want_shape=True):
    """Every kept (layer k, line i) in layer_run's order: yields (k, i, lu, ll, lo, hi, shape, G) -- shape on the grid
    points lo:hi, already divided by fac, and the three G coefficients (sp, ind, abs); with want_shape False
    (k, i, xwin, wn0, lw, dwp, lw_b, dwp_b) instead (dwp = dw / sqrt(ln 2): what humliv_bb receives)."""
    grid = np.ascontiguousarray(grid, dtype=np.float64)
    n = grid.size
    n_lines = len(lines["freq"])
    e_lev = np.asarray(e_lev if e_lev is not None else [], dtype=np.float64)
    nlev = e_lev.size
    temps, press = np.atleast_1d(np.asarray(temps, float)), np.atleast_1d(np.asarray(press, float))
    temps_b = temps if temps_b is None else np.atleast_1d(np.asarray(temps_b, float))
    assert temps_b.shape == temps.shape
    sp_step = grid[1] - grid[0]
    start = -IMXSIG * sp_step / 2
    delta = (start + sp_step) - start
    lin_grid = start + np.arange(IMXSIG) * delta
    ic = [O.closest_grid(grid, float(f)) for f in lines["freq"]]
    sqrt_ln2 = math.sqrt(math.log(2.0))
    for k in range(temps.size):
        T, Tb, P = float(temps[k]), float(temps_b[k]), float(press[k])
        P_atm = O.convert_to_atm(P)
        Ps_atm = O.convert_to_atm(float(p_self[k])) if (p_self is not None and self_broad is not None) else 0.0
        for i in range(n_lines):
            lu = ll = 0
            evu = evl = 0.0
            if nlev > 0:
                lu, ll = int(lines["lev_up"][i]), int(lines["lev_lo"][i])
                if lu < 0 or ll < 0 or lu == ll:
                    continue
                evu, evl = float(e_lev[lu]), float(e_lev[ll])
            freq = float(lines["freq"][i])
            xwin = lin_grid + grid[ic[i]]
            n_air, g_air = float(lines["t_dep_broad"][i]), float(lines["air_broad"][i])
            g_self = float(self_broad[i]) if self_broad is not None else 0.0
            lw = R.lorentz_width(T, P_atm, n_air, g_air, g_self, Ps_atm)
            dw = O.doppler_width(T, mm, freq)
            lw_b = R.lorentz_width(Tb, P_atm, n_air, g_air, g_self, Ps_atm)
            dw_b = O.doppler_width(Tb, mm, freq)
            wn0 = freq + float(p_shift[i]) * P_atm if p_shift is not None else freq
            if not want_shape:
                yield k, i, xwin, wn0, lw, dw / sqrt_ln2, lw_b, dw_b / sqrt_ln2
                continue
            shape = O.make_shape_bounds(xwin, wn0, lw, dw, lw_b, dw_b, 1 if smooth else 0)
            a, el = float(lines["a_coeff"][i]), float(lines["e_lower"][i])
            gu, gl = float(lines["g_up"][i]), float(lines["g_lo"][i])
            if linear_weights:
                G = O.calc_gcoeffs(freq, a, el, gu, gl, evu, evl, Tb)
                f_up, f_lo = lin_factor(T, Tb, el + freq - evu), lin_factor(T, Tb, el - evl)
                G = np.array([G[0] * f_up, G[1] * f_up, G[2] * f_lo])
                if dw_b != dw:
                    shape = shape * (dw / dw_b)      # fac at T_b: shape = y / fac(T), fac ~ dw
            else:
                G = O.calc_gcoeffs(freq, a, el, gu, gl, evu, evl, T)
            j0 = ic[i] - IMXSIG // 2
            mlo = -j0 if j0 < 0 else 0
            mhi = n - j0 if j0 + IMXSIG > n else IMXSIG
            if mhi <= mlo:
                continue
            yield k, i, lu, ll, j0 + mlo, j0 + mhi, shape[mlo:mhi], G


def populations(e_lev, temps, q_part, tvib):
    """pop [n_layers][max(n_levels, 1)] as layer_run forms them: boltz_ratio_nodeg(E_L, Tvib_L or T) / Q; 1 / Q for the
    'all' set."""
    e_lev = np.asarray(e_lev if e_lev is not None else [], dtype=np.float64)
    out = []
    for k, T in enumerate(np.atleast_1d(np.asarray(temps, float))):
        if e_lev.size:
            out.append([O.boltz_ratio_nodeg(float(e_lev[lv]), float(tvib[lv][k]) if tvib is not None else float(T)) / float(q_part[k])
                        for lv in range(e_lev.size)])
        else:
            out.append([1 / float(q_part[k])])
    return out


def abscoeff_layers(lines, mm, e_lev, temps, press, q_part, tvib, grid, temps_b=None, linear_weights=False, smooth=False,
                    p_shift=None, self_broad=None, p_self=None):
    """(abs, emi) [n_layers, n_grid]: the folded coefficient op.  lines: the dict oracle.abscoeff_layers takes."""
    temps = np.atleast_1d(np.asarray(temps, float))
    ab = np.zeros((temps.size, len(grid)))
    em = np.zeros((temps.size, len(grid)))
    pop = populations(e_lev, temps, q_part, tvib)
    for k, i, lu, ll, lo, hi, shape, G in _walk(lines, mm, e_lev, temps, press, grid, temps_b, linear_weights, smooth, p_shift,
                                                self_broad, p_self):
        wabs = pop[k][ll] * G[2] - pop[k][lu] * G[1]
        wemi = pop[k][lu] * G[0]
        ab[k, lo:hi] += shape * wabs
        em[k, lo:hi] += shape * wemi
    return ab, em


def level_pairs(lines, mm, e_lev, temps, press, grid, temps_b=None, linear_weights=False, smooth=False, p_shift=None,
                self_broad=None, p_self=None):
    """[max(n_levels, 1), 2, n_layers, n_grid]: the weights of kWeightLevelPair, A_L = Gabs_L - Gind_L | E_L = Gsp_L --
    what pop_L multiplies in the combine loop (sr_glevel_pairs_dev).  No population enters."""
    temps = np.atleast_1d(np.asarray(temps, float))
    nlev = len(e_lev) if e_lev is not None else 0
    tab = np.zeros((max(nlev, 1), 2, temps.size, len(grid)))
    for k, i, lu, ll, lo, hi, shape, G in _walk(lines, mm, e_lev, temps, press, grid, temps_b, linear_weights, smooth, p_shift,
                                                self_broad, p_self):
        tab[ll, 0, k, lo:hi] += shape * G[2]
        tab[lu, 0, k, lo:hi] -= shape * G[1]
        tab[lu, 1, k, lo:hi] += shape * G[0]
    return tab


def combine(tab, step_row, pop, tab_dT=None, dpop=None, dT=None):
    """sr_glevel_combine_dev's formula in numpy: abs[s] = sum_L pop[s, L] A_L[row[s]], emi likewise with E; with tab_dT
    also dabs[s] = sum_L dpop[s, L] A_L + pop[s, L] (A'_L - A_L) / dT.  (abs, emi) or ((abs, emi), (dabs, demi))."""
    step_row = np.asarray(step_row, int)
    pop = np.asarray(pop, float)
    t = tab[:, :, step_row, :]                                  # [L, 2, s, n]
    out = np.einsum("sl,lcsn->csn", pop, t)
    if tab_dT is None:
        return out[0], out[1]
    d = (tab_dT[:, :, step_row, :] - t) * (1.0 / dT)
    dout = np.einsum("sl,lcsn->csn", np.asarray(dpop, float), t) + np.einsum("sl,lcsn->csn", pop, d)
    return (out[0], out[1]), (dout[0], dout[1])


def bounds(lines, mm, temps, press, grid, e_lev=None, p_shift=None, self_broad=None, p_self=None):
    """[n_lines, n_layers, 6] ints: what sro_humliv_bounds returns for every (line, layer) at the layers' `temps` --
    il, ir, il2, ir2, k3lo, k3hi of the 13010-point window; -1 everywhere for a line the filter drops or whose centre
    lies outside its window (a sequential branch: nothing to freeze)."""
    temps = np.atleast_1d(np.asarray(temps, float))
    out = np.full((len(lines["freq"]), temps.size, 6), -1, dtype=np.int64)
    for k, i, xwin, wn0, lw, dwp, _, _ in _walk(lines, mm, e_lev, temps, press, grid, None, False, False, p_shift, self_broad,
                                                p_self, want_shape=False):
        b = O.humliv_bounds(xwin, 1, IMXSIG, wn0, lw, dwp)
        if b is not None:
            out[i, k] = b
    return out


def fd_quotient(lines, mm, e_lev, temps, press, q_of_T, tvib, grid, h, scheme="central", smooth=False, linear_weights=False,
                **shape_kw):
    """The reference's own difference quotient of the folded op in T, built as engine.coefficients_dT builds the
    product's: boundaries frozen at `temps`, the vibrational temperatures fixed when given (LTE: they follow T), the
    partition sum q_of_T(T) following T.  central: (c(T + h) - c(T - h)) / 2h; forward: (c(T + h) - c(T)) / h with c(T)
    the plain call.  Returns (dabs, demi)."""
    temps = np.atleast_1d(np.asarray(temps, float))

    def c(dt):
        t = temps + dt
        return abscoeff_layers(lines, mm, e_lev, t, press, q_of_T(t), tvib, grid, temps_b=temps, linear_weights=linear_weights,
                               smooth=smooth, **shape_kw)
    if scheme == "central":
        (ap, ep), (am, em) = c(h), c(-h)
        return (ap - am) / (2.0 * h), (ep - em) / (2.0 * h)
    (ap, ep), (a0, e0) = c(h), c(0.0)
    return (ap - a0) / h, (ep - e0) / h


def dcoeff_dT_smooth(lines, mm, e_lev, temps, press, q_of_T, tvib, grid, h=0.1, **shape_kw):
    """The reference derivative (d abs / d T, d emi / d T) [n_layers, n_grid] of the folded op with respect to each
    layer's kinetic temperature: the Richardson-extrapolated central difference (4 D(h / 2) - D(h)) / 3, h = 0.1 K, of
    the smooth=True reference with the boundaries frozen at T, exact weights, and populations and q_of_T(T) following
    T as LineSet.abscoeff_layers does (vibrational temperatures fixed when given).  With boundaries frozen and the
    single-precision casts dropped the differenced function is smooth in T (piecewise rational / exponential in the
    widths), so D(h) = c' + h^2 c''' / 6 + O(h^4) and the extrapolation leaves O(h^4).

    Its own error, measured by tests/test_frozen_reference_host.py on the many-lines case (h = 0.1 against h = 0.2, per
    layer, relative to the layer's largest derivative): the two extrapolations lie 2.7e-9 (abs) and 3.9e-10 (emi) apart
    at the worst layer.  That distance is the error of the h = 0.2 value; the h = 0.1 value's O(h^4) remainder is a
    sixteenth of it, ~2e-10 -- four orders below the smallest scheme error it is used to measure (1e-5)."""
    def D(hh):
        return fd_quotient(lines, mm, e_lev, temps, press, q_of_T, tvib, grid, hh, "central", smooth=True, **shape_kw)
    (a1, e1), (a2, e2) = D(h), D(0.5 * h)
    return (4.0 * a2 - a1) / 3.0, (4.0 * e2 - e1) / 3.0


def partition_sum_dT(mol, iso, temps):
    """d Q / d T of the oracle's interpolant (oracle.calc_partition_sum: the Lagrange polynomial through the two table
    temperatures <= T and the two > T of tests/golden/tips2003.npz), differentiated term by term in np.longdouble:
    sum_j q_j sum_(m != j) prod_(k != j, m) (T - x_k) / prod_(k != j) (x_j - x_k)."""
    import os
    g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "tips2003.npz"), allow_pickle=False)
    keys = [tuple(int(v) for v in k) for k in g["keys"]]
    tg = np.asarray(g["t_grid"], np.longdouble)
    qg = np.asarray(g["q_tab"][keys.index((int(mol), int(iso)))], np.longdouble)
    out = []
    for T in np.atleast_1d(np.asarray(temps, float)):
        n_le = int(np.sum(g["t_grid"] <= T))
        sel = list(range(max(0, n_le - 2), n_le)) + list(range(n_le, min(tg.size, n_le + 2)))
        xs, qs, Tl = tg[sel], qg[sel], np.longdouble(T)
        d = np.longdouble(0)
        for j in range(len(sel)):
            den = np.longdouble(1)
            for k in range(len(sel)):
                if k != j:
                    den = den * (xs[j] - xs[k])
            num = np.longdouble(0)
            for m in range(len(sel)):
                if m == j:
                    continue
                pr = np.longdouble(1)
                for k in range(len(sel)):
                    if k not in (j, m):
                        pr = pr * (Tl - xs[k])
                num = num + pr
            d = d + qs[j] * num / den
        out.append(float(d))
    return np.array(out)


def many_lines_case(oracle=O):
    """The many-lines case of the frozen-boundary tests, shared by the host and the GPU file: 600 lines x 20 000 points x
    4 layers whose ry spans Doppler to Lorentz (1e-3, 10, 80, 1013 hPa), 12 levels, non-LTE vibrational temperatures;
    among the lines six outer ones (3.3, 4 and 6 cm-1 beyond either grid end: humliv_bb's sequential branches) and four
    main lines centred beyond an end.  The temperatures keep +-3.2 K clear of the partition table's nodes."""
    from spectrobot_amd import synthetic as syn
    grid = syn.make_grid(2975.0, 5e-4, 20000)
    L = syn.make_lines(600, grid, config_id=23, n_levels=12)
    f = L["freq"].copy()
    pick = np.arange(10) * 59 + 7          # ten of the random lines move to the ends and beyond
    f[pick] = np.concatenate([grid[0] - np.array([3.3, 4.0, 6.0]), grid[-1] + np.array([3.3, 4.0, 6.0]),
                              grid[0] - np.array([0.3, 1.5]), grid[-1] + np.array([0.2, 2.0])])
    order = np.argsort(f, kind="stable")
    L = {k: np.ascontiguousarray(v[order]) for k, v in L.items()}
    L["freq"] = np.ascontiguousarray(f[order])
    temps = np.array([165.0, 172.0, 158.0, 181.0])
    press = np.array([1e-3, 10.0, 80.0, 1013.0])
    atm = syn.make_atmosphere(4, 12)
    tvib = np.ascontiguousarray(atm["tvib"] - atm["temps"] + temps)
    rng = np.random.default_rng(41)
    return dict(grid=grid, L=L, mm=syn.CH4_MM, e_lev=syn.CH4_LEVEL_ENERGIES, temps=temps, press=press, tvib=tvib,
                q_of_T=lambda t: oracle.partition_sums(6, 1, t), p_shift=rng.uniform(-0.03, 0.01, 600),
                self_broad=rng.uniform(0.05, 0.12, 600), p_self=0.05 * press)


def exercise(b_call, b_bounds):
    """What a boundary temperature changes, from two results of bounds(): (fraction of the (line, layer) pairs with a
    middle branch whose il, ir, il2 or ir2 differs, number of pairs whose region-3 interval differs)."""
    mid = (b_call[:, :, 0] >= 0) & (b_bounds[:, :, 0] >= 0)
    idx = np.any(b_call[:, :, :4] != b_bounds[:, :, :4], axis=2)
    r3 = np.any(b_call[:, :, 4:] != b_bounds[:, :, 4:], axis=2)
    return float(idx[mid].mean()), int(r3[mid].sum())


def layer_rel(x, y):
    """Per layer: max |x - y| over the layer's largest |y|."""
    x, y = np.asarray(x, float), np.asarray(y, float)
    return np.max(np.abs(x - y), axis=-1) / np.max(np.abs(y), axis=-1)
