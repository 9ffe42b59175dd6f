"""Reference of the coefficient op WITH pressure shift and self-broadening (include/spectrobot_hip.h,
sr_lineset_set_line_shape): a plain-Python composition of the oracle's own primitives that follows
oracle/sr_oracle.c::layer_run (mode 1) line by line, with the two changes the reference's code intends and does not
make (spect_classes.py:187 computes wn_0 = Freq + P_shift Pres_atm and :197 hands Freq to MakeShape; Lorenz_width's
Self_broad / Self_pres_atm, :1967-1972, are never passed):

    wn0 = Freq + p_shift P_atm                                     centre handed to make_shape
    lw  = (296/T)^n (gamma_air (P_atm - Ps_atm) + gamma_self Ps_atm)

Everything else stays at Freq: the Doppler width, the G coefficients, the window (ic = closest_grid(Freq)).
With p_shift = self_broad = None it equals oracle.abscoeff_layers(mode=1) bit for bit
(tests/test_lineshape_reference_host.py).  TEST INFRASTRUCTURE ONLY."""
import numpy as np

from oracle import oracle as O

IMXSIG = O.IMXSIG


def lorentz_width(T, P_atm, n_air, gamma_air, gamma_self=0.0, Ps_atm=0.0):
    """spcl:1972 through the oracle's lorenz_width: pow(296/T, n) * (1.0 * (x - 0.0) + 0.0 * 0.0) = pow(..) * x exactly,
    with x = gamma_air (P - Ps) + gamma_self Ps (= gamma_air P exactly for Ps = 0)."""
    x = gamma_air * (P_atm - Ps_atm) + gamma_self * Ps_atm
    return O.lorenz_width(T, x, n_air, 1.0)


def abscoeff_layers(lines, mm, e_lev, temps, press, q_part, tvib, grid, p_shift=None, self_broad=None, p_self=None):
    """(abs, emi) [n_layers, n_grid].  lines: the dict oracle.abscoeff_layers takes; p_shift / self_broad [n_lines]
    (cm^-1 / atm) or None; p_self [n_layers] hPa or None (0)."""
    grid = np.ascontiguousarray(grid, dtype=np.float64)
    n = grid.size
    n_lines = len(lines["freq"])
    e_lev = np.asarray(e_lev if e_lev is not None else [], dtype=np.float64)
    nlev = e_lev.size
    temps, press = np.asarray(temps, float), np.asarray(press, float)
    nlay = temps.size
    sp_step = grid[1] - grid[0]
    start = -IMXSIG * sp_step / 2
    delta = (start + sp_step) - start
    lin_grid = start + np.arange(IMXSIG) * delta
    ic = [O.closest_grid(grid, float(f)) for f in lines["freq"]]
    ab = np.zeros((nlay, n))
    em = np.zeros((nlay, n))
    for k in range(nlay):
        T, P = float(temps[k]), float(press[k])
        P_atm = O.convert_to_atm(P)
        Ps_atm = O.convert_to_atm(float(p_self[k])) if p_self is not None else 0.0
        if nlev > 0:
            pop = [O.boltz_ratio_nodeg(float(e_lev[lv]), float(tvib[lv][k]) if tvib is not None else T) / float(q_part[k])
                   for lv in range(nlev)]
        else:
            pop = [1 / float(q_part[k])]
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
            g_self = float(self_broad[i]) if self_broad is not None else 0.0
            lw = lorentz_width(T, P_atm, float(lines["t_dep_broad"][i]), float(lines["air_broad"][i]), g_self,
                               Ps_atm if self_broad is not None else 0.0)
            dw = O.doppler_width(T, mm, freq)
            wn0 = freq + float(p_shift[i]) * P_atm if p_shift is not None else freq
            shape = O.make_shape(xwin, wn0, lw, dw)
            G = O.calc_gcoeffs(freq, float(lines["a_coeff"][i]), float(lines["e_lower"][i]), float(lines["g_up"][i]),
                               float(lines["g_lo"][i]), evu, evl, T)
            j0 = ic[i] - IMXSIG // 2
            mlo = -j0 if j0 < 0 else 0
            mhi = n - j0 if j0 + IMXSIG > n else IMXSIG
            if mhi <= mlo:
                continue
            wabs = pop[ll] * G[2] - pop[lu] * G[1]
            wemi = pop[lu] * G[0]
            ab[k, j0 + mlo:j0 + mhi] += shape[mlo:mhi] * wabs
            em[k, j0 + mlo:j0 + mhi] += shape[mlo:mhi] * wemi
    return ab, em


def layer_max(a):
    """Largest |value| of every layer: what the effect sizes are fractions of."""
    return np.max(np.abs(a), axis=1, keepdims=True)


def effect(a, b):
    """Per layer: max |a - b| as a fraction of the layer's largest |b|."""
    return (np.max(np.abs(a - b), axis=1) / layer_max(b)[:, 0])
