#!/usr/bin/env python3
"""Generate tests/golden/line_strengths.npz FROM THE REFERENCE ITSELF: the line-strength family of spect_classes
(SpectLine.CalcStrength, CalcStrength_nonLTE, CalcStrength_from_Einstein, CalcStrength_from_Strength,
calc_A_coeff_from_strength; CalcStrength_at_T, Einstein_A_to_LineStrength_nonLTE, Einstein_B21_to_A, Boltz_pop_at_T,
alpha_nlte, BB, BB_erg).

Runs only where the reference tree and amdflang are (like make_golden.py, whose import_reference_spcl it uses: the
reference's Python under Python 3, its Fortran compiled into oracle/_ref/).  Nothing of the reference is committed.
One stub more than make_golden.py's: spect_base_module.vibtemp_to_ratio, which the reference calls but does not contain
-- with the definition of spectrobot_amd.spect_base_module.vibtemp_to_ratio (unpinned: the build's own).

Lines: N_LINKED linked to a 12-level CH4 table (lev_up / lev_lo) and N_ALL of the 'all' set (lev -1, E_vib = 0),
E_lower up to 3000 cm-1, one line with A = 0 (the G coefficients' zero rule).  Cases: LTE and three sets of
per-level vibrational temperatures tvib[case][level][T]; a line takes T_vib_lower = tvib[lev_lo], T_vib_upper =
tvib[lev_up] (the 'all' lines: the kinetic T, immaterial at E_vib = 0).  Outputs are [case][T][line].
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as MG  # noqa: E402  (sets sys.path for the repository root, dont_write_bytecode)

MOL, ISO, MM = 6, 1, 16.0313
ISO_AB = 0.98827
TEMPS = np.array([70.0, 110.0, 150.0, 180.0, 296.0])
LEVELS = np.array([0., 1311., 1533., 2587., 2612., 2830., 2846., 2917., 3019., 3062., 3065., 4223.])
N_LINKED, N_ALL = 140, 60
C2 = (6.62607015e-34 * 1.e7) * (299792458.0 * 1.e2) / (1.380649e-23 * 1.e7)


def vibtemp_to_ratio(E_vib, T_vib, T):
    return np.exp(-C2 * E_vib / T_vib) / np.exp(-C2 * E_vib / T)


def make_inputs(rng):
    n = N_LINKED + N_ALL
    nlev = len(LEVELS)
    lev_lo = np.full(n, -1, np.int32)
    lev_up = np.full(n, -1, np.int32)
    lo = rng.integers(0, nlev - 1, N_LINKED)
    up = np.array([rng.integers(l + 1, nlev) for l in lo])
    lev_lo[:N_LINKED], lev_up[:N_LINKED] = lo, up
    freq = np.empty(n)
    e_lower = np.empty(n)
    # linked: E_lower = E_vib_lo + rotational energy, nu near E_vib_up - E_vib_lo (at least 20 cm-1)
    freq[:N_LINKED] = np.maximum(LEVELS[up] - LEVELS[lo] + rng.uniform(-150.0, 150.0, N_LINKED), 20.0)
    e_lower[:N_LINKED] = np.minimum(LEVELS[lo] + rng.uniform(0.0, 1200.0, N_LINKED), 3000.0)
    freq[N_LINKED:] = rng.uniform(30.0, 3500.0, N_ALL)
    e_lower[N_LINKED:] = rng.uniform(0.0, 3000.0, N_ALL)
    g_lo = rng.integers(1, 60, n).astype(float)
    g_up = rng.integers(1, 60, n).astype(float)
    a_coeff = 10.0 ** rng.uniform(-3.0, 2.0, n)
    a_coeff[7] = 0.0
    strength = 10.0 ** rng.uniform(-26.0, -19.0, n)   # drawn apart from the A (as a line list's two columns may be)
    air_broad = rng.uniform(0.03, 0.08, n)
    t_dep = rng.uniform(0.5, 0.85, n)
    # per-level vibrational temperatures of the three non-LTE cases (level 0 in LTE: the ground state)
    tvib = np.empty((4, nlev, len(TEMPS)))
    tvib[0] = TEMPS[None, :]
    for c in range(1, 4):
        f = rng.uniform(0.6, 2.2, nlev)
        f[0] = 1.0
        tvib[c] = TEMPS[None, :] * f[:, None]
    return dict(freq=freq, e_lower=e_lower, a_coeff=a_coeff, g_up=g_up, g_lo=g_lo, strength=strength,
                air_broad=air_broad, t_dep_broad=t_dep, lev_up=lev_up, lev_lo=lev_lo, tvib=tvib)


def main():
    spcl, RF = MG.import_reference_spcl()
    sys.modules["spect_base_module"].vibtemp_to_ratio = vibtemp_to_ratio
    rng = np.random.default_rng(20261016)
    I = make_inputs(rng)
    n = len(I["freq"])
    iso = MG.IsoMolec(MOL, ISO, MM, LEVELS)
    lines = MG.ref_lines(spcl, MOL, ISO, I)
    for l, s in zip(lines, I["strength"]):
        l.Strength = float(s)
    nc, nt = I["tvib"].shape[0], len(TEMPS)
    out = {k: np.zeros((nc, nt, n)) for k in ("ein_ab", "ein_em", "str_ab", "str_em", "nonlte", "tvib_lo", "tvib_up")}
    q_t = np.array([spcl.CalcPartitionSum(MOL, ISO, temp=T) for T in TEMPS])
    for i, l in enumerate(lines):
        linked = i < N_LINKED
        for c in range(nc):
            for k, T in enumerate(TEMPS):
                tl = I["tvib"][c, I["lev_lo"][i], k] if linked else T
                tu = I["tvib"][c, I["lev_up"][i], k] if linked else T
                out["tvib_lo"][c, k, i], out["tvib_up"][c, k, i] = tl, tu
                ab, em = l.CalcStrength_from_Einstein(T, iso_ab=ISO_AB, isomolec=iso if linked else None,
                                                      T_vib_lower=tl, T_vib_upper=tu)
                out["ein_ab"][c, k, i], out["ein_em"][c, k, i] = ab, em
                ab, em = l.CalcStrength_from_Strength(T, iso_ab=ISO_AB, T_vib_lower=tl, T_vib_upper=tu)
                out["str_ab"][c, k, i], out["str_em"][c, k, i] = ab, em
                out["nonlte"][c, k, i] = l.CalcStrength_nonLTE(T, tl, tu) if l.A_coeff != 0.0 else 0.0
    cs = np.array([[l.CalcStrength(T) for l in lines] for T in TEMPS])
    # module functions on the lines' own numbers
    t_ref2 = 200.0
    at_t = np.array([[spcl.CalcStrength_at_T(MOL, ISO, l.Strength, l.Freq, l.E_lower, T, T_ref=t_ref2) for l in lines]
                     for T in TEMPS])
    a_from_s = np.array([l.calc_A_coeff_from_strength(iso_ab=ISO_AB) for l in lines])
    b21 = 10.0 ** rng.uniform(-3.0, 3.0, n)
    b21_to_a = np.array([spcl.Einstein_B21_to_A(b, w) for b, w in zip(b21, I["freq"])])
    nonlte_fn = np.array([[spcl.Einstein_A_to_LineStrength_nonLTE(l.A_coeff, l.Freq, l.E_lower, 0.9 * T, 1.3 * T,
                                                                  l.g_lo, l.g_up, q, iso_ab=ISO_AB) for l in lines]
                          for T, q in zip(TEMPS, q_t)])
    pop = np.array([[spcl.Boltz_pop_at_T(l.E_lower, T, l.g_lo, q) for l in lines] for T, q in zip(TEMPS, q_t)])
    r1 = rng.uniform(0.2, 3.0, n)
    r2 = rng.uniform(0.2, 3.0, n)
    alpha = np.array([[spcl.alpha_nlte(l.Freq, T, a, b) for l, a, b in zip(lines, r1, r2)] for T in TEMPS])
    bb = np.array([[spcl.BB(T, l.Freq) for l in lines] for T in TEMPS])
    bb_erg = np.array([[spcl.BB_erg(T, l.Freq) for l in lines] for T in TEMPS])
    np.savez_compressed(os.path.join(HERE, "line_strengths.npz"), mol=MOL, iso=ISO, mm=MM, iso_ab=ISO_AB, temps=TEMPS,
                        level_energies=LEVELS, n_linked=N_LINKED, q_t=q_t, t_ref2=t_ref2, b21=b21, r1=r1, r2=r2,
                        calc_strength=cs, calc_strength_at_t=at_t, a_from_strength=a_from_s, b21_to_a=b21_to_a,
                        nonlte_fn=nonlte_fn, boltz_pop=pop, alpha_nlte=alpha, bb=bb, bb_erg=bb_erg, **I, **out)
    print("line_strengths.npz: %d lines (%d linked), %d cases x %d temperatures" % (n, N_LINKED, nc, nt))


if __name__ == "__main__":
    main()
