"""Inputs, references and the census table of the tests that hold every compiled instance of sr_limb_jac_state_kernel to
the extended-precision reference (tests/test_state_instances_host.py, tests/test_gpu_state_instances.py).  A helper module
like its neighbours: no fixture, no pytest setting, nothing that needs a GPU.

The batch is many_gases_cases' for any gas count 1..8: three limb rays of 7, 15 and 23 segments (GEO3) on twelve
coefficient rows, the regime panel of limb_reference.panel_problem on the rows, 300 spectral points (two blocks of 256, the
last wave of the second ragged).  state() is many_gases_cases.state with the counts given instead of a kind's name and
the level gases chosen by rule from n_gas (level_gases); for five and eight gases it returns many_gases_cases' states bit
for bit (kind_spec names them).  references() is many_gases_cases.references with the options of a batch: observer order
(every ray's segments reversed), absorption alone, an initial intensity per launched point.

The yardstick is tests/limb_reference.py as it stands: errors in units of 2^-53 (A + (n_gas + 1) C) + 1e-290, every row
within KERNEL_MARGIN x K_PLAIN, K_PLAIN the distance of plain_fp64 from the reference on the case's own inputs.

K_PLAIN over every case of EXPECTED, measured on the CPU (host_columns, the 188 panel columns, a positive initial
intensity in place of the Planck start): see K_PLAIN_SEEN below, asserted live by tests/test_state_instances_host.py
against K_PLAIN_RAD = 41 and K_PLAIN_JAC = 25.

EXPECTED, the census.  The kernel is compiled as <NG, NP, COLS, ROWS, BANDS, INSTR, pack: SEVERAL, RAYBLK> for every
combination with (BANDS or not INSTR) and (NG >= 2 or not SEVERAL) (sr_limb_state_launch.inc): NG = 1..4 with NP = 8 and
16, NG = 6 and 8 with NP = 8 -- 48 + 3 x 96 + 2 x 48 = 432 instances.  The table lists each of them with the smallest
call that reaches it, written out from these rules of the host path:

  NG      the batch's gas count up to four; five and six gases run NG = 6, seven and eight NG = 8 (by_ngas_state_many).
  NP      16 iff the batch has at most four gases and more than 8 parameter slots -- n_col + n_lev + n_row and, with
          pointing, one hidden slot per gas (level_jac_np); with ray blocks the count is that of the ray touched by the
          most parameters (ray_jac_plan), and a parameter without weights touches none.
  COLS    a call with column parameters or with pointing; and limb_rays_state_jacobian without row parameters and with
          at most one level gas (sr_limb_rays_jac_state_dev: always).  The spectra instance without COLS, ROWS and
          SEVERAL is limb_rays_level_jacobian's ("level").
  ROWS    row parameters.   BANDS  limb_rays_state_bands.   INSTR  ... with instrument=True.
  SEVERAL two level gases in level_gases=.   RAYBLK  ray_blocks=True.

No compiled instance is barred by an argument check: the two conditions of the launcher are the only ones, and every
instance it compiles has a call.  (A call can be refused -- no parameter at all without instrument= or pointing= is -- but
no instance is reached by refused calls alone.)

An entry: (NG, NP, flags, call, n_gas, n_col, levs, n_row, option).  flags: the letters of C(OLS) R(OWS) B(ANDS) I(NSTR)
S(EVERAL) K (RAYBLK), '-' where off; call: "level", "state", "bands" or "instr"; levs: the level parameters of each level
gas; option: None, "observer" (observer order), "solo" (solo_absorption -- of a Planck start: absorption alone of nothing
is nothing), "planck" (a Planck initial intensity under the emission), "g_lo" (the tables a shard of a wider grid) or
"pointing".  Each kind's parameter 1 has no weights where the kind has more than one.  The rules the entries were written
by:
  - every kind a flag asks for has two parameters, the level kind is always there (2, or 2 + 1 with two level gases);
    an entry with pointing has one of each, so that its hidden slots fit a block of eight;
  - the parameter count (hidden slots included) is then raised to its target with column parameters (COLS) or level
    parameters of the first level gas.  With j = C + 2 R + 4 S: NP8 up to four gases -- 8 (a full block) where j + NG is
    even; NP16 -- 12 (nine that touch a ray beside the three without weights, for the plan per ray), but 16 (a full
    block) where (j + NG) mod 8 is 0, 17 (a second block) where it is 4, and 9 (the switch to NP16) where it is 2 and
    the plan is dense; five to eight gases (8 slots whatever the count) -- 8, small, 9, small by j mod 4, 17 for j = 3;
  - the instance without COLS, ROWS, SEVERAL and RAYBLK with INSTR has NO parameter: the plan is one block of unused slots;
  - five to eight gases: NG itself (six real gases, eight) where the number of set flags among C R S is even, NG - 1
    (the padding slot in use) where it is odd;
  - options: (None, observer, solo, None, planck, g_lo, pointing)[(j + NG + 4 [NP = 16]) mod 7]; pointing needs COLS (it
    is COLS) -- an entry without takes None.  Seven is coprime to every flag's stride, so each option meets both settings
    of each flag over the table.
An entry with ray blocks has the state and the option of the one without (their references are shared), unless the count
9 stands in its way; a BANDS or INSTR entry has those of its spectra twin (same NG, NP, C, R, S, K), except the one
without any parameter.
"""
import numpy as np

import limb_reference as R
import many_gases_cases as M

SEED, N_LAYERS, N_PTS, N_SEG, GEO3 = M.SEED, M.N_LAYERS, M.N_PTS, M.N_SEG, M.GEO3
G_LO, N_GRID = 37, M.N_PTS + 100         # option "g_lo": the tables cover points 37 .. 336 of a grid of 400
T_PLANCK = 250.0                         # option "planck": the initial temperature
OPTIONS = (None, "observer", "solo", "planck", "g_lo", "pointing")
FLAGS = "CRBISK"

panel_case, host_columns, host_dcol, path_arrays = M.panel_case, M.host_columns, M.host_dcol, M.path_arrays
pointing_row, k_plain = M.pointing_row, M.k_plain


def level_gases(n_gas, n_lg):
    """[(gas of the batch, levels, rows of its pair tables)] of n_lg level gases in a batch of n_gas: one -- gas 6, or the
    last below seven gases; two -- gas 5, or the last below six, and gas 2, or the last but one below four."""
    if n_lg == 0:
        return []
    if n_lg == 1:
        return [(min(6, n_gas - 1), 5, 14)]
    assert n_lg == 2 and n_gas >= 2
    return [(min(5, n_gas - 1), 4, 13), (min(2, n_gas - 2), 6, 15)]


def state(c, n_col, levs, n_row, seed=None, par_gas=None):
    """many_gases_cases.state by counts: n_col column parameters (gases cycling downwards from n_gas - 1, or par_gas),
    levs[k] level parameters of level gas k of level_gases(n_gas, len(levs)), n_row row parameters.  Parameter 1 of every
    kind has no weights.  seed: the stream of the random numbers (default: one of the counts' own)."""
    n_gas = c["n_gas"]
    N = len(c["names"])
    levs = tuple(levs)
    if seed is None:
        seed = 100 + n_col + 32 * (levs[0] if levs else 0) + 1024 * (levs[1] if len(levs) > 1 else 0) + 32768 * n_row
    rng = np.random.default_rng([SEED, n_gas, seed])
    lg_spec = level_gases(n_gas, len(levs))
    if par_gas is None:
        par_gas = (n_gas - 1 - np.arange(n_col)) % n_gas
    par_gas = np.asarray(par_gas, np.int32)
    assert par_gas.shape == (n_col,)
    seg_w = rng.uniform(0.0, 1.0, (n_col, N_SEG)) * (rng.random((n_col, N_SEG)) < 0.7)
    if n_col > 1:
        seg_w[1] = 0.0
    par_w = np.repeat(seg_w, 2, axis=1) * c["vmr"][par_gas] if n_col else np.zeros((0, 2 * N_SEG))
    lgases, n_lev = [], sum(levs)
    for gas, n_levels, n_tab in lg_spec:
        rows = rng.permutation(n_tab)[:N_LAYERS].astype(np.int32)
        tab = rng.uniform(0.1, 1.0, (n_levels, 2, n_tab, N)) * 1e-18
        w = rng.uniform(0.2, 1.0, (n_levels, 2, N_LAYERS, 1))
        tab[:, 0, rows] = w[:, 0] * c["coef_a"][gas][None]
        tab[:, 1, rows] = w[:, 1] * c["coef_e"][gas][None]
        lgases.append((gas, tab, rows))
    par_lgas = rng.permutation(np.repeat(np.arange(len(levs)), levs)).astype(np.int32) if n_lev else np.zeros(0, np.int32)
    par_level = np.array([rng.integers(0, lg_spec[k][1]) for k in par_lgas], np.int32)
    par_c = rng.uniform(-1.0, 1.0, (n_lev, N_LAYERS)) * (rng.random((n_lev, N_LAYERS)) < 0.7)
    if n_lev > 1:
        par_c[1] = 0.0
    shape = c["coef_a"].shape
    m_a, m_e = rng.uniform(-1.0, 1.0, shape[1:]), rng.uniform(-1.0, 1.0, shape[1:])
    dabs = c["coef_a"] * m_a[None] * rng.uniform(0.5, 1.0, shape)
    demi = c["coef_e"] * m_e[None] * rng.uniform(0.5, 1.0, shape)
    par_t = rng.uniform(-1.0, 1.0, (n_row, N_LAYERS)) * (rng.random((n_row, N_LAYERS)) > 0.3)
    if n_row > 1:
        par_t[1] = 0.0
    out = dict(c)
    out.update(n_col=n_col, n_lev=n_lev, n_row=n_row, levs=levs, par_gas=par_gas, par_w=par_w, lgases=lgases, par_lgas=par_lgas,
               par_level=par_level, par_c=par_c, dabs=dabs, demi=demi, par_t=par_t)
    return out


def kind_spec(n_gas, kind):
    """The arguments of state() that give many_gases_cases.state(c, kind) (five to eight gases: its 'cols' names gas 4)."""
    k = M.KINDS.index(kind)
    n_col, levs, n_row = dict(cols=(5, (), 0), cols9=(9, (), 0), cols17=(17, (), 0), lev6=(4, (5,), 0), lev52=(0, (3, 6), 0),
                              rows=(2, (), 3), all=(4, (3, 3), 3))[kind]
    return dict(n_col=n_col, levs=levs, n_row=n_row, seed=k, par_gas=[n_gas - 1, 4, 0, n_gas - 1, 3] if kind == "cols" else None)


def reversed_rays(s, *arrays):
    """Observer order: the case with every ray's segments listed backwards, and the [., n_seg] arrays likewise (None stays)."""
    so = s["geo"]["seg_off"]
    rev = np.concatenate([np.arange(so[r], so[r + 1])[::-1] for r in range(s["geo"]["n_rays"])])
    return (dict(s, geo=dict(s["geo"], seg_layer=s["geo"]["seg_layer"][rev])),) + tuple(None if a is None else a[:, rev] for a in arrays)


def references(s, col, dcol, I0=None, solo=False, hidden=None, observer=False, at=None):
    """Per ray: (the reference dict of limb_reference.recursion_reference, the plain-fp64 results (I, J)).  at None: on
    the panel's columns, I0 [N] per panel column; at [n_pts]: on the launched points, panel column at[j] at point j, I0
    [n_pts] per point (a Planck start differs from point to point).  I0 None: zeros."""
    if observer:
        s, col, dcol, hidden = reversed_rays(s, col, dcol, hidden)
    sel = (lambda a: a) if at is None else (lambda a: a[..., at])
    I0 = np.zeros(len(s["names"]) if at is None else len(at)) if I0 is None else np.asarray(I0)
    out = []
    for ray in range(s["geo"]["n_rays"]):
        ld = [sel(v) for v in M.ray_forms(s, col, dcol, ray, R.LD, hidden)]
        pl = [sel(v) for v in M.ray_forms(s, col, dcol, ray, np.float64, hidden)]
        ref = R.recursion_reference(*ld, I0, solo=solo, thin_ulps=s["n_gas"] + 1)
        out.append((ref, R.plain_fp64(*pl, I0, solo=solo)))
    return out


# ------------------------------------------------------------------------------------------------------------------
# the census
# ------------------------------------------------------------------------------------------------------------------
def compiled_instances():
    """The set the launcher's rules generate: (NG, NP, flags) of every instance the five state units compile."""
    out = set()
    for ng, nps in ((1, (8, 16)), (2, (8, 16)), (3, (8, 16)), (4, (8, 16)), (6, (8,)), (8, (8,))):
        for n_p in nps:
            for bits in range(64):
                on = [bool(bits >> k & 1) for k in range(6)]
                cols, rows, bands, instr, several, rayblk = on
                if (bands or not instr) and (ng >= 2 or not several):
                    out.add((ng, n_p, "".join(f if v else "-" for f, v in zip(FLAGS, on))))
    return out


def flags_of(inst):
    """(ng, np, cols, rows, bands, instr, several, rayblk) of an engine.StateInstance, as EXPECTED's (NG, NP, flags)."""
    return (int(inst[0]), int(inst[1]), "".join(f if v else "-" for f, v in zip(FLAGS, inst[2:])))


def entry_dict(e):
    ng, n_p, flags, call, n_gas, n_col, levs, n_row, option = e
    return dict(key=(ng, n_p, flags), ng=ng, np=n_p, flags=flags, call=call, n_gas=n_gas, n_col=n_col, levs=levs, n_row=n_row,
                option=option, n_state=n_col + sum(levs) + n_row, ray_blocks="K" in flags,
                twin=(ng, n_p, flags[:2] + "--" + flags[4:]))


def options_of(option):
    """What an option asks of the batch and of the reference: (LimbLOS keywords, solo, observer)."""
    kw = dict(observer=dict(LOS_order="observer"), solo=dict(solo_absorption=True, initial_temperature=T_PLANCK),
              planck=dict(initial_temperature=T_PLANCK))
    return kw.get(option, {}), option == "solo", option == "observer"


def make_los(eng, c, option):
    """The LimbLOS of a case with an option's keywords (pointing: the path arrays)."""
    g = c["geo"]
    kw = dict(options_of(option)[0])
    if option == "pointing":
        kw["path"] = path_arrays(c["n_gas"])
    return eng.LimbLOS(g["seg_off"], g["seg_layer"], g["pt_off"], c["x"], c["nd"], c["vmr"], col_scale=c["col_scale"], **kw)


def call_keywords(s, e, put):
    """The parameter keywords of the engine call of entry e (entry_dict) for its state s; put(array [..., N] on the panel's
    columns) -> the device tensor on the launched points."""
    kw = {}
    if s["n_col"]:
        kw.update(par_gas=s["par_gas"], par_w=s["par_w"])
    if len(s["lgases"]) == 2:
        kw.update(level_gases=[(g, put(tab), rows) for g, tab, rows in s["lgases"]], par_lgas=s["par_lgas"], par_level=s["par_level"],
                  par_c=s["par_c"])
    elif s["n_lev"]:
        gas, tab, rows = s["lgases"][0]
        kw.update(tab=put(tab), coef_row=rows, gas=gas, par_level=s["par_level"], par_c=s["par_c"])
    if s["n_row"]:
        kw.update(dcoeffs=(put(s["dabs"]), put(s["demi"])), par_t=s["par_t"])
    if e["call"] == "level":
        assert set(kw) == {"tab", "coef_row", "gas", "par_level", "par_c"}
    if e["option"] == "pointing":
        kw["pointing"] = True
    return kw


# (NG, NP, flags, call, n_gas, n_col, levs, n_row, option)
EXPECTED = (
    (1, 8, "------", "level", 1, 0, (2,), 0, "observer"),
    (1, 8, "-----K", "level", 1, 0, (2,), 0, "observer"),
    (1, 8, "--B---", "bands", 1, 0, (2,), 0, "observer"),
    (1, 8, "--B--K", "bands", 1, 0, (2,), 0, "observer"),
    (1, 8, "--BI--", "instr", 1, 0, (), 0, "observer"),
    (1, 8, "--BI-K", "instr", 1, 0, (2,), 0, "observer"),
    (1, 8, "-R----", "state", 1, 0, (2,), 2, None),
    (1, 8, "-R---K", "state", 1, 0, (2,), 2, None),
    (1, 8, "-RB---", "bands", 1, 0, (2,), 2, None),
    (1, 8, "-RB--K", "bands", 1, 0, (2,), 2, None),
    (1, 8, "-RBI--", "instr", 1, 0, (2,), 2, None),
    (1, 8, "-RBI-K", "instr", 1, 0, (2,), 2, None),
    (1, 8, "C-----", "state", 1, 6, (2,), 0, "solo"),
    (1, 8, "C----K", "state", 1, 6, (2,), 0, "solo"),
    (1, 8, "C-B---", "bands", 1, 6, (2,), 0, "solo"),
    (1, 8, "C-B--K", "bands", 1, 6, (2,), 0, "solo"),
    (1, 8, "C-BI--", "instr", 1, 6, (2,), 0, "solo"),
    (1, 8, "C-BI-K", "instr", 1, 6, (2,), 0, "solo"),
    (1, 8, "CR----", "state", 1, 4, (2,), 2, "planck"),
    (1, 8, "CR---K", "state", 1, 4, (2,), 2, "planck"),
    (1, 8, "CRB---", "bands", 1, 4, (2,), 2, "planck"),
    (1, 8, "CRB--K", "bands", 1, 4, (2,), 2, "planck"),
    (1, 8, "CRBI--", "instr", 1, 4, (2,), 2, "planck"),
    (1, 8, "CRBI-K", "instr", 1, 4, (2,), 2, "planck"),
    (1, 16, "------", "level", 1, 0, (12,), 0, "g_lo"),
    (1, 16, "-----K", "level", 1, 0, (12,), 0, "g_lo"),
    (1, 16, "--B---", "bands", 1, 0, (12,), 0, "g_lo"),
    (1, 16, "--B--K", "bands", 1, 0, (12,), 0, "g_lo"),
    (1, 16, "--BI--", "instr", 1, 0, (12,), 0, "g_lo"),
    (1, 16, "--BI-K", "instr", 1, 0, (12,), 0, "g_lo"),
    (1, 16, "-R----", "state", 1, 0, (10,), 2, None),
    (1, 16, "-R---K", "state", 1, 0, (10,), 2, None),
    (1, 16, "-RB---", "bands", 1, 0, (10,), 2, None),
    (1, 16, "-RB--K", "bands", 1, 0, (10,), 2, None),
    (1, 16, "-RBI--", "instr", 1, 0, (10,), 2, None),
    (1, 16, "-RBI-K", "instr", 1, 0, (10,), 2, None),
    (1, 16, "C-----", "state", 1, 7, (1,), 0, "pointing"),
    (1, 16, "C----K", "state", 1, 10, (1,), 0, "pointing"),
    (1, 16, "C-B---", "bands", 1, 7, (1,), 0, "pointing"),
    (1, 16, "C-B--K", "bands", 1, 10, (1,), 0, "pointing"),
    (1, 16, "C-BI--", "instr", 1, 7, (1,), 0, "pointing"),
    (1, 16, "C-BI-K", "instr", 1, 10, (1,), 0, "pointing"),
    (1, 16, "CR----", "state", 1, 13, (2,), 2, "observer"),
    (1, 16, "CR---K", "state", 1, 13, (2,), 2, "observer"),
    (1, 16, "CRB---", "bands", 1, 13, (2,), 2, "observer"),
    (1, 16, "CRB--K", "bands", 1, 13, (2,), 2, "observer"),
    (1, 16, "CRBI--", "instr", 1, 13, (2,), 2, "observer"),
    (1, 16, "CRBI-K", "instr", 1, 13, (2,), 2, "observer"),
    (2, 8, "------", "level", 2, 0, (8,), 0, "solo"),
    (2, 8, "-----K", "level", 2, 0, (8,), 0, "solo"),
    (2, 8, "----S-", "state", 2, 0, (7, 1), 0, None),
    (2, 8, "----SK", "state", 2, 0, (7, 1), 0, None),
    (2, 8, "--B---", "bands", 2, 0, (8,), 0, "solo"),
    (2, 8, "--B--K", "bands", 2, 0, (8,), 0, "solo"),
    (2, 8, "--B-S-", "bands", 2, 0, (7, 1), 0, None),
    (2, 8, "--B-SK", "bands", 2, 0, (7, 1), 0, None),
    (2, 8, "--BI--", "instr", 2, 0, (), 0, "solo"),
    (2, 8, "--BI-K", "instr", 2, 0, (8,), 0, "solo"),
    (2, 8, "--BIS-", "instr", 2, 0, (7, 1), 0, None),
    (2, 8, "--BISK", "instr", 2, 0, (7, 1), 0, None),
    (2, 8, "-R----", "state", 2, 0, (6,), 2, "planck"),
    (2, 8, "-R---K", "state", 2, 0, (6,), 2, "planck"),
    (2, 8, "-R--S-", "state", 2, 0, (5, 1), 2, "observer"),
    (2, 8, "-R--SK", "state", 2, 0, (5, 1), 2, "observer"),
    (2, 8, "-RB---", "bands", 2, 0, (6,), 2, "planck"),
    (2, 8, "-RB--K", "bands", 2, 0, (6,), 2, "planck"),
    (2, 8, "-RB-S-", "bands", 2, 0, (5, 1), 2, "observer"),
    (2, 8, "-RB-SK", "bands", 2, 0, (5, 1), 2, "observer"),
    (2, 8, "-RBI--", "instr", 2, 0, (6,), 2, "planck"),
    (2, 8, "-RBI-K", "instr", 2, 0, (6,), 2, "planck"),
    (2, 8, "-RBIS-", "instr", 2, 0, (5, 1), 2, "observer"),
    (2, 8, "-RBISK", "instr", 2, 0, (5, 1), 2, "observer"),
    (2, 8, "C-----", "state", 2, 2, (2,), 0, None),
    (2, 8, "C----K", "state", 2, 2, (2,), 0, None),
    (2, 8, "C---S-", "state", 2, 2, (2, 1), 0, None),
    (2, 8, "C---SK", "state", 2, 2, (2, 1), 0, None),
    (2, 8, "C-B---", "bands", 2, 2, (2,), 0, None),
    (2, 8, "C-B--K", "bands", 2, 2, (2,), 0, None),
    (2, 8, "C-B-S-", "bands", 2, 2, (2, 1), 0, None),
    (2, 8, "C-B-SK", "bands", 2, 2, (2, 1), 0, None),
    (2, 8, "C-BI--", "instr", 2, 2, (2,), 0, None),
    (2, 8, "C-BI-K", "instr", 2, 2, (2,), 0, None),
    (2, 8, "C-BIS-", "instr", 2, 2, (2, 1), 0, None),
    (2, 8, "C-BISK", "instr", 2, 2, (2, 1), 0, None),
    (2, 8, "CR----", "state", 2, 2, (2,), 2, "g_lo"),
    (2, 8, "CR---K", "state", 2, 2, (2,), 2, "g_lo"),
    (2, 8, "CR--S-", "state", 2, 2, (2, 1), 2, "solo"),
    (2, 8, "CR--SK", "state", 2, 2, (2, 1), 2, "solo"),
    (2, 8, "CRB---", "bands", 2, 2, (2,), 2, "g_lo"),
    (2, 8, "CRB--K", "bands", 2, 2, (2,), 2, "g_lo"),
    (2, 8, "CRB-S-", "bands", 2, 2, (2, 1), 2, "solo"),
    (2, 8, "CRB-SK", "bands", 2, 2, (2, 1), 2, "solo"),
    (2, 8, "CRBI--", "instr", 2, 2, (2,), 2, "g_lo"),
    (2, 8, "CRBI-K", "instr", 2, 2, (2,), 2, "g_lo"),
    (2, 8, "CRBIS-", "instr", 2, 2, (2, 1), 2, "solo"),
    (2, 8, "CRBISK", "instr", 2, 2, (2, 1), 2, "solo"),
    (2, 16, "------", "level", 2, 0, (9,), 0, None),
    (2, 16, "-----K", "level", 2, 0, (12,), 0, None),
    (2, 16, "----S-", "state", 2, 0, (11, 1), 0, None),
    (2, 16, "----SK", "state", 2, 0, (11, 1), 0, None),
    (2, 16, "--B---", "bands", 2, 0, (9,), 0, None),
    (2, 16, "--B--K", "bands", 2, 0, (12,), 0, None),
    (2, 16, "--B-S-", "bands", 2, 0, (11, 1), 0, None),
    (2, 16, "--B-SK", "bands", 2, 0, (11, 1), 0, None),
    (2, 16, "--BI--", "instr", 2, 0, (9,), 0, None),
    (2, 16, "--BI-K", "instr", 2, 0, (12,), 0, None),
    (2, 16, "--BIS-", "instr", 2, 0, (11, 1), 0, None),
    (2, 16, "--BISK", "instr", 2, 0, (11, 1), 0, None),
    (2, 16, "-R----", "state", 2, 0, (15,), 2, "observer"),
    (2, 16, "-R---K", "state", 2, 0, (15,), 2, "observer"),
    (2, 16, "-R--S-", "state", 2, 0, (13, 1), 2, "g_lo"),
    (2, 16, "-R--SK", "state", 2, 0, (13, 1), 2, "g_lo"),
    (2, 16, "-RB---", "bands", 2, 0, (15,), 2, "observer"),
    (2, 16, "-RB--K", "bands", 2, 0, (15,), 2, "observer"),
    (2, 16, "-RB-S-", "bands", 2, 0, (13, 1), 2, "g_lo"),
    (2, 16, "-RB-SK", "bands", 2, 0, (13, 1), 2, "g_lo"),
    (2, 16, "-RBI--", "instr", 2, 0, (15,), 2, "observer"),
    (2, 16, "-RBI-K", "instr", 2, 0, (15,), 2, "observer"),
    (2, 16, "-RBIS-", "instr", 2, 0, (13, 1), 2, "g_lo"),
    (2, 16, "-RBISK", "instr", 2, 0, (13, 1), 2, "g_lo"),
    (2, 16, "C-----", "state", 2, 10, (2,), 0, None),
    (2, 16, "C----K", "state", 2, 10, (2,), 0, None),
    (2, 16, "C---S-", "state", 2, 9, (2, 1), 0, "planck"),
    (2, 16, "C---SK", "state", 2, 9, (2, 1), 0, "planck"),
    (2, 16, "C-B---", "bands", 2, 10, (2,), 0, None),
    (2, 16, "C-B--K", "bands", 2, 10, (2,), 0, None),
    (2, 16, "C-B-S-", "bands", 2, 9, (2, 1), 0, "planck"),
    (2, 16, "C-B-SK", "bands", 2, 9, (2, 1), 0, "planck"),
    (2, 16, "C-BI--", "instr", 2, 10, (2,), 0, None),
    (2, 16, "C-BI-K", "instr", 2, 10, (2,), 0, None),
    (2, 16, "C-BIS-", "instr", 2, 9, (2, 1), 0, "planck"),
    (2, 16, "C-BISK", "instr", 2, 9, (2, 1), 0, "planck"),
    (2, 16, "CR----", "state", 2, 8, (2,), 2, "solo"),
    (2, 16, "CR---K", "state", 2, 8, (2,), 2, "solo"),
    (2, 16, "CR--S-", "state", 2, 7, (1, 1), 1, "pointing"),
    (2, 16, "CR--SK", "state", 2, 7, (1, 1), 1, "pointing"),
    (2, 16, "CRB---", "bands", 2, 8, (2,), 2, "solo"),
    (2, 16, "CRB--K", "bands", 2, 8, (2,), 2, "solo"),
    (2, 16, "CRB-S-", "bands", 2, 7, (1, 1), 1, "pointing"),
    (2, 16, "CRB-SK", "bands", 2, 7, (1, 1), 1, "pointing"),
    (2, 16, "CRBI--", "instr", 2, 8, (2,), 2, "solo"),
    (2, 16, "CRBI-K", "instr", 2, 8, (2,), 2, "solo"),
    (2, 16, "CRBIS-", "instr", 2, 7, (1, 1), 1, "pointing"),
    (2, 16, "CRBISK", "instr", 2, 7, (1, 1), 1, "pointing"),
    (3, 8, "------", "level", 3, 0, (2,), 0, None),
    (3, 8, "-----K", "level", 3, 0, (2,), 0, None),
    (3, 8, "----S-", "state", 3, 0, (2, 1), 0, None),
    (3, 8, "----SK", "state", 3, 0, (2, 1), 0, None),
    (3, 8, "--B---", "bands", 3, 0, (2,), 0, None),
    (3, 8, "--B--K", "bands", 3, 0, (2,), 0, None),
    (3, 8, "--B-S-", "bands", 3, 0, (2, 1), 0, None),
    (3, 8, "--B-SK", "bands", 3, 0, (2, 1), 0, None),
    (3, 8, "--BI--", "instr", 3, 0, (), 0, None),
    (3, 8, "--BI-K", "instr", 3, 0, (2,), 0, None),
    (3, 8, "--BIS-", "instr", 3, 0, (2, 1), 0, None),
    (3, 8, "--BISK", "instr", 3, 0, (2, 1), 0, None),
    (3, 8, "-R----", "state", 3, 0, (2,), 2, "g_lo"),
    (3, 8, "-R---K", "state", 3, 0, (2,), 2, "g_lo"),
    (3, 8, "-R--S-", "state", 3, 0, (2, 1), 2, "solo"),
    (3, 8, "-R--SK", "state", 3, 0, (2, 1), 2, "solo"),
    (3, 8, "-RB---", "bands", 3, 0, (2,), 2, "g_lo"),
    (3, 8, "-RB--K", "bands", 3, 0, (2,), 2, "g_lo"),
    (3, 8, "-RB-S-", "bands", 3, 0, (2, 1), 2, "solo"),
    (3, 8, "-RB-SK", "bands", 3, 0, (2, 1), 2, "solo"),
    (3, 8, "-RBI--", "instr", 3, 0, (2,), 2, "g_lo"),
    (3, 8, "-RBI-K", "instr", 3, 0, (2,), 2, "g_lo"),
    (3, 8, "-RBIS-", "instr", 3, 0, (2, 1), 2, "solo"),
    (3, 8, "-RBISK", "instr", 3, 0, (2, 1), 2, "solo"),
    (3, 8, "C-----", "state", 3, 6, (2,), 0, "planck"),
    (3, 8, "C----K", "state", 3, 6, (2,), 0, "planck"),
    (3, 8, "C---S-", "state", 3, 5, (2, 1), 0, "observer"),
    (3, 8, "C---SK", "state", 3, 5, (2, 1), 0, "observer"),
    (3, 8, "C-B---", "bands", 3, 6, (2,), 0, "planck"),
    (3, 8, "C-B--K", "bands", 3, 6, (2,), 0, "planck"),
    (3, 8, "C-B-S-", "bands", 3, 5, (2, 1), 0, "observer"),
    (3, 8, "C-B-SK", "bands", 3, 5, (2, 1), 0, "observer"),
    (3, 8, "C-BI--", "instr", 3, 6, (2,), 0, "planck"),
    (3, 8, "C-BI-K", "instr", 3, 6, (2,), 0, "planck"),
    (3, 8, "C-BIS-", "instr", 3, 5, (2, 1), 0, "observer"),
    (3, 8, "C-BISK", "instr", 3, 5, (2, 1), 0, "observer"),
    (3, 8, "CR----", "state", 3, 3, (1,), 1, "pointing"),
    (3, 8, "CR---K", "state", 3, 3, (1,), 1, "pointing"),
    (3, 8, "CR--S-", "state", 3, 3, (2, 1), 2, None),
    (3, 8, "CR--SK", "state", 3, 3, (2, 1), 2, None),
    (3, 8, "CRB---", "bands", 3, 3, (1,), 1, "pointing"),
    (3, 8, "CRB--K", "bands", 3, 3, (1,), 1, "pointing"),
    (3, 8, "CRB-S-", "bands", 3, 3, (2, 1), 2, None),
    (3, 8, "CRB-SK", "bands", 3, 3, (2, 1), 2, None),
    (3, 8, "CRBI--", "instr", 3, 3, (1,), 1, "pointing"),
    (3, 8, "CRBI-K", "instr", 3, 3, (1,), 1, "pointing"),
    (3, 8, "CRBIS-", "instr", 3, 3, (2, 1), 2, None),
    (3, 8, "CRBISK", "instr", 3, 3, (2, 1), 2, None),
    (3, 16, "------", "level", 3, 0, (12,), 0, None),
    (3, 16, "-----K", "level", 3, 0, (12,), 0, None),
    (3, 16, "----S-", "state", 3, 0, (11, 1), 0, "planck"),
    (3, 16, "----SK", "state", 3, 0, (11, 1), 0, "planck"),
    (3, 16, "--B---", "bands", 3, 0, (12,), 0, None),
    (3, 16, "--B--K", "bands", 3, 0, (12,), 0, None),
    (3, 16, "--B-S-", "bands", 3, 0, (11, 1), 0, "planck"),
    (3, 16, "--B-SK", "bands", 3, 0, (11, 1), 0, "planck"),
    (3, 16, "--BI--", "instr", 3, 0, (12,), 0, None),
    (3, 16, "--BI-K", "instr", 3, 0, (12,), 0, None),
    (3, 16, "--BIS-", "instr", 3, 0, (11, 1), 0, "planck"),
    (3, 16, "--BISK", "instr", 3, 0, (11, 1), 0, "planck"),
    (3, 16, "-R----", "state", 3, 0, (10,), 2, "solo"),
    (3, 16, "-R---K", "state", 3, 0, (10,), 2, "solo"),
    (3, 16, "-R--S-", "state", 3, 0, (9, 1), 2, None),
    (3, 16, "-R--SK", "state", 3, 0, (9, 1), 2, None),
    (3, 16, "-RB---", "bands", 3, 0, (10,), 2, "solo"),
    (3, 16, "-RB--K", "bands", 3, 0, (10,), 2, "solo"),
    (3, 16, "-RB-S-", "bands", 3, 0, (9, 1), 2, None),
    (3, 16, "-RB-SK", "bands", 3, 0, (9, 1), 2, None),
    (3, 16, "-RBI--", "instr", 3, 0, (10,), 2, "solo"),
    (3, 16, "-RBI-K", "instr", 3, 0, (10,), 2, "solo"),
    (3, 16, "-RBIS-", "instr", 3, 0, (9, 1), 2, None),
    (3, 16, "-RBISK", "instr", 3, 0, (9, 1), 2, None),
    (3, 16, "C-----", "state", 3, 15, (2,), 0, "observer"),
    (3, 16, "C----K", "state", 3, 15, (2,), 0, "observer"),
    (3, 16, "C---S-", "state", 3, 13, (2, 1), 0, "g_lo"),
    (3, 16, "C---SK", "state", 3, 13, (2, 1), 0, "g_lo"),
    (3, 16, "C-B---", "bands", 3, 15, (2,), 0, "observer"),
    (3, 16, "C-B--K", "bands", 3, 15, (2,), 0, "observer"),
    (3, 16, "C-B-S-", "bands", 3, 13, (2, 1), 0, "g_lo"),
    (3, 16, "C-B-SK", "bands", 3, 13, (2, 1), 0, "g_lo"),
    (3, 16, "C-BI--", "instr", 3, 15, (2,), 0, "observer"),
    (3, 16, "C-BI-K", "instr", 3, 15, (2,), 0, "observer"),
    (3, 16, "C-BIS-", "instr", 3, 13, (2, 1), 0, "g_lo"),
    (3, 16, "C-BISK", "instr", 3, 13, (2, 1), 0, "g_lo"),
    (3, 16, "CR----", "state", 3, 8, (2,), 2, None),
    (3, 16, "CR---K", "state", 3, 8, (2,), 2, None),
    (3, 16, "CR--S-", "state", 3, 4, (2, 1), 2, None),
    (3, 16, "CR--SK", "state", 3, 7, (2, 1), 2, None),
    (3, 16, "CRB---", "bands", 3, 8, (2,), 2, None),
    (3, 16, "CRB--K", "bands", 3, 8, (2,), 2, None),
    (3, 16, "CRB-S-", "bands", 3, 4, (2, 1), 2, None),
    (3, 16, "CRB-SK", "bands", 3, 7, (2, 1), 2, None),
    (3, 16, "CRBI--", "instr", 3, 8, (2,), 2, None),
    (3, 16, "CRBI-K", "instr", 3, 8, (2,), 2, None),
    (3, 16, "CRBIS-", "instr", 3, 4, (2, 1), 2, None),
    (3, 16, "CRBISK", "instr", 3, 7, (2, 1), 2, None),
    (4, 8, "------", "level", 4, 0, (8,), 0, "planck"),
    (4, 8, "-----K", "level", 4, 0, (8,), 0, "planck"),
    (4, 8, "----S-", "state", 4, 0, (7, 1), 0, "observer"),
    (4, 8, "----SK", "state", 4, 0, (7, 1), 0, "observer"),
    (4, 8, "--B---", "bands", 4, 0, (8,), 0, "planck"),
    (4, 8, "--B--K", "bands", 4, 0, (8,), 0, "planck"),
    (4, 8, "--B-S-", "bands", 4, 0, (7, 1), 0, "observer"),
    (4, 8, "--B-SK", "bands", 4, 0, (7, 1), 0, "observer"),
    (4, 8, "--BI--", "instr", 4, 0, (), 0, "planck"),
    (4, 8, "--BI-K", "instr", 4, 0, (8,), 0, "planck"),
    (4, 8, "--BIS-", "instr", 4, 0, (7, 1), 0, "observer"),
    (4, 8, "--BISK", "instr", 4, 0, (7, 1), 0, "observer"),
    (4, 8, "-R----", "state", 4, 0, (6,), 2, None),
    (4, 8, "-R---K", "state", 4, 0, (6,), 2, None),
    (4, 8, "-R--S-", "state", 4, 0, (5, 1), 2, None),
    (4, 8, "-R--SK", "state", 4, 0, (5, 1), 2, None),
    (4, 8, "-RB---", "bands", 4, 0, (6,), 2, None),
    (4, 8, "-RB--K", "bands", 4, 0, (6,), 2, None),
    (4, 8, "-RB-S-", "bands", 4, 0, (5, 1), 2, None),
    (4, 8, "-RB-SK", "bands", 4, 0, (5, 1), 2, None),
    (4, 8, "-RBI--", "instr", 4, 0, (6,), 2, None),
    (4, 8, "-RBI-K", "instr", 4, 0, (6,), 2, None),
    (4, 8, "-RBIS-", "instr", 4, 0, (5, 1), 2, None),
    (4, 8, "-RBISK", "instr", 4, 0, (5, 1), 2, None),
    (4, 8, "C-----", "state", 4, 2, (2,), 0, "g_lo"),
    (4, 8, "C----K", "state", 4, 2, (2,), 0, "g_lo"),
    (4, 8, "C---S-", "state", 4, 2, (2, 1), 0, "solo"),
    (4, 8, "C---SK", "state", 4, 2, (2, 1), 0, "solo"),
    (4, 8, "C-B---", "bands", 4, 2, (2,), 0, "g_lo"),
    (4, 8, "C-B--K", "bands", 4, 2, (2,), 0, "g_lo"),
    (4, 8, "C-B-S-", "bands", 4, 2, (2, 1), 0, "solo"),
    (4, 8, "C-B-SK", "bands", 4, 2, (2, 1), 0, "solo"),
    (4, 8, "C-BI--", "instr", 4, 2, (2,), 0, "g_lo"),
    (4, 8, "C-BI-K", "instr", 4, 2, (2,), 0, "g_lo"),
    (4, 8, "C-BIS-", "instr", 4, 2, (2, 1), 0, "solo"),
    (4, 8, "C-BISK", "instr", 4, 2, (2, 1), 0, "solo"),
    (4, 8, "CR----", "state", 4, 2, (2,), 2, None),
    (4, 8, "CR---K", "state", 4, 2, (2,), 2, None),
    (4, 8, "CR--S-", "state", 4, 2, (2, 1), 2, "planck"),
    (4, 8, "CR--SK", "state", 4, 2, (2, 1), 2, "planck"),
    (4, 8, "CRB---", "bands", 4, 2, (2,), 2, None),
    (4, 8, "CRB--K", "bands", 4, 2, (2,), 2, None),
    (4, 8, "CRB-S-", "bands", 4, 2, (2, 1), 2, "planck"),
    (4, 8, "CRB-SK", "bands", 4, 2, (2, 1), 2, "planck"),
    (4, 8, "CRBI--", "instr", 4, 2, (2,), 2, None),
    (4, 8, "CRBI-K", "instr", 4, 2, (2,), 2, None),
    (4, 8, "CRBIS-", "instr", 4, 2, (2, 1), 2, "planck"),
    (4, 8, "CRBISK", "instr", 4, 2, (2, 1), 2, "planck"),
    (4, 16, "------", "level", 4, 0, (17,), 0, "observer"),
    (4, 16, "-----K", "level", 4, 0, (17,), 0, "observer"),
    (4, 16, "----S-", "state", 4, 0, (15, 1), 0, "g_lo"),
    (4, 16, "----SK", "state", 4, 0, (15, 1), 0, "g_lo"),
    (4, 16, "--B---", "bands", 4, 0, (17,), 0, "observer"),
    (4, 16, "--B--K", "bands", 4, 0, (17,), 0, "observer"),
    (4, 16, "--B-S-", "bands", 4, 0, (15, 1), 0, "g_lo"),
    (4, 16, "--B-SK", "bands", 4, 0, (15, 1), 0, "g_lo"),
    (4, 16, "--BI--", "instr", 4, 0, (17,), 0, "observer"),
    (4, 16, "--BI-K", "instr", 4, 0, (17,), 0, "observer"),
    (4, 16, "--BIS-", "instr", 4, 0, (15, 1), 0, "g_lo"),
    (4, 16, "--BISK", "instr", 4, 0, (15, 1), 0, "g_lo"),
    (4, 16, "-R----", "state", 4, 0, (10,), 2, None),
    (4, 16, "-R---K", "state", 4, 0, (10,), 2, None),
    (4, 16, "-R--S-", "state", 4, 0, (6, 1), 2, None),
    (4, 16, "-R--SK", "state", 4, 0, (9, 1), 2, None),
    (4, 16, "-RB---", "bands", 4, 0, (10,), 2, None),
    (4, 16, "-RB--K", "bands", 4, 0, (10,), 2, None),
    (4, 16, "-RB-S-", "bands", 4, 0, (6, 1), 2, None),
    (4, 16, "-RB-SK", "bands", 4, 0, (9, 1), 2, None),
    (4, 16, "-RBI--", "instr", 4, 0, (10,), 2, None),
    (4, 16, "-RBI-K", "instr", 4, 0, (10,), 2, None),
    (4, 16, "-RBIS-", "instr", 4, 0, (6, 1), 2, None),
    (4, 16, "-RBISK", "instr", 4, 0, (9, 1), 2, None),
    (4, 16, "C-----", "state", 4, 10, (2,), 0, "solo"),
    (4, 16, "C----K", "state", 4, 10, (2,), 0, "solo"),
    (4, 16, "C---S-", "state", 4, 6, (1, 1), 0, "pointing"),
    (4, 16, "C---SK", "state", 4, 6, (1, 1), 0, "pointing"),
    (4, 16, "C-B---", "bands", 4, 10, (2,), 0, "solo"),
    (4, 16, "C-B--K", "bands", 4, 10, (2,), 0, "solo"),
    (4, 16, "C-B-S-", "bands", 4, 6, (1, 1), 0, "pointing"),
    (4, 16, "C-B-SK", "bands", 4, 6, (1, 1), 0, "pointing"),
    (4, 16, "C-BI--", "instr", 4, 10, (2,), 0, "solo"),
    (4, 16, "C-BI-K", "instr", 4, 10, (2,), 0, "solo"),
    (4, 16, "C-BIS-", "instr", 4, 6, (1, 1), 0, "pointing"),
    (4, 16, "C-BISK", "instr", 4, 6, (1, 1), 0, "pointing"),
    (4, 16, "CR----", "state", 4, 8, (2,), 2, "planck"),
    (4, 16, "CR---K", "state", 4, 8, (2,), 2, "planck"),
    (4, 16, "CR--S-", "state", 4, 7, (2, 1), 2, "observer"),
    (4, 16, "CR--SK", "state", 4, 7, (2, 1), 2, "observer"),
    (4, 16, "CRB---", "bands", 4, 8, (2,), 2, "planck"),
    (4, 16, "CRB--K", "bands", 4, 8, (2,), 2, "planck"),
    (4, 16, "CRB-S-", "bands", 4, 7, (2, 1), 2, "observer"),
    (4, 16, "CRB-SK", "bands", 4, 7, (2, 1), 2, "observer"),
    (4, 16, "CRBI--", "instr", 4, 8, (2,), 2, "planck"),
    (4, 16, "CRBI-K", "instr", 4, 8, (2,), 2, "planck"),
    (4, 16, "CRBIS-", "instr", 4, 7, (2, 1), 2, "observer"),
    (4, 16, "CRBISK", "instr", 4, 7, (2, 1), 2, "observer"),
    (6, 8, "------", "level", 6, 0, (8,), 0, None),
    (6, 8, "-----K", "level", 6, 0, (8,), 0, None),
    (6, 8, "----S-", "state", 5, 0, (7, 1), 0, None),
    (6, 8, "----SK", "state", 5, 0, (7, 1), 0, None),
    (6, 8, "--B---", "bands", 6, 0, (8,), 0, None),
    (6, 8, "--B--K", "bands", 6, 0, (8,), 0, None),
    (6, 8, "--B-S-", "bands", 5, 0, (7, 1), 0, None),
    (6, 8, "--B-SK", "bands", 5, 0, (7, 1), 0, None),
    (6, 8, "--BI--", "instr", 6, 0, (), 0, None),
    (6, 8, "--BI-K", "instr", 6, 0, (8,), 0, None),
    (6, 8, "--BIS-", "instr", 5, 0, (7, 1), 0, None),
    (6, 8, "--BISK", "instr", 5, 0, (7, 1), 0, None),
    (6, 8, "-R----", "state", 5, 0, (7,), 2, "observer"),
    (6, 8, "-R---K", "state", 5, 0, (7,), 2, "observer"),
    (6, 8, "-R--S-", "state", 6, 0, (6, 1), 2, "g_lo"),
    (6, 8, "-R--SK", "state", 6, 0, (6, 1), 2, "g_lo"),
    (6, 8, "-RB---", "bands", 5, 0, (7,), 2, "observer"),
    (6, 8, "-RB--K", "bands", 5, 0, (7,), 2, "observer"),
    (6, 8, "-RB-S-", "bands", 6, 0, (6, 1), 2, "g_lo"),
    (6, 8, "-RB-SK", "bands", 6, 0, (6, 1), 2, "g_lo"),
    (6, 8, "-RBI--", "instr", 5, 0, (7,), 2, "observer"),
    (6, 8, "-RBI-K", "instr", 5, 0, (7,), 2, "observer"),
    (6, 8, "-RBIS-", "instr", 6, 0, (6, 1), 2, "g_lo"),
    (6, 8, "-RBISK", "instr", 6, 0, (6, 1), 2, "g_lo"),
    (6, 8, "C-----", "state", 5, 2, (2,), 0, None),
    (6, 8, "C----K", "state", 5, 2, (2,), 0, None),
    (6, 8, "C---S-", "state", 6, 2, (2, 1), 0, "planck"),
    (6, 8, "C---SK", "state", 6, 2, (2, 1), 0, "planck"),
    (6, 8, "C-B---", "bands", 5, 2, (2,), 0, None),
    (6, 8, "C-B--K", "bands", 5, 2, (2,), 0, None),
    (6, 8, "C-B-S-", "bands", 6, 2, (2, 1), 0, "planck"),
    (6, 8, "C-B-SK", "bands", 6, 2, (2, 1), 0, "planck"),
    (6, 8, "C-BI--", "instr", 5, 2, (2,), 0, None),
    (6, 8, "C-BI-K", "instr", 5, 2, (2,), 0, None),
    (6, 8, "C-BIS-", "instr", 6, 2, (2, 1), 0, "planck"),
    (6, 8, "C-BISK", "instr", 6, 2, (2, 1), 0, "planck"),
    (6, 8, "CR----", "state", 6, 13, (2,), 2, "solo"),
    (6, 8, "CR---K", "state", 6, 13, (2,), 2, "solo"),
    (6, 8, "CR--S-", "state", 5, 1, (1, 1), 1, "pointing"),
    (6, 8, "CR--SK", "state", 5, 1, (1, 1), 1, "pointing"),
    (6, 8, "CRB---", "bands", 6, 13, (2,), 2, "solo"),
    (6, 8, "CRB--K", "bands", 6, 13, (2,), 2, "solo"),
    (6, 8, "CRB-S-", "bands", 5, 1, (1, 1), 1, "pointing"),
    (6, 8, "CRB-SK", "bands", 5, 1, (1, 1), 1, "pointing"),
    (6, 8, "CRBI--", "instr", 6, 13, (2,), 2, "solo"),
    (6, 8, "CRBI-K", "instr", 6, 13, (2,), 2, "solo"),
    (6, 8, "CRBIS-", "instr", 5, 1, (1, 1), 1, "pointing"),
    (6, 8, "CRBISK", "instr", 5, 1, (1, 1), 1, "pointing"),
    (8, 8, "------", "level", 8, 0, (8,), 0, "observer"),
    (8, 8, "-----K", "level", 8, 0, (8,), 0, "observer"),
    (8, 8, "----S-", "state", 7, 0, (7, 1), 0, "g_lo"),
    (8, 8, "----SK", "state", 7, 0, (7, 1), 0, "g_lo"),
    (8, 8, "--B---", "bands", 8, 0, (8,), 0, "observer"),
    (8, 8, "--B--K", "bands", 8, 0, (8,), 0, "observer"),
    (8, 8, "--B-S-", "bands", 7, 0, (7, 1), 0, "g_lo"),
    (8, 8, "--B-SK", "bands", 7, 0, (7, 1), 0, "g_lo"),
    (8, 8, "--BI--", "instr", 8, 0, (), 0, "observer"),
    (8, 8, "--BI-K", "instr", 8, 0, (8,), 0, "observer"),
    (8, 8, "--BIS-", "instr", 7, 0, (7, 1), 0, "g_lo"),
    (8, 8, "--BISK", "instr", 7, 0, (7, 1), 0, "g_lo"),
    (8, 8, "-R----", "state", 7, 0, (7,), 2, None),
    (8, 8, "-R---K", "state", 7, 0, (7,), 2, None),
    (8, 8, "-R--S-", "state", 8, 0, (6, 1), 2, None),
    (8, 8, "-R--SK", "state", 8, 0, (6, 1), 2, None),
    (8, 8, "-RB---", "bands", 7, 0, (7,), 2, None),
    (8, 8, "-RB--K", "bands", 7, 0, (7,), 2, None),
    (8, 8, "-RB-S-", "bands", 8, 0, (6, 1), 2, None),
    (8, 8, "-RB-SK", "bands", 8, 0, (6, 1), 2, None),
    (8, 8, "-RBI--", "instr", 7, 0, (7,), 2, None),
    (8, 8, "-RBI-K", "instr", 7, 0, (7,), 2, None),
    (8, 8, "-RBIS-", "instr", 8, 0, (6, 1), 2, None),
    (8, 8, "-RBISK", "instr", 8, 0, (6, 1), 2, None),
    (8, 8, "C-----", "state", 7, 2, (2,), 0, "solo"),
    (8, 8, "C----K", "state", 7, 2, (2,), 0, "solo"),
    (8, 8, "C---S-", "state", 8, 1, (1, 1), 0, "pointing"),
    (8, 8, "C---SK", "state", 8, 1, (1, 1), 0, "pointing"),
    (8, 8, "C-B---", "bands", 7, 2, (2,), 0, "solo"),
    (8, 8, "C-B--K", "bands", 7, 2, (2,), 0, "solo"),
    (8, 8, "C-B-S-", "bands", 8, 1, (1, 1), 0, "pointing"),
    (8, 8, "C-B-SK", "bands", 8, 1, (1, 1), 0, "pointing"),
    (8, 8, "C-BI--", "instr", 7, 2, (2,), 0, "solo"),
    (8, 8, "C-BI-K", "instr", 7, 2, (2,), 0, "solo"),
    (8, 8, "C-BIS-", "instr", 8, 1, (1, 1), 0, "pointing"),
    (8, 8, "C-BISK", "instr", 8, 1, (1, 1), 0, "pointing"),
    (8, 8, "CR----", "state", 8, 13, (2,), 2, "planck"),
    (8, 8, "CR---K", "state", 8, 13, (2,), 2, "planck"),
    (8, 8, "CR--S-", "state", 7, 2, (2, 1), 2, "observer"),
    (8, 8, "CR--SK", "state", 7, 2, (2, 1), 2, "observer"),
    (8, 8, "CRB---", "bands", 8, 13, (2,), 2, "planck"),
    (8, 8, "CRB--K", "bands", 8, 13, (2,), 2, "planck"),
    (8, 8, "CRB-S-", "bands", 7, 2, (2, 1), 2, "observer"),
    (8, 8, "CRB-SK", "bands", 7, 2, (2, 1), 2, "observer"),
    (8, 8, "CRBI--", "instr", 8, 13, (2,), 2, "planck"),
    (8, 8, "CRBI-K", "instr", 8, 13, (2,), 2, "planck"),
    (8, 8, "CRBIS-", "instr", 7, 2, (2, 1), 2, "observer"),
    (8, 8, "CRBISK", "instr", 7, 2, (2, 1), 2, "observer"),
)
BARRED = ()      # no compiled instance is out of every call's reach (module docstring)

# K_PLAIN of the cases, measured on the CPU by tests/test_state_instances_host.py (the largest over every case of a gas
# count): n_gas: (radiances, Jacobian rows)
K_PLAIN_SEEN = {1: (24.9, 24.0), 2: (24.9, 24.7), 3: (24.9, 23.5), 4: (24.9, 23.6), 5: (4.55, 6.21), 6: (24.9, 23.2), 7: (24.9, 20.5),
                8: (24.9, 22.9)}
# (24.9 is a Planck start crossing 23 equal segments of tau = -1e-13: exp(1e-13) is rounded the same way 23 times over, and
# nothing else is in the result -- the recorded K_PLAIN_RAD = 41 comes from the same effect on 41 segments.  No five-gas
# entry has an initial intensity.)
