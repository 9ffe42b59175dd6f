/*
 * spectrobot_hip.h -- C ABI of libspectrobot_hip.so, the MI355X (gfx950) engine
 * for SpectRobot's spectral hot path: per-line Voigt evaluation and per-layer
 * absorption / emission coefficient accumulation, plus the Curtis-Godson column
 * integrals and the limb radiance recursion that consume them.
 *
 * This is the drop-in boundary.  The reference reaches this path through three
 * f2py extension modules (`import lineshape`, `import fparts_mod`, `import
 * curgods`; spect_classes.py:18, 1685 and the absent spect_base_module) and
 * through the Python entry points spect_classes.calc_shapes_lines
 * (spect_classes.py:1378) + LutSet.add_PT (spect_main_module.py:1122) called
 * from make_abscoeff_isomolec(..., useLUTs=False) (spect_main_module.py:1880).
 * Each entry point below names the reference interface it replaces.  Plain
 * pointers and sizes only; no exceptions cross the boundary; every function
 * returns SR_OK (0) or a negative sr_status (the Fortran `stop`s of
 * lineshape.f:253-264 become SR_ERR_ARG).  All buffers are caller-owned.
 *
 * Pointer spaces: functions suffixed `_dev` take DEVICE pointers for the bulk
 * in/out arrays (HBM-resident data path); the others take HOST pointers and
 * stage through the device themselves (compat shims).  `stream` is a
 * hipStream_t passed as void* (NULL = default stream).
 */
#ifndef SPECTROBOT_HIP_H
#define SPECTROBOT_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum {
  SR_OK = 0,
  SR_ERR_ARG = -1,      /* bad argument (also: where humliv_bb would `stop`) */
  SR_ERR_LIMIT = -2,    /* a documented size limit exceeded */
  SR_ERR_HIP = -3,      /* HIP runtime error, see sr_last_error() */
  SR_ERR_NODEVICE = -4, /* no gfx950 device visible */
  SR_ERR_UNSUPPORTED = -5,
  SR_ERR_TABLE = -6     /* (mol, iso) not in the TIPS-2003 tables */
} sr_status;

#define SR_IMXSIG 13010 /* parameters.inc:65 -- points per line window */
#define SR_MAX_LEVELS 64

const char *sr_strerror(int status);
const char *sr_last_error(void); /* text of the last HIP failure on this thread */
int sr_abi_version(void);

/* Device selection / query (one process per GPU: call once per rank). */
int sr_set_device(int device);
int sr_device_info(char *name, int name_len, int *cu_count, double *hbm_gib);
/* Hardware queues.  The ROCm runtime maps a process's streams onto GPU_MAX_HW_QUEUES hardware queues (environment
 * variable, default 4, read ONCE when HIP initialises, i.e. at the process's first HIP call); streams that share a
 * queue wait for each other's kernels although no event orders them.  The coefficient op therefore runs on THREE
 * streams: the caller's (the wings kernel, which writes the output) and two of the handle's own whose stream order is
 * the order the phased schedule runs their kernels in anyway -- table preparation -> level-0 pass -> S2M, M2M -> M2L ->
 * next call's preparation on one, the zones kernel on the other.  Per thread and device the library adds ONE staging
 * stream (early host-to-device copies), so a process with one top-level lineset keeps caller + 3 <= 4 streams and its
 * pipeline overlaps fully on the runtime's default (measured per BASELINE step, profiles/two_stream_pipeline_ab.txt:
 * 5.16 ms with 4 queues and 5.16 with 8; the five-stream pipeline before it 5.45 with 4, 5.15 with 8).  The level-table
 * builds and per-level sub-linesets run on the same two streams.  Every further top-level lineset used CONCURRENTLY
 * adds two streams of its own: such a process, or one whose own code keeps several streams busy, still wants more
 * queues -- export GPU_MAX_HW_QUEUES=8 before its first HIP call (the Python package does so at import unless the
 * caller already set it).  *recommended = 8: that headroom, not a requirement of a single handle; *configured = what
 * this process runs with (the variable's value, 4 when unset).  Returns SR_OK; either pointer may be NULL.  Results do
 * not depend on the setting, only the schedule does. */
int sr_recommended_hw_queues(int *recommended, int *configured);
/* *live = HIP streams this library has created and not destroyed in this process, *created_total = all it ever created
 * (every stream it makes is counted where it is made).  A handle's two pipeline streams are destroyed with the handle
 * (sr_lineset_destroy); the staging stream belongs to the THREAD that first staged on a device, outlives every handle and
 * is never destroyed, so *live stays >= 1 per such (thread, device) for the rest of the process, also after the thread
 * has exited.  Needs no GPU; either pointer may be NULL.  Returns SR_OK. */
int sr_stream_census(int *live, int *created_total);

/* ------------------------------------------------------------------------ *
 * Fine-grained shims: the f2py call shapes, one reference routine each.     *
 * Host pointers.  All evaluated on the GPU.                                  *
 * ------------------------------------------------------------------------ */

/* lineshape.humliv_bb(x, i1, i2, x0, lw, dw) -> y      (lineshape.f:226-569)
 * x[n], y[n]; i1,i2 1-based inclusive.  All three branches: x(i1) < x0 < x(i2)
 * (the only one the reference's Python reaches) in parallel, the two
 * with x0 at or beyond an end as the Fortran's sequential loops. */
int sr_humliv_bb(const double *x, int n, int i1, int i2, double x0, double lw,
                 double dw, double *y);

/* lineshape.sum_all_lines(spe_ini, matrix, init, fin, n_lines, n_spe)
 * (lineshape.f:2-25).  spe[n_spe] is updated in place; rows is row-major
 * [n_lines][row_len] (the Fortran's matrix(ilin, i)); init/fin 1-based. */
int sr_sum_all_lines(double *spe, int64_t n_spe, const double *rows,
                     const int32_t *init, const int32_t *fin, int n_lines,
                     int row_len);

/* fparts_mod.bd_tips_2003(MOL, ISO) -> gi, t_grid[119], QT_grid[119]
 * (fparts_mod.f:33-295). */
int sr_bd_tips_2003(int mol, int iso, double *gi, double *t_grid119,
                    double *qt_grid119);

/* spect_classes.CalcPartitionSum(mol, iso, temp) (spect_classes.py:1692-1710),
 * vectorised over temps[n]. */
int sr_calc_partition_sum(int mol, int iso, const double *temps, int n,
                          double *q_out);

/* curgods.curgod_fort_{1..4}(nd, [vmr, [f,]] x, n_p) -> res (curgods.f:2-98),
 * batched: segment s covers samples off[s] .. off[s+1]-1 of the concatenated
 * arrays; res[n_seg].  vmr / f may be NULL for the variants that do not use
 * them. */
int sr_curgod(int which, const double *nd, const double *vmr, const double *f,
              const double *x, const int32_t *off, int n_seg, double *res);

/* ------------------------------------------------------------------------ *
 * Coarse-grained op: the real hot path.                                      *
 * ------------------------------------------------------------------------ */

/* Line list of one iso-molecule, structure of arrays, host pointers
 * (SpectLine fields, spect_classes.py:50-51). lev_up/lev_lo: index into the
 * level table or -1 (unidentified); ignored when n_levels == 0. */
typedef struct {
  int64_t n_lines;
  const double *freq;        /* Freq        cm^-1 */
  const double *a_coeff;     /* A_coeff     s^-1  */
  const double *e_lower;     /* E_lower     cm^-1 */
  const double *g_up, *g_lo; /* statistical weights */
  const double *air_broad;   /* Air_broad   cm^-1/atm */
  const double *t_dep_broad; /* T_dep_broad */
  const int32_t *lev_up, *lev_lo;
} sr_lines_desc;

/* The iso-molecule the lines belong to (sbm IsoMolec as the path uses it:
 * .mol .iso .MM .levels[].energy). n_levels == 0 is the reference's
 * "unidentified_lines" / 'all' set (spect_main_module.py:1937-1953). */
typedef struct {
  int mol, iso;
  double mm;
  int n_levels;
  const double *level_energy; /* [n_levels] cm^-1 */
} sr_isomolec_desc;

/* Spectral grid as prepare_spe_grid builds it (spect_main_module.py:1262-1272):
 * grid[j] = w0 + j*step (numpy arange), j < n_grid <= 2e6 (imxsig_long). */
typedef struct {
  double w0, step;
  int64_t n_grid;
} sr_grid_desc;

typedef struct sr_lineset sr_lineset; /* opaque, device resident */

/* Upload a line list.  Replaces the per-call Python list of SpectLine objects
 * handed to calc_shapes_lines (spect_classes.py:1378).  Applies the reference's
 * line filter (spect_classes.py:1384-1388 with LinkToMolec 122-150), finds each
 * line's window centre (closest_grid, spect_classes.py:1937-1943) and sorts by
 * centre.  n_kept (may be NULL) receives the number of lines retained.
 * Lines farther than half a window (~3.25 cm^-1 at the default step) from the grid are kept too:
 * their window sits on the first / last grid point, humliv_bb takes one of its outer branches
 * (lineshape.f:272-442) and their far wing inside the grid is added, as in the reference. */
int sr_lineset_create(const sr_lines_desc *lines, const sr_isomolec_desc *iso,
                      const sr_grid_desc *grid, sr_lineset **out,
                      int64_t *n_kept);
int sr_lineset_destroy(sr_lineset *ls);

/* Finite differences in temperature (no reference counterpart: the reference has no temperature Jacobian,
 * spect_main_module.py:300-306 is commented out).  The Humlicek region boundaries of a (line, layer) are index
 * computed (nint, lineshape.f:443-490) and the regions disagree by 1e-5..1e-4 at their seams, so c(T + dT) - c(T)
 * jumps wherever a boundary moves by a point: spikes of (1e-5 y) / dT in a difference quotient.  After this call
 * the coefficient calls on `ls` place il, ir, il2, ir2 and the region-3 interval of every (line, layer) as at the
 * temperatures temps_bounds[n_layers] (HOST, copied) while every width, running x and weight follows the call's
 * own temperatures: c(T + dT) and c(T) then share their region boundaries and the quotient is smooth, also for
 * a one-sided difference with a small dT.  temps_bounds == NULL or n_layers == 0 restores the default. */
int sr_lineset_set_bounds_temps(sr_lineset *ls, const double *temps_bounds, int n_layers);

/* With frozen boundaries (sr_lineset_set_bounds_temps(T_b)): on != 0 makes the next coefficient ops take every line
 * weight (G coefficients / normalisation; NOT the level populations, which the caller passes) at T_b and continue it to
 * the call's temperature by its first-order Taylor term, w(T_b) (1 + (T - T_b) d ln w / d T), while widths, running x and
 * shapes follow the call's T as always.  For temperature derivatives by difference (build's own: the reference has
 * none): (c_lin(T_b + dT) - c(T_b)) / dT is then free of the Boltzmann factors' curvature, the step can grow from
 * 0.002 to 0.05 K and the reference's single-precision staircase (1e-7 |c| / dT) shrinks with it.  0: exact weights. */
int sr_lineset_set_linear_weights(sr_lineset *ls, int on);

/* Pressure shift of the line centres and self-broadening (what spect_classes.py:161-206 and 1967-1972 intend: the
 * reference computes wn_0 = Freq + P_shift Pres_atm at :187 and then hands Freq to MakeShape at :197, and no caller
 * passes Self_broad / Self_pres_atm to Lorenz_width).  Opt-in per line set; a line set that was never given the data,
 * or was given it and had it taken back, computes exactly what it did before, bit for bit.
 *
 * For line i in layer k, with P_atm = convert_to_atm(P_k) and Ps_atm = convert_to_atm(p_self_k):
 *   shape centre    x0' = Freq_i + p_shift_i P_atm
 *   Lorentz width   lw  = (296 / T)^n_i (gamma_air,i (P_atm - Ps_atm) + gamma_self,i Ps_atm)
 * x0' replaces Freq_i wherever the centre POSITIONS the shape (the running x of every region, the region boundaries,
 * the outer branches' x).  Still taken at Freq_i: the Doppler width, the normalisation fac, the G coefficients and the
 * strengths, the window (ic = closest_grid(Freq_i), grid indices ic - 6505 .. ic + 6504), the sort order and the
 * candidate selection of tiles and shards.  Frozen boundaries (sr_lineset_set_bounds_temps) place their indices with
 * the same x0' and with lw at the boundary temperature.
 *
 * sr_lineset_set_line_shape: p_shift[n_lines] (cm^-1 / atm) and self_broad[n_lines] (cm^-1 / atm), in the order the
 * lines were given to sr_lineset_create (n_lines = that call's, else SR_ERR_ARG).  HOST, copied.  Either may be NULL
 * (that quantity keeps its default: no shift / air broadening only); both NULL restores the default.  SR_ERR_ARG for a
 * non-finite value, self_broad < 0, or the handle of a per-level sub-lineset.  The per-level sub-linesets cut earlier
 * are dropped and rebuilt on their next use.
 *
 * sr_lineset_set_self_pressure: the partial pressure of the gas itself, p_self_hpa[n_layers] (hPa; HOST, copied), for
 * the following coefficient calls with that many layers; a call with another layer count, or with a p_self outside
 * [0, P] of its layer, is refused with SR_ERR_ARG.  NULL or n_layers == 0 restores p_self = 0.  Without self_broad it
 * has no effect.  SR_ERR_ARG for a negative or non-finite value.
 *
 * Limits, checked per call before anything is copied or launched (outputs stay untouched):
 *   SR_ERR_LIMIT        max_i |p_shift_i| P_atm,k > SR_MAX_SHIFT_POINTS grid steps in some layer.  A main line's centre
 *                       lies within half a step of its window centre ic; shifted it stays within 1024.5 points of it,
 *                       of the window's 6505 to either side.  What the limit keeps: the window-end expansions (degree
 *                       5 over 64 points) see the centre >= 5417 points away, ratio 32 / 5417 (6441 unshifted: 2.8
 *                       times the truncation, of a term that is itself ~1e-8 of the line's peak), and the short series of
 *                       the far field's window bands (8 terms beyond 4096 points of ic) a ratio <= 32 / 3072, 1.4e-16.
 *                       HITRAN's largest shifts (~0.1 cm^-1 / atm) at 1.5 atm and a step of 5e-4 cm^-1 are 300 points.
 *   SR_ERR_UNSUPPORTED  a line changes humliv_bb's branch in some layer: an outer line (centre outside its own window,
 *                       sequential branches lineshape.f:272-442) whose shifted centre lies strictly inside its window,
 *                       or a main line centred beyond a grid end whose shifted centre leaves it.
 *
 * The VMR Jacobians of the limb calls hold the coefficients fixed: the dependence of lw on the gas's own VMR through
 * p_self is not differentiated; a retrieval refreshes p_self between its iterations. */
#define SR_MAX_SHIFT_POINTS 1024
int sr_lineset_set_line_shape(sr_lineset *ls, const double *p_shift, const double *self_broad, int64_t n_lines);
int sr_lineset_set_self_pressure(sr_lineset *ls, const double *p_self_hpa, int n_layers);

/* Layer stack (the Temps / Press lists of make_abscoeff_isomolec,
 * spect_main_module.py:1880, plus level.local_vibtemp, :2065). Host pointers.
 * tvib: [n_levels][n_layers] or NULL for LTE (:2062-2063).  q_part: [n_layers]
 * or NULL to have the library evaluate CalcPartitionSum(mol, iso, T). */
typedef struct {
  int n_layers;
  const double *temps; /* K   */
  const double *press; /* hPa */
  const double *tvib;
  const double *q_part;
} sr_layers_desc;

/* Stream contract of the coarse-grained calls: work is enqueued on `stream` and returns without
 * synchronising.  A lineset owns scratch that consecutive calls share; every call therefore first
 * orders `stream` after the end of the previous sr_abscoeff_layers* / sr_gcoeff_* call on the SAME
 * lineset (an event wait, free when both use one stream), so calls on unrelated streams are safe.
 * Calls on one lineset must still be ISSUED from one host thread at a time.  The sr_set_* mode
 * switches are process-wide atomics; a call reads them once at entry. */

/* abs/emi coefficient spectra for every layer over the grid shard
 * [g_lo, g_hi): what make_abscoeff_isomolec(..., useLUTs=False) returns as
 * AbsSetLOS lists (spect_main_module.py:2128-2131), i.e. calc_shapes_lines +
 * add_PT + the population-weighted combine (:1974-1990, :2036-2080).
 * abs_out / emi_out: DEVICE pointers, [n_layers][g_hi-g_lo] doubles. */
int sr_abscoeff_layers_dev(sr_lineset *ls, const sr_layers_desc *atm,
                           int64_t g_lo, int64_t g_hi, double *abs_out,
                           double *emi_out, void *stream);
/* Same with HOST output buffers (copies back; PCIe-inclusive). */
int sr_abscoeff_layers(sr_lineset *ls, const sr_layers_desc *atm, int64_t g_lo,
                       int64_t g_hi, double *abs_out, double *emi_out);

/* Line strengths (SpectLine.CalcStrength*, spect_classes.py:115-119, 208-310).  Here b(E, T) = exp(-c2 E / T) and
 * r_L = b(E_L, Tvib_L) / b(E_L, T) (spect_base_module.vibtemp_to_ratio; 1 for the 'all' set, whose E_vib is 0).
 *
 * HITRAN intensities s_ref[n_lines] (cm^-1 / (molecule cm^-2)) at t_ref, in the order the lines were given to
 * sr_lineset_create (n_lines = that call's ld->n_lines, else SR_ERR_ARG).  iso_ab: the isotopic abundance they include.
 * q_ref: Q(t_ref), or <= 0 for the library's CalcPartitionSum (evaluated by the calls that need it).  HOST, copied; a
 * later call replaces the set (after the calls in flight on the handle have finished with it). */
int sr_lineset_set_strengths(sr_lineset *ls, const double *s_ref, int64_t n_lines, double t_ref, double q_ref,
                             double iso_ab);

/* Strengths of every (layer, line).  s_ab / s_em: DEVICE [n_layers][n_lines], n_lines and line order as given to
 * sr_lineset_create; lines the lineset's filter dropped are 0.  s_em may be NULL.  atm->tvib NULL = LTE; atm->q_part as
 * everywhere (NULL: CalcPartitionSum); atm->press is not read (may be NULL).  Stream contract of the coefficient calls.
 *   SR_STRENGTH_EINSTEIN  CalcStrength_from_Einstein (spect_classes.py:219-254) times iso_ab, from the G coefficients of
 *                         the coefficient op (0 where A = 0 or a g = 0):
 *                           s_ab = iso_ab (G_abs b(E_vlo, Tvib_lo) - G_ind b(E_vup, Tvib_up)) / Q(T)
 *                           s_em = iso_ab G_sp b(E_vup, Tvib_up) / Q(T)
 *   SR_STRENGTH_HITRAN    CalcStrength_from_Strength (:256-289) from the intensities of sr_lineset_set_strengths (else
 *                         SR_ERR_ARG); iso_ab is not used (the intensities include theirs):
 *                           S(T) = s_ref Q(t_ref)/Q(T) b(E_low, T)/b(E_low, t_ref) (1 - b(nu, T))/(1 - b(nu, t_ref))
 *                                  (CalcStrength_at_T, :1713-1733)
 *                           s_ab = S(T) alpha_nlte(nu, T, r_lo, r_up)     (:1485-1488)
 *                           s_em = S(T) r_up BB_erg(T, nu)                (:2097-2107, with its own constants
 *                                  rc1 = 1.1904e-5, rhck = 1.4388: s_em is 0.05-0.2 % below the Einstein source's)
 * SR_ERR_TABLE: (mol, iso) not in the TIPS tables and Q not given (q_ref of the intensities, atm->q_part). */
enum { SR_STRENGTH_EINSTEIN = 0, SR_STRENGTH_HITRAN = 1 };
int sr_line_strengths_dev(sr_lineset *ls, const sr_layers_desc *atm, int source, double iso_ab,
                          double *s_ab, double *s_em, void *stream);

/* sr_abscoeff_layers_dev with every line weighted by the HITRAN source's s_ab / iso_ab and s_em / iso_ab instead of
 * the folded G weights, iso_ab being the abundance given to sr_lineset_set_strengths: the output keeps the meaning of
 * sr_abscoeff_layers_dev's (per molecule of the isotopologue; the abundance rides on the LOS col_scale).  Everything
 * else is that call's: stream contract, shards, far-field and exact modes, outer lines, frozen region boundaries.
 * For a line list whose Einstein A are missing or rounded; with s_ref from the A (Einstein_A_to_LineStrength_hitran)
 * abs equals sr_abscoeff_layers_dev's to rounding (the reference's LTE check, spect_main_Titan.py:186).
 * SR_ERR_ARG without sr_lineset_set_strengths; SR_ERR_UNSUPPORTED with sr_lineset_set_linear_weights(ls, 1). */
int sr_abscoeff_layers_from_strengths_dev(sr_lineset *ls, const sr_layers_desc *atm, int64_t g_lo, int64_t g_hi,
                                          double *abs_out, double *emi_out, void *stream);

/* Per-level, per-ctype G-coefficient spectra: what LutSet.add_PT -> SpectralGcoeff.BuildCoeff(lines,
 * Temp, Pres, preCalc_shapes=True) produce for ONE level at every (P, T) of the layer stack
 * (spect_main_module.py:1122-1168, spect_classes.py:1277-1337; called per level from
 * LookUpTable.make, spect_main_module.py:770-774, and make_abscoeff_isomolec, :1983-1990):
 *   sp_emission, ind_emission: sum over the lines whose UPPER level is `level` of G_ctype * shape,
 *   absorption:                sum over the lines whose LOWER level is `level` (spect_classes.py:1304-1313);
 * for an iso-molecule without levels (the 'all' set, spect_classes.py:1316-1319) level must be 0 and
 * every line counts; level = -1 on an iso-molecule WITH levels sums every linked line with the G
 * coefficients of its own levels (the 'all' LutSet of an LTE table, spect_main_module.py:742-748, 774).  No population enters (that is the caller's combine, spect_main_module.py:2073-2080).
 * g_out: DEVICE [3][n_layers][g_hi-g_lo], ctype 0 'sp_emission', 1 'ind_emission', 2 'absorption'.
 * atm->tvib / q_part are not used.  Lines of the level are cut into a sub-lineset on first use. */
int sr_gcoeff_layers_dev(sr_lineset *ls, const sr_layers_desc *atm, int level, int64_t g_lo, int64_t g_hi,
                         double *g_out, void *stream);

/* One level's share of the abs / emi coefficients, the reference's track_levels output
 * (spect_main_module.py:2083-2087): abs = pop_L (Gabs_L - Gind_L), emi = pop_L Gsp_L with
 * pop_L = exp(-c2 E_L / Tvib_L) / Q(T).  Summed over the levels this is sr_abscoeff_layers_dev.
 * abs_out / emi_out: DEVICE [n_layers][g_hi-g_lo]. */
int sr_abscoeff_level_dev(sr_lineset *ls, const sr_layers_desc *atm, int level, int64_t g_lo, int64_t g_hi,
                          double *abs_out, double *emi_out, void *stream);

/* Level-factored route (round 4).  The reference never re-evaluates a line shape when only the vibrational
 * temperatures change: the G spectra of a level depend on (P, T) alone (LutSet.add_PT -> BuildCoeff,
 * spect_main_module.py:1122-1168, spect_classes.py:1277-1337) and every LOS step is the population-weighted sum
 * abs += pop_L (Gabs_L - Gind_L), emi += pop_L Gsp_L over the levels (make_abscoeff_isomolec :2036-2106,
 * make_abscoeff_LUTS_fast :2200-2276).  Only the two spectra pop_L multiplies enter that sum, so the tables hold the
 * PAIR  A_L = Gabs_L - Gind_L,  E_L = Gsp_L  per level and (P, T) row.
 * Round 6: the MULTI-CHANNEL pass -- the near-field kernels walk the full line list ONCE (sr_zones_mc_kernel,
 * sr_wings_mc_kernel: every line's three weighted contributions go to the LDS plane of the level they belong to), the
 * far field stays one far-only pass per level sub-lineset (it is linear per output spectrum).  Before, every line was
 * evaluated twice (in its upper level's pass and in its lower level's) and a sparse level's pass cost twice its lines'
 * share; sr_set_level_route(0) keeps that route (one coefficient op per level), which the exact mode and counting
 * passes always take.  The two routes differ by summation order only.  The three ctypes apart: sr_gcoeff_levels_dev.
 * An iso-molecule without levels has the one pair of its 'all' set (n_levels counts as 1).
 * out: DEVICE [max(n_levels, 1)][2][n_layers][g_hi-g_lo] (level, A | E, row, point).  atm->tvib / q_part are not used.
 * Frozen region boundaries (sr_lineset_set_bounds_temps) apply as in every coefficient op. */
int sr_glevel_pairs_dev(sr_lineset *ls, const sr_layers_desc *atm, int64_t g_lo, int64_t g_hi, double *out, void *stream);
/* LookUpTable.make / LutSet.add_PT for ALL levels at once (spect_main_module.py:718-788, 1122-1168): the G spectra of
 * every level and ctype on the (P, T) rows of atm, by the multi-channel pass (or, where it does not apply, by
 * sr_gcoeff_layers_dev level by level).  g_out: DEVICE [max(n_levels, 1)][3][n_layers][g_hi-g_lo] =
 * level, (sp_emission | ind_emission | absorption), row, point -- per level the layout of sr_gcoeff_layers_dev. */
int sr_gcoeff_levels_dev(sr_lineset *ls, const sr_layers_desc *atm, int64_t g_lo, int64_t g_hi, double *g_out, void *stream);
/* 1 (default): level tables by the multi-channel pass; 0: one coefficient op per level (the A/B partner and fallback). */
int sr_set_level_route(int multi_channel);
/* HIP-event times [ms] of the last multi-channel table build on the handle (its last row batch; sr_set_timing(1)), on the
 * caller's stream: ms4[0] the full list's tables (sr_prep_kernel), [1] sr_zones_mc_kernel, [2] what was left of the far-only
 * passes when it ended, [3] sr_wings_mc_kernel.  With sr_set_overlap(0) the far passes run on the caller's stream too,
 * behind the zones kernel: [1] and [3] are then the two kernels' stand-alone durations.  SR_ERR_ARG if no timed build. */
int sr_last_level_tables_ms(sr_lineset *ls, float *ms4);

/* The combine loop of the level-factored route for n_steps LOS steps at once, each step on one (P, T) row of the
 * pair tables `tab` (as sr_glevel_pairs_dev writes them, n_rows rows):
 *   abs[s] = sum_L pop[s][L] A_L[row[s]],   emi[s] = sum_L pop[s][L] E_L[row[s]]          (smm:2073-2080)
 * in ONE pass over the tables: the steps of a row are taken together, its 2 n_levels spectra are read once.
 * Temperature derivative (optional; the reference has none): with tab_dT = the pair tables at T + dT
 * (region boundaries frozen at T), inv_dT = 1 / dT and dpop[s][L] = d pop_L / dT of the step,
 *   dabs[s] = sum_L dpop[s][L] A_L + pop[s][L] (A'_L - A_L) inv_dT,   demi[s] likewise with E
 * -- the population part analytic, only d G / d T by difference.  tab_dT == NULL: dabs_out / demi_out are not written.
 * step_row [n_steps], pop / dpop [n_steps][n_levels]: HOST.  abs_out / emi_out / dabs_out / demi_out: DEVICE
 * [n_steps][n_pts], rows in the caller's step order (a coefficient row per LOS step for the recursion kernels). */
int sr_glevel_combine_dev(const double *tab, const double *tab_dT, int n_levels, int n_rows, int64_t n_pts, int n_steps,
                          const int32_t *step_row, const double *pop, const double *dpop, double inv_dT,
                          double *abs_out, double *emi_out, double *dabs_out, double *demi_out, void *stream);

/* Look-up-table route: LutSet.calculate (spect_main_module.py:997-1066) for one level and
 * n_steps LOS steps on a table of G spectra resident in HBM, g_tab: DEVICE [3][n_pt][n_pts] (ctype-major,
 * one row per tabulated (P, T) couple, as sr_gcoeff_layers_dev writes them).  Per step, idx4[s] = table rows
 * (P1,T1), (P1,T2), (P2,T1), (P2,T2) and wgt4[s] = (wP1, wP2, wT1, wT2): first linear in P at both
 * temperatures, then linear in T (SpectralGcoeff.interpolate, spect_classes.py:1349-1375); idx4[s][2] < 0:
 * T only between rows idx4[s][0], idx4[s][1] with (wT1, wT2) (below the lowest tabulated pressure, :1007-1025).
 * combine == 0: out_a: DEVICE [3][n_steps][n_pts] receives the interpolated set (out_e unused);
 * combine != 0: the population-weighted combine of make_abscoeff_isomolec (:2073-2080) is applied on the fly,
 * out_a[s] += pop[s] G_abs; out_a[s] -= pop[s] G_ind; out_e[s] += pop[s] G_sp (DEVICE [n_steps][n_pts],
 * zeroed by the caller before the first level).  idx4 / wgt4 / pop: HOST.  A row outside the table or a weight
 * that is not finite (any of the four of any step) is refused with SR_ERR_ARG before anything is written. */
int sr_lut_interp_dev(const double *g_tab, int n_pt, int64_t n_pts, int n_steps, const int32_t *idx4,
                      const double *wgt4, const double *pop, int combine, double *out_a, double *out_e,
                      void *stream);

/* Limb radiance recursion for a batch of rays over the shard (the build's own
 * definition standing in for the absent sbm LineOfSight.radtran_fast, call
 * sites spect_main_module.py:2838, 3214; parity unpinned):
 * ray r crosses segments seg_off[r] .. seg_off[r+1]-1 in photon order; segment
 * s applies layer seg_layer[s] with absorber column seg_col[s] (cm^-2):
 *   tau = abs*col;  I <- I*exp(-tau) + emi*col*(1-exp(-tau))/tau.
 * abs_c/emi_c: DEVICE [n_layers][n_pts]; rad: DEVICE [n_rays][n_pts], read as
 * the initial intensity when init_from_rad != 0, else started from 0.
 * seg_* are HOST arrays. */
int sr_radiance_rays_dev(const double *abs_c, const double *emi_c, int n_layers,
                         int64_t n_pts, int n_rays, const int32_t *seg_off,
                         const int32_t *seg_layer, const double *seg_col,
                         int init_from_rad, double *rad, void *stream);

/* ------------------------------------------------------------------------ *
 * Device LOS pipeline: Curtis-Godson columns per segment on the device, then the      *
 * recursion, for a batch of rays through n_gas gases.  Stands in for the absent sbm                    *
 * LineOfSight.calc_radtran_steps + radtran_fast (call sites spect_main_module.py:2746-2767, 2834-2845, *
 * radtran_3D_ch4.py:297-315); the build's own definition, parity unpinned (columns: curgod_fort_2,     *
 * pinned).                                                                                             *
 * ------------------------------------------------------------------------ */
typedef struct {
  int n_rays, n_gas;        /* n_gas <= sr_limb_max_gases(.) of the entry, see below the struct */
  const int32_t *seg_off;   /* HOST [n_rays+1]: ray r crosses segments seg_off[r] .. seg_off[r+1]-1 */
  const int32_t *seg_layer; /* HOST [n_seg]: row of abs_c / emi_c (the LOS step's (P, T)) a segment applies */
  const int32_t *pt_off;    /* HOST [n_seg+1]: LOS sample points of segment s: pt_off[s] .. pt_off[s+1]-1 (>= 2) */
  const double *x;          /* HOST [n_pt] path coordinate of the sample points, cm, increasing inside a segment */
  const double *nd;         /* HOST [n_pt] number density, cm^-3 (exponential between sample points, curgods.f) */
  const double *vmr;        /* HOST [n_gas][n_pt] volume mixing ratio (linear between sample points) */
  const double *col_scale;  /* HOST [n_gas] factor on each gas's columns (isotopic abundance), NULL = 1 */
  int los_order;            /* 0 'photon': segments listed along the photon path (spect_main_module.py:2748);
                               1: listed from the observer outwards (walked backwards by the recursion) */
  int solo_absorption;      /* != 0: no emission term, I <- I exp(-tau) (radtran_3D_ch4.py:312) */
  int init_mode;            /* 0: I = 0; 1: rad holds the initial_intensity; 2: Planck spectrum at t_init on the
                               grid w0 + (g_lo + j) step (Calc_BB, spect_classes.py:1881-1892) */
  double t_init, w0, step;
  int64_t g_lo;             /* first grid index of the shard (Planck only) */
} sr_los_desc;

/* Curtis-Godson columns only: col_out HOST [n_gas][n_seg] = col_scale[g] * curgod_fort_2(nd, vmr_g, x) per segment
 * (curgods.f:24-45), evaluated on the device.  Synchronises. */
int sr_los_columns(const sr_los_desc *los, double *col_out);

/* The path of LIMB rays as a function of each ray's own tangent altitude z_t [km], the crossed shells held fixed
 * (geometry.limb_los(path=True)): per sample point its altitude and the derivatives of its path coordinate and of its
 * altitude.  With r_t = R + z_t and a shell end at radius hi > r_t, s_hi = sqrt(hi^2 - r_t^2), d s_hi / d z_t =
 * -r_t / s_hi (s = 0 with derivative 0 at the tangent point); sample point i of a segment [a, b] blends the ends
 * linearly, alt_i = sqrt(s_i^2 + r_t^2) - R, d alt_i / d z_t = (s_i d s_i + r_t) / (alt_i + R): 0 on a shell boundary, 1
 * at the tangent point.  The derivative is one-sided where z_t lies on a level (the tangent shell is the one above).
 * Not defined for 3-D paths, slant / nadir paths, adaptive stepping, observer order, the resident handles, refraction. */
typedef struct {
  const double *alt;     /* HOST [n_pt] altitude of the sample points, km */
  const double *dx_dz;   /* HOST [n_pt] d x / d z_t, cm per km */
  const double *dalt_dz; /* HOST [n_pt] d alt / d z_t */
} sr_los_path;

/* d col_g[s] / d z_t, the twin of sr_los_columns: dcol_out HOST [n_gas][n_seg] = col_scale[g] times the forward-mode
 * derivative of curgod_fort_2's sum over the segment, with d x from the path and, ln nd and every VMR being linear in
 * altitude inside a segment (slopes from its first and last sample point; zero where their altitudes coincide),
 *   d nd_i = nd_i slope_ln_nd dalt_dz[i],   d vmr_i = slope_vmr dalt_dz[i].
 * A segment whose path derivatives are all zero gives an exact 0.0.  path or one of its arrays NULL: SR_ERR_ARG;
 * los_order != 0: SR_ERR_UNSUPPORTED (observer-order batches re-list their sample points).  Synchronises.
 * The reference has no counterpart: checked against an extended-precision restatement and against differences of
 * rebuilt geometry (tests/pointing_reference.py, tests/test_gpu_pointing.py). */
int sr_los_columns_dz(const sr_los_desc *los, const sr_los_path *path, double *dcol_out);

/* Radiances of the ray batch.  abs_c / emi_c: DEVICE [n_gas][n_layers][n_pts]; rad: DEVICE [n_rays][n_pts].
 * Per-gas and per-level partial radiances (single_rads[(gas, iso)], single_rads[(gas, iso, lev)],
 * spect_main_module.py:2883-2887, 3287): sr_limb_rays_parts_dev below, all of them in one pass.  (An emission share
 * given as an explicit spectrum: pass it as emi_c with the total abs_c.) */
int sr_limb_rays_dev(const double *abs_c, const double *emi_c, int n_layers, int64_t n_pts, const sr_los_desc *los,
                     double *rad, void *stream);

/* A LOS batch resident on the device: the description staged, the Curtis-Godson columns of its segments integrated
 * (curgod_fort_2) and, where the rays share their shells, the folded sweep's records packed -- ONCE, as the reference
 * computes a line of sight's steps once (los.calc_radtran_steps, spect_main_module.py:2746-2767, 3147) and runs
 * radtran / radtran_fast on them for every call of the forward model (:2838, 3214).  The description's arrays are
 * copied; init_mode / t_init / w0 / step / los_order / solo_absorption are taken as given (g_lo per call).  n_layers:
 * rows of the coefficient tables the handle will be used with (seg_layer is checked against it).  Synchronises. */
typedef struct sr_los sr_los;
int sr_los_create(const sr_los_desc *los, int n_layers, sr_los **out);
int sr_los_destroy(sr_los *h);
/* The same with n_par column (VMR-profile) parameters staged alongside (par_gas, par_w as for sr_limb_rays_jac_dev): the
 * batch of a retrieval, whose paths, densities and parameter masks stay while the VMRs change every iteration.
 * sr_los_set_vmr: new VMRs [n_gas][n_pt] (HOST) at the batch's sample points -- one copy and the column kernel on
 * `stream` (photon-order batches only).  sr_limb_rays_jac_los_dev: radiances and d rad / d x_p through the resident
 * batch, launches only (the folded kernel for <= 8 parameters on shared shells, else the forward sensitivities). */
int sr_los_create_par(const sr_los_desc *los, int n_layers, int n_par, const int32_t *par_gas, const double *par_w,
                      sr_los **out);
int sr_los_set_vmr(sr_los *h, const double *vmr, void *stream);
/* The columns of a resident batch integrated again from its staged sample points (two launches, no copy): for callers
 * whose step includes the column integration by definition. */
int sr_los_refresh_columns(sr_los *h, void *stream);
int sr_limb_rays_jac_los_dev(const double *abs_c, const double *emi_c, int n_layers, int64_t n_pts, sr_los *h, int64_t g_lo,
                             double *rad, double *jac, void *stream);
/* The forward model of ONE retrieval iteration on such a batch in one call -- what spect_main_module.py:2736-2940 does
 * between `add_clim` of the new profiles and `chicalc`: x [n_par] (HOST, the parameter vector in the batch's parameter
 * order) -> VMRs of the retrieved gases at the sample points (sum_p x_p w_p: a profile that is sum_p mask_p x_p on the
 * levels, spect_main_module.py:256-283, interpolated like its masks) -> columns -> radiances and parameter Jacobians ->
 * instrument bands (sr_hires_to_lowres_shard_dev's arguments) -> the closed-form field-of-view integral of every pixel
 * (FOV_integr_1D, :3342-3374; three rays per pixel in the batch's order).
 * fov: [n_rays / 3][7] = delta, delta^3, 2 dmax^2, edge, m2, esse, has_edge per pixel (the geometry factors of the
 * rotated square pixel), or NULL: the rays themselves.  buf: DEVICE scratch [n_rays (1 + n_par)][n_pts].
 * out (HOST): [n_rays / 3 or n_rays][1 + n_par][n_bands], row 0 the radiance, row 1 + p the derivative to x_p.  A
 * spectral shard (g_lo, n_pts) returns its partial band integrals (the integral is linear: all-reduce `out`).
 * Synchronises `stream`. */
int sr_retrieval_forward_dev(const double *abs_c, const double *emi_c, int n_layers, int64_t n_pts, sr_los *h, int64_t g_lo,
                             const double *x, double w0, double step, const double *centers_nm, const double *widths_nm,
                             int n_bands, double n_sigma, int out_units, const double *fov, double *buf, double *out,
                             void *stream);
/* ... and the rest of the iteration in the same call: chi square of the simulated pixels against the observations and the
 * Levenberg-Marquardt step of the optimal-estimation algebra (inversion_algebra, spect_main_module.py:3433-3469) on the
 * band spectra and Jacobians the call has just brought to the host -- K^T S_y^-1 K, S^-1 = G + S_a^-1, S_x, the averaging
 * kernel, dx = (S^-1 + lambda diag S^-1)^-1 (K^T S_y^-1 (y - F) + S_a^-1 (x_a - x)); n_par x n_par LU with partial
 * pivoting, host fp64 (the system is n_par <= 64 wide: nothing for a GPU).  What the caller keeps: the positivity rule
 * of the update (:633-641), the stopping rule (:2963-2973), its bookkeeping.  Single process only (a spectral shard's
 * band integrals are partial: all-reduce first and use the Python algebra).
 *   oe->obs / noise [n_pix n_bands] pixel-major, mask [n_pix n_bands] (1 = used) or NULL, sa_inv [n_par][n_par],
 *   x_apriori [n_par]; pixels = rays / 3 with fov, or the centre ray of every three without (fov == NULL).
 *   out as sr_retrieval_forward_dev's with fov ([n_pix][1 + n_par][n_bands]; without fov the centre rays' rows);
 *   chi_sum = sum over the used elements of ((obs - sim) / noise)^2, n_used their number; dx [n_par], s_x / avk
 *   [n_par][n_par].  SR_ERR_TABLE when the system is singular. */
typedef struct {
  int32_t n_obs;
  const double *obs, *noise;
  const uint8_t *mask;
  const double *sa_inv, *x_apriori;
  double lambda_lm;
} sr_oe_desc;
int sr_retrieval_step_dev(const double *abs_c, const double *emi_c, int n_layers, int64_t n_pts, sr_los *h, int64_t g_lo,
                          const double *x, double w0, double step, const double *centers_nm, const double *widths_nm,
                          int n_bands, double n_sigma, int out_units, const double *fov, double *buf, double *out,
                          const sr_oe_desc *oe, double *chi_sum, int32_t *n_used, double *dx, double *s_x, double *avk,
                          void *stream);
/* ... and the loop around it, for a retrieval whose coefficient spectra stay as they are (only VMRs are retrieved: the
 * loop of inversion_fast_limb, spect_main_module.py:2725-2987): per iteration sr_retrieval_step_dev at the current
 * parameter vector, chi = chi_sum / (n_used - n_dof_par) (:2949), the stopping rule (:2960-2973: relative change below
 * chi_threshold -> *stop = 1 "converged", chi increased -> 2 "raised", else 0 after max_it), then x += dx with the
 * positivity rule (:616-624: a step that would leave a constrained parameter <= 0 is halved until it does not).
 *   chi_hist [max_it], *n_it of them filled; x_hist [max_it + 1][n_par]: the vector before every iteration and after
 *   the last update (*n_it updates when *stop == 0, *n_it - 1 otherwise); out: the LAST iteration's band spectra and
 *   Jacobians; s_x / avk: of the last iteration whose update was applied (as the reference stores them after
 *   inversion_algebra; untouched when there was none).  What the caller keeps is object bookkeeping. */
typedef struct {
  int32_t max_it;
  double chi_threshold;
  const uint8_t *positive; /* [n_par]: 1 = constrain_positive */
  int32_t n_dof_par;       /* parameters in use */
} sr_loop_desc;
int sr_retrieval_loop_dev(const double *abs_c, const double *emi_c, int n_layers, int64_t n_pts, sr_los *h, int64_t g_lo,
                          const double *x0, double w0, double step, const double *centers_nm, const double *widths_nm,
                          int n_bands, double n_sigma, int out_units, const double *fov, double *buf, double *out,
                          const sr_oe_desc *oe, const sr_loop_desc *lp, double *chi_hist, double *x_hist, int32_t *n_it,
                          int32_t *stop, double *s_x, double *avk, void *stream);
/* sr_limb_rays_dev on a resident LOS: kernel launches only (no staging copy, no column kernel, no host plan).
 * g_lo: grid index of abs_c's first point (Planck initial intensity, init_mode 2). */
int sr_limb_rays_los_dev(const double *abs_c, const double *emi_c, int n_layers, int64_t n_pts, sr_los *h, int64_t g_lo,
                         double *rad, void *stream);
/* One forward-model step of one gas in ONE call: sr_abscoeff_layers_dev into abs_out / emi_out, then the recursion of
 * the resident LOS (n_gas = 1) through them into rad [n_rays][g_hi - g_lo] -- what a caller of make_abscoeff_isomolec
 * + radtran_fast does per spectrum (spect_main_module.py:1979-1990, 2838).  A 1/8 spectral shard of BASELINE
 * configs[1] is 0.8 ms of device time: the host's enqueue time per step is what eight ranks must stay under. */
int sr_limb_step_dev(sr_lineset *ls, const sr_layers_desc *atm, int64_t g_lo, int64_t g_hi, double *abs_out,
                     double *emi_out, sr_los *h, double *rad, void *stream);

/* + Jacobian w.r.t. n_par VMR-profile parameters: the VMR of gas par_gas[p] at LOS sample point i is
 * sum_p par_w[p][i] x_p (mask values of RetParam / LinearProfile at the point, spect_main_module.py:319-375), so
 * d col_g[s] / d x_p = col_scale[g] curgod_fort_2(nd, par_w[p], x).  par_gas: HOST [n_par]; par_w: HOST
 * [n_par][n_pt]; jac: DEVICE [n_rays][n_par][n_pts].  The build's definition (unpinned): every route of this call and of
 * the Jacobian calls below is held to an extended-precision CPU reference of the recursion on a panel of regimes
 * (thin switch, range-reduction boundaries, saturated, zero and negative optical depths) in
 * tests/test_gpu_limb_reference.py, and checked against finite differences in tests/test_gpu_limb.py. */
int sr_limb_rays_jac_dev(const double *abs_c, const double *emi_c, int n_layers, int64_t n_pts,
                         const sr_los_desc *los, int n_par, const int32_t *par_gas, const double *par_w, double *rad,
                         double *jac, void *stream);

/* + Jacobian w.r.t. one scalar per layer acting through the coefficients (temperature; BASELINE configs[3]):
 * dabs / demi: DEVICE [n_gas][n_layers][n_pts]; jac: DEVICE [n_rays][n_layers][n_pts].  init_mode 0 or 2. */
int sr_limb_rays_jac_layer_dev(const double *abs_c, const double *emi_c, const double *dabs, const double *demi,
                               int n_layers, int64_t n_pts, const sr_los_desc *los, double *jac, void *stream);

/* Radiances and both kinds of Jacobian in ONE pass over each ray (round 3; BASELINE configs[3]: "Jacobians w.r.t. T
 * and VMR per layer").  Any of the three outputs may be left out: rad NULL; jac_layer NULL (then dabs = demi = NULL);
 * n_par = 0 (then par_gas = par_w = jac_par = NULL) -- but at least one Jacobian.  Each segment's own sensitivity
 * times the transmission of everything behind it is added to the rows it acts on; the host plans per ray which
 * access stores, which adds and which contributions are carried in registers across consecutive segments, so a
 * Jacobian row is written about once per crossing instead of memset + read-add-store per segment.  Falls back to the
 * forward-sensitivity kernels (sr_limb_rays_jac_dev / _jac_layer_dev under sr_set_jac_layer_mode(1)) when a segment
 * touches more than four parameters; same definitions, same layouts.
 * seg_jac_row (HOST [n_seg], or NULL: = seg_layer, n_jac_rows ignored): the row of jac_layer [n_rays][n_jac_rows][n_pts]
 * a segment's per-layer sensitivity is added to.  A 3-D path (spect_main_module.py:2746-2767 with use_tangent_sza =
 * False: vibrational temperatures follow the local SZA along the LOS) gives every LOS step its own coefficient row
 * (seg_layer) while the retrieved scalar still belongs to the step's altitude layer (seg_jac_row). */
int sr_limb_rays_jacobians_dev(const double *abs_c, const double *emi_c, const double *dabs, const double *demi,
                               int n_layers, int64_t n_pts, const sr_los_desc *los, const int32_t *seg_jac_row,
                               int n_jac_rows, int n_par, const int32_t *par_gas, const double *par_w, double *rad,
                               double *jac_layer, double *jac_par, void *stream);

/* Radiances and their Jacobian with respect to LEVEL parameters of one level-factored gas: gas `gas` of the batch has
 * abs[r] = sum_L pop[r][L] A_L[row[r]], emi[r] = sum_L pop[r][L] E_L[row[r]] on every coefficient row r (the combine
 * of sr_glevel_combine_dev on the pair tables `tab` of sr_glevel_pairs_dev, row[r] = coef_row[r]), and parameter p
 * moves the population of level par_level[p] on row r by d pop[r][par_level[p]] / d x_p = par_c[p][r].  Per segment s
 * on row r with column u of that gas, for every parameter with par_c[p][r] != 0,
 *   dtau = u par_c[p][r] A_lev[row[r]],   dE = u par_c[p][r] E_lev[row[r]],
 *   J_p <- J_p t + (-I_prev t dtau + dE f + E f' dtau)            (solo_absorption: the two source terms drop)
 * -- the recursion of sr_limb_rays_jac_layer_dev with dabs / demi read from the tables, so no derivative tables and no
 * per-row Jacobian are written.  Vibrational temperatures, Tvib_L[r] = Tvib0_L[r] + sum_p w[p][r] x_p:
 *   par_c[p][r] = w[p][r] pop[r][L] c2 E_L / Tvib_L[r]^2   (exact: the coefficients are linear in the populations,
 * Q(T) does not depend on Tvib); par_c = w differentiates with respect to the populations themselves.
 * abs_c / emi_c: DEVICE [n_gas][n_layers][n_pts], the combined coefficients of every gas (n_layers = coefficient
 * rows); tab: DEVICE [n_levels][2][n_tab_rows][n_pts]; coef_row: HOST [n_layers], each in [0, n_tab_rows); par_level:
 * HOST [n_par], each in [0, n_levels); par_c: HOST [n_par][n_layers]; rad: DEVICE [n_rays][n_pts] or NULL; jac: DEVICE
 * [n_rays][n_par][n_pts], every element written (a parameter a ray never touches: zeros).  los_order, solo_absorption
 * and init_mode 0 / 2 as the other ray-batch calls; init_mode 1 is refused (SR_ERR_ARG).  All arguments are checked
 * before the first copy or launch: a refused call leaves rad and jac untouched.
 * The reference has no counterpart (it has no derivative code at all): the build's definition, checked
 * against the composition sr_glevel_combine_dev + sr_limb_rays_jacobians_dev per level and against central differences
 * of the whole forward chain in Tvib (tests/test_gpu_tvib_jacobian.py). */
int sr_limb_rays_jac_level_dev(const double *abs_c, const double *emi_c, int n_layers, int64_t n_pts,
                               const sr_los_desc *los, int gas, const double *tab, int n_levels, int n_tab_rows,
                               const int32_t *coef_row, int n_par, const int32_t *par_level, const double *par_c,
                               double *rad, double *jac, void *stream);

/* Radiances and their Jacobian with respect to a MIXED state vector in one pass over each ray: n_col column parameters
 * (VMR-profile parameters, exactly those of sr_limb_rays_jac_dev) and n_lev level parameters of the one level-factored
 * gas `gas` (exactly those of sr_limb_rays_jac_level_dev).  Both kinds feed the same recursion,
 *   J_p <- J_p t + (-I_prev t dtau_p + dE_p f + E f' dtau_p)        (solo_absorption: the two source terms drop)
 * and differ in where dtau_p and dE_p of a segment s on coefficient row r come from:
 *   column parameter p of gas g = par_gas[p]:  dtau = abs_g[r] D,  dE = emi_g[r] D,  D = d u_g[s] / d x_p, the
 *     Curtis-Godson column of the mask par_w[p] over the segment's sample points (times col_scale[g]);
 *   level parameter p of level L = par_level[p]:  dtau = par_c[p][r] u A_L[coef_row[r]],  dE = par_c[p][r] u E_L[coef_row[r]],
 *     u the column of `gas` on s, A_L / E_L the pair tables `tab` of sr_glevel_pairs_dev.
 * One call instead of sr_limb_rays_jac_dev + sr_limb_rays_jac_level_dev on the same batch: the LOS is staged once, the
 * columns are integrated once and the recursion tau, t, f, f' runs once per block of parameters, whatever their kinds.
 * abs_c / emi_c: DEVICE [n_gas][n_layers][n_pts]; par_gas: HOST [n_col], each in [0, n_gas); par_w: HOST [n_col][n_pt]
 * at the LOS sample points; tab: DEVICE [n_levels][2][n_tab_rows][n_pts]; coef_row: HOST [n_layers], each in
 * [0, n_tab_rows); par_level: HOST [n_lev], each in [0, n_levels); par_c: HOST [n_lev][n_layers]; rad: DEVICE
 * [n_rays][n_pts] or NULL; jac: DEVICE [n_rays][n_col + n_lev][n_pts]: the column parameters in the caller's order, then
 * the level parameters in the caller's order; every element is written (a parameter a ray never touches: exact zeros).
 * Either kind may be empty, not both; with n_lev == 0, tab, coef_row, par_level and par_c may be NULL (n_col == 0:
 * par_gas and par_w).  los_order, solo_absorption and init_mode 0 / 2 as the other ray-batch calls; init_mode 1 is
 * refused (SR_ERR_ARG).  All arguments are checked before the first copy or launch: a refused call leaves rad and jac
 * untouched.
 * The reference has no counterpart (it has no derivative code at all): the build's definition, checked
 * against the two single-kind calls and against central differences of the whole forward chain
 * (tests/test_gpu_state_jacobian.py). */
int sr_limb_rays_jac_state_dev(const double *abs_c, const double *emi_c, int n_layers, int64_t n_pts,
                               const sr_los_desc *los, int n_col, const int32_t *par_gas, const double *par_w, int gas,
                               const double *tab, int n_levels, int n_tab_rows, const int32_t *coef_row, int n_lev,
                               const int32_t *par_level, const double *par_c, double *rad, double *jac, void *stream);

/* sr_limb_rays_jac_state_dev with a third kind of parameter in the same pass: n_row ROW parameters, which act through the
 * coefficients of every gas with a weight per coefficient row (a layer on a 1-D path, a LOS step on a 3-D path).  With
 * derivative spectra dabs_c / demi_c of the coefficients' shape, a segment s on row r gives row parameter p
 *   dtau = par_t[p][r] sum_g u_g[s] dabs_g[r],   dE = par_t[p][r] sum_g u_g[s] demi_g[r]      (u_g the gas columns)
 * in the recursion above: the per-row Jacobian of sr_limb_rays_jac_layer_dev contracted with the weights inside the
 * recursion, so [n_rays][n_layers][n_pts] is never written.  Kinetic-temperature nodes: dabs_c / demi_c = d abs / dT,
 * d emi / dT per row, par_t = the nodes' masks on the rows.  The columns are held fixed (the definition of the
 * temperature Jacobian here: pressure, columns and vibrational temperatures fixed); the density part of a temperature
 * change is a set of ordinary column parameters, which a caller who wants it adds to par_gas / par_w.
 * dabs_c / demi_c: DEVICE [n_gas][n_layers][n_pts]; par_t: HOST [n_row][n_layers]; every other argument as in
 * sr_limb_rays_jac_state_dev.  jac: DEVICE [n_rays][n_col + n_lev + n_row][n_pts]: the column parameters, then the level
 * parameters, then the row parameters, each kind in the caller's order; every element is written (exact zeros for a
 * parameter a ray never touches or whose weights are all zero).  Any kind may be empty, not all; n_row == 0 is
 * sr_limb_rays_jac_state_dev itself (dabs_c, demi_c and par_t may then be NULL).  init_mode 1 is refused (SR_ERR_ARG),
 * n_pts above the limit SR_ERR_LIMIT.  All arguments are checked before the first copy or launch: a refused call leaves
 * rad and jac untouched.
 * The reference has no counterpart: the build's definition, checked against an extended-precision recursion, against
 * sr_limb_rays_jac_layer_dev contracted on the host and against central differences (tests/test_gpu_state_rows.py). */
int sr_limb_rays_jac_state_rows_dev(const double *abs_c, const double *emi_c, int n_layers, int64_t n_pts,
                                    const sr_los_desc *los, int n_col, const int32_t *par_gas, const double *par_w, int gas,
                                    const double *tab, int n_levels, int n_tab_rows, const int32_t *coef_row, int n_lev,
                                    const int32_t *par_level, const double *par_c, const double *dabs_c, const double *demi_c,
                                    int n_row, const double *par_t, double *rad, double *jac, void *stream);

/* sr_limb_rays_jac_state_rows_dev on the instrument's bands, in one call: the same recursion for the same mixed state
 * vector (column, level and row parameters, every argument up to par_t as there), but the hi-res spectra rad
 * [n_rays][n_pts] and jac [n_rays][n_par][n_pts] are never written: the recursion kernel integrates the bands in its
 * epilogue (sr_hires_to_lowres_shard_dev's weights, one v_mfma_f64_16x16x4 product per wave and 16-band tile), the
 * partial sums are added on the device and the closed-form field of view of sr_retrieval_forward_dev is applied to the
 * few KB that reach the host.  What sr_limb_rays_jac_state_rows_dev + sr_hires_to_lowres_shard_dev on rad and on jac +
 * the field-of-view integral compute, up to the order of the band sums.
 * The hi-res grid is the descriptor's: point j of the tables is w0 + (g_lo + j) step with los->w0, los->step, los->g_lo
 * (as for the Planck background); a descriptor without a grid (step <= 0) is refused.  A spectral shard (g_lo > 0 or
 * fewer points than the grid) returns PARTIAL band integrals with the semantics of sr_hires_to_lowres_shard_dev: shards
 * that each hold the next shard's first point add up to the whole.
 * centers_nm / widths_nm: HOST [n_bands]; n_sigma, out_units as sr_hires_to_lowres_dev; fov: HOST [n_rays / 3][7] as
 * sr_retrieval_forward_dev's (n_rays a multiple of 3), or NULL: the rays themselves; out: HOST
 * [n_rays / 3 or n_rays][1 + n_par][n_bands], n_par = n_col + n_lev + n_row: row 0 the radiance, row 1 + p the
 * derivative to parameter p in the call's order (column, level, row parameters).  A parameter a ray never touches is an
 * exact 0.0 in every band, a band whose window misses the grid an exact 0.0 in every row.  n_row == 0 needs no dabs_c /
 * demi_c / par_t.  init_mode 1 is refused (SR_ERR_ARG), n_pts above the limit SR_ERR_LIMIT.  All arguments are checked
 * before the first copy or launch: a refused call leaves out untouched.  Synchronises the stream.
 * Checked against the composition of the calls it replaces (tests/test_gpu_state_bands.py). */
int sr_limb_rays_state_bands_dev(const double *abs_c, const double *emi_c, int n_layers, int64_t n_pts,
                                 const sr_los_desc *los, int n_col, const int32_t *par_gas, const double *par_w, int gas,
                                 const double *tab, int n_levels, int n_tab_rows, const int32_t *coef_row, int n_lev,
                                 const int32_t *par_level, const double *par_c, const double *dabs_c, const double *demi_c,
                                 int n_row, const double *par_t, const double *centers_nm, const double *widths_nm,
                                 int n_bands, double n_sigma, int out_units, const double *fov, double *out, void *stream);

/* sr_limb_rays_jac_state_rows_dev for level parameters of SEVERAL level-factored gases in the same pass: a batch whose
 * gases lgas[0 .. n_lgas) are each combined from pair tables of their own (two non-LTE emitters in one window) gets the
 * vibrational-temperature parameters of all of them from ONE walk of each ray, together with the column and the row
 * parameters.  Level parameter p belongs to level gas k = par_lgas[p] and to its level L = par_level[p]; a segment s on
 * coefficient row r gives it
 *   dtau = par_c[p][r] u_g[s] A^k_L[lgas[k].coef_row[r]],   dE = par_c[p][r] u_g[s] E^k_L[lgas[k].coef_row[r]],
 * g = lgas[k].gas that gas's index in the batch, u_g its column, A^k / E^k its tables -- the term of
 * sr_limb_rays_jac_state_dev with the gas chosen per parameter; the recursion is unchanged (a parameter of gas A moves
 * only A's populations).  Column and row parameters exactly as in sr_limb_rays_jac_state_rows_dev.
 * sr_level_gas: gas in [0, n_gas), no gas twice; tab: DEVICE [n_levels][2][n_tab_rows][n_pts] (sr_glevel_pairs_dev);
 * coef_row: HOST [n_layers], each in [0, n_tab_rows).  The gases may differ in n_levels, n_tab_rows and coef_row.
 * lgas: HOST [n_lgas], 1 <= n_lgas <= n_gas; par_lgas: HOST [n_lev], each in [0, n_lgas) (may be NULL with n_lgas == 1);
 * par_level: HOST [n_lev], each a level of its gas; par_c: HOST [n_lev][n_layers]; every other argument as in
 * sr_limb_rays_jac_state_rows_dev.  jac: DEVICE [n_rays][n_col + n_lev + n_row][n_pts]: the column parameters, the level
 * parameters, the row parameters, each kind in the CALLER's order (the level parameters of the gases may be interleaved);
 * every element is written.  n_lgas == 1 is sr_limb_rays_jac_state_rows_dev itself with that gas (bit for bit); with
 * n_lev == 0 the tables and row maps are not read and may be NULL.
 * Refused before the first copy or launch, rad and jac untouched (SR_ERR_ARG unless said otherwise): n_lgas outside
 * 1 .. n_gas, a gas out of range or named twice, a NULL tab or coef_row, a coef_row value outside its gas's tables,
 * par_lgas[p] outside [0, n_lgas), par_level[p] not a level of its gas, init_mode 1; n_pts above the limit and n_levels
 * above 65536 with several gases SR_ERR_LIMIT.
 * The reference has no counterpart: the build's definition, checked against one sr_limb_rays_jac_state_rows_dev per
 * level gas, against the extended-precision recursion and against central differences (tests/test_gpu_state_gases.py). */
typedef struct sr_level_gas {
  int32_t gas;             /* index of the gas in the batch */
  int32_t n_levels;        /* levels of its pair tables */
  int32_t n_tab_rows;      /* (P, T) rows of its pair tables */
  const double *tab;       /* DEVICE [n_levels][2][n_tab_rows][n_pts] */
  const int32_t *coef_row; /* HOST [n_layers]: the table row of every coefficient row */
} sr_level_gas;
int sr_limb_rays_jac_state_gases_dev(const double *abs_c, const double *emi_c, int n_layers, int64_t n_pts,
                                     const sr_los_desc *los, int n_col, const int32_t *par_gas, const double *par_w, int n_lgas,
                                     const sr_level_gas *lgas, int n_lev, const int32_t *par_lgas, const int32_t *par_level,
                                     const double *par_c, const double *dabs_c, const double *demi_c, int n_row,
                                     const double *par_t, double *rad, double *jac, void *stream);

/* sr_limb_rays_state_bands_dev for several level-factored gases: the state arguments of
 * sr_limb_rays_jac_state_gases_dev up to par_t, then the band arguments of sr_limb_rays_state_bands_dev, with their
 * meaning, limits and refusals (a refused call leaves out untouched).  out: HOST [n_rays / 3 or n_rays][1 + n_par][n_bands],
 * rows as there with the level parameters in the caller's order.  n_lgas == 1 is sr_limb_rays_state_bands_dev itself.
 * Synchronises the stream.  Checked against sr_limb_rays_jac_state_gases_dev + the instrument step + the field of view
 * (tests/test_gpu_state_gases.py). */
int sr_limb_rays_state_bands_gases_dev(const double *abs_c, const double *emi_c, int n_layers, int64_t n_pts,
                                       const sr_los_desc *los, int n_col, const int32_t *par_gas, const double *par_w, int n_lgas,
                                       const sr_level_gas *lgas, int n_lev, const int32_t *par_lgas, const int32_t *par_level,
                                       const double *par_c, const double *dabs_c, const double *demi_c, int n_row,
                                       const double *par_t, const double *centers_nm, const double *widths_nm, int n_bands,
                                       double n_sigma, int out_units, const double *fov, double *out, void *stream);

/* sr_limb_rays_state_bands_dev / sr_limb_rays_state_bands_gases_dev with the two INSTRUMENT rows: the derivatives of the
 * radiance's bands to the band centre and to the logarithm of the ILS width (sr_hires_to_lowres_instr_shard_dev's
 * definition, window membership held fixed), from the same call: in parameter block 0 the recursion kernel multiplies the
 * wave's radiance row with the 16-band tiles of the two derivative weight tables too (the same v_mfma_f64_16x16x4 chain);
 * the hi-res radiance is never written.  The arguments, limits and refusals of the two calls; in addition
 * n_col + n_lev + n_row == 0 is allowed (the radiance and the instrument rows alone).
 * out: HOST [n_rays / 3 or n_rays][1 + n_par + 2][n_bands]: rows 0 .. n_par as the call without the instrument rows
 * returns them (bit for bit), row 1 + n_par = d / d centre (per nm), row 2 + n_par = d / d ln width.  The field of view
 * is linear in the rays' band values and is applied to the two rows as to the others.  A band whose window misses the
 * grid or holds fewer than two points is an exact 0.0 in every row.  A refused call leaves out untouched.  Synchronises
 * the stream.  Checked against the extended-precision reference (tests/test_gpu_state_bands_instr.py). */
int sr_limb_rays_state_bands_instr_dev(const double *abs_c, const double *emi_c, int n_layers, int64_t n_pts,
                                       const sr_los_desc *los, int n_col, const int32_t *par_gas, const double *par_w, int gas,
                                       const double *tab, int n_levels, int n_tab_rows, const int32_t *coef_row, int n_lev,
                                       const int32_t *par_level, const double *par_c, const double *dabs_c, const double *demi_c,
                                       int n_row, const double *par_t, const double *centers_nm, const double *widths_nm,
                                       int n_bands, double n_sigma, int out_units, const double *fov, double *out, void *stream);
int sr_limb_rays_state_bands_instr_gases_dev(const double *abs_c, const double *emi_c, int n_layers, int64_t n_pts,
                                             const sr_los_desc *los, int n_col, const int32_t *par_gas, const double *par_w,
                                             int n_lgas, const sr_level_gas *lgas, int n_lev, const int32_t *par_lgas,
                                             const int32_t *par_level, const double *par_c, const double *dabs_c,
                                             const double *demi_c, int n_row, const double *par_t, const double *centers_nm,
                                             const double *widths_nm, int n_bands, double n_sigma, int out_units,
                                             const double *fov, double *out, void *stream);

/* The mixed-state calls with the POINTING derivative: d I / d z_t of every ray's own tangent altitude (for a batch:
 * d / d delta with every z_t -> z_t + delta), the crossed shells held fixed.  In a 1-D scene a ray's radiance depends on
 * z_t through its columns only, d I / d z_t = sum_g sum_s d I / d u_g[s] d u_g[s] / d z_t: n_gas more column slots of the
 * same pass, slot g of gas g with D = d col_g / d z_t (sr_los_columns_dz's kernel, staged with the batch), added up
 * afterwards; the recursion kernel is the one of the calls without.
 * sr_limb_rays_jac_state_path_dev: the arguments of sr_limb_rays_jac_state_gases_dev with `path` in front of rad;
 * n_state = n_col + n_lev + n_row may be 0.  jac: DEVICE [n_rays][n_state + n_gas][n_pts]: rows 0 .. n_state - 1 what
 * the call without returns (bit for bit), row n_state the pointing derivative; the rows behind it are workspace.
 * sr_limb_rays_state_bands_path_dev: the arguments of sr_limb_rays_state_bands_gases_dev, then instrument (!= 0: with
 * the two instrument rows) and path.  out: HOST [n_rays / 3 or n_rays][1 + n_state + 1 (+ 2)][n_bands]: the radiance,
 * the state rows, the pointing row, the instrument rows; the per-gas rows are added on the host, before the field of
 * view (which is linear in the rays' band values).  Synchronises the stream.
 * Refused before the first copy or launch, outputs untouched: path or one of its arrays NULL (SR_ERR_ARG), los_order
 * != 0 (SR_ERR_UNSUPPORTED), and whatever the twin entries refuse.
 * The reference has no counterpart: checked against the extended-precision recursion and against central differences
 * of rebuilt batches (tests/test_gpu_pointing.py). */
int sr_limb_rays_jac_state_path_dev(const double *abs_c, const double *emi_c, int n_layers, int64_t n_pts,
                                    const sr_los_desc *los, int n_col, const int32_t *par_gas, const double *par_w, int n_lgas,
                                    const sr_level_gas *lgas, int n_lev, const int32_t *par_lgas, const int32_t *par_level,
                                    const double *par_c, const double *dabs_c, const double *demi_c, int n_row,
                                    const double *par_t, const sr_los_path *path, double *rad, double *jac, void *stream);
int sr_limb_rays_state_bands_path_dev(const double *abs_c, const double *emi_c, int n_layers, int64_t n_pts,
                                      const sr_los_desc *los, int n_col, const int32_t *par_gas, const double *par_w, int n_lgas,
                                      const sr_level_gas *lgas, int n_lev, const int32_t *par_lgas, const int32_t *par_level,
                                      const double *par_c, const double *dabs_c, const double *demi_c, int n_row,
                                      const double *par_t, const double *centers_nm, const double *widths_nm, int n_bands,
                                      double n_sigma, int out_units, const double *fov, double *out, void *stream,
                                      int instrument, const sr_los_path *path);

/* The radiance budget of the ray batch: which gas, and which level of the level-factored gas `gas`, emits the radiance
 * that arrives.  The recursion is linear in the emission: with tau = sum_g abs_g[r] u_g, t = exp(-tau), f = (1 - t) / tau
 * of a segment on coefficient row r,
 *   I = I0 T(all) + sum_s E_s f_s T(after s),   E_s = sum_g emi_g[r_s] u_{g,s},
 * and PART k, a share e_k[r] of the emission of one gas g(k), arrives as the same recursion with that share as the only
 * source and the TOTAL absorption:  C_k <- C_k t + e_k[r] u_{g(k)} f  (from 0);  the background  B <- B t  (from I0).
 *   part_level[k] = -1: gas part, e_k[r] = emi_c[part_gas[k]][r] (the whole emission of that gas);
 *   part_level[k] >= 0: level part of gas `gas` (part_gas[k] must equal gas),
 *                       e_k[r] = part_c[k][r] * E_lev[coef_row[r]], E_L = tab[L][1] of sr_glevel_pairs_dev.
 * part_c = the populations gives the level's radiance (single_rads[(gas, iso, lev)]); part_c = populations times an
 * altitude mask the radiance the level emits inside an altitude band.  Several parts may name the same level.  The gas
 * parts and B add up to I; the level parts of all levels with part_c = pop add up to the gas part; with
 * solo_absorption every part is exactly zero and B = I.
 * abs_c / emi_c: DEVICE [n_gas][n_layers][n_pts]; tab: DEVICE [n_levels][2][n_tab_rows][n_pts]; coef_row: HOST
 * [n_layers], each in [0, n_tab_rows); part_gas, part_level: HOST [n_part]; part_c: HOST [n_part][n_layers] (rows of gas
 * parts ignored); tab, coef_row and part_c may be NULL when there is no level part.  rad: DEVICE [n_rays][n_pts] or
 * NULL; parts: DEVICE [n_rays][n_part + 1][n_pts], row n_part is B, every element written.  los_order, solo_absorption
 * and init_mode 0 / 2 as the other ray-batch calls; init_mode 1 is refused (SR_ERR_ARG).  All arguments are checked
 * before the first copy or launch: a refused call leaves rad and parts untouched.
 * The reference's single_rads come from the absent spect_base_module: the build's definition, checked against
 * sr_glevel_combine_dev + sr_limb_rays_dev per part, closure and the CPU oracle's recursion (tests/test_gpu_parts.py). */
int sr_limb_rays_parts_dev(const double *abs_c, const double *emi_c, int n_layers, int64_t n_pts, const sr_los_desc *los,
                           int gas, const double *tab, int n_levels, int n_tab_rows, const int32_t *coef_row, int n_part,
                           const int32_t *part_gas, const int32_t *part_level, const double *part_c, double *rad,
                           double *parts, void *stream);

/* Radiances and their Jacobian with respect to n_par retrieval parameters on which the absorber
 * columns depend linearly, col_s = sum_p dcol_dpar[s][p] * x_p (VMR profile parameters of the
 * reference's RetParam / LinearProfile classes, spect_main_module.py:319-375; the reference's own
 * derivative code lives in the absent spect_base_module, call site spect_main_module.py:2874, so this
 * is the build's definition, parity unpinned, checked against the extended-precision reference of
 * tests/test_gpu_limb_reference.py (test_host_column_jacobian) and against finite differences).  Same recursion
 * and layouts as sr_radiance_rays_dev; dcol_dpar: HOST [n_seg][n_par]; rad: DEVICE [n_rays][n_pts];
 * jac: DEVICE [n_rays][n_par][n_pts] = d rad / d x_p. */
int sr_radiance_jac_dev(const double *abs_c, const double *emi_c, int n_layers, int64_t n_pts, int n_rays,
                        const int32_t *seg_off, const int32_t *seg_layer, const double *seg_col,
                        const double *dcol_dpar, int n_par, double *rad, double *jac, void *stream);

/* Radiance Jacobian with respect to one scalar per layer that acts through the layer's own
 * coefficients -- its temperature (BASELINE configs[3]: "Jacobians w.r.t. T ... per layer"; the
 * reference has no temperature Jacobian, spect_main_module.py:300-306 is commented out: build's
 * definition, parity unpinned, checked against the extended-precision reference of
 * tests/test_gpu_limb_reference.py (test_host_layer_jacobian) and against finite differences of the whole chain).
 * dabs / demi: DEVICE [n_layers][n_pts] = d(abs, emi of layer k)/d(parameter of layer k), e.g. central
 * differences of two sr_abscoeff_layers_dev calls at T +- dT; jac: DEVICE [n_rays][n_layers][n_pts]. */
int sr_radiance_jac_layer_dev(const double *abs_c, const double *emi_c, const double *dabs, const double *demi,
                              int n_layers, int64_t n_pts, int n_rays, const int32_t *seg_off,
                              const int32_t *seg_layer, const double *seg_col, double *jac, void *stream);

/* Instrument step that follows the path: what
 * SpectralIntensity.hires_to_lowres(lowres_obs, spectral_widths) does
 * (spect_classes.py:1180-1191) for a hi-res spectrum on the cm^-1 grid
 * w0 + j*step in 'ergscm2': conversion of grid and spectrum to nm
 * (spect_classes.py:404-407, 779-783), Gaussian ILS over +-n_sigma sigma by the
 * trapezoid rule on the irregular nm grid (spect_classes.py:883-918, 1926-1934,
 * 1162-1164), conversion to the observation's units (out_units 0 'Wm2',
 * 1 'ergscm2', 2 'nWcm2'; spect_classes.py:1200-1235).
 * rad: DEVICE [n_rays][n_pts] (the whole spectrum); centers_nm / widths_nm:
 * HOST [n_bands] (band centres and Gaussian sigmas, nm); out_host: HOST
 * [n_rays][n_bands].  Synchronises the stream. */
int sr_hires_to_lowres_dev(const double *rad, int n_rays, int64_t n_pts, double w0, double step,
                           const double *centers_nm, const double *widths_nm, int n_bands, double n_sigma,
                           int out_units, double *out_host, void *stream);
/* The same for a spectral shard: rad DEVICE [n_rays][n_pts] holds grid points g_lo .. g_lo + n_pts - 1 of the grid
 * w0 + j step; out_host receives the PARTIAL band integrals over the trapezoids between those points (bands whose
 * window misses the shard: 0).  A multi-GPU retrieval gives every rank its shard plus the next rank's first point
 * and sums the partial integrals over the ranks (one all-reduce of n_rays x n_bands doubles):
 * spect_main_module.py:2814-2818 splits the forward model spectrally in the same way. */
int sr_hires_to_lowres_shard_dev(const double *rad, int n_rays, int64_t n_pts, int64_t g_lo, double w0, double step,
                                 const double *centers_nm, const double *widths_nm, int n_bands, double n_sigma,
                                 int out_units, double *out_host, void *stream);

/* sr_hires_to_lowres_shard_dev with the two instrument derivatives of every band.  With x_i = 1e7 / g_i the nm grid,
 * t_i = (x_i - f_b) / w_b, W_i the trapezoid weights of band b (band_b = k sum_i s_i W_i over the window
 * f_b - n_sigma w_b <= x_i <= f_b + n_sigma w_b, k the unit factor), and the window's MEMBERSHIP HELD FIXED:
 *   centre f_b -> f_b + delta (nm):   d band_b / d delta = k sum_i s_i W_i t_i / w_b
 *   width  w_b -> w_b e^eta:          d band_b / d eta   = k sum_i s_i W_i (t_i^2 - 1)
 * The membership is piecewise constant in f and w; between its jumps these sums are the exact derivatives of the value,
 * and a jump (a grid point entering or leaving at +-n_sigma) is of relative size exp(-n_sigma^2 / 2).  The factors are
 * applied to the weights themselves (two more weight tables from the same pass over the window), and all three tables
 * are applied in one read of the spectrum.
 * out_host: HOST [n_rays][3][n_bands]: row 0 the value (sr_hires_to_lowres_shard_dev's, bit for bit), row 1 d / d delta,
 * row 2 d / d eta.  A band whose window holds fewer than two points or misses the grid: exact 0.0 in all rows; a shard's
 * rows are partial sums that add up over the shards.  Any parametrisation of the centres and widths (one global shift, an
 * offset and a slope, ...) is a chain rule on these rows.  Arguments, limits, refusals and status codes as
 * sr_hires_to_lowres_shard_dev.  Synchronises the stream.  Checked against an extended-precision reference
 * (tests/test_gpu_lowres_instr.py). */
int sr_hires_to_lowres_instr_shard_dev(const double *rad, int n_rays, int64_t n_pts, int64_t g_lo, double w0, double step,
                                       const double *centers_nm, const double *widths_nm, int n_bands, double n_sigma,
                                       int out_units, double *out_host, void *stream);

/* A TABULATED instrument line shape for every band integral of the calling thread.  The instrument model above is a
 * Gaussian of width w_b around f_b, cut at +-n_sigma; a measured response (an asymmetric grating channel, the lobes of an
 * FTS with their negative wings) is given as n_tab knots phi_k at the uniformly spaced REDUCED offsets
 * t_k = t_lo + k h, h = (t_hi - t_lo) / (n_tab - 1), t = (x - f_b) / w_b: one table for all bands (n_shapes = 1) or one per
 * band (n_shapes = n_bands of the calls that follow, table b for band b).  phi^ is the cubic Hermite interpolant of the
 * knots -- slopes (phi_(k+1) - phi_(k-1)) / (2 h) inside, the one-sided differences at the two ends; C1 inside
 * [t_lo, t_hi], identically 0 outside; t = t_hi is the last knot.  With p_i = g_i^2 1e-7 c_i (c_i the trapezoid interval
 * weights) over the window f_b + t_lo w_b <= x_i <= f_b + t_hi w_b (decided on the fp64 nm values; n_sigma is not used,
 * but still checked to be > 0):
 *   value:                 W_i   =  p_i phi^(t_i) / w
 *   d / d centre (per nm): W^f_i = -p_i phi^'(t_i) / w^2
 *   d / d ln width:        W^w_i = -p_i (phi^(t_i) + t_i phi^'(t_i)) / w
 * the window's membership held fixed (a jump at an end is phi^ at the table's end: keep it small).  For
 * phi = exp(-t^2 / 2) / sqrt(2 pi) these are the Gaussian's three tables.  The values are used AS GIVEN: the library does
 * not normalise (sr_ils_area gives the interpolant's exact integral to divide by).  Everything that reads the weight table
 * -- sr_hires_to_lowres[_shard|_instr_shard]_dev, sr_retrieval_forward / _step / _loop_dev, the
 * sr_limb_rays_state_bands*_dev entries and the recursion kernel's band epilogue -- then integrates with this shape;
 * their signatures, units, shards and layouts are unchanged.
 * sr_set_ils copies the table (phi: HOST [n_shapes][n_tab]); it is scoped to the calling thread and costs no launch: the
 * next band call rebuilds its weight table (the binding is part of the table's key).  NULL: the Gaussian again, as the
 * library always was.  SR_ERR_ARG for a NULL phi, n_tab < 4, n_shapes < 1, t_lo >= t_hi or not finite, a knot that is
 * not finite; SR_ERR_LIMIT for n_tab > SR_MAX_ILS_TAB; a refused descriptor leaves the binding as it was.  A band call
 * whose n_bands matches neither n_shapes == 1 nor n_shapes == n_bands returns SR_ERR_ARG before its first copy or launch.
 * Checked against an extended-precision reference (tests/test_gpu_ils.py). */
#define SR_MAX_ILS_TAB 65536
typedef struct sr_ils_desc {
  int32_t n_shapes;   /* 1, or n_bands of the calls that follow */
  int32_t n_tab;      /* 4 .. SR_MAX_ILS_TAB */
  double t_lo, t_hi;  /* t_lo < t_hi, finite */
  const double *phi;  /* HOST [n_shapes][n_tab], finite; copied by the call */
} sr_ils_desc;
int sr_set_ils(const sr_ils_desc *ils);
/* area: HOST [n_shapes], the exact integral over t of each table's interpolant,
 * sum_k h (phi_k + phi_(k+1)) / 2 + h^2 (m_k - m_(k+1)) / 12.  Refusals as sr_set_ils (and a NULL argument). */
int sr_ils_area(const sr_ils_desc *ils, double *area);

/* Absorbers without lines: a cross-section, collision-induced-absorption or extinction TABLE as a gas of the coefficient
 * rows.  The build's own definition (the reference has no counterpart).  A table is n_sets sets; set k has a
 * temperature set_temp[k] (kept for the caller's plans: the calls below take the plan, not the policy), a regular
 * wavenumber axis set_v0[k] + i set_dv[k], i < n_k = set_off[k+1] - set_off[k], and the values values[set_off[k] + i],
 * used as given (negative ones included).  At grid point j, nu_j = w0 + (double)(g_lo + j) step (unfused, as the limb
 * calls form it), t = (nu_j - v0_k) / dv_k, i = floor(t):
 *   s_k(j) = a_k[i] + (a_k[i+1] - a_k[i]) (t - i);  a_k[n_k - 1] at t == n_k - 1;  exactly 0 where t < 0 or t > n_k - 1.
 * Row r with sets (lo, hi) = set2[r], weights w2[r], their temperature derivatives dw2[r], scale c_r (1 without `scale`):
 *   abs  = c_r (w_lo s_lo + w_hi s_hi)            emi  = source ? abs B(nu_j, temps[r]) : 0
 *   dabs = c_r (dw_lo s_lo + dw_hi s_hi)          demi = source ? dabs B + abs dB/dT : 0
 * B = 2 h c^2 nu^3 / (exp(c2 nu / T) - 1), the Planck function of the limb calls' init_mode 2; the scale is held fixed
 * under d / dT.  accumulate != 0: the four outputs are added to (a point outside both of a row's sets is left as it is;
 * without a source emi / demi are left as they are).
 * sr_abs_table_create: all arrays HOST, copied; the handle is device-resident on the current device.  SR_ERR_ARG: a NULL
 * argument, n_sets <= 0, set_off[0] != 0, a set shorter than 2, dv <= 0 or not finite, v0 not finite, a temperature <= 0 or
 * not finite; SR_ERR_LIMIT: n_sets > SR_MAX_ABS_SETS or more than SR_MAX_ABS_VALUES values.
 * sr_abs_table_layers_dev: temps, scale (or NULL), set2, w2, dw2 (or NULL) are HOST arrays of n_rows rows, staged through
 * the calling thread's pinned ring (no stream is made); abs_out, emi_out, dabs_out, demi_out DEVICE [n_rows][n_pts],
 * dabs_out / demi_out NULL: no derivative.  Runs on `stream` (hipStream_t), ordered after the handle's creation; the
 * handle belongs to the device it was made on, and sr_abs_table_destroy waits for its last call.  Every argument is
 * checked before the first copy or launch and a refused call leaves the outputs untouched:
 * SR_ERR_ARG for a NULL handle, temps, set2, w2, abs_out or emi_out, n_rows <= 0, n_pts <= 0, g_lo < 0, a set index
 * outside 0 .. n_sets - 1, a temperature <= 0 or not finite, a scale, weight, w0 or step that is not finite, dabs_out
 * without dw2, exactly one of dabs_out / demi_out with a source, the handle on another device; SR_ERR_LIMIT for
 * n_pts > 2000000, g_lo + n_pts > INT32_MAX or n_rows > SR_MAX_ABS_ROWS.
 * Checked against an extended-precision reference (tests/test_gpu_absorber_table.py). */
#define SR_MAX_ABS_SETS 4096
#define SR_MAX_ABS_VALUES 134217728 /* 2^27: 1 GiB of values */
#define SR_MAX_ABS_ROWS 65536
typedef struct sr_abs_table sr_abs_table;
int sr_abs_table_create(int n_sets, const double *set_temp, const double *set_v0, const double *set_dv, const int64_t *set_off,
                        const double *values, sr_abs_table **out);
int sr_abs_table_destroy(sr_abs_table *h);
int sr_abs_table_layers_dev(sr_abs_table *h, int n_rows, const double *temps, const double *scale, const int32_t *set2,
                            const double *w2, const double *dw2, double w0, double step, int64_t g_lo, int64_t n_pts,
                            int source, int accumulate, double *abs_out, double *emi_out, double *dabs_out, double *demi_out,
                            void *stream);

/* Single-scattering solar source of coefficient rows: sunlight, attenuated on its way in, scattered once into the line of
 * sight, as an emission coefficient like any other.  The build's own definition (the reference has no counterpart;
 * DESIGN.md).  For output row r (a layer of a 1-D scene or a LOS step of a 3-D batch) and grid point j:
 *   tau[r][j] = sum_{k < n_k} u[r][k] tab_abs[k][j]          n_k = n_gas n_layers, k = g n_layers + l
 *   S[r][j]   = w[r] sun[j] exp(-tau[r][j])                  exactly 0 where w[r] == 0 or tau >= 700
 *   emi_out[r][j] (+)= sca_abs[src_row[r]][j] S[r][j]
 * u[r][k] >= 0: the slant column of gas g in layer l along the straight ray from the row's point towards the sun (dense,
 * mostly zeros, read as it is); w[r] = albedo x phase function / 4 pi, 0 for a row in shadow: its optical depth is not
 * evaluated, its output an exact 0, and with accumulate != 0 the row of emi_out is left untouched.  tab_abs DEVICE
 * [n_k][n_pts] (the stacked absorption rows of the scene), sca_abs DEVICE [n_src][n_pts] (the scatterer's own absorption
 * rows), sun DEVICE [n_pts] (the solar irradiance on the grid, in units consistent with the scene's emission rows), emi_out
 * DEVICE [n_rows][n_pts]; trans_out DEVICE [n_rows][n_pts] or NULL: exp(-tau) itself, 1 for a row without columns, 0 in
 * shadow and where tau >= 700.  accumulate != 0 adds to emi_out.  Every Jacobian of the library treats these rows as
 * coefficients: the solar attenuation is held fixed under d / d(VMR, T, Tvib) within one linearisation.
 * The descriptor's arrays are HOST arrays, staged through the calling thread's pinned ring (no stream is made) with the
 * lists of the chunks of four k in which any lit row of a tile of 16 rows has a column; chunks that are not listed
 * would only have added exact zeros, so the result does not depend on the lists (sr_set_solar_full_lists(1) lists every
 * chunk on the calling thread until it is set back: the check of that, not a mode of use).  One fused fp64 kernel (v_mfma_f64_16x16x4 + the exponential) on `stream`; one writer per element, no
 * atomics, the same call gives the same bits.  Every argument is checked before the first copy or launch and a refused
 * call leaves the outputs untouched: SR_ERR_ARG for a NULL desc, u, w, src_row, tab_abs, sca_abs, sun or emi_out,
 * n_rows <= 0, n_k <= 0, n_src <= 0, n_pts <= 0, a u or w that is negative or not finite, a src_row outside
 * 0 .. n_src - 1; SR_ERR_LIMIT for n_rows > SR_MAX_ABS_ROWS, n_rows n_k > SR_MAX_SOLAR_VALUES (the staged tile of u:
 * 64 MiB of pinned memory per slot of the ring) or n_pts > 2000000.  The ring has four slots that grow and are kept: a
 * thread that made calls of the largest size retains up to 256 MiB of pinned host memory and as much device memory.
 * sr_solar_chunk_lists: the lists alone, on the host (no GPU): tile_off HOST [ceil(n_rows / 16) + 1], chunks HOST
 * [ceil(n_rows / 16) ceil(n_k / 4)] (room for every chunk), *n_listed the number listed; the descriptor's checks
 * without src_row's range.  Checked against an extended-precision reference (tests/test_gpu_solar_source.py). */
#define SR_MAX_SOLAR_VALUES 8388608 /* 2^23 */
typedef struct {
  int32_t n_rows;
  const double *u;        /* [n_rows][n_k] */
  const double *w;        /* [n_rows] */
  const int32_t *src_row; /* [n_rows] */
} sr_solar_desc;
int sr_set_solar_full_lists(int on);
int sr_solar_chunk_lists(const sr_solar_desc *desc, int n_k, int32_t *tile_off, int32_t *chunks, int32_t *n_listed);
int sr_solar_source_rows_dev(const sr_solar_desc *desc, const double *tab_abs, int n_k, const double *sca_abs, int n_src,
                             const double *sun, int64_t n_pts, int accumulate, double *emi_out, double *trans_out,
                             void *stream);

/* The solar attenuation in the Jacobians: d radiance / d (column parameter) THROUGH the optical depth of the solar source.
 * The build's own definition.  For parameter p, ray y and grid point j:
 *   dtau[p][r][j] = sum_{k < n_k} du[p][r][k] tab_abs[k][j]
 *   jac[y][par_slot[p]][j] (+)= - sum_{r < n_rows} q[y][r][j] dtau[p][r][j]
 * du HOST [n_par][n_rows][n_k] = d u[r][k] / d x_p (geometry.solar_column_weights: any finite sign, dense, mostly zeros,
 * read as it is); tab_abs DEVICE [n_k][n_pts] as above; q DEVICE [n_rays][n_rows][n_pts], finite: d rad[y] / d eps_r for
 * emi[r] -> emi[r] + eps_r (the solar rows of r alone), i.e. sr_limb_rays_jac_layer_dev with dabs = 0 and demi = those
 * rows; jac DEVICE [n_rays][n_jac_rows][n_pts], parameter p in row par_slot[p] (HOST [n_par], each row named at most
 * once), the rows not named are left as they are; accumulate != 0 adds to the rows named (a parameter whose du is all
 * zero then leaves its row unread).  With a derivative table in tab_abs' place (d abs / d T) the same call gives the
 * term of a temperature parameter.  du and par_slot are staged through the calling thread's pinned ring (no stream is
 * made) with the chunk lists per (parameter, tile of 16 rows); chunks and tiles that are not listed would only have added
 * exact zeros (sr_set_solar_full_lists(1) lists every one: the check of that).  One fused fp64 kernel
 * (v_mfma_f64_16x16x4, then the product with q and the row sum) on `stream`; one writer per element, no atomics, the same
 * call gives the same bits.  Every argument is checked before the first copy or launch and a refused call leaves jac
 * untouched: SR_ERR_ARG for a NULL desc, du, tab_abs, q, par_slot or jac, n_par <= 0, n_rows <= 0, n_k <= 0, n_rays <= 0,
 * n_pts <= 0, n_jac_rows <= 0, a du that is not finite, a par_slot outside 0 .. n_jac_rows - 1 or named twice;
 * SR_ERR_LIMIT for n_rows > SR_MAX_ABS_ROWS, n_par n_rows n_k > SR_MAX_SOLAR_VALUES, n_pts > 2000000, or more than
 * INT32_MAX blocks (8 ceil(n_pts / 2048) n_par ceil(n_rays / 8)).
 * sr_solar_jacobian_chunk_lists: the lists alone, on the host (no GPU): tile_off HOST [n_par ceil(n_rows / 16) + 1] (the
 * tiles of parameter p from p ceil(n_rows / 16) on), chunks HOST [n_par ceil(n_rows / 16) ceil(n_k / 4)] (room for every
 * chunk), *n_listed the number listed.  Checked against an extended-precision reference (tests/test_gpu_solar_jacobian.py). */
typedef struct {
  int32_t n_par;
  int32_t n_rows;
  const double *du; /* [n_par][n_rows][n_k] */
} sr_solar_jac_desc;
int sr_solar_jacobian_chunk_lists(const sr_solar_jac_desc *desc, int n_k, int32_t *tile_off, int32_t *chunks, int32_t *n_listed);
int sr_solar_jacobian_rows_dev(const sr_solar_jac_desc *desc, const double *tab_abs, int n_k, const double *q, int n_rays,
                               int64_t n_pts, const int32_t *par_slot, double *jac, int n_jac_rows, int accumulate,
                               void *stream);

/* Multiple scattering of sunlight: the diffuse field of a plane-parallel two-stream solve per grid point, with delta
 * scaling and a Lambertian lower boundary, as emission rows of a scatterer.  The build's own definition.
 * Layers l = 0 .. N-1 bottom to top (N = n_layers), interfaces i = 0 .. N; per layer and grid point j, with
 * t_g = v[g][l] tab_abs[g N + l][j] and f_g = max(asym_g, 0)^2:
 *   sigma' = sum ssa_g (1 - f_g) t_g, alpha = sum (1 - ssa_g) t_g, dtau' = sigma' + alpha,
 *   co = max(alpha / dtau', 2^-52), omega' = 1 - co, g' = sum ssa_g (asym_g - f_g) t_g / sigma' (0 where sigma' == 0)
 * and the quadrature two-stream equations of Meador & Weaver (1980), tau downward, the source that of the layer's middle:
 *   dF+/dtau = gamma1 F+ - gamma2 F- - S+,  dF-/dtau = gamma2 F+ - gamma1 F- + S-,
 *   gamma1 -+ gamma2 = sqrt3 co, sqrt3 (1 - omega' g'),  gamma3 = (1 - sqrt3 g' mu0) / 2,
 *   S+ = omega' D gamma3, S- = omega' D (1 - gamma3), D = sun[j] beam[l][j]
 * with F-(top) = 0, F+(bottom) = surface_albedo (F-(bottom) + max(mu0, 0) sun[j] beam[N][j]) and F+- continuous at the
 * interfaces; a layer with dtau' == 0 passes light through unchanged.  Outputs:
 *   J_l[j] = sqrt3 (F+_l + F-_l + F+_{l+1} + F-_{l+1}) / (8 pi)          the mean diffuse intensity of layer l
 *   emi_out[l][j] (+)= ssa_G (1 - f_G) tab_abs[G N + l][j] J_l[j]        G = out_gas
 * The diffuse field holds light scattered once or more; scattered into the line of sight it is orders two and above
 * (order one stays sr_solar_source_rows_dev's, with the exact phase function and the unscaled beam).  The direction-
 * dependent term of the diffuse source is dropped.  Every output is >= 0; emi_out is an exact 0 for ssa_G == 0, every
 * output where sun beam is 0 on all rows and surface_albedo is 0, or every ssa is 0 and surface_albedo is 0.
 * desc: v HOST [n_gas][n_layers] >= 0, the vertical column of gas g in layer l; ssa HOST [n_gas] in [0, 1]; asym HOST
 * [n_gas] in [-0.5, 1); mu0 in [-1, 1]; surface_albedo in [0, 1].  tab_abs DEVICE [n_gas n_layers][n_pts] (the stacked
 * absorption rows, as sr_solar_source_rows_dev takes them); beam DEVICE [n_layers + 1][n_pts] in [0, 1]: the transmission
 * of the direct beam at the layers' middle points and, row n_layers, at the lower boundary (the caller makes it, e.g. by
 * sr_solar_source_rows_dev's trans_out with delta-scaled columns); sun DEVICE [n_pts] >= 0.  emi_out DEVICE
 * [n_layers][n_pts], or NULL with out_gas = -1; j_out DEVICE [n_layers][n_pts] or NULL; flux_out DEVICE
 * [2][n_layers + 1][n_pts] or NULL: F+, then F-, at the interfaces.  accumulate != 0 adds to emi_out.
 * v and the per-gas coefficients are staged through the calling thread's pinned ring (no stream is made).  One thread
 * per grid point walks the layers up, leaving four doubles per (layer, point) in a workspace of the calling thread (grow-
 * only, at most 256 MiB per device; a larger call runs in point chunks, one launch after the other), and down again; the
 * calls of one thread share that workspace, so they belong on one stream at a time.  One writer per element, no atomics,
 * the same call gives the same bits.  Every argument is checked before the first copy or launch and a refused call
 * leaves the outputs untouched: SR_ERR_ARG for a NULL desc, v, ssa, asym, tab_abs, beam or sun, n_gas <= 0,
 * n_layers <= 0, n_pts <= 0, a v, ssa, asym, mu0 or surface_albedo that is not finite or outside its range, an out_gas
 * outside -1 .. n_gas - 1, emi_out without out_gas or out_gas without emi_out, all three outputs NULL; SR_ERR_LIMIT for
 * n_gas > 8, n_layers > SR_MAX_ABS_ROWS or n_pts > 2000000.
 * Checked against an extended-precision reference (tests/test_gpu_diffuse_source.py). */
typedef struct {
  int32_t n_gas, n_layers;
  const double *v, *ssa, *asym; /* [n_gas][n_layers], [n_gas], [n_gas] */
  double mu0, surface_albedo;
} sr_diffuse_desc;
int sr_diffuse_source_rows_dev(const sr_diffuse_desc *desc, const double *tab_abs, const double *beam, const double *sun,
                               int64_t n_pts, int out_gas, int accumulate, double *emi_out, double *j_out, double *flux_out,
                               void *stream);

/* Thermal emission as a source of the same two-stream diffuse field: alone (the night side, thermal windows) or together
 * with the sun's in one walk of the layers.  The build's own definition; notation, equations, boundary
 * conditions and outputs are sr_diffuse_source_rows_dev's.  The thermal source of layer l is isotropic and constant over
 * the layer, at the layer's own temperature:
 *   S+ = S- = 2 pi co B_l,   B_l = B(nu_j, T_l) = 2 h c^2 nu_j^3 / (exp(c2 nu_j / T_l) - 1),  nu_j = w0 + (g_lo + j) step
 * so that a layer with nothing coming in sends out E+_th = E-_th = (2 pi / sqrt3) B_l (1 - R - T) (Kirchhoff's law for
 * the layer; R, T its two-stream reflection and transmission), added to the solar E+- where there is a sun.  A layer with
 * alpha == 0 at a point has a thermal source of exactly 0 there (the floor of co invents no emission).  A Lambertian
 * surface of emissivity 1 - surface_albedo at t_surface adds (1 - surface_albedo) (2 pi / sqrt3) B(nu_j, t_surface) to
 * the upwelling at the lower boundary (the two-stream value: everything at one temperature gives J = B exactly);
 * t_surface = 0 is no emitting surface.  F-(top) = 0.  The rows:
 *   own_emission == 0:  emi_out[l][j] (+)= ssa_G (1 - f_G) tab_abs[G N + l][j] J_l[j]
 *   own_emission != 0:  emi_out[l][j] (+)= tab_abs[G N + l][j] ((1 - ssa_G) B_l + ssa_G (1 - f_G) J_l[j])
 * the second the scatterer's complete thermal row: its own emission by Kirchhoff's law and the scattered field.  Deep
 * inside a thick isothermal column it tends to tab_abs B (1 - ssa_G f_G): for asym > 0 the forward peak's share of the
 * line-of-sight source is left out, as it is for the solar rows.  Every output is >= 0, and an exact 0 where no layer has
 * an absorber, no surface emits and no sun shines.
 * desc, tab_abs, n_pts, out_gas, accumulate, emi_out, j_out, flux_out, stream: as sr_diffuse_source_rows_dev takes them.
 * beam and sun: both given (as the sibling takes them), or both NULL for thermal emission alone; desc->mu0 is not read
 * when both are NULL.  th: temps HOST [n_layers] > 0, the layers' temperatures; t_surface >= 0; w0, step, g_lo: the
 * spectral grid of the points; own_emission: the rows' form.  B is evaluated in the kernel as sr_abs_table_layers_dev
 * evaluates it (no array of Planck values is made); the night call reads tab_abs alone.  Kernel layout, workspace, point
 * chunks above 256 MiB, staging through the calling thread's pinned ring (temps with v) and the one-stream rule are the
 * sibling's.  One writer per element, no atomics, the same call gives the same bits.  Every argument is checked before
 * the first copy or launch and a refused call leaves the outputs untouched: the sibling's refusals (beam and sun as
 * above), and SR_ERR_ARG for a NULL th or temps, a temperature <= 0 or not finite, t_surface < 0 or not finite, a w0 or
 * step that is not finite, g_lo < 0, exactly one of beam and sun, own_emission without emi_out; SR_ERR_LIMIT for
 * g_lo + n_pts > INT32_MAX.
 * Checked against an extended-precision reference (tests/test_gpu_diffuse_thermal.py). */
typedef struct {
  const double *temps; /* HOST [n_layers], > 0 */
  double t_surface, w0, step;
  int64_t g_lo;
  int32_t own_emission;
} sr_diffuse_thermal_desc;
int sr_diffuse_thermal_rows_dev(const sr_diffuse_desc *desc, const sr_diffuse_thermal_desc *th, const double *tab_abs,
                                const double *beam, const double *sun, int64_t n_pts, int out_gas, int accumulate,
                                double *emi_out, double *j_out, double *flux_out, void *stream);

/* The diffuse field for several columns of illumination over one atmosphere, and the emission rows of LOS steps that
 * see it: a 3-D limb batch, whose steps each have their own solar zenith angle.  The build's own definition (DESIGN.md
 * 4.11e).  For column c < n_col, with mu0[c] and beam[c] [n_layers + 1][n_pts], J[c][l][j] and F+-[c][i][j] are exactly
 * what sr_diffuse_source_rows_dev defines for (desc's v, ssa, asym, surface_albedo; mu0[c], beam[c]): the atmosphere and
 * its optics are shared, only the illumination differs, and the columns are independent.  Then for output row r < n_rows
 *   emi_out[r][j] (+)= ssa_G (1 - f_G) sca_abs[src_row[r]][j] sum_c col_w[r][c] J[c][row_layer[r]][j]      G = out_gas
 * c ascending, the sum started from its first term; every addend is >= 0.  A row whose weights are all zero is an exact
 * 0, and under accumulate its row of emi_out keeps its bits; the same holds for every row when ssa_G == 0.
 * desc: as sr_diffuse_source_rows_dev takes it; its mu0 is not read.  cols: mu0 HOST [n_col], each in [-1, 1]; col_w HOST
 * [n_rows][n_col], finite and >= 0 (e.g. linear interpolation in mu between the columns); row_layer HOST [n_rows], the
 * layer 0 .. n_layers - 1 of every row, in any order, a layer any number of times; src_row HOST [n_rows], 0 .. n_src - 1.
 * tab_abs and sun as the sibling takes them; beam DEVICE [n_col][n_layers + 1][n_pts]; sca_abs DEVICE [n_src][n_pts], the
 * scatterer's absorption on the rows' own places.  emi_out DEVICE [n_rows][n_pts], or NULL with out_gas = -1 and
 * n_rows = 0; j_out DEVICE [n_col][n_layers][n_pts] or NULL; flux_out DEVICE [n_col][2][n_layers + 1][n_pts] or NULL.
 * One thread per grid point walks the layers once for all columns: the layer operators R, T, 1 - R, 1 - R - T and the
 * elimination are formed once, the sources per column from two shared factors (E+ + E- = D fs, E+ - E- = D mu0 fd), and
 * the rows are written from the downward sweep, so J goes to memory only where j_out asks for it.  The roundings differ
 * from sr_diffuse_source_rows_dev's in the sources; both stay inside the reference's bound.  A column's j_out and
 * flux_out bits do not depend on which other columns share the call.  A call runs the kernel instance of the next
 * column count of 1, 2, 4, 8.  v, the coefficients, mu0, col_w, src_row and the rows sorted by layer are staged through
 * the calling thread's pinned ring; the workspace, 2 + 2 x (instance's columns) doubles per (layer, point), is the
 * sibling's (grow-only, at most 256 MiB per device, a larger call runs in point chunks; one stream at a time per thread).
 * One writer per element, no atomics, the same call gives the same bits.  Every argument is checked before the first
 * copy or launch and a refused call leaves the outputs untouched: SR_ERR_ARG for a NULL desc, v, ssa, asym, cols, mu0,
 * tab_abs, beam or sun, with rows a NULL col_w, row_layer, src_row or sca_abs or n_src <= 0, n_gas <= 0, n_layers <= 0,
 * n_pts <= 0, n_col <= 0, n_rows < 0, a v, ssa, asym, surface_albedo, mu0, col_w, row_layer or src_row that is not
 * finite or outside its range, an out_gas outside -1 .. n_gas - 1, emi_out without out_gas or without rows and the
 * reverse, all three outputs NULL; SR_ERR_LIMIT for n_col > SR_MAX_DIFFUSE_COLUMNS, n_rows > SR_MAX_ABS_ROWS, n_gas > 8,
 * n_layers > SR_MAX_ABS_ROWS or n_pts > 2000000.
 * Checked against an extended-precision reference (tests/test_gpu_diffuse_columns.py). */
#define SR_MAX_DIFFUSE_COLUMNS 8
typedef struct {
  int32_t n_col, n_rows;
  const double *mu0;          /* HOST [n_col], each in [-1, 1] */
  const double *col_w;        /* HOST [n_rows][n_col], finite, >= 0 */
  const int32_t *row_layer;   /* HOST [n_rows], 0 .. n_layers-1, any order, a layer any number of times */
  const int32_t *src_row;     /* HOST [n_rows], 0 .. n_src-1 */
} sr_diffuse_columns_desc;
int sr_diffuse_source_columns_dev(const sr_diffuse_desc *desc, const sr_diffuse_columns_desc *cols,
                                  const double *tab_abs, const double *beam, const double *sun, int64_t n_pts,
                                  const double *sca_abs, int n_src, int out_gas, int accumulate,
                                  double *emi_out, double *j_out, double *flux_out, void *stream);

/* The diffuse rows in the Jacobians: d radiance / d (column parameter) THROUGH the two-stream solve of
 * sr_diffuse_source_rows_dev.  The build's own definition.  A parameter x_p moves, per layer l and grid
 * point j, in the notation above,
 *   d t_g[l] = dv[p][g][l] tab_abs[g N + l][j],   d D_l = D_l dlnbeam[p][l][j],   d Ub_0 = Ub_0 dlnbeam[p][N][j]
 * (Ub_0 = surface_albedo max(mu0, 0) sun beam[N], the boundary's term) and dJ[p][l][j] is the tangent of J_l along that
 * direction, of the function AS BUILT: co = max(alpha / dtau', 2^-52) has derivative 0 where the floor holds, g' = 0 where
 * sigma' == 0 has derivative 0 there, and a layer with dtau' == 0 passes light through whatever dv says (every derivative
 * of its operators is 0).  Then
 *   jac[y][par_slot[p]][j] (+)= sum_{l < N} q[y][l][j] dJ[p][l][j]            l ascending, one writer per element
 * with q[y][l] = d rad[y] / d J_l: sr_limb_rays_jac_layer_dev with dabs = 0 and demi[g] = ssa_g (1 - f_g) tab_abs[g] for
 * every solar gas (per unit J, so that a row in shadow, J = 0, enters no division).
 * desc: as sr_diffuse_source_rows_dev takes it, the state the tangent is taken at.  jdesc: dv HOST [n_par][n_gas][n_layers]
 * = d v / d x_p (geometry.vertical_column_weights: any finite sign, dense, mostly zeros, read as it is).  tab_abs, beam, sun:
 * as above.  dlnbeam DEVICE [n_par][n_layers + 1][n_pts] = d ln beam / d x_p, finite, row n_layers the boundary's, or NULL:
 * the beam is held fixed.  q DEVICE [n_rays][n_layers][n_pts], finite, and jac DEVICE [n_rays][n_jac_rows][n_pts] come
 * together, or both NULL with dj_out; parameter p in row par_slot[p] (HOST [n_par], each row named at most once), the rows
 * not named are left as they are; accumulate != 0 adds to the rows named.  dj_out DEVICE [n_par][n_layers][n_pts] or NULL:
 * dJ itself (always overwritten), the counterpart of j_out.
 * v, dv, the per-gas coefficients, par_slot and per parameter the range of layers with any non-zero dv (made on the host
 * before any device work; outside it the layer operators stand still and only the sources follow the beam) are staged
 * through the calling thread's pinned ring (no stream is made).  Two kernels on `stream`: one thread per grid point and
 * tile of four parameters walks the layers up and down with the tangents beside the base quantities (19 doubles per
 * (tile, layer, point) in the source's workspace, 23 without dj_out), then the product with q as a register tile of
 * 8 rays x 4 parameters.  A call whose workspace would pass 256 MiB runs in point chunks and groups of parameter tiles, one
 * launch after the other: a parameter's rows do not depend on the tile it stands in, a point's not on its chunk.  The
 * workspace is the one sr_diffuse_source_rows_dev uses, one per (calling thread, device): the calls of one thread to
 * either entry belong on one stream at a time (two streams would race on it).  No
 * atomics, the same call gives the same bits.  Every argument is checked before the first copy or launch and a refused
 * call leaves the outputs untouched, in this order: SR_ERR_ARG for a NULL desc, v, ssa, asym, jdesc, dv, tab_abs, beam or
 * sun, n_gas <= 0, n_layers <= 0, n_pts <= 0, n_par <= 0, q without jac or jac without q, neither jac nor dj_out, jac
 * without par_slot or with n_rays <= 0 or n_jac_rows <= 0, a v, ssa, asym, mu0 or surface_albedo that is not finite or
 * outside its range; SR_ERR_ARG for a dv that is not finite; SR_ERR_LIMIT for n_gas > 8, n_layers > SR_MAX_ABS_ROWS,
 * n_pts > 2000000 or n_par n_gas n_layers > SR_MAX_SOLAR_VALUES; SR_ERR_ARG for a par_slot outside 0 .. n_jac_rows - 1 or
 * named twice.  Checked against an extended-precision reference (tests/test_gpu_diffuse_jacobian.py). */
typedef struct {
  int32_t n_par;
  const double *dv; /* [n_par][n_gas][n_layers] */
} sr_diffuse_jac_desc;
int sr_diffuse_jacobian_rows_dev(const sr_diffuse_desc *desc, const sr_diffuse_jac_desc *jdesc, const double *tab_abs,
                                 const double *beam, const double *sun, const double *dlnbeam, const double *q, int n_rays,
                                 int64_t n_pts, const int32_t *par_slot, double *jac, int n_jac_rows, int accumulate,
                                 double *dj_out, void *stream);

/* The diffuse rows along a direction in the haze optics: d radiance / d (ssa, asym, surface_albedo) THROUGH the two-stream
 * solve of sr_diffuse_source_rows_dev.  The build's own definition.  Parameter p moves ssa_g by
 * dssa[p][g], asym_g by dasym[p][g] and surface_albedo by dalb[p]; the per-gas coefficients as built move by
 *   f = max(asym, 0)^2, df = 2 max(asym, 0) dasym (0 for asym <= 0)
 *   d(ssa (1 - f)) = dssa (1 - f) - ssa df,  d(1 - ssa) = -dssa,  d(ssa (asym - f)) = dssa (asym - f) + ssa (dasym - df)
 * and per layer and grid point the three sums by these times t_g = v[g][l] tab_abs[g N + l][j], the source by
 * d D_l = D_l dlnbeam[p][l][j], the boundary by
 *   d Rb_0 = dalb[p],   d Ub_0 = Ub_0 dlnbeam[p][N][j] + dalb[p] max(mu0, 0) sun[j] beam[N][j]
 * (no division by the albedo: 0 is an ordinary state).  dJ[p][l][j] is the tangent of J_l of the function AS BUILT, with
 * sr_diffuse_jacobian_rows_dev's three rules (the floor of co, g' = 0 where sigma' == 0, an empty layer), and
 *   jac[y][par_slot[p]][j] (+)= sum_{l < N} q[y][l][j] dJ[p][l][j]            l ascending, one writer per element
 * by the contraction kernel of sr_diffuse_jacobian_rows_dev.  desc, tab_abs, beam, sun, dlnbeam, q, n_rays, n_pts,
 * par_slot, jac, n_jac_rows, accumulate, dj_out, stream: as sr_diffuse_jacobian_rows_dev takes them.  odesc: dssa and
 * dasym HOST [n_par][n_gas], either may be NULL (zeros: a direction in the albedo only); dalb HOST [n_par] or NULL
 * (zeros); finite, any sign.  The coefficients' tangents and per parameter the range of layers in which a gas with a
 * non-zero tangent has a column (empty for a direction in the albedo alone: the operators of every layer stand still and
 * only the boundary's terms are carried upward) are made on the host and staged through the calling thread's pinned
 * ring.  Kernels, workspace, chunks, tiles and the one-stream rule: those of sr_diffuse_jacobian_rows_dev, the tangent
 * kernel in its optics instance (four parameters per tile).  Every argument is checked before the first copy or launch
 * and a refused call leaves the outputs untouched, in the order of sr_diffuse_jacobian_rows_dev: SR_ERR_ARG for a NULL
 * desc, v, ssa, asym, odesc, tab_abs, beam or sun or dssa, dasym and dalb all NULL, n_gas <= 0, n_layers <= 0, n_pts <= 0,
 * n_par <= 0, q without jac or jac without q, neither jac nor dj_out, jac without par_slot or with n_rays <= 0 or
 * n_jac_rows <= 0, a v, ssa, asym, mu0 or surface_albedo that is not finite or outside its range; SR_ERR_ARG for a dssa,
 * dasym or dalb that is not finite; SR_ERR_LIMIT for n_gas > 8, n_layers > SR_MAX_ABS_ROWS, n_pts > 2000000 or
 * n_par n_gas n_layers > SR_MAX_SOLAR_VALUES; SR_ERR_ARG for a par_slot outside 0 .. n_jac_rows - 1 or named twice.
 * Checked against an extended-precision reference (tests/test_gpu_diffuse_optics.py). */
typedef struct {
  int32_t n_par;
  const double *dssa, *dasym, *dalb; /* [n_par][n_gas] x2, [n_par] */
} sr_diffuse_optics_desc;
int sr_diffuse_optics_jacobian_rows_dev(const sr_diffuse_desc *desc, const sr_diffuse_optics_desc *odesc, const double *tab_abs,
                                        const double *beam, const double *sun, const double *dlnbeam, const double *q, int n_rays,
                                        int64_t n_pts, const int32_t *par_slot, double *jac, int n_jac_rows, int accumulate,
                                        double *dj_out, void *stream);

/* Evaluation mode of the coefficient op.  Far region-1 wings by local Taylor expansions per box of grid
 * points (truncation <= sr_far_field_truncation_bound() of a line's own contribution: 1.6e-11 as built by default, degree
 * 19; 2.6e-13 with -DSR_KFD=22; a box takes a line from sr_far_field_min_distance() on), near field exact, with the expansions built
 * 2: from box pairs -- multipole moments of the lines of a source box (sr_s2m_kernel, sr_m2m_kernel)
 *    translated to every well-separated target box of the level (sr_m2l_kernel), per-line expansions only for
 *    the (line, box) pairs no box pair covers;
 * 1: per line and box at every level (sr_farfield_kernel);
 * 3 (default): 2 -- except for line sets with fewer than 0.35 lines per grid point (the per-level sub-linesets of the
 *    pair tables and look-up tables), which take 1: the box pairs cost S2M / M2M / M2L over every box whatever it
 *    holds;
 * 0: every (line, point) evaluated exactly (sr_abscoeff_wings_kernel + sr_abscoeff_cores_kernel). */
int sr_set_far_field(int on);
/* Far-field mode only: how the kernels of a call share the chip.  1 (default): the decoupled, phased pipeline -- the
 * table preparation, the far-field chain (level-0 pass | S2M -> M2M -> M2L) and the zones kernel run on internal
 * streams on scratch of the call's parity, each as soon as what it reads is ready (the preparation of call c + 1
 * while call c computes), the zones kernel gated behind the level-0 pass and S2M of its own call; only the wings
 * kernel, which writes abs_out / emi_out, is on the caller's stream.  0: the kernels one after the other on the
 * caller's stream (per-kernel times for sr_last_kernel_ms; what the exact mode and counting passes always run).  The
 * caller's stream sees the op complete in order in both modes. */
int sr_set_overlap(int on);
/* Measurement hook of the serial schedule (sr_set_overlap(0)) only: kernel `kernel` of every coefficient op is launched n
 * times back to back -- 0 sr_prep_kernel, 1 level-0 far-field pass, 2 S2M + M2M, 3 M2L, 4 zones, 5 wings; -1: off -- so
 * that ONE kernel can run for seconds beside a power sampler (tools/energy_by_kernel.py).  The call's results are not
 * meaningful while a repeat is set (a repeated M2L adds into its coefficients, the repeated zones kernel stores over the
 * wings kernel's sums). */
int sr_set_kernel_repeat(int kernel, int n);
/* Memory knob: the per-(line, layer) record tables (128 B each, plus the far-field scratch of a layer) of one launch are kept
 * under this many bytes (default 48 GiB of the 288 GB); a longer layer stack (the reference
 * allows imxstp = 8000 LOS steps) is processed in batches of layers. */
int sr_set_table_budget(int64_t bytes);
/* Radiance Jacobians of the device LOS pipeline (sr_limb_rays_jac_dev with more than 8 parameters,
 * sr_limb_rays_jac_layer_dev with more than 8 layers, sr_limb_rays_jacobians_dev).  0 (default): one pass over each
 * ray, every segment's sensitivity times the transmission behind it added to the rows it acts on
 * (sr_limb_adjoint_kernel); where the rays walk their shells -- the coefficient rows, or with seg_jac_row the Jacobian
 * rows -- monotonically inwards and outwards again (limb, slant and nadir paths), the FOLDED kernel: the shells are
 * walked once per sweep, a ray's far-side and near-side segment of a shell together, two rays per thread, every
 * Jacobian value stored once (sr_limb_adjoint_fold_kernel; what enters a near-side segment is taken as the observed
 * radiance minus what the segments in front of it emit: values agree with mode 2 to ~1e-15 of the radiance x d tau).
 * 1: the forward-sensitivity kernels always (they carry 16 derivatives through the recursion and repeat it per block
 * of 16) -- kept as the check of the others.  2: one pass per ray in path order, one ray per thread, always.
 * 3: path order, two rays per thread sharing a shell's coefficient loads (sr_limb_adjoint_sync_kernel; the bits of 2). */
int sr_set_jac_layer_mode(int forward);
/* The far field's truncation bound, relative to a line's own contribution at the point: 18 theta^-(degree + 1) of the
 * library as built (theta = 4, degree 19: 1.6e-11; -DSR_KFD=22: 2.6e-13).  The exact mode (sr_set_far_field(0)) has none.
 * What the far-field mode may differ by from the exact mode and from the CPU oracle beyond rounding. */
double sr_far_field_truncation_bound(void);
/* The admissibility rule that holds that bound, as the kernels apply it: a box of level `level` (64 << level grid points,
 * 0 <= level < 5) takes a line by its expansion when the box's centre is at least this many grid points from the line's
 * centre index -- 4 half-widths + pole_margin, the layer's pole margin in grid points (ceil(0.71 dw' / step) + 1 with
 * the layer's largest Doppler width dw'), and from level 1 upwards a margin of 0.074 half-widths, without which the bound
 * is missed at the box edge away from the line.  A multiple of 1/2 (box centres sit between two points).  Host arithmetic,
 * the same expression the kernels compile; -1.0: level or margin out of range.  For tests and error models. */
double sr_far_field_min_distance(int level, int pole_margin);
/* sr_retrieval_forward_dev / _step_dev / _loop_dev with up to 8 parameters on a folded batch: 1 (default) the recursion
 * kernel integrates the instrument bands in its epilogue (partial sums per 64 points; the 1 + n_par spectra per ray
 * are never written: `buf` stays untouched); 0: spectra into `buf`, then sr_hires_to_lowres_shard_dev's kernels -- the
 * same numbers up to the summation order (<= 1e-13 relative), kept as the check and the A/B partner. */
int sr_set_band_fusion(int on);
/* Which recursion kernel the most recent sr_limb_rays_dev call on this thread launched: 1 the path-order kernels
 * (sr_limb_kernel / sr_limb_split_kernel), 2 the folded sweep (sr_limb_fold_fwd_kernel: ray batches that share their
 * shells), 0 none yet.  Diagnostic (tests pin the choice: a 3-D batch with a coefficient row per LOS step must not fold). */
int sr_last_limb_route(void);
/* Parameter blocks PER RAY in the mixed-state calls (everything that runs sr_limb_jac_state_kernel:
 * sr_limb_rays_jac_level_dev, sr_limb_rays_jac_state_dev, _jac_state_rows_dev, sr_limb_rays_state_bands_dev and their
 * _gases, _instr and _path forms).  0 (default): the parameter list of the BATCH is cut into blocks of 8 or 16 and every
 * ray is walked once per block, whether or not it touches one of the block's parameters.  1: every ray lists the
 * parameters that touch it -- a column parameter iff par_w[p] is non-zero at one of the ray's sample points, a level or
 * row parameter iff par_c[p][r] / par_t[p][r] is non-zero on the coefficient row r of one of its segments, the hidden
 * pointing slots always -- in the dense plan's order, and cuts its own list into blocks of 8 (no ray is touched by more
 * than 8) or 16; a ray is walked once per block of ITS list, at least once (the radiance).  The rows of parameters that
 * do not touch a ray are exact zeros in both settings (with 1 the output is cleared on the stream ahead of the launch);
 * the other rows and the radiances are the same arithmetic, slot for slot.  Signatures, layouts, limits and refusals
 * are unchanged.  Process-wide, read once at a call's entry, as sr_set_band_fusion.  Latitude-box states (a ray crosses
 * two or three of the boxes) and mixed 1-D states with many altitude nodes are what it is for; opt-in.
 * sr_last_state_route: the plan of the calling thread's most recent such call, 1 dense, 2 per ray, 0 none yet;
 * sr_last_state_walks: its (ray, block) pairs, the number of times a ray was walked.
 * sr_state_ray_plan: the per-ray plan itself on the host, for tests and tools -- no device is touched.  The arguments as
 * the state calls name them (par_lgas NULL: one level gas; n_hid: hidden pointing slots, 0 .. 4, or 0 .. 8 for a
 * batch of more than four gases).  sizes4: np, the
 * largest block count of a ray (gridDim.z), the number of ray blocks n_rb, the number of entries n_ent.  The arrays may
 * each be NULL (a first call for the sizes): ray_blk_off [n_rays + 1], blk [n_rb][2], col_row [n_rb][np],
 * ent_off [n_rb][n_layers + 1], slot_par [n_rb][np], ent_slot / ent_level / ent_c [n_ent].
 * Checked against the extended-precision recursion and the dense plan (tests/test_gpu_state_rayblocks.py).
 * sr_last_state_instance: the census of the state kernel's compiled instances.  out[8] = NG, NP, COLS, ROWS, BANDS, INSTR,
 * SEVERAL, RAYBLK of the instance the calling thread's most recent such call launched: the template's gas count (6 for a
 * five-gas batch, 8 for seven), its slots per block (8 or 16), and 0 / 1 for column slots, row slots, the band epilogue,
 * the instrument rows, several level gases, parameter blocks per ray.  The values are the compile-time constants of the
 * instantiation that was launched, recorded where it is launched, not what the call asked for.  SR_ERR_ARG for a null
 * pointer and before the thread's first launch.  tests/test_gpu_state_instances.py holds every instance to the reference. */
int sr_set_state_ray_blocks(int on);
/* The gases a ray batch may carry, sr_los_desc.n_gas: sr_limb_max_gases(0) = 8 for the entries of the path-order radiance
 * kernels and of the state kernel, sr_limb_max_gases(1) = 4 for the entries of every kernel that keeps four gas slots in
 * its packed records (folded, adjoint, forward-sensitivity, parts, retrieval loop).
 *   8: sr_los_create, sr_los_columns, sr_los_columns_dz, sr_los_set_vmr, sr_limb_rays_dev, sr_limb_rays_los_dev,
 *      sr_state_ray_plan, and every state entry -- sr_limb_rays_jac_level_dev, sr_limb_rays_jac_state_dev,
 *      sr_limb_rays_jac_state_rows_dev, sr_limb_rays_jac_state_gases_dev, sr_limb_rays_state_bands_dev,
 *      sr_limb_rays_state_bands_gases_dev, sr_limb_rays_state_bands_instr_dev, sr_limb_rays_state_bands_instr_gases_dev and
 *      the pointing forms sr_limb_rays_jac_state_path_dev, sr_limb_rays_state_bands_path_dev.  At most four of the eight
 *      gases are level-factored (n_lgas <= 4), any of the eight indices.
 *   4: sr_los_create_par with parameters, sr_limb_rays_jac_los_dev, sr_retrieval_forward_dev, sr_retrieval_step_dev,
 *      sr_retrieval_loop_dev, sr_limb_rays_jac_dev, sr_limb_rays_jac_layer_dev, sr_limb_rays_jacobians_dev,
 *      sr_limb_rays_parts_dev.
 * A batch beyond its entry's limit is refused with SR_ERR_LIMIT before the first copy or launch, outputs untouched.  With
 * more than four gases the radiance calls take the path-order kernels (sr_last_limb_route() reads 1: no folded records
 * are made), and the state plan packs a column slot's gas into three bits, eight slots per block. */
int sr_limb_max_gases(int folded);
int sr_last_state_route(void);
int64_t sr_last_state_walks(void);
int sr_last_state_instance(int32_t out[8]);
int sr_state_ray_plan(const sr_los_desc *los, int n_layers, int n_col, const int32_t *par_gas, const double *par_w, int n_lev,
                      const int32_t *par_lgas, const int32_t *par_level, const double *par_c, int n_row, const double *par_t,
                      int n_hid, int32_t *sizes4, int32_t *ray_blk_off, int32_t *blk, int32_t *col_row, int32_t *ent_off,
                      int32_t *slot_par, int32_t *ent_slot, int32_t *ent_level, double *ent_c);
/* Tuning knob of the exact wings kernel: grid points per lane (4 or 8; default 8). */
int sr_set_points_per_lane(int p);

/* Executed-work accounting for bench.py's roofline (far-field mode only).  sr_set_counting(1): the
 * following sr_abscoeff_layers* calls run the counting instantiations of the three coefficient kernels
 * (same results; one atomic per wave and counter) -- not for timed runs.  sr_last_eval_counts: the
 * counters of the most recent such call on this lineset, counts10[0] (line, box) far-field expansions,
 * [1] region-1 evaluations done point by point, [2] window-end expansions, [3] (point, level)
 * far-field polynomial evaluations, [4] region-2, [5] region-3, [6] region-4 evaluations, [7] (line, side)
 * multipole expansions and [8] (source box, target box, layer) translations of the box-pair far field
 * (sr_set_far_field(2)), [9] 0.  Synchronises. */
int sr_set_counting(int on);
int sr_last_eval_counts(sr_lineset *ls, uint64_t *counts10);

/* Timing hook for bench.py: HIP-event times (ms) of the kernels of the most
 * recent sr_abscoeff_layers* call on this lineset, measured on the stream they
 * were launched on.  ms5[0] sr_prep_kernel.  Far-field mode with overlap (the
 * default): ms5[1] = the whole coefficient op (far field + near wings + near
 * zones, which run partly side by side), rest 0.  Far-field mode without overlap:
 * ms5[1] sr_farfield_kernel, ms5[2] sr_abscoeff_near_wings_kernel, ms5[3]
 * sr_abscoeff_near_zones_kernel.  Exact mode: ms5[1] sr_abscoeff_wings_kernel,
 * ms5[2] sr_abscoeff_cores_kernel.  Unused entries 0.  Synchronises. */
int sr_last_kernel_ms(sr_lineset *ls, float *ms5);
/* 0: the coefficient op records no timing events (seven hipEventRecord fewer per call: a 1/8 spectral shard's step is
 * bound by the host's enqueue time before anything else); sr_last_kernel_ms then returns SR_ERR_ARG.  1 (default). */
int sr_set_timing(int on);
/* sr_set_timing(2): additionally two events around the recursion of sr_retrieval_forward_dev / _step_dev / _loop_dev
 * (record packing + the one-sweep kernel with the bands in its epilogue); sr_los_last_kernel_ms: their HIP-event time for
 * the most recent such call on the handle (SR_ERR_ARG when it was not timed).  Synchronises.  bench.py --config 4. */
int sr_los_last_kernel_ms(sr_los *h, float *ms);

#ifdef __cplusplus
}
#endif
#endif
