// sr_kernels.hpp -- launch interface between the host API and the kernels.
#pragma once
#include <hip/hip_runtime.h>
#include "sr_device.hpp"
#include "sr_limb_plan.hpp"
#include "sr_limb_common.hpp"

namespace sr {

// Device-resident line list (filtered, sorted by window centre).
struct LinesDev {
  const double *freq, *hcf, *a_coeff, *b21, *b12, *e_lower, *g_up, *g_lo, *air_broad, *t_dep;
  const double *evib_up, *evib_lo;
  const int *ic, *lev_up, *lev_lo;
  int n_lines;
  const double *s_ref; // sr_lineset_set_strengths: HITRAN intensities at WeightMode::t_ref (kWeightStrength); else null
  // sr_lineset_set_line_shape: pressure shift of the centre and self-broadening, cm^-1 / atm; each null when unset (the
  // same for every line of a launch: the test is wave-uniform)
  const double *p_shift, *self_broad;
};

// Device-resident layer stack; per-layer scalars are evaluated on the host in
// fp64 with correctly rounded sqrt (80 values) and uploaded.
struct LayersDev {
  const double *temps, *p_atm, *trat, *sqk; // T, P[atm], 296/T, sqrt(2 N_A k T ln2 / MM)
  const double *ltrat;                      // log(296/T): (296/T)^n = exp(n log(296/T)), a third of pow()'s instructions
  const double *pop;                        // [n_layers][n_pop] level populations / Q
  const double *ltrat_b, *sqk_b;            // the same two at the temperatures the region BOUNDARIES are placed at
  const double *temps_b;                    // those temperatures
  int frozen;                               // (sr_lineset_set_bounds_temps), used when frozen != 0
  int linear_w;                             // frozen only: the line weights LINEARISED about temps_b (sr_lineset_set_linear_weights)
  int n_layers, n_pop;
  double sqrt_ln2, sqrt_pi_ln2;
  const double *qrat;                       // kWeightStrength / line strengths: Q(t_ref) / Q(T) [n_layers]
  const double *rvib;                       //   r_L = b(E_L, Tvib_L) / b(E_L, T) [n_layers][n_pop] (vibtemp_to_ratio)
  const double *ps_atm;                     // sr_lineset_set_self_pressure: the gas's own partial pressure [atm] (0 when unset)
};

// What the two output channels ("abs", "emi") of the coefficient kernels accumulate, chosen per call:
// the weights of line i in layer k, from its three G coefficients and its levels' populations.
enum { kWeightFolded = 0, kWeightGabsGsp = 1, kWeightGind = 2, kWeightTracked = 3, kWeightLevelPair = 4, kWeightChannels = 5,
       kWeightStrength = 6 };
struct WeightMode {
  int mode;  // kWeightFolded: abs = pop_lo G_abs - pop_up G_ind, emi = pop_up G_sp (smm:2073-2080)
             // kWeightGabsGsp: abs = [lev_lo == level] G_abs, emi = [lev_up == level] G_sp   (BuildCoeff)
             // kWeightGind:    abs = [lev_up == level] G_ind, emi = 0
             // kWeightTracked: the folded weights restricted to `level` (smm:2083-2087)
             // kWeightLevelPair: abs = [lev_lo == level] G_abs - [lev_up == level] G_ind, emi = [lev_up == level] G_sp:
             //                 the two spectra the combine loop multiplies by pop_level (smm:2078-2080), i.e. the
             //                 tracked weights with unit populations -- the level-factored route (sr_glevel_pairs_dev)
             // kWeightChannels: the multi-channel pass (sr_glevel_pairs_dev / sr_gcoeff_levels_dev): wabs = G_abs, wemi = G_sp,
             //                 FastRec::w3 = -G_ind (level == 0: pair tables) or +G_ind (level == 1: three ctypes apart);
             //                 which spectrum each goes to follows from the line's levels (McChannels)
             // kWeightStrength: abs = s_ab / iso_ab, emi = s_em / iso_ab of the HITRAN intensities (LinesDev::s_ref at
             //                 t_ref; hitran_strength), i.e. the folded weights' meaning with S(T) in place of the G's
  int level;
  double t_ref = 0.0, inv_iso_ab = 0.0; // kWeightStrength only
};

// Direct index into the sorted window-centre list: first[x - x0] = number of lines with
// centre < x, for x in [x0, x0 + n_tab) (x0 = smallest centre, last entry = n_lines), so a
// kernel finds a candidate range with ONE load instead of a 17-step dependent binary search
// (which was most of a far-field box's lifetime).  line_lo / n_sub select the lines whose
// window meets the shard: the kernels' record tables are indexed relative to line_lo.
struct IcIndex {
  const int *first;
  int x0, n_tab, line_lo, n_sub;
};
// What the kernels of a call read of its shard [g_lo, g_hi): the record tables [n_layers][ix.n_sub] of the lines that
// meet it, the centre index and the layers' widest zones (zmax [n_layers], host bound: sr_api.hip, fill_layer_stage)
struct ShardTables {
  const FastRec *fast;
  const ColdRec *cold;
  IcIndex ix;
  const int *zmax;
  int n_layers, g_lo, g_hi;
};

// Far-field (local expansion) hierarchy over one shard: level l has boxes of
// 64 << l points starting at g_lo.
// (kTheta, kFD): the truncation bound is 18 * kTheta^-(kFD+1) of a line's own contribution (what the admissible
// distance has to be for it: ff_thr2 below);
// a smaller kTheta shrinks the exactly evaluated near field, a larger kFD costs far-field
// time and registers.  Config 2, sum of the coefficient kernels (tools/sweep_farfield.sh):
// (8,14) 18.2 ms and (5,19) 17.2 ms with the first far-field kernel; with the streamed
// recurrence (6,17) 13.8, (5,19) 13.4, (4,22) 12.8, (4,24) 13.2, (3,28) 13.2.
// (4, 22): bound 2.6e-13 -- rounds 2-5, and most of round 6.
// The degree follows the ACCURACY BUDGET since the end of round 6: the results must match the reference to 1e-6
// (north_star), the parity tests hold 1e-10 against the oracle; degree 22 bought agreement with the exact mode at fp64
// noise (1.5e-14 measured on the headline workload) with Joules the step does not have -- it is bound by the socket's
// power cap.  Same box, headline / far-field-vs-exact error / level-table build (tools/ab_order.sh,
// profiles/r06_far_field_order.txt): 22: 183.9 spectra/s, 1.6e-14, 12.8 ms; 20: 189.7, 3.2e-13, 12.5; 19: 191.6,
// 1.4e-12, 12.3; 18: 191.2, 6.3e-12, 12.0; 17: 189.7, 2.9e-11, 11.9; 15: 192.8, 5.7e-10, 12.4.
// (4, 19): bound 1.6e-11 of a line's own contribution; -DSR_KFD=22 restores the old one (the tests take their far-field
// tolerances from sr_far_field_truncation_bound()).
#ifndef SR_KTHETA // tools/sweep_farfield.sh builds variants with -DSR_KTHETA= -DSR_KFD= into a separate file
#define SR_KTHETA 4
#endif
#ifndef SR_KFD
#define SR_KFD 19
#endif
constexpr int kTheta = SR_KTHETA; // admissible distance, in box half-widths
constexpr int kFD = SR_KFD;       // expansion degree
constexpr int kFC = kFD + 1;   // coefficients per box and output
constexpr int kMaxFarLevels = 5;
// The admissible distance.  A (line, box) pair of level l (box of W = 64 << l points, half-width h = W / 2) may be
// expanded when the box centre is at least  kTheta h + pm (+ the level's margin)  grid points from the line's centre
// index; ff_thr2 is TWICE that (box centres sit on half points), the one expression every kernel and the host's
// sr_far_field_min_distance share.  pm: the layer's pole margin (sr_api.hip, fill_layer_stage).
// What the bound 18 kTheta^-(kFD+1) asks of it.  Beyond pm the wing is ~ 1/x^2; for a line D points from the box centre,
// t = (j - centre) / h in [-1, 1] and r = h / D:  (D + h t)^-2 = D^-2 sum_n (n + 1) (-r t)^n, and what is left after
// degree d, relative to the line's own value at the point, sum_(n > d) (n + 1) r^n = r^(d+1) (d + 2 - (d + 1) r) / (1 - r)^2, is
//   edge facing the line (t = -1):  (d + 2 - (d + 1) r) r^(d+1)     (4, 19) at r = 1/4: 16 x 4^-20
//   edge away from it   (t = +1):  (d + 2 + (d + 1) r) r^(d+1)                          26 x 4^-20 = 1.44 x the bound
// (the absolute error is larger at the facing edge, the line itself smaller at the far one).  At r = 1/kTheta the
// constant 18 holds for the facing edge only; for both it takes r <= r*, the root of
// (d + 2 + (d + 1) r) (kTheta r)^(d+1) = 18: (4, 19) r* = 0.245488, D >= h / r* = (4 + 0.07352) h; (4, 22) 0.244642,
// (4 + 0.08761) h.  kFarMarginQ10 is that excess over kTheta in 1/1024 of h, rounded up: 76 and 90 (bisection in long
// double at compile time, checked against these two below).
// Levels >= 1 carry the margin.  Level 0 does not: there the "+ 1" of pm and the half-point inset of the outermost
// points (t = +-(1 - 1/64)) are worth more than the margin's 2.4 points -- 1.36e-11 of 1.64e-11 at degree 19, 2.25e-13
// of 2.56e-13 at 22, worst over the panel of tests/test_farfield_reference_host.py -- so the near kernels, which know level 0 only, the box
// pairs ("valid pairs are admissible at level 0") and the default dense path, whose per-line expansions are level 0's,
// stay as they were.  Ownership stays monotone down the hierarchy: a parent admissible at (2 kTheta + 2 m) h puts its
// children at >= (2 kTheta - 1 + 2 m) h >= (kTheta + m) h.
constexpr long double ff_far_edge_over_bound(long double r) {
  long double p = 1.0L;
  for (int n = 0; n <= kFD; ++n) p *= kTheta * r;
  return (kFD + 2 + (kFD + 1) * r) * p / 18.0L;
}
constexpr int ff_margin_q10() {
  long double lo = 0.5L / kTheta, hi = 1.0L / kTheta; // over_bound(lo) < 1 <= over_bound(hi), increasing in r
  for (int i = 0; i < 80; ++i) {
    const long double mid = 0.5L * (lo + hi);
    (ff_far_edge_over_bound(mid) <= 1.0L ? lo : hi) = mid;
  }
  const long double q = 1024.0L * (1.0L / lo - kTheta);
  const int qi = (int)q;
  return qi + (qi < q ? 1 : 0);
}
constexpr int kFarMarginQ10 = ff_margin_q10();
// kTheta = 5 computes wrong results (profiles/r06_far_field_order.txt); the degrees are those whose level 0 was checked
static_assert(kTheta == 4, "the far field is built and checked for kTheta = 4 only");
static_assert((kFD == 19 && kFarMarginQ10 == 76) || (kFD == 22 && kFarMarginQ10 == 90),
              "far-field degree without a checked admissible distance: 19 (default) or 22");
__host__ __device__ constexpr int ff_thr2(int level, int pm) {
  const int W = 64 << level;
  return kTheta * W + 2 * pm + (level > 0 ? (W * kFarMarginQ10 + 1023) / 1024 : 0);
}
#ifndef SR_FAR_SUPER
#define SR_FAR_SUPER 16384
#endif
constexpr int kFarSuper = SR_FAR_SUPER; // points per super-tile of sr_farfield_kernel's block order (a multiple of the widest box)
// Far field by box pairs (sr_set_far_field(2)): the lines of a SOURCE box (64 << l line centres wide, same frame
// as the target boxes) are summed into multipole moments about the box centre (sr_s2m_kernel, sr_m2m_kernel) and
// translated to the local expansion of every target box of the level that is well separated from it
// (sr_m2l_kernel); only the (line, box) pairs no box pair covers keep their own expansion (level 0 of
// sr_farfield_kernel).  Moments: orders q = 2..kFD of the Laurent series at infinity, scaled by the box
// half-width and by 1/(q-1)!, for the two running-x anchors of the reference (right / left wing) and the two
// output weights.
constexpr int kMQ = kFD - 1;         // multipole orders per (side, weight)
constexpr int kMomPerBox = 4 * kMQ;  // [side: 0 right-going, 1 left-going][abs, emi][q - 2]
constexpr int kSrcPad = 112;         // level-0 source boxes left of the shard start: 7168 points >= kHalf, a multiple of the widest box
constexpr int kM2LOffsets = 104;     // |box offset| < this (level 0: (|o| + 1) 64 <= kHalf)
constexpr int kM2LRow = (kFC + 15) / 16 * 16; // columns of the translation operator (kFC, padded with zeros to MFMA tiles)
constexpr int kM2LQ = (kMQ + 3) / 4 * 4;      // rows (kMQ, padded with zeros)
struct FarParams {
  int n_levels, n_layers, n_boxes_total;
  int top_first; // block order of sr_farfield_kernel: widest two levels of a layer group first
  int folded0;   // level 0 holds every level's far field (sr_l2l_kernel ran): one polynomial per point
  int box_count[kMaxFarLevels], box_off[kMaxFarLevels];
  const int *pm; // [n_layers] pole margin in grid points
  double *coef;  // [n_layers][n_boxes_total][2][kFC]
  // box-pair mode (m2l != 0)
  int m2l;
  int rows; // per-line mode (m2l == 0) for a SPARSE line set: sr_farfield_rows_kernel (eight layers of a box per wave)
  int n_src[kMaxFarLevels], src_off[kMaxFarLevels]; // source boxes per level (storage index = box + (kSrcPad >> level))
  // Lines beyond the grid ends have their window on the first / last grid point (closest_grid, spect_classes.py:1941)
  // and their centre up to kHalf points outside it: they are sorted first / last (indices of the shard's line
  // table), take no part in the box moments and keep per-line expansions (level 0) over their whole window.
  int disp_lo_end, disp_hi_begin;
  const int *pm_src; // [n_layers] largest pole radius |sqrt(1/2 + ry^2)| dw' of the layer's lines, in grid points
  double *mom;       // [sum n_src][n_layers][kMomPerBox]
  const double *tab; // [2: o > 0, o < 0][kM2LOffsets][kM2LQ][kM2LRow] translation operator (host, long double)
};
// Executed-work counters of the counting instantiations (sr_set_counting): index into cnt[kCntN].
enum {
  kCntExpansions = 0, // (line, box) far-field expansions          sr_farfield_kernel
  kCntRegion1 = 1,    // region-1 evaluations done point by point  sr_abscoeff_near_wings_kernel
  kCntWindowEnds = 2, // per-line degree-5 window-end expansions   sr_abscoeff_near_wings_kernel
  kCntPolyPoints = 3, // (point, level) far-field polynomial evaluations, two outputs each
  kCntRegion2 = 4,    // region-2 evaluations                      sr_abscoeff_near_zones_kernel
  kCntRegion3 = 5,    // region-3 evaluations
  kCntRegion4 = 6,    // region-4 evaluations
  kCntS2M = 7,        // (line, side) multipole expansions (box-pair mode)  sr_s2m_kernel
  kCntM2L = 8,        // (source box, target box, layer) translations      sr_m2l_kernel
  kCntN = 10
};
// cnt: device counters [kCntN] or nullptr (the timed instantiations: no counting code)
int launch_farfield(const ShardTables &t, const FarParams &fp, unsigned long long *cnt, hipStream_t st);
// box-pair mode: moments of the level-0 source boxes, the wider levels, the translations (after the level-0 pass
// of launch_farfield, which stores; the translations add at level 0 and store above)
// which: bit 0 = moments + upward pass (sr_s2m_kernel, sr_m2m_kernel), bit 1 = translations (sr_m2l_kernel)
int launch_m2l(const ShardTables &t, const FarParams &fp, unsigned long long *cnt, hipStream_t st, int which = 3);
void m2l_table_host(double *tab); // [2][kM2LOffsets][kM2LQ][kM2LRow]
// part 1: wing-only pairs + far-field polynomials (writes); part 2: general pairs (adds)
// z_abs / z_emi (part 1 only): the zones kernel's sums in a buffer of their own; the wings kernel writes z + its sums
int launch_near(int part, int add, const ShardTables &t, const GridParams &gp, const FarParams &fp, double *abs_out,
                double *emi_out, unsigned long long *cnt, hipStream_t st, const double *z_abs = nullptr,
                const double *z_emi = nullptr);

// ---- the multi-channel pass (sr_zones_mc_kernel, sr_wings_mc_kernel) ----
// Which output spectrum ("channel") each of a line's three weights goes to: channel = stride * level + offset.
//   pair tables  (sr_glevel_pairs_dev):  stride 2; wabs -> (lev_lo, 0) abs, wemi -> (lev_up, 1) emi, w3 = -G_ind -> (lev_up, 0) abs
//   three ctypes (sr_gcoeff_levels_dev): stride 3; wemi -> (lev_up, 0) sp_emission, w3 = +G_ind -> (lev_up, 1) ind_emission,
//                                        wabs -> (lev_lo, 2) absorption
struct McChannels {
  int stride, o_lo, o_up_e, o_up_a, n_ch; // n_ch = stride * n_levels
};
// One far-only pass of a level sub-lineset: its coefficients [n_layers][n_boxes_total][2][kFC] (nullptr: no lines) and
// the channels its two outputs belong to (-1: none)
struct McFarPass {
  const double *coef;
  int ch_a, ch_e;
};
#ifndef SR_MC_IMAGE
#define SR_MC_IMAGE 256
#endif
#ifndef SR_MC_WAVES
#define SR_MC_WAVES 8
#endif
#ifndef SR_MC_WING_WAVES
#define SR_MC_WING_WAVES 2
#endif
constexpr int kMcWingWaves = SR_MC_WING_WAVES; // waves sharing a slot's image in sr_wings_mc_kernel
constexpr int kMcImage = SR_MC_IMAGE, kMcWaves = SR_MC_WAVES; // points per LDS image of sr_zones_mc_kernel, waves sharing it
// lev_up / lev_lo: the lineset's arrays offset to the first line of the shard's record table (IcIndex::line_lo)
// out [n_ch][n_rows_total][g_hi - g_lo]; the launch's layers are rows row0 .. row0 + n_layers - 1.  zones stores, wings adds.
// One SPARSE far-only pass of a table build's batch (launch_far_batch): the sub-lineset's lines and centre index, the
// lines whose windows meet the shard, the weights, where its records [n_layers][n_sub] and coefficients go
struct FarBatchItem {
  LinesDev L;
  const int *first;
  int first_x0, first_n, line_lo, n_sub;
  WeightMode W;
  FastRec *fast;
  double *coef;
};
int launch_far_batch(const FarBatchItem *items, int n_items, int max_n_sub, const LayersDev &A, const GridParams &gp, const int *zmax,
                     int g_lo, const FarParams &fp, const double *l2l_tab, hipStream_t st);
// the downward pass: a far pass's wider levels folded into its level-0 coefficients (in place); tab: l2l_table_host
void l2l_table_host(double *tab); // [2][kFC][kFC]
int launch_l2l(double *coef, int n_layers, const FarParams &fp, const double *tab, hipStream_t st);
int zones_mc_image(int n_ch);     // points per image sr_zones_mc_kernel takes for n_ch planes (0: they do not fit the LDS)
size_t wings_mc_lds(int n_ch);    // bytes of LDS of a sr_wings_mc_kernel workgroup
int launch_zones_mc(const ShardTables &t, const int *lev_up, const int *lev_lo, const GridParams &gp, const McChannels &mc,
                    double *out, int n_rows_total, int row0, hipStream_t st);
int launch_wings_mc(const ShardTables &t, const int *lev_up, const int *lev_lo, const FarParams &fp, const McChannels &mc,
                    const McFarPass *far, int n_far, double *out, int n_rows_total, int row0, hipStream_t st);

int launch_prep(const LinesDev &L, const LayersDev &A, const GridParams &gp, const WeightMode &W, int line_lo,
                int n_sub, int cold_lo, int cold_hi, FastRec *fast, ColdRec *cold, hipStream_t st);
// Lines whose centre lies outside their own window (humliv_bb's outer branches, lineshape.f:272-442):
// records per (line, layer), then one thread per (grid point, layer) adds them in line order.
int launch_outer(const LinesDev &Lo, int n_out, const LayersDev &A, const GridParams &gp, const WeightMode &W,
                 OuterRec *recs, int g_lo, int g_hi, double *abs_out, double *emi_out, hipStream_t st);
// Line strengths of every (input line, layer) in input order (sr_line_strengths_dev); inpos: input -> device position
int launch_line_strengths(const LinesDev &L, const LinesDev &Lo, const int *inpos, int n_in, const LayersDev &A,
                          int source, double iso_ab, double t_ref, double *s_ab, double *s_em, hipStream_t st);
int abscoeff_tile_points(int variant);
// which = 0: wings kernel (writes abs/emi), 1: cores kernel (adds into them)
int launch_abscoeff(int variant, int which, const ShardTables &t, const GridParams &gp, double *abs_out, double *emi_out,
                    hipStream_t st);
// prof[g] = sum_p x_p prof[n_gas + p] over the parameters of gas g (gases without parameters untouched)
// x_host: HOST [n_par] (passed as kernel arguments, kVmrParArg per launch)
constexpr int kVmrParArg = 32;
int launch_los_vmr_from_params(double *prof, int n_gas, int n_par, int n_pt, const int *par_gas, const double *x_host, hipStream_t st);
int launch_los_columns(const double *nd, const double *x, const double *prof, const double *scale, const int *pt_off,
                       int n_seg, int n_pt, int n_prof, double *col, hipStream_t st);
// d col / d z_t of the gases (rows [n_gas][n_seg] at dcol) from the path derivatives of the sample points
int launch_los_columns_dz(const double *nd, const double *x, const double *prof, const double *scale, const int *pt_off,
                          const double *alt, const double *dx_dz, const double *dalt_dz, int n_seg, int n_pt, int n_gas,
                          double *dcol, hipStream_t st);
// row n_state of jac [n_rays][n_state + n_hid][n_pts] += the rows behind it
int launch_jac_rows_sum(double *jac, int n_rays, int n_state, int n_hid, int n_pts, hipStream_t st);
int launch_limb(const double *abs_c, const double *emi_c, int n_pts, int n_layers, int n_rays, const int *seg_off,
                const int *seg_layer, const double *col, const LimbOpts &o, double *rad, hipStream_t st);
// ... its instances of five to eight gases (sr_limb_many.hip), which launch_limb hands such a batch to
int launch_limb_many(const double *abs_c, const double *emi_c, int n_pts, int n_layers, int n_rays, const int *seg_off,
                     const int *seg_layer, const double *col, const LimbOpts &o, double *rad, hipStream_t st);
int launch_limb_jac(const double *abs_c, const double *emi_c, int n_pts, int n_layers, int n_rays, const int *seg_off,
                    const int *seg_layer, const double *col, const double *dcol, const int *par_gas, int n_par,
                    const LimbOpts &o, double *rad, double *jac, hipStream_t st);
// the forward-sensitivity kernel (16 layers per thread when there are more than 8; `forward` is ignored: the one-pass
// formulation is launch_limb_adjoint)
int launch_limb_jac_layer(const double *abs_c, const double *emi_c, const double *dabs, const double *demi, int n_pts,
                          int n_layers, int n_rays, const int *seg_off, const int *seg_layer, const double *col,
                          const LimbOpts &o, double *jac, hipStream_t st);
// Level-parameter and mixed-state Jacobians (sr_limb_jac_state_kernel): one launcher over one record, StateLaunch below
// (LevelEnt, an entry of its plan, and LevelGasTabs: sr_limb_plan.hpp).
struct StateLaunch {
  // The batch, as launch_limb_jac takes it.  dcol: the rows of the column parameters, caller's order (not read, and may
  // be null, without column slots).
  const double *abs_c, *emi_c;
  int n_pts, n_layers, n_rays;
  const int *seg_off, *seg_layer;
  const double *col, *dcol;
  LimbOpts o;
  // The level tables.  One level-factored gas (lgas null): gas `gas` of the batch, pair tables tab with n_tab_rows rows,
  // coef_row [n_layers].  SEVERAL (lgas given, batches of two to four gases; the kernel's instances whose parameter
  // pack ends in a LevelGasTabs): level gas k has the tables lgas->tab[k] with lgas->n_tab_rows[k] rows, is gas
  // lgas->gas[k] of the batch, and coef_row [n_lgas][n_layers] holds its row map at k n_layers; the level slots are
  // sorted by (level gas, level) and an entry's `level` is level | level gas << kLevelEntGasShift; gas, tab and
  // n_tab_rows are not read.
  int gas;
  const double *tab;
  int n_tab_rows;
  const LevelGasTabs *lgas;
  const int *coef_row;
  // The plan of n_par = n_col + n_lev + n_row parameters: the column parameters first (rows of dcol), then the level
  // parameters in level order, then the row parameters in the caller's order, in blocks of level_jac_np(n_par).
  // blk [n_blocks][2] = the number of column slots of a block (its first slots: parameters block NP + q) and their
  // gases, two bits per slot; ent_off [n_blocks][n_layers + 1] into ent, the entries of every (parameter block,
  // coefficient row) with a non-zero coefficient, in level order, slot numbers counted over all slots of a block;
  // slot_par [n_blocks][NP] = the parameter an accumulator belongs to, or -1.  blk == nullptr: no column parameters
  // (n_col = 0), the kernel instances without column code.
  int n_blocks;
  const int *blk, *ent_off;
  const LevelEnt *ent;
  const int *slot_par;
  int n_par;
  // ROW parameters (the kernel's ROWS = true instances; both null: none).  dabs / demi [n_gas][n_layers][n_pts]: the
  // derivative spectra a row parameter acts through.  A row slot has, on every coefficient row it weights, one entry
  // behind that row's level entries: level = kLevelEntRows, c = the weight.
  const double *dabs, *demi;
  // The output.  Spectra (lowres_scratch null): rad [n_rays][n_pts] (may be null), jac [n_rays][n_par][n_pts].
  // Or the instrument bands in the epilogue (the kernel's BANDS = true instances): no spectra are written; the band
  // integrals' partial sums per wave (64 points) go to lowres_scratch, the instrument step's scratch, whose weight table
  // is in place (launch_lowres_weights; scratch sized for n_rays (1 + n_par) rows, fused), rows as launch_fold_dense
  // orders them: row ray = the radiance, row n_rays + ray n_par + p = parameter p.  launch_lowres_sum_blocks finishes them.
  // instr (bands only): the kernel's INSTR = true instances -- the scratch of an instr call, three weight tables; every
  // ray has two more parameter rows in `part`, n_par and n_par + 1 of n_par + 2: the radiance's bands d / d centre and
  // d / d ln width; n_par, here the number of state parameters, may then be 0, with one block whose slots are all unused.
  double *rad, *jac;
  const void *lowres_scratch;
  int n_bands;
  bool instr;
  // Parameter blocks PER RAY (ray_jac_plan; the kernel's instances whose pack ends in a StateRayBlocks), ray_blk_off
  // given: blk, ent_off and slot_par are then indexed by ray_blk_off[ray] + block, n_blocks is the largest block count
  // of a ray, col_row [ray blocks][np] the dcol row of every column slot, np (8 or 16) the plan's slots per block.  The
  // launcher clears the parameter rows of jac, or of the partial sums, on the stream first: a ray's blocks write the
  // rows of its own parameters only.  ray_blk_off null (the default): the dense plan, as above.
  const int *ray_blk_off, *col_row;
  int np;
};
int launch_limb_jac_state(const StateLaunch &L, hipStream_t st);
// The census of the state kernel's instances: the compile-time parameters of the instance the calling thread launched
// last, written by launch_state_instances (sr_limb_state_launch.inc) in whichever unit launched it, from the constexpr
// values of that instantiation -- never from the request.  One record, defined in sr_api.hip beside the last state
// route; ng == 0: no launch yet.  Read by sr_last_state_instance.
struct StateInstance {
  int ng, np;
  bool cols, rows, bands, instr, several, rayblk;
};
extern thread_local StateInstance g_last_state_instance;
// The state units behind it, one translation unit each (sr_limb_state_unit.hpp): the kernel's instances for a pair of gas
// counts and 8 or 16 slots per block, and those of five to eight gases (sr_limb_many.hip, 8 slots).  From the prelude of
// launch_limb_jac_state -- the checks made, bd the band scratch's layout, n_row_par the parameter rows of a ray in
// `part`, the rows of a launch with blocks per ray cleared; a gas count that is not the unit's is hipErrorInvalidValue.
int launch_limb_jac_state_12_np8(const StateLaunch &L, const FoldBands &bd, int n_row_par, hipStream_t st);
int launch_limb_jac_state_12_np16(const StateLaunch &L, const FoldBands &bd, int n_row_par, hipStream_t st);
int launch_limb_jac_state_34_np8(const StateLaunch &L, const FoldBands &bd, int n_row_par, hipStream_t st);
int launch_limb_jac_state_34_np16(const StateLaunch &L, const FoldBands &bd, int n_row_par, hipStream_t st);
int launch_limb_jac_state_many(const StateLaunch &L, const FoldBands &bd, int n_row_par, hipStream_t st);
// Radiance budget (sr_limb_parts_kernel): the n_part parts and the background are n_part + 1 slots in blocks of
// limb_parts_np(n_part); slot_level [n_blocks][NP]: >= 0 the first row of a level's E plane in the pair tables,
// (2 L + 1) n_tab_rows, -1 - g the gas part of gas g,
// kPartNoSource no source (background, unused slot); slot_part [n_blocks][NP]: the row of `parts` a slot is written to
// (n_part: the background, which starts at the initial intensity) or -1; words [n_blocks][n_layers]: bit q = slot q
// has a source on the row, bit 16 + q = its table value is loaded (not passed on from slot q - 1);
// cc [n_blocks][n_layers][NP]: the coefficients of the level parts (a gas part: its gas index as an int64).
constexpr int kPartNoSource = -2147483647 - 1;
inline int limb_parts_np(int n_part) { return n_part + 1 > kLevelJacNPSmall ? kLevelJacNPLarge : kLevelJacNPSmall; }
int launch_limb_parts(const double *abs_c, const double *emi_c, int n_pts, int n_layers, int n_rays, const int *seg_off,
                      const int *seg_layer, const double *col, const LimbOpts &o, int gas, const double *tab,
                      const int *coef_row, int n_blocks, const unsigned *words, const double *cc, const int *slot_level,
                      const int *slot_part, int n_part, double *rad, double *parts, hipStream_t st);
// One pass per ray for radiances, per-layer and column-parameter Jacobians (sr_limb_adjoint_kernel)
struct SegProg;
// plan [n_seg][kAdjPlanInts] (sr_limb_plan.hpp: build_adj_plan)
int launch_adj_pack(const int *plan, const double *col, int n_gas, int n_seg, SegProg *out, hipStream_t st);
size_t adj_prog_bytes(int n_seg);
int launch_limb_adjoint(const double *abs_c, const double *emi_c, const double *dabs, const double *demi, int n_pts,
                        int n_layers, int n_jrows, int n_rays, const int *seg_off, const SegProg *prog, const int *zero_off,
                        const int *zero_row, int n_par, const LimbOpts &o, double *rad, double *jac_layer,
                        double *jac_par, hipStream_t st);
// The layer-synchronous variant (sched [n_batches][n_visits][1 + kAdjSyncRays]: sr_limb_plan.hpp, build_sync_schedule)
int launch_limb_adjoint_sync(const double *abs_c, const double *emi_c, const double *dabs, const double *demi, int n_pts,
                             int n_layers, int n_jrows, int n_rays, const SegProg *prog, const int *zero_off,
                             const int *zero_row, int n_par, const LimbOpts &o, const int *sched, int n_visits, double *rad,
                             double *jac_layer, double *jac_par, hipStream_t st);
// The folded variant (sr_limb_adjoint_fold_kernel): both segments of a ray in a shell together, every Jacobian value
// stored once; one ray per thread.  plan [n_rays][n_visits][kFoldPlanInts]
struct FoldRec;
size_t fold_rec_bytes(int n_rec);
int launch_fold_pack(const int *plan, const double *col, int n_gas, int n_seg, int n_rec, FoldRec *out, hipStream_t st);
// two_rows: the two segments of a shell read different coefficient rows (3-D paths)
int launch_limb_adjoint_fold(const double *abs_c, const double *emi_c, const double *dabs, const double *demi, int n_pts,
                             int n_layers, int n_jrows, int two_rows, int n_rays, const FoldRec *rec, const int *zero_off,
                             const int *zero_row, int n_par, const LimbOpts &o, int n_visits, double *rad, double *jac_layer,
                             double *jac_par, hipStream_t st);
// The folded recursion for up to kFoldDensePar column parameters whose masks may cover the whole path (one sweep, three
// accumulators per parameter): sr_limb_fold_sens_lds_kernel.  plan [n_rays][n_visits][4] = layer, far segment, near segment, 0
constexpr int kFoldDensePar = 8;
struct FoldDense;
size_t fold_dense_bytes(int n_rec);
int launch_fold_dense(const int *plan, const double *col, const int *par_gas_host, int n_par, int n_seg, int n_rec, FoldDense *rec,
                      const double *abs_c, const double *emi_c, int n_pts, int n_layers, int n_rays, int n_visits,
                      const LimbOpts &o, double *rad, double *jac_par, hipStream_t st, const void *lowres_scratch = nullptr,
                      int n_bands = 0);
// (lowres_scratch: the instrument step's scratch with its weight table in place (launch_lowres_weights) -- the kernel then
// leaves the band integrals' partial sums per wave (64 points) there instead of the spectra in rad / jac_par:
// launch_lowres_sum_blocks finishes them)
// The radiances of a ray batch, folded (sr_limb_fold_fwd_kernel; the plan and records of launch_fold_dense with no parameters)
// pack = false: `rec` was packed by an earlier call with the same plan and columns (a device-resident LOS, sr_los_create)
int launch_fold_fwd(const int *plan, const double *col, int n_seg, int n_rec, FoldDense *rec, const double *abs_c,
                    const double *emi_c, int n_pts, int n_layers, int n_rays, int n_visits, const LimbOpts &o, double *rad,
                    hipStream_t st, bool pack = true);
// the grid of the kernels that deal their blocks by limb_block(): the point blocks rounded up to the eight XCDs
inline unsigned limb_grid(int n_pb, int n_rays) { return (unsigned)(((n_pb + 7) / 8) * 8) * (unsigned)n_rays; }
// launch_limb takes the latency-bound split kernel below this many waves
inline bool limb_launch_is_small(int n_pts, int n_rays) { return (long)((n_pts + 63) / 64) * n_rays < 2048; }
int launch_radiance(const double *abs_c, const double *emi_c, int n_pts, int n_rays, const int *seg_off,
                    const int *seg_layer, const double *seg_col, int init_from_rad, double *rad,
                    hipStream_t st);
int launch_radiance_jac_layer(const double *abs_c, const double *emi_c, const double *dabs, const double *demi,
                              int n_pts, int n_layers, int n_rays, const int *seg_off, const int *seg_layer,
                              const double *seg_col, double *jac, hipStream_t st);
int launch_radiance_jac(const double *abs_c, const double *emi_c, int n_pts, int n_rays, const int *seg_off,
                        const int *seg_layer, const double *seg_col, const double *dcol, int n_par, double *rad,
                        double *jac, hipStream_t st);
// outer != 0: x0 at or beyond an end of x(i1..i2) (the sequential branches of humliv_bb)
int launch_humliv(const double *x, int i1, int i2, double x0, double lw, double dwp, double *y, int outer,
                  hipStream_t st);
int launch_sum_lines(double *spe, long n_spe, const double *rows, const int *init, const int *fin,
                     int n_lines, int row_len, hipStream_t st);
// scratch: lowres_scratch_bytes(...) of device memory (the bands' weight table and point ranges, then the chunks' partial
// sums).  weights = false: the table and ranges at the head of `scratch` are those of an earlier call with the same
// grid window and bands (a retrieval's instrument step: every iteration the same bands)
// instr: the scratch carries the weight tables of the two instrument derivatives behind the weights (three tables in all)
size_t lowres_scratch_bytes(int n_pts, int n_bands, int n_rays, bool fused = false, bool instr = false);
// the scratch's layout: the bands' weight table and point ranges, then the partial sums (the band integrals of sr_ops.hip
// and the limb launchers with a band epilogue, sr_limb.hip)
// instr (the instrument derivatives, see sr_lowres_weights_kernel): THREE tables one behind the other in W and in Wt -- the
// weights, then those of d / d centre and of d / d ln width ([3][n_bands][n_pts]; Wt: band tile `tile` of table k is tile
// k n_tiles + tile) -- and nothing else moves; without it the layout is what it always was.
struct LowresScratch {
  double *W;   // [n_bands][n_pts]
  int *range;  // [n_bands][2]
  double *Wt;  // [band tiles][n_pts][16]: the same weights, band-minor in tiles of 16 (zero columns beyond n_bands)
  double *part;
};
inline LowresScratch lowres_layout(void *scratch, int n_pts, int n_bands, bool instr = false) {
  const size_t n_tab = instr ? kLowresTables : 1;
  LowresScratch L;
  L.W = static_cast<double *>(scratch);
  L.range = reinterpret_cast<int *>(L.W + n_tab * n_bands * n_pts); // (before the partial sums: their size follows n_rays)
  L.Wt = reinterpret_cast<double *>(L.range + 2 * (size_t)n_bands + 2);
  L.part = L.Wt + n_tab * ((n_bands + 15) / 16) * 16 * n_pts;
  return L;
}
int launch_lowres_weights(int n_pts, int g_lo, double w0, double gstep, const double *cen, const double *wid, int n_bands,
                          double n_sigma, void *scratch, hipStream_t st, bool instr = false);
// launch_lowres_weights for a tabulated line shape (sr_lowres_weights_tab_kernel): tab, device [n_shapes][n_tab][2], the
// knots with their slopes per knot interval at the reduced offsets t_lo .. t_hi; n_shapes 1 or n_bands
int launch_lowres_weights_tab(int n_pts, int g_lo, double w0, double gstep, const double *cen, const double *wid, int n_bands,
                              const double *tab, int n_shapes, int n_tab, double t_lo, double t_hi, void *scratch, hipStream_t st,
                              bool instr = false);
int launch_lowres_sum_blocks(int n_pts, int n_rows, int n_bands, int out_units, double *out, void *scratch, hipStream_t st,
                             bool instr = false);
int launch_lowres_instr(const double *rad, int n_pts, int n_rays, int n_bands, int out_units, double *out, void *scratch,
                        hipStream_t st);
int launch_lowres(const double *rad, int n_pts, int g_lo, int n_rays, double w0, double gstep, const double *cen,
                  const double *wid, int n_bands, double n_sigma, int out_units, double *out, void *scratch, hipStream_t st,
                  bool weights = true);
int launch_lut(int combine, const double *tab, int n_pt, int n_pts, int n_steps, const int *idx, const double *wgt,
               const double *pop, double *out_a, double *out_e, hipStream_t st);
// Level-factored combine (sr_glevel_combine_dev): rows_used [n_used] table rows that have steps, row_off [n_used + 1]
// into step_of [n_steps] (the steps of each used row), pop / dpop [n_steps][n_levels] in the caller's step order.
int launch_glevel_combine(const double *tab, const double *tab_dT, int n_levels, int n_rows, int n_pts, int n_used,
                          const int *rows_used, const int *row_off, const int *step_of, const double *pop,
                          const double *dpop, double inv_dT, double *abs_out, double *emi_out, double *dabs_out,
                          double *demi_out, hipStream_t st);
int launch_curgod(int which, const double *nd, const double *vmr, const double *f, const double *x,
                  const int *off, int n_seg, double *res, hipStream_t st);
// A tabulated absorber on coefficient rows (sr_abs_table_layers_dev, sr_absorber_table.inc).  One launch serves rows
// row0 .. row1 - 1, which together use n_used <= kAbsTabMaxSets sets: set_v0 / set_dv / set_off / set_n [n_used] describe
// them (axis, offset into values, length), slot2 [n_rows][2] numbers a row's two sets inside this list.  temps, scale,
// slot2, w2, dw2 are device arrays indexed by the row; dw2, dabs_out, demi_out may be null (no derivative).
constexpr int kAbsTabMaxSets = 16;
int launch_absorber_table(int n_used, const double *set_v0, const double *set_dv, const long long *set_off, const int *set_n,
                          const double *values, int row0, int row1, const double *temps, const double *scale, const int *slot2,
                          const double *w2, const double *dw2, double w0, double gstep, int g_lo, int n_pts, bool source,
                          bool accumulate, double *abs_out, double *emi_out, double *dabs_out, double *demi_out, hipStream_t st);
// The single-scattering solar source of coefficient rows (sr_solar_source_rows_dev; sr_solar_source.hip, a unit of its
// own).  tab_abs [n_k][n_pts], u [n_rows][n_k], w / src_row [n_rows], tile_off / chunks: solar_chunk_lists
// (sr_solar_plan.hpp), sca_abs [n_src][n_pts], sun [n_pts]: device arrays; trans_out may be null.
int launch_solar_source(const double *tab_abs, int n_k, int n_pts, const double *u, const double *w, const int *src_row,
                        int n_rows, const int *tile_off, const int *chunks, const double *sca_abs, const double *sun,
                        bool accumulate, double *emi_out, double *trans_out, hipStream_t st);
// the solar attenuation in the Jacobians (sr_solar_jac.inc); the grid is limb_grid(point blocks, n_par x ray groups)
int launch_solar_jac(const double *tab_abs, int n_k, int n_pts, const double *du, int n_par, int n_rows, const int *tile_off,
                     const int *chunks, const double *q, int n_rays, const int *par_slot, bool accumulate, double *jac,
                     int n_jac_rows, hipStream_t st);
// the two-stream diffuse field (sr_diffuse_source.inc) on the points [p_lo, p_hi) of the grid: v [n_gas][n_layers], coef
// [3][kDiffuseGases] (ssa (1 - f), 1 - ssa, ssa (asym - f); zeros beyond n_gas) and temps [n_layers] staged device arrays,
// beam [n_layers + 1][n_pts], ws [4][n_layers][ws_stride] with ws_stride >= the points rounded up to 256; emi_out (with
// out_gas, whose weights are coef's), j_out and flux_out may each be null.  temps null: the sun alone (t_surface, the grid
// and own are not read); else the surface's temperature (0: none), the grid (w0, step, g_lo: point j has nu = w0 +
// (g_lo + j) step), own: the scatterer's complete thermal row, and beam and sun both null: the night instance.  temps and
// beam both null is refused.
int launch_diffuse_field(const double *tab_abs, int n_gas, int n_layers, int n_pts, int p_lo, int p_hi, const double *v,
                         const double *coef, const double *temps, const double *beam, const double *sun, double mu0,
                         double albedo, double t_surface, double w0, double step, int g_lo, bool own, int out_gas, double *ws,
                         int ws_stride, bool accumulate, double *emi_out, double *j_out, double *flux_out, hipStream_t st);
// the diffuse rows in the Jacobians (sr_diffuse_jac.inc) on the points [p_lo, p_hi) and the parameters [par_lo, par_hi):
// dv [n_par][n_gas][n_layers], mask [n_par][2] (diffuse_jac_masks, sr_solar_plan.hpp), v and coef as above: staged device
// arrays; dlnbeam [n_par][n_layers + 1][n_pts] or null; ws [tiles][3 + 4 kDiffuseJacPars][n_layers][ws_stride], tiles =
// ceil((par_hi - par_lo) / kDiffuseJacPars), ws_stride >= the points rounded up to 256; dJ of (p, l, j) goes to
// dj[((p - dj_par0) n_layers + l) dj_stride + j - dj_joff].  The contraction reads it from there and q [n_rays][n_layers]
// [n_pts] and writes jac[ray][par_slot[p]][j]; its grid is limb_grid(point blocks, parameter tiles x ray tiles).
int launch_diffuse_tangent(const double *tab_abs, int n_gas, int n_layers, int n_pts, int p_lo, int p_hi, int par_lo, int par_hi,
                           const double *v, const double *dv, const double *coef, const int *mask, const double *beam,
                           const double *sun, const double *dlnbeam, double mu0, double albedo, double *ws, int ws_stride,
                           double *dj, int dj_stride, int dj_joff, int dj_par0, hipStream_t st);
// the same along a direction in the optics: dopt [n_par][kDiffuseOpt] in dv's place, it and mask from diffuse_optics_plan
// (sr_solar_plan.hpp); workspace and dJ as above, the contraction is launch_diffuse_contract
int launch_diffuse_optics_tangent(const double *tab_abs, int n_gas, int n_layers, int n_pts, int p_lo, int p_hi, int par_lo,
                                  int par_hi, const double *v, const double *dopt, const double *coef, const int *mask,
                                  const double *beam, const double *sun, const double *dlnbeam, double mu0, double albedo,
                                  double *ws, int ws_stride, double *dj, int dj_stride, int dj_joff, int dj_par0, hipStream_t st);
int launch_diffuse_contract(const double *q, int n_rays, int n_layers, int n_pts, int p_lo, int p_hi, int par_lo, int par_hi,
                            const double *dj, int dj_stride, int dj_joff, int dj_par0, const int *par_slot, bool accumulate,
                            double *jac, int n_jac_rows, hipStream_t st);
// the two-stream diffuse source for n_col <= kDiffuseColumns columns of illumination and the rows of LOS steps
// (sr_diffuse_columns.inc) on the points [p_lo, p_hi): v and coef as above, beam [n_col][n_layers + 1][n_pts]; mu0 [NC],
// col_w [n_rows][NC], row_off [n_layers + 1] and row_ix from diffuse_columns_plan (sr_solar_plan.hpp), NC =
// diffuse_columns_instance(n_col), and src_row [n_rows]: staged device arrays; ws [2 + 2 NC][n_layers][ws_stride],
// ws_stride >= the points rounded up to 256; emi_out [n_rows][n_pts] (null: row_off all zero), j_out [n_col][n_layers]
// [n_pts] and flux_out [n_col][2][n_layers + 1][n_pts] may each be null.
int launch_diffuse_columns(const double *tab_abs, int n_gas, int n_layers, int n_pts, int p_lo, int p_hi, const double *v,
                           const double *coef, const double *beam, int n_col, const double *sun, const double *mu0, double albedo,
                           double w_out, const int *row_off, const int *row_ix, const int *src_row, const double *col_w,
                           const double *sca_abs, double *ws, int ws_stride, bool accumulate, double *emi_out, double *j_out,
                           double *flux_out, hipStream_t st);

} // namespace sr
