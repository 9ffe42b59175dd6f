// sr_limb_plan.hpp -- the host plans of the limb kernels: record layouts, checks of a ray batch and the planners.
// Plain C++17, no HIP: the library's host path (sr_api.hip) and the CPU harnesses under tools/ compile the same text.
// Nothing here touches the error string, a stream or device memory.
#pragma once
#include <algorithm>
#include <climits>
#include <cstddef>
#include <cstdint>
#include <numeric>
#include <utility>
#include <vector>

#include "../../include/spectrobot_hip.h"

namespace sr {

// ---- record layouts the host plans and the kernels share ----

// One pass per ray for radiances, per-layer and column-parameter Jacobians (sr_limb_adjoint_kernel and its variants)
constexpr int kAdjEnt = 4;   // column parameters a segment may touch (more: the forward-sensitivity kernel is used)
constexpr int kAdjSlots = 4; // registers a ray's runs of consecutive touches are carried in (ent_gf's slot field; the kernels' slot[4])
constexpr int kAdjPlanInts = 4 + 2 * kAdjEnt;  // ints per segment of the host plan: layer, flags, n_ent, jrow, ent_p[kAdjEnt], ent_gf[kAdjEnt]
constexpr int kFoldPlanInts = kAdjPlanInts + 2; // layer, far segment, near segment, n_ent, ent_p[kAdjEnt], ent_gf[kAdjEnt], layer_n, jrow
// The layer-synchronous variant for rays that share their coefficient rows (1-D atmospheres): kAdjSyncRays rays per
// thread, sched [n_batches][n_visits][1 + kAdjSyncRays] = layer, segment of each ray in that shell on that side (or -1)
#ifndef SR_ADJ_SYNC_RAYS
#define SR_ADJ_SYNC_RAYS 2 // rays per thread: 2: 1.98 ms per configs[3] set, 4: 2.14-2.19, 8: 3.69; one ray per thread (mode 2): 2.05-2.16 (tools/adjoint_probe.py)
#endif
constexpr int kAdjSyncRays = SR_ADJ_SYNC_RAYS;

// Level-parameter and mixed-state Jacobians (sr_limb_jac_state_kernel): LevelEnt, an entry of its plan.
struct __attribute__((aligned(16))) LevelEnt {
  int slot, level; // accumulator of the block, level of the pair tables
  double c;        // d pop[row][level] / d x_p
};
// the `level` of an entry that belongs to a row slot (StateLaunch::dabs / demi): its c is the slot's weight on the row
constexpr int kLevelEntRows = -2;
// several level-factored gases (StateLaunch::lgas): an entry's `level` is level | level gas << kLevelEntGasShift, and the
// kernel's last argument holds, per level gas, the tables, their row count and the gas's index in the batch
constexpr int kLevelEntGasShift = 16, kLevelEntLevelMask = (1 << kLevelEntGasShift) - 1;
constexpr int kLevelGasMax = 4;
// Gases of a ray batch.  kLimbGasMax: what the path-order radiance kernels and the state kernel take (check_los of their
// entries); kFoldGasMax: every kernel with four gas slots in its packed records or registers (the folded, adjoint,
// forward-sensitivity, parts and retrieval-loop kernels).  At most kLevelGasMax of a batch's gases are level-factored.
constexpr int kLimbGasMax = 8, kFoldGasMax = 4;
struct LevelGasTabs {
  const double *tab[kLevelGasMax];
  int n_tab_rows[kLevelGasMax];
  int gas[kLevelGasMax];
};
constexpr int kLevelJacNPSmall = 8, kLevelJacNPLarge = 16;
// The state plan's gas word (blk[2 b + 1]) holds the gas of every column slot of a block: two bits per slot for a batch
// of at most four gases (16 slots), three for a batch of five to eight -- 24 bits of the int, so such a batch has blocks
// of kLevelJacNPSmall slots whatever its parameter count.
inline int state_gas_bits(int n_gas) { return n_gas > kFoldGasMax ? 3 : 2; }
inline int level_jac_np(int n_par, int gas_bits = 2) {
  return gas_bits == 2 && n_par > kLevelJacNPSmall ? kLevelJacNPLarge : kLevelJacNPSmall;
}

// ---- checks of a call's arguments ----

// coef_row [n_layers] of the level-table calls: rows of tables with n_tab_rows rows
inline bool coef_rows_in_range(const int32_t *coef_row, int n_layers, int n_tab_rows) {
  for (int r = 0; r < n_layers; ++r)
    if (coef_row[r] < 0 || coef_row[r] >= n_tab_rows) return false; // would read out of the tables
  return true;
}

// 0 .. n-1 in level order (stable; a level below 0 counts as -1 and comes first): cut into blocks of NP, a block then
// touches few levels and the entries of one level are neighbours
inline std::vector<int> order_by_level(int n, const int32_t *level) {
  std::vector<int> order(n);
  std::iota(order.begin(), order.end(), 0);
  std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return std::max(level[a], -1) < std::max(level[b], -1); });
  return order;
}

struct LosShape {
  int n_seg = 0, n_pt = 0;
};

// gas_max: the gases the calling entry's kernels take, kLimbGasMax or kFoldGasMax
inline int check_los(const sr_los_desc *los, int n_layers, LosShape *out, int gas_max = kFoldGasMax) {
  if (!los || los->n_rays <= 0 || los->n_gas <= 0 || !los->seg_off || !los->x || !los->nd || !los->vmr) return SR_ERR_ARG;
  if (los->n_gas > gas_max) return SR_ERR_LIMIT;
  if (los->init_mode < 0 || los->init_mode > 2) return SR_ERR_ARG;
  if (los->init_mode == 2 && !(los->t_init > 0.0 && los->step > 0.0)) return SR_ERR_ARG;
  const int n_seg = los->seg_off[los->n_rays];
  if (los->seg_off[0] != 0 || n_seg <= 0 || !los->seg_layer || !los->pt_off) return SR_ERR_ARG;
  for (int r = 0; r < los->n_rays; ++r)
    if (los->seg_off[r + 1] < los->seg_off[r]) return SR_ERR_ARG;
  if (los->pt_off[0] != 0) return SR_ERR_ARG;
  for (int s = 0; s < n_seg; ++s) {
    if (n_layers > 0 && (los->seg_layer[s] < 0 || los->seg_layer[s] >= n_layers)) return SR_ERR_ARG; // out-of-bounds read
    const int np = los->pt_off[s + 1] - los->pt_off[s];
    if (np < 2) return SR_ERR_ARG;
    if (np > 8000) return SR_ERR_LIMIT; // imxstp, parameters.inc:64
  }
  out->n_seg = n_seg;
  out->n_pt = los->pt_off[n_seg];
  return SR_OK;
}

// check_los + the column parameters staged with the batch
inline int check_los_par(const sr_los_desc *los, int n_layers, int n_par, const int32_t *par_gas, const double *par_w, LosShape *out,
                         int gas_max = kFoldGasMax) {
  const int rc = check_los(los, n_layers, out, gas_max);
  if (rc) return rc;
  if (n_par < 0 || (n_par > 0 && (!par_gas || !par_w))) return SR_ERR_ARG;
  for (int p = 0; p < n_par; ++p)
    if (par_gas[p] < 0 || par_gas[p] >= los->n_gas) return SR_ERR_ARG;
  return SR_OK;
}

// ---- the shells of a ray batch ----

// The two sides of rays that walk the shells strictly inwards down to a turning shell and strictly outwards again (limb
// rays; slant / nadir rays are the outward half, their first segment counted as the inward one): far / near
// [n_rays][n_layers] = the segment's index in WALK order (LOS_order 'observer' reverses every ray, as stage_los lists the
// columns) or -1, and the range of shells touched.  false: some ray is not of that shape.
// row_of_seg (caller's segment order, or NULL: seg_layer): the SHELL of a segment where that is not its coefficient row
// (3-D paths: seg_jac_row).
inline bool fold_sides(const sr_los_desc *los, int n_layers, const int32_t *row_of_seg, std::vector<int> *far_out,
                       std::vector<int> *near_out, int *l_min_out, int *l_max_out) {
  const int nr = los->n_rays;
  std::vector<int> &far = *far_out, &near = *near_out;
  far.assign((size_t)nr * n_layers, -1);
  near.assign((size_t)nr * n_layers, -1);
  int l_min = n_layers, l_max = -1;
  bool ok = true;
  for (int r = 0; r < nr && ok; ++r) {
    const int a = los->seg_off[r], m = los->seg_off[r + 1] - a;
    auto lay = [&](int q) { return (row_of_seg ? row_of_seg : los->seg_layer)[los->los_order == 0 ? a + q : a + (m - 1 - q)]; };
    int q = 0, prev = INT_MAX;
    for (; q < m; ++q) { // far side: strictly inwards
      const int k = lay(q);
      if (k >= prev) break;
      far[(size_t)r * n_layers + k] = a + q;
      prev = k;
      l_min = std::min(l_min, k); l_max = std::max(l_max, k);
    }
    prev = q < m ? lay(q) - 1 : prev;
    if (q < m && q > 0 && lay(q) < lay(q - 1)) ok = false;
    for (; q < m && ok; ++q) { // near side: strictly outwards (its first shell may be the far side's last)
      const int k = lay(q);
      if (k <= prev) { ok = false; break; }
      near[(size_t)r * n_layers + k] = a + q;
      prev = k;
      l_min = std::min(l_min, k); l_max = std::max(l_max, k);
    }
  }
  *l_min_out = l_min;
  *l_max_out = l_max;
  return ok && l_max >= l_min;
}

// The shells of [l_min, l_max] some ray of the batch has a segment in (fold_sides' far / near [n_rays][n_shells]),
// outermost first: the visits of the folded kernels.
inline std::vector<int> fold_shells(const std::vector<int> &far, const std::vector<int> &near, int n_rays, int n_shells, int l_min,
                                    int l_max) {
  std::vector<int> shells;
  for (int k = l_max; k >= l_min; --k) {
    bool any = false;
    for (int r = 0; r < n_rays && !any; ++r) any = far[(size_t)r * n_shells + k] >= 0 || near[(size_t)r * n_shells + k] >= 0;
    if (any) shells.push_back(k);
  }
  return shells;
}

// ---- the one-pass Jacobian kernels' plans ----

// Plan of the one-pass Jacobian kernel (sr_limb_adjoint_kernel): per segment, in the order the recursion walks
// them, the layer with its first-touch flag and the column parameters the segment touches (d col / d x_p != 0 iff
// the parameter's weight is non-zero at one of the segment's sample points), runs of consecutive touches carried
// in one of kAdjSlots registers; per ray the rows it never touches.  Returns false when a segment touches more than
// kAdjEnt parameters (the forward-sensitivity kernel takes those calls).
struct AdjPlan {
  std::vector<int> seg;      // [n_seg][kAdjPlanInts]
  std::vector<int> zero_off; // [n_rays + 1]
  std::vector<int> zero_row; // layer rows (< n_layers) and parameter rows (n_layers + p)
};
// The column-parameter entries of a ray's walk, step by step (a segment, or a shell visit of the folded plan): the
// parameters whose next touch (touch[p]: ascending steps) is this step; runs of consecutive touches are carried in one
// of kAdjSlots registers while one is free.
struct RunPlan {
  bool slot_busy[kAdjSlots] = {};
  std::vector<int> slot_of, pos;
  std::vector<char> seen; // the parameter has been written in this ray
  explicit RunPlan(int n_par) : slot_of(std::max(n_par, 1), -1), pos(std::max(n_par, 1), 0), seen(std::max(n_par, 1), 0) {}
  // the step's entries (ent_p[kAdjEnt], ent_gf[kAdjEnt]); returns their number, or -1 when more than kAdjEnt touch it
  int step(int at, const std::vector<std::vector<int>> &touch, const int32_t *par_gas, int *ent_p, int *ent_gf) {
    int n_ent = 0;
    for (int p = 0; p < (int)touch.size(); ++p) {
      if (pos[p] >= (int)touch[p].size() || touch[p][pos[p]] != at) continue;
      if (n_ent == kAdjEnt) return -1;
      const bool next_too = pos[p] + 1 < (int)touch[p].size() && touch[p][pos[p] + 1] == at + 1;
      int fl = 0, sl = slot_of[p];
      if (sl < 0) { // no carry in: a run starts here
        fl |= 1;
        if (next_too)
          for (int c = 0; c < kAdjSlots; ++c)
            if (!slot_busy[c]) { sl = c; slot_busy[c] = true; break; }
      }
      const bool carry_out = next_too && sl >= 0;
      if (!carry_out) {
        fl |= 2;                    // written here
        if (!seen[p]) fl |= 4;      // first write of this parameter in the ray: store
        seen[p] = 1;
        if (sl >= 0) slot_busy[sl] = false;
        slot_of[p] = -1;
      } else {
        slot_of[p] = sl;
      }
      ent_p[n_ent] = p;
      ent_gf[n_ent] = par_gas[p] | (std::max(sl, 0) << 8) | (fl << 16);
      ++n_ent;
      ++pos[p];
    }
    return n_ent;
  }
};

inline bool build_adj_plan(const sr_los_desc *los, int n_layers, const int32_t *seg_jrow, int n_jrows, int n_par,
                           const int32_t *par_gas, const double *par_w, bool want_layer, int n_pt, AdjPlan *out) {
  const int nr = los->n_rays, n_seg = los->seg_off[nr];
  out->seg.assign((size_t)n_seg * kAdjPlanInts, 0);
  out->zero_off.assign(nr + 1, 0);
  out->zero_row.clear();
  std::vector<char> lay_seen(n_jrows);
  std::vector<std::vector<int>> touch(n_par); // walk positions (within the ray) of the segments touching p
  for (int r = 0; r < nr; ++r) {
    const int a = los->seg_off[r], b = los->seg_off[r + 1], m = b - a;
    std::fill(lay_seen.begin(), lay_seen.end(), 0);
    auto orig = [&](int q) { return los->los_order == 0 ? a + q : a + (m - 1 - q); }; // walk position -> caller's segment
    for (int q = 0; q < m; ++q) {
      int *pl = &out->seg[(size_t)(a + q) * kAdjPlanInts];
      const int k = los->seg_layer[orig(q)], jr = seg_jrow ? seg_jrow[orig(q)] : k;
      pl[0] = k;
      pl[1] = lay_seen[jr] ? 0 : 1;
      pl[3] = jr;
      lay_seen[jr] = 1;
    }
    for (int p = 0; p < n_par; ++p) {
      touch[p].clear();
      const double *w = par_w + (size_t)p * n_pt;
      for (int q = 0; q < m; ++q) {
        const int s = orig(q);
        bool nz = false;
        for (int i = los->pt_off[s]; i < los->pt_off[s + 1] && !nz; ++i) nz = w[i] != 0.0;
        if (nz) touch[p].push_back(q);
      }
    }
    RunPlan runs(n_par);
    for (int q = 0; q < m; ++q) {
      int *pl = &out->seg[(size_t)(a + q) * kAdjPlanInts];
      pl[2] = runs.step(q, touch, par_gas, pl + 4, pl + 4 + kAdjEnt);
      if (pl[2] < 0) return false;
    }
    if (want_layer)
      for (int k = 0; k < n_jrows; ++k)
        if (!lay_seen[k]) out->zero_row.push_back(k);
    for (int p = 0; p < n_par; ++p)
      if (!runs.seen[p]) out->zero_row.push_back(n_jrows + p);
    out->zero_off[r + 1] = (int)out->zero_row.size();
  }
  return true;
}

// The folded plan (sr_limb_adjoint_fold_kernel, the default): plan [n_rays][n_vis][kFoldPlanInts], one visit per shell
// of `shells` (fold_shells: outermost first) with the ray's far-side and near-side segment there (far / near
// [n_rays][n_shells], fold_sides); a column parameter's touches -- read off the per-segment plan `adj` -- are planned over
// the VISITS (a level acts on the same shells on both sides: one run, one register, one store).  A record:
//   pl[0]  coefficient row of the far-side segment, pl[12] of the near-side one: the shell, or with two_rows (3-D paths:
//          a coefficient row per LOS step, shells = Jacobian rows) the segments' own -- a side without a segment takes
//          the other's: its loads are not used
//   pl[1], pl[2]  far-side and near-side segment or -1;  pl[3], pl[4 ..], pl[4 + kAdjEnt ..]  the visit's entries
//   pl[13] the shell = the row of the per-layer Jacobian
// false (plan left empty): a shell's two segments touch more than kAdjEnt parameters between them -- such calls take one
// ray per thread in path order.
inline bool build_fold_plan(const AdjPlan &adj, const std::vector<int> &far, const std::vector<int> &near,
                            const std::vector<int> &shells, int n_rays, int n_shells, bool two_rows, int n_par,
                            const int32_t *par_gas, std::vector<int> *plan) {
  const int n_vis = (int)shells.size();
  std::vector<int> &fplan = *plan;
  fplan.assign((size_t)n_rays * n_vis * kFoldPlanInts, 0);
  bool fits = true;
  std::vector<std::vector<int>> touch(n_par);
  auto rec_at = [&](int ray, int v) { return &fplan[((size_t)ray * n_vis + v) * kFoldPlanInts]; };
  for (int ray = 0; ray < n_rays && fits; ++ray) {
    for (int v = 0; v < n_vis; ++v) {
      int *pl = rec_at(ray, v);
      pl[1] = far[(size_t)ray * n_shells + shells[v]];
      pl[2] = near[(size_t)ray * n_shells + shells[v]];
      const int row_f = pl[1] >= 0 ? adj.seg[(size_t)pl[1] * kAdjPlanInts] : -1;
      const int row_n = pl[2] >= 0 ? adj.seg[(size_t)pl[2] * kAdjPlanInts] : -1;
      pl[0] = two_rows ? (row_f >= 0 ? row_f : std::max(row_n, 0)) : shells[v];
      pl[4 + 2 * kAdjEnt] = two_rows ? (row_n >= 0 ? row_n : std::max(row_f, 0)) : shells[v];
      pl[5 + 2 * kAdjEnt] = shells[v];
    }
    if (n_par == 0) continue;
    for (int p = 0; p < n_par; ++p) touch[p].clear();
    for (int v = 0; v < n_vis; ++v) {
      const int *pl = rec_at(ray, v);
      for (int side = 1; side <= 2; ++side) {
        if (pl[side] < 0) continue;
        const int *sp = &adj.seg[(size_t)pl[side] * kAdjPlanInts];
        for (int e = 0; e < sp[2]; ++e)
          if (touch[sp[4 + e]].empty() || touch[sp[4 + e]].back() != v) touch[sp[4 + e]].push_back(v);
      }
    }
    RunPlan runs(n_par);
    for (int v = 0; v < n_vis && fits; ++v) {
      int *pl = rec_at(ray, v);
      pl[3] = runs.step(v, touch, par_gas, pl + 4, pl + 4 + kAdjEnt);
      fits = pl[3] >= 0;
    }
  }
  if (!fits) fplan.clear();
  return fits;
}

// The layer-synchronous schedule (sr_limb_adjoint_sync_kernel) of rays that share their coefficient rows and walk them
// monotonically down to a turning shell and up again (fold_sides' far / near [n_rays][n_layers]): the shells are listed
// once -- far side from the outermost shell inwards, near side outwards -- with every ray's segment in each, so that the
// kernel loads a shell's coefficients once for kAdjSyncRays rays.  sched [n_batches][n_visits][1 + kAdjSyncRays] = the
// layer, then the segment of each ray of the batch there or -1 (also the rays the last batch does not have).  Every
// batch walks every visit (a batch skips nothing: a visit none of its rays takes costs one load).
inline void build_sync_schedule(const std::vector<int> &far, const std::vector<int> &near, int n_rays, int n_layers, int l_min,
                                int l_max, std::vector<int> *sched_out, int *n_visits_out) {
  std::vector<std::pair<int, int>> visits; // (side, layer)
  for (int k = l_max; k >= l_min; --k) {
    bool any = false;
    for (int r = 0; r < n_rays && !any; ++r) any = far[(size_t)r * n_layers + k] >= 0;
    if (any) visits.push_back({0, k});
  }
  for (int k = l_min; k <= l_max; ++k) {
    bool any = false;
    for (int r = 0; r < n_rays && !any; ++r) any = near[(size_t)r * n_layers + k] >= 0;
    if (any) visits.push_back({1, k});
  }
  const int n_visits = (int)visits.size(), n_batches = (n_rays + kAdjSyncRays - 1) / kAdjSyncRays;
  std::vector<int> &sched = *sched_out;
  sched.assign((size_t)n_batches * n_visits * (1 + kAdjSyncRays), -1);
  for (int bt = 0; bt < n_batches; ++bt)
    for (int v = 0; v < n_visits; ++v) {
      int *sv = &sched[((size_t)bt * n_visits + v) * (1 + kAdjSyncRays)];
      sv[0] = visits[v].second;
      for (int i = 0; i < kAdjSyncRays; ++i) {
        const int r = bt * kAdjSyncRays + i;
        if (r < n_rays) sv[1 + i] = (visits[v].first ? near : far)[(size_t)r * n_layers + visits[v].second];
      }
    }
  *n_visits_out = n_visits;
}

// ---- the state kernel's plan ----

// The host plan of sr_limb_jac_state_kernel: the column parameters in the caller's order, then the level parameters in
// level order, then the row parameters in the caller's order, NP per block: a block's column slots come first and stand
// for consecutive rows of dcol (blk: their number and gases), a row's level entries come in level order without a sort
// of their own, the entries of its row slots (level kLevelEntRows, c = par_t[p][r]) behind them.
// par_lgas (several level-factored gases): level parameter p belongs to level gas par_lgas[p]; the level parameters are
// then listed by (level gas, level) and an entry carries level | level gas << kLevelEntGasShift.  Without it the plan is
// the one-gas plan, word for word.
// n_hid (the pointing derivative): n_hid more column slots behind the caller's, slot g of gas g, whose rows of dcol follow
// the caller's; their rows of jac come LAST, n_col + n_lev + n_row + g, the other kinds keep the rows they have without.
// gas_bits (state_gas_bits of the batch): the bits a column slot's gas takes in the gas word; with 3 the blocks have
// kLevelJacNPSmall slots.  With 2 the plan is what it always was.
struct LevelJacPlan {
  int n_blocks;
  std::vector<int> blk, ent_off, slot_par;
  std::vector<LevelEnt> ent;
};
inline LevelJacPlan level_jac_plan(int n_col, const int32_t *par_gas, int n_lev, const int32_t *par_level, const double *par_c,
                                   int n_layers, int n_row = 0, const double *par_t = nullptr, const int32_t *par_lgas = nullptr,
                                   int n_hid = 0, int gas_bits = 2) {
  const int n_state = n_col + n_lev + n_row;
  const int nc_all = n_col + n_hid, n_cl = nc_all + n_lev, n_par = n_cl + n_row, np = level_jac_np(n_par, gas_bits);
  const int n_blocks = std::max(1, (n_par + np - 1) / np); // (no parameter at all, the instrument rows alone: one block of unused slots)
  std::vector<int32_t> packed; // the `level` words of the entries: the level, with several level gases the gas above it
  if (par_lgas) {
    packed.resize((size_t)n_lev);
    for (int p = 0; p < n_lev; ++p) packed[p] = par_level[p] | par_lgas[p] << kLevelEntGasShift;
    par_level = packed.data();
  }
  const std::vector<int> order = order_by_level(n_lev, par_level);
  LevelJacPlan P{n_blocks, std::vector<int>((size_t)n_blocks * 2, 0), std::vector<int>((size_t)n_blocks * (n_layers + 1)),
                 std::vector<int>((size_t)n_blocks * np, -1), {}};
  for (int b = 0; b < n_blocks; ++b) {
    const int i0 = b * np, i1 = std::min(n_par, i0 + np), nc = std::max(0, std::min(nc_all, i1) - i0);
    unsigned gases = 0u;
    for (int i = i0; i < i0 + nc; ++i) gases |= (unsigned)(i < n_col ? par_gas[i] : i - n_col) << (gas_bits * (i - i0));
    P.blk[2 * b] = nc;
    P.blk[2 * b + 1] = (int)gases;
    for (int i = i0; i < i1; ++i)
      P.slot_par[i] = i < n_col ? i : i < nc_all ? n_state + (i - n_col) : i < n_cl ? n_col + order[i - nc_all] : i - n_hid;
    for (int r = 0; r < n_layers; ++r) {
      P.ent_off[(size_t)b * (n_layers + 1) + r] = (int)P.ent.size();
      for (int i = std::max(i0, nc_all); i < std::min(i1, n_cl); ++i) {
        const int p = order[i - nc_all];
        const double c = par_c[(size_t)p * n_layers + r];
        if (c != 0.0) P.ent.push_back(LevelEnt{i - i0, par_level[p], c});
      }
      for (int i = std::max(i0, n_cl); i < i1; ++i) {
        const double c = par_t[(size_t)(i - n_cl) * n_layers + r];
        if (c != 0.0) P.ent.push_back(LevelEnt{i - i0, kLevelEntRows, c});
      }
    }
    P.ent_off[(size_t)b * (n_layers + 1) + n_layers] = (int)P.ent.size();
  }
  return P;
}

// The plan PER RAY (sr_set_state_ray_blocks; the kernel's instances whose parameter pack ends in a StateRayBlocks): every
// ray lists the parameters that touch it -- a column parameter iff par_w[p] is non-zero at one of the ray's sample points,
// a level or row parameter iff par_c[p][r] / par_t[p][r] is non-zero on the coefficient row r of one of its segments, the
// n_hid hidden slots always -- in level_jac_plan's order (columns, hidden, levels by (level gas, level), rows), and cuts
// ITS list into blocks of np: 8 if no ray is touched by more than 8 parameters (or gas_bits is 3), else 16.  A ray has at least block 0 (the
// radiance's), also with an empty list.  The blocks of all rays lie one behind the other: ray_blk_off [n_rays + 1] is the
// prefix sum of the rays' block counts, and blk [.][2], col_row [.][np], ent_off [.][n_layers + 1] and slot_par [.][np]
// are indexed by ray_blk_off[ray] + block.  col_row: the row of dcol behind each column slot (p of a caller's parameter,
// n_col + g of hidden slot g; 0 behind the other slots), since a ray's column slots are no longer consecutive parameters.
// The entries of (ray block, row) are the dense plan's entries of the block's parameters on that row, in its order, with
// the block's slot numbers -- on the rows the ray has a segment on; the other rows' lists, which the ray never reads,
// are empty (with a coefficient row per LOS step they would be n_rays times the dense plan's).  n_blocks: the largest
// block count of a ray, the launch's gridDim.z.
struct RayJacPlan {
  int np, n_blocks;
  std::vector<int> ray_blk_off, blk, col_row, ent_off, slot_par;
  std::vector<LevelEnt> ent;
};
inline RayJacPlan ray_jac_plan(const sr_los_desc *los, int n_col, const int32_t *par_gas, const double *par_w, int n_lev,
                               const int32_t *par_level, const double *par_c, int n_layers, int n_row = 0,
                               const double *par_t = nullptr, const int32_t *par_lgas = nullptr, int n_hid = 0, int gas_bits = 2) {
  const int n_rays = los->n_rays, n_state = n_col + n_lev + n_row, n_pt = los->pt_off[los->seg_off[n_rays]];
  std::vector<int32_t> packed;
  if (par_lgas) {
    packed.resize((size_t)n_lev);
    for (int p = 0; p < n_lev; ++p) packed[p] = par_level[p] | par_lgas[p] << kLevelEntGasShift;
    par_level = packed.data();
  }
  const std::vector<int> order = order_by_level(n_lev, par_level);
  // a ray's list: (kind 0 column / hidden, 1 level, 2 row; index within the kind -- a hidden slot g is column n_col + g)
  struct Item { int kind, idx; };
  std::vector<std::vector<Item>> lists(n_rays);
  std::vector<std::vector<int>> rows_of(n_rays); // the distinct coefficient rows of a ray, ascending
  std::vector<char> on_ray((size_t)std::max(n_layers, 1));
  size_t longest = 0;
  for (int ray = 0; ray < n_rays; ++ray) {
    const int s0 = los->seg_off[ray], s1 = los->seg_off[ray + 1];
    std::fill(on_ray.begin(), on_ray.end(), 0);
    for (int s = s0; s < s1; ++s) on_ray[los->seg_layer[s]] = 1;
    for (int r = 0; r < n_layers; ++r)
      if (on_ray[r]) rows_of[ray].push_back(r);
    auto weighs = [&](const double *c) { // a level or row parameter's coefficients [n_layers]
      for (int r : rows_of[ray])
        if (c[r] != 0.0) return true;
      return false;
    };
    std::vector<Item> &lst = lists[ray];
    for (int p = 0; p < n_col; ++p) {
      const double *w = par_w + (size_t)p * n_pt;
      bool nz = false;
      for (int i = los->pt_off[s0]; i < los->pt_off[s1] && !nz; ++i) nz = w[i] != 0.0;
      if (nz) lst.push_back(Item{0, p});
    }
    for (int g = 0; g < n_hid; ++g) lst.push_back(Item{0, n_col + g});
    for (int i = 0; i < n_lev; ++i)
      if (weighs(par_c + (size_t)order[i] * n_layers)) lst.push_back(Item{1, order[i]});
    for (int p = 0; p < n_row; ++p)
      if (weighs(par_t + (size_t)p * n_layers)) lst.push_back(Item{2, p});
    longest = std::max(longest, lst.size());
  }
  RayJacPlan P{};
  P.np = level_jac_np((int)std::min(longest, (size_t)INT_MAX), gas_bits);
  const int np = P.np;
  P.ray_blk_off.assign((size_t)n_rays + 1, 0);
  for (int ray = 0; ray < n_rays; ++ray) {
    const int nb = std::max(1, ((int)lists[ray].size() + np - 1) / np);
    P.ray_blk_off[ray + 1] = P.ray_blk_off[ray] + nb;
    P.n_blocks = std::max(P.n_blocks, nb);
  }
  const size_t n_rb = (size_t)P.ray_blk_off[n_rays];
  P.blk.assign(n_rb * 2, 0);
  P.col_row.assign(n_rb * np, 0);
  P.slot_par.assign(n_rb * np, -1);
  P.ent_off.assign(n_rb * (n_layers + 1), 0);
  for (int ray = 0; ray < n_rays; ++ray) {
    const std::vector<Item> &lst = lists[ray];
    for (int rb = P.ray_blk_off[ray]; rb < P.ray_blk_off[ray + 1]; ++rb) {
      const int i0 = (rb - P.ray_blk_off[ray]) * np, i1 = std::min((int)lst.size(), i0 + np);
      int nc = 0;
      unsigned gases = 0u;
      for (int i = i0; i < i1; ++i) {
        const Item &it = lst[i];
        const int q = i - i0;
        if (it.kind == 0) {
          gases |= (unsigned)(it.idx < n_col ? par_gas[it.idx] : it.idx - n_col) << (gas_bits * q);
          P.col_row[(size_t)rb * np + q] = it.idx;
          ++nc;
        }
        P.slot_par[(size_t)rb * np + q] = it.kind == 0   ? (it.idx < n_col ? it.idx : n_state + (it.idx - n_col))
                                          : it.kind == 1 ? n_col + it.idx
                                                         : n_col + n_lev + it.idx;
      }
      P.blk[2 * (size_t)rb] = nc;
      P.blk[2 * (size_t)rb + 1] = (int)gases;
      int *eo = &P.ent_off[(size_t)rb * (n_layers + 1)];
      size_t next_row = 0;
      for (int r = 0; r < n_layers; ++r) {
        eo[r] = (int)P.ent.size();
        if (next_row == rows_of[ray].size() || rows_of[ray][next_row] != r) continue;
        ++next_row;
        for (int i = i0; i < i1; ++i) {
          const Item &it = lst[i];
          if (it.kind == 0) continue;
          const double c = (it.kind == 1 ? par_c : par_t)[(size_t)it.idx * n_layers + r];
          if (c != 0.0) P.ent.push_back(LevelEnt{i - i0, it.kind == 1 ? par_level[it.idx] : kLevelEntRows, c});
        }
      }
      eo[n_layers] = (int)P.ent.size();
    }
  }
  return P;
}

} // namespace sr
