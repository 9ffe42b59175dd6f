// The host plans of the one-pass limb Jacobian kernels and of the state kernel (spectrobot_amd/csrc/sr_limb_plan.hpp, no
// kernel text), interpreted the way the kernels read them, on hand-built ray batches.  Every (parameter, segment) touch
// and every (Jacobian row, segment) visit gets a random contribution (whole numbers: their sums are exact in any order);
// outputs start as NaN.
//   segment plan (sr_limb_adjoint_kernel, build_adj_plan): each ray walked with its carries in kAdjSlots slots, by bit 0
//     (run starts), bit 1 (write) and bit 2 (first write stores, else adds) of ent_gf, bit 0 of `flags` for the layer row,
//     and the zero_row lists: every output ends as the plain sum of its contributions or exactly 0, is stored exactly
//     once per ray before any add, and no slot is read without a carry in or overwritten while it holds one;
//   folded plan (build_fold_plan): the same through the kFoldPlanInts records over the visits; every segment of a ray
//     exactly once, as a far or a near entry, the shells strictly descending, pl[0], pl[12], pl[13] as build_fold_plan's
//     comment states, for one-row and two-row calls;
//   sync schedule (build_sync_schedule): every segment of every ray exactly once, in a visit of its own layer, a ray's
//     segments in walk order (far visits before near visits), the tail batch padded with -1;
//   level_jac_plan at its block boundaries (n_par = NP - 1, NP, NP + 1 for both NP, with and without par_lgas and n_hid):
//     slot_par a permutation onto the rows its comment promises, ent_off monotone and ending at ent.size(), the entries
//     those of the non-zero coefficients, in level order, row entries behind them.
// Built with AddressSanitizer and UBSan by tools/host_sim/run.sh limb_plan_host.
#include <cmath>
#include <cstdio>
#include <functional>
#include <random>

#include "sr_limb_plan.hpp"
using namespace sr;

static int g_bad = 0;
static const char *g_case = "";
#define CHECK(cond, ...)                                      \
  do {                                                        \
    if (!(cond)) {                                            \
      if (g_bad++ < 40) {                                     \
        std::printf("%s: " #cond " -- ", g_case);             \
        std::printf(__VA_ARGS__);                             \
        std::printf("\n");                                    \
      }                                                       \
    }                                                         \
  } while (0)

struct Ray { // in walk (photon) order
  std::vector<int> layer, jrow; // coefficient row; shell where it is not the coefficient row (3-D paths), else empty
};
// from shell `top` down to the turning shell `tan` and up again; twice: the far and the near side both have a segment there
static Ray limb(int top, int tan, bool twice) {
  Ray r;
  for (int k = top; k >= tan; --k) r.layer.push_back(k);
  for (int k = twice ? tan : tan + 1; k <= top; ++k) r.layer.push_back(k);
  return r;
}
static Ray slant(int bottom, int top) { // the outward half only
  Ray r;
  for (int k = bottom; k <= top; ++k) r.layer.push_back(k);
  return r;
}
static int shell_of(const Ray &r, int q) { return r.jrow.empty() ? r.layer[q] : r.jrow[q]; }

struct Case {
  const char *name;
  int n_layers, n_jrows; // n_jrows 0: no seg_jrow (the rows are the layers)
  int n_gas, n_par;
  std::vector<Ray> rays;
  std::function<bool(int p, const Ray &ray, int q)> touches;
  bool adj_fits, v_shaped, fold_fits;
};

// a ray's outputs as the kernels write them: stores, adds and the carry slots
struct Outputs {
  std::vector<double> par, lay;
  std::vector<int> par_stores, lay_stores;
  double slot[kAdjSlots];
  int owner[kAdjSlots]; // the parameter whose carry the slot holds, or -1
  Outputs(int n_par, int n_jrows) : par(n_par, NAN), lay(n_jrows, NAN), par_stores(n_par, 0), lay_stores(n_jrows, 0) {
    for (int c = 0; c < kAdjSlots; ++c) slot[c] = 0.0, owner[c] = -1;
  }
  static void put(std::vector<double> &out, std::vector<int> &stores, int row, double v, bool store) {
    CHECK(row >= 0 && row < (int)out.size(), "row %d", row);
    if (row < 0 || row >= (int)out.size()) return;
    if (store) {
      CHECK(stores[row] == 0, "row %d stored twice", row);
      out[row] = v;
      ++stores[row];
    } else {
      CHECK(stores[row] == 1, "row %d added to before its store", row);
      out[row] += v;
    }
  }
  void zero_rows(const AdjPlan &P, int ray, int n_jrows, bool want_layer) {
    for (int q = P.zero_off[ray]; q < P.zero_off[ray + 1]; ++q) {
      const int row = P.zero_row[q];
      if (row < n_jrows) {
        CHECK(want_layer, "layer row %d zeroed without a per-layer Jacobian", row);
        if (want_layer) put(lay, lay_stores, row, 0.0, true);
      } else {
        put(par, par_stores, row - n_jrows, 0.0, true);
      }
    }
  }
  void entry(int p, int gf, double v, const int32_t *par_gas) {
    const int g = gf & 0xff, sl = (gf >> 8) & 0xff, fl = gf >> 16;
    CHECK(p >= 0 && p < (int)par.size() && g == par_gas[p], "parameter %d gas %d", p, g);
    CHECK(sl < kAdjSlots && (fl & ~7) == 0, "slot %d flags %d", sl, fl);
    if (p < 0 || p >= (int)par.size() || sl >= kAdjSlots) return;
    if (!(fl & 1)) {
      CHECK(owner[sl] == p, "parameter %d reads slot %d without a carry in (holds %d)", p, sl, owner[sl]);
      v += slot[sl];
      owner[sl] = -1;
    }
    if (fl & 2) {
      put(par, par_stores, p, v, (fl & 4) != 0);
    } else {
      CHECK(owner[sl] < 0, "parameter %d overwrites the carry of %d in slot %d", p, owner[sl], sl);
      CHECK(!(fl & 4), "parameter %d: a store flag on a carry", p);
      slot[sl] = v;
      owner[sl] = p;
    }
  }
  void finish(const std::vector<double> &want_par, const std::vector<double> &want_lay, bool want_layer, int ray, const char *what) {
    for (int c = 0; c < kAdjSlots; ++c) CHECK(owner[c] < 0, "%s, ray %d: the carry of parameter %d is never written", what, ray, owner[c]);
    for (size_t p = 0; p < par.size(); ++p)
      CHECK(par[p] == want_par[p] && par_stores[p] == 1, "%s, ray %d parameter %zu: %g, plain sum %g, stores %d", what, ray, p, par[p], want_par[p], par_stores[p]);
    for (size_t k = 0; want_layer && k < lay.size(); ++k)
      CHECK(lay[k] == want_lay[k] && lay_stores[k] == 1, "%s, ray %d row %zu: %g, plain sum %g, stores %d", what, ray, k, lay[k], want_lay[k], lay_stores[k]);
  }
};

static void run_case(const Case &c, int los_order, bool want_layer, std::mt19937_64 &rng) {
  g_case = c.name;
  const int nr = (int)c.rays.size(), n_par = c.n_par;
  const bool two_rows = c.n_jrows > 0;
  const int n_jrows = two_rows ? c.n_jrows : c.n_layers;
  // the batch as a caller hands it over: observer order lists every ray backwards
  std::vector<int32_t> seg_off{0};
  for (const Ray &r : c.rays) seg_off.push_back(seg_off.back() + (int)r.layer.size());
  const int n_seg = seg_off.back(), n_pt = 2 * n_seg;
  std::vector<int32_t> seg_layer(n_seg), seg_jrow(n_seg), pt_off(n_seg + 1), par_gas(std::max(n_par, 1));
  std::vector<double> x(n_pt), nd(n_pt, 1.0), vmr((size_t)c.n_gas * n_pt, 1e-3), par_w((size_t)std::max(n_par, 1) * n_pt, 0.0);
  std::vector<int> w_layer(n_seg), w_jrow(n_seg), ray_of(n_seg); // by WALK-order segment index, the plans' numbering
  std::vector<double> c_lay(n_seg), c_par((size_t)std::max(n_par, 1) * n_seg, 0.0);
  std::uniform_int_distribution<int> whole(1, 1000);
  for (int p = 0; p < n_par; ++p) par_gas[p] = p % c.n_gas;
  for (int s = 0; s <= n_seg; ++s) pt_off[s] = 2 * s;
  for (int i = 0; i < n_pt; ++i) x[i] = (double)(i & 1);
  for (int r = 0; r < nr; ++r) {
    const Ray &ray = c.rays[r];
    const int a = seg_off[r], m = (int)ray.layer.size();
    for (int q = 0; q < m; ++q) {
      const int s = los_order == 0 ? a + q : a + (m - 1 - q);
      seg_layer[s] = w_layer[a + q] = ray.layer[q];
      seg_jrow[s] = w_jrow[a + q] = shell_of(ray, q);
      ray_of[a + q] = r;
      c_lay[a + q] = whole(rng);
      for (int p = 0; p < n_par; ++p)
        if (c.touches(p, ray, q)) {
          par_w[(size_t)p * n_pt + 2 * s + 1] = 0.5; // (the second sample point alone)
          c_par[(size_t)p * n_seg + a + q] = whole(rng);
        }
    }
  }
  sr_los_desc los{};
  los.n_rays = nr; los.n_gas = c.n_gas;
  los.seg_off = seg_off.data(); los.seg_layer = seg_layer.data(); los.pt_off = pt_off.data();
  los.x = x.data(); los.nd = nd.data(); los.vmr = vmr.data();
  los.los_order = los_order;
  LosShape shape;
  const int rc = check_los_par(&los, c.n_layers, n_par, par_gas.data(), par_w.data(), &shape);
  CHECK(rc == SR_OK && shape.n_seg == n_seg && shape.n_pt == n_pt, "check_los_par %d", rc);
  if (rc != SR_OK) return;
  // the plain sums
  std::vector<std::vector<double>> want_par(nr, std::vector<double>(n_par, 0.0)), want_lay(nr, std::vector<double>(n_jrows, 0.0));
  for (int s = 0; s < n_seg; ++s) {
    want_lay[ray_of[s]][w_jrow[s]] += c_lay[s];
    for (int p = 0; p < n_par; ++p) want_par[ray_of[s]][p] += c_par[(size_t)p * n_seg + s];
  }

  // ---- the segment plan
  AdjPlan P;
  const int32_t *jrow_arg = two_rows ? seg_jrow.data() : nullptr;
  const bool fits = build_adj_plan(&los, c.n_layers, jrow_arg, n_jrows, n_par, par_gas.data(), par_w.data(), want_layer, n_pt, &P);
  CHECK(fits == c.adj_fits, "build_adj_plan says %d", (int)fits);
  if (!fits) return;
  CHECK((int)P.seg.size() == n_seg * kAdjPlanInts && (int)P.zero_off.size() == nr + 1 && P.zero_off[nr] == (int)P.zero_row.size(), "sizes");
  for (int r = 0; r < nr; ++r) {
    Outputs O(n_par, n_jrows);
    O.zero_rows(P, r, n_jrows, want_layer);
    for (int s = seg_off[r]; s < seg_off[r + 1]; ++s) {
      const int *pl = &P.seg[(size_t)s * kAdjPlanInts];
      CHECK(pl[0] == w_layer[s] && pl[3] == w_jrow[s] && (pl[1] & ~1) == 0, "segment %d: layer %d row %d flags %d", s, pl[0], pl[3], pl[1]);
      if (want_layer) Outputs::put(O.lay, O.lay_stores, pl[3], c_lay[s], (pl[1] & 1) != 0);
      CHECK(pl[2] >= 0 && pl[2] <= kAdjEnt, "segment %d: %d entries", s, pl[2]);
      int n_touch = 0;
      for (int p = 0; p < n_par; ++p) n_touch += c_par[(size_t)p * n_seg + s] != 0.0;
      CHECK(pl[2] == n_touch, "segment %d: %d entries for %d touches", s, pl[2], n_touch);
      for (int e = 0; e < pl[2]; ++e) {
        const int p = pl[4 + e];
        CHECK(p >= 0 && p < n_par && c_par[(size_t)p * n_seg + s] != 0.0, "segment %d: an entry of parameter %d, which does not touch it", s, p);
        if (p >= 0 && p < n_par) O.entry(p, pl[4 + kAdjEnt + e], c_par[(size_t)p * n_seg + s], par_gas.data());
      }
    }
    O.finish(want_par[r], want_lay[r], want_layer, r, "segment plan");
  }

  // ---- the two sides
  const int n_sh = n_jrows;
  std::vector<int> far, near;
  int l_min = n_sh, l_max = -1;
  const bool ok = fold_sides(&los, n_sh, jrow_arg, &far, &near, &l_min, &l_max);
  CHECK(ok == c.v_shaped, "fold_sides says %d", (int)ok);
  if (!ok) return;

  // ---- the folded plan
  const std::vector<int> shells = fold_shells(far, near, nr, n_sh, l_min, l_max);
  const int n_vis = (int)shells.size();
  for (int v = 0; v < n_vis; ++v) CHECK(shells[v] >= l_min && shells[v] <= l_max && (v == 0 || shells[v] < shells[v - 1]), "shell %d of visit %d", shells[v], v);
  std::vector<int> fplan;
  const bool ffits = build_fold_plan(P, far, near, shells, nr, n_sh, two_rows, n_par, par_gas.data(), &fplan);
  CHECK(ffits == c.fold_fits, "build_fold_plan says %d", (int)ffits);
  CHECK((int)fplan.size() == (ffits ? nr * n_vis * kFoldPlanInts : 0), "fold plan of %zu ints", fplan.size());
  if (ffits && (int)fplan.size() == nr * n_vis * kFoldPlanInts) {
    std::vector<int> seen(n_seg, 0);
    for (int r = 0; r < nr; ++r) {
      Outputs O(n_par, n_jrows);
      O.zero_rows(P, r, n_jrows, want_layer);
      for (int v = 0; v < n_vis; ++v) {
        const int *pl = &fplan[((size_t)r * n_vis + v) * kFoldPlanInts];
        const int sf = pl[1], sn = pl[2], shell = pl[13];
        CHECK(shell == shells[v], "ray %d visit %d: shell %d", r, v, shell);
        double d = 0.0;
        for (int s : {sf, sn}) {
          if (s < 0) continue;
          CHECK(s >= seg_off[r] && s < seg_off[r + 1] && w_jrow[s] == shell, "ray %d visit %d: segment %d", r, v, s);
          if (s < seg_off[r] || s >= seg_off[r + 1]) return;
          ++seen[s];
          d += c_lay[s];
        }
        CHECK(sf < 0 || sn < 0 || sf < sn, "ray %d visit %d: far %d near %d", r, v, sf, sn);
        if (two_rows) {
          CHECK(pl[0] == (sf >= 0 ? w_layer[sf] : sn >= 0 ? w_layer[sn] : 0), "ray %d visit %d: far row %d", r, v, pl[0]);
          CHECK(pl[12] == (sn >= 0 ? w_layer[sn] : sf >= 0 ? w_layer[sf] : 0), "ray %d visit %d: near row %d", r, v, pl[12]);
        } else {
          CHECK(pl[0] == shell && pl[12] == shell, "ray %d visit %d: rows %d %d", r, v, pl[0], pl[12]);
        }
        if (sf < 0 && sn < 0) { // the kernel skips the record
          CHECK(pl[3] == 0, "ray %d visit %d: entries without a segment", r, v);
          continue;
        }
        if (want_layer) Outputs::put(O.lay, O.lay_stores, shell, d, true); // the kernel stores a visit's row, once
        CHECK(pl[3] >= 0 && pl[3] <= kAdjEnt, "ray %d visit %d: %d entries", r, v, pl[3]);
        for (int e = 0; e < pl[3]; ++e) {
          const int p = pl[4 + e];
          if (p < 0 || p >= n_par) { CHECK(false, "ray %d visit %d: parameter %d", r, v, p); continue; }
          const double val = (sf >= 0 ? c_par[(size_t)p * n_seg + sf] : 0.0) + (sn >= 0 ? c_par[(size_t)p * n_seg + sn] : 0.0);
          CHECK(val != 0.0, "ray %d visit %d: an entry of parameter %d, which touches neither segment", r, v, p);
          O.entry(p, pl[4 + kAdjEnt + e], val, par_gas.data());
        }
      }
      O.finish(want_par[r], want_lay[r], want_layer, r, "folded plan");
    }
    for (int s = 0; s < n_seg; ++s) CHECK(seen[s] == 1, "segment %d in %d visits of the folded plan", s, seen[s]);
  }

  // ---- the layer-synchronous schedule (rays that share their coefficient rows)
  if (two_rows) return;
  std::vector<int> sched;
  int n_visits = -1;
  build_sync_schedule(far, near, nr, c.n_layers, l_min, l_max, &sched, &n_visits);
  const int n_batches = (nr + kAdjSyncRays - 1) / kAdjSyncRays, stride = 1 + kAdjSyncRays;
  CHECK(n_visits > 0 && (int)sched.size() == n_batches * n_visits * stride, "schedule of %zu ints, %d visits", sched.size(), n_visits);
  if ((int)sched.size() != n_batches * n_visits * stride) return;
  std::vector<int> next(nr); // the segment a ray takes next: its own, in walk order
  for (int r = 0; r < nr; ++r) next[r] = seg_off[r];
  for (int bt = 0; bt < n_batches; ++bt) {
    bool up = false;
    for (int v = 0; v < n_visits; ++v) {
      const int *sv = &sched[((size_t)bt * n_visits + v) * stride];
      CHECK(sv[0] == sched[(size_t)v * stride], "batch %d visit %d: layer %d", bt, v, sv[0]);
      if (v > 0) { // far visits strictly inwards, then near visits strictly outwards (the turn may repeat its shell)
        const int prev = sv[-stride];
        CHECK(!up || sv[0] > prev, "batch %d visit %d: layer %d behind %d on the way out", bt, v, sv[0], prev);
        if (sv[0] >= prev) up = true;
      }
      for (int i = 0; i < kAdjSyncRays; ++i) {
        const int r = bt * kAdjSyncRays + i, s = sv[1 + i];
        if (r >= nr) { CHECK(s == -1, "batch %d: the padding holds %d", bt, s); continue; }
        if (s < 0) { CHECK(s == -1, "batch %d visit %d: %d", bt, v, s); continue; }
        CHECK(s == next[r] && s < seg_off[r + 1], "ray %d takes segment %d, its next is %d", r, s, next[r]);
        CHECK(s >= 0 && s < n_seg && w_layer[s] == sv[0], "ray %d: segment %d in a visit of layer %d", r, s, sv[0]);
        if (s == next[r]) ++next[r];
      }
    }
  }
  for (int r = 0; r < nr; ++r) CHECK(next[r] == seg_off[r + 1], "ray %d: %d of its segments scheduled", r, next[r] - seg_off[r]);
}

// level_jac_plan for n_col column, n_lev level and n_row row parameters, n_hid hidden column slots
static void check_level_plan(int n_col, int n_lev, int n_row, int n_hid, bool lgas, std::mt19937_64 &rng) {
  g_case = "level_jac_plan";
  std::uniform_real_distribution<double> U(0.0, 1.0);
  const int n_layers = 5, n_gas = 3, n_levels = 6, n_state = n_col + n_lev + n_row, n_all = n_state + n_hid;
  std::vector<int32_t> par_gas(n_col), par_level(n_lev), par_lgas(n_lev);
  for (auto &g : par_gas) g = (int)(U(rng) * n_gas) % n_gas;
  for (auto &l : par_level) l = (int)(U(rng) * n_levels) % n_levels;
  for (auto &k : par_lgas) k = (int)(U(rng) * 3) % 3;
  std::vector<double> par_c((size_t)n_lev * n_layers), par_t((size_t)n_row * n_layers);
  for (auto &v : par_c) v = U(rng) < 0.6 ? 0.2 + U(rng) : 0.0;
  for (auto &v : par_t) v = U(rng) < 0.6 ? 0.2 + U(rng) : 0.0;
  const LevelJacPlan P = level_jac_plan(n_col, par_gas.data(), n_lev, par_level.data(), par_c.data(), n_layers, n_row, par_t.data(),
                                        lgas ? par_lgas.data() : nullptr, n_hid);
  const int np = level_jac_np(n_all), nc_all = n_col + n_hid, n_cl = nc_all + n_lev;
  auto word = [&](int p) { return lgas ? par_level[p] | par_lgas[p] << kLevelEntGasShift : par_level[p]; };
  CHECK(np == (n_all > kLevelJacNPSmall ? kLevelJacNPLarge : kLevelJacNPSmall), "NP %d for %d", np, n_all);
  CHECK(P.n_blocks == std::max(1, (n_all + np - 1) / np), "%d blocks for %d parameters", P.n_blocks, n_all);
  CHECK((int)P.blk.size() == 2 * P.n_blocks && (int)P.slot_par.size() == P.n_blocks * np && (int)P.ent_off.size() == P.n_blocks * (n_layers + 1), "sizes");
  if ((int)P.slot_par.size() != P.n_blocks * np || (int)P.ent_off.size() != P.n_blocks * (n_layers + 1)) return;
  // slot_par: a permutation onto the rows; column slots the caller's rows, hidden slots the LAST rows, level slots by
  // (level gas, level) onto n_col + p, row slots n_col + n_lev + p in the caller's order
  std::vector<int> hit(n_all, 0);
  int prev_word = INT_MIN;
  for (int i = 0; i < P.n_blocks * np; ++i) {
    const int row = P.slot_par[i];
    if (i >= n_all) { CHECK(row == -1, "slot %d beyond the parameters holds %d", i, row); continue; }
    CHECK(row >= 0 && row < n_all, "slot %d: row %d", i, row);
    if (row < 0 || row >= n_all) continue;
    ++hit[row];
    if (i < n_col) CHECK(row == i, "column slot %d: row %d", i, row);
    else if (i < nc_all) CHECK(row == n_state + (i - n_col), "hidden slot %d: row %d", i, row);
    else if (i < n_cl) {
      CHECK(row >= n_col && row < n_col + n_lev, "level slot %d: row %d", i, row);
      if (row >= n_col && row < n_col + n_lev) {
        CHECK(word(row - n_col) >= prev_word, "level slot %d out of level order", i);
        prev_word = word(row - n_col);
      }
    } else CHECK(row == i - n_hid, "row slot %d: row %d", i, row);
  }
  for (int row = 0; row < n_all; ++row) CHECK(hit[row] == 1, "row %d on %d slots", row, hit[row]);
  int at = 0;
  for (int b = 0; b < P.n_blocks; ++b) {
    const int i0 = b * np, nc = std::max(0, std::min(nc_all, i0 + np) - i0);
    CHECK(P.blk[2 * b] == nc, "block %d: %d column slots", b, P.blk[2 * b]);
    for (int q = 0; q < nc; ++q) {
      const int i = i0 + q, g = ((unsigned)P.blk[2 * b + 1] >> (2 * q)) & 3;
      CHECK(g == (i < n_col ? par_gas[i] : i - n_col), "block %d slot %d: gas %d", b, q, g);
    }
    for (int r = 0; r <= n_layers; ++r) {
      const int off = P.ent_off[(size_t)b * (n_layers + 1) + r];
      CHECK(off >= at && off <= (int)P.ent.size(), "block %d row %d: offset %d behind %d", b, r, off, at);
      if (off < at || off > (int)P.ent.size()) return;
      if (r > 0) { // the entries of row r - 1: [at, off)
        int n_want = 0, last = INT_MIN;
        for (int i = std::max(i0, nc_all); i < std::min(i0 + np, n_all); ++i)
          n_want += (i < n_cl ? par_c[(size_t)(P.slot_par[i] - n_col) * n_layers + (r - 1)] : par_t[(size_t)(i - n_cl) * n_layers + (r - 1)]) != 0.0;
        CHECK(off - at == n_want, "block %d row %d: %d entries for %d non-zero coefficients", b, r - 1, off - at, n_want);
        for (int e = at; e < off; ++e) {
          const LevelEnt &E = P.ent[e];
          const int i = i0 + E.slot;
          CHECK(E.slot >= 0 && E.slot < np && i >= nc_all && i < n_all, "entry %d: slot %d", e, E.slot);
          if (E.slot < 0 || E.slot >= np || i < nc_all || i >= n_all) continue;
          if (i < n_cl) {
            const int p = P.slot_par[i] - n_col;
            CHECK(E.level == word(p) && E.c == par_c[(size_t)p * n_layers + (r - 1)] && E.level >= last, "entry %d: level %d c %g", e, E.level, E.c);
            last = E.level;
          } else {
            CHECK(E.level == kLevelEntRows && E.c == par_t[(size_t)(i - n_cl) * n_layers + (r - 1)], "entry %d: row slot, level %d c %g", e, E.level, E.c);
            last = INT_MAX; // no level entry behind a row entry
          }
        }
      } else CHECK(off == at, "block %d starts at %d, the block before ended at %d", b, off, at);
      at = off;
    }
  }
  CHECK(at == (int)P.ent.size(), "the offsets end at %d of %zu entries", at, P.ent.size());
}

int main() {
  std::mt19937_64 rng(20261019);
  // level L of a gas acts on the shells L and L - 1 (triangular weights: runs of two, on the way down and again on the way up)
  auto triangular = [](int p, const Ray &ray, int q) { const int k = shell_of(ray, q); return k == p || k == p - 1; };
  auto in_shell = [](int shell, int n) { // parameters 0 .. n - 1 touch that shell, parameter n + k the shell k
    return [=](int p, const Ray &ray, int q) { return p < n ? shell_of(ray, q) == shell : shell_of(ray, q) == p - n; };
  };
  Ray steps3d_a{{0, 1, 2, 3, 4, 5}, {3, 2, 1, 1, 2, 3}}, steps3d_b{{6, 7, 8, 9}, {3, 2, 2, 3}}, steps3d_c{{10, 11}, {2, 3}};
  const std::vector<Case> cases = {
      // turning shells 0 (once), 2 (twice), 5 (once: misses the lower shells), 7 (twice: the top shell alone), 3: five rays,
      // kAdjSyncRays = 2: a partial last batch
      {"limb rays", 8, 0, 2, 9, {limb(7, 0, false), limb(7, 2, true), limb(6, 5, false), limb(7, 7, true), limb(7, 3, false)}, triangular, true, true, true},
      {"slant and limb rays", 8, 0, 3, 9, {slant(3, 7), limb(7, 1, true), slant(0, 5)}, triangular, true, true, true},
      {"one ray", 6, 0, 1, 7, {limb(5, 2, false)}, triangular, true, true, true},
      {"no parameter", 6, 0, 1, 0, {limb(5, 2, true), limb(4, 0, false), slant(1, 5)}, triangular, true, true, true},
      {"kAdjEnt touches in a shell", 6, 0, 2, kAdjEnt + 6, {limb(5, 1, false), limb(5, 3, true)}, in_shell(3, kAdjEnt - 1), true, true, true},
      {"kAdjEnt + 1 touches in a segment", 6, 0, 2, kAdjEnt + 6, {limb(5, 1, false), limb(5, 3, true)}, in_shell(3, kAdjEnt), false, true, true},
      // shell 3: kAdjEnt - 1 parameters touch its far-side segment, as many others its near-side one
      {"a visit over kAdjEnt, its segments not", 6, 0, 2, 2 * (kAdjEnt - 1), {limb(5, 1, false), limb(5, 0, true)},
       [](int p, const Ray &ray, int q) { return shell_of(ray, q) == 3 && (p < kAdjEnt - 1) == (2 * q < (int)ray.layer.size()); }, true, true, false},
      {"a ray that is no V", 6, 0, 2, 7, {limb(5, 2, false), Ray{{5, 4, 5, 4, 3}, {}}}, triangular, true, false, true},
      {"a ray that turns outwards twice", 6, 0, 1, 7, {Ray{{3, 2, 3, 2}, {}}}, triangular, true, false, true},
      // 3-D paths: a coefficient row per LOS step (12 rows), four altitude layers as Jacobian rows
      {"rows per LOS step", 12, 4, 2, 5, {steps3d_a, steps3d_b, steps3d_c}, triangular, true, true, true},
      {"rows per LOS step, a visit over kAdjEnt", 12, 4, 2, 2 * (kAdjEnt - 1), {steps3d_a, steps3d_b},
       [](int p, const Ray &ray, int q) { return shell_of(ray, q) == 2 && (p < kAdjEnt - 1) == (2 * q < (int)ray.layer.size()); }, true, true, false},
  };
  for (const Case &c : cases)
    for (int los_order = 0; los_order < 2; ++los_order)
      for (int want_layer = 0; want_layer < 2; ++want_layer) {
        const int before = g_bad;
        run_case(c, los_order, want_layer != 0, rng);
        std::printf("%-42s order %d, per-layer rows %d: %s\n", c.name, los_order, want_layer, g_bad == before ? "ok" : "FAILED");
      }
  const int before = g_bad;
  int n_plans = 0;
  for (int n_par : {kLevelJacNPSmall - 1, kLevelJacNPSmall, kLevelJacNPSmall + 1, kLevelJacNPLarge - 1, kLevelJacNPLarge, kLevelJacNPLarge + 1,
                    2 * kLevelJacNPLarge + 1})
    for (int n_hid : {0, 3})
      for (int lgas = 0; lgas < 2; ++lgas)
        for (int split = 0; split < 4; ++split) { // all level slots; columns + levels; all three kinds; columns and rows alone
          const int n = n_par - n_hid;
          const int n_col = split == 0 ? 0 : split == 3 ? n / 2 : n / 3, n_row = split == 2 ? n / 4 : split == 3 ? n - n_col : 0;
          check_level_plan(n_col, n - n_col - n_row, n_row, n_hid, lgas != 0, rng);
          ++n_plans;
        }
  check_level_plan(0, 0, 0, 0, false, rng); // no parameter at all: one block of unused slots
  std::printf("level_jac_plan, %d plans: %s\n", n_plans + 1, g_bad == before ? "ok" : "FAILED");
  std::printf(g_bad ? "FAILED (%d checks)\n" : "all plans hold\n", g_bad);
  return g_bad != 0;
}
