// Host build of sr_limb_jac_state_kernel's own text and of its host plan (sr_limb_state.inc and sr_limb_plan.hpp, the files the library
// compiles, behind tools/host_sim/hip_on_host.hpp with threaded lanes): a block is 256 threads, a wave's barrier a real barrier, v_mfma_f64_16x16x4 emulated in its operand layout,
// exact division for the reciprocal.  Every case runs the BANDS = false and the BANDS = true instance on the same inputs
// and reads the partial sums as sr_lowres_sum_blocks_kernel does (`part` starts as NaN: a slot that is read must have
// been written): |fused - sum_j spectrum_j W_j| <= 1e-12 of the row's largest band, exact zeros for all-zero spectra and
// the band outside the grid.  Then the INSTR = true instance with two more weight tables behind the first (further band
// tiles of Wt) and two more parameter rows per ray: its value and parameter rows must be the BANDS instance's bit for bit,
// its two instrument rows the plain sums of the radiance with tables 1 and 2 -- also for no parameter at all.  Built with AddressSanitizer and UBSan by tools/host_sim/run.sh state_bands_host: indexing, plan, tile and row mapping on a
// machine without a GPU -- not the compiled gfx950 code.
#define HOST_SIM_THREADED_LANES
#include "hip_on_host.hpp"
namespace sr {
#include "sr_limb_state.inc"
}
using namespace sr;

template <int NG, bool COLS, bool ROWS>
static int run_case(int n_pts, int n_col, int n_lev, int n_row, int n_bands, int init_mode, int solo, unsigned seed) {
  std::mt19937_64 rng(seed);
  std::uniform_real_distribution<double> U(0.0, 1.0);
  const int n_layers = 6, n_rays = 3, n_levels = 4, n_tab_rows = 3, gas = NG - 1;
  std::vector<int> seg_off{0}, seg_layer;
  for (int r = 0; r < n_rays; ++r) { // down to layer 2 r and up again
    for (int k = n_layers - 1; k >= 2 * r; --k) seg_layer.push_back(k);
    for (int k = 2 * r + 1; k < n_layers; ++k) seg_layer.push_back(k);
    seg_off.push_back((int)seg_layer.size());
  }
  const int n_seg = (int)seg_layer.size(), n_par = n_col + n_lev + n_row;
  auto rnd = [&](size_t n, double lo, double hi) { std::vector<double> v(n); for (auto &x : v) x = lo + (hi - lo) * U(rng); return v; };
  const size_t gs = (size_t)n_layers * n_pts;
  auto a = rnd(NG * gs, 0.0, 0.4), e = rnd(NG * gs, 0.0, 0.3), da = rnd(NG * gs, -0.02, 0.02), de = rnd(NG * gs, -0.02, 0.02);
  auto col = rnd((size_t)NG * n_seg, 0.2, 1.5), dcol = rnd((size_t)std::max(n_col, 1) * n_seg, 0.1, 1.0);
  auto tab = rnd((size_t)n_levels * 2 * n_tab_rows * n_pts, 0.0, 0.3);
  std::vector<int> coef_row{0, 1, 1, 2, 2, 0}, par_gas(n_col), par_level(n_lev);
  for (auto &g : par_gas) g = (int)(U(rng) * NG) % NG;
  for (auto &l : par_level) l = (int)(U(rng) * n_levels) % n_levels;
  std::vector<double> par_c((size_t)n_lev * n_layers), par_t((size_t)n_row * n_layers);
  for (auto &c : par_c) c = U(rng) < 0.6 ? 0.2 + U(rng) : 0.0;
  for (auto &c : par_t) c = U(rng) < 0.6 ? 0.2 + U(rng) : 0.0;
  if (n_lev) for (int r = 0; r < n_layers; ++r) par_c[(size_t)(n_lev - 1) * n_layers + r] = r < 2 ? 0.7 : 0.0; // layers 0, 1 only
  if (n_row) for (int r = 0; r < n_layers; ++r) par_t[(size_t)(n_row - 1) * n_layers + r] = r < 2 ? 0.5 : 0.0;
  const LevelJacPlan P = level_jac_plan(n_col, par_gas.data(), n_lev, par_level.data(), par_c.data(), n_layers, n_row, par_t.data());
  std::vector<LevelEnt> ent = P.ent;
  ent.push_back(LevelEnt{0, 0, 0.0});
  LimbOpts o{NG, n_seg, solo, init_mode, 0, 250.0, 2975.0, 5e-4};
  const int n_pb = (n_pts + 255) / 256, n_slots = 4 * n_pb, n_tiles = (n_bands + 15) / 16;
  const unsigned gx = (unsigned)((n_pb + 7) / 8 * 8) * n_rays;
  // weights: band b on [r0, r1)
  std::vector<int> range(2 * n_bands);
  std::vector<double> Wt((size_t)n_tiles * n_pts * 16, 0.0);
  for (int b = 0; b < n_bands; ++b) {
    int r0 = (int)(U(rng) * n_pts), r1 = r0 + 2 + (int)(U(rng) * (n_pts - r0));
    if (b == 0) r0 = r1 = 0;                  // outside the grid
    if (b == 1) { r0 = 0; r1 = n_pts; }       // the whole grid
    r1 = std::min(r1, n_pts);
    if (r1 - r0 < 2) r0 = r1 = 0;
    range[2 * b] = r0; range[2 * b + 1] = r1;
    for (int j = r0; j < r1; ++j) Wt[((size_t)(b >> 4) * n_pts + j) * 16 + (b & 15)] = 0.1 + U(rng);
  }
  // the instrument tables: tables 1 and 2 behind the weights, on the same ranges
  std::vector<double> Wt3((size_t)3 * n_tiles * n_pts * 16, 0.0);
  std::copy(Wt.begin(), Wt.end(), Wt3.begin());
  for (int k = 1; k < 3; ++k)
    for (int b = 0; b < n_bands; ++b)
      for (int j = range[2 * b]; j < range[2 * b + 1]; ++j) Wt3[((size_t)(k * n_tiles + (b >> 4)) * n_pts + j) * 16 + (b & 15)] = U(rng) - 0.5;
  const int n_par3 = n_par + 2;
  std::vector<double> part3((size_t)n_rays * (1 + n_par3) * n_slots * n_tiles * 16, NAN);
  const int n_rows_out = n_rays * (1 + n_par);
  std::vector<double> rad((size_t)n_rays * n_pts, NAN), jac((size_t)n_rays * n_par * n_pts, NAN);
  std::vector<double> part((size_t)n_rows_out * n_slots * n_tiles * 16, NAN);
  const double *pda = da.data(), *pde = de.data();
  const int *blk = COLS ? P.blk.data() : nullptr;
  auto go = [&](auto np) {
    constexpr int NP = decltype(np)::value;
    const FoldBands bd{Wt.data(), range.data(), part.data(), n_bands};
    const FoldBands bd3{Wt3.data(), range.data(), part3.data(), n_bands};
    if constexpr (ROWS)
      launch(gx, P.n_blocks, [&] { sr_limb_jac_state_kernel<NG, NP, COLS, true, true, true, const double *, const double *>(a.data(), e.data(), n_pts, n_layers, seg_off.data(), seg_layer.data(), col.data(), dcol.data(), o, n_rays, gas, tab.data(), n_tab_rows, coef_row.data(), blk, P.ent_off.data(), ent.data(), P.slot_par.data(), n_par3, nullptr, bd3, pda, pde); });
    else
      launch(gx, P.n_blocks, [&] { sr_limb_jac_state_kernel<NG, NP, COLS, false, true, true>(a.data(), e.data(), n_pts, n_layers, seg_off.data(), seg_layer.data(), col.data(), dcol.data(), o, n_rays, gas, tab.data(), n_tab_rows, coef_row.data(), blk, P.ent_off.data(), ent.data(), P.slot_par.data(), n_par3, nullptr, bd3); });
    if (n_par == 0) { // no parameter: there is no other instance to compare with; the radiance from the one-slot-free state call
      launch(gx, P.n_blocks, [&] { sr_limb_jac_state_kernel<NG, NP, COLS, false, false, false>(a.data(), e.data(), n_pts, n_layers, seg_off.data(), seg_layer.data(), col.data(), dcol.data(), o, n_rays, gas, tab.data(), n_tab_rows, coef_row.data(), blk, P.ent_off.data(), ent.data(), P.slot_par.data(), n_par, rad.data(), jac.data()); });
      return;
    }
    if constexpr (ROWS) {
      launch(gx, P.n_blocks, [&] { sr_limb_jac_state_kernel<NG, NP, COLS, true, false, false, const double *, const double *>(a.data(), e.data(), n_pts, n_layers, seg_off.data(), seg_layer.data(), col.data(), dcol.data(), o, n_rays, gas, tab.data(), n_tab_rows, coef_row.data(), blk, P.ent_off.data(), ent.data(), P.slot_par.data(), n_par, rad.data(), jac.data(), pda, pde); });
      launch(gx, P.n_blocks, [&] { sr_limb_jac_state_kernel<NG, NP, COLS, true, true, false, const double *, const double *>(a.data(), e.data(), n_pts, n_layers, seg_off.data(), seg_layer.data(), col.data(), dcol.data(), o, n_rays, gas, tab.data(), n_tab_rows, coef_row.data(), blk, P.ent_off.data(), ent.data(), P.slot_par.data(), n_par, nullptr, bd, pda, pde); });
    } else {
      launch(gx, P.n_blocks, [&] { sr_limb_jac_state_kernel<NG, NP, COLS, false, false, false>(a.data(), e.data(), n_pts, n_layers, seg_off.data(), seg_layer.data(), col.data(), dcol.data(), o, n_rays, gas, tab.data(), n_tab_rows, coef_row.data(), blk, P.ent_off.data(), ent.data(), P.slot_par.data(), n_par, rad.data(), jac.data()); });
      launch(gx, P.n_blocks, [&] { sr_limb_jac_state_kernel<NG, NP, COLS, false, true, false>(a.data(), e.data(), n_pts, n_layers, seg_off.data(), seg_layer.data(), col.data(), dcol.data(), o, n_rays, gas, tab.data(), n_tab_rows, coef_row.data(), blk, P.ent_off.data(), ent.data(), P.slot_par.data(), n_par, nullptr, bd); });
    }
  };
  if (level_jac_np(n_par) == 16) go(std::integral_constant<int, 16>{});
  else go(std::integral_constant<int, 8>{});
  // the sum kernel's reading of `part`, and the plain band sums of the hi-res spectra
  int bad = 0, zeros = 0, nonfinite = 0;
  double worst = 0.0;
  for (int ray = 0; ray < (n_par > 0 ? n_rays : 0); ++ray) // (no parameter: only the INSTR instance ran)
    for (int q = 0; q <= n_par; ++q) {
      const size_t row = q == 0 ? (size_t)ray : (size_t)n_rays + (size_t)ray * n_par + (q - 1);
      const double *sp = q == 0 ? &rad[(size_t)ray * n_pts] : &jac[((size_t)ray * n_par + (q - 1)) * n_pts];
      double scale = 0.0;
      std::vector<double> f(n_bands), u(n_bands);
      bool all_zero = true;
      for (int j = 0; j < n_pts; ++j) all_zero = all_zero && sp[j] == 0.0;
      for (int b = 0; b < n_bands; ++b) {
        const int r0 = range[2 * b], r1 = range[2 * b + 1], tile = b >> 4, c16 = b & 15;
        double v = 0.0, w = 0.0;
        if (r1 > r0)
          for (int c = r0 >> 6; c <= (r1 - 1) >> 6; ++c) v += part[((row * n_slots + c) * n_tiles + tile) * 16 + c16];
        for (int j = 0; j < n_pts; ++j) w = std::fma(sp[j], Wt[((size_t)tile * n_pts + j) * 16 + c16], w);
        f[b] = v; u[b] = w;
        scale = std::max(scale, std::fabs(w));
        if (!std::isfinite(v)) ++nonfinite;
      }
      for (int b = 0; b < n_bands; ++b) {
        if (all_zero) { if (f[b] != 0.0) ++bad; else ++zeros; continue; }
        const double d = std::fabs(f[b] - u[b]) / (scale > 0 ? scale : 1.0);
        worst = std::max(worst, d);
        if (!(d <= 1e-12)) ++bad;
        if ((b == 0) && f[b] != 0.0) ++bad;
      }
    }
  // the INSTR instance: value and parameter rows bit for bit, the two instrument rows against plain sums of the radiance
  int bad3 = 0;
  double worst3 = 0.0;
  for (int ray = 0; ray < n_rays; ++ray)
    for (int q = 0; q <= n_par3; ++q) {
      const size_t row3 = q == 0 ? (size_t)ray : (size_t)n_rays + (size_t)ray * n_par3 + (q - 1);
      const size_t row = q == 0 ? (size_t)ray : (size_t)n_rays + (size_t)ray * n_par + (q - 1);
      const int k = q - n_par; // 1, 2: the instrument rows
      const double *sp = &rad[(size_t)ray * n_pts];
      double scale = 0.0;
      std::vector<double> f(n_bands), u(n_bands);
      for (int b = 0; b < n_bands; ++b) {
        const int r0 = range[2 * b], r1 = range[2 * b + 1], tile = b >> 4, c16 = b & 15;
        double v = 0.0, w = 0.0;
        if (r1 > r0)
          for (int c = r0 >> 6; c <= (r1 - 1) >> 6; ++c) {
            const double x = part3[((row3 * n_slots + c) * n_tiles + tile) * 16 + c16];
            v += x;
            if (k <= 0 && n_par > 0 && std::memcmp(&x, &part[((row * n_slots + c) * n_tiles + tile) * 16 + c16], sizeof x) != 0) ++bad3;
          }
        if (k > 0 || n_par == 0)
          for (int j = 0; j < n_pts; ++j) w = std::fma(sp[j], Wt3[((size_t)(std::max(k, 0) * n_tiles + tile) * n_pts + j) * 16 + c16], w);
        f[b] = v; u[b] = w;
        scale = std::max(scale, std::fabs(w));
        if (!std::isfinite(v)) ++nonfinite;
      }
      if (k > 0 || n_par == 0)
        for (int b = 0; b < n_bands; ++b) {
          const double d = std::fabs(f[b] - u[b]) / (scale > 0 ? scale : 1.0);
          worst3 = std::max(worst3, d);
          if (!(d <= 1e-12) || (b == 0 && f[b] != 0.0) || (b == 1 && f[b] == 0.0 && solo == 0)) ++bad3;
        }
    }
  std::printf("  with the instrument rows: worst %.2e, bad %d\n", worst3, bad3);
  bad += bad3;
  std::printf("NG %d COLS %d ROWS %d n_pts %d pars %d+%d+%d bands %d init %d solo %d: worst %.2e, exact-zero entries %d, non-finite %d, bad %d\n",
              NG, (int)COLS, (int)ROWS, n_pts, n_col, n_lev, n_row, n_bands, init_mode, solo, worst, zeros, nonfinite, bad);
  return bad + nonfinite;
}

int main() {
  int bad = 0;
  bad += run_case<1, true, false>(63, 3, 0, 0, 7, 0, 0, 1);
  bad += run_case<2, false, false>(257, 0, 5, 0, 7, 0, 0, 2);
  bad += run_case<2, false, true>(300, 0, 0, 4, 7, 2, 0, 3);
  bad += run_case<1, false, false>(257, 0, 8, 0, 7, 0, 0, 4);
  bad += run_case<2, false, false>(300, 0, 16, 0, 37, 0, 0, 5);
  bad += run_case<1, false, false>(257, 0, 17, 0, 7, 2, 1, 6);
  bad += run_case<2, true, true>(300, 5, 12, 3, 37, 0, 0, 7);
  bad += run_case<3, true, true>(700, 5, 12, 3, 20, 2, 0, 8);
  bad += run_case<1, false, false>(257, 0, 0, 0, 20, 0, 0, 9);   // no parameter: the radiance and the instrument rows alone
  std::printf(bad ? "FAILED\n" : "all cases agree\n");
  return bad != 0;
}
