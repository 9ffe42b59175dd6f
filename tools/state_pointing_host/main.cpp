// Host build of sr_limb_jac_state_kernel's own text with its host plan (sr_limb_state.inc and sr_limb_plan.hpp, the files the
// library compiles, behind tools/host_sim/hip_on_host.hpp) for the HIDDEN column slots of the pointing derivative: level_jac_plan with n_hid = n_gas, slot g of gas g
// behind the caller's column slots, its row of dcol behind theirs, its row of jac behind the state's.  A block is 256
// threads run one after the other (no band epilogue here), exact division for the reciprocal.  Every case plans and runs
// ONE pass with the hidden slots and compares it with the pass without them -- the radiance and every state row bit for
// bit -- and, per gas, with a pass whose only parameter is one column parameter of that gas on the hidden slot's D row:
// the hidden row bit for bit; every element written (outputs start as NaN), the row sum as the device's small kernel
// forms it.  Built with AddressSanitizer and UBSan by tools/host_sim/run.sh state_pointing_host: the plan for hidden slots (block boundaries at 8 and 16
// slots, row placement) and every index the kernel forms from it, on a machine without a GPU -- not the compiled gfx950
// code.
#include "hip_on_host.hpp"
namespace sr {
#include "sr_limb_state.inc"
}
using namespace sr;

static bool same(const double *a, const double *b, size_t n) { return std::memcmp(a, b, n * sizeof(double)) == 0; }

template <int NG, bool ROWS>
static int run_case(int n_pts, int n_col, int n_lev, int n_row, int init_mode, int solo, unsigned seed) {
  std::mt19937_64 rng(seed);
  std::uniform_real_distribution<double> U(0.0, 1.0);
  const int n_layers = 6, n_rays = 3, n_levels = 5, n_tab = 4, lgas = NG - 1;
  const std::vector<int> map{0, 2, 1, 3, 3, 0};
  std::vector<int> seg_off{0}, seg_layer;
  for (int r = 0; r < n_rays; ++r) { // down to layer 2 r and up again
    for (int k = n_layers - 1; k >= 2 * r; --k) seg_layer.push_back(k);
    for (int k = 2 * r + 1; k < n_layers; ++k) seg_layer.push_back(k);
    seg_off.push_back((int)seg_layer.size());
  }
  const int n_seg = (int)seg_layer.size(), n_state = n_col + n_lev + n_row;
  auto rnd = [&](size_t n, double lo, double hi) { std::vector<double> v(n); for (auto &x : v) x = lo + (hi - lo) * U(rng); return v; };
  const size_t gs = (size_t)n_layers * n_pts;
  auto a = rnd(NG * gs, 0.0, 0.4), e = rnd(NG * gs, 0.0, 0.3), da = rnd(NG * gs, -0.02, 0.02), de = rnd(NG * gs, -0.02, 0.02);
  auto col = rnd((size_t)NG * n_seg, 0.2, 1.5);
  auto dcol = rnd((size_t)(n_col + NG) * n_seg, -1.0, 1.0); // exactly sized: the caller's rows, then the hidden ones
  auto tab = rnd((size_t)n_levels * 2 * n_tab * n_pts, 0.0, 0.3);
  std::vector<int> par_gas(n_col), par_level(n_lev);
  for (auto &g : par_gas) g = (int)(U(rng) * NG) % NG;
  for (auto &l : par_level) l = (int)(U(rng) * n_levels) % n_levels;
  std::vector<double> par_c((size_t)n_lev * n_layers), par_t((size_t)n_row * n_layers);
  for (auto &c : par_c) c = U(rng) < 0.6 ? 0.2 + U(rng) : 0.0;
  for (auto &c : par_t) c = U(rng) < 0.6 ? 0.2 + U(rng) : 0.0;
  LimbOpts o{NG, n_seg, solo, init_mode, 0, 250.0, 2975.0, 5e-4};
  const int n_pb = (n_pts + 255) / 256;
  const unsigned gx = (unsigned)((n_pb + 7) / 8 * 8) * n_rays;
  const double *pda = da.data(), *pde = de.data();

  // one pass: nc column parameters pg on the rows d of dcol, the level and row parameters or none, n_hid hidden slots
  auto pass = [&](int nc, const int *pg, const double *d, bool state, int n_hid, std::vector<double> &rad, std::vector<double> &jac) {
    const int nl = state ? n_lev : 0, nr = state ? n_row : 0, n_all = nc + nl + nr + n_hid;
    const LevelJacPlan P = level_jac_plan(nc, pg, nl, par_level.data(), par_c.data(), n_layers, nr, par_t.data(), nullptr, n_hid);
    std::vector<LevelEnt> ent = P.ent; // (exactly sized too)
    std::vector<int> slot_par = P.slot_par, blk = P.blk, ent_off = P.ent_off;
    rad.assign((size_t)n_rays * n_pts, NAN);
    jac.assign((size_t)n_rays * n_all * n_pts, NAN);
    auto go = [&](auto np) {
      constexpr int NP = decltype(np)::value;
      if (ROWS && nr > 0)
        launch(gx, P.n_blocks, [&] { sr_limb_jac_state_kernel<NG, NP, true, true, false, false, const double *, const double *>(a.data(), e.data(), n_pts, n_layers, seg_off.data(), seg_layer.data(), col.data(), d, o, n_rays, lgas, tab.data(), n_tab, map.data(), blk.data(), ent_off.data(), ent.data(), slot_par.data(), n_all, rad.data(), jac.data(), pda, pde); });
      else
        launch(gx, P.n_blocks, [&] { sr_limb_jac_state_kernel<NG, NP, true, false, false, false>(a.data(), e.data(), n_pts, n_layers, seg_off.data(), seg_layer.data(), col.data(), d, o, n_rays, lgas, tab.data(), n_tab, map.data(), blk.data(), ent_off.data(), ent.data(), slot_par.data(), n_all, rad.data(), jac.data()); });
    };
    if (level_jac_np(n_all) == 16) go(std::integral_constant<int, 16>{});
    else go(std::integral_constant<int, 8>{});
    return P.n_blocks;
  };

  std::vector<double> rad, jac, rad0, jac0, rad_g, jac_g;
  const int n_blocks = pass(n_col, par_gas.data(), dcol.data(), true, NG, rad, jac);
  int bad = 0, nonfinite = 0;
  for (double v : rad) nonfinite += !std::isfinite(v);
  for (double v : jac) nonfinite += !std::isfinite(v);
  auto row = [&](const std::vector<double> &j, int n, int ray, int p) { return &j[((size_t)ray * n + p) * n_pts]; };
  if (n_state > 0) { // the state rows and the radiance: the pass without hidden slots
    pass(n_col, par_gas.data(), dcol.data(), true, 0, rad0, jac0);
    bad += !same(rad.data(), rad0.data(), rad.size());
    for (int ray = 0; ray < n_rays; ++ray)
      for (int p = 0; p < n_state; ++p) bad += !same(row(jac, n_state + NG, ray, p), row(jac0, n_state, ray, p), n_pts);
  }
  for (int g = 0; g < NG; ++g) { // hidden row g: one column parameter of gas g on the hidden slot's D row
    pass(1, &g, dcol.data() + (size_t)(n_col + g) * n_seg, false, 0, rad_g, jac_g);
    bad += !same(rad.data(), rad_g.data(), rad.size());
    for (int ray = 0; ray < n_rays; ++ray) bad += !same(row(jac, n_state + NG, ray, n_state + g), row(jac_g, 1, ray, 0), n_pts);
  }
  // the row sum of the spectra route, in gas order, into row n_state (sr_jac_rows_sum_kernel's loop)
  for (int ray = 0; ray < n_rays; ++ray)
    for (int j = 0; j < n_pts; ++j) {
      double *r0 = &jac[((size_t)ray * (n_state + NG) + n_state) * n_pts + j];
      double v = r0[0];
      for (int g = 1; g < NG; ++g) v = v + r0[(size_t)g * n_pts];
      r0[0] = v;
      nonfinite += !std::isfinite(v);
    }
  std::printf("NG %d ROWS %d n_pts %d pars %d+%d+%d (+%d hidden) in %d block(s), init %d solo %d: rows that differ %d, non-finite %d\n", NG,
              (int)ROWS, n_pts, n_col, n_lev, n_row, NG, n_blocks, init_mode, solo, bad, nonfinite);
  return bad + nonfinite;
}

int main() {
  int bad = 0;
  bad += run_case<1, false>(300, 0, 0, 0, 0, 0, 1);      // the pointing row alone
  bad += run_case<2, false>(257, 7, 0, 0, 0, 0, 2);      // 9 column slots: past a block of 8
  bad += run_case<4, false>(300, 13, 0, 0, 2, 0, 3);     // 17 column slots: past a block of 16
  bad += run_case<2, false>(63, 3, 5, 0, 0, 1, 4);       // level slots behind the hidden ones
  bad += run_case<3, true>(300, 5, 7, 4, 2, 0, 5);       // all three kinds, the hidden slots across two blocks
  bad += run_case<4, true>(257, 14, 0, 3, 0, 0, 6);      // hidden slots split between two blocks of 16
  bad += run_case<2, true>(300, 0, 0, 6, 0, 0, 7);       // row slots and the hidden ones
  std::printf(bad ? "FAILED\n" : "all cases agree\n");
  return bad != 0;
}
