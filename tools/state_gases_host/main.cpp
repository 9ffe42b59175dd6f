// Host build of sr_limb_jac_state_kernel's own text with its host plan (sr_limb_state.inc and sr_limb_plan.hpp, the files the
// library compiles, behind tools/host_sim/hip_on_host.hpp) for the instances that take the level parameters of SEVERAL level-factored gases: a block is 256 threads
// run one after the other (no band epilogue here, so no barrier is needed), exact division for the reciprocal.  Every case
// plans and runs ONE pass for two or three level gases -- tables of different levels and rows, row maps of their own,
// the level parameters interleaved in the caller's order -- and, per level gas, the one-gas instance on the same inputs:
// the level rows of gas k must be bit for bit those of its own pass, the column and row rows and the radiances bit for
// bit those of every pass, every element written (outputs start as NaN).  Built with AddressSanitizer and UBSan by
// tools/host_sim/run.sh state_gases_host: the plan for mixed blocks and every index the kernel forms from it, on a machine without a GPU -- not the
// compiled gfx950 code.
#include "hip_on_host.hpp"
namespace sr {
#include "sr_limb_state.inc"
}
using namespace sr;

static bool same(const double *a, const double *b, size_t n) { return std::memcmp(a, b, n * sizeof(double)) == 0; }

template <int NG, bool COLS, bool ROWS>
static int run_case(int n_pts, int n_col, std::vector<int> levs, int n_row, int init_mode, int solo, unsigned seed) {
  std::mt19937_64 rng(seed);
  std::uniform_real_distribution<double> U(0.0, 1.0);
  const int n_layers = 6, n_rays = 3, n_lgas = (int)levs.size();
  const int n_levels[3] = {12, 5, 3}, n_tab[3] = {4, 7, 5}, lgas_gas[3] = {NG - 1, 0, 1};
  const std::vector<int> maps[3] = {{0, 2, 1, 3, 3, 0}, {6, 0, 4, 4, 2, 5}, {1, 1, 0, 4, 3, 2}};
  std::vector<int> seg_off{0}, seg_layer;
  for (int r = 0; r < n_rays; ++r) { // down to layer 2 r and up again
    for (int k = n_layers - 1; k >= 2 * r; --k) seg_layer.push_back(k);
    for (int k = 2 * r + 1; k < n_layers; ++k) seg_layer.push_back(k);
    seg_off.push_back((int)seg_layer.size());
  }
  const int n_seg = (int)seg_layer.size(), n_lev = std::accumulate(levs.begin(), levs.end(), 0), n_par = n_col + n_lev + n_row;
  auto rnd = [&](size_t n, double lo, double hi) { std::vector<double> v(n); for (auto &x : v) x = lo + (hi - lo) * U(rng); return v; };
  const size_t gs = (size_t)n_layers * n_pts;
  auto a = rnd(NG * gs, 0.0, 0.4), e = rnd(NG * gs, 0.0, 0.3), da = rnd(NG * gs, -0.02, 0.02), de = rnd(NG * gs, -0.02, 0.02);
  auto col = rnd((size_t)NG * n_seg, 0.2, 1.5), dcol = rnd((size_t)std::max(n_col, 1) * n_seg, 0.1, 1.0);
  std::vector<std::vector<double>> tabs;
  for (int k = 0; k < n_lgas; ++k) tabs.push_back(rnd((size_t)n_levels[k] * 2 * n_tab[k] * n_pts, 0.0, 0.3)); // exactly sized: a wrong row or level is out of bounds
  std::vector<int> par_gas(n_col), par_lgas, par_level(n_lev);
  for (auto &g : par_gas) g = (int)(U(rng) * NG) % NG;
  for (int k = 0; k < n_lgas; ++k) par_lgas.insert(par_lgas.end(), levs[k], k);
  std::shuffle(par_lgas.begin(), par_lgas.end(), rng);
  for (int p = 0; p < n_lev; ++p) par_level[p] = (int)(U(rng) * n_levels[par_lgas[p]]) % n_levels[par_lgas[p]];
  for (int k = 0; k < n_lgas; ++k) // the highest and the lowest level of every gas occur
    for (int p = 0, seen = 0; p < n_lev && seen < 2; ++p)
      if (par_lgas[p] == k) par_level[p] = seen++ ? 0 : n_levels[k] - 1;
  std::vector<double> par_c((size_t)n_lev * n_layers), par_t((size_t)n_row * n_layers);
  for (auto &c : par_c) c = U(rng) < 0.6 ? 0.2 + U(rng) : 0.0;
  for (auto &c : par_t) c = U(rng) < 0.6 ? 0.2 + U(rng) : 0.0;
  LimbOpts o{NG, n_seg, solo, init_mode, 0, 250.0, 2975.0, 5e-4};
  const int n_pb = (n_pts + 255) / 256;
  const unsigned gx = (unsigned)((n_pb + 7) / 8 * 8) * n_rays;
  const double *pda = da.data(), *pde = de.data();

  // one pass with the level parameters `idx` (all of them: several gases; those of gas k: the one-gas instance)
  auto pass = [&](int k_only, std::vector<double> &rad, std::vector<double> &jac, std::vector<int> &idx) {
    idx.clear();
    for (int p = 0; p < n_lev; ++p)
      if (k_only < 0 || par_lgas[p] == k_only) idx.push_back(p);
    const int nl = (int)idx.size(), np_all = n_col + nl + n_row;
    std::vector<int> lev(nl), lg(nl);
    std::vector<double> c((size_t)nl * n_layers);
    for (int i = 0; i < nl; ++i) {
      lev[i] = par_level[idx[i]];
      lg[i] = par_lgas[idx[i]];
      std::copy_n(&par_c[(size_t)idx[i] * n_layers], n_layers, &c[(size_t)i * n_layers]);
    }
    const LevelJacPlan P = level_jac_plan(n_col, par_gas.data(), nl, lev.data(), c.data(), n_layers, n_row, par_t.data(),
                                          k_only < 0 ? lg.data() : nullptr);
    std::vector<LevelEnt> ent = P.ent; // (exactly sized too)
    rad.assign((size_t)n_rays * n_pts, NAN);
    jac.assign((size_t)n_rays * np_all * n_pts, NAN);
    const int *blk = COLS ? P.blk.data() : nullptr;
    std::vector<int> rows;
    LevelGasTabs T{};
    if (k_only < 0) {
      for (int k = 0; k < n_lgas; ++k) {
        rows.insert(rows.end(), maps[k].begin(), maps[k].end());
        T.tab[k] = tabs[k].data(); T.n_tab_rows[k] = n_tab[k]; T.gas[k] = lgas_gas[k];
      }
    } else {
      rows = maps[k_only];
    }
    auto go = [&](auto np) {
      constexpr int NP = decltype(np)::value;
      if (k_only < 0) {
        if constexpr (ROWS)
          launch(gx, P.n_blocks, [&] { sr_limb_jac_state_kernel<NG, NP, COLS, true, false, false, const double *, const double *, LevelGasTabs>(a.data(), e.data(), n_pts, n_layers, seg_off.data(), seg_layer.data(), col.data(), dcol.data(), o, n_rays, -1, nullptr, 0, rows.data(), blk, P.ent_off.data(), ent.data(), P.slot_par.data(), np_all, rad.data(), jac.data(), pda, pde, T); });
        else
          launch(gx, P.n_blocks, [&] { sr_limb_jac_state_kernel<NG, NP, COLS, false, false, false, LevelGasTabs>(a.data(), e.data(), n_pts, n_layers, seg_off.data(), seg_layer.data(), col.data(), dcol.data(), o, n_rays, -1, nullptr, 0, rows.data(), blk, P.ent_off.data(), ent.data(), P.slot_par.data(), np_all, rad.data(), jac.data(), T); });
      } else {
        const int k = k_only;
        if constexpr (ROWS)
          launch(gx, P.n_blocks, [&] { sr_limb_jac_state_kernel<NG, NP, COLS, true, false, false, const double *, const double *>(a.data(), e.data(), n_pts, n_layers, seg_off.data(), seg_layer.data(), col.data(), dcol.data(), o, n_rays, lgas_gas[k], tabs[k].data(), n_tab[k], rows.data(), blk, P.ent_off.data(), ent.data(), P.slot_par.data(), np_all, rad.data(), jac.data(), pda, pde); });
        else
          launch(gx, P.n_blocks, [&] { sr_limb_jac_state_kernel<NG, NP, COLS, false, false, false>(a.data(), e.data(), n_pts, n_layers, seg_off.data(), seg_layer.data(), col.data(), dcol.data(), o, n_rays, lgas_gas[k], tabs[k].data(), n_tab[k], rows.data(), blk, P.ent_off.data(), ent.data(), P.slot_par.data(), np_all, rad.data(), jac.data()); });
      }
    };
    if (level_jac_np(np_all) == 16) go(std::integral_constant<int, 16>{});
    else go(std::integral_constant<int, 8>{});
    return P.n_blocks;
  };

  std::vector<double> rad, jac, rad_k, jac_k;
  std::vector<int> all, idx;
  const int n_blocks = pass(-1, rad, jac, all);
  int bad = 0, nonfinite = 0;
  for (double v : rad) nonfinite += !std::isfinite(v);
  for (double v : jac) nonfinite += !std::isfinite(v);
  for (int k = 0; k < n_lgas; ++k) {
    pass(k, rad_k, jac_k, idx);
    const int nl = (int)idx.size(), npk = n_col + nl + n_row;
    bad += !same(rad.data(), rad_k.data(), rad.size());
    for (int ray = 0; ray < n_rays; ++ray) {
      auto row = [&](const std::vector<double> &j, int n, int p) { return &j[((size_t)ray * n + p) * n_pts]; };
      for (int p = 0; p < n_col; ++p) bad += !same(row(jac, n_par, p), row(jac_k, npk, p), n_pts);
      for (int i = 0; i < nl; ++i) bad += !same(row(jac, n_par, n_col + idx[i]), row(jac_k, npk, n_col + i), n_pts);
      for (int p = 0; p < n_row; ++p) bad += !same(row(jac, n_par, n_col + n_lev + p), row(jac_k, npk, n_col + nl + p), n_pts);
    }
  }
  std::printf("NG %d COLS %d ROWS %d n_pts %d pars %d+(", NG, (int)COLS, (int)ROWS, n_pts, n_col);
  for (int k = 0; k < n_lgas; ++k) std::printf("%s%d", k ? "+" : "", levs[k]);
  std::printf(")+%d in %d block(s), init %d solo %d: rows that differ from the one-gas passes %d, non-finite %d\n", n_row, n_blocks,
              init_mode, solo, bad, nonfinite);
  return bad + nonfinite;
}

int main() {
  int bad = 0;
  bad += run_case<2, false, false>(300, 0, {3, 2}, 0, 0, 0, 1);      // eight slots
  bad += run_case<2, true, false>(257, 3, {4, 4}, 0, 0, 0, 2);       // sixteen slots, column slots in front
  bad += run_case<3, true, true>(300, 5, {7, 5}, 4, 2, 0, 3);        // two blocks, level slots of both gases in both
  bad += run_case<2, false, false>(63, 0, {9, 8}, 0, 0, 1, 4);       // two blocks of level slots alone
  bad += run_case<3, false, false>(300, 0, {2, 2, 1}, 0, 0, 0, 5);   // three level gases
  bad += run_case<4, true, true>(257, 5, {5, 4, 3}, 4, 2, 0, 6);
  bad += run_case<4, false, true>(300, 0, {6, 3}, 3, 0, 0, 7);       // row slots, no column code
  std::printf(bad ? "FAILED\n" : "all cases agree\n");
  return bad != 0;
}
