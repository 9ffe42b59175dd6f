// Host build of sr_limb_jac_state_kernel's own text with its two host plans (sr_limb_state.inc and sr_limb_plan.hpp, the files
// the library compiles, behind tools/host_sim/hip_on_host.hpp) for the instances with the parameter blocks PER RAY
// (sr_set_state_ray_blocks): a block is 256 threads run one after the other (spectra only: no band epilogue, no barrier),
// exact division for the reciprocal.  Every case draws a limb batch -- six rays of different tangent rows on twelve
// coefficient rows, or a coefficient row per LOS step -- and column, level and row parameters that each touch a few rays,
// plans it densely (level_jac_plan) and per ray (ray_jac_plan), and runs both instances: the dense one into a buffer of NaN
// (it writes every element), the per-ray one into a buffer of zeros (the host clears it ahead of the launch).  The two must
// agree bit for bit -- the slots' arithmetic is the same text --, a row of a parameter that does not touch the ray must be
// an exact zero in both, and both are held to a plain loop per (ray, parameter) written from the header's formulas
// (std::exp, IEEE division) within 1e-10 of the row's largest value.  Built with AddressSanitizer and UBSan by
// tools/host_sim/run.sh state_rayblocks_host: the plan and every index the kernel forms from it (ray_blk_off, col_row, the
// entry lists of a ray block, exactly sized arrays) on a machine without a GPU -- not the compiled gfx950 code.
#include "hip_on_host.hpp"
namespace sr {
#include "sr_limb_state.inc"
}
using namespace sr;

struct Case {
  int n_pts, n_layers, n_col, n_lev, n_row, n_lgas, n_hid;
  bool step_rows, observer, small;
  int init_mode, solo;
  unsigned seed;
};

template <int NG, bool COLS, bool ROWS, bool SEVERAL>
static int run_case(const Case &cs) {
  std::mt19937_64 rng(cs.seed);
  std::uniform_real_distribution<double> U(0.0, 1.0);
  const int n_pts = cs.n_pts, n_col = cs.n_col, n_lev = cs.n_lev, n_row = cs.n_row, n_hid = cs.n_hid;
  std::vector<int> seg_off{0}, seg_layer;
  int n_layers = cs.n_layers;
  if (cs.step_rows) {
    for (int m : {5, 9, 7}) {
      for (int i = 0; i < m; ++i) seg_layer.push_back((int)seg_layer.size());
      seg_off.push_back((int)seg_layer.size());
    }
    n_layers = (int)seg_layer.size();
  } else {
    for (int t : {n_layers - 1, 2, 0, n_layers - 3, 5, 7}) {
      for (int k = n_layers - 1; k >= t; --k) seg_layer.push_back(k);
      for (int k = t + 1; k < n_layers; ++k) seg_layer.push_back(k);
      seg_off.push_back((int)seg_layer.size());
    }
  }
  const int n_rays = (int)seg_off.size() - 1, n_seg = (int)seg_layer.size(), n_state = n_col + n_lev + n_row, n_par = n_state + n_hid;
  std::vector<int> pt_off(n_seg + 1);
  for (int s = 0; s <= n_seg; ++s) pt_off[s] = 2 * s;
  const int n_pt = 2 * n_seg;
  auto rnd = [&](size_t n, double lo, double hi) { std::vector<double> v(n); for (auto &x : v) x = lo + (hi - lo) * U(rng); return v; };
  const size_t gs = (size_t)n_layers * n_pts;
  auto a = rnd(NG * gs, 0.01, 0.3), e = rnd(NG * gs, 0.0, 0.3), da = rnd(NG * gs, -0.02, 0.02), de = rnd(NG * gs, -0.02, 0.02);
  auto col = rnd((size_t)NG * n_seg, 0.2, 1.5);
  const int n_levels[2] = {5, 3}, n_tab[2] = {n_layers + 1, n_layers}, lgas_gas[2] = {NG - 1, 0};
  std::vector<std::vector<double>> tabs;
  std::vector<std::vector<int>> maps;
  for (int k = 0; k < cs.n_lgas; ++k) {
    tabs.push_back(rnd((size_t)n_levels[k] * 2 * n_tab[k] * n_pts, 0.0, 0.3)); // exactly sized: a wrong row or level is out of bounds
    std::vector<int> m(n_layers);
    for (auto &r : m) r = (int)(U(rng) * n_tab[k]) % n_tab[k];
    maps.push_back(m);
  }
  // parameters that touch a few rays each: a column parameter weights the sample points of one or two rays (some of none),
  // a level or row parameter a few coefficient rows
  const double keep = cs.small ? 0.12 : 0.3;
  std::vector<int> par_gas(n_col), par_lgas(n_lev), par_level(n_lev);
  std::vector<double> par_w((size_t)std::max(n_col, 1) * n_pt, 0.0), par_c((size_t)n_lev * n_layers, 0.0), par_t((size_t)n_row * n_layers, 0.0);
  for (int p = 0; p < n_col; ++p) {
    par_gas[p] = (int)(U(rng) * NG) % NG;
    for (int ray = 0; ray < n_rays; ++ray)
      if (ray > 0 && U(rng) < keep)
        for (int i = pt_off[seg_off[ray]]; i < pt_off[seg_off[ray + 1]]; ++i) par_w[(size_t)p * n_pt + i] = U(rng) < 0.6 ? 0.2 + U(rng) : 0.0;
  }
  for (int p = 0; p < n_lev; ++p) {
    par_lgas[p] = p % cs.n_lgas;
    par_level[p] = (int)(U(rng) * n_levels[par_lgas[p]]) % n_levels[par_lgas[p]];
  }
  auto few_rows = [&](std::vector<double> &w, int n) {
    for (int p = 0; p < n; ++p) {
      const int r0 = (int)(U(rng) * (n_layers - 1)) % (n_layers - 1); // (never the top row: ray 0 of the limb batch sees it alone)
      for (int r = std::max(0, r0 - 2); r <= r0; ++r) w[(size_t)p * n_layers + r] = U(rng) < 0.7 ? (U(rng) < 0.5 ? -1.0 : 1.0) * (0.2 + U(rng)) : 0.0;
    }
  };
  few_rows(par_c, n_lev);
  few_rows(par_t, n_row);
  // d col / d x_p: linear in the weights (any linear map serves the index check); the hidden slots' rows behind them
  std::vector<double> dcol((size_t)std::max(n_col + n_hid, 1) * n_seg, 0.0);
  for (int p = 0; p < n_col; ++p)
    for (int s = 0; s < n_seg; ++s) dcol[(size_t)p * n_seg + s] = 0.5 * (par_w[(size_t)p * n_pt + 2 * s] + par_w[(size_t)p * n_pt + 2 * s + 1]);
  for (int g = 0; g < n_hid; ++g)
    for (int s = 0; s < n_seg; ++s) dcol[(size_t)(n_col + g) * n_seg + s] = 0.1 + U(rng);
  // the kernel walks seg_layer / col as staged: observer order re-lists them reversed per ray; the plans see the caller's
  std::vector<int> walk_layer = seg_layer;
  if (cs.observer)
    for (int r = 0; r < n_rays; ++r) std::reverse(walk_layer.begin() + seg_off[r], walk_layer.begin() + seg_off[r + 1]);
  sr_los_desc los{};
  los.n_rays = n_rays, los.n_gas = NG, los.seg_off = seg_off.data(), los.seg_layer = seg_layer.data(), los.pt_off = pt_off.data();
  los.los_order = cs.observer ? 1 : 0;
  LimbOpts o{NG, n_seg, cs.solo, cs.init_mode, 0, 250.0, 2975.0, 5e-4};
  const int n_pb = (n_pts + 255) / 256;
  const unsigned gx = (unsigned)((n_pb + 7) / 8 * 8) * n_rays;
  const double *pda = da.data(), *pde = de.data();
  const int32_t *lg = SEVERAL ? par_lgas.data() : nullptr;
  LevelGasTabs T{};
  std::vector<int> rows;
  for (int k = 0; k < cs.n_lgas; ++k) {
    rows.insert(rows.end(), maps[k].begin(), maps[k].end());
    T.tab[k] = tabs[k].data(); T.n_tab_rows[k] = n_tab[k]; T.gas[k] = lgas_gas[k];
  }
  const int gas = SEVERAL ? -1 : lgas_gas[0], ntr = SEVERAL ? 0 : n_tab[0];
  const double *tab = SEVERAL ? nullptr : tabs[0].data();

  auto pass = [&](bool per_ray, std::vector<double> &rad, std::vector<double> &jac, int *walks) {
    LevelJacPlan P{};
    RayJacPlan Rp{};
    if (per_ray) {
      Rp = ray_jac_plan(&los, n_col, par_gas.data(), par_w.data(), n_lev, par_level.data(), par_c.data(), n_layers, n_row, par_t.data(), lg, n_hid);
      P.n_blocks = Rp.n_blocks;
      P.blk = Rp.blk, P.ent_off = Rp.ent_off, P.slot_par = Rp.slot_par, P.ent = Rp.ent;
      *walks = Rp.ray_blk_off.back();
    } else {
      P = level_jac_plan(n_col, par_gas.data(), n_lev, par_level.data(), par_c.data(), n_layers, n_row, par_t.data(), lg, n_hid);
      *walks = n_rays * P.n_blocks;
    }
    std::vector<LevelEnt> ent = P.ent; // (exactly sized)
    rad.assign((size_t)n_rays * n_pts, NAN);
    jac.assign((size_t)n_rays * n_par * n_pts, per_ray ? 0.0 : NAN);
    const int *blk = COLS ? P.blk.data() : nullptr;
    const StateRayBlocks rbk{Rp.ray_blk_off.data(), Rp.col_row.data()};
    const int np_plan = per_ray ? Rp.np : level_jac_np(n_par);
    auto go = [&](auto np, auto rb) {
      constexpr int NP = decltype(np)::value;
      constexpr bool RB = decltype(rb)::value;
      auto call = [&](auto... pack) {
        launch(gx, P.n_blocks, [&] {
          sr_limb_jac_state_kernel<NG, NP, COLS, ROWS, false, false, decltype(pack)...>(
              a.data(), e.data(), n_pts, n_layers, seg_off.data(), walk_layer.data(), col.data(), dcol.data(), o, n_rays, gas, tab, ntr,
              rows.data(), blk, P.ent_off.data(), ent.data(), P.slot_par.data(), n_par, rad.data(), jac.data(), pack...);
        });
      };
      auto with_rb = [&](auto... pack) {
        if constexpr (RB) call(pack..., rbk);
        else call(pack...);
      };
      if constexpr (ROWS && SEVERAL) with_rb(pda, pde, T);
      else if constexpr (ROWS) with_rb(pda, pde);
      else if constexpr (SEVERAL) with_rb(T);
      else with_rb();
    };
    auto by_np = [&](auto rb) {
      if (np_plan == 16) go(std::integral_constant<int, 16>{}, rb);
      else go(std::integral_constant<int, 8>{}, rb);
    };
    if (per_ray) by_np(std::true_type{});
    else by_np(std::false_type{});
    return np_plan;
  };

  std::vector<double> rad_d, jac_d, rad_r, jac_r;
  int walks_d = 0, walks_r = 0;
  pass(false, rad_d, jac_d, &walks_d);
  const int np_r = pass(true, rad_r, jac_r, &walks_r);
  int bad = 0, nonfinite = 0, nonzero = 0;
  double worst = 0.0;
  for (double v : rad_r) nonfinite += !std::isfinite(v);
  for (double v : jac_r) nonfinite += !std::isfinite(v);
  for (double v : jac_d) nonfinite += !std::isfinite(v);
  bad += std::memcmp(rad_d.data(), rad_r.data(), rad_d.size() * sizeof(double)) != 0;
  bad += std::memcmp(jac_d.data(), jac_r.data(), jac_d.size() * sizeof(double)) != 0;
  // the plain loop, ray by ray and parameter by parameter
  for (int ray = 0; ray < n_rays; ++ray) {
    const int s0 = seg_off[ray], s1 = seg_off[ray + 1];
    for (int p = 0; p < n_par; ++p) {
      bool touched = p >= n_state;
      for (int s = s0; s < s1 && !touched; ++s) {
        const int r = seg_layer[s];
        if (p < n_col) touched = par_w[(size_t)p * n_pt + 2 * s] != 0.0 || par_w[(size_t)p * n_pt + 2 * s + 1] != 0.0;
        else if (p < n_col + n_lev) touched = par_c[(size_t)(p - n_col) * n_layers + r] != 0.0;
        else touched = par_t[(size_t)(p - n_col - n_lev) * n_layers + r] != 0.0;
      }
      std::vector<double> ref(n_pts);
      double big = 0.0;
      for (int j = 0; j < n_pts; ++j) {
        double I = limb_initial(o, nullptr, 0, j), J = 0.0;
        for (int s = s0; s < s1; ++s) {
          const int r = walk_layer[s];
          double tau = 0.0, E = 0.0, dtau = 0.0, dE = 0.0;
          for (int g = 0; g < NG; ++g) {
            const double u = col[(size_t)g * n_seg + s];
            tau += a[g * gs + (size_t)r * n_pts + j] * u;
            E += e[g * gs + (size_t)r * n_pts + j] * u;
          }
          if (p < n_col || p >= n_state) {
            const int g = p < n_col ? par_gas[p] : p - n_state;
            const double D = dcol[(size_t)(p < n_col ? p : n_col + (p - n_state)) * n_seg + s];
            dtau = a[g * gs + (size_t)r * n_pts + j] * D, dE = e[g * gs + (size_t)r * n_pts + j] * D;
          } else if (p < n_col + n_lev) {
            const int q = p - n_col, k = par_lgas[q];
            const size_t pl = (size_t)n_tab[k] * n_pts;
            const double *tl = tabs[k].data() + (size_t)par_level[q] * 2 * pl + (size_t)maps[k][r] * n_pts + j;
            const double w = par_c[(size_t)q * n_layers + r] * col[(size_t)lgas_gas[k] * n_seg + s];
            dtau = w * tl[0], dE = w * tl[pl];
          } else {
            const double w = par_t[(size_t)(p - n_col - n_lev) * n_layers + r];
            for (int g = 0; g < NG; ++g) {
              const double u = col[(size_t)g * n_seg + s];
              dtau += w * u * da[g * gs + (size_t)r * n_pts + j], dE += w * u * de[g * gs + (size_t)r * n_pts + j];
            }
          }
          const double t = std::exp(-tau), f = -std::expm1(-tau) / tau, fp = (tau * t + std::expm1(-tau)) / (tau * tau);
          J = J * t + (-I * t * dtau + (cs.solo ? 0.0 : dE * f + E * fp * dtau));
          I = I * t + (cs.solo ? 0.0 : E * f);
        }
        ref[j] = J;
        big = std::max(big, std::fabs(J));
        if (p == 0) worst = std::max(worst, std::fabs(rad_r[(size_t)ray * n_pts + j] - I) / std::max(std::fabs(I), 1e-300));
      }
      for (int j = 0; j < n_pts; ++j) {
        const double got = jac_r[((size_t)ray * n_par + p) * n_pts + j];
        if (!touched) nonzero += got != 0.0 || jac_d[((size_t)ray * n_par + p) * n_pts + j] != 0.0;
        else if (big > 0.0) worst = std::max(worst, std::fabs(got - ref[j]) / big);
      }
    }
  }
  const bool fewer = cs.small || walks_r < walks_d;
  std::printf("NG %d COLS %d ROWS %d gases %d n_pts %d rows %d pars %d+%d+%d(+%d) init %d solo %d observer %d: NP %d, walks %d (dense %d), "
              "dense vs per ray differ %d, non-finite %d, untouched rows not zero %d, against the plain loop %.2e\n",
              NG, (int)COLS, (int)ROWS, cs.n_lgas, n_pts, n_layers, n_col, n_lev, n_row, n_hid, cs.init_mode, cs.solo, (int)cs.observer, np_r,
              walks_r, walks_d, bad, nonfinite, nonzero, worst);
  return bad + nonfinite + nonzero + !(worst < 1e-10) + !fewer + (cs.small && np_r != 8);
}

int main() {
  int bad = 0;
  //                                   pts lay col lev row lgas hid step   obs    small init solo seed
  bad += run_case<3, true, false, false>({300, 12, 37, 0, 0, 1, 0, false, false, false, 0, 0, 1});   // columns only, three dense blocks
  bad += run_case<3, true, false, false>({300, 12, 27, 10, 0, 1, 0, false, false, false, 0, 0, 2});  // columns + levels
  bad += run_case<3, true, true, false>({300, 12, 21, 10, 6, 1, 0, false, false, false, 2, 0, 3});   // all kinds, Planck background
  bad += run_case<3, true, true, true>({257, 12, 21, 10, 6, 2, 0, false, false, false, 0, 0, 4});    // two level gases
  bad += run_case<3, true, true, true>({300, 12, 18, 10, 6, 2, 3, false, false, false, 0, 0, 5});    // hidden pointing slots on every ray
  bad += run_case<3, false, true, false>({300, 12, 0, 14, 9, 1, 0, false, false, false, 2, 1, 6});   // no column code, solo absorption
  bad += run_case<3, true, true, false>({300, 12, 21, 10, 6, 1, 0, false, true, false, 0, 0, 7});    // observer order
  bad += run_case<3, true, true, false>({300, 21, 9, 10, 6, 1, 0, true, false, false, 0, 0, 8});     // a coefficient row per LOS step
  bad += run_case<3, true, true, false>({300, 12, 5, 3, 2, 1, 0, false, false, true, 0, 0, 9});      // few touches: the eight-slot instances
  bad += run_case<1, true, false, false>({63, 12, 20, 6, 0, 1, 0, false, false, false, 0, 0, 10});   // one gas, less than a wave
  std::printf(bad ? "FAILED\n" : "all cases agree\n");
  return bad != 0;
}
