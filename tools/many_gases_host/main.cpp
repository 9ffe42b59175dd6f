// Host build of the kernel text that runs batches of five to eight gases -- sr_limb_kernel, sr_limb_split_kernel
// (sr_limb_forward.inc) and sr_limb_jac_state_kernel (sr_limb_state.inc) with its host plans (sr_limb_plan.hpp, three bits
// per column slot), the files the library compiles, behind tools/host_sim/hip_on_host.hpp with threaded lanes: a block is
// 256 threads, a block's and a wave's barrier real barriers, v_mfma_f64_16x16x4 emulated in its operand layout, exact
// division for the reciprocal.  3 rays, 12 layers, 65 points.  Every case is checked against PLAIN LOOPS over the same
// plan's parameters -- the definitions, one (ray, point, parameter) at a time: 1e-12 of a row's largest value, every
// element written (outputs start as NaN).  Cases: sr_limb_kernel<8>, sr_limb_split_kernel<5>; the state kernel
// <8, 8, COLS, ROWS> with column slots on gases 0, 4, 7, 5, 3, a level gas with index 6 and row slots, its BANDS instance
// against the band sums of those spectra; two level gases (5 and 2); parameter blocks per ray; and the PADDED launches -- a
// batch of seven gases on the eight-gas instance, of five on the six-gas one -- against the instances of exactly seven and
// five gases (compiled here only), which must agree in every value (==: a padding slot adds exact zeros); and the words
// of the dense plan and of the plan per ray with eight hidden slots, decoded.  Built with
// AddressSanitizer and UBSan by tools/host_sim/run.sh many_gases_host -- indexing, plans, gas words, tile and row mapping
// on a machine without a GPU, not the compiled gfx950 code.
#define HOST_SIM_THREADED_LANES
#include "hip_on_host.hpp"
static pthread_barrier_t g_block_bar;
static void block_barrier() { pthread_barrier_wait(&g_block_bar); }
#define __syncthreads block_barrier
namespace sr {
#include "sr_limb_forward.inc"
#include "sr_limb_state.inc"
}
using namespace sr;

struct Batch {
  int n_gas, n_pts, n_layers = 12, n_rays = 3, n_seg;
  std::vector<int> seg_off{0}, seg_layer;
  std::vector<double> a, e, da, de, col;
  LimbOpts o;
  unsigned gx;
};
static std::vector<double> rnd(std::mt19937_64 &rng, size_t n, double lo, double hi) {
  std::uniform_real_distribution<double> U(lo, hi);
  std::vector<double> v(n);
  for (auto &x : v) x = U(rng);
  return v;
}
static Batch make_batch(int n_gas, int n_pts, unsigned seed, int block_pts) {
  Batch b;
  std::mt19937_64 rng(seed);
  b.n_gas = n_gas, b.n_pts = n_pts;
  const int tangent[3] = {8, 4, 0};
  for (int r = 0; r < 3; ++r) {
    for (int k = b.n_layers - 1; k > tangent[r]; --k) b.seg_layer.push_back(k);
    for (int k = tangent[r]; k < b.n_layers; ++k) b.seg_layer.push_back(k);
    b.seg_off.push_back((int)b.seg_layer.size());
  }
  b.n_seg = (int)b.seg_layer.size();
  const size_t gs = (size_t)b.n_layers * n_pts; // exactly n_gas tables: a read of gas n_gas is out of bounds
  b.a = rnd(rng, n_gas * gs, 0.0, 0.2), b.e = rnd(rng, n_gas * gs, 0.0, 0.3);
  b.da = rnd(rng, n_gas * gs, -0.02, 0.02), b.de = rnd(rng, n_gas * gs, -0.02, 0.02);
  b.col = rnd(rng, (size_t)n_gas * b.n_seg, 0.2, 1.5);
  b.o = LimbOpts{n_gas, b.n_seg, 0, 0, 0, 250.0, 2975.0, 5e-4};
  const int n_pb = (n_pts + block_pts - 1) / block_pts;
  b.gx = (unsigned)((n_pb + 7) / 8 * 8) * b.n_rays;
  return b;
}

// a state: column parameters (gas, row of dcol), level parameters (level gas, level, c[row]), row parameters (w[row])
struct State {
  std::vector<int> par_gas, par_lgas, par_level, lgas_gas, n_levels, n_tab;
  std::vector<std::vector<int>> maps;
  std::vector<std::vector<double>> tabs;
  std::vector<double> dcol, par_w, par_c, par_t;
  int n_col = 0, n_lev = 0, n_row = 0;
};

// the definitions, one (ray, point) at a time: I and J_p [n_par] in path order
static void plain(const Batch &b, const State &s, std::vector<double> &rad, std::vector<double> &jac) {
  const int n_par = s.n_col + s.n_lev + s.n_row, n_pts = b.n_pts;
  const size_t gs = (size_t)b.n_layers * n_pts;
  rad.assign((size_t)b.n_rays * n_pts, NAN);
  jac.assign((size_t)b.n_rays * n_par * n_pts, NAN);
  for (int ray = 0; ray < b.n_rays; ++ray)
    for (int j = 0; j < n_pts; ++j) {
      double I = 0.0;
      std::vector<double> J(n_par, 0.0);
      for (int sg = b.seg_off[ray]; sg < b.seg_off[ray + 1]; ++sg) {
        const int r = b.seg_layer[sg];
        const size_t at = (size_t)r * n_pts + j;
        double tau = 0.0, E = 0.0;
        for (int g = 0; g < b.n_gas; ++g) {
          tau += b.a[g * gs + at] * b.col[(size_t)g * b.n_seg + sg];
          E += b.e[g * gs + at] * b.col[(size_t)g * b.n_seg + sg];
        }
        const Atten A = attenuation(tau);
        const double fp = atten_fprime(A, tau);
        for (int p = 0; p < n_par; ++p) {
          double dtau = 0.0, dE = 0.0;
          if (p < s.n_col) {
            const double D = s.dcol[(size_t)p * b.n_seg + sg];
            dtau = b.a[s.par_gas[p] * gs + at] * D, dE = b.e[s.par_gas[p] * gs + at] * D;
          } else if (p < s.n_col + s.n_lev) {
            const int q = p - s.n_col, k = s.par_lgas[q], L = s.par_level[q];
            const size_t pl = (size_t)s.n_tab[k] * n_pts;
            const double *tl = s.tabs[k].data() + (size_t)L * 2 * pl + (size_t)s.maps[k][r] * n_pts + j;
            const double c = s.par_c[(size_t)q * b.n_layers + r], u = b.col[(size_t)s.lgas_gas[k] * b.n_seg + sg];
            dtau = c * (u * tl[0]), dE = c * (u * tl[pl]);
          } else {
            const double w = s.par_t[(size_t)(p - s.n_col - s.n_lev) * b.n_layers + r];
            for (int g = 0; g < b.n_gas; ++g) {
              dtau += b.da[g * gs + at] * b.col[(size_t)g * b.n_seg + sg];
              dE += b.de[g * gs + at] * b.col[(size_t)g * b.n_seg + sg];
            }
            dtau *= w, dE *= w;
          }
          J[p] = J[p] * A.t + (-I * A.t * dtau + dE * A.f + E * fp * dtau);
        }
        I = I * A.t + E * A.f;
      }
      rad[(size_t)ray * n_pts + j] = I;
      for (int p = 0; p < n_par; ++p) jac[((size_t)ray * n_par + p) * n_pts + j] = J[p];
    }
}

// rows of n values: max |got - want| / the row's largest |want| over all rows; NaN anywhere counts as infinite
static double row_distance(const std::vector<double> &got, const std::vector<double> &want, int n) {
  double worst = 0.0;
  for (size_t r = 0; r * n < want.size(); ++r) {
    double scale = 0.0;
    for (int j = 0; j < n; ++j) scale = std::max(scale, std::fabs(want[r * n + j]));
    for (int j = 0; j < n; ++j) {
      const double d = std::fabs(got[r * n + j] - want[r * n + j]) / (scale > 0 ? scale : 1.0);
      worst = std::isfinite(d) ? std::max(worst, d) : INFINITY;
    }
  }
  return worst;
}
static int equal_values(const std::vector<double> &x, const std::vector<double> &y) {
  int bad = x.size() != y.size();
  for (size_t i = 0; i < std::min(x.size(), y.size()); ++i) bad += !(x[i] == y[i]);
  return bad;
}

template <int NG>
static int radiance_case(int n_gas, unsigned seed) {
  int bad = 0;
  for (int split = 0; split < 2; ++split) {
    const Batch b = make_batch(n_gas, 65, seed, split ? 64 : 256);
    std::vector<double> want, none, rad((size_t)b.n_rays * b.n_pts, NAN);
    plain(b, State{}, want, none);
    if (split)
      launch(b.gx, 1, [&] { sr_limb_split_kernel<NG>(b.a.data(), b.e.data(), b.n_pts, b.n_layers, b.seg_off.data(), b.seg_layer.data(), b.col.data(), b.o, b.n_rays, rad.data()); });
    else
      launch(b.gx, 1, [&] { sr_limb_kernel<NG>(b.a.data(), b.e.data(), b.n_pts, b.n_layers, b.seg_off.data(), b.seg_layer.data(), b.col.data(), b.o, b.n_rays, rad.data()); });
    const double d = row_distance(rad, want, b.n_pts);
    std::printf("%s<%d>, %d gases: |kernel - plain loops| / row max %.2e\n", split ? "sr_limb_split_kernel" : "sr_limb_kernel", NG, n_gas, d);
    bad += !(d <= 1e-12);
  }
  return bad;
}

static State make_state(const Batch &b, const std::vector<int> &col_gases, const std::vector<int> &lgas_gas, const std::vector<int> &levs,
                        int n_row, unsigned seed) {
  std::mt19937_64 rng(seed);
  std::uniform_real_distribution<double> U(0.0, 1.0);
  State s;
  s.par_gas = col_gases, s.n_col = (int)col_gases.size(), s.n_row = n_row, s.lgas_gas = lgas_gas;
  s.dcol = rnd(rng, (size_t)std::max(s.n_col, 1) * b.n_seg, 0.1, 1.0);
  for (size_t k = 0; k < lgas_gas.size(); ++k) {
    s.n_levels.push_back(4 + 2 * (int)k), s.n_tab.push_back(13 + (int)k);
    std::vector<int> m(b.n_layers);
    for (auto &v : m) v = (int)(U(rng) * s.n_tab[k]) % s.n_tab[k];
    s.maps.push_back(m);
    s.tabs.push_back(rnd(rng, (size_t)s.n_levels[k] * 2 * s.n_tab[k] * b.n_pts, 0.0, 0.3)); // exactly sized
    s.par_lgas.insert(s.par_lgas.end(), levs[k], (int)k);
  }
  std::shuffle(s.par_lgas.begin(), s.par_lgas.end(), rng);
  s.n_lev = (int)s.par_lgas.size();
  for (int k : s.par_lgas) s.par_level.push_back((int)(U(rng) * s.n_levels[k]) % s.n_levels[k]);
  s.par_c.resize((size_t)s.n_lev * b.n_layers), s.par_t.resize((size_t)n_row * b.n_layers);
  for (auto &c : s.par_c) c = U(rng) < 0.6 ? 0.2 + U(rng) : 0.0;
  for (auto &c : s.par_t) c = U(rng) < 0.6 ? 0.2 + U(rng) : 0.0;
  return s;
}

// one launch of the state kernel's NG instance on the batch (b.n_gas <= NG: padded when smaller), dense plan or per ray
template <int NG, bool ROWS, bool BANDS>
static void state_launch(const Batch &b, const State &s, bool per_ray, const std::vector<double> &par_w, std::vector<double> &rad,
                         std::vector<double> &jac, const FoldBands *bands = nullptr) {
  const int n_par = s.n_col + s.n_lev + s.n_row, bits = state_gas_bits(b.n_gas);
  const bool several = s.lgas_gas.size() > 1;
  LevelJacPlan P{};
  RayJacPlan R{};
  if (per_ray) {
    sr_los_desc los{};
    std::vector<int> pt_off(b.n_seg + 1);
    for (int i = 0; i <= b.n_seg; ++i) pt_off[i] = 2 * i;
    los.n_rays = b.n_rays, los.n_gas = b.n_gas, los.seg_off = b.seg_off.data(), los.seg_layer = b.seg_layer.data(), los.pt_off = pt_off.data();
    R = ray_jac_plan(&los, s.n_col, s.par_gas.data(), par_w.data(), s.n_lev, s.par_level.data(), s.par_c.data(), b.n_layers, s.n_row,
                     s.par_t.data(), several ? s.par_lgas.data() : nullptr, 0, bits);
    P.n_blocks = R.n_blocks;
    P.blk.swap(R.blk), P.ent_off.swap(R.ent_off), P.slot_par.swap(R.slot_par), P.ent.swap(R.ent);
  } else {
    P = level_jac_plan(s.n_col, s.par_gas.data(), s.n_lev, s.par_level.data(), s.par_c.data(), b.n_layers, s.n_row, s.par_t.data(),
                       several ? s.par_lgas.data() : nullptr, 0, bits);
  }
  std::vector<LevelEnt> ent = P.ent;
  ent.push_back(LevelEnt{0, 0, 0.0});
  rad.assign((size_t)b.n_rays * b.n_pts, NAN);
  jac.assign((size_t)b.n_rays * n_par * b.n_pts, per_ray ? 0.0 : NAN); // (per ray: the launcher clears the rows first)
  std::vector<int> rows;
  LevelGasTabs T{};
  for (size_t k = 0; k < s.lgas_gas.size(); ++k) {
    rows.insert(rows.end(), s.maps[k].begin(), s.maps[k].end());
    T.tab[k] = s.tabs[k].data(), T.n_tab_rows[k] = s.n_tab[k], T.gas[k] = s.lgas_gas[k];
  }
  if (rows.empty()) rows.assign(b.n_layers, 0);
  const int gas = several || s.lgas_gas.empty() ? -1 : s.lgas_gas[0], n_tab = several || s.lgas_gas.empty() ? 0 : s.n_tab[0];
  const double *tab = several || s.lgas_gas.empty() ? nullptr : s.tabs[0].data();
  const StateRayBlocks rbk{R.ray_blk_off.data(), R.col_row.data()};
  const double *pda = b.da.data(), *pde = b.de.data();
  std::conditional_t<BANDS, FoldBands, double *> out;
  if constexpr (BANDS) out = *bands;
  else out = jac.data();
  auto go = [&](auto... pack) {
    launch(b.gx, P.n_blocks, [&] {
      sr_limb_jac_state_kernel<NG, 8, true, ROWS, BANDS, false, decltype(pack)...>(
          b.a.data(), b.e.data(), b.n_pts, b.n_layers, b.seg_off.data(), b.seg_layer.data(), b.col.data(), s.dcol.data(), b.o, b.n_rays, gas,
          tab, n_tab, rows.data(), P.blk.data(), P.ent_off.data(), ent.data(), P.slot_par.data(), n_par, BANDS ? nullptr : rad.data(), out,
          pack...);
    });
  };
  if constexpr (ROWS) {
    if (several) go(pda, pde, T);
    else go(pda, pde);
  } else {
    if (several && per_ray) go(T, rbk);
    else if (several) go(T);
    else if (per_ray) go(rbk);
    else go();
  }
  // the gas words decode to the parameters' gases, three bits per slot, eight slots per block
  if (!per_ray)
    for (int p = 0; p < s.n_col; ++p)
      if (((unsigned)P.blk[2 * (p / 8) + 1] >> (3 * (p % 8)) & 7u) != (unsigned)s.par_gas[p]) std::printf("gas word of column slot %d is wrong\n", p), std::abort();
}

static int state_cases() {
  int bad = 0;
  // <8, 8, COLS, ROWS>: column slots on gases 0, 4, 7, 5, 3, a level gas with index 6, row slots; then its BANDS instance
  {
    const Batch b = make_batch(8, 65, 11, 256);
    const State s = make_state(b, {0, 4, 7, 5, 3}, {6}, {4}, 3, 12);
    const int n_par = s.n_col + s.n_lev + s.n_row;
    std::vector<double> want_r, want_j, rad, jac, none_r, none_j;
    plain(b, s, want_r, want_j);
    state_launch<8, true, false>(b, s, false, {}, rad, jac);
    const double d_r = row_distance(rad, want_r, b.n_pts), d_j = row_distance(jac, want_j, b.n_pts);
    std::printf("state <8, 8, COLS, ROWS>, 5 + 4 + 3 parameters: radiances %.2e, Jacobian rows %.2e of a row's largest value\n", d_r, d_j);
    bad += !(d_r <= 1e-12) + !(d_j <= 1e-12);
    // bands: 20 bands, two tiles; part starts as NaN
    std::mt19937_64 rng(13);
    std::uniform_real_distribution<double> U(0.0, 1.0);
    const int n_bands = 20, n_tiles = 2, n_slots = 4 * ((b.n_pts + 255) / 256);
    std::vector<int> range(2 * n_bands);
    std::vector<double> Wt((size_t)n_tiles * b.n_pts * 16, 0.0), part((size_t)b.n_rays * (1 + n_par) * n_slots * n_tiles * 16, NAN);
    for (int k = 0; k < n_bands; ++k) {
      int r0 = (int)(U(rng) * b.n_pts), r1 = std::min(b.n_pts, r0 + 2 + (int)(U(rng) * (b.n_pts - r0)));
      if (k == 0 || r1 - r0 < 2) r0 = r1 = 0;
      if (k == 1) r0 = 0, r1 = b.n_pts;
      range[2 * k] = r0, range[2 * k + 1] = r1;
      for (int j = r0; j < r1; ++j) Wt[((size_t)(k >> 4) * b.n_pts + j) * 16 + (k & 15)] = 0.1 + U(rng);
    }
    const FoldBands bd{Wt.data(), range.data(), part.data(), n_bands};
    state_launch<8, true, true>(b, s, false, {}, none_r, none_j, &bd);
    double worst = 0.0;
    for (int ray = 0; ray < b.n_rays; ++ray)
      for (int q = 0; q <= n_par; ++q) {
        const size_t row = q == 0 ? (size_t)ray : (size_t)b.n_rays + (size_t)ray * n_par + (q - 1);
        const double *sp = q == 0 ? &rad[(size_t)ray * b.n_pts] : &jac[((size_t)ray * n_par + (q - 1)) * b.n_pts];
        std::vector<double> f(n_bands), u(n_bands);
        double scale = 0.0;
        for (int k = 0; k < n_bands; ++k) {
          double v = 0.0, w = 0.0;
          if (range[2 * k + 1] > range[2 * k])
            for (int c = range[2 * k] >> 6; c <= (range[2 * k + 1] - 1) >> 6; ++c) v += part[((row * n_slots + c) * n_tiles + (k >> 4)) * 16 + (k & 15)];
          for (int j = 0; j < b.n_pts; ++j) w = std::fma(sp[j], Wt[((size_t)(k >> 4) * b.n_pts + j) * 16 + (k & 15)], w);
          f[k] = v, u[k] = w, scale = std::max(scale, std::fabs(w));
        }
        for (int k = 0; k < n_bands; ++k) {
          const double d = std::fabs(f[k] - u[k]) / (scale > 0 ? scale : 1.0);
          worst = std::isfinite(d) ? std::max(worst, d) : INFINITY;
        }
        bad += f[0] != 0.0;
      }
    std::printf("state <8, 8, COLS, ROWS, BANDS>, 20 bands: |fused - band sums of the spectra| / row max %.2e\n", worst);
    bad += !(worst <= 1e-12);
  }
  // two level gases (5 and 2), nine column slots: two blocks; dense and with parameter blocks per ray
  {
    const Batch b = make_batch(8, 65, 21, 256);
    State s = make_state(b, {7, 6, 5, 4, 3, 2, 1, 0, 7}, {5, 2}, {3, 4}, 0, 22);
    // weights at the sample points, two per segment: parameter p is seen on the segments where it has a dcol
    std::mt19937_64 rng(23);
    std::uniform_real_distribution<double> U(0.0, 1.0);
    std::vector<double> par_w((size_t)s.n_col * 2 * b.n_seg, 0.0);
    for (int p = 0; p < s.n_col; ++p)
      for (int sg = 0; sg < b.n_seg; ++sg) {
        const bool on = p != 1 && (sg + p) % 3 != 0 && !(p == 2 && sg >= b.seg_off[1]); // 1: no weights; 2: the first ray only
        if (!on) s.dcol[(size_t)p * b.n_seg + sg] = 0.0;
        par_w[((size_t)p * b.n_seg + sg) * 2] = par_w[((size_t)p * b.n_seg + sg) * 2 + 1] = on ? 1.0 : 0.0;
      }
    std::vector<double> want_r, want_j, rad, jac;
    plain(b, s, want_r, want_j);
    for (int per_ray = 0; per_ray < 2; ++per_ray) {
      state_launch<8, false, false>(b, s, per_ray != 0, par_w, rad, jac);
      const double d_r = row_distance(rad, want_r, b.n_pts), d_j = row_distance(jac, want_j, b.n_pts);
      std::printf("state <8, 8, COLS> two level gases, 9 + 7 parameters, %s: radiances %.2e, Jacobian rows %.2e\n",
                  per_ray ? "blocks per ray" : "dense plan", d_r, d_j);
      bad += !(d_r <= 1e-12) + !(d_j <= 1e-12);
    }
  }
  // padded launches: seven gases on <8>, five on <6>, against the instances of exactly seven and five gases
  {
    const Batch b7 = make_batch(7, 65, 31, 256), b5 = make_batch(5, 65, 32, 256);
    const State s7 = make_state(b7, {0, 4, 6, 5, 3}, {6}, {4}, 3, 33), s5 = make_state(b5, {4, 0, 3}, {4, 2}, {2, 3}, 0, 34);
    std::vector<double> r_pad, j_pad, r_own, j_own;
    state_launch<8, true, false>(b7, s7, false, {}, r_pad, j_pad);
    state_launch<7, true, false>(b7, s7, false, {}, r_own, j_own);
    int diff = equal_values(r_pad, r_own) + equal_values(j_pad, j_own);
    state_launch<6, false, false>(b5, s5, false, {}, r_pad, j_pad);
    state_launch<5, false, false>(b5, s5, false, {}, r_own, j_own);
    diff += equal_values(r_pad, r_own) + equal_values(j_pad, j_own);
    std::printf("padded launches (7 gases on <8>, 5 on <6>) against the unpadded instances: %d values differ\n", diff);
    bad += diff;
  }
  return bad;
}

// The dense plan and the plan per ray of an eight-gas batch with column parameters of gases 0, 4, 7, 5, 3 and the eight
// hidden slots of a pointing call: thirteen column slots in two blocks of eight, three bits per slot, the hidden slots'
// rows of jac behind the state's; the same call on four gases (four hidden slots) gives the words of two bits in one block
// of sixteen slots.
static int plan_words() {
  int bad = 0;
  const Batch b = make_batch(8, 65, 41, 256);
  std::vector<int> pt_off(b.n_seg + 1);
  for (int i = 0; i <= b.n_seg; ++i) pt_off[i] = 2 * i;
  std::vector<double> ones((size_t)5 * 2 * b.n_seg, 1.0);
  for (int n_gas : {8, 4}) {
    const std::vector<int> gases = n_gas == 8 ? std::vector<int>{0, 4, 7, 5, 3} : std::vector<int>{0, 3, 2, 1, 3};
    const int bits = state_gas_bits(n_gas), np = n_gas == 8 ? 8 : 16, n_slots = 5 + n_gas;
    std::vector<int> want = gases;
    for (int g = 0; g < n_gas; ++g) want.push_back(g);
    const LevelJacPlan P = level_jac_plan(5, gases.data(), 0, nullptr, nullptr, b.n_layers, 0, nullptr, nullptr, n_gas, bits);
    sr_los_desc los{};
    los.n_rays = b.n_rays, los.n_gas = n_gas, los.seg_off = b.seg_off.data(), los.seg_layer = b.seg_layer.data(), los.pt_off = pt_off.data();
    const RayJacPlan R = ray_jac_plan(&los, 5, gases.data(), ones.data(), 0, nullptr, nullptr, b.n_layers, 0, nullptr, nullptr, n_gas, bits);
    bad += bits != (n_gas == 8 ? 3 : 2) || level_jac_np(n_slots, bits) != np || R.np != np;
    bad += P.n_blocks != (n_slots + np - 1) / np || R.n_blocks != P.n_blocks || R.ray_blk_off[b.n_rays] != b.n_rays * P.n_blocks;
    for (int q = 0; q < n_slots; ++q) {
      const int blk = q / np, slot = q % np, par = q < 5 ? q : 5 + (q - 5); // (hidden slot g: row n_state + g, n_state = 5)
      const unsigned mask = (1u << bits) - 1u;
      bad += (int)((unsigned)P.blk[2 * blk + 1] >> (bits * slot) & mask) != want[q];
      bad += P.slot_par[(size_t)blk * np + slot] != par;
      for (int ray = 0; ray < b.n_rays; ++ray) {
        const size_t rb = (size_t)R.ray_blk_off[ray] + blk;
        bad += (int)((unsigned)R.blk[2 * rb + 1] >> (bits * slot) & mask) != want[q];
        bad += R.slot_par[rb * np + slot] != par || R.col_row[rb * np + slot] != q;
      }
    }
    for (int blk = 0; blk < P.n_blocks; ++blk) bad += P.blk[2 * blk] != std::min(np, n_slots - blk * np);
    std::printf("plans of %d gases, 5 column parameters + %d hidden slots: %d block(s) of %d slots, %d bits per slot\n", n_gas, n_gas,
                P.n_blocks, np, bits);
  }
  std::printf("plan words that do not decode to their gases and rows: %d\n", bad);
  return bad;
}

int main() {
  pthread_barrier_init(&g_block_bar, nullptr, 256);
  int bad = 0;
  bad += radiance_case<8>(8, 1);
  bad += radiance_case<5>(5, 2);
  bad += state_cases();
  bad += plan_words();
  std::printf(bad ? "FAILED\n" : "all cases agree\n");
  return bad != 0;
}
