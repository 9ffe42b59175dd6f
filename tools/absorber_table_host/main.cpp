// Host build of sr_absorber_table_kernel's own text (spectrobot_amd/csrc/sr_absorber_table.inc, the file the library
// compiles): the blocks and lanes of its launch walked one after the other.  Every buffer has exactly the size the
// launcher gives it, so that AddressSanitizer sees an index beyond it; the outputs start as NaN (or, accumulating, as a
// known pattern), so that the comparison sees a place that was not written.  Against plain loops written here in long
// double, to the bound of tests/absorber_table_reference.py.  The cases are those of tests/test_gpu_absorber_table.py:
// 300 grid points (a full block of 256 and a partial one), g_lo 0 and 4097, 5 rows in chunks of 2 rows per block, 4 sets --
// one finer than the grid, one coarser, one covering points 100 .. 180 whose lower end is bitwise a grid point and whose
// upper end lies between two, one whose last knot is bitwise grid point 256 (the block boundary) -- rows that use one set
// or two, scales 1 .. 1e18; with and without source, derivative and accumulation; a table no point of the grid reaches.
// Built with AddressSanitizer and UBSan by tools/host_sim/run.sh absorber_table_host: indexing, range tests and row
// mapping on a machine without a GPU -- not the compiled gfx950 code.
#include "hip_on_host.hpp"
namespace sr {
#include "sr_absorber_table.inc"
}

typedef long double LDb;
struct Set { double v0, dv; std::vector<double> a; };

static LDb interp(const Set &s, double nu, LDb *t_out, LDb *slope) {
  const int n = (int)s.a.size();
  const LDb t = ((LDb)nu - s.v0) / s.dv;
  *t_out = 0; *slope = 0;
  if (t < 0 || t > n - 1) return 0;
  const int i = std::min((int)std::floor(t), n - 1), i1 = std::min(i + 1, n - 1);
  *t_out = t; *slope = std::fabs((LDb)s.a[i1] - s.a[i]);
  return s.a[i] + ((LDb)s.a[i1] - s.a[i]) * (t - i);
}

template <bool SOURCE, bool DERIV, bool ACC> static int run_case(int g_lo, bool far_away, unsigned seed) {
  std::mt19937_64 rng(seed);
  std::uniform_real_distribution<double> U(0.0, 1.0);
  const int n_pts = 300, n_rows = 5, rows_per_block = 2;
  const double w0 = 2900.0, gstep = (2900.0 + 0.01) - 2900.0;
  auto nu = [&](int j) { return w0 + (double)(g_lo + j) * gstep; };
  std::vector<Set> sets(4);
  sets[0] = {nu(0) - 0.013, gstep / 3.7, std::vector<double>(1120)};
  sets[1] = {nu(0) - 0.5, 0.13, std::vector<double>(40)};
  sets[2] = {nu(100), (nu(180) + 0.4 * gstep - nu(100)) / 32.0, std::vector<double>(33)};
  sets[3] = {nu(256) - 2.0, 0.015625, std::vector<double>(129)};
  if (far_away) for (Set &s : sets) s.v0 += 1000.0;
  if (!far_away && ((nu(100) - sets[2].v0) / sets[2].dv != 0.0 || (nu(256) - sets[3].v0) / sets[3].dv != 128.0)) { std::printf("case not exact\n"); return 1; }
  std::vector<double> values, v0, dv;
  std::vector<long long> off;
  std::vector<int> nn;
  for (Set &s : sets) {
    for (double &x : s.a) x = 1e-20 * (U(rng) - 0.1); // (some negative values: used as given)
    off.push_back((long long)values.size());
    values.insert(values.end(), s.a.begin(), s.a.end());
    v0.push_back(s.v0); dv.push_back(s.dv); nn.push_back((int)s.a.size());
  }
  const std::vector<double> temps = {140.0, 200.0, 170.0, 230.0, 310.0}, scale = {1.0, 1e5, 1e9, 1e14, 1e18};
  const std::vector<int> slot2 = {0, 0, 1, 2, 0, 1, 1, 2, 3, 3};
  const std::vector<double> w2 = {1, 0, 1, 0, 0.6, 0.4, 0.4, 0.6, 1, 0}, dw2 = {0, 0, -0.02, 0.02, -0.02, 0.02, -0.02, 0.02, 0, 0};
  const size_t n_out = (size_t)n_rows * n_pts;
  auto pattern = [&](int k, size_t at) { return ACC ? (1e-7 * (k + 1)) * (1.0 + (double)(at % 17)) : (double)NAN; };
  std::vector<double> out[4];
  for (int k = 0; k < 4; ++k) {
    out[k].resize(n_out);
    for (size_t at = 0; at < n_out; ++at) out[k][at] = pattern(k, at);
  }
  gridDim.x = (n_pts + 255) / 256; gridDim.y = (n_rows + rows_per_block - 1) / rows_per_block; blockDim.x = 256;
  for (unsigned by = 0; by < gridDim.y; ++by)
    for (unsigned bx = 0; bx < gridDim.x; ++bx)
      for (unsigned t = 0; t < 256; ++t) {
        blockIdx.x = bx; blockIdx.y = by; threadIdx.x = t;
        sr::sr_absorber_table_kernel<SOURCE, DERIV, ACC>(4, v0.data(), dv.data(), off.data(), nn.data(), values.data(), 0, n_rows, rows_per_block,
                                                         temps.data(), scale.data(), slot2.data(), w2.data(), DERIV ? dw2.data() : nullptr, w0, gstep,
                                                         g_lo, n_pts, out[0].data(), out[1].data(), DERIV ? out[2].data() : nullptr,
                                                         DERIV ? out[3].data() : nullptr);
      }
  // the plain loops
  int bad = 0;
  const LDb eps = std::ldexp((LDb)1, -53);
  for (int r = 0; r < n_rows; ++r)
    for (int j = 0; j < n_pts; ++j) {
      const size_t at = (size_t)r * n_pts + j;
      const double x = nu(j);
      LDb t0, t1, d0, d1;
      const LDb s0 = interp(sets[slot2[2 * r]], x, &t0, &d0), s1 = interp(sets[slot2[2 * r + 1]], x, &t1, &d1);
      const bool touched = t0 != 0 || t1 != 0 || s0 != 0 || s1 != 0 || d0 != 0 || d1 != 0;
      const LDb c = scale[r], T = temps[r], xx = (LDb)sr::kC2 * x / T, ex = std::exp(xx);
      const LDb B = 2 * (LDb)sr::kHcgs * ((LDb)sr::kCcgs * sr::kCcgs) * ((LDb)x * x * x) / (ex - 1), dB = B * (xx / T) * (ex / (ex - 1));
      LDb ref[4], bound[4];
      for (int d = 0; d < 2; ++d) {
        const double *w = d ? &dw2[2 * r] : &w2[2 * r];
        ref[2 * d] = c * (w[0] * s0 + w[1] * s1);
        bound[2 * d] = eps * (8 * c * (std::fabs(w[0] * s0) + std::fabs(w[1] * s1)) + 4 * c * (std::fabs(w[0]) * t0 * d0 + std::fabs(w[1]) * t1 * d1));
      }
      ref[1] = SOURCE ? ref[0] * B : 0;
      bound[1] = bound[0] * B + eps * (8 + 2 * xx) * std::fabs(ref[1]);
      ref[3] = SOURCE ? ref[2] * B + ref[0] * dB : 0;
      bound[3] = bound[2] * B + eps * (8 + 2 * xx) * std::fabs(ref[2] * B) + bound[0] * dB + eps * (12 + 2 * xx) * std::fabs(ref[0] * dB);
      for (int k = 0; k < (DERIV ? 4 : 2); ++k) {
        const double v = out[k][at], p = pattern(k, at);
        bool ok;
        if (ACC && (!touched || (!SOURCE && (k & 1)))) ok = std::memcmp(&v, &p, sizeof v) == 0; // left as it was, bit for bit
        else if (ACC) ok = std::fabs((LDb)v - (p + ref[k])) <= bound[k] + eps * std::fabs(p + ref[k]);
        else if (ref[k] == 0 && bound[k] == 0) ok = v == 0.0;
        else ok = std::fabs((LDb)v - ref[k]) <= bound[k];
        if (!ok && bad++ < 10) std::printf("row %d point %d output %d: %.17g, plain %.17Lg (bound %.3Lg)\n", r, j, k, v, ref[k], bound[k]);
      }
    }
  std::printf("source %d deriv %d acc %d g_lo %d%s: %s\n", SOURCE, DERIV, ACC, g_lo, far_away ? " (no point in any set)" : "", bad ? "FAILED" : "ok");
  return bad;
}

template <bool S, bool D, bool A> static int run_all(unsigned &seed) {
  int bad = run_case<S, D, A>(0, false, seed++);
  bad += run_case<S, D, A>(4097, false, seed++);
  bad += run_case<S, D, A>(0, true, seed++);
  return bad;
}

int main() {
  unsigned seed = 20261020;
  int bad = 0;
  bad += run_all<true, true, false>(seed);
  bad += run_all<true, false, false>(seed);
  bad += run_all<false, true, false>(seed);
  bad += run_all<false, false, false>(seed);
  bad += run_all<true, true, true>(seed);
  bad += run_all<true, false, true>(seed);
  bad += run_all<false, true, true>(seed);
  bad += run_all<false, false, true>(seed);
  std::printf(bad ? "FAILED\n" : "all cases ok\n");
  return bad ? 1 : 0;
}
