// Host build of sr_lowres_weights_tab_kernel's own text (spectrobot_amd/csrc/sr_lowres_weights_tab.inc, the file the library compiles): the blocks and threads of
// its launch walked one after the other.  Every buffer has exactly the size the launcher gives it and starts as NaN, so that
// AddressSanitizer sees an index beyond it and the comparison a place that was not written.  Against plain loops written
// here (long double, the slopes m_k per unit of t, the window by a linear scan): W, Wt with the zero columns of its last
// tile, range, and with INSTR the two derivative tables, to 1e-12 of the band's largest weight; a band outside the grid and
// the points outside a window exact zeros.  The cases: one table for all bands and one per band (n_shapes = n_bands);
// 19 and 33 bands (a partial last tile of Wt) and 16 (none); a band whose window's lower end is bitwise a grid point
// (t = t_lo exactly there), one whose upper end is (t = t_hi: the last knot, interval n_tab - 2 with s = 1 by the clamp) and
// one with a grid point exactly on an interior knot: those three weights are p phi_k / w to a few ulp.  Built with
// AddressSanitizer and UBSan by tools/host_sim/run.sh ils_host: indexing, clamp, table and tile mapping on a machine without a GPU -- not the
// compiled gfx950 code.
#include "hip_on_host.hpp"
namespace sr {
#include "sr_lowres_weights_tab.inc"
}

struct Case { int n_pts, g_lo, n_bands, n_shapes, n_tab; double t_lo, t_hi; };

template <bool INSTR> static int run_case(const Case &c, unsigned seed) {
  std::mt19937_64 rng(seed);
  std::uniform_real_distribution<double> U(0.0, 1.0);
  const double w0 = 2975.0, gstep = (2975.0 + 5e-4) - 2975.0;
  const int n = c.n_pts, nb = c.n_bands, nt = c.n_tab, n_rows = (nb + 15) / 16 * 16, n_tab3 = INSTR ? 3 : 1;
  const double h = (c.t_hi - c.t_lo) / (nt - 1);
  auto gcm = [&](int i) { return w0 + (double)(c.g_lo + n - 1 - i) * gstep; };
  auto xnm = [&](int i) { return 1.e7 / gcm(i); };
  // tables: a skewed bell with a ripple, non-zero at both ends of the support
  std::vector<double> phi((size_t)c.n_shapes * nt), tab(2 * phi.size());
  for (int q = 0; q < c.n_shapes; ++q)
    for (int k = 0; k < nt; ++k) {
      const double t = c.t_lo + k * h;
      phi[(size_t)q * nt + k] = std::exp(-0.5 * t * t) * (1.0 + (0.3 - 0.05 * q) * std::tanh(t)) + 0.05 * std::sin(3.0 * t + q) + 0.02;
    }
  for (int q = 0; q < c.n_shapes; ++q) // knots and slopes per knot interval, as sr_set_ils forms them
    for (int k = 0; k < nt; ++k) {
      const double *p = &phi[(size_t)q * nt];
      tab[2 * ((size_t)q * nt + k)] = p[k];
      tab[2 * ((size_t)q * nt + k) + 1] = k == 0 ? p[1] - p[0] : k == nt - 1 ? p[k] - p[k - 1] : (p[k + 1] - p[k - 1]) / 2.0;
    }
  // bands
  const int kx = n / 2 + 3, k_knot = nt / 3;
  const double xk = xnm(kx), wx = 0.25, t_knot = c.t_lo + k_knot * h, span = xnm(n - 1) - xnm(0);
  std::vector<double> cen(nb), wid(nb);
  for (int b = 0; b < nb; ++b) {
    cen[b] = xnm(0) + span * (0.05 + 0.9 * U(rng));
    wid[b] = span * (0.01 + 0.2 * U(rng)) / (c.t_hi - c.t_lo);
  }
  cen[0] = xk - c.t_lo * wx; wid[0] = wx;                       // lower end == x_k
  cen[1] = xk - c.t_hi * wx; wid[1] = wx;                       // upper end == x_k
  cen[2] = xk - t_knot * wx; wid[2] = wx;                       // x_k on an interior knot
  cen[3] = xnm(n - 1) + 100.0 * span; wid[3] = 0.01 * span;     // outside the grid
  cen[4] = xnm(n / 2); wid[4] = 10.0 * span;                    // the whole grid
  if (cen[0] + c.t_lo * wx != xk || cen[1] + c.t_hi * wx != xk || (xk - cen[2]) / wx != t_knot) { std::printf("case not exact\n"); return 1; }
  std::vector<double> W((size_t)n_tab3 * nb * n, NAN), Wt((size_t)n_tab3 * (n_rows / 16) * n * 16, NAN);
  std::vector<int> range(2 * (size_t)nb, -7);
  gridDim.x = (n + 255) / 256; gridDim.y = n_rows; blockDim.x = 256;
  for (unsigned by = 0; by < gridDim.y; ++by)
    for (unsigned bx = 0; bx < gridDim.x; ++bx)
      for (unsigned t = 0; t < 256; ++t) {
        blockIdx.x = bx; blockIdx.y = by; threadIdx.x = t;
        sr::sr_lowres_weights_tab_kernel<INSTR>(n, c.g_lo, w0, gstep, cen.data(), wid.data(), tab.data(), c.n_shapes, nt, c.t_lo, c.t_hi,
                                                nb, W.data(), range.data(), Wt.data());
      }
  // the plain loops
  int bad = 0;
  const size_t tab_w = (size_t)nb * n, tab_wt = (size_t)(n_rows / 16) * n * 16;
  for (int b = 0; b < n_rows; ++b) {
    std::vector<long double> ref((size_t)3 * n, 0.0L);
    int i0 = n, i1 = 0;
    if (b < nb) {
      const double f = cen[b], w = wid[b], lo = f + c.t_lo * w, hi = f + c.t_hi * w;
      for (int i = 0; i < n; ++i)
        if (xnm(i) >= lo && xnm(i) <= hi) { i0 = std::min(i0, i); i1 = std::max(i1, i + 1); }
      const double *p = &phi[(size_t)(c.n_shapes > 1 ? b : 0) * nt];
      const long double hl = ((long double)c.t_hi - c.t_lo) / (nt - 1);
      auto slope = [&](int k) -> long double {
        return k == 0 ? ((long double)p[1] - p[0]) / hl : k == nt - 1 ? ((long double)p[k] - p[k - 1]) / hl : ((long double)p[k + 1] - p[k - 1]) / (2 * hl);
      };
      if (i1 - i0 >= 2)
        for (int i = i0; i < i1; ++i) {
          const long double g = gcm(i), x = xnm(i), t = (x - f) / w;
          const long double xl = i > i0 ? xnm(i - 1) : xnm(i), xr = i + 1 < i1 ? xnm(i + 1) : xnm(i);
          const long double pw = g * g * 1e-7L * (xr - xl) / 2;
          const long double q = (t - c.t_lo) / hl;
          const int k = std::min(std::max((int)std::floor(q), 0), nt - 2);
          const long double s = q - k, m0 = slope(k), m1 = slope(k + 1), p0 = p[k], p1 = p[k + 1];
          const long double f0 = (2 * s * s * s - 3 * s * s + 1) * p0 + (s * s * s - 2 * s * s + s) * hl * m0 + (3 * s * s - 2 * s * s * s) * p1 +
                                 (s * s * s - s * s) * hl * m1;
          const long double f1 = (6 * s * s - 6 * s) * (p0 - p1) / hl + (3 * s * s - 4 * s + 1) * m0 + (3 * s * s - 2 * s) * m1;
          const int j = n - 1 - i;
          ref[j] = pw * f0 / w;
          ref[(size_t)n + j] = -pw * f1 / ((long double)w * w);
          ref[(size_t)2 * n + j] = -pw * (f0 + t * f1) / w;
        }
      const bool any = i1 - i0 >= 2;
      if (range[2 * b] != (any ? n - i1 : 0) || range[2 * b + 1] != (any ? n - i0 : 0)) { std::printf("band %d: range\n", b); ++bad; }
    }
    for (int k = 0; k < n_tab3; ++k) {
      long double big = 0;
      for (int j = 0; j < n; ++j) big = std::max(big, std::fabs(ref[(size_t)k * n + j]));
      for (int j = 0; j < n; ++j) {
        const long double r = ref[(size_t)k * n + j];
        const double vt = Wt[k * tab_wt + ((size_t)(b >> 4) * n + j) * 16 + (b & 15)];
        const double v = b < nb ? W[k * tab_w + (size_t)b * n + j] : vt;
        const bool ok = r == 0 ? (v == 0.0 && vt == 0.0) : (v == vt && std::fabs(v - r) <= 1e-12L * big);
        if (!ok && bad++ < 10) std::printf("band %d table %d point %d: %.17g / %.17g, plain %.17Lg\n", b, k, j, v, vt, r);
      }
    }
  }
  // the three exact points: p phi_k / w
  struct { int b, knot; } ex[3] = {{0, 0}, {1, nt - 1}, {2, k_knot}};
  for (auto e : ex) {
    const int i = kx, j = n - 1 - kx; // x_k is nm point kx, i.e. cm-1 index n - 1 - kx of the tables
    const double *p = &phi[(size_t)(c.n_shapes > 1 ? e.b : 0) * nt];
    const bool first = e.b == 0, last = e.b == 1;
    const long double xl = first ? xnm(i) : xnm(i - 1), xr = last ? xnm(i) : xnm(i + 1);
    const long double want = (long double)gcm(i) * gcm(i) * 1e-7L * (xr - xl) / 2 * p[e.knot] / wid[e.b];
    const double v = W[(size_t)e.b * n + j];
    if (!(std::fabs(v - want) <= 8 * 1.2e-16L * std::fabs(want)) || want == 0) { std::printf("exact point of band %d: %.17g, p phi_k / w %.17Lg\n", e.b, v, want); ++bad; }
    const int out = first ? j + 1 : last ? j - 1 : -1; // the neighbour outside the window (nm index i - 1 <-> j + 1)
    if (out >= 0 && W[(size_t)e.b * n + out] != 0.0) { std::printf("band %d: the neighbour outside is not 0\n", e.b); ++bad; }
  }
  std::printf("%s n_pts %d g_lo %d bands %d shapes %d knots %d [%g, %g]: %s\n", INSTR ? "instr" : "value", n, c.g_lo, nb, c.n_shapes, nt, c.t_lo,
              c.t_hi, bad ? "FAILED" : "ok");
  return bad;
}

int main() {
  const Case cases[] = {{300, 0, 19, 1, 65, -5.0, 3.0},   {300, 0, 19, 19, 65, -5.0, 3.0}, {600, 0, 33, 33, 65, -5.0, 3.0},
                        {600, 40, 16, 16, 33, -4.0, 4.0}, {257, 0, 5, 1, 4, -3.0, 3.0},    {513, 7, 33, 1, 161, -5.0, 5.0}};
  int bad = 0;
  unsigned seed = 20261019;
  for (const Case &c : cases) {
    bad += run_case<false>(c, seed++);
    bad += run_case<true>(c, seed++);
  }
  std::printf(bad ? "FAILED\n" : "all cases ok\n");
  return bad ? 1 : 0;
}
