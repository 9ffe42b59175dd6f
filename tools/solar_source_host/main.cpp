// Host build of sr_solar_source_kernel's own text (spectrobot_amd/csrc/sr_solar_source.inc on sr_solar_tile.inc with the
// chunk lists of sr_solar_plan.hpp, the files the library compiles) behind tools/host_sim/hip_on_host.hpp with threaded lanes: a block is
// 256 threads, its barrier a real barrier, v_mfma_f64_16x16x4 emulated in its operand layout.  Every buffer has exactly
// the size the entry gives it, so that AddressSanitizer sees an index beyond it; the outputs start as NaN (or, accumulating,
// as a known pattern), so that the comparison sees a place that was not written.  Against plain loops in long double to
// the bound of tests/solar_source_reference.py, on the panel of tests/test_gpu_solar_source.py: n_rows 1, 15, 17, 33, 65 x
// n_k 1, 3, 5, 13, 160 x n_pts 1, 63, 65, 257 (tile, chunk and store edges) with columns laid out as a ray's are, rows in
// shadow, a row without columns and a row beyond tau = 700; the overwrite instance with the transmission on the whole
// panel, the other three on its corners; sparse lists against full lists, which must agree in every bit.  Behind the
// panel n_k = 259 at 17 rows x 63 and 65 points, overwrite with the transmission and accumulate: with every chunk listed
// a tile walks 65 chunks -- one whole batch of kSolarBatch, then a batch of one chunk padded to a pair, the last chunk of
// three k.  The
// exponential here is the host's (the device routine is pinned on the GPU).  Built with AddressSanitizer and UBSan by
// tools/host_sim/run.sh solar_source_host -- indexing, lists, tile and row mapping on a machine without a GPU, not the
// compiled gfx950 code.
#define HOST_SIM_THREADED_LANES
#include "hip_on_host.hpp"
static pthread_barrier_t g_block_bar;
static void block_barrier() { pthread_barrier_wait(&g_block_bar); }
#define __syncthreads block_barrier
#include "sr_solar_plan.hpp"
namespace sr {
static inline double exp_bounded(double u) { return std::exp(u); }
#include "sr_solar_tile.inc"
#include "sr_solar_source.inc"
}
using namespace sr;

typedef long double LDb;

struct Case {
  int n_rows, n_k, n_pts, n_src;
  std::vector<double> A, U, w, sca, sun;
  std::vector<int> src;
};

static Case make_case(int n_rows, int n_k, int n_pts, unsigned seed) {
  std::mt19937_64 rng(seed);
  std::uniform_real_distribution<double> R(0.0, 1.0);
  Case c{n_rows, n_k, n_pts, std::max(n_rows / 2, 1), {}, {}, {}, {}, {}, {}};
  c.A.resize((size_t)n_k * n_pts);
  for (double &x : c.A) x = 0.15 + 1.35 * R(rng);
  c.U.assign((size_t)n_rows * n_k, 0.0);
  c.w.resize(n_rows);
  c.src.resize(n_rows);
  for (int r = 0; r < n_rows; ++r) {
    const int own = (int)(R(rng) * std::max((int)(0.8 * n_k), 1));
    double sum = 0.0;
    for (int k = std::max(r % 4 == 1 ? own - 3 : own, 0); k < n_k; ++k) sum += c.U[(size_t)r * n_k + k] = 0.2 + 0.8 * R(rng);
    const double target = std::exp(std::log(1e-3) + R(rng) * std::log(300.0 / 1e-3));
    for (int k = 0; k < n_k; ++k) c.U[(size_t)r * n_k + k] *= target / (1.5 * sum);
    c.w[r] = r % 7 == 3 ? 0.0 : 0.01 + 0.09 * R(rng); // (rows in shadow: their columns stay, and are not to be used)
    c.src[r] = (int)(R(rng) * c.n_src) % c.n_src;
  }
  if (n_rows > 2) {
    for (int k = 0; k < n_k; ++k) c.U[(size_t)2 * n_k + k] = 0.0; // a row without columns
    c.w[2] = 0.05;
  }
  if (n_rows > 5) c.U[(size_t)5 * n_k + (n_k - 1)] = 6000.0, c.w[5] = 0.05; // tau >= 900
  c.sca.resize((size_t)c.n_src * n_pts);
  for (double &x : c.sca) x = 1e-9 + 9.9e-8 * R(rng);
  c.sun.resize(n_pts);
  for (double &x : c.sun) x = 5.0 + 15.0 * R(rng);
  return c;
}

template <bool ACC, bool TRANS> static void run_kernel(const Case &c, bool full, std::vector<double> &emi, std::vector<double> &tr) {
  std::vector<int> off, ch;
  solar_chunk_lists(c.U.data(), c.w.data(), c.n_rows, c.n_k, full, off, ch);
  if (ch.empty()) ch.reserve(1); // (the entry keeps room for one element: the pointer is never read)
  const int n_pb = (c.n_pts + 255) / 256, n_tiles = (c.n_rows + kSolarRows - 1) / kSolarRows;
  launch((unsigned)((n_pb + 7) / 8 * 8) * n_tiles, 1, [&] {
    sr_solar_source_kernel<ACC, TRANS>(c.A.data(), c.n_k, c.n_pts, c.U.data(), c.w.data(), c.src.data(), c.n_rows, off.data(), ch.data(),
                                       c.sca.data(), c.sun.data(), emi.data(), TRANS ? tr.data() : nullptr);
  });
}

template <bool ACC, bool TRANS> static int check_case(const Case &c) {
  const size_t n_out = (size_t)c.n_rows * c.n_pts;
  auto pattern = [&](size_t at) { return ACC ? 1e-9 * (1.0 + (double)(at % 17)) : (double)NAN; };
  std::vector<double> emi[2], tr[2];
  for (int f = 0; f < 2; ++f) {
    emi[f].resize(n_out);
    tr[f].assign(n_out, NAN);
    for (size_t at = 0; at < n_out; ++at) emi[f][at] = pattern(at);
    run_kernel<ACC, TRANS>(c, f == 1, emi[f], tr[f]);
  }
  int bad = 0;
  if (std::memcmp(emi[0].data(), emi[1].data(), n_out * sizeof(double)) || (TRANS && std::memcmp(tr[0].data(), tr[1].data(), n_out * sizeof(double)))) {
    std::printf("sparse and full lists differ\n");
    ++bad;
  }
  const LDb eps = std::ldexp((LDb)1, -53);
  for (int r = 0; r < c.n_rows; ++r) {
    int K = 0;
    for (int k = 0; k < c.n_k; ++k) K += c.U[(size_t)r * c.n_k + k] != 0.0;
    for (int j = 0; j < c.n_pts; ++j) {
      const size_t at = (size_t)r * c.n_pts + j;
      LDb tau = 0;
      for (int k = 0; k < c.n_k; ++k) tau += (LDb)c.U[(size_t)r * c.n_k + k] * c.A[(size_t)k * c.n_pts + j];
      const bool lit = c.w[r] != 0.0 && tau < 700;
      const LDb T = lit ? std::exp(-tau) : 0, S = (LDb)c.sca[(size_t)c.src[r] * c.n_pts + j] * c.w[r] * c.sun[j] * T;
      const double v = emi[0][at], p = pattern(at);
      bool ok;
      if (ACC && c.w[r] == 0.0) ok = std::memcmp(&v, &p, sizeof v) == 0; // left as it was, bit for bit
      else if (ACC) ok = std::fabs((LDb)v - (p + S)) <= eps * S * ((K + 2) * tau + 8) + eps * (p + S);
      else if (!lit) ok = v == 0.0;
      else ok = std::fabs((LDb)v - S) <= eps * S * ((K + 2) * tau + 8);
      if (TRANS) {
        const double t = tr[0][at];
        ok = ok && (lit ? std::fabs((LDb)t - T) <= eps * T * ((K + 2) * tau + 5) : t == 0.0) && (K != 0 || !lit || t == 1.0);
      }
      if (!ok && bad++ < 10) std::printf("row %d point %d: %.17g, plain %.17Lg (tau %.6Lg)\n", r, j, v, S, tau);
    }
  }
  return bad;
}

int main() {
  pthread_barrier_init(&g_block_bar, nullptr, 256);
  const int rows[] = {1, 15, 17, 33, 65}, ks[] = {1, 3, 5, 13, 160}, pts[] = {1, 63, 65, 257};
  unsigned seed = 20261020;
  int bad = 0, n = 0;
  for (int a = 0; a < 5; ++a)
    for (int b = 0; b < 5; ++b)
      for (int d = 0; d < 4; ++d) {
        const Case c = make_case(rows[a], ks[b], pts[d], seed++);
        int bc = check_case<false, true>(c);
        const bool corner = (a == 0 || a == 4) && (b == 0 || b == 4) && (d == 0 || d == 3);
        if (corner || (a == 2 && b == 3 && d == 2)) bc += check_case<false, false>(c) + check_case<true, true>(c) + check_case<true, false>(c);
        if (bc) std::printf("n_rows %d n_k %d n_pts %d: FAILED\n", rows[a], ks[b], pts[d]);
        bad += bc;
        ++n;
      }
  for (int d = 1; d < 3; ++d) { // a second batch of chunks: 65 with every chunk listed
    const Case c = make_case(17, 259, pts[d], seed++);
    const int bc = check_case<false, true>(c) + check_case<true, false>(c);
    if (bc) std::printf("n_rows 17 n_k 259 n_pts %d: FAILED\n", pts[d]);
    bad += bc;
    ++n;
  }
  std::printf(bad ? "FAILED\n" : "all %d cases ok\n", n);
  return bad ? 1 : 0;
}
