// Host build of sr_solar_jac_kernel's own text (spectrobot_amd/csrc/sr_solar_jac.inc on sr_solar_tile.inc with the chunk
// lists of sr_solar_plan.hpp, the files the library compiles) behind tools/host_sim/hip_on_host.hpp with threaded lanes: a block is
// 256 threads, its barrier a real barrier, v_mfma_f64_16x16x4 emulated in its operand layout.  Every buffer has exactly
// the size the entry gives it, so that AddressSanitizer sees an index beyond it; jac starts as a known pattern with more
// rows than parameters, so that the comparison sees a place that was not written and one that should not have been.
// Against plain loops in long double to the bound of tests/solar_jacobian_reference.py, on the panel of
// tests/test_gpu_solar_jacobian.py: n_rows 1, 15, 17, 33 x n_k 1, 3, 5, 13, 160 x n_pts 1, 63, 65, 257 with (n_rays, n_par)
// cycling through (1, 1), (3, 2), (NR + 1, 5), (9, 17) -- tile, chunk, store and ray-group edges --, du of both signs laid
// out as a mask's columns are, a parameter without columns and a ray whose q is zero; the overwrite instance on the whole
// panel (the widest shape on a diagonal of it, the (3, 2) shape in its place elsewhere), the accumulating one on a fifth
// of it; sparse lists against full lists, which must agree in every bit.  Behind the panel n_k = 259 at 17 rows x 63 and 65
// points, (NR + 1, 2), both instances: with every chunk listed a tile walks 65 chunks -- one whole batch of kSolarBatch,
// then a batch of one chunk padded to a pair, the last chunk of three k.  Built with AddressSanitizer and UBSan by tools/host_sim/run.sh
// solar_jacobian_host -- indexing, lists, tile, row and ray mapping on a machine without a GPU, not the compiled gfx950 code.
#define HOST_SIM_THREADED_LANES
#include "hip_on_host.hpp"
static pthread_barrier_t g_block_bar;
static void block_barrier() { pthread_barrier_wait(&g_block_bar); }
#define __syncthreads block_barrier
#include "sr_solar_plan.hpp"
namespace sr {
#include "sr_solar_tile.inc"
#include "sr_solar_jac.inc"
}
using namespace sr;

typedef long double LDb;

struct Case {
  int n_par, n_rows, n_k, n_pts, n_rays, n_jac_rows;
  std::vector<double> A, dU, Q;
  std::vector<int> slot;
};

static Case make_case(int n_rows, int n_k, int n_pts, int n_rays, int n_par, unsigned seed) {
  std::mt19937_64 rng(seed);
  std::uniform_real_distribution<double> R(0.0, 1.0);
  Case c{n_par, n_rows, n_k, n_pts, n_rays, n_par + 2, {}, {}, {}, {}};
  c.A.resize((size_t)n_k * n_pts);
  for (double &x : c.A) x = 0.15 + 1.35 * R(rng);
  c.dU.assign((size_t)n_par * n_rows * n_k, 0.0);
  for (int p = 0; p < n_par; ++p) {
    if (n_par > 1 && p == 1) continue; // a parameter without columns
    // a mask touches a few neighbouring k; the rows below it cross them (mu > 0), one row in four a few more (mu < 0)
    const int k0 = (int)(R(rng) * n_k), k1 = std::min(k0 + 1 + (int)(R(rng) * 3), n_k), r_top = 1 + (int)(R(rng) * n_rows);
    for (int r = 0; r < r_top; ++r)
      for (int k = k0; k < k1; ++k)
        if (R(rng) < 0.8) c.dU[((size_t)p * n_rows + r) * n_k + k] = (R(rng) < 0.5 ? -1.0 : 1.0) * (0.2 + 0.8 * R(rng));
  }
  c.Q.resize((size_t)n_rays * n_rows * n_pts);
  for (double &x : c.Q) x = (R(rng) < 0.5 ? -1.0 : 1.0) * (1e-9 + 9.9e-8 * R(rng));
  if (n_rays > 1)
    for (size_t at = 0; at < (size_t)n_rows * n_pts; ++at) c.Q[(size_t)n_rows * n_pts + at] = 0.0; // a ray that sees no row
  for (int p = 0; p < n_par; ++p) c.slot.push_back(n_par + 1 - p); // rows 2 .. n_par + 1, backwards: rows 0 and 1 are not named
  return c;
}

template <bool ACC> static void run_kernel(const Case &c, bool full, std::vector<double> &jac) {
  std::vector<int> off, ch;
  solar_jac_chunk_lists(c.dU.data(), c.n_par, c.n_rows, c.n_k, full, off, ch);
  if (ch.empty()) ch.reserve(1); // (the entry keeps room for one element: the pointer is never read)
  const int n_pb = (c.n_pts + 255) / 256, n_items = c.n_par * ((c.n_rays + kSolarJacRays - 1) / kSolarJacRays);
  launch((unsigned)((n_pb + 7) / 8 * 8) * n_items, 1, [&] {
    sr_solar_jac_kernel<kSolarJacRays, ACC>(c.A.data(), c.n_k, c.n_pts, c.dU.data(), c.n_par, c.n_rows, off.data(), ch.data(),
                                            c.Q.data(), c.n_rays, c.slot.data(), jac.data(), c.n_jac_rows);
  });
}

template <bool ACC> static int check_case(const Case &c) {
  const size_t n_out = (size_t)c.n_rays * c.n_jac_rows * c.n_pts;
  auto pattern = [&](size_t at) { return 1e-9 * (1.0 + (double)(at % 17)) * (at % 3 ? 1.0 : -1.0); };
  std::vector<double> jac[2];
  for (int f = 0; f < 2; ++f) {
    jac[f].resize(n_out);
    for (size_t at = 0; at < n_out; ++at) jac[f][at] = pattern(at);
    run_kernel<ACC>(c, f == 1, jac[f]);
  }
  int bad = 0;
  if (std::memcmp(jac[0].data(), jac[1].data(), n_out * sizeof(double))) {
    std::printf("sparse and full lists differ\n");
    ++bad;
  }
  const LDb eps = std::ldexp((LDb)1, -53);
  std::vector<int> row_of_slot((size_t)c.n_jac_rows, -1);
  for (int p = 0; p < c.n_par; ++p) row_of_slot[(size_t)c.slot[p]] = p;
  for (int y = 0; y < c.n_rays; ++y)
    for (int s = 0; s < c.n_jac_rows; ++s)
      for (int j = 0; j < c.n_pts; ++j) {
        const size_t at = ((size_t)y * c.n_jac_rows + s) * c.n_pts + j;
        const double v = jac[0][at], pat = pattern(at);
        const int p = row_of_slot[(size_t)s];
        bool ok;
        if (p < 0) {
          ok = std::memcmp(&v, &pat, sizeof v) == 0; // a row that is not named: left as it was, bit for bit
        } else {
          LDb sum = 0, b = 0;
          int R = 0;
          for (int r = 0; r < c.n_rows; ++r) {
            const double *ur = c.dU.data() + ((size_t)p * c.n_rows + r) * c.n_k;
            int K = 0;
            for (int k = 0; k < c.n_k; ++k) K += ur[k] != 0.0;
            R += K != 0;
          }
          for (int r = 0; r < c.n_rows; ++r) {
            const double *ur = c.dU.data() + ((size_t)p * c.n_rows + r) * c.n_k;
            LDb dtau = 0, mag = 0;
            int K = 0;
            for (int k = 0; k < c.n_k; ++k) {
              dtau += (LDb)ur[k] * c.A[(size_t)k * c.n_pts + j];
              mag += std::fabs((LDb)ur[k]) * c.A[(size_t)k * c.n_pts + j];
              K += ur[k] != 0.0;
            }
            const LDb qv = c.Q[((size_t)y * c.n_rows + r) * c.n_pts + j];
            sum += qv * dtau;
            b += std::fabs(qv) * (K + R + 2) * mag;
          }
          b *= eps;
          const LDb want = ACC ? (LDb)pat - sum : -sum;
          if (ACC) b += eps * std::fabs(want);
          ok = b > 0 ? std::fabs((LDb)v - want) <= b : (ACC ? std::memcmp(&v, &pat, sizeof v) == 0 : v == 0.0);
          if (!ok && bad < 10) std::printf("ray %d slot %d (parameter %d) point %d: %.17g, plain %.17Lg, bound %.3Lg\n", y, s, p, j, v, want, b);
        }
        if (!ok) ++bad;
      }
  return bad;
}

int main() {
  pthread_barrier_init(&g_block_bar, nullptr, 256);
  const int rows[] = {1, 15, 17, 33}, ks[] = {1, 3, 5, 13, 160}, pts[] = {1, 63, 65, 257};
  const int shape[4][2] = {{1, 1}, {3, 2}, {kSolarJacRays + 1, 5}, {9, 17}};
  unsigned seed = 20261020;
  int bad = 0, n = 0;
  for (int a = 0; a < 4; ++a)
    for (int b = 0; b < 5; ++b)
      for (int d = 0; d < 4; ++d) {
        int which = (n + n / 4) % 4;          // (every n_pts meets every shape)
        if (which == 3 && b != a) which = 1; // (the widest shape, 272 blocks of threads a launch, on a diagonal of the panel)
        const int *s = shape[which];
        const Case c = make_case(rows[a], ks[b], pts[d], s[0], s[1], seed++);
        int bc = check_case<false>(c);
        if (n % 5 == 0 || which == 3) bc += check_case<true>(c); // the accumulating instance on a fifth of the panel and the widest shape
        if (bc) std::printf("n_rows %d n_k %d n_pts %d n_rays %d n_par %d: FAILED\n", rows[a], ks[b], pts[d], s[0], s[1]);
        bad += bc;
        ++n;
      }
  for (int d = 1; d < 3; ++d) { // a second batch of chunks: 65 with every chunk listed
    const Case c = make_case(17, 259, pts[d], kSolarJacRays + 1, 2, seed++);
    const int bc = check_case<false>(c) + check_case<true>(c);
    if (bc) std::printf("n_rows 17 n_k 259 n_pts %d n_rays %d n_par 2: FAILED\n", pts[d], kSolarJacRays + 1);
    bad += bc;
    ++n;
  }
  std::printf(bad ? "FAILED\n" : "all %d cases ok\n", n);
  return bad ? 1 : 0;
}
