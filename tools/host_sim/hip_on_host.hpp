// What a kernel's own text needs to compile and run as plain C++ on a machine without a GPU: the harnesses under
// tools/*_host include this, then the kernel files of spectrobot_amd/csrc inside namespace sr, and are built with
// AddressSanitizer and UBSan by tools/host_sim/run.sh -- indexing, plans, tile and row mapping, not the compiled gfx950
// code.  The reciprocal is an exact division.
// A block's 256 lanes run one after the other by default (kernels without a barrier).  With HOST_SIM_THREADED_LANES defined
// before the include a block is 256 threads, a wave's barrier a real barrier and v_mfma_f64_16x16x4 is emulated in its
// operand layout; without it the barrier is nothing and the MFMA returns its accumulator (text that is parsed, never run).
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <numeric>
#include <random>
#include <type_traits>
#include <vector>
#define __device__
#define __global__
#define __host__
#define __forceinline__ inline
#define __launch_bounds__(x)
#define __shared__ static
#define __builtin_amdgcn_fence(a, b) ((void)0)
#define SR_PIN_SCALARS(a, b) ((void)0)
using std::max;
using std::min;
struct Dim { unsigned x, y, z; };
typedef double v4d __attribute__((ext_vector_type(4)));
static inline double fma3(double a, double b, double c) { return std::fma(a, b, c); }
template <int NR> static inline double fast_rcp(double d) { return 1.0 / d; }
static Dim blockIdx{0, 0, 0}, blockDim{256, 1, 1}, gridDim{1, 1, 1};

#ifdef HOST_SIM_THREADED_LANES
#include <pthread.h>
static thread_local Dim threadIdx{0, 0, 0};
static pthread_barrier_t g_bar[4];
static double g_opA[4][64], g_opB[4][64];
static void wave_barrier() { pthread_barrier_wait(&g_bar[threadIdx.x >> 6]); }
// D[i][j] += sum_k A[i][k] B[k][j]; A: lane = 16 k + i, B: lane = 16 k + j, D: lane = 16 (i % 4) + j, register i / 4
static v4d mfma(double a, double b, v4d acc, int, int, int) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  g_opA[w][lane] = a;
  g_opB[w][lane] = b;
  wave_barrier();
  for (int r = 0; r < 4; ++r) {
    const int i = (lane >> 4) + 4 * r, j = lane & 15;
    double v = acc[r];
    for (int k = 0; k < 4; ++k) v = std::fma(g_opA[w][16 * k + i], g_opB[w][16 * k + j], v);
    acc[r] = v;
  }
  wave_barrier();
  return acc;
}
template <class F> struct Thunk { F f; unsigned tid; };
template <class F> static void *run_thread(void *p) {
  auto *t = static_cast<Thunk<F> *>(p);
  threadIdx.x = t->tid;
  t->f();
  return nullptr;
}
// f() for every lane of the blocks (x, 0, z), x < gx, z < gz
template <class F> static void launch(unsigned gx, unsigned gz, F f) {
  for (unsigned z = 0; z < gz; ++z)
    for (unsigned x = 0; x < gx; ++x) {
      blockIdx.x = x; blockIdx.z = z;
      for (auto &b : g_bar) pthread_barrier_init(&b, nullptr, 64);
      std::vector<pthread_t> th(256);
      std::vector<Thunk<F>> tk(256, Thunk<F>{f, 0});
      for (unsigned t = 0; t < 256; ++t) { tk[t].tid = t; pthread_create(&th[t], nullptr, run_thread<F>, &tk[t]); }
      for (auto &t : th) pthread_join(t, nullptr);
      for (auto &b : g_bar) pthread_barrier_destroy(&b);
    }
}
#else
static Dim threadIdx{0, 0, 0};
static void wave_barrier() {}
static v4d mfma(double, double, v4d acc, int, int, int) { return acc; }
template <class F> static void launch(unsigned gx, unsigned gz, F f) {
  for (unsigned z = 0; z < gz; ++z)
    for (unsigned x = 0; x < gx; ++x)
      for (unsigned t = 0; t < 256; ++t) {
        blockIdx.x = x; blockIdx.z = z; threadIdx.x = t;
        f();
      }
}
#endif
#define __builtin_amdgcn_wave_barrier wave_barrier
#define __builtin_amdgcn_mfma_f64_16x16x4f64 mfma

#include "sr_limb_plan.hpp"
#include "sr_limb_common.hpp"
