// sr_limb_common.hpp -- what the limb recursion kernels share: a segment's attenuation, the options of a ray batch, the
// initial intensity, the band epilogue's record, the block order and the coefficient loads.  No HIP header of its own: the includer provides the
// qualifiers, blockIdx, fma3 and fast_rcp -- sr_device.hpp in the library, tools/host_sim/hip_on_host.hpp in a host build.
#pragma once
#include <cstddef>
#include "sr_constants.hpp"

namespace sr {

// One segment of the radiance recursion: t = exp(-tau), em1 = 1 - exp(-tau) and f = em1 / tau (1 where
// |tau| <= 1e-12) from ONE range reduction and polynomial: -tau = n ln2 + r, e^r - 1 = r (1 + r P(r)) =: pm1 with
// exp_bounded's polynomial, s = 2^n, t = s + s pm1, em1 = (1 - s) - s pm1 (n = 0: -pm1, exact for thin segments; no
// cancellation otherwise: |r| <= 0.35), the quotient by reciprocal + two Newton steps.  ~30 instructions for what
// exp() + expm1() + an IEEE division spent ~95 on: the recursion kernels are VALU-bound (64 rays x 160 segments
// x 1e5 points), sr_limb_kernel 1.5 -> see DESIGN.md.  tau may be negative (stimulated emission).
struct Atten {
  double t, em1, f, rtau; // rtau = 1 / tau (unspecified where |tau| <= 1e-12)
  double fp0;             // f'(tau) from the polynomial, valid where the reduction left n = 0 (atten_fprime)
  bool thin, n0;
};
__device__ inline Atten attenuation(double tau) {
  const double x = -tau;
  const double n = rint(x * 0x1.71547652b82fep+0);  // log2(e)
  double r = fma(-n, 0x1.62e42fefa39efp-1, x);      // ln2 hi
  r = fma(-n, 0x1.abc9e3b39803fp-56, r);            // ln2 lo
  double p = fma3(r, 0x1.ade156a5dcb37p-26, 0x1.28af3fca7ab0cp-22);
  p = fma3(r, p, 0x1.71dee623fde64p-19);
  p = fma3(r, p, 0x1.a01997c89e6b0p-16);
  p = fma3(r, p, 0x1.a01a014761f6ep-13);
  p = fma3(r, p, 0x1.6c16c1852b7b0p-10);
  p = fma3(r, p, 0x1.1111111122322p-7);
  p = fma3(r, p, 0x1.55555555502a1p-5);
  p = fma3(r, p, 0x1.5555555555511p-3);
  p = fma3(r, p, 0x1.000000000000bp-1);
  const double pm1 = r * fma(r, p, 1.0);
  const double s = ldexp(1.0, (int)fmin(fmax(n, -1100.0), 1100.0));
  Atten A;
  A.t = fma(s, pm1, s);
  A.em1 = fma(-s, pm1, 1.0 - s);
  A.thin = !(fabs(tau) > 1e-12);
  A.rtau = fast_rcp<2>(tau);
  A.f = A.thin ? 1.0 : A.em1 * A.rtau;
  A.n0 = n == 0.0;
  A.fp0 = fma(fabs(r) < 0x1p-4 ? p - 0x1.6p-50 : p, 1.0 - r, -1.0);
  return A;
}
// f'(tau) = (tau e^-tau - (1 - e^-tau)) / tau^2 of the same segment (-1/2 where |tau| <= 1e-12).  The closed form is a
// difference of nearly equal numbers for small tau (good to ~2^-53 / tau of f').  Where the reduction left n = 0
// (|tau| < ln2 / 2: r = -tau exactly, e^r = 1 + r + r^2 p) the same polynomial gives it without one:
// tau t - em1 = r^2 (p - 1 - r p), so f' = p (1 - r) - 1, p ~ 1/2.  The minimax fit's constant term is 11 ulp above 1/2
// (what the higher coefficients make up for towards |r| = 0.35): taken off below |r| = 1/16, where nothing makes up
// for it.  <= 3 units of 2^-53 below 1/64, <= 18 anywhere (checked on the host against long double).  Beyond n = 0
// the closed form loses under three bits.
__device__ __forceinline__ double atten_fprime(const Atten &A, double tau) {
  return A.thin ? -0.5 : (A.n0 ? A.fp0 : (tau * A.t - A.em1) * (A.rtau * A.rtau));
}

// Options of the device LOS pipeline (include/spectrobot_hip.h: sr_los_desc)
struct LimbOpts {
  int n_gas, n_seg_total, solo_absorption, init_mode, g_lo;
  double t_init, w0, gstep;
};

__device__ inline double limb_initial(const LimbOpts &o, const double *rad, size_t at, int j) {
  if (o.init_mode == 1) return rad[at];
  if (o.init_mode == 2) { // Calc_BB, spect_classes.py:1886
    const double nu = o.w0 + (double)(o.g_lo + j) * o.gstep;
    return 2 * kHcgs * (kCcgs * kCcgs) * (nu * nu * nu) / (exp(kC2 * nu / o.t_init) - 1);
  }
  return 0.0;
}

// Where the recursion kernels with a band epilogue (BANDS = true: sr_limb_fold_sens_lds_kernel, sr_limb_jac_state_kernel)
// find the instrument step's weight table and leave their partial sums; see the comment above the former.
struct FoldBands {
  const double *Wt;  // [band tiles][n_pts][16]
  const int *range;  // [n_bands][2]
  double *part;
  int n_bands;
};
constexpr int kLowresTables = 3; // the weight tables of a call with the instrument derivatives: value, d / d centre, d / d ln width
constexpr int kBandRow = 68; // doubles per row of a wave's tile of values (64 + padding: rows 8 banks apart)

// Block -> (point block, ray) of the ray-batch kernels.  With the rays on the grid's slow axis the resident blocks
// work on one or two rays at a time and every ray streams the coefficient tables from HBM again (64 rays: 4.0 GB
// fetched for 0.13 GB of tables, the kernel bound by that).  Here the point blocks are dealt round-robin to the
// eight XCDs (workgroup ids are) and ALL rays of a point block follow each other on one XCD: the 80 layers x 2 KB
// of a point block are read from HBM once and by the other rays from that XCD's L2.
__device__ inline bool limb_block(int n_pb, int n_rays, int &pb, int &ray) {
  const int id = blockIdx.x, q = id >> 3;
  ray = q % n_rays;
  pb = (id & 7) + 8 * (q / n_rays);
  return pb < n_pb;
}

// abs / emi of every gas at ofs = row n_pts + point: one segment's coefficients in the ray-batch kernels that load a
// segment ahead (where the loads are interleaved with those of the columns they are written out).
template <int NG>
__device__ __forceinline__ void limb_load_coef(const double *__restrict__ abs_c, const double *__restrict__ emi_c, size_t gstride,
                                               size_t ofs, double (&a)[NG], double (&e)[NG]) {
#pragma unroll
  for (int g = 0; g < NG; ++g) {
    a[g] = abs_c[g * gstride + ofs];
    e[g] = emi_c[g * gstride + ofs];
  }
}
// ... of an instance with more gas slots than the batch has gases (the state kernel above four gases: n_live gases in NG
// slots): a padding slot reads gas 0's rows, so that every load is valid; its column is an exact zero where it is used.
template <int NG>
__device__ __forceinline__ void limb_load_coef_padded(const double *__restrict__ abs_c, const double *__restrict__ emi_c,
                                                      size_t gstride, size_t ofs, int n_live, double (&a)[NG], double (&e)[NG]) {
#pragma unroll
  for (int g = 0; g < NG; ++g) {
    const size_t at = (g < n_live ? (size_t)g : (size_t)0) * gstride + ofs;
    a[g] = abs_c[at];
    e[g] = emi_c[at];
  }
}

} // namespace sr
