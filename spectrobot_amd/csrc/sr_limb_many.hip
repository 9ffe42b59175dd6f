// sr_limb_many.hip -- the limb kernels' instances for batches of five to eight gases (kFoldGasMax < n_gas <= kLimbGasMax):
// the path-order radiance kernels (sr_limb_forward.inc) and the state kernel (sr_limb_state.inc), the same kernel text as
// the instances of one to four gases in sr_kernels.hip.  A translation unit of its own: the state kernel's instances are
// most of that file's compile time, and these are compiled beside it, not behind it.  No other limb kernel has an
// instance above four gases; their entries refuse such a batch (check_los with kFoldGasMax).
//
//   sr_limb_kernel<NG>, sr_limb_split_kernel<NG>   NG = 5, 6, 7, 8: one instance per gas count (eight small kernels)
//   sr_limb_jac_state_kernel<NG, 8, ...>           NG = 6 and 8: a batch of five gases runs the six-gas instance, one of
//                                                  seven the eight-gas one, the padding slot behind o.n_gas (see the
//                                                  kernel's comment); NP = 8 only -- the gas word holds 8 slots of 3 bits
#include <climits>
#include <cstdlib>

#include "sr_device.hpp"
#include "sr_kernels.hpp"

namespace sr {

typedef double v4d __attribute__((ext_vector_type(4)));

#include "sr_limb_forward.inc"
#define SR_PIN_SCALARS(a, b) asm volatile("" : "+s"(a), "+s"(b))
#include "sr_limb_state.inc"

int launch_limb_many(const double *abs_c, const double *emi_c, int n_pts, int n_layers, int n_rays, const int *seg_off,
                     const int *seg_layer, const double *col, const LimbOpts &o, double *rad, hipStream_t st);
int launch_limb_jac_state_many(const StateLaunch &L, const FoldBands &bd, int n_row_par, hipStream_t st);
template <class F>
inline void by_flag(bool on, F &&f) {
  if (on) f(std::true_type{});
  else f(std::false_type{});
}
#include "sr_limb_state_launch.inc"

namespace {

// f(integral_constant<int, NG>) for the radiance kernels: NG = n_gas
template <class F>
inline bool by_ngas_many(int n_gas, F &&f) {
  switch (n_gas) {
    case 5: f(std::integral_constant<int, 5>{}); return true;
    case 6: f(std::integral_constant<int, 6>{}); return true;
    case 7: f(std::integral_constant<int, 7>{}); return true;
    case 8: f(std::integral_constant<int, 8>{}); return true;
    default: return false;
  }
}
// ... for the state kernel: the next even NG, the slot behind the batch's gases a padding slot
template <class F>
inline bool by_ngas_state_many(int n_gas, F &&f) {
  switch (n_gas) {
    case 5: case 6: f(std::integral_constant<int, 6>{}); return true;
    case 7: case 8: f(std::integral_constant<int, 8>{}); return true;
    default: return false;
  }
}
} // namespace

// launch_limb for n_gas = 5..8: the same two kernels by the same rule
int launch_limb_many(const double *abs_c, const double *emi_c, int n_pts, int n_layers, int n_rays, const int *seg_off,
                     const int *seg_layer, const double *col, const LimbOpts &o, double *rad, hipStream_t st) {
  if (n_pts <= 0 || n_rays <= 0) return 0;
  bool found;
  if (limb_launch_is_small(n_pts, n_rays)) {
    const dim3 gs(limb_grid((n_pts + 63) / 64, n_rays));
    found = by_ngas_many(o.n_gas, [&](auto ng) {
      hipLaunchKernelGGL(sr_limb_split_kernel<decltype(ng)::value>, gs, dim3(64 * kLimbParts), 0, st, abs_c, emi_c, n_pts, n_layers,
                         seg_off, seg_layer, col, o, n_rays, rad);
    });
  } else {
    const dim3 grid(limb_grid((n_pts + 255) / 256, n_rays));
    found = by_ngas_many(o.n_gas, [&](auto ng) {
      hipLaunchKernelGGL(sr_limb_kernel<decltype(ng)::value>, grid, dim3(256), 0, st, abs_c, emi_c, n_pts, n_layers, seg_off, seg_layer,
                         col, o, n_rays, rad);
    });
  }
  return found ? (int)hipGetLastError() : (int)hipErrorInvalidValue; // (a missing instance is an error, never a skipped launch)
}

// launch_limb_jac_state for n_gas = 5..8, from its prelude (the checks, the band scratch's layout, the rows cleared ahead
// of a launch with blocks per ray): the one body of sr_limb_state_launch.inc behind this unit's gas counts, NP = 8
int launch_limb_jac_state_many(const StateLaunch &L, const FoldBands &bd, int n_row_par, hipStream_t st) {
  if (L.ray_blk_off && L.np != kLevelJacNPSmall) return (int)hipErrorInvalidValue; // (the plan of such a batch: state_gas_bits)
  return launch_state_instances(L, bd, n_row_par, st, [&](auto &&f) { return by_ngas_state_many(L.o.n_gas, f); },
                                [&](auto &&f) { f(std::integral_constant<int, kLevelJacNPSmall>{}); });
}

} // namespace sr
