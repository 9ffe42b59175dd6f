// sr_limb_many.hip -- the limb kernels' instances for batches of five to eight gases (kFoldGasMax < n_gas <= kLimbGasMax):
// the path-order radiance kernels (sr_limb_forward.inc) and the state kernel (sr_limb_state.inc), the same kernel text as
// the instances of one to four gases in sr_limb.hip and sr_limb_state_*.hip.  The state part is a state unit like those
// (sr_limb_state_unit.hpp).  No other limb kernel has an instance above four gases; their entries refuse such a batch
// (check_los with kFoldGasMax).
//
//   sr_limb_kernel<NG>, sr_limb_split_kernel<NG>   NG = 5, 6, 7, 8: one instance per gas count (eight small kernels)
//   sr_limb_jac_state_kernel<NG, 8, ...>           NG = 6 and 8: a batch of five gases runs the six-gas instance, one of
//                                                  seven the eight-gas one, the padding slot behind o.n_gas (see the
//                                                  kernel's comment); NP = 8 only -- the gas word holds 8 slots of 3 bits
#include "sr_limb_state_unit.hpp"

namespace sr {

#include "sr_limb_forward.inc"

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

// the state unit of n_gas = 5..8, NP = 8 (the plan of such a batch: state_gas_bits)
int launch_limb_jac_state_many(const StateLaunch &L, const FoldBands &bd, int n_row_par, hipStream_t st) {
  return launch_state_instances<kLevelJacNPSmall>(L, bd, n_row_par, st, [&](auto &&f) { return by_ngas_state_many(L.o.n_gas, f); });
}

} // namespace sr
