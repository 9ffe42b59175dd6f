// sr_limb_dispatch.hpp -- the limb launchers' dispatch on the kernels' compile-time parameters, for every unit that
// launches limb kernels (sr_limb.hip, sr_limb_many.hip and the state units behind sr_limb_state_unit.hpp).
#pragma once
#include <type_traits>
#include "sr_limb_plan.hpp"

namespace sr {

// by_ngas_of<NG...>: f(integral_constant<int, NG>) for the one of the counts NG... that n_gas is.
// false: no instance for that count -- the launcher answers hipErrorInvalidValue, never a skipped launch.
template <int... NG, class F>
inline bool by_ngas_of(int n_gas, F &&f) {
  return ((n_gas == NG && (f(std::integral_constant<int, NG>{}), true)) || ...);
}
// by_ngas: a batch of n_gas gases, NG = 1..kFoldGasMax.  A larger batch has no instance behind it: launch_limb hands
// such a batch to sr_limb_many.hip before it comes here, the state kernel's launch goes by state units (state_unit,
// sr_limb.hip), and the entries of every other kernel refuse it (check_los with kFoldGasMax).
template <class F>
inline bool by_ngas(int n_gas, F &&f) { return by_ngas_of<1, 2, 3, 4>(n_gas, f); }
// by_ngas_many: the radiance kernels of five to eight gases, NG = n_gas
template <class F>
inline bool by_ngas_many(int n_gas, F &&f) { return by_ngas_of<5, 6, 7, 8>(n_gas, f); }
// ... the state kernel of five to eight gases: the next even NG, the slot behind the batch's gases a padding slot
template <class F>
inline bool by_ngas_state_many(int n_gas, F &&f) { return n_gas > kFoldGasMax && by_ngas_of<6, 8>(n_gas + (n_gas & 1), f); }
// by_level_np: f(integral_constant<int, NP>) for the accumulators per thread level_jac_np() / limb_parts_np() chose.
template <class F>
inline void by_level_np(int np, F &&f) {
  if (np == kLevelJacNPLarge) f(std::integral_constant<int, kLevelJacNPLarge>{});
  else f(std::integral_constant<int, kLevelJacNPSmall>{});
}
// by_flag: f(bool_constant<on>) for a kernel's boolean template parameter.
template <class F>
inline void by_flag(bool on, F &&f) {
  if (on) f(std::true_type{});
  else f(std::false_type{});
}
// by_jac_kinds: f(bool_constant<per-layer>, bool_constant<per-parameter>) for the Jacobians a one-pass call asks for.
// (false, false) does not exist as a kernel: a call without per-layer Jacobians is a per-parameter one.
template <class F>
inline void by_jac_kinds(bool layer, bool par, F &&f) {
  if (layer && par) f(std::true_type{}, std::true_type{});
  else if (layer) f(std::true_type{}, std::false_type{});
  else f(std::false_type{}, std::true_type{});
}

} // namespace sr
