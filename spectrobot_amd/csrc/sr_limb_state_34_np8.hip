// sr_limb_state_34_np8.hip -- sr_limb_jac_state_kernel's instances for batches of 3 or 4 gases with 8 slots per block.
#include "sr_limb_state_unit.hpp"

namespace sr {

int launch_limb_jac_state_34_np8(const StateLaunch &L, const FoldBands &bd, int n_row_par, hipStream_t st) {
  return launch_state_instances<kLevelJacNPSmall>(L, bd, n_row_par, st, [&](auto &&f) { return by_ngas_of<3, 4>(L.o.n_gas, f); });
}

} // namespace sr
