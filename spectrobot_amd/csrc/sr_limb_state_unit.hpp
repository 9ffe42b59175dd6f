// sr_limb_state_unit.hpp -- what a translation unit with instances of sr_limb_jac_state_kernel is made of: the kernel's
// text (sr_limb_state.inc) and the one launch body (sr_limb_state_launch.inc), which a unit instantiates for its gas counts
// and its slots per block.  The instances are most of the library's compile time, so they are cut into units
// that compile side by side -- sr_limb_state_{12,34}_np{8,16}.hip for one to four gases, sr_limb_many.hip for five to
// eight -- and a unit is this header and one function; launch_limb_jac_state (sr_limb.hip) picks the unit.
#pragma once
#include <climits>
#include <cstdlib>

#include "sr_device.hpp"
#include "sr_kernels.hpp"
#include "sr_limb_dispatch.hpp"

// (the library pins the two scalars to registers through an empty asm; a host build defines the macro to nothing)
#define SR_PIN_SCALARS(a, b) asm volatile("" : "+s"(a), "+s"(b))

namespace sr {

#include "sr_limb_state.inc"
#include "sr_limb_state_launch.inc"

} // namespace sr
