// sr_constants.hpp -- the physical constants of the device code and of its host builds (no HIP).
#pragma once

namespace sr {

// spect_classes.py:39-47 (scipy.constants CODATA-2018)
constexpr double kTref = 296.0;
constexpr double kHpaToAtm = 0.00098692326671601;
constexpr double kHcgs = 6.62607015e-34 * 1.e7;
constexpr double kCcgs = 299792458.0 * 1.e2;
constexpr double kKcgs = 1.380649e-23 * 1.e7;
constexpr double kC2 = kHcgs * kCcgs / kKcgs;
constexpr double kAvogadro = 6.02214076e23;
constexpr double kPi = 3.141592653589793;
constexpr double kLn2 = 0.6931471805599453; // math.log(2.0)

} // namespace sr
