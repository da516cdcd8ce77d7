// box_rule.hpp — what a box  lo <= theta <= hi  asks of one coefficient: the clamp, the binding set and the direction fix-up of the projected
// L-BFGS step (include/gdmix_fe.h, "(ABI 26) box constraints"; include/gdmix_re.h, "box constraints"). One copy, for the fixed effect's
// step (fe_qn.hip, BoxRule) and the random effect's per-entity solve (re_owlqn.hpp, BoxRule). Plain C++: the clamp returns the bound itself.
#pragma once
#include <hip/hip_runtime.h>

namespace gdmix {

__device__ __forceinline__ double box_clamp(double v, double lo, double hi) { return v < lo ? lo : (v > hi ? hi : v); }      // exactly the bound's double
// j is in the binding set: at a bound with the gradient pushing out of the box, or pinned
__device__ __forceinline__ bool box_binding(double g, double x, double lo, double hi) {
  return (x <= lo && g > 0.0) || (x >= hi && g < 0.0) || lo == hi;
}
// the direction entry as it is used: 0 on the binding set, and where x sits at a bound and d points out of the box
__device__ __forceinline__ double box_direction(double d, bool binding, double x, double lo, double hi) {
  return (binding || (x <= lo && d < 0.0) || (x >= hi && d > 0.0)) ? 0.0 : d;
}

}  // namespace gdmix
