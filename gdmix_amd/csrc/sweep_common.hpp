// sweep_common.hpp — what the two l2_reg_weight sweeps share on the device (re_sweep.hip, fe_sweep.hip): how many models a pass
// carries, the coefficient arrays of a pass, their slot-major transpose and the workspace it needs. The score kernels differ and stay
// with their units.
#pragma once
#include "re_internal.hpp"

namespace gdmix {

constexpr int SWEEP_MAX_KP = GDMIX_RE_SWEEP_MODELS_PER_PASS;   // models one pass carries (accumulators and gathers in flight: registers)

// the instantiation that carries k models, k <= SWEEP_MAX_KP
inline int sweep_width(int k) { return k <= 1 ? 1 : (k <= 2 ? 2 : (k <= 4 ? 4 : 8)); }

// bytes of the slot-major array of K models of P coefficients each (the widest pass decides)
inline size_t sweep_workspace_bytes(int64_t P, int K) { return (size_t)P * (size_t)sweep_width(K < SWEEP_MAX_KP ? K : SWEEP_MAX_KP) * 8; }

template <int KP>
struct SweepThetas { const double* p[KP]; };

// tm[s * KP + k] = theta_k[s]: coalesced reads of KP arrays, KP * 8 contiguous bytes written per slot
template <int KP>
__global__ __launch_bounds__(256) void sweep_transpose_kernel(SweepThetas<KP> T, int64_t P, double* __restrict__ tm) {
  const int64_t s = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= P) return;
  double v[KP];
#pragma unroll
  for (int k = 0; k < KP; ++k) v[k] = T.p[k][s];
#pragma unroll
  for (int k = 0; k < KP; ++k) tm[s * KP + k] = v[k];
}

}  // namespace gdmix
