// fe_sweep.hip — the device side of a sweep over l2_reg_weight inside one fixed-effect stage (gdmix_amd/fe_model.py): K coefficient
// vectors trained on one shard score a second raw shard (the validation data) in ONE pass over its non-zeros. The contract is stated
// in include/gdmix_fe.h (gdmix_fe_score_models); this unit is its only implementation and adds symbols only: no kernel of another
// unit changes.
//
//   sweep_transpose_kernel      (sweep_common.hpp, shared with re_sweep.hip) the KP coefficient vectors of a pass -> one slot-major
//                               array [num_features + 1][KP] (only when the caller gave a workspace): the KP coefficients of a feature are one contiguous KP * 8-byte read — for
//                               KP = 8 half a 128-byte line — instead of KP lines KP arrays apart. The vectors are tiny next to X.
//   fe_sweep_score_kernel       one thread per sample straight off the reader's sample-major arrays, as fe_score_kernel (fe_solve.hip);
//                               (column, value) of a non-zero are loaded once and feed KP accumulators, KP in {1, 2, 4, 8} models per
//                               pass (more models: more passes). Row k of the output is bit for bit what fe_score_kernel writes for
//                               model k: the accumulator starts at the intercept, the row's products are added in the row's order,
//                               each step one fused multiply-add — what the compiler makes of `acc += (double)v * t` there
//                               (v_cvt_f64_f32 + v_fmac_f64 in its ISA, -ffp-contract=fast being hipcc's default), stated explicitly
//                               here so that the two kernels cannot drift apart. fe_score_kernel's "four at a time, then the tail" is
//                               load scheduling only: one accumulator, one order. Here 4 non-zeros are in flight for KP <= 2 and 2 for
//                               KP = 4, 8 (2 x 8 coefficient pairs + 8 accumulators = 48 VGPRs of doubles: full occupancy is kept).
#include <stdint.h>
#include <math.h>

#include "sweep_common.hpp"
#include "../../include/gdmix_fe.h"

namespace gdmix {

template <int KP, bool SLOT_MAJOR>
__device__ __forceinline__ void fe_sweep_fetch(const SweepThetas<KP>& T, const double* __restrict__ tm, int64_t j, double (&t)[KP]) {
  if (SLOT_MAJOR) {
#pragma unroll
    for (int k = 0; k < KP; ++k) t[k] = tm[j * KP + k];
  } else {
#pragma unroll
    for (int k = 0; k < KP; ++k) t[k] = T.p[k][j];
  }
}

template <int KP, bool SLOT_MAJOR>
__global__ __launch_bounds__(256) void fe_sweep_score_kernel(int64_t n, const int64_t* __restrict__ row_nnz_ptr, const int64_t* __restrict__ col_global,
                                                             const float* __restrict__ val, const float* __restrict__ offset, SweepThetas<KP> T,
                                                             const double* __restrict__ tm, int64_t D, int ic, int kn, float* __restrict__ score,
                                                             float* __restrict__ per_coord) {
  constexpr int U = KP <= 2 ? 4 : 2;      // non-zeros in flight
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  double acc[KP];
  if (ic) {
    fe_sweep_fetch<KP, SLOT_MAJOR>(T, tm, D, acc);
  } else {
#pragma unroll
    for (int k = 0; k < KP; ++k) acc[k] = 0.0;
  }
  if (row_nnz_ptr) {
    int64_t k = row_nnz_ptr[i];
    const int64_t k1 = row_nnz_ptr[i + 1];
    for (; k + U <= k1; k += U) {
      float v[U];
      int64_t c[U];
      double t[U][KP];
#pragma unroll
      for (int u = 0; u < U; ++u) { v[u] = val[k + u]; c[u] = col_global[k + u]; }
#pragma unroll
      for (int u = 0; u < U; ++u) fe_sweep_fetch<KP, SLOT_MAJOR>(T, tm, c[u], t[u]);
#pragma unroll
      for (int u = 0; u < U; ++u) {
#pragma unroll
        for (int m = 0; m < KP; ++m) acc[m] = fma((double)v[u], t[u][m], acc[m]);
      }
    }
    for (; k < k1; ++k) {
      const float v = val[k];
      double t[KP];
      fe_sweep_fetch<KP, SLOT_MAJOR>(T, tm, col_global[k], t);
#pragma unroll
      for (int m = 0; m < KP; ++m) acc[m] = fma((double)v, t[m], acc[m]);
    }
  }
  const double off = offset ? (double)offset[i] : 0.0;
#pragma unroll
  for (int m = 0; m < KP; ++m) {
    if (m < kn) {
      const double z = acc[m] + off;
      score[(int64_t)m * n + i] = (float)z;
      if (per_coord) per_coord[(int64_t)m * n + i] = (float)(z - off);
    }
  }
}

// one pass: models [0, kn) of `thetas`, kn <= KP (the unused places of a pass read model 0 again and store nothing)
template <int KP>
static hipError_t fe_sweep_pass(int64_t n, const int64_t* rp, const int64_t* col, const float* val, const float* offset, const double* const* thetas,
                                int kn, int64_t D, int ic, double* tm, float* score, float* per_coord, hipStream_t s) {
  SweepThetas<KP> T;
  for (int k = 0; k < KP; ++k) T.p[k] = thetas[k < kn ? k : 0];
  const unsigned blocks = (unsigned)((n + 255) / 256);
  if (tm) {
    const int64_t P = D + ic;
    hipLaunchKernelGGL((sweep_transpose_kernel<KP>), dim3((unsigned)((P + 255) / 256)), dim3(256), 0, s, T, P, tm);
    hipLaunchKernelGGL((fe_sweep_score_kernel<KP, true>), dim3(blocks), dim3(256), 0, s, n, rp, col, val, offset, T, (const double*)tm, D, ic, kn, score,
                       per_coord);
  } else {
    hipLaunchKernelGGL((fe_sweep_score_kernel<KP, false>), dim3(blocks), dim3(256), 0, s, n, rp, col, val, offset, T, (const double*)nullptr, D, ic, kn, score,
                       per_coord);
  }
  return hipGetLastError();
}

}  // namespace gdmix

using namespace gdmix;

extern "C" {

GDMIX_API size_t gdmix_fe_score_models_workspace_bytes(int64_t num_features, int K) {
  if (num_features < 0 || K < 1) return 0;
  return sweep_workspace_bytes(num_features + 1, K);
}

GDMIX_API int gdmix_fe_score_models(gdmix_re_ctx* ctx, int64_t n, const int64_t* row_nnz_ptr, const int64_t* col_global, const float* val,
                                    const float* offset, const double* const* thetas, int K, int64_t num_features, int has_intercept,
                                    float* score, float* per_coord, void* workspace, size_t workspace_bytes, void* stream) {
  if (!ctx || n < 0 || !thetas || K < 1 || num_features < 0) { set_error("gdmix_fe_score_models: bad argument"); return GDMIX_RE_EINVAL; }
  if (row_nnz_ptr && (!col_global || !val)) { set_error("gdmix_fe_score_models: row_nnz_ptr without col_global / val"); return GDMIX_RE_EINVAL; }
  for (int k = 0; k < K; ++k)
    if (!thetas[k]) { set_error("gdmix_fe_score_models: coefficient array %d is NULL", k); return GDMIX_RE_EINVAL; }
  if (n == 0) return GDMIX_RE_OK;
  if (!score) { set_error("gdmix_fe_score_models: score is NULL"); return GDMIX_RE_EINVAL; }
  if ((n + 255) / 256 > 0x7fffffffLL) { set_error("gdmix_fe_score_models: too many samples for one launch"); return GDMIX_RE_ERANGE; }
  const int ic = has_intercept ? 1 : 0;
  if (num_features + ic < 1) { set_error("gdmix_fe_score_models: a model without coefficients"); return GDMIX_RE_EINVAL; }
  if (workspace && workspace_bytes < gdmix_fe_score_models_workspace_bytes(num_features, K)) {
    set_error("gdmix_fe_score_models: workspace of %zu bytes, %zu needed (gdmix_fe_score_models_workspace_bytes)", workspace_bytes,
              gdmix_fe_score_models_workspace_bytes(num_features, K));
    return GDMIX_RE_ENOMEM;
  }
  HIP_TRY(hipSetDevice(ctx->impl.device));
  hipStream_t s = static_cast<hipStream_t>(stream);
  double* tm = static_cast<double*>(workspace);
  for (int first = 0; first < K; first += SWEEP_MAX_KP) {
    const int kn = K - first < SWEEP_MAX_KP ? K - first : SWEEP_MAX_KP;
    float* sc = score + (int64_t)first * n;
    float* pc = per_coord ? per_coord + (int64_t)first * n : nullptr;
    hipError_t rc;
    switch (sweep_width(kn)) {
      case 1: rc = fe_sweep_pass<1>(n, row_nnz_ptr, col_global, val, offset, thetas + first, kn, num_features, ic, tm, sc, pc, s); break;
      case 2: rc = fe_sweep_pass<2>(n, row_nnz_ptr, col_global, val, offset, thetas + first, kn, num_features, ic, tm, sc, pc, s); break;
      case 4: rc = fe_sweep_pass<4>(n, row_nnz_ptr, col_global, val, offset, thetas + first, kn, num_features, ic, tm, sc, pc, s); break;
      default: rc = fe_sweep_pass<8>(n, row_nnz_ptr, col_global, val, offset, thetas + first, kn, num_features, ic, tm, sc, pc, s); break;
    }
    HIP_TRY(rc);
  }
  return GDMIX_RE_OK;
}

}  // extern "C"
