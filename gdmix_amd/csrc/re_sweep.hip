// re_sweep.hip — the device side of a sweep over l2_reg_weight inside one stage (gdmix_amd/sweep.py): K models trained on one packed
// batch score a second packed batch (the validation partition) in ONE pass over its non-zeros. The contracts are stated in
// include/gdmix_re.h ("sweep"); this unit is their only implementation and adds symbols only: no kernel of another unit changes.
//
//   join_entity_kernel    one thread per entity of the evaluation batch: has_model, and the intercept's place in the training batch's
//                         coefficient array.
//   join_feature_kernel   one thread per coefficient slot (feature) of the evaluation batch: its entity by the wavefront-wide bisection of
//                         ent_feat_ptr (re_search.hpp) re_score_kernel uses for samples (entities have 1 .. 65 k features: dealt by
//                         feature, not by entity), then a bisection of the same entity's ascending feature list in the training batch. Reads 4 B and
//                         writes 8 B per slot, plus log2(d_train) dependent 4 B probes into one entity's list (cached: neighbouring lanes
//                         probe the same list).
//   sweep_transpose_kernel (sweep_common.hpp, shared with fe_sweep.hip) the KP coefficient arrays of a pass -> one slot-major array
//                         [P_train][KP] (only when the caller gave a workspace: the K coefficients of a slot then are one contiguous KP * 8-byte read instead of KP distant lines).
//   sweep_score_kernel    one thread per sample, the entity search of re_score_kernel; (value, column, coefficient place) of a non-zero are
//                         loaded once and feed KP accumulators, KP in {1, 2, 4, 8} models per pass (more models: more passes). Row k of
//                         the output is bit for bit what re_score_kernel writes for the mapped coefficients of model k: the same
//                         products in the same order, each step one fused multiply-add (what the compiler makes of `acc += v * t` in
//                         re_score_kernel; stated explicitly here), a coefficient the training entity does not have enters as +0.0.
#include <stdint.h>
#include <math.h>

#include "re_search.hpp"
#include "sweep_common.hpp"

namespace gdmix {

// ---- join -----------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void join_entity_kernel(const int64_t* __restrict__ eval_feat_ptr, int64_t E_eval, const int64_t* __restrict__ train_feat_ptr,
                                                          int64_t E_train, int ic, const int32_t* __restrict__ train_entity,
                                                          int64_t* __restrict__ coef_pos, uint8_t* __restrict__ has_model) {
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= E_eval) return;
  const int64_t te = train_entity[e];
  const bool model = te >= 0 && te < E_train;
  has_model[e] = model ? 1 : 0;
  if (ic) coef_pos[eval_feat_ptr[e] + e] = model ? train_feat_ptr[te] + te : (int64_t)-1;
}

__global__ __launch_bounds__(256) void join_feature_kernel(const int64_t* __restrict__ eval_feat_ptr, const int32_t* __restrict__ eval_unique, int64_t E_eval,
                                                           int64_t D_eval, const int64_t* __restrict__ train_feat_ptr,
                                                           const int32_t* __restrict__ train_unique, int64_t E_train, int ic,
                                                           const int32_t* __restrict__ train_entity, int64_t* __restrict__ coef_pos) {
  const int lane = threadIdx.x & (WAVE - 1);
  const int64_t f = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t ff = f - lane;
  if (ff >= D_eval) return;
  const int64_t e = wave_entity_of(eval_feat_ptr, E_eval, D_eval, ff, f, lane);
  if (f >= D_eval) return;
  const int64_t te = train_entity[e];
  int64_t pos = -1;
  if (te >= 0 && te < E_train) {
    const int32_t want = eval_unique[f];
    const int64_t t0 = train_feat_ptr[te], t1 = train_feat_ptr[te + 1];
    int64_t lo = t0, hi = t1;       // the first j in [t0, t1) with train_unique[j] >= want
    while (lo < hi) {
      const int64_t mid = (lo + hi) >> 1;
      if (train_unique[mid] < want) lo = mid + 1; else hi = mid;
    }
    if (lo < t1 && train_unique[lo] == want) pos = lo + te * ic + ic;
  }
  coef_pos[f + e * ic + ic] = pos;
}

// ---- score ----------------------------------------------------------------------------------------------------------------------------
// the KP coefficients at place `pos` of the training batch's array (pos < 0: the entity has no coefficient there: +0.0, as the mapped array has)
template <int KP, bool SLOT_MAJOR>
__device__ __forceinline__ void sweep_fetch(const SweepThetas<KP>& T, const double* __restrict__ tm, int64_t pos, double (&t)[KP]) {
  if (pos < 0) {
#pragma unroll
    for (int k = 0; k < KP; ++k) t[k] = 0.0;
  } else if (SLOT_MAJOR) {
#pragma unroll
    for (int k = 0; k < KP; ++k) t[k] = tm[pos * KP + k];
  } else {
#pragma unroll
    for (int k = 0; k < KP; ++k) t[k] = T.p[k][pos];
  }
}

template <int KP, bool SLOT_MAJOR>
__global__ __launch_bounds__(256) void sweep_score_kernel(BatchDev B, int64_t E, int64_t N, int ic, SweepThetas<KP> T, const double* __restrict__ tm,
                                                          const int64_t* __restrict__ coef_pos, const uint8_t* __restrict__ has_model, int kn,
                                                          float* __restrict__ logit, float* __restrict__ per_coord) {
  const int lane = threadIdx.x & (WAVE - 1);
  const int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t gf = g - lane;
  if (gf >= N) return;
  const int64_t e = wave_entity_of(B.ent_row_ptr, E, N, gf, g, lane);
  if (g >= N) return;
  const int64_t r0 = B.ent_row_ptr[e], z0 = B.ent_nnz_ptr[e];
  const double off = (double)B.offset[g];
  const bool model = has_model ? has_model[e] != 0 : true;
  double z[KP];
#pragma unroll
  for (int k = 0; k < KP; ++k) z[k] = off;
  if (model) {
    const int64_t c0 = B.ent_feat_ptr[e] + e * ic;
    const int32_t* rp = B.row_ptr + r0 + e + (g - r0);
    const int k0 = rp[0], k1 = rp[1];
    const float* __restrict__ val = B.csr_val + z0;
    const int32_t* __restrict__ col = B.csr_col + z0;
    const int64_t* __restrict__ cp = coef_pos + c0 + ic;
    double acc[KP];
    if (ic) {
      sweep_fetch<KP, SLOT_MAJOR>(T, tm, coef_pos[c0], acc);
    } else {
#pragma unroll
      for (int k = 0; k < KP; ++k) acc[k] = 0.0;
    }
    int j = k0;
    for (; j + 2 <= k1; j += 2) {   // two non-zeros' gathers in flight (2 KP lines); every model's sum keeps the row's order
      const float v0 = val[j], v1 = val[j + 1];
      const int64_t p0 = cp[col[j]], p1 = cp[col[j + 1]];
      double t0[KP], t1[KP];
      sweep_fetch<KP, SLOT_MAJOR>(T, tm, p0, t0);
      sweep_fetch<KP, SLOT_MAJOR>(T, tm, p1, t1);
#pragma unroll
      for (int k = 0; k < KP; ++k) {
        acc[k] = fma((double)v0, t0[k], acc[k]);
        acc[k] = fma((double)v1, t1[k], acc[k]);
      }
    }
    if (j < k1) {
      const float v0 = val[j];
      double t0[KP];
      sweep_fetch<KP, SLOT_MAJOR>(T, tm, cp[col[j]], t0);
#pragma unroll
      for (int k = 0; k < KP; ++k) acc[k] = fma((double)v0, t0[k], acc[k]);
    }
#pragma unroll
    for (int k = 0; k < KP; ++k) z[k] = acc[k] + off;
  }
#pragma unroll
  for (int k = 0; k < KP; ++k) {
    if (k < kn) {
      logit[(int64_t)k * N + g] = (float)z[k];
      if (per_coord) per_coord[(int64_t)k * N + g] = (float)(z[k] - off);
    }
  }
}

// one pass: models [first, first + kn) of `thetas`, kn <= KP (the unused places of a pass read model `first` again and store nothing)
template <int KP>
static hipError_t sweep_pass(const BatchDev& B, int64_t E, int64_t N, int ic, const double* const* thetas, int kn, int64_t P_train, double* tm,
                             const int64_t* coef_pos, const uint8_t* has_model, float* logit, float* per_coord, hipStream_t s) {
  SweepThetas<KP> T;
  for (int k = 0; k < KP; ++k) T.p[k] = thetas[k < kn ? k : 0];
  const unsigned blocks = (unsigned)((N + 255) / 256);
  if (tm) {
    hipLaunchKernelGGL((sweep_transpose_kernel<KP>), dim3((unsigned)((P_train + 255) / 256)), dim3(256), 0, s, T, P_train, tm);
    hipLaunchKernelGGL((sweep_score_kernel<KP, true>), dim3(blocks), dim3(256), 0, s, B, E, N, ic, T, (const double*)tm, coef_pos, has_model, kn, logit, per_coord);
  } else {
    hipLaunchKernelGGL((sweep_score_kernel<KP, false>), dim3(blocks), dim3(256), 0, s, B, E, N, ic, T, (const double*)nullptr, coef_pos, has_model, kn, logit,
                       per_coord);
  }
  return hipGetLastError();
}

}  // namespace gdmix

using namespace gdmix;

extern "C" {

GDMIX_API int gdmix_re_join_features(gdmix_re_ctx* ctx, const gdmix_re_packed* eval, const gdmix_re_packed* train, int has_intercept,
                                     const int32_t* train_entity, int64_t* coef_pos, uint8_t* has_model, void* stream) {
  if (!ctx || !eval || !train) { set_error("gdmix_re_join_features: NULL argument"); return GDMIX_RE_EINVAL; }
  if (eval->E < 0 || eval->D < 0 || train->E < 0 || train->D < 0) { set_error("gdmix_re_join_features: bad batch"); return GDMIX_RE_EINVAL; }
  if (eval->E == 0) return GDMIX_RE_OK;
  if (!train_entity || !coef_pos || !has_model || !eval->ent_feat_ptr || (eval->D > 0 && !eval->unique_global)) {
    set_error("gdmix_re_join_features: NULL array");
    return GDMIX_RE_EINVAL;
  }
  if (train->E > 0 && (!train->ent_feat_ptr || (train->D > 0 && !train->unique_global))) { set_error("gdmix_re_join_features: NULL array of the training batch"); return GDMIX_RE_EINVAL; }
  if (eval->E >= ((int64_t)1 << 31) || train->E >= ((int64_t)1 << 31)) { set_error("gdmix_re_join_features: 2^31 entities or more"); return GDMIX_RE_ERANGE; }
  HIP_TRY(hipSetDevice(ctx->impl.device));
  hipStream_t s = static_cast<hipStream_t>(stream);
  HIP_TRY(join_unique(&ctx->impl, s));       // reads unique_global of both batches
  const int ic = has_intercept ? 1 : 0;
  hipLaunchKernelGGL(join_entity_kernel, dim3((unsigned)((eval->E + 255) / 256)), dim3(256), 0, s, (const int64_t*)eval->ent_feat_ptr, eval->E,
                     (const int64_t*)train->ent_feat_ptr, train->E, ic, train_entity, coef_pos, has_model);
  if (eval->D > 0) {
    const int64_t blocks = (eval->D + 255) / 256;
    if (blocks > 0x7fffffffLL) { set_error("gdmix_re_join_features: too many features"); return GDMIX_RE_ERANGE; }
    hipLaunchKernelGGL(join_feature_kernel, dim3((unsigned)blocks), dim3(256), 0, s, (const int64_t*)eval->ent_feat_ptr, (const int32_t*)eval->unique_global,
                       eval->E, eval->D, (const int64_t*)train->ent_feat_ptr, (const int32_t*)train->unique_global, train->E, ic, train_entity, coef_pos);
  }
  HIP_TRY(hipGetLastError());
  return GDMIX_RE_OK;
}

GDMIX_API size_t gdmix_re_score_models_workspace_bytes(int64_t P_train, int K) {
  if (P_train < 0 || K < 1) return 0;
  return sweep_workspace_bytes(P_train, K);
}

GDMIX_API int gdmix_re_score_models(gdmix_re_ctx* ctx, const gdmix_re_packed* eval, int has_intercept, const double* const* thetas, int K,
                                    int64_t P_train, const int64_t* coef_pos, const uint8_t* has_model, float* logit, float* logit_per_coord,
                                    void* workspace, size_t workspace_bytes, void* stream) {
  if (!ctx || !eval || !thetas || K < 1 || P_train < 0) { set_error("gdmix_re_score_models: bad argument"); return GDMIX_RE_EINVAL; }
  if (eval->E <= 0 || eval->N <= 0) return GDMIX_RE_OK;
  if (!logit || !coef_pos) { set_error("gdmix_re_score_models: NULL array"); return GDMIX_RE_EINVAL; }
  for (int k = 0; k < K; ++k)
    if (!thetas[k]) { set_error("gdmix_re_score_models: coefficient array %d is NULL", k); return GDMIX_RE_EINVAL; }
  if ((eval->N + 255) / 256 > 0x7fffffffLL) { set_error("gdmix_re_score_models: too many samples"); return GDMIX_RE_ERANGE; }
  if (workspace && workspace_bytes < gdmix_re_score_models_workspace_bytes(P_train, K)) {
    set_error("gdmix_re_score_models: workspace of %zu bytes, %zu needed (gdmix_re_score_models_workspace_bytes)", workspace_bytes,
              gdmix_re_score_models_workspace_bytes(P_train, K));
    return GDMIX_RE_ENOMEM;
  }
  HIP_TRY(hipSetDevice(ctx->impl.device));
  hipStream_t s = static_cast<hipStream_t>(stream);
  HIP_TRY(join_unique(&ctx->impl, s));
  const BatchDev B = batch_dev(eval);
  const int ic = has_intercept ? 1 : 0;
  double* tm = (workspace && P_train > 0) ? static_cast<double*>(workspace) : nullptr;
  const int64_t N = eval->N;
  for (int first = 0; first < K; first += SWEEP_MAX_KP) {
    const int kn = K - first < SWEEP_MAX_KP ? K - first : SWEEP_MAX_KP;
    float* lo = logit + (int64_t)first * N;
    float* pc = logit_per_coord ? logit_per_coord + (int64_t)first * N : nullptr;
    hipError_t rc;
    switch (sweep_width(kn)) {
      case 1: rc = sweep_pass<1>(B, eval->E, N, ic, thetas + first, kn, P_train, tm, coef_pos, has_model, lo, pc, s); break;
      case 2: rc = sweep_pass<2>(B, eval->E, N, ic, thetas + first, kn, P_train, tm, coef_pos, has_model, lo, pc, s); break;
      case 4: rc = sweep_pass<4>(B, eval->E, N, ic, thetas + first, kn, P_train, tm, coef_pos, has_model, lo, pc, s); break;
      default: rc = sweep_pass<8>(B, eval->E, N, ic, thetas + first, kn, P_train, tm, coef_pos, has_model, lo, pc, s); break;
    }
    HIP_TRY(rc);
  }
  return GDMIX_RE_OK;
}

}  // extern "C"
