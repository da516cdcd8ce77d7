// re_sweep.hip — the device side of a sweep over l2_reg_weight inside one stage (gdmix_amd/sweep.py): K models trained on one packed
// batch score a second packed batch (the validation partition) in ONE pass over its non-zeros. The contracts are stated in
// include/gdmix_re.h ("sweep"); this unit is their only implementation and adds symbols only: no kernel of another unit changes.
//
//   join_entity_kernel    one thread per entity of the evaluation batch: has_model, and the intercept's place in the training batch's
//                         coefficient array.
//   join_feature_kernel   one thread per coefficient slot (feature) of the evaluation batch: its entity by the wavefront-wide bisection of
//                         ent_feat_ptr re_score_kernel uses for samples (entities have 1 .. 65 k features: dealt by feature, not by
//                         entity), then a bisection of the same entity's ascending feature list in the training batch. Reads 4 B and
//                         writes 8 B per slot, plus log2(d_train) dependent 4 B probes into one entity's list (cached: neighbouring lanes
//                         probe the same list).
//   sweep_transpose_kernel the KP coefficient arrays of a pass -> one slot-major array [P_train][KP] (only when the caller gave a
//                         workspace: the K coefficients of a slot then are one contiguous KP * 8-byte read instead of KP distant lines).
//   sweep_score_kernel    one thread per sample, the entity search of re_score_kernel; (value, column, coefficient place) of a non-zero are
//                         loaded once and feed KP accumulators, KP in {1, 2, 4, 8} models per pass (more models: more passes). Row k of
//                         the output is bit for bit what re_score_kernel writes for the mapped coefficients of model k: the same
//                         products in the same order, each step one fused multiply-add (what the compiler makes of `acc += v * t` in
//                         re_score_kernel; stated explicitly here), a coefficient the training entity does not have enters as +0.0.
#include <stdint.h>
#include <math.h>

#include "re_internal.hpp"

namespace gdmix {

#define HIP_TRY(expr)                                                                        \
  do {                                                                                       \
    hipError_t _rc = (expr);                                                                 \
    if (_rc != hipSuccess) {                                                                 \
      set_error("%s failed: %s (%s:%d)", #expr, hipGetErrorString(_rc), __FILE__, __LINE__); \
      return GDMIX_RE_EHIP;                                                                  \
    }                                                                                        \
  } while (0)

constexpr int SWEEP_WAVE = 64;
constexpr int SWEEP_MAX_KP = GDMIX_RE_SWEEP_MODELS_PER_PASS;   // models one pass carries (accumulators and gathers in flight: registers)

// largest e in [lo, hi] with ptr[e] <= g (ptr[lo] <= g) — the two searches of re_score_kernel (re_solve.hip), restated: that unit
// keeps them to itself
__device__ __forceinline__ int64_t sweep_owner(const int64_t* __restrict__ ptr, int64_t lo, int64_t hi, int64_t g) {
  while (lo < hi) {
    const int64_t mid = (lo + hi + 1) >> 1;
    if (ptr[mid] <= g) lo = mid; else hi = mid - 1;
  }
  return lo;
}
// the same by a whole wavefront (uniform arguments, all lanes active): 64 probes per step
__device__ __forceinline__ int64_t sweep_wave_owner(const int64_t* __restrict__ ptr, int64_t lo, int64_t hi, int64_t g, int lane) {
  while (lo < hi) {
    const int64_t step = (hi - lo + SWEEP_WAVE - 1) / SWEEP_WAVE;
    const int64_t probe = lo + (int64_t)(lane + 1) * step;
    const bool le = ptr[probe < hi ? probe : hi] <= g;     // non-decreasing in the lane index
    const int c = __popcll(__ballot(le));
    const int64_t below = lo + (int64_t)c * step;
    const int64_t above = lo + (int64_t)(c + 1) * step;
    const int64_t nhi = (c < SWEEP_WAVE && above <= hi) ? above - 1 : hi;
    lo = below < hi ? below : hi;
    hi = (c == SWEEP_WAVE) ? lo : nhi;
  }
  return lo;
}
// the entity of item g of a wavefront's 64 consecutive items [gf, gf + 64) under the offsets `ptr` ([E + 1], items in all: M)
__device__ __forceinline__ int64_t sweep_entity_of(const int64_t* __restrict__ ptr, int64_t E, int64_t M, int64_t gf, int64_t g, int lane) {
  const int64_t gl = (gf + SWEEP_WAVE - 1 < M) ? gf + SWEEP_WAVE - 1 : M - 1;
  const int64_t e_lo = sweep_wave_owner(ptr, 0, E - 1, gf, lane);
  const int64_t w_hi = (e_lo + SWEEP_WAVE < E) ? e_lo + SWEEP_WAVE : E - 1;   // 64 items span at most 64 non-empty entities
  const int64_t e_hi = sweep_wave_owner(ptr, e_lo, (ptr[w_hi] > gl) ? w_hi : E - 1, gl, lane);
  return sweep_owner(ptr, e_lo, e_hi, g < M ? g : gl);
}

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
  const int lane = threadIdx.x & (SWEEP_WAVE - 1);
  const int64_t f = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t ff = f - lane;
  if (ff >= D_eval) return;
  const int64_t e = sweep_entity_of(eval_feat_ptr, E_eval, D_eval, ff, f, lane);
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
  const int lane = threadIdx.x & (SWEEP_WAVE - 1);
  const int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t gf = g - lane;
  if (gf >= N) return;
  const int64_t e = sweep_entity_of(B.ent_row_ptr, E, N, gf, g, lane);
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

static BatchDev sweep_batch_dev(const gdmix_re_packed* b) {
  BatchDev B;
  B.ent_row_ptr = b->ent_row_ptr; B.ent_nnz_ptr = b->ent_nnz_ptr; B.ent_feat_ptr = b->ent_feat_ptr; B.row_ptr = b->row_ptr;
  B.csr_col = b->csr_col; B.csr_val = b->csr_val; B.col_ptr = b->col_ptr; B.csc_row = b->csc_row; B.csc_val = b->csc_val;
  B.y = b->y; B.offset = b->offset; B.weight = b->weight; B.order = b->order;
  return B;
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
  const int kp = K < SWEEP_MAX_KP ? K : SWEEP_MAX_KP;
  return (size_t)P_train * (size_t)(kp <= 1 ? 1 : (kp <= 2 ? 2 : (kp <= 4 ? 4 : 8))) * 8;
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
  const BatchDev B = sweep_batch_dev(eval);
  const int ic = has_intercept ? 1 : 0;
  double* tm = (workspace && P_train > 0) ? static_cast<double*>(workspace) : nullptr;
  const int64_t N = eval->N;
  for (int first = 0; first < K; first += SWEEP_MAX_KP) {
    const int kn = K - first < SWEEP_MAX_KP ? K - first : SWEEP_MAX_KP;
    float* lo = logit + (int64_t)first * N;
    float* pc = logit_per_coord ? logit_per_coord + (int64_t)first * N : nullptr;
    hipError_t rc;
    if (kn == 1) rc = sweep_pass<1>(B, eval->E, N, ic, thetas + first, kn, P_train, tm, coef_pos, has_model, lo, pc, s);
    else if (kn == 2) rc = sweep_pass<2>(B, eval->E, N, ic, thetas + first, kn, P_train, tm, coef_pos, has_model, lo, pc, s);
    else if (kn <= 4) rc = sweep_pass<4>(B, eval->E, N, ic, thetas + first, kn, P_train, tm, coef_pos, has_model, lo, pc, s);
    else rc = sweep_pass<8>(B, eval->E, N, ic, thetas + first, kn, P_train, tm, coef_pos, has_model, lo, pc, s);
    HIP_TRY(rc);
  }
  return GDMIX_RE_OK;
}

}  // extern "C"
