// re_evaluate_poisson.hip — the Poisson loss of a scored set on the device, per entity and over a whole stage: PL = sum_i (exp(s_i) - y_i s_i),
// the fp32 score and label widened to fp64 first. The contract (NaN handling, the trees, the bound, limits) is stated in include/gdmix_re.h,
// "poisson evaluation"; this unit is its only implementation. AUC and MSE stay in re_evaluate.hip, whose structs and entry points this does not touch.
//
//   eval_pl_small_kernel   entities of at most 64 samples (the testing knob of re_evaluate.hip, gdmix_re_set_eval_small_max, applies): a
//                          wavefront takes FOUR consecutive entities and chooses its width from their sizes as eval_small_kernel does (16, 32
//                          or 64 lanes per entity); lane i holds sample i; one fp64 xor-butterfly over the group (the same tree on every lane).
//   eval_pl_big_kernel     every larger entity: one workgroup, the fixed-shape sum of re_eval_sum.hpp.
//   accumulator            a batch: the accumulator's sum of re_eval_sum.hpp. The batches' sums are added to a (hi, lo) pair with TwoSum, so
//                          the stage's total is the rounded exact sum of its batches' sums, in whatever order they came.
// The shape of every sum is SSE's: the constants, the trees and the accumulator's geometry are the same code (re_eval_sum.hpp).
// Never a floating-point atomic; NaN scores are left out and counted (integer atomics: their sum has no order).
// The kernels and the entry points' bodies are templates over the per-sample term: PlTerm (gdmix_re_eval_pl_*) and LlTerm, the logistic loss
// (gdmix_re_eval_ll_*; include/gdmix_re.h, "ranking evaluation"). The Poisson instantiation does the operations it did as plain kernels, in their order.
#include <stdint.h>
#include <math.h>
#include <string.h>

#include "re_internal.hpp"
#include "re_eval_sum.hpp"

namespace gdmix {

// exp(s) - y s: exp_any (<= 0.98 ulp), then ONE rounding (the product is not rounded apart)
__device__ __forceinline__ double pl_term(float s, float y) {
  const double z = (double)s;
  return __builtin_fma(-(double)y, z, exp_any(z));
}

struct PlTerm { static __device__ __forceinline__ double term(float s, float y) { return pl_term(s, y); } };

// the logistic loss of a score: max(z, 0) - z [y > 0.5] + log(1 + exp(-|z|)) (include/gdmix_re.h, "ranking evaluation", log loss). The first two
// terms are formed as max(-z, 0) for a positive and max(z, 0) for a negative: the same number without a rounding, and no inf - inf.
// u = 1 + e is rounded before the logarithm, as in the solve kernels' logistic_terms: an absolute error, not a relative one
// (tools/logloss_check.c measures it).
__device__ __forceinline__ double ll_term(float s, float y) {
  const double z = (double)s;
  const double e = exp_neg(fabs(z));
  return fmax(y > 0.5f ? -z : z, 0.0) + log_1_2(1.0 + e);
}
struct LlTerm { static __device__ __forceinline__ double term(float s, float y) { return ll_term(s, y); } };

struct PlOutDev { double* pl; int32_t* n; int32_t* n_nan; };

template <class Term>
__global__ __launch_bounds__(64) void eval_pl_small_kernel(const int64_t* __restrict__ ent_row_ptr, int64_t E, const float* __restrict__ score,
                                                           const float* __restrict__ label, PlOutDev O, int small_max) {
  const int lane = threadIdx.x;
  const int64_t e0 = (int64_t)blockIdx.x * 4;
  const int64_t last = e0 + 4 < E ? e0 + 4 : E;
  const int64_t mine = ent_row_ptr[e0 + lane < last ? e0 + lane : last];   // lanes 0 .. 4 matter
  int64_t rp[5];
#pragma unroll
  for (int k = 0; k < 5; ++k) rp[k] = __shfl(mine, k);
  int nmax = 0;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int64_t n = rp[k + 1] - rp[k];
    if (n <= small_max && (int)n > nmax) nmax = (int)n;
  }
  const int W = nmax <= 16 ? 16 : (nmax <= 32 ? 32 : 64);   // lanes per entity; 64 / W entities per pass, W / 16 passes
  const int per_pass = 64 / W;
  const int g = lane / W, li = lane & (W - 1);
  for (int pass = 0; pass < W / 16; ++pass) {
    const int k = pass * per_pass + g;
    const int64_t start = k == 0 ? rp[0] : (k == 1 ? rp[1] : (k == 2 ? rp[2] : rp[3]));
    const int64_t end = k == 0 ? rp[1] : (k == 1 ? rp[2] : (k == 2 ? rp[3] : rp[4]));
    const int64_t n = end - start;
    const bool ent_ok = e0 + k < E && n <= small_max;
    const bool have = ent_ok && li < n;
    float s = 0.0f, y = 0.0f;
    if (have) { s = score[start + li]; y = label[start + li]; }
    const bool nan = have && s != s;
    double pl = (have && !nan) ? Term::term(s, y) : 0.0;
    uint32_t c = ((have && !nan) ? 1u : 0u) | ((nan ? 1u : 0u) << 16);   // two counts <= 64 in one word
    for (int off = 1; off < W; off <<= 1) {
      pl += __shfl_xor(pl, off);
      c += __shfl_xor(c, off);
    }
    if (ent_ok && li == 0) {
      if (O.pl) O.pl[e0 + k] = pl;
      if (O.n) O.n[e0 + k] = (int)(c & 0xFFFFu);
      if (O.n_nan) O.n_nan[e0 + k] = (int)(c >> 16);
    }
  }
}

// one workgroup per entity of the batch; those of the small path leave at once (the choice is uniform over the workgroup)
template <class Term>
__global__ __launch_bounds__(EVAL_THREADS) void eval_pl_big_kernel(const int64_t* __restrict__ ent_row_ptr, const float* __restrict__ score,
                                                                   const float* __restrict__ label, PlOutDev O, int small_max) {
  __shared__ double lds[EVAL_THREADS];
  __shared__ unsigned nan_count;
  const int64_t e = blockIdx.x;
  const int64_t r0 = ent_row_ptr[e], r1 = ent_row_ptr[e + 1];
  if (r1 - r0 <= small_max) return;
  if (threadIdx.x == 0) nan_count = 0u;
  __syncthreads();
  double top = 0.0, total = 0.0, run = 0.0;   // the lane sum of re_eval_sum.hpp, as sse_lane of re_evaluate.hip
  int in_run = 0, runs = 0;
  unsigned nans = 0u;
  for (int64_t i = r0 + threadIdx.x; i < r1; i += EVAL_THREADS) {
    const float s = score[i];
    if (s == s) run += Term::term(s, label[i]); else ++nans;
    if (++in_run == EVAL_RUN) {
      total += run; run = 0.0; in_run = 0;
      if (++runs == EVAL_RUNS) { top += total; total = 0.0; runs = 0; }
    }
  }
  if (nans) atomicAdd(&nan_count, nans);
  const double pl = eval_block_tree(top + (total + run), lds);   // (its barriers order the count too)
  if (threadIdx.x == 0) {
    if (O.pl) O.pl[e] = pl;
    if (O.n) O.n[e] = (int)((r1 - r0) - (int64_t)nan_count);
    if (O.n_nan) O.n_nan[e] = (int)nan_count;
  }
}

// the accumulator's device state: [0] hi, [1] lo of the total, [2] the NaN scores (u64) in its head; then a batch's workgroup sums.
// The lane loop is the accumulator's of re_eval_sum.hpp (one level of runs), as in eval_acc_add_kernel.
template <class Term>
__global__ __launch_bounds__(EVAL_THREADS) void eval_pl_acc_add_kernel(const float* __restrict__ score, const float* __restrict__ label, int64_t N,
                                                                       double* __restrict__ group_sum, unsigned long long* __restrict__ n_nan) {
  __shared__ double lds[EVAL_THREADS];
  const int64_t stride = (int64_t)gridDim.x * EVAL_THREADS;
  double total = 0.0, run = 0.0;
  int in_run = 0;
  unsigned nans = 0u;
  for (int64_t i = (int64_t)blockIdx.x * EVAL_THREADS + threadIdx.x; i < N; i += stride) {
    const float s = score[i];
    if (s == s) run += Term::term(s, label[i]); else ++nans;
    if (++in_run == EVAL_RUN) { total += run; run = 0.0; in_run = 0; }
  }
  if (nans) atomicAdd(n_nan, (unsigned long long)nans);
  const double v = eval_block_tree(total + run, lds);
  if (threadIdx.x == 0) group_sum[blockIdx.x] = v;
}

// the workgroup sums of a batch -> one sum, added to the accumulator's (hi, lo) without losing the rounding error of the addition
__global__ __launch_bounds__(EVAL_THREADS) void eval_pl_acc_sum_kernel(const double* __restrict__ group_sum, int groups, double* __restrict__ state) {
  __shared__ double lds[EVAL_THREADS];
  const double v = acc_group_tree(group_sum, groups, lds);
  if (threadIdx.x == 0) {
    const double hi = state[0], lo = state[1];
    const double s = hi + v, bb = s - hi;
    const double err = (hi - (s - bb)) + (v - bb);   // TwoSum: hi + v = s + err exactly
    const double l2 = lo + err;
    const double h2 = s + l2;                        // FastTwoSum: |s| >= |l2|
    state[0] = h2;
    state[1] = l2 - (h2 - s);
  }
}

// ---- the entry points' bodies: one per call, instantiated for the two terms ("gdmix_re_eval_pl" / "gdmix_re_eval_ll" in the messages) ------
template <class Term>
static int term_entities(const char* who, gdmix_re_ctx* ctx, const int64_t* ent_row_ptr, int64_t E, int64_t N, const float* score, const float* label,
                         const gdmix_re_eval_pl_out* out, void* stream) {
  if (!ctx || !out || E < 0 || N < 0) { set_error("%s_entities: bad argument", who); return GDMIX_RE_EINVAL; }
  if (N >= EVAL_LIMIT || E >= EVAL_LIMIT) {
    set_error("%s_entities: %lld samples / %lld entities; an evaluation takes fewer than 2^31 of each", who, (long long)N, (long long)E);
    return GDMIX_RE_ERANGE;
  }
  if (E == 0) return GDMIX_RE_OK;
  if (!ent_row_ptr || (N > 0 && (!score || !label))) { set_error("%s_entities: NULL input", who); return GDMIX_RE_EINVAL; }
  gdmix_ctx_impl* ci = &ctx->impl;
  hipStream_t s = static_cast<hipStream_t>(stream);
  HIP_TRY(hipSetDevice(ci->device));
  const int small_max = ci->eval_small_set ? ci->eval_small_max : 64;
  const PlOutDev O = {out->pl, out->n, out->n_nan};
  hipLaunchKernelGGL(eval_pl_small_kernel<Term>, dim3((unsigned)((E + 3) / 4)), dim3(64), 0, s, ent_row_ptr, E, score, label, O, small_max);
  hipLaunchKernelGGL(eval_pl_big_kernel<Term>, dim3((unsigned)E), dim3(EVAL_THREADS), 0, s, ent_row_ptr, score, label, O, small_max);
  HIP_TRY(hipGetLastError());
  return GDMIX_RE_OK;
}

static int term_acc_reset(const char* who, gdmix_re_ctx* ctx, gdmix_re_eval_pl_acc* acc, void* stream) {
  if (!ctx || !acc || !acc->state) { set_error("%s_acc_reset: bad argument (acc->state is required)", who); return GDMIX_RE_EINVAL; }
  static_assert(GDMIX_RE_EVAL_PL_STATE_BYTES >= ACC_STATE_BYTES && GDMIX_RE_EVAL_LL_STATE_BYTES == GDMIX_RE_EVAL_PL_STATE_BYTES, "the accumulator's device state");
  HIP_TRY(hipSetDevice(ctx->impl.device));
  HIP_TRY(hipMemsetAsync(acc->state, 0, ACC_HEAD_BYTES, static_cast<hipStream_t>(stream)));
  acc->count = 0;
  return GDMIX_RE_OK;
}

template <class Term>
static int term_acc_add(const char* who, gdmix_re_ctx* ctx, gdmix_re_eval_pl_acc* acc, const float* score, const float* label, int64_t N, void* stream) {
  if (!ctx || !acc || !acc->state || N < 0 || acc->count < 0) { set_error("%s_acc_add: bad argument", who); return GDMIX_RE_EINVAL; }
  if (N == 0) return GDMIX_RE_OK;
  if (acc->count + N >= EVAL_LIMIT) {
    set_error("%s_acc_add: %lld + %lld samples; an evaluation takes fewer than 2^31", who, (long long)acc->count, (long long)N);
    return GDMIX_RE_ERANGE;
  }
  if (!score || !label) { set_error("%s_acc_add: NULL input", who); return GDMIX_RE_EINVAL; }
  hipStream_t s = static_cast<hipStream_t>(stream);
  HIP_TRY(hipSetDevice(ctx->impl.device));
  const int64_t groups = acc_groups(N);
  double* state = static_cast<double*>(acc->state);
  double* group_sum = acc_group_sums(acc->state);
  hipLaunchKernelGGL(eval_pl_acc_add_kernel<Term>, dim3((unsigned)groups), dim3(EVAL_THREADS), 0, s, score, label, N, group_sum,
                     reinterpret_cast<unsigned long long*>(state + 2));
  hipLaunchKernelGGL(eval_pl_acc_sum_kernel, dim3(1), dim3(EVAL_THREADS), 0, s, (const double*)group_sum, (int)groups, state);
  HIP_TRY(hipGetLastError());
  acc->count += N;
  return GDMIX_RE_OK;
}

static int term_acc_finish(const char* who, gdmix_re_ctx* ctx, const gdmix_re_eval_pl_acc* acc, gdmix_re_eval_pl_totals* host_out, void* stream) {
  if (!ctx || !acc || !acc->state || !host_out || acc->count < 0) { set_error("%s_acc_finish: bad argument", who); return GDMIX_RE_EINVAL; }
  hipStream_t s = static_cast<hipStream_t>(stream);
  HIP_TRY(hipSetDevice(ctx->impl.device));
  double st[3] = {0.0, 0.0, 0.0};
  HIP_TRY(hipMemcpyAsync(st, acc->state, sizeof(st), hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  uint64_t n_nan = 0;
  memcpy(&n_nan, &st[2], 8);
  host_out->pl = st[0] + st[1];
  host_out->n_nan = (int64_t)n_nan;
  host_out->n = acc->count - (int64_t)n_nan;
  return GDMIX_RE_OK;
}

}  // namespace gdmix

using namespace gdmix;

extern "C" {

#define GDMIX_TERM_FAMILY(prefix, Term)                                                                                                               \
  GDMIX_API int prefix##_entities(gdmix_re_ctx* ctx, const int64_t* ent_row_ptr, int64_t E, int64_t N, const float* score, const float* label,        \
                                  const gdmix_re_eval_pl_out* out, void* stream) {                                                                    \
    return term_entities<Term>(#prefix, ctx, ent_row_ptr, E, N, score, label, out, stream);                                                           \
  }                                                                                                                                                   \
  GDMIX_API int prefix##_acc_reset(gdmix_re_ctx* ctx, gdmix_re_eval_pl_acc* acc, void* stream) { return term_acc_reset(#prefix, ctx, acc, stream); }  \
  GDMIX_API int prefix##_acc_add(gdmix_re_ctx* ctx, gdmix_re_eval_pl_acc* acc, const float* score, const float* label, int64_t N, void* stream) {     \
    return term_acc_add<Term>(#prefix, ctx, acc, score, label, N, stream);                                                                            \
  }                                                                                                                                                   \
  GDMIX_API int prefix##_acc_finish(gdmix_re_ctx* ctx, const gdmix_re_eval_pl_acc* acc, gdmix_re_eval_pl_totals* host_out, void* stream) {            \
    return term_acc_finish(#prefix, ctx, acc, host_out, stream);                                                                                      \
  }

GDMIX_TERM_FAMILY(gdmix_re_eval_pl, PlTerm)
GDMIX_TERM_FAMILY(gdmix_re_eval_ll, LlTerm)
#undef GDMIX_TERM_FAMILY

}  // extern "C"
