// re_eval_sum.hpp — what the two evaluation units (re_evaluate.hip: SSE; re_evaluate_poisson.hip: PL and the logistic loss LL) share: the shape of the fixed-shape
// fp64 sum of one term per sample — its constants, its block tree, the accumulator's geometry — stated HERE and only here; the error
// bounds of include/gdmix_re.h ("SSE", "poisson evaluation") are bounds of this shape.
//
//   lane sum      a lane adds at most EVAL_RUN = 2 048 terms in a row, at most EVAL_RUNS = 64 such sums in a row and at most 64 of those
//                 (fewer than 2^31 samples on 256 lanes). NaN scores are left out. The loops themselves stay in the kernels (sse_lane,
//                 eval_pl_big_kernel; the accumulators' eval_acc_add_kernel and eval_pl_acc_add_kernel with one level of runs): a loop
//                 shared as a template over the term compiled to other code for the Poisson kernel than the loop written in it
//                 (the placement of the last two additions, the order of two address registers), whichever way it returned its results.
//   block tree    the 256 lane sums of a workgroup -> one, 8 levels, the same tree whatever the data (eval_block_tree).
//   large entity  one workgroup, strided over its samples: lane sum, block tree.
//   accumulator   a batch: acc_groups(N) <= ACC_MAX_GROUPS workgroups, 16 samples per lane until the grid is full, so at most 2 048 terms
//                 per lane (one level of runs); block tree; the workgroup sums in ACC_PER_THREAD = 16-term runs and one more block tree
//                 (acc_group_tree). What becomes of that one sum is the metric's business (SSE: added; PL: TwoSum into a pair).
//                 Device state: a head of ACC_HEAD_BYTES for the metric's totals, then the batch's workgroup sums (acc_group_sums).
//   Longest chain of roundings: 2 048 + 64 + 64 + 8 + 16 + 8 + 3 < 4 096. The shape depends on the sample count alone: two runs give the
//   same bits. Never a floating-point atomic.
// Also here, for the units that rank (re_evaluate.hip, re_evaluate_weighted.hip): the sortable key of a score, the lane width of the
// four-per-wavefront kernels, the in-order workgroup scan of the reduce-then-scan passes and the lane sum over stored terms.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stddef.h>

namespace gdmix {

constexpr int EVAL_THREADS = 256;           // lanes of every workgroup that sums
constexpr int EVAL_RUN = 2048;              // terms a lane adds in a row,
constexpr int EVAL_RUNS = 64;               // sums of such runs it adds in a row
constexpr int ACC_MAX_GROUPS = 4096;        // workgroups of an accumulator batch (their sums: 16 per lane of the last tree)
constexpr int ACC_PER_THREAD = 16;
constexpr size_t ACC_HEAD_BYTES = 256;      // of the accumulator's device state: the metric's totals; the workgroup sums follow
constexpr size_t ACC_STATE_BYTES = ACC_HEAD_BYTES + (size_t)ACC_MAX_GROUPS * 8;
constexpr int64_t EVAL_LIMIT = (int64_t)1 << 31;   // an evaluation takes fewer samples and fewer entities than this
static_assert(ACC_MAX_GROUPS == EVAL_THREADS * ACC_PER_THREAD, "the last tree takes every workgroup sum");

// workgroups of a batch of N samples: 16 samples per lane until the grid is full
inline int64_t acc_groups(int64_t N) {
  const int64_t groups = (N + (int64_t)EVAL_THREADS * 16 - 1) / ((int64_t)EVAL_THREADS * 16);
  return groups > ACC_MAX_GROUPS ? ACC_MAX_GROUPS : groups;
}
inline double* acc_group_sums(void* state) { return reinterpret_cast<double*>(static_cast<char*>(state) + ACC_HEAD_BYTES); }

// the 256 lane sums of a workgroup -> one (the same tree whatever the data)
__device__ __forceinline__ double eval_block_tree(double v, double* lds) {
  const int t = threadIdx.x;
  lds[t] = v;
  __syncthreads();
  for (int off = EVAL_THREADS / 2; off > 0; off >>= 1) {
    if (t < off) lds[t] += lds[t + off];
    __syncthreads();
  }
  const double r = lds[0];
  __syncthreads();
  return r;
}

// the workgroup sums of an accumulator batch -> one sum (one workgroup of EVAL_THREADS lanes)
__device__ __forceinline__ double acc_group_tree(const double* __restrict__ group_sum, int groups, double* lds) {
  double v = 0.0;
  for (int j = 0; j < ACC_PER_THREAD; ++j) {
    const int i = threadIdx.x * ACC_PER_THREAD + j;
    if (i < groups) v += group_sum[i];
  }
  return eval_block_tree(v, lds);
}

// ---- what the ranking units share ------------------------------------------------------------------------------------------------------
constexpr uint32_t KEY_NAN = 0xFFFFFFFFu;   // the key of no score (it is the image of a NaN): sorts behind +inf, counted apart

// fp32 score -> uint32 that orders as the floats do; -0 and +0 get one key
__device__ __forceinline__ uint32_t sortable_key(float s) {
  if (s != s) return KEY_NAN;
  uint32_t b = __float_as_uint(s);
  if (s == 0.0f) b = 0u;
  return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
__device__ __forceinline__ uint64_t key33(float s, float y) {
  const uint32_t k = sortable_key(s);
  return ((uint64_t)k << 1) | (uint64_t)((k != KEY_NAN && y > 0.5f) ? 1u : 0u);
}
__device__ __forceinline__ int small_width(int nmax) { return nmax <= 16 ? 16 : (nmax <= 32 ? 32 : 64); }   // lanes per entity of the four-per-wavefront kernels

// inclusive scan of one state per thread in thread order (Hillis-Steele through LDS: 8 steps for 256 threads); S: a state with an
// associative rank_combine(a, b) (found by its argument type)
template <int THREADS, class S>
__device__ __forceinline__ S eval_block_scan(S v, S* lds) {
  const int t = threadIdx.x;
  lds[t] = v;
  __syncthreads();
  for (int off = 1; off < THREADS; off <<= 1) {
    S left = v;
    const bool take = t >= off;
    if (take) left = lds[t - off];
    __syncthreads();
    if (take) v = rank_combine(left, v);
    lds[t] = v;
    __syncthreads();
  }
  return v;
}

// the lane sum over stored terms (sse_lane's shape)
__device__ __forceinline__ double terms_lane(const double* __restrict__ terms, int64_t begin, int64_t end, int64_t stride) {
  double top = 0.0, total = 0.0, run = 0.0;
  int in_run = 0, runs = 0;
  for (int64_t i = begin; i < end; i += stride) {
    run += terms[i];
    if (++in_run == EVAL_RUN) {
      total += run; run = 0.0; in_run = 0;
      if (++runs == EVAL_RUNS) { top += total; total = 0.0; runs = 0; }
    }
  }
  return top + (total + run);
}

// a sum v added to an accumulator's (hi, lo) pair without losing the rounding error of the addition
__device__ __forceinline__ void acc_two_sum(double* pair, double v) {
  const double hi = pair[0], lo = pair[1];
  const double s = hi + v, bb = s - hi;
  const double err = (hi - (s - bb)) + (v - bb);   // TwoSum: hi + v = s + err exactly
  const double l2 = lo + err;
  const double h2 = s + l2;                        // FastTwoSum: |s| >= |l2|
  pair[0] = h2;
  pair[1] = l2 - (h2 - s);
}

}  // namespace gdmix
