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

}  // namespace gdmix
