// fe_step_shares.hpp — the shares of a three-launch step of the fixed effect (fe_qn.hip, fe_tron.hip): K sums, value KMAX of them a maximum
// of non-negative terms, from the lanes of the products kernel's virtual blocks into acc_part[vb][K], and from there in one fixed order into
// the decision's LDS. Every addition has its place: lane loop (the caller's), wavefront, wavefronts 0..3 of the block, then per value four
// partial totals over the blocks b = g, g + 4, ... and these in order g = 0..3. nvb is a function of P alone, so a fit has the same bits on
// every run and on every worker.
#pragma once
#include "fe_internal.hpp"

namespace gdmix {

// products kernel, all threads of the block: lane k of a wavefront keeps value k, thread k adds the four wavefronts and writes acc_part[vb][k]
template <int K, int KMAX>
__device__ __forceinline__ void fe_shares_store(const double (&acc)[K], double* acc_part, int vb) {
  static_assert(K <= WAVE, "one lane per value");
  __shared__ double red[FE_WAVES][K];
  const int tid = threadIdx.x, lane = tid & (WAVE - 1), wv = tid >> 6;
  double mine = 0.0;
#pragma unroll
  for (int k = 0; k < K; ++k) {
    const double t = (k == KMAX) ? wave_max_nonneg(acc[k]) : wave_sum(acc[k]);
    if (lane == k) mine = t;
  }
  if (lane < K) red[wv][lane] = mine;
  __syncthreads();
  if (tid < K) {
    double s = red[0][tid];
#pragma unroll
    for (int w = 1; w < FE_WAVES; ++w) s = (tid == KMAX) ? fmax(s, red[w][tid]) : s + red[w][tid];
    acc_part[(size_t)vb * K + tid] = s;
  }
}

// decide kernel, all threads of its one block: value v of block b by thread (b % 4) * 64 + v, the four partial totals combined in order into
// tot (LDS). The caller's next __syncthreads() publishes tot.
template <int K, int KMAX>
__device__ __forceinline__ void fe_shares_total(const double* acc_part, int nvb, double (&tot)[K]) {
  static_assert(FE_THREADS == 4 * WAVE, "four groups of one lane per value");
  static_assert(K <= WAVE, "one lane per value");
  __shared__ double part4[4][WAVE];
  const int tid = threadIdx.x, v = tid & (WAVE - 1), g = tid >> 6;
  if (v < K) {
    double s = 0.0;
    int b = g;
    for (; b + 28 < nvb; b += 32) {   // eight loads in flight
      double t[8];
#pragma unroll
      for (int q = 0; q < 8; ++q) t[q] = acc_part[(size_t)(b + 4 * q) * K + v];
#pragma unroll
      for (int q = 0; q < 8; ++q) s = (v == KMAX) ? fmax(s, t[q]) : s + t[q];
    }
    for (; b < nvb; b += 4) {
      const double t = acc_part[(size_t)b * K + v];
      s = (v == KMAX) ? fmax(s, t) : s + t;
    }
    part4[g][v] = s;
  }
  __syncthreads();
  if (tid < K) {
    double s = part4[0][tid];
#pragma unroll
    for (int k = 1; k < 4; ++k) s = (tid == KMAX) ? fmax(s, part4[k][tid]) : s + part4[k][tid];
    tot[tid] = s;
  }
}

}  // namespace gdmix
