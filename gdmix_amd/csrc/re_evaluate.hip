// re_evaluate.hip — the stage metric on the device: exact AUC (as integers) and MSE, per entity and over a whole stage.
// The contract (key, twoU, SSE, NaN handling, limits) is stated in include/gdmix_re.h; this unit is its only implementation.
//
//   eval_small_kernel     entities of at most 64 samples, no sort: a wavefront takes FOUR consecutive entities of the batch and
//                         chooses its width from their sizes (ent_row_ptr; no classify pass): all four <= 16 samples -> one pass,
//                         an entity per 16-lane row; all <= 32 -> two passes, an entity per row pair; else four passes, an entity
//                         per wavefront (larger entities are left to the sort path). Lane i holds sample i. The negatives' 32-bit
//                         keys go through LDS (every other lane stores a key no score has): a lane reads its group's W keys with
//                         W/4 ds_read_b128 — 4 LDS reads for a row against 15 two-register DPP rotates, and one code path for all
//                         three widths, which is why it is LDS and not DPP — and counts (k_j < k_i) + (k_j <= k_i). Integer and
//                         fp64 xor-butterflies over the group (the same tree on every lane: a fixed order). 8 B read per sample,
//                         no atomics, nothing written but the per-entity outputs. One dependent load chain per pass (row pointers ->
//                         samples); a C2 wavefront whose four entities have at most 16 samples is one pass.
//   sort path             entities above the small limit, and the global metric: composite key segment << 33 | key33, rocPRIM radix
//                         sort over the bits in use (the only vendor call besides the prefix sum that numbers the large entities),
//                         then the rank-sum pass, reduce-then-scan in two launches (rank_reduce_kernel, rank_scan_kernel): no
//                         workgroup waits for another. Its time is the radix sort's passes over 8 B keys (profiles/evaluate_bench.txt).
//   SSE                   the fixed-shape sum of re_eval_sum.hpp over the non-negative fp64 terms (y - s)^2 (a large entity: one workgroup;
//                         the accumulator: its batches' sums are added in the order they were given). Relative error below 2.5e-13.
//   ranking               gdmix_re_eval_topk_entities (include/gdmix_re.h, "ranking evaluation"): the four integers of precision@k for up to
//                         four k. topk_small_kernel: eval_small_kernel's geometry with the keys of all valid samples through LDS, and that
//                         kernel's outputs from the same read when the caller wants them; topk_big_kernel: a workgroup per large entity on
//                         its sorted segment (binary searches for the tie group of the cut). The sort path's steps up to the sorted keys
//                         (sort_big_entities) and from them to the AUC outputs (rank_and_finish) are shared by the two entry points.
#include <stdint.h>
#include <math.h>

#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_scan.hpp>

#include "re_internal.hpp"
#include "re_eval_sum.hpp"

namespace gdmix {

constexpr uint32_t KEY_NAN = 0xFFFFFFFFu;   // the key of no score (it is the image of a NaN): sorts behind +inf, counted apart
constexpr int RANK_THREADS = 256, RANK_ITEMS = 16, RANK_TILE = RANK_THREADS * RANK_ITEMS;

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
__device__ __forceinline__ double sq_err(float s, float y) {
  const double d = (double)y - (double)s;
  return d * d;
}
// one fp64 division of exactly converted integers (exact below 2^26 samples; the host redoes larger entities)
__device__ __forceinline__ double auc_of(uint64_t two_u, int64_t n_pos, int64_t n_neg) {
  if (n_pos == 0 || n_neg == 0) return __longlong_as_double(0x7ff8000000000000ll);
  return (double)two_u / (2.0 * (double)n_pos * (double)n_neg);
}

struct EvalOutDev {
  uint64_t* two_u; int32_t* n_pos; int32_t* n_neg; int32_t* n_nan; double* sse; double* auc;
};
__device__ __forceinline__ void write_entity(const EvalOutDev& O, int64_t e, uint64_t two_u, int n_pos, int n_neg, int n_nan, double sse) {
  if (O.two_u) O.two_u[e] = two_u;
  if (O.n_pos) O.n_pos[e] = n_pos;
  if (O.n_neg) O.n_neg[e] = n_neg;
  if (O.n_nan) O.n_nan[e] = n_nan;
  if (O.sse) O.sse[e] = sse;
  if (O.auc) O.auc[e] = auc_of(two_u, n_pos, n_neg);
}

// ---- small entities ---------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void eval_small_kernel(const int64_t* __restrict__ ent_row_ptr, int64_t E, const float* __restrict__ score,
                                                        const float* __restrict__ label, EvalOutDev O, int small_max) {
  __shared__ __attribute__((aligned(16))) uint32_t neg_keys[64];
  const int lane = threadIdx.x;
  const int64_t e0 = (int64_t)blockIdx.x * 4;
  // the five row pointers of the wavefront's four entities (clamped at the end of the batch: an entity of no samples)
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
  const int g = lane / W, li = lane & (W - 1), base = lane & ~(W - 1);
  for (int pass = 0; pass < W / 16; ++pass) {
    const int k = pass * per_pass + g;
    const int64_t start = k == 0 ? rp[0] : (k == 1 ? rp[1] : (k == 2 ? rp[2] : rp[3]));
    const int64_t end = k == 0 ? rp[1] : (k == 1 ? rp[2] : (k == 2 ? rp[3] : rp[4]));
    const int64_t n = end - start;
    const bool ent_ok = e0 + k < E && n <= small_max;
    const bool have = ent_ok && li < n;
    float s = 0.0f, y = 0.0f;
    if (have) { s = score[start + li]; y = label[start + li]; }
    const uint32_t key = have ? sortable_key(s) : KEY_NAN;
    const bool nan = have && key == KEY_NAN;
    const bool pos = have && !nan && y > 0.5f;
    const bool neg = have && !nan && !pos;
    neg_keys[lane] = neg ? key : KEY_NAN;
    __syncthreads();
    uint32_t cnt = 0;
    for (int j = 0; j < W; j += 4) {
      const uint4 v = *reinterpret_cast<const uint4*>(&neg_keys[base + j]);
      cnt += (uint32_t)(v.x < key) + (uint32_t)(v.x <= key) + (uint32_t)(v.y < key) + (uint32_t)(v.y <= key) +
             (uint32_t)(v.z < key) + (uint32_t)(v.z <= key) + (uint32_t)(v.w < key) + (uint32_t)(v.w <= key);
    }
    __syncthreads();   // the next pass overwrites the keys
    // two packed integer sums (2 * less + equal <= 2 048 and the counts <= 64 fit 16 bits each) and the fp64 sum, over the group
    uint32_t a = (pos ? cnt : 0u) | ((pos ? 1u : 0u) << 16);
    uint32_t b = (neg ? 1u : 0u) | ((nan ? 1u : 0u) << 16);
    double sse = (have && !nan) ? sq_err(s, y) : 0.0;
    for (int off = 1; off < W; off <<= 1) {
      a += __shfl_xor(a, off);
      b += __shfl_xor(b, off);
      sse += __shfl_xor(sse, off);
    }
    if (ent_ok && li == 0) write_entity(O, e0 + k, a & 0xFFFFu, (int)(a >> 16), (int)(b & 0xFFFFu), (int)(b >> 16), sse);
  }
}

// ---- the large entities of a batch: numbering, keys --------------------------------------------------------------------------------
// mark[e] = 1 << 32 | n_e for an entity of the sort path, 0 otherwise: ONE prefix sum numbers them (high half) and lays their samples
// out (low half; the batch has fewer than 2^31 samples)
__global__ void eval_mark_kernel(const int64_t* __restrict__ ent_row_ptr, int64_t E, int small_max, int64_t* __restrict__ mark) {
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e > E) return;
  int64_t v = 0;
  if (e < E) {
    const int64_t n = ent_row_ptr[e + 1] - ent_row_ptr[e];
    if (n > small_max) v = ((int64_t)1 << 32) | n;
  }
  mark[e] = v;
}
__global__ void eval_big_list_kernel(const int64_t* __restrict__ mark, const int64_t* __restrict__ offs, int64_t E, int32_t* __restrict__ big_list,
                                     int32_t* __restrict__ big_off) {
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= E || mark[e] == 0) return;
  const int64_t o = offs[e];
  big_list[o >> 32] = (int32_t)e;
  big_off[o >> 32] = (int32_t)(o & 0xFFFFFFFFll);
}
// one thread per sample of a large entity, in the entities' order: segment = the entity's number among the large ones
__global__ void eval_big_keys_kernel(const int64_t* __restrict__ ent_row_ptr, const int32_t* __restrict__ big_list, const int32_t* __restrict__ big_off,
                                     int nbig, int64_t M, const float* __restrict__ score, const float* __restrict__ label, uint64_t* __restrict__ keys) {
  const int64_t m = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (m >= M) return;
  int lo = 0, hi = nbig - 1;   // the last b with big_off[b] <= m
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if ((int64_t)big_off[mid] <= m) lo = mid; else hi = mid - 1;
  }
  const int64_t i = ent_row_ptr[big_list[lo]] + (m - big_off[lo]);
  keys[m] = ((uint64_t)lo << 33) | key33(score[i], label[i]);
}

// ---- rank-sum pass over sorted keys --------------------------------------------------------------------------------------------------
// With C the running count of negatives, a positive at index i adds (C[i] - C[ss]) + (C[gs] - C[ss]): ss the start of its segment,
// gs the start of its tie group (equal segment and score; a tie's negatives sort in front of its positives). The scanned state of a
// stretch of elements: n its negatives, g / s the negatives in front of its last tie-group / segment head (flags: it has one).
struct RankState { uint32_t n, g, s, f; };
__device__ __forceinline__ RankState rank_combine(const RankState& a, const RankState& b) {
  RankState r;
  r.n = a.n + b.n;
  r.g = (b.f & 1u) ? a.n + b.g : a.g;
  r.s = (b.f & 2u) ? a.n + b.s : a.s;
  r.f = a.f | b.f;
  return r;
}
__device__ __forceinline__ RankState rank_element(uint64_t key, uint64_t prev, bool first) {
  RankState r;
  const uint32_t k32 = (uint32_t)(key >> 1);
  r.n = ((key & 1ull) == 0ull && k32 != KEY_NAN) ? 1u : 0u;
  r.g = 0u; r.s = 0u;
  r.f = ((first || (key >> 1) != (prev >> 1)) ? 1u : 0u) | ((first || (key >> 33) != (prev >> 33)) ? 2u : 0u);
  return r;
}
// inclusive scan of one state per thread in thread order (Hillis-Steele through LDS: 8 steps for 256 threads)
__device__ __forceinline__ RankState rank_block_scan(RankState v, RankState* lds) {
  const int t = threadIdx.x;
  lds[t] = v;
  __syncthreads();
  for (int off = 1; off < RANK_THREADS; off <<= 1) {
    RankState left = v;
    const bool take = t >= off;
    if (take) left = lds[t - off];
    __syncthreads();
    if (take) v = rank_combine(left, v);
    lds[t] = v;
    __syncthreads();
  }
  return v;
}
// a thread's RANK_ITEMS consecutive keys, folded in order (read from memory here and once more by the walk of rank_scan_kernel: the
// second read hits the cache, and no key array is held in registers across the workgroup scans)
__device__ __forceinline__ int rank_count(int64_t M, int64_t first) {
  const int64_t left = M - first;
  return left <= 0 ? 0 : (left < RANK_ITEMS ? (int)left : RANK_ITEMS);
}
__device__ __forceinline__ RankState rank_fold(const uint64_t* __restrict__ keys, int64_t first, int cnt) {
  RankState v = {0u, 0u, 0u, 0u};
  uint64_t p = (cnt > 0 && first > 0) ? keys[first - 1] : 0ull;
  for (int j = 0; j < cnt; ++j) {
    const uint64_t k = keys[first + j];
    v = rank_combine(v, rank_element(k, p, first + j == 0));
    p = k;
  }
  return v;
}

__global__ __launch_bounds__(RANK_THREADS) void rank_reduce_kernel(const uint64_t* __restrict__ keys, int64_t M, RankState* __restrict__ partial) {
  __shared__ RankState lds[RANK_THREADS];
  const int64_t first = (int64_t)blockIdx.x * RANK_TILE + (int64_t)threadIdx.x * RANK_ITEMS;
  const RankState v = rank_block_scan(rank_fold(keys, first, rank_count(M, first)), lds);
  if (threadIdx.x == RANK_THREADS - 1) partial[blockIdx.x] = v;
}

struct RankAcc { uint64_t two_u; uint32_t n_pos, n_neg, n_nan; };
__device__ __forceinline__ void rank_flush(uint64_t* acc_two_u, uint32_t* acc_cnt, uint32_t seg, const RankAcc& a) {
  if (a.two_u) atomicAdd(reinterpret_cast<unsigned long long*>(acc_two_u + seg), (unsigned long long)a.two_u);
  if (a.n_pos) atomicAdd(acc_cnt + 3 * (size_t)seg + 0, a.n_pos);
  if (a.n_neg) atomicAdd(acc_cnt + 3 * (size_t)seg + 1, a.n_neg);
  if (a.n_nan) atomicAdd(acc_cnt + 3 * (size_t)seg + 2, a.n_nan);
}

__global__ __launch_bounds__(RANK_THREADS) void rank_scan_kernel(const uint64_t* __restrict__ keys, int64_t M, const RankState* __restrict__ partial,
                                                                 uint64_t* __restrict__ acc_two_u, uint32_t* __restrict__ acc_cnt) {
  __shared__ RankState lds[RANK_THREADS];
  __shared__ RankState block_prefix;
  const int t = threadIdx.x;
  // the state in front of this workgroup's tile: the partials of the tiles before it, folded in order
  {
    const int nb = blockIdx.x;
    const int c = (nb + RANK_THREADS - 1) / RANK_THREADS;
    RankState v = {0u, 0u, 0u, 0u};
    for (int j = t * c; j < (t + 1) * c && j < nb; ++j) v = rank_combine(v, partial[j]);
    v = rank_block_scan(v, lds);
    if (t == RANK_THREADS - 1) block_prefix = v;
    __syncthreads();
  }
  const int64_t first = (int64_t)blockIdx.x * RANK_TILE + (int64_t)t * RANK_ITEMS;
  const int cnt = rank_count(M, first);
  (void)rank_block_scan(rank_fold(keys, first, cnt), lds);
  RankState run = block_prefix;
  if (t > 0) run = rank_combine(run, lds[t - 1]);   // (lds holds the inclusive scan)
  // walk the items: totals per run of one segment
  RankAcc a = {0ull, 0u, 0u, 0u};
  uint32_t seg = cnt > 0 ? (uint32_t)(keys[first] >> 33) : 0u;
  bool flushed = false;
  uint64_t p = (cnt > 0 && first > 0) ? keys[first - 1] : 0ull;
  for (int j = 0; j < cnt; ++j) {
    const uint64_t k = keys[first + j];
    const uint32_t sj = (uint32_t)(k >> 33);
    if (sj != seg) { rank_flush(acc_two_u, acc_cnt, seg, a); a = {0ull, 0u, 0u, 0u}; seg = sj; flushed = true; }
    run = rank_combine(run, rank_element(k, p, first + j == 0));
    p = k;
    const uint32_t k32 = (uint32_t)(k >> 1);
    if (k32 == KEY_NAN) a.n_nan += 1u;
    else if (k & 1ull) { a.n_pos += 1u; a.two_u += (uint64_t)(run.n - run.s) + (uint64_t)(run.g - run.s); }
    else a.n_neg += 1u;
  }
  // a wavefront whose lanes all stayed inside one and the same segment adds its sums up first and sends one set of atomics
  const bool have = cnt > 0;
  const unsigned long long with = __ballot(have);
  if (with == 0ull) return;
  const uint32_t seg0 = __shfl(seg, __ffsll((long long)with) - 1);
  if (__all(!have || (!flushed && seg == seg0))) {
    for (int off = 1; off < 64; off <<= 1) {
      a.two_u += __shfl_xor(a.two_u, off);
      a.n_pos += __shfl_xor(a.n_pos, off);
      a.n_neg += __shfl_xor(a.n_neg, off);
      a.n_nan += __shfl_xor(a.n_nan, off);
    }
    if ((t & 63) == 0) rank_flush(acc_two_u, acc_cnt, seg0, a);
  } else if (have) {
    rank_flush(acc_two_u, acc_cnt, seg, a);
  }
}

// ---- SSE: the fixed-shape sum of re_eval_sum.hpp ---------------------------------------------------------------------------------------
// lane t of `stride` lanes adds the terms i = begin + t, begin + t + stride, ...: EVAL_RUN in a row, EVAL_RUNS such runs in a row, and those
// sums in a row (at most 64 of them below 2^31 samples on 256 lanes)
__device__ __forceinline__ double sse_lane(const float* __restrict__ score, const float* __restrict__ label, int64_t begin, int64_t end, int64_t stride) {
  double top = 0.0, total = 0.0, run = 0.0;
  int in_run = 0, runs = 0;
  for (int64_t i = begin; i < end; i += stride) {
    const float s = score[i];
    if (s == s) run += sq_err(s, label[i]);
    if (++in_run == EVAL_RUN) {
      total += run; run = 0.0; in_run = 0;
      if (++runs == EVAL_RUNS) { top += total; total = 0.0; runs = 0; }
    }
  }
  return top + (total + run);
}

// one workgroup per large entity: its SSE, then its outputs from the rank-sum totals
__global__ __launch_bounds__(EVAL_THREADS) void eval_big_finish_kernel(const int64_t* __restrict__ ent_row_ptr, const int32_t* __restrict__ big_list,
                                                                       const float* __restrict__ score, const float* __restrict__ label,
                                                                       const uint64_t* __restrict__ acc_two_u, const uint32_t* __restrict__ acc_cnt, EvalOutDev O) {
  __shared__ double lds[EVAL_THREADS];
  const int b = blockIdx.x;
  const int64_t e = big_list[b];
  const int64_t r0 = ent_row_ptr[e], r1 = ent_row_ptr[e + 1];
  double sse = 0.0;
  if (O.sse) sse = eval_block_tree(sse_lane(score, label, r0 + threadIdx.x, r1, EVAL_THREADS), lds);
  if (threadIdx.x == 0)
    write_entity(O, e, acc_two_u[b], (int)acc_cnt[3 * (size_t)b], (int)acc_cnt[3 * (size_t)b + 1], (int)acc_cnt[3 * (size_t)b + 2], sse);
}

// accumulator: a batch's keys appended (segment 0) and its SSE, in the one read of the samples (the accumulator's
// lane sum of re_eval_sum.hpp: one level of runs)
__global__ __launch_bounds__(EVAL_THREADS) void eval_acc_add_kernel(const float* __restrict__ score, const float* __restrict__ label, int64_t N,
                                                                    uint64_t* __restrict__ keys, double* __restrict__ group_sum) {
  __shared__ double lds[EVAL_THREADS];
  const int64_t stride = (int64_t)gridDim.x * EVAL_THREADS;
  double total = 0.0, run = 0.0;
  int in_run = 0;
  for (int64_t i = (int64_t)blockIdx.x * EVAL_THREADS + threadIdx.x; i < N; i += stride) {
    const float s = score[i], y = label[i];
    keys[i] = key33(s, y);
    if (s == s) run += sq_err(s, y);
    if (++in_run == EVAL_RUN) { total += run; run = 0.0; in_run = 0; }
  }
  const double v = eval_block_tree(total + run, lds);
  if (threadIdx.x == 0) group_sum[blockIdx.x] = v;
}
// the workgroup sums of a batch -> added to the accumulator's SSE (one workgroup; batches add up in the order they were given)
__global__ __launch_bounds__(EVAL_THREADS) void eval_acc_sum_kernel(const double* __restrict__ group_sum, int groups, double* __restrict__ sse) {
  __shared__ double lds[EVAL_THREADS];
  const double v = acc_group_tree(group_sum, groups, lds);
  if (threadIdx.x == 0) *sse += v;
}

// ---- ranking: the four integers of precision@k per entity (include/gdmix_re.h, "ranking evaluation") --------------------------------------
constexpr int TOPK_MAX = 4, TOPK_THREADS = 256;
struct TopkKs { int32_t k[TOPK_MAX]; int nk; };
struct TopkOutDev { int32_t* hits_sure; int32_t* slots; int32_t* tie_pos; int32_t* tie_size; };   // [nk][E] each, k-major
__device__ __forceinline__ void write_topk(const TopkOutDev& T, int64_t E, int kk, int64_t e, int hits_sure, int slots, int tie_pos, int tie_size) {
  const size_t at = (size_t)kk * (size_t)E + (size_t)e;
  if (T.hits_sure) T.hits_sure[at] = hits_sure;
  if (T.slots) T.slots[at] = slots;
  if (T.tie_pos) T.tie_pos[at] = tie_pos;
  if (T.tie_size) T.tie_size[at] = tie_size;
}

// Small entities: eval_small_kernel's geometry (four entities per wavefront, 16 / 32 / 64 lanes each, lane i holds sample i), with the keys
// of ALL valid samples through LDS (every other lane stores KEY_NAN, which is above every score's key): lane i counts lt = #{k_j < k_i} and
// le = #{k_j <= k_i}; with n valid samples gt = n - le and ge = n - lt. Sample i is above the cut <=> ge <= k - 1, in the tie group of the
// cut <=> gt < k <= ge. The four integers of a k are sums of flags over the group, four 8-bit fields of one word (each at most 64).
// The loop over k runs on the counts in registers. WITH_AUC: the wavefront also does what eval_small_kernel does, with that
// kernel's operations in that kernel's order (the same integers, the same bits of sse), from the one read of the samples.
template <bool WITH_AUC>
__global__ __launch_bounds__(64) void topk_small_kernel(const int64_t* __restrict__ ent_row_ptr, int64_t E, const float* __restrict__ score,
                                                        const float* __restrict__ label, TopkOutDev T, TopkKs K, EvalOutDev O, int small_max) {
  __shared__ __attribute__((aligned(16))) uint32_t all_keys[64];
  __shared__ __attribute__((aligned(16))) uint32_t neg_keys[64];
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
  const int W = nmax <= 16 ? 16 : (nmax <= 32 ? 32 : 64);
  const int per_pass = 64 / W;
  const int g = lane / W, li = lane & (W - 1), base = lane & ~(W - 1);
  for (int pass = 0; pass < W / 16; ++pass) {
    const int k = pass * per_pass + g;
    const int64_t start = k == 0 ? rp[0] : (k == 1 ? rp[1] : (k == 2 ? rp[2] : rp[3]));
    const int64_t end = k == 0 ? rp[1] : (k == 1 ? rp[2] : (k == 2 ? rp[3] : rp[4]));
    const int64_t n = end - start;
    const bool ent_ok = e0 + k < E && n <= small_max;
    const bool have = ent_ok && li < n;
    float s = 0.0f, y = 0.0f;
    if (have) { s = score[start + li]; y = label[start + li]; }
    const uint32_t key = have ? sortable_key(s) : KEY_NAN;
    const bool nan = have && key == KEY_NAN;
    const bool pos = have && !nan && y > 0.5f;
    const bool neg = have && !nan && !pos;
    all_keys[lane] = key;                       // KEY_NAN for a NaN score and for a lane without a sample
    if (WITH_AUC) neg_keys[lane] = neg ? key : KEY_NAN;
    __syncthreads();
    uint32_t lt = 0, le = 0, cnt = 0;
    for (int j = 0; j < W; j += 4) {
      const uint4 v = *reinterpret_cast<const uint4*>(&all_keys[base + j]);
      lt += (uint32_t)(v.x < key) + (uint32_t)(v.y < key) + (uint32_t)(v.z < key) + (uint32_t)(v.w < key);
      le += (uint32_t)(v.x <= key) + (uint32_t)(v.y <= key) + (uint32_t)(v.z <= key) + (uint32_t)(v.w <= key);
      if (WITH_AUC) {
        const uint4 u = *reinterpret_cast<const uint4*>(&neg_keys[base + j]);
        cnt += (uint32_t)(u.x < key) + (uint32_t)(u.x <= key) + (uint32_t)(u.y < key) + (uint32_t)(u.y <= key) +
               (uint32_t)(u.z < key) + (uint32_t)(u.z <= key) + (uint32_t)(u.w < key) + (uint32_t)(u.w <= key);
      }
    }
    __syncthreads();   // the next pass overwrites the keys
    uint32_t a = (pos ? cnt : 0u) | ((pos ? 1u : 0u) << 16);
    uint32_t b = (neg ? 1u : 0u) | ((nan ? 1u : 0u) << 16);
    double sse = (WITH_AUC && have && !nan) ? sq_err(s, y) : 0.0;
    for (int off = 1; off < W; off <<= 1) {
      a += __shfl_xor(a, off);
      b += __shfl_xor(b, off);
      if (WITH_AUC) sse += __shfl_xor(sse, off);
    }
    const int n_pos = (int)(a >> 16), n_neg = (int)(b & 0xFFFFu);
    if (WITH_AUC && ent_ok && li == 0) write_entity(O, e0 + k, a & 0xFFFFu, n_pos, n_neg, (int)(b >> 16), sse);
    const int nv = n_pos + n_neg;               // valid samples; a valid lane's le counts valid keys only (KEY_NAN is above its key)
    const int gt = nv - (int)le, ge = nv - (int)lt;
    const bool valid = have && !nan;
    for (int kk = 0; kk < K.nk; ++kk) {
      const int64_t kv = K.k[kk];
      const bool above = valid && (int64_t)ge <= kv - 1;
      const bool tie = valid && (int64_t)gt < kv && kv <= (int64_t)ge;
      // fields: hits (pos & above) | above << 8 | tie_pos << 16 | tie_size << 24
      uint32_t w = ((pos && above) ? 1u : 0u) | ((above ? 1u : 0u) << 8) | (((pos && tie) ? 1u : 0u) << 16) | ((tie ? 1u : 0u) << 24);
      for (int off = 1; off < W; off <<= 1) w += __shfl_xor(w, off);
      if (ent_ok && li == 0) {
        if ((int64_t)nv <= kv) write_topk(T, E, kk, e0 + k, n_pos, 0, 0, 0);
        else write_topk(T, E, kk, e0 + k, (int)(w & 0xFFu), (int)(kv - (int64_t)((w >> 8) & 0xFFu)), (int)((w >> 16) & 0xFFu), (int)(w >> 24));
      }
    }
  }
}

// Large entities: one workgroup on the entity's sorted segment (ascending 33-bit keys under the segment number; a tie's negatives in front
// of its positives; NaN keys last). With n valid keys and n > k the cut key c is at position n - k; three binary searches in the segment
// (c << 1, c << 1 | 1, (c + 1) << 1) give the tie group and its positives; the positives above the cut are counted by the workgroup over
// the keys behind the tie group — fewer than k of them (n <= k: over all n valid keys).
__device__ __forceinline__ int64_t seg_lower_bound(const uint64_t* __restrict__ seg, int64_t n, uint64_t want33) {   // first i < n with key33 >= want33, or n
  int64_t lo = 0, hi = n;
  while (lo < hi) {
    const int64_t mid = lo + ((hi - lo) >> 1);
    if ((seg[mid] & 0x1FFFFFFFFull) < want33) lo = mid + 1; else hi = mid;
  }
  return lo;
}
__global__ __launch_bounds__(TOPK_THREADS) void topk_big_kernel(const int64_t* __restrict__ ent_row_ptr, const int32_t* __restrict__ big_list,
                                                                const int32_t* __restrict__ big_off, const uint64_t* __restrict__ sorted, int64_t E,
                                                                TopkOutDev T, TopkKs K) {
  __shared__ int64_t sh_from, sh_nv;
  __shared__ int sh_out[3];
  __shared__ unsigned sh_hits;
  const int b = blockIdx.x;
  const int64_t e = big_list[b];
  const int64_t n_all = ent_row_ptr[e + 1] - ent_row_ptr[e];
  const uint64_t* seg = sorted + big_off[b];
  for (int kk = 0; kk < K.nk; ++kk) {
    const int64_t kv = K.k[kk];
    if (threadIdx.x == 0) {
      const int64_t nv = seg_lower_bound(seg, n_all, (uint64_t)KEY_NAN << 1);
      int64_t from = 0;
      int slots = 0, tie_pos = 0, tie_size = 0;
      if (nv > kv) {
        const uint64_t c = (seg[nv - kv] & 0x1FFFFFFFFull) >> 1;
        const int64_t lo = seg_lower_bound(seg, nv, c << 1), mid = seg_lower_bound(seg, nv, (c << 1) | 1ull), hi = seg_lower_bound(seg, nv, (c + 1ull) << 1);
        slots = (int)(kv - (nv - hi));
        tie_pos = (int)(hi - mid);
        tie_size = (int)(hi - lo);
        from = hi;
      }
      sh_from = from; sh_nv = nv;
      sh_out[0] = slots; sh_out[1] = tie_pos; sh_out[2] = tie_size;
      sh_hits = 0u;
    }
    __syncthreads();
    const int64_t from = sh_from, nv = sh_nv;
    unsigned hits = 0u;
    for (int64_t i = from + threadIdx.x; i < nv; i += TOPK_THREADS) hits += (unsigned)(seg[i] & 1ull);
    if (hits) atomicAdd(&sh_hits, hits);
    __syncthreads();
    if (threadIdx.x == 0) write_topk(T, E, kk, e, (int)sh_hits, sh_out[0], sh_out[1], sh_out[2]);
    __syncthreads();   // the next k resets the shared words
  }
}

static size_t up256(size_t x) { return (x + 255) & ~(size_t)255; }
static int64_t rank_tiles(int64_t M) { return (M + RANK_TILE - 1) / RANK_TILE; }

// device temporary of the context (grow-only): rocPRIM's temporary storage, whose size only the library can tell
int eval_tmp(gdmix_ctx_impl* ci, size_t bytes, hipStream_t s, void** out) {
  if (ci->eval_tmp_bytes < bytes) {
    HIP_TRY(hipStreamSynchronize(s));
    if (ci->eval_tmp) { HIP_TRY(hipFree(ci->eval_tmp)); ci->eval_tmp = nullptr; ci->eval_tmp_bytes = 0; }
    const size_t want = bytes + bytes / 4 + 4096;
    const hipError_t rc = hipMalloc(&ci->eval_tmp, want);
    if (rc != hipSuccess) { set_error("evaluate: a %zu-byte device temporary for the sort: %s", want, hipGetErrorString(rc)); return GDMIX_RE_ENOMEM; }
    ci->eval_tmp_bytes = want;
  }
  *out = ci->eval_tmp;
  return GDMIX_RE_OK;
}

// sorted keys -> per-segment totals in acc_two_u / acc_cnt (zeroed here)
static int rank_sum(const uint64_t* sorted, int64_t M, int64_t segments, RankState* partial, uint64_t* acc_two_u, uint32_t* acc_cnt, hipStream_t s) {
  HIP_TRY(hipMemsetAsync(acc_two_u, 0, (size_t)segments * 8, s));
  HIP_TRY(hipMemsetAsync(acc_cnt, 0, (size_t)segments * 12, s));
  if (M <= 0) return GDMIX_RE_OK;
  const int nb = (int)rank_tiles(M);
  hipLaunchKernelGGL(rank_reduce_kernel, dim3(nb), dim3(RANK_THREADS), 0, s, sorted, M, partial);
  hipLaunchKernelGGL(rank_scan_kernel, dim3(nb), dim3(RANK_THREADS), 0, s, sorted, M, (const RankState*)partial, acc_two_u, acc_cnt);
  HIP_TRY(hipGetLastError());
  return GDMIX_RE_OK;
}

static int sort_keys(gdmix_ctx_impl* ci, uint64_t* in, uint64_t* out, int64_t M, unsigned end_bit, hipStream_t s) {
  size_t bytes = 0;
  HIP_TRY((rocprim::radix_sort_keys(nullptr, bytes, (unsigned long long*)nullptr, (unsigned long long*)nullptr, (size_t)M, 0u, end_bit, s)));
  void* tmp = nullptr;
  const int rc = eval_tmp(ci, bytes ? bytes : 1, s, &tmp);
  if (rc != GDMIX_RE_OK) return rc;
  HIP_TRY((rocprim::radix_sort_keys(tmp, bytes, reinterpret_cast<unsigned long long*>(in), reinterpret_cast<unsigned long long*>(out), (size_t)M, 0u,
                                    end_bit, s)));
  return GDMIX_RE_OK;
}

struct EvalLayout { size_t mark, offs, big_list, big_off, keys_a, keys_b, partial, acc_two_u, acc_cnt, total; };
static EvalLayout eval_layout(int64_t E, int64_t N) {
  EvalLayout L;
  size_t off = 0;
  auto take = [&](size_t bytes) { const size_t o = off; off = up256(off + bytes); return o; };
  L.mark = take((size_t)(E + 1) * 8);
  L.offs = take((size_t)(E + 1) * 8);
  L.big_list = take((size_t)(E + 1) * 4);
  L.big_off = take((size_t)(E + 1) * 4);
  L.keys_a = take((size_t)N * 8);
  L.keys_b = take((size_t)N * 8);
  L.partial = take((size_t)(rank_tiles(N) + 1) * sizeof(RankState));
  L.acc_two_u = take((size_t)(E + 1) * 8);
  L.acc_cnt = take((size_t)(E + 1) * 12);
  L.total = off;
  return L;
}
struct AccLayout { size_t sorted, partial, acc_two_u, acc_cnt, total; };
static AccLayout acc_layout(int64_t N) {
  AccLayout L;
  size_t off = 0;
  auto take = [&](size_t bytes) { const size_t o = off; off = up256(off + bytes); return o; };
  L.sorted = take((size_t)N * 8);
  L.partial = take((size_t)(rank_tiles(N) + 1) * sizeof(RankState));
  L.acc_two_u = take(8);
  L.acc_cnt = take(12);
  L.total = off;
  return L;
}

// ---- the sort path's steps, shared by gdmix_re_eval_entities and gdmix_re_eval_topk_entities --------------------------------------------
// mark -> one prefix sum -> (the one synchronisation: how many entities are large) -> list -> keys -> radix sort. `sorted` holds the
// segments of the large entities in their order, segment b at big_off[b], a NaN score's key last in its segment.
struct SortedBig { int64_t nbig, M; int32_t* big_list; int32_t* big_off; uint64_t* sorted; RankState* partial; uint64_t* acc_two_u; uint32_t* acc_cnt; };
static int sort_big_entities(gdmix_ctx_impl* ci, const char* who, const int64_t* ent_row_ptr, int64_t E, int64_t N, const float* score, const float* label,
                             int small_max, const EvalLayout& L, char* base, hipStream_t s, SortedBig* B) {
  int64_t* mark = reinterpret_cast<int64_t*>(base + L.mark);
  int64_t* offs = reinterpret_cast<int64_t*>(base + L.offs);
  int32_t* big_list = reinterpret_cast<int32_t*>(base + L.big_list);
  int32_t* big_off = reinterpret_cast<int32_t*>(base + L.big_off);
  uint64_t* keys_a = reinterpret_cast<uint64_t*>(base + L.keys_a);
  uint64_t* keys_b = reinterpret_cast<uint64_t*>(base + L.keys_b);
  B->nbig = 0; B->M = 0;
  B->big_list = big_list; B->big_off = big_off; B->sorted = keys_b;
  B->partial = reinterpret_cast<RankState*>(base + L.partial);
  B->acc_two_u = reinterpret_cast<uint64_t*>(base + L.acc_two_u);
  B->acc_cnt = reinterpret_cast<uint32_t*>(base + L.acc_cnt);
  // the entities of the sort path: numbered and laid out by one prefix sum
  hipLaunchKernelGGL(eval_mark_kernel, dim3((unsigned)((E + 1 + 255) / 256)), dim3(256), 0, s, ent_row_ptr, E, small_max, mark);
  HIP_TRY(hipGetLastError());
  size_t scan_bytes = 0;
  HIP_TRY((rocprim::exclusive_scan(nullptr, scan_bytes, (int64_t*)nullptr, (int64_t*)nullptr, (int64_t)0, (size_t)E + 1, rocprim::plus<int64_t>(), s)));
  void* tmp = nullptr;
  int rc = eval_tmp(ci, scan_bytes ? scan_bytes : 1, s, &tmp);
  if (rc != GDMIX_RE_OK) return rc;
  HIP_TRY((rocprim::exclusive_scan(tmp, scan_bytes, mark, offs, (int64_t)0, (size_t)E + 1, rocprim::plus<int64_t>(), s)));
  int64_t total = 0;
  HIP_TRY(fetch_small(ci, 2, offs + E, sizeof(int64_t), &total, s));
  const int64_t nbig = total >> 32, M = total & 0xFFFFFFFFll;
  if (nbig == 0) return GDMIX_RE_OK;
  if (M > N) { set_error("%s: ent_row_ptr covers %lld samples, N is %lld", who, (long long)M, (long long)N); return GDMIX_RE_EINVAL; }
  hipLaunchKernelGGL(eval_big_list_kernel, dim3((unsigned)((E + 255) / 256)), dim3(256), 0, s, (const int64_t*)mark, (const int64_t*)offs, E, big_list, big_off);
  if (M > 0) hipLaunchKernelGGL(eval_big_keys_kernel, dim3((unsigned)((M + 255) / 256)), dim3(256), 0, s, ent_row_ptr, (const int32_t*)big_list,
                                (const int32_t*)big_off, (int)nbig, M, score, label, keys_a);
  HIP_TRY(hipGetLastError());
  unsigned sbits = 0;
  while (((int64_t)1 << sbits) < nbig) ++sbits;
  if (M > 0) {
    rc = sort_keys(ci, keys_a, keys_b, M, 33u + sbits, s);
    if (rc != GDMIX_RE_OK) return rc;
  }
  B->nbig = nbig; B->M = M;
  return GDMIX_RE_OK;
}
// the rank-sum pass over the sorted segments, then a workgroup per large entity: its SSE and its outputs
static int rank_and_finish(const SortedBig& B, const int64_t* ent_row_ptr, const float* score, const float* label, const EvalOutDev& O, hipStream_t s) {
  const int rc = rank_sum(B.sorted, B.M, B.nbig, B.partial, B.acc_two_u, B.acc_cnt, s);
  if (rc != GDMIX_RE_OK) return rc;
  hipLaunchKernelGGL(eval_big_finish_kernel, dim3((unsigned)B.nbig), dim3(EVAL_THREADS), 0, s, ent_row_ptr, (const int32_t*)B.big_list, score, label,
                     (const uint64_t*)B.acc_two_u, (const uint32_t*)B.acc_cnt, O);
  HIP_TRY(hipGetLastError());
  return GDMIX_RE_OK;
}

}  // namespace gdmix

using namespace gdmix;

extern "C" {

GDMIX_API int gdmix_re_set_eval_small_max(gdmix_re_ctx* ctx, int small_max) {
  if (!ctx || small_max < 0 || small_max > 64) { set_error("gdmix_re_set_eval_small_max: 0 .. 64"); return GDMIX_RE_EINVAL; }
  ctx->impl.eval_small_max = small_max;
  ctx->impl.eval_small_set = 1;
  return GDMIX_RE_OK;
}

GDMIX_API size_t gdmix_re_eval_workspace_bytes(int64_t E, int64_t N) {
  if (E < 0 || N < 0 || E >= EVAL_LIMIT || N >= EVAL_LIMIT) return 0;
  return eval_layout(E, N).total;
}

GDMIX_API int gdmix_re_eval_entities(gdmix_re_ctx* ctx, const int64_t* ent_row_ptr, int64_t E, int64_t N, const float* score, const float* label,
                                     const gdmix_re_eval_out* out, void* workspace, size_t workspace_bytes, void* stream) {
  if (!ctx || !out || E < 0 || N < 0) { set_error("gdmix_re_eval_entities: bad argument"); return GDMIX_RE_EINVAL; }
  if (N >= EVAL_LIMIT || E >= EVAL_LIMIT) {
    set_error("gdmix_re_eval_entities: %lld samples / %lld entities; an evaluation takes fewer than 2^31 of each", (long long)N, (long long)E);
    return GDMIX_RE_ERANGE;
  }
  if (E == 0) return GDMIX_RE_OK;
  if (!ent_row_ptr || (N > 0 && (!score || !label))) { set_error("gdmix_re_eval_entities: NULL input"); return GDMIX_RE_EINVAL; }
  const EvalLayout L = eval_layout(E, N);
  if (!workspace || workspace_bytes < L.total) {
    set_error("gdmix_re_eval_entities: workspace of %zu bytes, %zu needed (gdmix_re_eval_workspace_bytes)", workspace_bytes, L.total);
    return GDMIX_RE_ENOMEM;
  }
  gdmix_ctx_impl* ci = &ctx->impl;
  hipStream_t s = static_cast<hipStream_t>(stream);
  const int small_max = ci->eval_small_set ? ci->eval_small_max : 64;
  const EvalOutDev O = {out->two_u, out->n_pos, out->n_neg, out->n_nan, out->sse, out->auc};
  // (with a limit of 0 — every entity through the sort path — this launch still writes the entities of no samples)
  hipLaunchKernelGGL(eval_small_kernel, dim3((unsigned)((E + 3) / 4)), dim3(64), 0, s, ent_row_ptr, E, score, label, O, small_max);
  HIP_TRY(hipGetLastError());
  SortedBig B;
  int rc = sort_big_entities(ci, "gdmix_re_eval_entities", ent_row_ptr, E, N, score, label, small_max, L, static_cast<char*>(workspace), s, &B);
  if (rc != GDMIX_RE_OK || B.nbig == 0) return rc;
  return rank_and_finish(B, ent_row_ptr, score, label, O, s);
}

GDMIX_API size_t gdmix_re_eval_topk_workspace_bytes(int64_t E, int64_t N) { return gdmix_re_eval_workspace_bytes(E, N); }

GDMIX_API int gdmix_re_eval_topk_entities(gdmix_re_ctx* ctx, const int64_t* ent_row_ptr, int64_t E, int64_t N, const float* score, const float* label,
                                          const int32_t* ks, int nk, const gdmix_re_eval_topk_out* out, const gdmix_re_eval_out* auc_out,
                                          void* workspace, size_t workspace_bytes, void* stream) {
  if (!ctx || !out || E < 0 || N < 0) { set_error("gdmix_re_eval_topk_entities: bad argument"); return GDMIX_RE_EINVAL; }
  if (!ks || nk < 1 || nk > TOPK_MAX) { set_error("gdmix_re_eval_topk_entities: nk = %d; 1 .. %d values of k in ks", nk, TOPK_MAX); return GDMIX_RE_EINVAL; }
  TopkKs K;
  K.nk = nk;
  for (int i = 0; i < TOPK_MAX; ++i) K.k[i] = i < nk ? ks[i] : 0;
  for (int i = 0; i < nk; ++i) {
    if (ks[i] < 1) { set_error("gdmix_re_eval_topk_entities: ks[%d] = %d; every k is at least 1", i, (int)ks[i]); return GDMIX_RE_EINVAL; }
    for (int j = 0; j < i; ++j)
      if (ks[j] == ks[i]) { set_error("gdmix_re_eval_topk_entities: ks[%d] = ks[%d] = %d; the values of k are distinct", j, i, (int)ks[i]); return GDMIX_RE_EINVAL; }
  }
  if (N >= EVAL_LIMIT || E >= EVAL_LIMIT) {
    set_error("gdmix_re_eval_topk_entities: %lld samples / %lld entities; an evaluation takes fewer than 2^31 of each", (long long)N, (long long)E);
    return GDMIX_RE_ERANGE;
  }
  if (E == 0) return GDMIX_RE_OK;
  if (!ent_row_ptr || (N > 0 && (!score || !label))) { set_error("gdmix_re_eval_topk_entities: NULL input"); return GDMIX_RE_EINVAL; }
  const EvalLayout L = eval_layout(E, N);
  if (!workspace || workspace_bytes < L.total) {
    set_error("gdmix_re_eval_topk_entities: workspace of %zu bytes, %zu needed (gdmix_re_eval_topk_workspace_bytes)", workspace_bytes, L.total);
    return GDMIX_RE_ENOMEM;
  }
  gdmix_ctx_impl* ci = &ctx->impl;
  hipStream_t s = static_cast<hipStream_t>(stream);
  const int small_max = ci->eval_small_set ? ci->eval_small_max : 64;
  const bool with_auc = auc_out != nullptr;
  EvalOutDev O = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
  if (with_auc) O = {auc_out->two_u, auc_out->n_pos, auc_out->n_neg, auc_out->n_nan, auc_out->sse, auc_out->auc};
  const TopkOutDev T = {out->hits_sure, out->slots, out->tie_pos, out->tie_size};
  if (with_auc) hipLaunchKernelGGL(topk_small_kernel<true>, dim3((unsigned)((E + 3) / 4)), dim3(64), 0, s, ent_row_ptr, E, score, label, T, K, O, small_max);
  else hipLaunchKernelGGL(topk_small_kernel<false>, dim3((unsigned)((E + 3) / 4)), dim3(64), 0, s, ent_row_ptr, E, score, label, T, K, O, small_max);
  HIP_TRY(hipGetLastError());
  SortedBig B;
  int rc = sort_big_entities(ci, "gdmix_re_eval_topk_entities", ent_row_ptr, E, N, score, label, small_max, L, static_cast<char*>(workspace), s, &B);
  if (rc != GDMIX_RE_OK || B.nbig == 0) return rc;
  hipLaunchKernelGGL(topk_big_kernel, dim3((unsigned)B.nbig), dim3(TOPK_THREADS), 0, s, ent_row_ptr, (const int32_t*)B.big_list, (const int32_t*)B.big_off,
                     (const uint64_t*)B.sorted, E, T, K);
  HIP_TRY(hipGetLastError());
  return with_auc ? rank_and_finish(B, ent_row_ptr, score, label, O, s) : GDMIX_RE_OK;
}

GDMIX_API int gdmix_re_eval_acc_reset(gdmix_re_ctx* ctx, gdmix_re_eval_acc* acc, void* stream) {
  if (!ctx || !acc || acc->capacity < 0 || !acc->state) { set_error("gdmix_re_eval_acc_reset: bad argument (acc->state is required)"); return GDMIX_RE_EINVAL; }
  static_assert(GDMIX_RE_EVAL_ACC_STATE_BYTES >= ACC_STATE_BYTES, "the accumulator's device state");
  HIP_TRY(hipMemsetAsync(acc->state, 0, ACC_HEAD_BYTES, static_cast<hipStream_t>(stream)));
  acc->count = 0;
  return GDMIX_RE_OK;
}

GDMIX_API int gdmix_re_eval_acc_add(gdmix_re_ctx* ctx, gdmix_re_eval_acc* acc, const float* score, const float* label, int64_t N, void* stream) {
  if (!ctx || !acc || !acc->state || N < 0 || acc->capacity < 0 || acc->count < 0) { set_error("gdmix_re_eval_acc_add: bad argument"); return GDMIX_RE_EINVAL; }
  if (N == 0) return GDMIX_RE_OK;
  if (acc->count + N >= EVAL_LIMIT) {
    set_error("gdmix_re_eval_acc_add: %lld + %lld samples; an evaluation takes fewer than 2^31", (long long)acc->count, (long long)N);
    return GDMIX_RE_ERANGE;
  }
  if (!acc->keys || acc->count + N > acc->capacity) {
    set_error("gdmix_re_eval_acc_add: key buffer of %lld samples, %lld + %lld to hold", (long long)acc->capacity, (long long)acc->count, (long long)N);
    return GDMIX_RE_ENOMEM;
  }
  if (!score || !label) { set_error("gdmix_re_eval_acc_add: NULL input"); return GDMIX_RE_EINVAL; }
  hipStream_t s = static_cast<hipStream_t>(stream);
  const int64_t groups = acc_groups(N);
  double* sse = static_cast<double*>(acc->state);
  double* group_sum = acc_group_sums(acc->state);
  hipLaunchKernelGGL(eval_acc_add_kernel, dim3((unsigned)groups), dim3(EVAL_THREADS), 0, s, score, label, N, acc->keys + acc->count, group_sum);
  hipLaunchKernelGGL(eval_acc_sum_kernel, dim3(1), dim3(EVAL_THREADS), 0, s, (const double*)group_sum, (int)groups, sse);
  HIP_TRY(hipGetLastError());
  acc->count += N;
  return GDMIX_RE_OK;
}

GDMIX_API size_t gdmix_re_eval_acc_workspace_bytes(int64_t N) {
  if (N < 0 || N >= EVAL_LIMIT) return 0;
  return acc_layout(N).total;
}

GDMIX_API int gdmix_re_eval_acc_finish(gdmix_re_ctx* ctx, const gdmix_re_eval_acc* acc, void* workspace, size_t workspace_bytes,
                                       gdmix_re_eval_totals* host_out, void* stream) {
  if (!ctx || !acc || !acc->state || !host_out || acc->count < 0 || acc->count >= EVAL_LIMIT) { set_error("gdmix_re_eval_acc_finish: bad argument"); return GDMIX_RE_EINVAL; }
  gdmix_ctx_impl* ci = &ctx->impl;
  const int64_t M = acc->count;
  const AccLayout L = acc_layout(M);
  if (!workspace || workspace_bytes < L.total || (M > 0 && (!acc->keys || acc->capacity < M))) {
    set_error("gdmix_re_eval_acc_finish: workspace of %zu bytes, %zu needed for %lld samples (gdmix_re_eval_acc_workspace_bytes)", workspace_bytes,
              L.total, (long long)M);
    return GDMIX_RE_ENOMEM;
  }
  hipStream_t s = static_cast<hipStream_t>(stream);
  char* base = static_cast<char*>(workspace);
  uint64_t* sorted = reinterpret_cast<uint64_t*>(base + L.sorted);
  uint64_t* acc_two_u = reinterpret_cast<uint64_t*>(base + L.acc_two_u);
  uint32_t* acc_cnt = reinterpret_cast<uint32_t*>(base + L.acc_cnt);
  int rc = GDMIX_RE_OK;
  if (M > 0) {
    rc = sort_keys(ci, acc->keys, sorted, M, 33u, s);
    if (rc != GDMIX_RE_OK) return rc;
  }
  rc = rank_sum(sorted, M, 1, reinterpret_cast<RankState*>(base + L.partial), acc_two_u, acc_cnt, s);
  if (rc != GDMIX_RE_OK) return rc;
  uint64_t two_u = 0;
  uint32_t cnt[3] = {0, 0, 0};
  double sse = 0.0;
  HIP_TRY(hipMemcpyAsync(&two_u, acc_two_u, 8, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipMemcpyAsync(cnt, acc_cnt, 12, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipMemcpyAsync(&sse, acc->state, 8, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  host_out->two_u = two_u;
  host_out->n_pos = cnt[0];
  host_out->n_neg = cnt[1];
  host_out->n_nan = cnt[2];
  host_out->n = M;
  host_out->sse = sse;
  return GDMIX_RE_OK;
}

}  // extern "C"
