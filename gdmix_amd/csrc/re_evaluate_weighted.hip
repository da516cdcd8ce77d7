// re_evaluate_weighted.hip — the sample-weighted rank sum on the device: twoU_w, W_pos, W_neg and the weighted AUC, per entity and over a
// whole stage. The contract (weights, bad weights, the term, the bound, the accumulator's word) is stated in include/gdmix_re.h,
// "weighted evaluation"; this unit is its only implementation. The weighted log loss lives next to its term in re_evaluate_poisson.hip.
//
//   w_small_kernel     entities of at most 64 samples, no sort: eval_small_kernel's geometry (four consecutive entities per wavefront, 16, 32
//                      or 64 lanes each, lane i holds sample i). The negatives' keys and weights go through LDS as two arrays of 32-bit words
//                      (every other lane stores the key no score has and a weight of 0): a lane reads its group's W pairs with W / 2
//                      ds_read_b128 and adds, in sample order and in fp64, the weight below its key and the weight at it. A positive forms
//                      w (2 below + at); three fp64 xor-butterflies over the group (term, W_pos, W_neg: the same tree on every lane) and one
//                      integer butterfly for the two counts. 12 B read per sample, no atomics.
//   sort path          entities above the small limit: numbered by eval_number_big (re_evaluate.hip), composite key segment << 33 | key33 with
//                      the canonical weight as the VALUE of one rocPRIM radix sort of pairs (stable: equal keys keep their sample order), then
//                      w_reduce_kernel / w_scan_kernel, reduce-then-scan in two launches over a state of five fp64 sums and two counts: no
//                      workgroup waits for another. The scan is SEGMENTED (a head restarts a sum; nothing is ever subtracted), so every
//                      prefix is a sum of non-negative numbers and keeps a relative bound. The last element of a tie group writes the group's
//                      term, every other position 0.0; the last element of a segment writes its totals. w_big_finish_kernel: a workgroup per
//                      entity adds its segment of terms in the fixed tree of re_eval_sum.hpp.
//   accumulator        gdmix_re_eval_acc's 8-byte keys hold key33 << 31 | the weight's 31 bits below the sign (a bad weight: all ones).
//                      finish sorts the words over all 64 bits, runs the same scan with one segment (the word is key and value at once:
//                      WordSrc) and adds the terms over POSITIONS of the sorted array (eval_sum_positions): the bits depend on the multiset
//                      of (score, label, weight) alone.
#include <stdint.h>
#include <math.h>

#include <rocprim/device/device_radix_sort.hpp>

#include "re_internal.hpp"
#include "re_eval_sum.hpp"

namespace gdmix {

constexpr int W_SCAN_THREADS = 256, W_SCAN_ITEMS = 16, W_SCAN_TILE = W_SCAN_THREADS * W_SCAN_ITEMS;
static_assert(W_SCAN_TILE == GDMIX_RE_EVAL_W_SCAN_TILE, "the scan's tile, as the header names it");
constexpr uint64_t KEY33_BAD = 0x1FFFFFFFFull;   // the 33-bit key of a sample with a bad weight: above a NaN score's (whose label bit is 0)
constexpr uint32_t W_BAD_BITS = 0x7FFFFFFFu;     // the canonical bits of a bad weight (a NaN with a clear sign)

// the weight of sample i: ones without a weight array. A good weight is finite and not negative; -0 is 0.
__device__ __forceinline__ float weight_at(const float* __restrict__ weight, int64_t i) { return weight ? weight[i] : 1.0f; }
__device__ __forceinline__ bool weight_bad(float w) { return !(w >= 0.0f) || w == INFINITY; }
__device__ __forceinline__ uint32_t weight_bits(float w) { return weight_bad(w) ? W_BAD_BITS : (__float_as_uint(w) & 0x7FFFFFFFu); }

// P (2 Nbefore + N): the doubling is exact, then one rounding of the sum and one of the product, on every path
__device__ __forceinline__ double w_term(double P, double Nbefore, double N) {
#pragma clang fp contract(off)
  const double x = 2.0 * Nbefore + N;
  return P * x;
}
__device__ __forceinline__ double w_auc_of(double two_u_w, double w_pos, double w_neg) {
  if (!(w_pos > 0.0) || !(w_neg > 0.0)) return __longlong_as_double(0x7ff8000000000000ll);
  return two_u_w / (2.0 * w_pos * w_neg);
}

struct WOutDev { double* two_u_w; double* w_pos; double* w_neg; int32_t* n_nan; int32_t* n_bad; double* auc; };
__device__ __forceinline__ void write_w(const WOutDev& O, int64_t e, double two_u_w, double w_pos, double w_neg, int n_nan, int n_bad) {
  if (O.two_u_w) O.two_u_w[e] = two_u_w;
  if (O.w_pos) O.w_pos[e] = w_pos;
  if (O.w_neg) O.w_neg[e] = w_neg;
  if (O.n_nan) O.n_nan[e] = n_nan;
  if (O.n_bad) O.n_bad[e] = n_bad;
  if (O.auc) O.auc[e] = w_auc_of(two_u_w, w_pos, w_neg);
}

// ---- small entities ---------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void w_small_kernel(const int64_t* __restrict__ ent_row_ptr, int64_t E, const float* __restrict__ score,
                                                     const float* __restrict__ label, const float* __restrict__ weight, WOutDev O, int small_max) {
  __shared__ __attribute__((aligned(16))) uint32_t neg_keys[64];
  __shared__ __attribute__((aligned(16))) float neg_w[64];
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
  const int W = small_width(nmax);
  const int per_pass = 64 / W;
  const int g = lane / W, li = lane & (W - 1), base = lane & ~(W - 1);
  for (int pass = 0; pass < W / 16; ++pass) {
    const int k = pass * per_pass + g;
    const int64_t start = k == 0 ? rp[0] : (k == 1 ? rp[1] : (k == 2 ? rp[2] : rp[3]));
    const int64_t end = k == 0 ? rp[1] : (k == 1 ? rp[2] : (k == 2 ? rp[3] : rp[4]));
    const int64_t n = end - start;
    const bool ent_ok = e0 + k < E && n <= small_max;
    const bool have = ent_ok && li < n;
    float s = 0.0f, y = 0.0f, wf = 0.0f;
    if (have) { s = score[start + li]; y = label[start + li]; wf = weight_at(weight, start + li); }
    const bool bad = have && weight_bad(wf);
    const uint32_t key = (have && !bad) ? sortable_key(s) : KEY_NAN;
    const bool nan = have && !bad && key == KEY_NAN;
    const bool valid = have && !bad && !nan;
    const bool pos = valid && y > 0.5f;
    const bool neg = valid && !pos;
    const double w = valid ? (double)wf : 0.0;      // (-0.0f widens to -0.0, which adds as 0)
    neg_keys[lane] = neg ? key : KEY_NAN;
    neg_w[lane] = neg ? wf : 0.0f;
    __syncthreads();
    double below = 0.0, at = 0.0;
    for (int j = 0; j < W; j += 4) {
      const uint4 kk = *reinterpret_cast<const uint4*>(&neg_keys[base + j]);
      const float4 ww = *reinterpret_cast<const float4*>(&neg_w[base + j]);
      below += kk.x < key ? (double)ww.x : 0.0;  at += kk.x == key ? (double)ww.x : 0.0;
      below += kk.y < key ? (double)ww.y : 0.0;  at += kk.y == key ? (double)ww.y : 0.0;
      below += kk.z < key ? (double)ww.z : 0.0;  at += kk.z == key ? (double)ww.z : 0.0;
      below += kk.w < key ? (double)ww.w : 0.0;  at += kk.w == key ? (double)ww.w : 0.0;
    }
    __syncthreads();   // the next pass overwrites the pairs
    double term = pos ? w_term(w, below, at) : 0.0;
    double wp = pos ? w : 0.0, wn = neg ? w : 0.0;
    uint32_t c = (nan ? 1u : 0u) | ((bad ? 1u : 0u) << 16);   // two counts <= 64 in one word
    for (int off = 1; off < W; off <<= 1) {
      term += __shfl_xor(term, off);
      wp += __shfl_xor(wp, off);
      wn += __shfl_xor(wn, off);
      c += __shfl_xor(c, off);
    }
    if (ent_ok && li == 0) write_w(O, e0 + k, term, wp, wn, (int)(c & 0xFFFFu), (int)(c >> 16));
  }
}

// ---- the sort path: keys and values ----------------------------------------------------------------------------------------------------
// one thread per sample of a large entity, in the entities' order (eval_big_keys_kernel's search): the composite key and the canonical weight
__global__ void w_big_pairs_kernel(const int64_t* __restrict__ ent_row_ptr, const int32_t* __restrict__ big_list, const int32_t* __restrict__ big_off,
                                   int nbig, int64_t M, const float* __restrict__ score, const float* __restrict__ label, const float* __restrict__ weight,
                                   uint64_t* __restrict__ keys, uint32_t* __restrict__ vals) {
  const int64_t m = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (m >= M) return;
  int lo = 0, hi = nbig - 1;   // the last b with big_off[b] <= m
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if ((int64_t)big_off[mid] <= m) lo = mid; else hi = mid - 1;
  }
  const int64_t i = ent_row_ptr[big_list[lo]] + (m - big_off[lo]);
  const uint32_t wb = weight_bits(weight_at(weight, i));
  keys[m] = ((uint64_t)lo << 33) | (wb == W_BAD_BITS ? KEY33_BAD : key33(score[i], label[i]));
  vals[m] = wb;
}
// the accumulator's word of a sample
__global__ void w_acc_add_kernel(const float* __restrict__ score, const float* __restrict__ label, const float* __restrict__ weight, int64_t N,
                                 uint64_t* __restrict__ words) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < N; i += stride) {
    const uint32_t wb = weight_bits(weight_at(weight, i));
    words[i] = wb == W_BAD_BITS ? ~0ull : ((key33(score[i], label[i]) << 31) | (uint64_t)wb);
  }
}

// where the scan reads element i from: key = segment << 33 | key33, bits = the canonical weight
struct PairSrc {
  const uint64_t* keys; const uint32_t* vals;
  __device__ __forceinline__ uint64_t key(int64_t i) const { return keys[i]; }
  __device__ __forceinline__ uint32_t bits(int64_t i) const { return vals[i]; }
};
struct WordSrc {
  const uint64_t* words;
  __device__ __forceinline__ uint64_t key(int64_t i) const { return words[i] >> 31; }
  __device__ __forceinline__ uint32_t bits(int64_t i) const { return (uint32_t)words[i] & 0x7FFFFFFFu; }
};

// ---- the scan -------------------------------------------------------------------------------------------------------------------------
// The state of a stretch of sorted elements. n, p: the negative and positive weight behind its last segment head (of the whole stretch if
// it has none), nan, bad: the counts there. gp, gn: the positive and negative weight behind its last tie-group head (a segment head is one);
// bef: the negative weight between its last segment head (or its start) and its last tie-group head. f: it has a tie-group head (1), a
// segment head (2). Only sums of non-negative numbers: a head REPLACES the left stretch's sum.
struct WState { double n, p, bef, gp, gn; uint32_t nan, bad, f; };
__device__ __forceinline__ WState rank_combine(const WState& a, const WState& b) {
  WState r;
  const bool seg = (b.f & 2u) != 0u;
  r.n = seg ? b.n : a.n + b.n;
  r.p = seg ? b.p : a.p + b.p;
  r.nan = seg ? b.nan : a.nan + b.nan;
  r.bad = seg ? b.bad : a.bad + b.bad;
  if (b.f & 1u) {
    r.gp = b.gp; r.gn = b.gn;
    r.bef = seg ? b.bef : a.n + b.bef;
  } else {
    r.gp = a.gp + b.gp; r.gn = a.gn + b.gn;
    r.bef = a.bef;
  }
  r.f = a.f | b.f;
  return r;
}
__device__ __forceinline__ WState w_element(uint64_t key, uint32_t bits, uint64_t prev, bool first) {
  WState r;
  const uint64_t k33 = key & KEY33_BAD;
  const bool bad = k33 == KEY33_BAD;
  const bool nan = !bad && (uint32_t)(k33 >> 1) == KEY_NAN;
  const double w = (bad || nan) ? 0.0 : (double)__uint_as_float(bits);
  const bool pos = (k33 & 1ull) != 0ull;
  r.p = pos ? w : 0.0;
  r.n = pos ? 0.0 : w;
  r.gp = r.p; r.gn = r.n; r.bef = 0.0;
  r.nan = nan ? 1u : 0u;
  r.bad = bad ? 1u : 0u;
  r.f = ((first || (key >> 1) != (prev >> 1)) ? 1u : 0u) | ((first || (key >> 33) != (prev >> 33)) ? 2u : 0u);
  return r;
}
__device__ __forceinline__ WState w_none() { return {0.0, 0.0, 0.0, 0.0, 0.0, 0u, 0u, 0u}; }   // the empty stretch: adds exact zeros
__device__ __forceinline__ int w_count(int64_t M, int64_t first) {
  const int64_t left = M - first;
  return left <= 0 ? 0 : (left < W_SCAN_ITEMS ? (int)left : W_SCAN_ITEMS);
}
template <class Src>
__device__ __forceinline__ WState w_fold(const Src& src, int64_t first, int cnt) {
  WState v = w_none();
  uint64_t p = (cnt > 0 && first > 0) ? src.key(first - 1) : 0ull;
  for (int j = 0; j < cnt; ++j) {
    const uint64_t k = src.key(first + j);
    v = rank_combine(v, w_element(k, src.bits(first + j), p, first + j == 0));
    p = k;
  }
  return v;
}
template <class Src>
__global__ __launch_bounds__(W_SCAN_THREADS) void w_reduce_kernel(Src src, int64_t M, WState* __restrict__ partial) {
  __shared__ WState lds[W_SCAN_THREADS];
  const int64_t first = (int64_t)blockIdx.x * W_SCAN_TILE + (int64_t)threadIdx.x * W_SCAN_ITEMS;
  const WState v = eval_block_scan<W_SCAN_THREADS>(w_fold(src, first, w_count(M, first)), lds);
  if (threadIdx.x == W_SCAN_THREADS - 1) partial[blockIdx.x] = v;
}
struct WSegTotals { double w_pos, w_neg; int32_t n_nan, n_bad; };
// A thread walks its keys with the state in front of them (pr_scan_kernel's walk). The LAST element of a tie group writes the group's term,
// every other position 0.0; the last element of a segment also writes the segment's totals. Every position of `terms` and every segment of
// `seg` is written by exactly one thread: no atomics.
template <class Src>
__global__ __launch_bounds__(W_SCAN_THREADS) void w_scan_kernel(Src src, int64_t M, const WState* __restrict__ partial, double* __restrict__ terms,
                                                                WSegTotals* __restrict__ seg) {
  __shared__ WState lds[W_SCAN_THREADS];
  __shared__ WState block_prefix;
  const int t = threadIdx.x;
  // the state in front of this workgroup's tile: the partials of the tiles before it, folded in order
  {
    const int nb = blockIdx.x;
    const int c = (nb + W_SCAN_THREADS - 1) / W_SCAN_THREADS;
    WState v = w_none();
    for (int j = t * c; j < (t + 1) * c && j < nb; ++j) v = rank_combine(v, partial[j]);
    v = eval_block_scan<W_SCAN_THREADS>(v, lds);
    if (t == W_SCAN_THREADS - 1) block_prefix = v;
    __syncthreads();
  }
  const int64_t first = (int64_t)blockIdx.x * W_SCAN_TILE + (int64_t)t * W_SCAN_ITEMS;
  const int cnt = w_count(M, first);
  (void)eval_block_scan<W_SCAN_THREADS>(w_fold(src, first, cnt), lds);
  WState run = block_prefix;
  if (t > 0) run = rank_combine(run, lds[t - 1]);   // (lds holds the inclusive scan)
  uint64_t p = (cnt > 0 && first > 0) ? src.key(first - 1) : 0ull;
  uint64_t k = cnt > 0 ? src.key(first) : 0ull;
  for (int j = 0; j < cnt; ++j) {
    const int64_t i = first + j;
    const bool at_end = i + 1 == M;
    const uint64_t next = at_end ? 0ull : src.key(i + 1);
    run = rank_combine(run, w_element(k, src.bits(i), p, i == 0));
    double term = 0.0;
    if (at_end || (next >> 1) != (k >> 1)) {
      term = w_term(run.gp, run.bef, run.gn);
      if (at_end || (next >> 33) != (k >> 33)) {
        WSegTotals tot;
        tot.w_pos = run.p; tot.w_neg = run.n; tot.n_nan = (int32_t)run.nan; tot.n_bad = (int32_t)run.bad;
        seg[k >> 33] = tot;
      }
    }
    terms[i] = term;
    p = k; k = next;
  }
}

// one workgroup per large entity: the fixed-shape sum over its segment of `terms`, then its outputs
__global__ __launch_bounds__(EVAL_THREADS) void w_big_finish_kernel(const int64_t* __restrict__ ent_row_ptr, const int32_t* __restrict__ big_list,
                                                                    const int32_t* __restrict__ big_off, const double* __restrict__ terms,
                                                                    const WSegTotals* __restrict__ seg, WOutDev O) {
  __shared__ double lds[EVAL_THREADS];
  const int b = blockIdx.x;
  const int64_t e = big_list[b];
  const int64_t n = ent_row_ptr[e + 1] - ent_row_ptr[e], m0 = big_off[b];
  const double sum = eval_block_tree(terms_lane(terms, m0 + threadIdx.x, m0 + n, EVAL_THREADS), lds);
  if (threadIdx.x == 0) {
    const WSegTotals c = seg[b];
    write_w(O, e, sum, c.w_pos, c.w_neg, c.n_nan, c.n_bad);
  }
}

static size_t w_up256(size_t x) { return (x + 255) & ~(size_t)255; }
static int64_t w_tiles(int64_t M) { return (M + W_SCAN_TILE - 1) / W_SCAN_TILE; }

struct WLayout { size_t mark, offs, big_list, big_off, keys_a, keys_b, vals_a, vals_b, terms, partial, seg, total; };
static WLayout w_layout(int64_t E, int64_t N) {
  WLayout L;
  size_t off = 0;
  auto take = [&](size_t bytes) { const size_t o = off; off = w_up256(off + bytes); return o; };
  L.mark = take((size_t)(E + 1) * 8);
  L.offs = take((size_t)(E + 1) * 8);
  L.big_list = take((size_t)(E + 1) * 4);
  L.big_off = take((size_t)(E + 1) * 4);
  L.keys_a = take((size_t)N * 8);
  L.keys_b = take((size_t)N * 8);
  L.vals_a = take((size_t)N * 4);
  L.vals_b = take((size_t)N * 4);
  L.terms = take((size_t)N * 8);
  L.partial = take((size_t)(w_tiles(N) + 1) * sizeof(WState));
  L.seg = take((size_t)(E + 1) * sizeof(WSegTotals));
  L.total = off;
  return L;
}
struct WAccLayout { size_t sorted, terms, partial, seg, group_sum, sum, total; };
static WAccLayout w_acc_layout(int64_t N) {
  WAccLayout L;
  size_t off = 0;
  auto take = [&](size_t bytes) { const size_t o = off; off = w_up256(off + bytes); return o; };
  L.sorted = take((size_t)N * 8);
  L.terms = take((size_t)N * 8);
  L.partial = take((size_t)(w_tiles(N) + 1) * sizeof(WState));
  L.seg = take(sizeof(WSegTotals));
  L.group_sum = take((size_t)ACC_MAX_GROUPS * 8);
  L.sum = take(8);
  L.total = off;
  return L;
}

// sorted elements -> terms[M] and the segments' totals
template <class Src>
static int w_terms(const Src& src, int64_t M, WState* partial, double* terms, WSegTotals* seg, hipStream_t s) {
  const int nb = (int)w_tiles(M);
  hipLaunchKernelGGL(w_reduce_kernel<Src>, dim3(nb), dim3(W_SCAN_THREADS), 0, s, src, M, partial);
  hipLaunchKernelGGL(w_scan_kernel<Src>, dim3(nb), dim3(W_SCAN_THREADS), 0, s, src, M, (const WState*)partial, terms, seg);
  HIP_TRY(hipGetLastError());
  return GDMIX_RE_OK;
}

// the one radix sort of the sort path: 8-byte keys over the bits in use, the 4-byte weight carried as the value
static int w_sort_pairs(gdmix_ctx_impl* ci, uint64_t* keys_in, uint64_t* keys_out, uint32_t* vals_in, uint32_t* vals_out, int64_t M, unsigned end_bit,
                        hipStream_t s) {
  unsigned long long* const nokey = nullptr;
  uint32_t* const noval = nullptr;
  size_t bytes = 0;
  HIP_TRY((rocprim::radix_sort_pairs(nullptr, bytes, nokey, nokey, noval, noval, (size_t)M, 0u, end_bit, s)));
  void* tmp = nullptr;
  const int rc = eval_tmp(ci, bytes ? bytes : 1, s, &tmp);
  if (rc != GDMIX_RE_OK) return rc;
  HIP_TRY((rocprim::radix_sort_pairs(tmp, bytes, reinterpret_cast<unsigned long long*>(keys_in), reinterpret_cast<unsigned long long*>(keys_out), vals_in,
                                     vals_out, (size_t)M, 0u, end_bit, s)));
  return GDMIX_RE_OK;
}

}  // namespace gdmix

using namespace gdmix;

extern "C" {

GDMIX_API size_t gdmix_re_eval_w_workspace_bytes(int64_t E, int64_t N) {
  if (E < 0 || N < 0 || E >= EVAL_LIMIT || N >= EVAL_LIMIT) return 0;
  return w_layout(E, N).total;
}

GDMIX_API int gdmix_re_eval_w_entities(gdmix_re_ctx* ctx, const int64_t* ent_row_ptr, int64_t E, int64_t N, const float* score, const float* label,
                                       const float* weight, const gdmix_re_eval_w_out* out, void* workspace, size_t workspace_bytes, void* stream) {
  if (!ctx || !out || E < 0 || N < 0) { set_error("gdmix_re_eval_w_entities: bad argument"); return GDMIX_RE_EINVAL; }
  if (N >= EVAL_LIMIT || E >= EVAL_LIMIT) {
    set_error("gdmix_re_eval_w_entities: %lld samples / %lld entities; an evaluation takes fewer than 2^31 of each", (long long)N, (long long)E);
    return GDMIX_RE_ERANGE;
  }
  if (E == 0) return GDMIX_RE_OK;
  if (!ent_row_ptr || (N > 0 && (!score || !label))) { set_error("gdmix_re_eval_w_entities: NULL input"); return GDMIX_RE_EINVAL; }
  const WLayout L = w_layout(E, N);
  if (!workspace || workspace_bytes < L.total) {
    set_error("gdmix_re_eval_w_entities: workspace of %zu bytes, %zu needed (gdmix_re_eval_w_workspace_bytes)", workspace_bytes, L.total);
    return GDMIX_RE_ENOMEM;
  }
  gdmix_ctx_impl* ci = &ctx->impl;
  hipStream_t s = static_cast<hipStream_t>(stream);
  char* base = static_cast<char*>(workspace);
  const int small_max = ci->eval_small_set ? ci->eval_small_max : 64;
  const WOutDev O = {out->two_u_w, out->w_pos, out->w_neg, out->n_nan, out->n_bad_weight, out->auc};
  // (with a limit of 0 this launch still writes the entities of no samples)
  hipLaunchKernelGGL(w_small_kernel, dim3((unsigned)((E + 3) / 4)), dim3(64), 0, s, ent_row_ptr, E, score, label, weight, O, small_max);
  HIP_TRY(hipGetLastError());
  int32_t* big_list = reinterpret_cast<int32_t*>(base + L.big_list);
  int32_t* big_off = reinterpret_cast<int32_t*>(base + L.big_off);
  int64_t nbig = 0, M = 0;
  int rc = eval_number_big(ci, "gdmix_re_eval_w_entities", ent_row_ptr, E, N, small_max, reinterpret_cast<int64_t*>(base + L.mark),
                           reinterpret_cast<int64_t*>(base + L.offs), big_list, big_off, s, &nbig, &M);
  if (rc != GDMIX_RE_OK || nbig == 0) return rc;
  uint64_t* keys_a = reinterpret_cast<uint64_t*>(base + L.keys_a);
  uint64_t* keys_b = reinterpret_cast<uint64_t*>(base + L.keys_b);
  uint32_t* vals_a = reinterpret_cast<uint32_t*>(base + L.vals_a);
  uint32_t* vals_b = reinterpret_cast<uint32_t*>(base + L.vals_b);
  double* terms = reinterpret_cast<double*>(base + L.terms);
  WSegTotals* seg = reinterpret_cast<WSegTotals*>(base + L.seg);
  hipLaunchKernelGGL(w_big_pairs_kernel, dim3((unsigned)((M + 255) / 256)), dim3(256), 0, s, ent_row_ptr, (const int32_t*)big_list, (const int32_t*)big_off,
                     (int)nbig, M, score, label, weight, keys_a, vals_a);
  HIP_TRY(hipGetLastError());
  unsigned sbits = 0;
  while (((int64_t)1 << sbits) < nbig) ++sbits;
  rc = w_sort_pairs(ci, keys_a, keys_b, vals_a, vals_b, M, 33u + sbits, s);
  if (rc != GDMIX_RE_OK) return rc;
  const PairSrc src = {keys_b, vals_b};
  rc = w_terms(src, M, reinterpret_cast<WState*>(base + L.partial), terms, seg, s);
  if (rc != GDMIX_RE_OK) return rc;
  hipLaunchKernelGGL(w_big_finish_kernel, dim3((unsigned)nbig), dim3(EVAL_THREADS), 0, s, ent_row_ptr, (const int32_t*)big_list, (const int32_t*)big_off,
                     (const double*)terms, (const WSegTotals*)seg, O);
  HIP_TRY(hipGetLastError());
  return GDMIX_RE_OK;
}

GDMIX_API int gdmix_re_eval_w_acc_add(gdmix_re_ctx* ctx, gdmix_re_eval_acc* acc, const float* score, const float* label, const float* weight, int64_t N,
                                      void* stream) {
  if (!ctx || !acc || !acc->state || N < 0 || acc->capacity < 0 || acc->count < 0) { set_error("gdmix_re_eval_w_acc_add: bad argument"); return GDMIX_RE_EINVAL; }
  if (N == 0) return GDMIX_RE_OK;
  if (acc->count + N >= EVAL_LIMIT) {
    set_error("gdmix_re_eval_w_acc_add: %lld + %lld samples; an evaluation takes fewer than 2^31", (long long)acc->count, (long long)N);
    return GDMIX_RE_ERANGE;
  }
  if (!acc->keys || acc->count + N > acc->capacity) {
    set_error("gdmix_re_eval_w_acc_add: key buffer of %lld samples, %lld + %lld to hold", (long long)acc->capacity, (long long)acc->count, (long long)N);
    return GDMIX_RE_ENOMEM;
  }
  if (!score || !label) { set_error("gdmix_re_eval_w_acc_add: NULL input"); return GDMIX_RE_EINVAL; }
  const int64_t blocks = (N + 256 * 16 - 1) / (256 * 16);
  hipLaunchKernelGGL(w_acc_add_kernel, dim3((unsigned)(blocks > 65536 ? 65536 : blocks)), dim3(256), 0, static_cast<hipStream_t>(stream), score, label, weight, N,
                     acc->keys + acc->count);
  HIP_TRY(hipGetLastError());
  acc->count += N;
  return GDMIX_RE_OK;
}

GDMIX_API size_t gdmix_re_eval_w_acc_workspace_bytes(int64_t N) {
  if (N < 0 || N >= EVAL_LIMIT) return 0;
  return w_acc_layout(N).total;
}

GDMIX_API int gdmix_re_eval_w_acc_finish(gdmix_re_ctx* ctx, const gdmix_re_eval_acc* acc, void* workspace, size_t workspace_bytes,
                                         gdmix_re_eval_w_totals* host_out, void* stream) {
  if (!ctx || !acc || !host_out || acc->count < 0 || acc->count >= EVAL_LIMIT) { set_error("gdmix_re_eval_w_acc_finish: bad argument"); return GDMIX_RE_EINVAL; }
  const int64_t M = acc->count;
  host_out->two_u_w = 0.0; host_out->w_pos = 0.0; host_out->w_neg = 0.0;
  host_out->n = M; host_out->n_nan = 0; host_out->n_bad_weight = 0;
  if (M == 0) return GDMIX_RE_OK;
  const WAccLayout L = w_acc_layout(M);
  if (!workspace || workspace_bytes < L.total || !acc->keys || acc->capacity < M) {
    set_error("gdmix_re_eval_w_acc_finish: workspace of %zu bytes, %zu needed for %lld samples (gdmix_re_eval_w_acc_workspace_bytes)", workspace_bytes, L.total,
              (long long)M);
    return GDMIX_RE_ENOMEM;
  }
  gdmix_ctx_impl* ci = &ctx->impl;
  hipStream_t s = static_cast<hipStream_t>(stream);
  char* base = static_cast<char*>(workspace);
  uint64_t* sorted = reinterpret_cast<uint64_t*>(base + L.sorted);
  double* terms = reinterpret_cast<double*>(base + L.terms);
  WSegTotals* seg = reinterpret_cast<WSegTotals*>(base + L.seg);
  double* sum = reinterpret_cast<double*>(base + L.sum);
  // the accumulator's words are read, not written; all 64 bits take part: equal keys are ordered by their weights
  int rc = sort_keys(ci, acc->keys, sorted, M, 64u, s);
  if (rc != GDMIX_RE_OK) return rc;
  const WordSrc src = {sorted};
  rc = w_terms(src, M, reinterpret_cast<WState*>(base + L.partial), terms, seg, s);
  if (rc != GDMIX_RE_OK) return rc;
  rc = eval_sum_positions(terms, M, reinterpret_cast<double*>(base + L.group_sum), sum, s);
  if (rc != GDMIX_RE_OK) return rc;
  WSegTotals tot = {0.0, 0.0, 0, 0};
  double two_u_w = 0.0;
  HIP_TRY(hipMemcpyAsync(&tot, seg, sizeof(tot), hipMemcpyDeviceToHost, s));
  HIP_TRY(hipMemcpyAsync(&two_u_w, sum, 8, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  host_out->two_u_w = two_u_w;
  host_out->w_pos = tot.w_pos;
  host_out->w_neg = tot.w_neg;
  host_out->n_nan = tot.n_nan;
  host_out->n_bad_weight = tot.n_bad;
  return GDMIX_RE_OK;
}

}  // extern "C"
