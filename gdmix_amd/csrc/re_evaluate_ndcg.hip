// re_evaluate_ndcg.hip — NDCG@K on graded labels, per entity: the two discounted sums dcg and idcg for up to four K and the three counts.
// The contract (valid samples, the label domain, gain, discount, ties in expectation, the bound) is stated in include/gdmix_re.h, "NDCG";
// this unit is its only implementation. The division and the null cases are the host's (gdmix_amd/metrics.py).
//
//   terms              Every path adds one non-negative fp64 term per RANK or per TIE GROUP; nothing is ever subtracted (no prefix sum of
//                      discounts is differenced), so every sum keeps a relative bound.
//                        gain      ndcg_gain: 2^y - 1. y = i + f; 2^i by the exponent; an integral label gives (2^i) - 1. A fraction f goes
//                                  through exp_any and log_1_2 of re_device.hpp: m = 2^f - 1 = (u - 1) x / log(u) with x = f ln 2, u = exp(x)
//                                  (the classical expm1 from exp and log: relative accuracy for a small f too), gain = fma(2^i, m, 2^i - 1).
//                        discount  ndcg_disc: ln 2 / log(r + 2), log(r + 2) = e ln 2 + log_1_2(m) with r + 2 = m 2^e.
//   ndcg_small_kernel  entities of at most 64 samples, no sort: topk_small_kernel's geometry (four consecutive entities per wavefront, 16, 32
//                      or 64 lanes each, lane i holds sample i). Through LDS go the complemented score keys, the label keys and the fp64
//                      gains. A lane learns: a, the keys above its own; t, the keys equal to it; G, its tie group's gain sum (in lane order);
//                      how many equal keys sit on lower lanes — rank rs = a + that, distinct inside the entity —; and the same two counts
//                      over the label keys — the ideal rank ri. The lane of rank rs < K adds (G / t) d(rs) to dcg@K: summed over the ranks
//                      [a, min(a + t, K)) of a group that is the group's gain mean times its discounts, the expectation under a random order
//                      inside the group. Every lane adds g d(ri) to idcg@K when ri < K. d(0 .. 63) is a table built once per wavefront in
//                      LDS. xor butterflies over the entity's lanes add the 2 nk sums and the counts. All K from the one ranking.
//   sort path          entities above the small limit, numbered by eval_number_big (re_evaluate.hip). ndcg_keys_kernel writes, per sample,
//                      segment << 32 | complemented score key (a NaN score: all ones, last in its segment) with the label's bits as the
//                      VALUE of one rocPRIM radix sort of pairs, and segment << 32 | complemented label key for a second sort of keys only
//                      (labels descend; a sample that is not valid or whose label is bad gets the key of label 0: gain 0 wherever it lands).
//                      ndcg_reduce_kernel / ndcg_scan_kernel: reduce-then-scan over the first array, a SEGMENTED sum restarted at every
//                      tie-group head of (gain, discounts of the ranks below each K, size); the rank is the position inside the segment. The
//                      last element of a group writes (G / t) * D_K per K, every other position 0.0. ndcg_ideal_kernel: g d(r) per position of
//                      the second array. ndcg_big_finish_kernel: a workgroup per entity adds its segments in the fixed tree of re_eval_sum.hpp
//                      (idcg@K over the first min(K, n) positions) and counts.
#include <stdint.h>
#include <math.h>

#include <rocprim/device/device_radix_sort.hpp>

#include "re_internal.hpp"
#include "re_device.hpp"
#include "re_eval_sum.hpp"

namespace gdmix {

constexpr int NDCG_MAX = 4;                                  // values of K in one call
constexpr int NDCG_SCAN_THREADS = 256, NDCG_SCAN_ITEMS = 16, NDCG_SCAN_TILE = NDCG_SCAN_THREADS * NDCG_SCAN_ITEMS;
static_assert(NDCG_SCAN_TILE == GDMIX_RE_EVAL_NDCG_SCAN_TILE, "the scan's tile, as the header names it");
static_assert(NDCG_SCAN_THREADS == EVAL_THREADS, "the sort path's workgroup width is the summing workgroups'");
constexpr double NDCG_LN2 = 6.93147180559945309417e-01, NDCG_LN2_HI = 6.93147180369123816490e-01, NDCG_LN2_LO = 1.90821492927058770002e-10;

struct NdcgKs { int32_t k[NDCG_MAX]; int nk; int32_t kmax; };   // kmax: the largest of them
struct NdcgOutDev { double* dcg; double* idcg; int32_t* n; int32_t* n_nan; int32_t* n_bad; };

// the label domain: finite and in [0, 64] (-0 is 0)
__device__ __forceinline__ bool label_bad(float y) { return !(y >= 0.0f && y <= 64.0f); }
// the key labels are ranked by: the bits of a good label (non-negative floats order as their bits; -0 -> 0), 0 for anything else
__device__ __forceinline__ uint32_t label_key(float y, bool counts) { return (counts && !label_bad(y) && y != 0.0f) ? __float_as_uint(y) : 0u; }

// 2^y - 1 for y in [0, 64]
__device__ __forceinline__ double ndcg_gain(double y) {
  const double fl = floor(y);
  const double f = y - fl;                                    // exact
  const double p = __builtin_amdgcn_ldexp(1.0, (int)fl);      // 2^i
  const double whole = p - 1.0;                               // exact up to i = 53, correctly rounded beyond
  if (f == 0.0) return whole;
  const double x = f * NDCG_LN2;
  const double u = exp_any(x);                                // in [1, 2]
  const double m = (u == 1.0) ? x : (u - 1.0) * x / log_1_2(u);
  return __builtin_fma(p, m, whole);
}
__device__ __forceinline__ double gain_of_bits(uint32_t label_bits) { return label_bits ? ndcg_gain((double)__uint_as_float(label_bits)) : 0.0; }

// 1 / log2(r + 2) for the 0-based rank r < 2^31
__device__ __forceinline__ double ndcg_disc(int64_t r) {
  const uint64_t x = (uint64_t)r + 2u;
  const int e = 63 - __clzll((long long)x);
  const double m = __builtin_amdgcn_ldexp((double)x, -e);     // in [1, 2), exact
  const double L = (double)e * NDCG_LN2_HI + __builtin_fma((double)e, NDCG_LN2_LO, log_1_2(m));   // (e ln2_hi is exact: ln2_hi has 32 bits)
  return NDCG_LN2 / L;
}

// ---- small entities ---------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void ndcg_small_kernel(const int64_t* __restrict__ ent_row_ptr, int64_t E, const float* __restrict__ score,
                                                        const float* __restrict__ label, NdcgOutDev O, NdcgKs K, int small_max) {
  __shared__ __attribute__((aligned(16))) uint32_t s_keys[64];
  __shared__ __attribute__((aligned(16))) uint32_t l_keys[64];
  __shared__ __attribute__((aligned(16))) double gains[64];
  __shared__ double disc[64];
  const int lane = threadIdx.x;
  disc[lane] = ndcg_disc(lane);
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
    float s = 0.0f, y = 0.0f;
    if (have) { s = score[start + li]; y = label[start + li]; }
    const uint32_t sk = have ? sortable_key(s) : KEY_NAN;
    const bool nan = have && sk == KEY_NAN;
    const bool valid = have && !nan;
    const bool bad = valid && label_bad(y);
    const uint32_t key = valid ? ~sk : KEY_NAN;       // a smaller key is a greater score; KEY_NAN (no valid score has it) is above them all
    const uint32_t lk = label_key(y, valid);
    const double gain = gain_of_bits(lk);
    s_keys[lane] = key;
    l_keys[lane] = lk;
    gains[lane] = gain;
    __syncthreads();
    uint32_t a = 0, t = 0, lower = 0, la = 0, llower = 0;
    double G = 0.0;
    for (int j = 0; j < W; j += 4) {
      const uint4 kk = *reinterpret_cast<const uint4*>(&s_keys[base + j]);
      const uint4 ll = *reinterpret_cast<const uint4*>(&l_keys[base + j]);
      const double2 g01 = *reinterpret_cast<const double2*>(&gains[base + j]);
      const double2 g23 = *reinterpret_cast<const double2*>(&gains[base + j + 2]);
      const bool e0q = kk.x == key, e1q = kk.y == key, e2q = kk.z == key, e3q = kk.w == key;
      a += (uint32_t)(kk.x < key) + (uint32_t)(kk.y < key) + (uint32_t)(kk.z < key) + (uint32_t)(kk.w < key);
      t += (uint32_t)e0q + (uint32_t)e1q + (uint32_t)e2q + (uint32_t)e3q;
      lower += (uint32_t)(e0q && j < li) + (uint32_t)(e1q && j + 1 < li) + (uint32_t)(e2q && j + 2 < li) + (uint32_t)(e3q && j + 3 < li);
      G += e0q ? g01.x : 0.0;  G += e1q ? g01.y : 0.0;  G += e2q ? g23.x : 0.0;  G += e3q ? g23.y : 0.0;
      la += (uint32_t)(ll.x > lk) + (uint32_t)(ll.y > lk) + (uint32_t)(ll.z > lk) + (uint32_t)(ll.w > lk);
      llower += (uint32_t)(ll.x == lk && j < li) + (uint32_t)(ll.y == lk && j + 1 < li) + (uint32_t)(ll.z == lk && j + 2 < li) +
                (uint32_t)(ll.w == lk && j + 3 < li);
    }
    const int rs = (int)(a + lower), ri = (int)(la + llower);   // both below W <= 64 (rs of a lane that is not valid is not used)
    const double per_rank = valid ? (G / (double)t) * disc[rs & 63] : 0.0;
    const double ideal = gain * disc[ri & 63];
    __syncthreads();   // the next pass overwrites the keys
    uint32_t c = (valid ? 1u : 0u) | ((nan ? 1u : 0u) << 8) | ((bad ? 1u : 0u) << 16);   // three counts <= 64 in one word
    for (int off = 1; off < W; off <<= 1) c += __shfl_xor(c, off);
    if (ent_ok && li == 0) {
      if (O.n) O.n[e0 + k] = (int)(c & 0xFFu);
      if (O.n_nan) O.n_nan[e0 + k] = (int)((c >> 8) & 0xFFu);
      if (O.n_bad) O.n_bad[e0 + k] = (int)(c >> 16);
    }
    for (int kk = 0; kk < K.nk; ++kk) {
      const int kv = K.k[kk];
      double d = rs < kv ? per_rank : 0.0, id = ri < kv ? ideal : 0.0;
      for (int off = 1; off < W; off <<= 1) {
        d += __shfl_xor(d, off);
        id += __shfl_xor(id, off);
      }
      if (ent_ok && li == 0) {
        const size_t at = (size_t)kk * (size_t)E + (size_t)(e0 + k);
        if (O.dcg) O.dcg[at] = d;
        if (O.idcg) O.idcg[at] = id;
      }
    }
  }
}

// ---- the sort path: keys and values ----------------------------------------------------------------------------------------------------
// one thread per sample of a large entity, in the entities' order (eval_big_keys_kernel's search)
__global__ void ndcg_keys_kernel(const int64_t* __restrict__ ent_row_ptr, const int32_t* __restrict__ big_list, const int32_t* __restrict__ big_off,
                                 int nbig, int64_t M, const float* __restrict__ score, const float* __restrict__ label,
                                 uint64_t* __restrict__ s_keys, uint32_t* __restrict__ s_vals, uint64_t* __restrict__ l_keys) {
  const int64_t m = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (m >= M) return;
  int lo = 0, hi = nbig - 1;   // the last b with big_off[b] <= m
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if ((int64_t)big_off[mid] <= m) lo = mid; else hi = mid - 1;
  }
  const int64_t i = ent_row_ptr[big_list[lo]] + (m - big_off[lo]);
  const uint32_t sk = sortable_key(score[i]);
  const bool valid = sk != KEY_NAN;
  const float y = label[i];
  s_keys[m] = ((uint64_t)lo << 32) | (uint64_t)(valid ? ~sk : KEY_NAN);
  s_vals[m] = __float_as_uint(y);
  l_keys[m] = ((uint64_t)lo << 32) | (uint64_t)(~label_key(y, valid));
}

// The state of a stretch of sorted elements: g, d[k], cnt — the gain sum, the sum of the discounts of the ranks below K_k and the number of
// elements behind its last tie-group head (of the whole stretch if it has none); f: it has a head. A segment's first element is a head
// (the segment number is part of the key). Only sums of non-negative numbers: a head REPLACES the left stretch's sums.
struct NState { double g; double d[NDCG_MAX]; uint32_t cnt, f; };
__device__ __forceinline__ NState rank_combine(const NState& a, const NState& b) {
  if (b.f) return b;
  NState r;
  r.g = a.g + b.g;
#pragma unroll
  for (int k = 0; k < NDCG_MAX; ++k) r.d[k] = a.d[k] + b.d[k];
  r.cnt = a.cnt + b.cnt;
  r.f = a.f;
  return r;
}
__device__ __forceinline__ NState ndcg_none() { return {0.0, {0.0, 0.0, 0.0, 0.0}, 0u, 0u}; }   // the empty stretch: adds exact zeros
// element i of the sorted pairs: its rank is its position in its segment
__device__ __forceinline__ NState ndcg_element(uint64_t key, uint32_t bits, uint64_t prev, int64_t i, const int32_t* __restrict__ big_off, const NdcgKs& K) {
  NState r;
  const bool valid = (uint32_t)key != KEY_NAN;
  const float y = __uint_as_float(bits);
  r.g = gain_of_bits(label_key(y, valid));
  const int64_t rank = i - (int64_t)big_off[key >> 32];
  const double d = (valid && rank < (int64_t)K.kmax) ? ndcg_disc(rank) : 0.0;   // no discount is formed beyond the largest K
#pragma unroll
  for (int k = 0; k < NDCG_MAX; ++k) r.d[k] = (k < K.nk && rank < (int64_t)K.k[k]) ? d : 0.0;
  r.cnt = 1u;
  r.f = (i == 0 || key != prev) ? 1u : 0u;
  return r;
}
__device__ __forceinline__ int ndcg_count(int64_t M, int64_t first) {
  const int64_t left = M - first;
  return left <= 0 ? 0 : (left < NDCG_SCAN_ITEMS ? (int)left : NDCG_SCAN_ITEMS);
}
__device__ __forceinline__ NState ndcg_fold(const uint64_t* __restrict__ keys, const uint32_t* __restrict__ vals, int64_t first, int cnt,
                                            const int32_t* __restrict__ big_off, const NdcgKs& K) {
  NState v = ndcg_none();
  uint64_t p = (cnt > 0 && first > 0) ? keys[first - 1] : 0ull;
  for (int j = 0; j < cnt; ++j) {
    const uint64_t k = keys[first + j];
    v = rank_combine(v, ndcg_element(k, vals[first + j], p, first + j, big_off, K));
    p = k;
  }
  return v;
}
__global__ __launch_bounds__(NDCG_SCAN_THREADS) void ndcg_reduce_kernel(const uint64_t* __restrict__ keys, const uint32_t* __restrict__ vals, int64_t M,
                                                                        const int32_t* __restrict__ big_off, NdcgKs K, NState* __restrict__ partial) {
  __shared__ NState lds[NDCG_SCAN_THREADS];
  const int64_t first = (int64_t)blockIdx.x * NDCG_SCAN_TILE + (int64_t)threadIdx.x * NDCG_SCAN_ITEMS;
  const NState v = eval_block_scan<NDCG_SCAN_THREADS>(ndcg_fold(keys, vals, first, ndcg_count(M, first), big_off, K), lds);
  if (threadIdx.x == NDCG_SCAN_THREADS - 1) partial[blockIdx.x] = v;
}
// A thread walks its elements with the state in front of them (w_scan_kernel's walk). The LAST element of a tie group writes the group's
// term per K, every other position 0.0. Every position of dcg_terms[k] is written by exactly one thread: no atomics.
__global__ __launch_bounds__(NDCG_SCAN_THREADS) void ndcg_scan_kernel(const uint64_t* __restrict__ keys, const uint32_t* __restrict__ vals, int64_t M,
                                                                      const int32_t* __restrict__ big_off, NdcgKs K, const NState* __restrict__ partial,
                                                                      double* __restrict__ dcg_terms) {
  __shared__ NState lds[NDCG_SCAN_THREADS];
  __shared__ NState block_prefix;
  const int t = threadIdx.x;
  // the state in front of this workgroup's tile: the partials of the tiles before it, folded in order
  {
    const int nb = blockIdx.x;
    const int c = (nb + NDCG_SCAN_THREADS - 1) / NDCG_SCAN_THREADS;
    NState v = ndcg_none();
    for (int j = t * c; j < (t + 1) * c && j < nb; ++j) v = rank_combine(v, partial[j]);
    v = eval_block_scan<NDCG_SCAN_THREADS>(v, lds);
    if (t == NDCG_SCAN_THREADS - 1) block_prefix = v;
    __syncthreads();
  }
  const int64_t first = (int64_t)blockIdx.x * NDCG_SCAN_TILE + (int64_t)t * NDCG_SCAN_ITEMS;
  const int cnt = ndcg_count(M, first);
  (void)eval_block_scan<NDCG_SCAN_THREADS>(ndcg_fold(keys, vals, first, cnt, big_off, K), lds);
  NState run = block_prefix;
  if (t > 0) run = rank_combine(run, lds[t - 1]);   // (lds holds the inclusive scan)
  uint64_t p = (cnt > 0 && first > 0) ? keys[first - 1] : 0ull;
  uint64_t k = cnt > 0 ? keys[first] : 0ull;
  for (int j = 0; j < cnt; ++j) {
    const int64_t i = first + j;
    const bool at_end = i + 1 == M;
    const uint64_t next = at_end ? 0ull : keys[i + 1];
    run = rank_combine(run, ndcg_element(k, vals[i], p, i, big_off, K));
    const bool group_end = at_end || next != k;
    const double mean = group_end ? run.g / (double)run.cnt : 0.0;
    for (int kk = 0; kk < K.nk; ++kk) dcg_terms[(size_t)kk * (size_t)M + (size_t)i] = group_end ? mean * run.d[kk] : 0.0;
    p = k; k = next;
  }
}
// the sorted label keys (labels descending inside a segment) -> g(y) d(r) per position
__global__ void ndcg_ideal_kernel(const uint64_t* __restrict__ l_sorted, int64_t M, const int32_t* __restrict__ big_off, int32_t kmax,
                                  double* __restrict__ idcg_terms) {
  const int64_t m = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (m >= M) return;
  const uint64_t key = l_sorted[m];
  const uint32_t lk = ~(uint32_t)key;
  const int64_t rank = m - (int64_t)big_off[key >> 32];
  idcg_terms[m] = (lk && rank < (int64_t)kmax) ? gain_of_bits(lk) * ndcg_disc(rank) : 0.0;
}

// one workgroup per large entity: its counts, then the fixed-shape sums over its segments of terms
__global__ __launch_bounds__(EVAL_THREADS) void ndcg_big_finish_kernel(const int64_t* __restrict__ ent_row_ptr, const int32_t* __restrict__ big_list,
                                                                       const int32_t* __restrict__ big_off, const uint64_t* __restrict__ keys,
                                                                       const uint32_t* __restrict__ vals, const double* __restrict__ dcg_terms,
                                                                       const double* __restrict__ idcg_terms, int64_t M, int64_t E, NdcgKs K, NdcgOutDev O) {
  __shared__ double lds[EVAL_THREADS];
  __shared__ unsigned sh_nan, sh_bad;
  const int b = blockIdx.x;
  const int64_t e = big_list[b];
  const int64_t n = ent_row_ptr[e + 1] - ent_row_ptr[e], m0 = big_off[b];
  if (threadIdx.x == 0) { sh_nan = 0u; sh_bad = 0u; }
  __syncthreads();
  unsigned nan = 0u, bad = 0u;
  for (int64_t i = m0 + threadIdx.x; i < m0 + n; i += EVAL_THREADS) {
    const bool valid = (uint32_t)keys[i] != KEY_NAN;
    nan += valid ? 0u : 1u;
    bad += (valid && label_bad(__uint_as_float(vals[i]))) ? 1u : 0u;
  }
  if (nan) atomicAdd(&sh_nan, nan);
  if (bad) atomicAdd(&sh_bad, bad);
  __syncthreads();
  if (threadIdx.x == 0) {
    if (O.n) O.n[e] = (int32_t)(n - (int64_t)sh_nan);
    if (O.n_nan) O.n_nan[e] = (int32_t)sh_nan;
    if (O.n_bad) O.n_bad[e] = (int32_t)sh_bad;
  }
  for (int kk = 0; kk < K.nk; ++kk) {
    const int64_t kv = K.k[kk], top = n < kv ? n : kv;
    const double d = eval_block_tree(terms_lane(dcg_terms + (size_t)kk * (size_t)M, m0 + threadIdx.x, m0 + n, EVAL_THREADS), lds);
    const double id = eval_block_tree(terms_lane(idcg_terms, m0 + threadIdx.x, m0 + top, EVAL_THREADS), lds);
    if (threadIdx.x == 0) {
      const size_t at = (size_t)kk * (size_t)E + (size_t)e;
      if (O.dcg) O.dcg[at] = d;
      if (O.idcg) O.idcg[at] = id;
    }
  }
}

static size_t n_up256(size_t x) { return (x + 255) & ~(size_t)255; }
static int64_t ndcg_tiles(int64_t M) { return (M + NDCG_SCAN_TILE - 1) / NDCG_SCAN_TILE; }

// keys_a: the score keys, later the sorted label keys; keys_b: the sorted score keys; keys_c: the label keys
struct NdcgLayout { size_t mark, offs, big_list, big_off, keys_a, keys_b, keys_c, vals_a, vals_b, dcg_terms, idcg_terms, partial, total; };
static NdcgLayout ndcg_layout(int64_t E, int64_t N) {
  NdcgLayout L;
  size_t off = 0;
  auto take = [&](size_t bytes) { const size_t o = off; off = n_up256(off + bytes); return o; };
  L.mark = take((size_t)(E + 1) * 8);
  L.offs = take((size_t)(E + 1) * 8);
  L.big_list = take((size_t)(E + 1) * 4);
  L.big_off = take((size_t)(E + 1) * 4);
  L.keys_a = take((size_t)N * 8);
  L.keys_b = take((size_t)N * 8);
  L.keys_c = take((size_t)N * 8);
  L.vals_a = take((size_t)N * 4);
  L.vals_b = take((size_t)N * 4);
  L.dcg_terms = take((size_t)N * 8 * NDCG_MAX);
  L.idcg_terms = take((size_t)N * 8);
  L.partial = take((size_t)(ndcg_tiles(N) + 1) * sizeof(NState));
  L.total = off;
  return L;
}

// the first radix sort of the sort path: 8-byte keys over the bits in use, the label's 4 bytes carried as the value
static int ndcg_sort_pairs(gdmix_ctx_impl* ci, uint64_t* keys_in, uint64_t* keys_out, uint32_t* vals_in, uint32_t* vals_out, int64_t M, unsigned end_bit,
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

GDMIX_API size_t gdmix_re_eval_ndcg_workspace_bytes(int64_t E, int64_t N) {
  if (E < 0 || N < 0 || E >= EVAL_LIMIT || N >= EVAL_LIMIT) return 0;
  return ndcg_layout(E, N).total;
}

GDMIX_API int gdmix_re_eval_ndcg_entities(gdmix_re_ctx* ctx, const int64_t* ent_row_ptr, int64_t E, int64_t N, const float* score, const float* label,
                                          const int32_t* ks, int nk, const gdmix_re_eval_ndcg_out* out, void* workspace, size_t workspace_bytes,
                                          void* stream) {
  if (!ctx || !out || E < 0 || N < 0) { set_error("gdmix_re_eval_ndcg_entities: bad argument"); return GDMIX_RE_EINVAL; }
  if (!ks || nk < 1 || nk > NDCG_MAX) { set_error("gdmix_re_eval_ndcg_entities: nk = %d; 1 .. %d values of k in ks", nk, NDCG_MAX); return GDMIX_RE_EINVAL; }
  for (int i = 0; i < nk; ++i) {
    if (ks[i] < 1) { set_error("gdmix_re_eval_ndcg_entities: ks[%d] = %d; every k is at least 1", i, (int)ks[i]); return GDMIX_RE_EINVAL; }
    for (int j = 0; j < i; ++j)
      if (ks[j] == ks[i]) { set_error("gdmix_re_eval_ndcg_entities: ks[%d] = ks[%d] = %d; the values of k are distinct", j, i, (int)ks[i]); return GDMIX_RE_EINVAL; }
  }
  if (N >= EVAL_LIMIT || E >= EVAL_LIMIT) {
    set_error("gdmix_re_eval_ndcg_entities: %lld samples / %lld entities; an evaluation takes fewer than 2^31 of each", (long long)N, (long long)E);
    return GDMIX_RE_ERANGE;
  }
  if (E == 0) return GDMIX_RE_OK;
  if (!ent_row_ptr || (N > 0 && (!score || !label))) { set_error("gdmix_re_eval_ndcg_entities: NULL input"); return GDMIX_RE_EINVAL; }
  const NdcgLayout L = ndcg_layout(E, N);
  if (!workspace || workspace_bytes < L.total) {
    set_error("gdmix_re_eval_ndcg_entities: workspace of %zu bytes, %zu needed (gdmix_re_eval_ndcg_workspace_bytes)", workspace_bytes, L.total);
    return GDMIX_RE_ENOMEM;
  }
  gdmix_ctx_impl* ci = &ctx->impl;
  hipStream_t s = static_cast<hipStream_t>(stream);
  char* base = static_cast<char*>(workspace);
  const int small_max = ci->eval_small_set ? ci->eval_small_max : 64;
  const NdcgOutDev O = {out->dcg, out->idcg, out->n, out->n_nan, out->n_bad_label};
  NdcgKs K;
  K.nk = nk; K.kmax = 0;
  for (int i = 0; i < NDCG_MAX; ++i) {
    K.k[i] = i < nk ? ks[i] : 0;
    if (K.k[i] > K.kmax) K.kmax = K.k[i];
  }
  // (with a limit of 0 this launch still writes the entities of no samples)
  hipLaunchKernelGGL(ndcg_small_kernel, dim3((unsigned)((E + 3) / 4)), dim3(64), 0, s, ent_row_ptr, E, score, label, O, K, small_max);
  HIP_TRY(hipGetLastError());
  int32_t* big_list = reinterpret_cast<int32_t*>(base + L.big_list);
  int32_t* big_off = reinterpret_cast<int32_t*>(base + L.big_off);
  int64_t nbig = 0, M = 0;
  int rc = eval_number_big(ci, "gdmix_re_eval_ndcg_entities", ent_row_ptr, E, N, small_max, reinterpret_cast<int64_t*>(base + L.mark),
                           reinterpret_cast<int64_t*>(base + L.offs), big_list, big_off, s, &nbig, &M);
  if (rc != GDMIX_RE_OK || nbig == 0) return rc;
  uint64_t* keys_a = reinterpret_cast<uint64_t*>(base + L.keys_a);
  uint64_t* keys_b = reinterpret_cast<uint64_t*>(base + L.keys_b);
  uint64_t* keys_c = reinterpret_cast<uint64_t*>(base + L.keys_c);
  uint32_t* vals_a = reinterpret_cast<uint32_t*>(base + L.vals_a);
  uint32_t* vals_b = reinterpret_cast<uint32_t*>(base + L.vals_b);
  double* dcg_terms = reinterpret_cast<double*>(base + L.dcg_terms);
  double* idcg_terms = reinterpret_cast<double*>(base + L.idcg_terms);
  NState* partial = reinterpret_cast<NState*>(base + L.partial);
  hipLaunchKernelGGL(ndcg_keys_kernel, dim3((unsigned)((M + 255) / 256)), dim3(256), 0, s, ent_row_ptr, (const int32_t*)big_list, (const int32_t*)big_off,
                     (int)nbig, M, score, label, keys_a, vals_a, keys_c);
  HIP_TRY(hipGetLastError());
  unsigned sbits = 0;
  while (((int64_t)1 << sbits) < nbig) ++sbits;
  rc = ndcg_sort_pairs(ci, keys_a, keys_b, vals_a, vals_b, M, 32u + sbits, s);
  if (rc != GDMIX_RE_OK) return rc;
  rc = sort_keys(ci, keys_c, keys_a, M, 32u + sbits, s);      // (keys_a is free again: the sorted label keys)
  if (rc != GDMIX_RE_OK) return rc;
  const int nb = (int)ndcg_tiles(M);
  hipLaunchKernelGGL(ndcg_reduce_kernel, dim3(nb), dim3(NDCG_SCAN_THREADS), 0, s, (const uint64_t*)keys_b, (const uint32_t*)vals_b, M, (const int32_t*)big_off, K,
                     partial);
  hipLaunchKernelGGL(ndcg_scan_kernel, dim3(nb), dim3(NDCG_SCAN_THREADS), 0, s, (const uint64_t*)keys_b, (const uint32_t*)vals_b, M, (const int32_t*)big_off, K,
                     (const NState*)partial, dcg_terms);
  hipLaunchKernelGGL(ndcg_ideal_kernel, dim3((unsigned)((M + 255) / 256)), dim3(256), 0, s, (const uint64_t*)keys_a, M, (const int32_t*)big_off, K.kmax,
                     idcg_terms);
  HIP_TRY(hipGetLastError());
  hipLaunchKernelGGL(ndcg_big_finish_kernel, dim3((unsigned)nbig), dim3(EVAL_THREADS), 0, s, ent_row_ptr, (const int32_t*)big_list, (const int32_t*)big_off,
                     (const uint64_t*)keys_b, (const uint32_t*)vals_b, (const double*)dcg_terms, (const double*)idcg_terms, M, E, K, O);
  HIP_TRY(hipGetLastError());
  return GDMIX_RE_OK;
}

}  // extern "C"
