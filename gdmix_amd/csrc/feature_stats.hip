// feature_stats.hip — feature normalisation: the exact column statistics of a stage's training data (include/gdmix_re.h, "feature
// normalisation", states the definitions and the bounds). This unit adds symbols only: no kernel of another unit changes.
//
// Every accumulator is an integer (64-bit adds, a 32-bit unsigned max): integer addition commutes, so what comes out does not depend on
// the order of the entries, on how the data are cut into calls, on the launch geometry or on which of the two paths below ran.
//
//   stats_kernel<W, VEC, PASS, LDS>
//     W     bytes of a column id (8: int64, 4: int32, 2: uint16)
//     VEC   four consecutive entries per lane, one 16-byte load of `val` and one (W = 8: two) of `col`; the host checks the alignment.
//           Otherwise one entry per lane (a chunk that starts at an odd entry of a shard).
//     PASS  1: count += 1, max of the bit pattern of |x| (non-negative floats order as their bits do);
//           2: the four limb sums of rint(x 2^shift1) and rint(x^2 2^shift2).
//     LDS   the table of num_features x (PASS 1: 12, PASS 2: 32) bytes is private to the workgroup (dynamic LDS): LDS atomics inside the
//           grid-stride loop, then one global atomic per touched slot and workgroup. Otherwise global atomics per entry.
//   In both paths a wavefront whose live lanes all hold the same column (D = 1, an intercept-like column, sorted data) adds its terms
//   with shuffles first and issues one atomic per accumulator: 64 adds on one address serialise, in LDS and at the memory side alike.
//   The grid-stride loop is wavefront-uniform (every lane of a wavefront makes the same number of trips), so the shuffles are safe.
//   stats_expand_kernel: scale[P] in coefficient order from factor[num_features]: one lane per feature slot of the batch (its entity by
//   bisection of ent_feat_ptr), one lane per entity for the intercept slots (1.0).
#include <stdint.h>
#include <stdlib.h>
#include <math.h>

#include "re_internal.hpp"

namespace gdmix {

constexpr int STATS_THREADS = 512;
constexpr int STATS_LDS_MAX_FEATURES = 4096;      // the LDS path up to here (GDMIX_STATS_LDS_MAX_FEATURES overrides: a test hook)
constexpr int STATS_LDS_HARD_MAX = 5000;          // 5 000 x 32 B = 160 000 B of the CU's 160 KiB
constexpr int STATS_SLOT_BYTES_1 = 12, STATS_SLOT_BYTES_2 = 32;

template <int W> struct StatsCol;
template <> struct StatsCol<8> { typedef int64_t type; };
template <> struct StatsCol<4> { typedef int32_t type; };
template <> struct StatsCol<2> { typedef uint16_t type; };

template <int W>
__device__ __forceinline__ void stats_load4(const void* __restrict__ col, int64_t q, int64_t c[4]) {
  if (W == 8) {
    const longlong2* p = reinterpret_cast<const longlong2*>(col) + 2 * q;
    const longlong2 a = p[0], b = p[1];
    c[0] = a.x; c[1] = a.y; c[2] = b.x; c[3] = b.y;
  } else if (W == 4) {
    const int4 a = reinterpret_cast<const int4*>(col)[q];
    c[0] = a.x; c[1] = a.y; c[2] = a.z; c[3] = a.w;
  } else {
    const ushort4 a = reinterpret_cast<const ushort4*>(col)[q];
    c[0] = a.x; c[1] = a.y; c[2] = a.z; c[3] = a.w;
  }
}

__device__ __forceinline__ long long stats_wave_sum(long long v) {
#pragma unroll
  for (int o = WAVE / 2; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}
__device__ __forceinline__ unsigned stats_wave_max(unsigned v) {
#pragma unroll
  for (int o = WAVE / 2; o > 0; o >>= 1) { const unsigned w = __shfl_xor(v, o); v = w > v ? w : v; }
  return v;
}

struct StatsArgs {
  const void* col;
  const float* val;
  int64_t Z, D;
  // pass 1
  unsigned long long* count;
  unsigned* max_bits;
  // pass 2
  const int32_t* limb_bits;
  const int32_t* shift1;
  const int32_t* shift2;
  unsigned long long* limbs;
  unsigned long long* bad;
};

// one entry per lane, every lane of the wavefront present (live: the entry exists). `tab64` / `tab32`: the accumulators (LDS or global).
template <int PASS>
__device__ __forceinline__ void stats_entry(const StatsArgs& A, bool live, int64_t idx, int64_t c, float x, unsigned long long* tab64, unsigned* tab32,
                                            int lane) {
  const unsigned bits = __float_as_uint(x) & 0x7fffffffu;
  bool ok = live && c >= 0 && c < A.D && bits < 0x7f800000u;
  long long t1 = 0, t2 = 0;
  int L = 0;
  if (PASS == 2 && ok) {
    L = A.limb_bits[c];
    if (L == 0) {             // a dead feature has no accumulator: a zero adds nothing, anything else was not there in pass 1
      ok = bits == 0;
      live = live && !ok;     // (a zero on a dead feature is neither added nor bad)
      ok = false;
    } else {
      const int s1 = A.shift1[c], s2 = A.shift2[c];
      const double xd = (double)x;
      if (fabs(xd) < ldexp(1.0, 2 * L - s1)) {      // |x| < 2^(E + 1): both terms are below 2^(2 L) in magnitude
        t1 = (long long)rint(ldexp(xd, s1));
        t2 = (long long)rint(ldexp(xd * xd, s2));   // the square of a float is exact in fp64
      } else {
        ok = false;
      }
    }
  }
  if (live && !ok) {
    atomicAdd(&A.bad[0], 1ull);
    atomicMin(&A.bad[1], (unsigned long long)idx);
  }
  const unsigned long long mask = __ballot(ok);
  if (mask == 0) return;
  const int leader = __ffsll((long long)mask) - 1;
  const int64_t c0 = __shfl(c, leader);
  const bool uniform = __ballot(ok && c == c0) == mask;
  if (PASS == 1) {
    if (uniform) {
      const unsigned m = stats_wave_max(ok ? bits : 0u);
      if (lane == leader) {
        atomicAdd(&tab64[c0], (unsigned long long)__popcll(mask));
        atomicMax(&tab32[c0], m);
      }
    } else if (ok) {
      atomicAdd(&tab64[c], 1ull);
      atomicMax(&tab32[c], bits);
    }
  } else {
    const long long m = (1ll << L) - 1;
    long long h1 = t1 >> L, l1 = t1 & m, h2 = t2 >> L, l2 = t2 & m;      // (arithmetic shift: hi 2^L + lo = t for negative t too)
    if (uniform) {
      if (!ok) { h1 = 0; l1 = 0; h2 = 0; l2 = 0; }
      h1 = stats_wave_sum(h1); l1 = stats_wave_sum(l1); h2 = stats_wave_sum(h2); l2 = stats_wave_sum(l2);
      if (lane == leader) {
        unsigned long long* p = tab64 + 4 * c0;
        atomicAdd(p + 0, (unsigned long long)h1); atomicAdd(p + 1, (unsigned long long)l1);
        atomicAdd(p + 2, (unsigned long long)h2); atomicAdd(p + 3, (unsigned long long)l2);
      }
    } else if (ok) {
      unsigned long long* p = tab64 + 4 * c;
      atomicAdd(p + 0, (unsigned long long)h1); atomicAdd(p + 1, (unsigned long long)l1);
      atomicAdd(p + 2, (unsigned long long)h2); atomicAdd(p + 3, (unsigned long long)l2);
    }
  }
}

template <int W, bool VEC, int PASS, bool LDS>
__global__ __launch_bounds__(STATS_THREADS) void stats_kernel(StatsArgs A) {
  extern __shared__ unsigned long long stats_lds[];
  const int lane = threadIdx.x & (WAVE - 1);
  const int64_t n64 = (PASS == 1 ? 1 : 4) * A.D;            // 64-bit slots of the table
  unsigned long long* tab64 = LDS ? stats_lds : (PASS == 1 ? A.count : A.limbs);
  unsigned* tab32 = LDS ? reinterpret_cast<unsigned*>(stats_lds + n64) : A.max_bits;
  if (LDS) {
    for (int64_t s = threadIdx.x; s < n64; s += blockDim.x) stats_lds[s] = 0;
    if (PASS == 1)
      for (int64_t s = threadIdx.x; s < A.D; s += blockDim.x) tab32[s] = 0;
    __syncthreads();
  }
  const int64_t per = VEC ? 4 : 1;
  const int64_t nq = (A.Z + per - 1) / per;                  // lane-sized pieces of the call
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  typedef typename StatsCol<W>::type col_t;
  for (int64_t base = (int64_t)blockIdx.x * blockDim.x + threadIdx.x - lane; base < nq; base += stride) {
    const int64_t q = base + lane;
    if (VEC) {
      int64_t c[4] = {0, 0, 0, 0};
      float x[4] = {0.f, 0.f, 0.f, 0.f};
      const int64_t i0 = 4 * q;
      if (q < nq) {
        if (i0 + 4 <= A.Z) {
          stats_load4<W>(A.col, q, c);
          const float4 v = reinterpret_cast<const float4*>(A.val)[q];
          x[0] = v.x; x[1] = v.y; x[2] = v.z; x[3] = v.w;
        } else {
          for (int k = 0; k < 4; ++k)
            if (i0 + k < A.Z) { c[k] = (int64_t)static_cast<const col_t*>(A.col)[i0 + k]; x[k] = A.val[i0 + k]; }
        }
      }
#pragma unroll
      for (int k = 0; k < 4; ++k) stats_entry<PASS>(A, q < nq && i0 + k < A.Z, i0 + k, c[k], x[k], tab64, tab32, lane);
    } else {
      const bool live = q < nq;
      const int64_t c = live ? (int64_t)static_cast<const col_t*>(A.col)[q] : 0;
      const float x = live ? A.val[q] : 0.f;
      stats_entry<PASS>(A, live, q, c, x, tab64, tab32, lane);
    }
  }
  if (LDS) {
    __syncthreads();
    unsigned long long* out64 = PASS == 1 ? A.count : A.limbs;
    for (int64_t s = threadIdx.x; s < n64; s += blockDim.x) {
      const unsigned long long v = stats_lds[s];
      if (v) atomicAdd(&out64[s], v);
    }
    if (PASS == 1)
      for (int64_t s = threadIdx.x; s < A.D; s += blockDim.x) {
        const unsigned v = tab32[s];
        if (v) atomicMax(&A.max_bits[s], v);
      }
  }
}

__global__ __launch_bounds__(256) void stats_expand_kernel(int64_t E, int64_t D, int ic, const int64_t* __restrict__ ent_feat_ptr,
                                                           const int32_t* __restrict__ unique_global, int64_t num_features,
                                                           const double* __restrict__ factor, double* __restrict__ scale) {
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (ic && t < E) scale[ent_feat_ptr[t] + t] = 1.0;
  if (t >= D) return;
  int64_t lo = 0, hi = E - 1;            // the largest e with ent_feat_ptr[e] <= t: the entity that owns slot t (entities without features own none)
  while (lo < hi) {
    const int64_t mid = (lo + hi + 1) >> 1;
    if (ent_feat_ptr[mid] <= t) lo = mid; else hi = mid - 1;
  }
  const int64_t g = unique_global[t];
  scale[t + (ic ? lo + 1 : 0)] = (g >= 0 && g < num_features) ? factor[g] : 1.0;
}

static int stats_lds_max_features() {
  const char* e = getenv("GDMIX_STATS_LDS_MAX_FEATURES");
  long v = STATS_LDS_MAX_FEATURES;
  if (e && *e) v = strtol(e, nullptr, 10);
  if (v < 0) v = 0;
  if (v > STATS_LDS_HARD_MAX) v = STATS_LDS_HARD_MAX;
  return (int)v;
}

template <int W, bool VEC, int PASS, bool LDS>
static hipError_t stats_launch_one(const StatsArgs& A, int blocks, size_t lds_bytes, hipStream_t s) {
  if (LDS && lds_bytes > 64 * 1024) {
    static DynLdsOnce once;
    const hipError_t rc = once.set(reinterpret_cast<const void*>(&stats_kernel<W, VEC, PASS, LDS>), 160 * 1000);
    if (rc != hipSuccess) return rc;
  }
  hipLaunchKernelGGL((stats_kernel<W, VEC, PASS, LDS>), dim3((unsigned)blocks), dim3(STATS_THREADS), LDS ? lds_bytes : 0, s, A);
  return hipGetLastError();
}
template <int W, int PASS>
static hipError_t stats_launch_w(const StatsArgs& A, bool vec, bool lds, int blocks, size_t lds_bytes, hipStream_t s) {
  if (vec) return lds ? stats_launch_one<W, true, PASS, true>(A, blocks, lds_bytes, s) : stats_launch_one<W, true, PASS, false>(A, blocks, 0, s);
  return lds ? stats_launch_one<W, false, PASS, true>(A, blocks, lds_bytes, s) : stats_launch_one<W, false, PASS, false>(A, blocks, 0, s);
}

template <int PASS>
static int stats_run(gdmix_re_ctx* ctx, const char* what, StatsArgs A, int col_width, void* stream) {
  if (!ctx) { set_error("%s: NULL context", what); return GDMIX_RE_EINVAL; }
  if (A.Z < 0 || A.D < 0) { set_error("%s: negative Z or num_features", what); return GDMIX_RE_EINVAL; }
  if (col_width != 8 && col_width != 4 && col_width != 2) { set_error("%s: col_width %d (8: int64, 4: int32, 2: uint16)", what, col_width); return GDMIX_RE_EINVAL; }
  if (!A.bad) { set_error("%s: NULL bad", what); return GDMIX_RE_EINVAL; }
  if (A.Z == 0) return GDMIX_RE_OK;
  if (!A.col || !A.val) { set_error("%s: NULL col or val", what); return GDMIX_RE_EINVAL; }
  if (A.D > 0 && (PASS == 1 ? (!A.count || !A.max_bits) : (!A.limb_bits || !A.shift1 || !A.shift2 || !A.limbs))) {
    set_error("%s: NULL accumulator or shift array", what);
    return GDMIX_RE_EINVAL;
  }
  HIP_TRY(hipSetDevice(ctx->impl.device));
  const uintptr_t pc = reinterpret_cast<uintptr_t>(A.col), pv = reinterpret_cast<uintptr_t>(A.val);
  const bool vec = (pv & 15) == 0 && (pc & (uintptr_t)(col_width == 2 ? 7 : 15)) == 0;
  const bool lds = A.D > 0 && A.D <= stats_lds_max_features();
  const size_t lds_bytes = lds ? (size_t)A.D * (PASS == 1 ? STATS_SLOT_BYTES_1 : STATS_SLOT_BYTES_2) : 0;
  // workgroups: what the entries need, at most as many as stay resident (the LDS table bounds that: one flush per workgroup)
  const int cus = ctx->impl.num_cus > 0 ? ctx->impl.num_cus : 256;
  int per_cu = 4;
  if (lds) { const size_t fit = (size_t)160 * 1024 / (lds_bytes + 256); per_cu = fit < 1 ? 1 : (fit > 4 ? 4 : (int)fit); }
  const int64_t nq = vec ? (A.Z + 3) / 4 : A.Z;
  int64_t blocks = (nq + STATS_THREADS - 1) / STATS_THREADS;
  if (blocks > (int64_t)cus * per_cu) blocks = (int64_t)cus * per_cu;
  hipStream_t s = static_cast<hipStream_t>(stream);
  hipError_t rc;
  if (col_width == 8) rc = stats_launch_w<8, PASS>(A, vec, lds, (int)blocks, lds_bytes, s);
  else if (col_width == 4) rc = stats_launch_w<4, PASS>(A, vec, lds, (int)blocks, lds_bytes, s);
  else rc = stats_launch_w<2, PASS>(A, vec, lds, (int)blocks, lds_bytes, s);
  if (rc != hipSuccess) { set_error("%s: launch failed: %s", what, hipGetErrorString(rc)); return GDMIX_RE_EHIP; }
  return GDMIX_RE_OK;
}

}  // namespace gdmix

using namespace gdmix;

extern "C" {

GDMIX_API int gdmix_re_feature_extent(gdmix_re_ctx* ctx, const void* col, int col_width, const float* val, int64_t Z, int64_t num_features,
                                      uint64_t* count, uint32_t* max_abs_bits, int64_t* bad, void* stream) {
  StatsArgs A = {};
  A.col = col; A.val = val; A.Z = Z; A.D = num_features;
  A.count = reinterpret_cast<unsigned long long*>(count);
  A.max_bits = max_abs_bits;
  A.bad = reinterpret_cast<unsigned long long*>(bad);
  return stats_run<1>(ctx, "gdmix_re_feature_extent", A, col_width, stream);
}

GDMIX_API int gdmix_re_feature_moments(gdmix_re_ctx* ctx, const void* col, int col_width, const float* val, int64_t Z, int64_t num_features,
                                       const int32_t* limb_bits, const int32_t* shift1, const int32_t* shift2, int64_t* limbs, int64_t* bad,
                                       void* stream) {
  StatsArgs A = {};
  A.col = col; A.val = val; A.Z = Z; A.D = num_features;
  A.limb_bits = limb_bits; A.shift1 = shift1; A.shift2 = shift2;
  A.limbs = reinterpret_cast<unsigned long long*>(limbs);
  A.bad = reinterpret_cast<unsigned long long*>(bad);
  return stats_run<2>(ctx, "gdmix_re_feature_moments", A, col_width, stream);
}

GDMIX_API int gdmix_re_feature_scale_expand(gdmix_re_ctx* ctx, const gdmix_re_packed* packed, int has_intercept, const double* factor,
                                            int64_t num_features, double* scale, void* stream) {
  if (!ctx || !packed) { set_error("gdmix_re_feature_scale_expand: NULL argument"); return GDMIX_RE_EINVAL; }
  if (packed->E < 0 || packed->D < 0 || num_features < 0) { set_error("gdmix_re_feature_scale_expand: bad batch"); return GDMIX_RE_EINVAL; }
  const int64_t E = packed->E, D = packed->D;
  const int ic = has_intercept ? 1 : 0;
  const int64_t n = D > (ic ? E : 0) ? D : (ic ? E : 0);
  if (n == 0) return GDMIX_RE_OK;
  if (!scale || !packed->ent_feat_ptr || (D > 0 && (!factor || !packed->unique_global))) {
    set_error("gdmix_re_feature_scale_expand: NULL array");
    return GDMIX_RE_EINVAL;
  }
  if (D > 0 && E == 0) { set_error("gdmix_re_feature_scale_expand: feature slots without an entity"); return GDMIX_RE_EINVAL; }
  if ((n + 255) / 256 > 0x7fffffffLL) { set_error("gdmix_re_feature_scale_expand: too many coefficients"); return GDMIX_RE_ERANGE; }
  HIP_TRY(hipSetDevice(ctx->impl.device));
  hipStream_t s = static_cast<hipStream_t>(stream);
  HIP_TRY(join_unique(&ctx->impl, s));      // unique_global may still be written by a deferred compaction
  hipLaunchKernelGGL(stats_expand_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, E, D, ic, packed->ent_feat_ptr, packed->unique_global,
                     num_features, factor, scale);
  HIP_TRY(hipGetLastError());
  return GDMIX_RE_OK;
}

}  // extern "C"
