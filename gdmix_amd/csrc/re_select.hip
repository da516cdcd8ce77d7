// re_select.hip — per-entity feature selection by Pearson correlation on the device (include/gdmix_re.h, "feature selection", ABI 22).
//
// A column-subsetting pass between two packs: pack -> score and select on the packed CSC -> filter the raw non-zeros -> pack again.
// No pack or solve kernel knows about it; the second pack sees a raw batch that simply does not contain the dropped features.
//
//   plan    sel_entity_kernel     a wavefront per entity: Sy, Syy, k_e; a lane per column: Sx, Sxx, Sxy over the column's cells (fp64, sample
//                                 order, adjacent duplicates of a cell combined first), q, key = (float)q. Entities of at most small_max
//                                 features rank by counting across the lanes: #{key_j > key_i or (== and j < i)} < k_e; the others leave
//                                 their sort words (~key bits, local index)
//           rocPRIM               a segmented radix sort of the sort words of the larger entities (empty segments for the others)
//           sel_rank_big_kernel   position in the sorted segment < k_e
//           sel_row_count_kernel  kept non-zeros of every row (a wavefront per entity, a lane per row); rocPRIM exclusive scan: the output
//                                 row pointers and kept_nnz
//           sel_totals_kernel     the counts, by one workgroup (integer sums)
//   apply   sel_copy_kernel       the kept non-zeros of every row to their output positions
// One lane adds one column, one cell after another, and the label sums have a shape that depends on n alone: a key is a function of the
// entity's own data alone, whichever ranking path takes the entity and wherever it sits in the batch. The ranking compares keys and indices only, so both paths give the same mask.
#include "re_internal.hpp"
#include "re_device.hpp"

#include <math.h>

#include <rocprim/device/device_scan.hpp>
#include <rocprim/device/device_segmented_radix_sort.hpp>

namespace gdmix {

constexpr int SEL_THREADS = 256;
constexpr int SEL_SMALL_MAX = 1024;   // features of an entity that ranks by counting: up to 64 in registers, up to this many through LDS
enum { SEL_TOT_AFFECTED = 0, SEL_TOT_KEPT = 1, SEL_TOT_NNZ = 2, SEL_TOT_WORDS = 8 };

__host__ __device__ __forceinline__ int64_t sel_k(double R, int64_t n, int64_t d) {
  const double t = ceil(R * (double)n);
  return t >= (double)d ? d : (t > 0.0 ? (int64_t)t : 0);
}

constexpr int SEL_WAVES = SEL_THREADS / 64;   // entities per workgroup of the wavefront-per-entity kernels

__device__ __forceinline__ double sel_wave_sum(double v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;   // the same bits in every lane (an addition commutes)
}

// One wavefront per entity. Sy, Syy: 64 strided partial sums, then a butterfly (a shape that depends on n alone). A lane per column: Sx,
// Sxx, Sxy over the column's cells, one after another, q, the key. An entity of at most 64 features has all its keys in one register across
// the wavefront and ranks by counting against the other lanes; one of at most small_max (<= 1024) counts against its keys in LDS (4 KB per
// wavefront); a larger one leaves its sort words for the segmented sort and is an empty segment otherwise.
__global__ __launch_bounds__(SEL_THREADS) void sel_entity_kernel(int64_t E, const int64_t* __restrict__ ent_row_ptr, const int64_t* __restrict__ ent_nnz_ptr,
                                                                 const int64_t* __restrict__ ent_feat_ptr, const int32_t* __restrict__ col_ptr,
                                                                 const int32_t* __restrict__ csc_row, const float* __restrict__ csc_val,
                                                                 const float* __restrict__ y, double R, int small_max, float* __restrict__ keys,
                                                                 uint8_t* __restrict__ keep, int32_t* __restrict__ ent_k, uint32_t* __restrict__ seg_begin,
                                                                 uint32_t* __restrict__ seg_end, unsigned long long* __restrict__ sort_in) {
  __shared__ float wave_keys[SEL_WAVES][SEL_SMALL_MAX];
  const int64_t e = (int64_t)blockIdx.x * SEL_WAVES + (threadIdx.x >> 6);
  if (e >= E) return;   // (the whole wavefront; the kernel has no workgroup barrier)
  const int lane = threadIdx.x & 63;
  float* __restrict__ lds_keys = wave_keys[threadIdx.x >> 6];
  const int64_t r0 = ent_row_ptr[e], f0 = ent_feat_ptr[e], z0 = ent_nnz_ptr[e], z_end = ent_nnz_ptr[e + 1];
  const int64_t n = ent_row_ptr[e + 1] - r0, d = ent_feat_ptr[e + 1] - f0;
  double s = 0.0, ss = 0.0;
  for (int64_t i = lane; i < n; i += 64) {
    const double v = (double)y[r0 + i];
    s += v;
    ss += v * v;
  }
  const double Sy = sel_wave_sum(s), Syy = sel_wave_sum(ss);
  const int64_t k = sel_k(R, n, d);
  const bool big = d > small_max;
  if (lane == 0) {
    ent_k[e] = (int32_t)k;
    seg_begin[e] = (uint32_t)f0;
    seg_end[e] = (uint32_t)(big ? f0 + d : f0);
  }
  const double nd = (double)n;
  const double By = nd * Syy - Sy * Sy;
  const bool by_ok = By > 0x1p-30 * nd * Syy;
  const int32_t* cp = col_ptr + z0 + e;
  float key = 0.0f;
  for (int64_t j = lane; j < d; j += 64) {
    int64_t c = z0 + cp[j], c1 = z0 + cp[j + 1];
    c = c < z0 ? z0 : c;
    c1 = c1 > z_end ? z_end : c1;   // (a pack's offsets stay inside the entity; a batch that is not a pack's must not be read past it)
    double Sx = 0.0, Sxx = 0.0, Sxy = 0.0;
    while (c < c1) {
      const int32_t r = csc_row[c];
      double x = (double)csc_val[c];
      ++c;
      while (c < c1 && csc_row[c] == r) { x += (double)csc_val[c]; ++c; }   // duplicates of (sample, feature) lie next to each other
      const double yi = (r >= 0 && r < n) ? (double)y[r0 + r] : 0.0;
      Sx += x;
      Sxx += x * x;
      Sxy += x * yi;
    }
    const double A = nd * Sxy - Sx * Sy, Bx = nd * Sxx - Sx * Sx;
    double q = 0.0;
    if (by_ok && Bx > 0x1p-30 * nd * Sxx) q = A * A / Bx;
    key = (float)q;
    if (!(key >= 0.0f)) key = 0.0f;   // a NaN (infinite sums) ranks with the constant columns
    keys[f0 + j] = key;
    if (big) sort_in[f0 + j] = ((unsigned long long)(~__float_as_uint(key)) << 32) | (unsigned long long)(uint32_t)j;
    else if (d > 64) lds_keys[j] = key;
  }
  if (big || d <= 0) return;
  if (k >= d) {
    for (int64_t j = lane; j < d; j += 64) keep[f0 + j] = 1;
    return;
  }
  if (d <= 64) {   // lane j < d holds key j
    int ahead = 0;
    for (int t = 0; t < (int)d; ++t) {
      const float other = __shfl(key, t, 64);
      ahead += (other > key || (other == key && t < lane)) ? 1 : 0;
    }
    if (lane < d) keep[f0 + lane] = ahead < k ? 1 : 0;
    return;
  }
  // 64 < d <= small_max <= SEL_SMALL_MAX: the keys are in the wavefront's LDS row; every lane reads the same word at a time
  wave_lds_fence();
  for (int j = lane; j < (int)d; j += 64) {
    const float mine = lds_keys[j];
    int ahead = 0;
    for (int t = 0; t < (int)d; ++t) {
      const float other = lds_keys[t];
      ahead += (other > mine || (other == mine && t < j)) ? 1 : 0;
    }
    keep[f0 + j] = ahead < k ? 1 : 0;
  }
}

// an entity of the sort path: position t of its sorted segment holds the local index of the feature of rank t
__global__ __launch_bounds__(SEL_THREADS) void sel_rank_big_kernel(int64_t E, const int64_t* __restrict__ ent_feat_ptr, const int32_t* __restrict__ ent_k,
                                                                   const unsigned long long* __restrict__ sorted, int small_max,
                                                                   uint8_t* __restrict__ keep) {
  const int64_t e = (int64_t)blockIdx.x * SEL_WAVES + (threadIdx.x >> 6);
  if (e >= E) return;
  const int64_t f0 = ent_feat_ptr[e], d = ent_feat_ptr[e + 1] - f0;
  if (d <= small_max) return;
  const int64_t k = ent_k[e];
  for (int64_t t = threadIdx.x & 63; t < d; t += 64) {
    const int64_t local = (int64_t)(sorted[f0 + t] & 0xffffffffull);
    if (local < d) keep[f0 + local] = t < k ? 1 : 0;
  }
}

// kept non-zeros of every row, a lane per row of the wavefront's entity
__global__ __launch_bounds__(SEL_THREADS) void sel_row_count_kernel(int64_t E, int64_t D, const int64_t* __restrict__ ent_row_ptr,
                                                                    const int64_t* __restrict__ ent_nnz_ptr, const int64_t* __restrict__ ent_feat_ptr,
                                                                    const int32_t* __restrict__ row_ptr, const int32_t* __restrict__ csr_col,
                                                                    const uint8_t* __restrict__ keep, int32_t* __restrict__ row_ent,
                                                                    int64_t* __restrict__ cnt) {
  const int64_t e = (int64_t)blockIdx.x * SEL_WAVES + (threadIdx.x >> 6);
  if (e >= E) return;
  const int64_t r0 = ent_row_ptr[e], n = ent_row_ptr[e + 1] - r0, z0 = ent_nnz_ptr[e], z_end = ent_nnz_ptr[e + 1], f0 = ent_feat_ptr[e];
  const int32_t* rp = row_ptr + r0 + e;
  for (int64_t r = threadIdx.x & 63; r < n; r += 64) {
    int64_t kept = 0, z = z0 + rp[r], z1 = z0 + rp[r + 1];
    z = z < z0 ? z0 : z;
    z1 = z1 > z_end ? z_end : z1;
    for (; z < z1; ++z) {
      const int64_t f = f0 + csr_col[z];
      kept += (f >= 0 && f < D && keep[f]) ? 1 : 0;
    }
    row_ent[r0 + r] = (int32_t)e;
    cnt[r0 + r] = kept;
  }
}

__global__ __launch_bounds__(1024) void sel_totals_kernel(int64_t E, int64_t N, const int64_t* __restrict__ ent_feat_ptr, const int32_t* __restrict__ ent_k,
                                                          const int64_t* __restrict__ scan, unsigned long long* __restrict__ totals) {
  __shared__ unsigned long long sa[1024], sk[1024];
  unsigned long long a = 0, k = 0;
  for (int64_t e = threadIdx.x; e < E; e += 1024) {
    const int64_t d = ent_feat_ptr[e + 1] - ent_feat_ptr[e];
    k += (unsigned long long)ent_k[e];
    a += ent_k[e] < d ? 1 : 0;
  }
  sa[threadIdx.x] = a; sk[threadIdx.x] = k;
  __syncthreads();
  for (int off = 512; off > 0; off >>= 1) {
    if ((int)threadIdx.x < off) { sa[threadIdx.x] += sa[threadIdx.x + off]; sk[threadIdx.x] += sk[threadIdx.x + off]; }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    totals[SEL_TOT_AFFECTED] = sa[0];
    totals[SEL_TOT_KEPT] = sk[0];
    totals[SEL_TOT_NNZ] = (unsigned long long)scan[N];
  }
}

// row i: its kept non-zeros, in order, from output position scan[i] on. A caller whose Z_out is not the plan's total gets nothing written.
__global__ __launch_bounds__(SEL_THREADS) void sel_copy_kernel(int64_t N, int64_t D, int64_t Z_in, int64_t Z_out, const int64_t* __restrict__ in_row_nnz_ptr,
                                                               const int64_t* __restrict__ in_col, const float* __restrict__ in_val,
                                                               const int64_t* __restrict__ ent_feat_ptr, const int32_t* __restrict__ csr_col,
                                                               const uint8_t* __restrict__ keep, const int32_t* __restrict__ row_ent,
                                                               const int64_t* __restrict__ scan, int64_t* __restrict__ out_row_nnz_ptr,
                                                               int64_t* __restrict__ out_col, float* __restrict__ out_val) {
  if (scan[N] != Z_out) return;
  const int64_t i = (int64_t)blockIdx.x * SEL_THREADS + threadIdx.x;
  if (i > N) return;
  out_row_nnz_ptr[i] = scan[i];
  if (i == N) return;
  const int64_t f0 = ent_feat_ptr[row_ent[i]];
  int64_t o = scan[i];
  const int64_t o1 = scan[i + 1];
  int64_t z = in_row_nnz_ptr[i], z1 = in_row_nnz_ptr[i + 1];
  z = z < 0 ? 0 : z;
  z1 = z1 > Z_in ? Z_in : z1;
  for (; z < z1 && o < o1; ++z) {
    const int64_t f = f0 + csr_col[z];
    if (f >= 0 && f < D && keep[f]) {
      out_col[o] = in_col[z];
      out_val[o] = in_val[z];
      ++o;
    }
  }
}

struct SelLayout { size_t keep, keys, sort_in, sort_out, ent_k, seg_begin, seg_end, row_ent, cnt, scan, totals, total; };

static SelLayout sel_layout(int64_t E, int64_t N, int64_t Z) {
  SelLayout L;
  size_t off = 0;
  auto take = [&](size_t bytes) { size_t o = off; off += (bytes + 255) & ~(size_t)255; return o; };
  L.keep = take((size_t)Z + 1);
  L.keys = take((size_t)(Z + 1) * 4);
  L.sort_in = take((size_t)(Z + 1) * 8);
  L.sort_out = take((size_t)(Z + 1) * 8);
  L.ent_k = take((size_t)(E + 1) * 4);
  L.seg_begin = take((size_t)(E + 1) * 4);
  L.seg_end = take((size_t)(E + 1) * 4);
  L.row_ent = take((size_t)(N + 1) * 4);
  L.cnt = take((size_t)(N + 1) * 8);
  L.scan = take((size_t)(N + 1) * 8);
  L.totals = take(SEL_TOT_WORDS * 8);
  L.total = off;
  return L;
}

static bool sel_in_range(int64_t E, int64_t N, int64_t Z) {
  const int64_t lim = (int64_t)1 << 31;
  return E >= 0 && N >= 0 && Z >= 0 && E < lim && N < lim && Z < lim;
}

}  // namespace gdmix

using namespace gdmix;

extern "C" {

GDMIX_API size_t gdmix_re_select_workspace_bytes(int64_t E, int64_t N, int64_t Z) {
  if (!sel_in_range(E, N, Z)) return 0;
  return sel_layout(E, N, Z).total;
}

GDMIX_API int gdmix_re_set_select_small_max(gdmix_re_ctx* ctx, int small_max) {
  if (!ctx || small_max < 0 || small_max > SEL_SMALL_MAX) { set_error("gdmix_re_set_select_small_max: 0 .. %d", SEL_SMALL_MAX); return GDMIX_RE_EINVAL; }
  ctx->impl.sel_small_max = small_max;
  ctx->impl.sel_small_set = 1;
  return GDMIX_RE_OK;
}

GDMIX_API int gdmix_re_select_plan(gdmix_re_ctx* ctx, const gdmix_re_packed* packed, double R, void* workspace, size_t workspace_bytes, float* keys_out,
                                   uint8_t* keep_out, gdmix_re_select_counts* counts, void* stream) {
  if (!ctx || !packed || !workspace || !counts) { set_error("gdmix_re_select_plan: NULL argument"); return GDMIX_RE_EINVAL; }
  if (!(R > 0.0) || !isfinite(R)) { set_error("gdmix_re_select_plan: the ratio must be finite and above 0, not %g", R); return GDMIX_RE_EINVAL; }
  const int64_t E = packed->E, N = packed->N, Z = packed->Z, D = packed->D;
  if (E < 0 || N < 0 || Z < 0 || D < 0 || D > Z) { set_error("gdmix_re_select_plan: bad batch dimensions"); return GDMIX_RE_EINVAL; }
  if (!sel_in_range(E, N, Z)) {
    set_error("gdmix_re_select_plan: %lld entities, %lld samples, %lld non-zeros; a selection pass takes fewer than 2^31 of each", (long long)E, (long long)N,
              (long long)Z);
    return GDMIX_RE_ERANGE;
  }
  if (D > 0 && !keep_out) { set_error("gdmix_re_select_plan: NULL argument"); return GDMIX_RE_EINVAL; }
  if (!packed->ent_row_ptr || !packed->ent_nnz_ptr || !packed->ent_feat_ptr || (N > 0 && (!packed->row_ptr || !packed->y)) ||
      (Z > 0 && (!packed->csr_col || !packed->col_ptr || !packed->csc_row || !packed->csc_val))) {
    set_error("gdmix_re_select_plan: the packed batch has NULL arrays");
    return GDMIX_RE_EINVAL;
  }
  const SelLayout L = sel_layout(E, N, Z);
  if (workspace_bytes < L.total) { set_error("gdmix_re_select_plan: workspace too small: %zu < %zu", workspace_bytes, L.total); return GDMIX_RE_ENOMEM; }
  gdmix_ctx_impl* ci = &ctx->impl;
  ci->sel_plan_ws = nullptr;
  HIP_TRY(hipSetDevice(ci->device));
  hipStream_t s = static_cast<hipStream_t>(stream);
  char* base = static_cast<char*>(workspace);
  uint8_t* keep = reinterpret_cast<uint8_t*>(base + L.keep);
  float* keys = reinterpret_cast<float*>(base + L.keys);
  unsigned long long* sort_in = reinterpret_cast<unsigned long long*>(base + L.sort_in);
  unsigned long long* sort_out = reinterpret_cast<unsigned long long*>(base + L.sort_out);
  int32_t* ent_k = reinterpret_cast<int32_t*>(base + L.ent_k);
  uint32_t* seg_begin = reinterpret_cast<uint32_t*>(base + L.seg_begin);
  uint32_t* seg_end = reinterpret_cast<uint32_t*>(base + L.seg_end);
  int32_t* row_ent = reinterpret_cast<int32_t*>(base + L.row_ent);
  int64_t* cnt = reinterpret_cast<int64_t*>(base + L.cnt);
  int64_t* scan = reinterpret_cast<int64_t*>(base + L.scan);
  unsigned long long* totals = reinterpret_cast<unsigned long long*>(base + L.totals);
  const int small_max = ci->sel_small_set ? ci->sel_small_max : SEL_SMALL_MAX;
  HIP_TRY(hipMemsetAsync(totals, 0, SEL_TOT_WORDS * 8, s));
  HIP_TRY(hipMemsetAsync(keep, 0, (size_t)D + 1, s));
  auto waves = [](int64_t entities) { return dim3((unsigned)((entities + SEL_WAVES - 1) / SEL_WAVES)); };
  HIP_TRY(hipMemsetAsync(cnt, 0, (size_t)(N + 1) * 8, s));   // (rows that no entity owns, and entry N)
  HIP_TRY(hipMemsetAsync(row_ent, 0, (size_t)(N + 1) * 4, s));
  if (E > 0) {
    hipLaunchKernelGGL(sel_entity_kernel, waves(E), dim3(SEL_THREADS), 0, s, E, packed->ent_row_ptr, (const int64_t*)packed->ent_nnz_ptr,
                       (const int64_t*)packed->ent_feat_ptr, (const int32_t*)packed->col_ptr, (const int32_t*)packed->csc_row,
                       (const float*)packed->csc_val, packed->y, R, small_max, keys, keep, ent_k, seg_begin, seg_end, sort_in);
    HIP_TRY(hipGetLastError());
    // max_p bounds every d_e from above (host, since the pack): a batch without an entity above the limit skips the sort
    if (D > 0 && (packed->max_p <= 0 || packed->max_p > small_max)) {
      size_t bytes = 0;
      HIP_TRY((rocprim::segmented_radix_sort_keys(nullptr, bytes, sort_in, sort_out, (unsigned)D, (unsigned)E, seg_begin, seg_end, 0u, 64u, s)));
      void* tmp = nullptr;
      const int rc = eval_tmp(ci, bytes ? bytes : 1, s, &tmp);
      if (rc != GDMIX_RE_OK) return rc;
      HIP_TRY((rocprim::segmented_radix_sort_keys(tmp, bytes, sort_in, sort_out, (unsigned)D, (unsigned)E, seg_begin, seg_end, 0u, 64u, s)));
      hipLaunchKernelGGL(sel_rank_big_kernel, waves(E), dim3(SEL_THREADS), 0, s, E, (const int64_t*)packed->ent_feat_ptr, (const int32_t*)ent_k,
                         (const unsigned long long*)sort_out, small_max, keep);
      HIP_TRY(hipGetLastError());
    }
    hipLaunchKernelGGL(sel_row_count_kernel, waves(E), dim3(SEL_THREADS), 0, s, E, D, packed->ent_row_ptr, (const int64_t*)packed->ent_nnz_ptr,
                       (const int64_t*)packed->ent_feat_ptr, (const int32_t*)packed->row_ptr, (const int32_t*)packed->csr_col, (const uint8_t*)keep, row_ent,
                       cnt);
    HIP_TRY(hipGetLastError());
    size_t bytes = 0;
    HIP_TRY((rocprim::exclusive_scan(nullptr, bytes, (int64_t*)nullptr, (int64_t*)nullptr, (int64_t)0, (size_t)N + 1, rocprim::plus<int64_t>(), s)));
    void* tmp = nullptr;
    const int rc = eval_tmp(ci, bytes ? bytes : 1, s, &tmp);
    if (rc != GDMIX_RE_OK) return rc;
    HIP_TRY((rocprim::exclusive_scan(tmp, bytes, cnt, scan, (int64_t)0, (size_t)N + 1, rocprim::plus<int64_t>(), s)));
    hipLaunchKernelGGL(sel_totals_kernel, dim3(1), dim3(1024), 0, s, E, N, (const int64_t*)packed->ent_feat_ptr, (const int32_t*)ent_k, (const int64_t*)scan,
                       totals);
    HIP_TRY(hipGetLastError());
  } else {
    HIP_TRY(hipMemsetAsync(scan, 0, (size_t)(N + 1) * 8, s));
  }
  if (D > 0) {
    HIP_TRY(hipMemcpyAsync(keep_out, keep, (size_t)D, hipMemcpyDeviceToDevice, s));
    if (keys_out) HIP_TRY(hipMemcpyAsync(keys_out, keys, (size_t)D * 4, hipMemcpyDeviceToDevice, s));
  }
  unsigned long long host[SEL_TOT_WORDS];
  HIP_TRY(hipMemcpyAsync(host, totals, sizeof(host), hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  counts->entities = E;
  counts->affected = (int64_t)host[SEL_TOT_AFFECTED];
  counts->features = D;
  counts->kept = (int64_t)host[SEL_TOT_KEPT];
  counts->dropped = D - counts->kept;
  counts->kept_nnz = (int64_t)host[SEL_TOT_NNZ];
  if (counts->kept < 0 || counts->kept > D || counts->kept_nnz < 0 || counts->kept_nnz > Z) {
    set_error("gdmix_re_select_plan: the packed batch does not describe %lld features and %lld non-zeros (kept %lld, %lld)", (long long)D, (long long)Z,
              (long long)counts->kept, (long long)counts->kept_nnz);
    return GDMIX_RE_EINVAL;
  }
  ci->sel_plan_ws = workspace;
  ci->sel_plan_E = E; ci->sel_plan_N = N; ci->sel_plan_Z = Z; ci->sel_plan_D = D;
  ci->sel_plan_nnz = counts->kept_nnz;
  return GDMIX_RE_OK;
}

GDMIX_API int gdmix_re_select_apply(gdmix_re_ctx* ctx, const gdmix_re_raw_batch* raw, const gdmix_re_packed* packed, void* workspace,
                                    const gdmix_re_select_out* out, void* stream) {
  if (!ctx || !raw || !packed || !workspace || !out) { set_error("gdmix_re_select_apply: NULL argument"); return GDMIX_RE_EINVAL; }
  gdmix_ctx_impl* ci = &ctx->impl;
  const int64_t E = packed->E, N = packed->N, Z = packed->Z, D = packed->D;
  if (ci->sel_plan_ws != workspace || ci->sel_plan_E != E || ci->sel_plan_N != N || ci->sel_plan_Z != Z || ci->sel_plan_D != D) {
    set_error("gdmix_re_select_apply: the workspace does not hold this context's last gdmix_re_select_plan of this batch");
    return GDMIX_RE_EINVAL;
  }
  if (raw->E != E || raw->N != N || raw->Z != Z) { set_error("gdmix_re_select_apply: the raw batch is not the one that was packed"); return GDMIX_RE_EINVAL; }
  if (out->Z != ci->sel_plan_nnz) {
    set_error("gdmix_re_select_apply: the output is sized for %lld non-zeros, the plan kept %lld", (long long)out->Z, (long long)ci->sel_plan_nnz);
    return GDMIX_RE_EINVAL;
  }
  if (!raw->row_nnz_ptr || !out->row_nnz_ptr || (Z > 0 && (!raw->col_global || !raw->val)) || (out->Z > 0 && (!out->col_global || !out->val))) {
    set_error("gdmix_re_select_apply: NULL arrays");
    return GDMIX_RE_EINVAL;
  }
  const SelLayout L = sel_layout(E, N, Z);
  HIP_TRY(hipSetDevice(ci->device));
  hipStream_t s = static_cast<hipStream_t>(stream);
  char* base = static_cast<char*>(workspace);
  hipLaunchKernelGGL(sel_copy_kernel, dim3((unsigned)((N + 1 + SEL_THREADS - 1) / SEL_THREADS)), dim3(SEL_THREADS), 0, s, N, D, Z, out->Z, raw->row_nnz_ptr,
                     raw->col_global, raw->val, (const int64_t*)packed->ent_feat_ptr, (const int32_t*)packed->csr_col,
                     reinterpret_cast<const uint8_t*>(base + L.keep), reinterpret_cast<const int32_t*>(base + L.row_ent),
                     reinterpret_cast<const int64_t*>(base + L.scan), out->row_nnz_ptr, out->col_global, out->val);
  HIP_TRY(hipGetLastError());
  return GDMIX_RE_OK;
}

}  // extern "C"
