// re_group.hip — a sample-major data set grouped by entity on the device, and per-row values moved between sample order and grouped
// order (include/gdmix_re.h, "(ABI 27) row grouping"). What the partition job does between two stages of the coordinate chain, for the
// coordinates of a descent that stay in HBM (gdmix_amd/descent.py).
//
//   group   group_keys_kernel     key = entity_index (E for a row that belongs to no entity: it sorts behind every entity), value = the row
//           rocPRIM               stable radix sort of the (key, row) pairs over the bits of E: the sorted rows land in out->row_of
//           group_mark_kernel     per sorted position: does an entity start here, how many non-zeros has the row; N' by the one valid
//                                 position whose successor is not valid
//           rocPRIM               exclusive prefix sums of both: the entity's slot, and out->row_nnz_ptr
//           group_finish_kernel   present and ent_row_ptr by the positions where an entity starts; E', Z'
//           (the counts come back: one synchronise)
//           ds_nnz_kernel         the non-zeros, by OUTPUT position (re_rowsubset.hpp): the only pass that moves real bytes
//   rows    rows_gather_kernel, rows_scatter_kernel, offsets_combine_kernel: a thread per row
// Keys, flags and sums are integers: the same bits on every run and for every launch geometry.
#include "re_rowsubset.hpp"

#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_scan.hpp>

namespace gdmix {

constexpr int GRP_THREADS = 256;
enum { GRP_TOT_ENT = 4, GRP_TOT_BAD = 5 };   // next to DS_TOT_ROWS / DS_TOT_NNZ, which ds_nnz_kernel compares its counts with

__global__ __launch_bounds__(GRP_THREADS) void group_keys_kernel(int64_t N, int64_t E, const int32_t* __restrict__ entity_index,
                                                                 uint32_t* __restrict__ keys, int32_t* __restrict__ rows) {
  const int64_t i = (int64_t)blockIdx.x * GRP_THREADS + threadIdx.x;
  if (i >= N) return;
  const int32_t e = entity_index[i];
  keys[i] = (e >= 0 && (int64_t)e < E) ? (uint32_t)e : (uint32_t)E;
  rows[i] = (int32_t)i;
}

// thread i <= N over the sorted pairs. head[i]: an entity's first row sits at i; len[i]: the non-zeros of the row at i (0 behind the
// grouped rows, and at i = N, where the sums end). A row whose pointers lie outside [0, Z] or decrease counts as bad and gets no non-zero.
__global__ __launch_bounds__(GRP_THREADS) void group_mark_kernel(int64_t N, int64_t Z, int64_t E, const uint32_t* __restrict__ keys,
                                                                 const int32_t* __restrict__ rows, const int64_t* __restrict__ row_nnz_ptr,
                                                                 int64_t* __restrict__ head, int64_t* __restrict__ len,
                                                                 unsigned long long* __restrict__ totals) {
  const int64_t i = (int64_t)blockIdx.x * GRP_THREADS + threadIdx.x;
  if (i > N) return;
  int64_t h = 0, l = 0;
  if (i < N) {
    const uint32_t key = keys[i];
    if ((int64_t)key < E) {
      h = (i == 0 || keys[i - 1] != key) ? 1 : 0;
      const int64_t r = rows[i];
      const int64_t a = row_nnz_ptr[r], b = row_nnz_ptr[r + 1];
      if (a >= 0 && a <= b && b <= Z) l = b - a;
      else atomicAdd(&totals[GRP_TOT_BAD], 1ull);
      if (i == N - 1 || (int64_t)keys[i + 1] >= E) totals[DS_TOT_ROWS] = (unsigned long long)(i + 1);   // (one thread at most: the keys are sorted)
    }
  }
  head[i] = h;
  len[i] = l;
}

// thread i <= N. slot = the exclusive sum of head: the entity's place among the present ones; out_row_nnz_ptr = that of len.
__global__ __launch_bounds__(GRP_THREADS) void group_finish_kernel(int64_t N, int64_t E, const uint32_t* __restrict__ keys, const int64_t* __restrict__ head,
                                                                   const int64_t* __restrict__ slot, const int64_t* __restrict__ out_row_nnz_ptr,
                                                                   int64_t cap_entities, int32_t* __restrict__ present, int64_t* __restrict__ ent_row_ptr,
                                                                   unsigned long long* __restrict__ totals) {
  const int64_t i = (int64_t)blockIdx.x * GRP_THREADS + threadIdx.x;
  if (i > N) return;
  if (i == N) {
    const int64_t n_ent = slot[N];
    totals[GRP_TOT_ENT] = (unsigned long long)n_ent;
    totals[DS_TOT_NNZ] = (unsigned long long)out_row_nnz_ptr[N];
    if (n_ent >= 0 && n_ent <= cap_entities) ent_row_ptr[n_ent] = (int64_t)totals[DS_TOT_ROWS];   // (written by the launch before this one)
    return;
  }
  if (head[i]) {
    const int64_t k = slot[i];
    if (k >= 0 && k < cap_entities) { present[k] = (int32_t)keys[i]; ent_row_ptr[k] = i; }
  }
}

__global__ __launch_bounds__(GRP_THREADS) void rows_gather_kernel(float* __restrict__ dst, int64_t n_dst, const float* __restrict__ src, int64_t n_src,
                                                                  const int32_t* __restrict__ row_of) {
  const int64_t i = (int64_t)blockIdx.x * GRP_THREADS + threadIdx.x;
  if (i >= n_dst) return;
  const int64_t r = row_of[i];
  dst[i] = (r >= 0 && r < n_src) ? src[r] : 0.0f;
}

__global__ __launch_bounds__(GRP_THREADS) void rows_scatter_kernel(float* __restrict__ dst, int64_t n_dst, const float* __restrict__ src, int64_t n_src,
                                                                   const int32_t* __restrict__ row_of) {
  const int64_t i = (int64_t)blockIdx.x * GRP_THREADS + threadIdx.x;
  if (i >= n_src) return;
  const int64_t r = row_of[i];
  if (r >= 0 && r < n_dst) dst[r] = src[i];
}

struct CombineParts { const float* p[GDMIX_RE_COMBINE_MAX]; };

// fp32 additions from left to right (the header states the order); the part left out has a NULL pointer here
__global__ __launch_bounds__(GRP_THREADS) void offsets_combine_kernel(float* __restrict__ dst, int64_t n_dst, const float* __restrict__ base, CombineParts parts,
                                                                      int K, const int32_t* __restrict__ row_of, int64_t n_src) {
  const int64_t i = (int64_t)blockIdx.x * GRP_THREADS + threadIdx.x;
  if (i >= n_dst) return;
  const int64_t r = row_of ? (int64_t)row_of[i] : i;
  float acc = 0.0f;
  if (r >= 0 && r < n_src) {
    if (base) acc = base[r];
#pragma unroll
    for (int k = 0; k < GDMIX_RE_COMBINE_MAX; ++k)
      if (k < K && parts.p[k]) acc = acc + parts.p[k][r];
  }
  dst[i] = acc;
}

struct GroupLayout { size_t keys_in, keys_out, rows_in, head, slot, len, totals, total; };

static GroupLayout group_layout(int64_t N) {
  GroupLayout L;
  size_t off = 0;
  auto take = [&](size_t bytes) { size_t o = off; off += (bytes + 255) & ~(size_t)255; return o; };
  L.keys_in = take((size_t)(N + 1) * 4);
  L.keys_out = take((size_t)(N + 1) * 4);
  L.rows_in = take((size_t)(N + 1) * 4);
  L.head = take((size_t)(N + 1) * 8);
  L.slot = take((size_t)(N + 1) * 8);
  L.len = take((size_t)(N + 1) * 8);
  L.totals = take(DS_TOT_WORDS * 8);
  L.total = off;
  return L;
}

static unsigned group_grid(int64_t threads) { return (unsigned)((threads + GRP_THREADS - 1) / GRP_THREADS); }

static int rows_check(const char* who, const gdmix_re_ctx* ctx, const void* dst, int64_t n_dst, const void* src, int64_t n_src) {
  if (!ctx) { set_error("%s: NULL context", who); return GDMIX_RE_EINVAL; }
  if (n_dst < 0 || n_src < 0 || n_dst >= ((int64_t)1 << 31) || n_src >= ((int64_t)1 << 31)) {
    set_error("%s: %lld and %lld rows; a row map is int32 and takes fewer than 2^31", who, (long long)n_dst, (long long)n_src);
    return GDMIX_RE_ERANGE;
  }
  if ((n_dst > 0 && !dst) || (n_src > 0 && !src)) { set_error("%s: NULL array", who); return GDMIX_RE_EINVAL; }
  return GDMIX_RE_OK;
}

}  // namespace gdmix

using namespace gdmix;

extern "C" {

GDMIX_API size_t gdmix_re_group_workspace_bytes(int64_t N, int64_t E) {
  if (N < 0 || E < 0 || N >= ((int64_t)1 << 31) || E >= ((int64_t)1 << 31)) return 0;
  return group_layout(N).total;
}

GDMIX_API int gdmix_re_group_rows(gdmix_re_ctx* ctx, int64_t N, int64_t Z, int64_t E, const int64_t* row_nnz_ptr, const int64_t* col_global, const float* val,
                                  const int32_t* entity_index, void* workspace, size_t workspace_bytes, const gdmix_re_group_out* out,
                                  gdmix_re_group_counts* counts, void* stream) {
  const char* who = "gdmix_re_group_rows";
  if (!ctx || !out || !counts || !workspace) { set_error("%s: NULL argument", who); return GDMIX_RE_EINVAL; }
  if (N < 0 || Z < 0 || E < 0) { set_error("%s: negative dimension", who); return GDMIX_RE_EINVAL; }
  if (N >= ((int64_t)1 << 31) || E >= ((int64_t)1 << 31)) {
    set_error("%s: %lld rows of %lld entities; grouping takes fewer than 2^31 of either", who, (long long)N, (long long)E);
    return GDMIX_RE_ERANGE;
  }
  if (!row_nnz_ptr || (N > 0 && !entity_index) || (Z > 0 && (!col_global || !val))) { set_error("%s: the input has NULL arrays", who); return GDMIX_RE_EINVAL; }
  if (!out->ent_row_ptr || !out->row_nnz_ptr || (N > 0 && !out->row_of) || (N > 0 && E > 0 && !out->present) || (Z > 0 && (!out->col_global || !out->val))) {
    set_error("%s: the output has NULL arrays", who);
    return GDMIX_RE_EINVAL;
  }
  const GroupLayout L = group_layout(N);
  if (workspace_bytes < L.total) { set_error("%s: workspace too small: %zu < %zu", who, workspace_bytes, L.total); return GDMIX_RE_ENOMEM; }
  gdmix_ctx_impl* ci = &ctx->impl;
  HIP_TRY(hipSetDevice(ci->device));
  hipStream_t s = static_cast<hipStream_t>(stream);
  char* base = static_cast<char*>(workspace);
  uint32_t* keys_in = reinterpret_cast<uint32_t*>(base + L.keys_in);
  uint32_t* keys_out = reinterpret_cast<uint32_t*>(base + L.keys_out);
  int32_t* rows_in = reinterpret_cast<int32_t*>(base + L.rows_in);
  int64_t* head = reinterpret_cast<int64_t*>(base + L.head);
  int64_t* slot = reinterpret_cast<int64_t*>(base + L.slot);
  int64_t* len = reinterpret_cast<int64_t*>(base + L.len);
  unsigned long long* totals = reinterpret_cast<unsigned long long*>(base + L.totals);
  const int64_t cap_entities = N < E ? N : E;
  HIP_TRY(hipMemsetAsync(totals, 0, DS_TOT_WORDS * 8, s));
  HIP_TRY(hipMemsetAsync(out->ent_row_ptr, 0, 8, s));   // N' == 0: the single entry of each pointer array
  HIP_TRY(hipMemsetAsync(out->row_nnz_ptr, 0, 8, s));
  if (N > 0) {
    unsigned end_bit = 1;
    while (end_bit < 32 && ((uint64_t)E >> end_bit) != 0) ++end_bit;   // the keys are 0 .. E
    size_t sort_bytes = 0, scan_bytes = 0;
    HIP_TRY((rocprim::radix_sort_pairs(nullptr, sort_bytes, (uint32_t*)nullptr, (uint32_t*)nullptr, (int32_t*)nullptr, (int32_t*)nullptr, (size_t)N, 0u, end_bit, s)));
    HIP_TRY((rocprim::exclusive_scan(nullptr, scan_bytes, (int64_t*)nullptr, (int64_t*)nullptr, (int64_t)0, (size_t)N + 1, rocprim::plus<int64_t>(), s)));
    size_t tmp_bytes = sort_bytes > scan_bytes ? sort_bytes : scan_bytes;   // (rocPRIM takes it by reference)
    void* tmp = nullptr;
    const int rc = eval_tmp(ci, tmp_bytes ? tmp_bytes : 1, s, &tmp);
    if (rc != GDMIX_RE_OK) return rc;
    hipLaunchKernelGGL(group_keys_kernel, dim3(group_grid(N)), dim3(GRP_THREADS), 0, s, N, E, entity_index, keys_in, rows_in);
    HIP_TRY((rocprim::radix_sort_pairs(tmp, tmp_bytes, keys_in, keys_out, rows_in, out->row_of, (size_t)N, 0u, end_bit, s)));
    hipLaunchKernelGGL(group_mark_kernel, dim3(group_grid(N + 1)), dim3(GRP_THREADS), 0, s, N, Z, E, (const uint32_t*)keys_out, (const int32_t*)out->row_of,
                       row_nnz_ptr, head, len, totals);
    HIP_TRY((rocprim::exclusive_scan(tmp, tmp_bytes, head, slot, (int64_t)0, (size_t)N + 1, rocprim::plus<int64_t>(), s)));
    HIP_TRY((rocprim::exclusive_scan(tmp, tmp_bytes, len, out->row_nnz_ptr, (int64_t)0, (size_t)N + 1, rocprim::plus<int64_t>(), s)));
    hipLaunchKernelGGL(group_finish_kernel, dim3(group_grid(N + 1)), dim3(GRP_THREADS), 0, s, N, E, (const uint32_t*)keys_out, (const int64_t*)head,
                       (const int64_t*)slot, (const int64_t*)out->row_nnz_ptr, cap_entities, out->present, out->ent_row_ptr, totals);
    HIP_TRY(hipGetLastError());
  }
  unsigned long long host[DS_TOT_WORDS];
  HIP_TRY(hipMemcpyAsync(host, totals, sizeof(host), hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  counts->rows = N;
  counts->grouped = (int64_t)host[DS_TOT_ROWS];
  counts->grouped_nnz = (int64_t)host[DS_TOT_NNZ];
  counts->entities = (int64_t)host[GRP_TOT_ENT];
  counts->left_out = N - counts->grouped;
  if (host[GRP_TOT_BAD] != 0 || counts->grouped < 0 || counts->grouped > N || counts->grouped_nnz < 0 || counts->grouped_nnz > Z ||
      counts->entities < 0 || counts->entities > cap_entities) {
    set_error("%s: the row pointers do not describe %lld non-zeros (%llu rows outside them; grouped %lld rows, %lld non-zeros, %lld entities)", who,
              (long long)Z, host[GRP_TOT_BAD], (long long)counts->grouped, (long long)counts->grouped_nnz, (long long)counts->entities);
    return GDMIX_RE_EINVAL;
  }
  if (counts->grouped_nnz > 0) {
    const int64_t tiles = (counts->grouped_nnz + DS_TILE - 1) / DS_TILE;
    if (tiles > 0x7fffffffll) { set_error("%s: %lld non-zeros are more than one launch copies", who, (long long)counts->grouped_nnz); return GDMIX_RE_ERANGE; }
    const int wide = (((uintptr_t)out->col_global | (uintptr_t)out->val) & 15) == 0;
    const int wide_in = (((uintptr_t)col_global | (uintptr_t)val) & 15) == 0;
    hipLaunchKernelGGL(ds_nnz_kernel, dim3((unsigned)tiles), dim3(DS_THREADS), 0, s, counts->grouped, counts->grouped_nnz, row_nnz_ptr, col_global, val,
                       (const int32_t*)out->row_of, (const int64_t*)out->row_nnz_ptr, (const unsigned long long*)totals, out->col_global, out->val, wide,
                       wide_in);
    HIP_TRY(hipGetLastError());
  }
  return GDMIX_RE_OK;
}

GDMIX_API int gdmix_re_rows_gather_f32(gdmix_re_ctx* ctx, float* dst, int64_t n_dst, const float* src, int64_t n_src, const int32_t* row_of, void* stream) {
  const int rc = rows_check("gdmix_re_rows_gather_f32", ctx, dst, n_dst, src, n_src);
  if (rc != GDMIX_RE_OK) return rc;
  if (n_dst == 0) return GDMIX_RE_OK;
  if (!row_of) { set_error("gdmix_re_rows_gather_f32: row_of is NULL"); return GDMIX_RE_EINVAL; }
  HIP_TRY(hipSetDevice(ctx->impl.device));
  hipLaunchKernelGGL(rows_gather_kernel, dim3(group_grid(n_dst)), dim3(GRP_THREADS), 0, static_cast<hipStream_t>(stream), dst, n_dst, src, n_src, row_of);
  HIP_TRY(hipGetLastError());
  return GDMIX_RE_OK;
}

GDMIX_API int gdmix_re_rows_scatter_f32(gdmix_re_ctx* ctx, float* dst, int64_t n_dst, const float* src, int64_t n_src, const int32_t* row_of, int keep_rest,
                                        void* stream) {
  const int rc = rows_check("gdmix_re_rows_scatter_f32", ctx, dst, n_dst, src, n_src);
  if (rc != GDMIX_RE_OK) return rc;
  if (n_dst == 0) return GDMIX_RE_OK;
  if (n_src > 0 && !row_of) { set_error("gdmix_re_rows_scatter_f32: row_of is NULL"); return GDMIX_RE_EINVAL; }
  HIP_TRY(hipSetDevice(ctx->impl.device));
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (!keep_rest) HIP_TRY(hipMemsetAsync(dst, 0, (size_t)n_dst * 4, s));
  if (n_src > 0) hipLaunchKernelGGL(rows_scatter_kernel, dim3(group_grid(n_src)), dim3(GRP_THREADS), 0, s, dst, n_dst, src, n_src, row_of);
  HIP_TRY(hipGetLastError());
  return GDMIX_RE_OK;
}

GDMIX_API int gdmix_re_offsets_combine(gdmix_re_ctx* ctx, float* dst, int64_t n_dst, const float* base, const float* const* parts, int K, int skip,
                                       const int32_t* row_of, int64_t n_src, void* stream) {
  const int rc = rows_check("gdmix_re_offsets_combine", ctx, dst, n_dst, dst, n_src);
  if (rc != GDMIX_RE_OK) return rc;
  if (K < 0 || K > GDMIX_RE_COMBINE_MAX || (K > 0 && !parts)) { set_error("gdmix_re_offsets_combine: 0 <= K <= %d parts", GDMIX_RE_COMBINE_MAX); return GDMIX_RE_EINVAL; }
  if (!row_of && n_dst > n_src) { set_error("gdmix_re_offsets_combine: without row_of the output has the source's rows"); return GDMIX_RE_EINVAL; }
  CombineParts cp;
  for (int k = 0; k < GDMIX_RE_COMBINE_MAX; ++k) cp.p[k] = nullptr;
  for (int k = 0; k < K; ++k) {
    if (k == skip) continue;
    if (!parts[k] && n_src > 0) { set_error("gdmix_re_offsets_combine: part %d is NULL", k); return GDMIX_RE_EINVAL; }
    cp.p[k] = parts[k];
  }
  if (n_dst == 0) return GDMIX_RE_OK;
  HIP_TRY(hipSetDevice(ctx->impl.device));
  hipLaunchKernelGGL(offsets_combine_kernel, dim3(group_grid(n_dst)), dim3(GRP_THREADS), 0, static_cast<hipStream_t>(stream), dst, n_dst, base, cp, K, row_of,
                     n_src);
  HIP_TRY(hipGetLastError());
  return GDMIX_RE_OK;
}

}  // extern "C"
