// re_downsample.hip — down-sampling of a raw entity-grouped batch on the device (include/gdmix_re.h, "down-sampling", ABI 21).
//
// A row-subsetting pass over a gdmix_re_raw_batch in front of gdmix_re_pack: no pack or solve kernel knows about it. A row's fate
// is a pure function of (seed, uid); kept rows keep their order.
//
//   plan    ds_flag_kernel       a keep flag per row, per chunk of DS_CHUNK rows the kept rows / their non-zeros, the stage's counts
//           ds_chunk_scan_kernel exclusive scan of the chunk sums by one workgroup, the totals
//           ds_row_scan_kernel   exclusive scans inside every chunk: kept rows (int32) and kept non-zeros (int64) in front of each row
//   apply   ds_rows_kernel       the row arrays (y, offset, weight, row_nnz_ptr, the source row) and ent_row_ptr, by input row
//           ds_nnz_kernel        the non-zeros (col_global, val), by OUTPUT position: the only pass that moves real bytes
// The scans are integer sums: the same bits whatever the launch geometry. The scans, the copy of the non-zeros and the workspace layout
// are shared with the active-data cap (re_cap.hip): re_rowsubset.hpp.
#include "re_rowsubset.hpp"

#include <math.h>

namespace gdmix {

// keep[i], and per chunk the number of kept rows and of their non-zeros; totals[POS] / totals[NEG_KEPT] by one atomic per workgroup
__global__ __launch_bounds__(DS_THREADS) void ds_flag_kernel(int64_t N, const int64_t* __restrict__ row_nnz_ptr, const int64_t* __restrict__ uid,
                                                             const float* __restrict__ y, uint64_t seed_mixed, uint64_t T, int negatives_only,
                                                             uint8_t* __restrict__ keep, long long* __restrict__ chunk_rows,
                                                             long long* __restrict__ chunk_nnz, unsigned long long* __restrict__ totals) {
  __shared__ long long part[4][DS_THREADS / 64];
  const int64_t base = (int64_t)blockIdx.x * DS_CHUNK;
  long long rows = 0, nnz = 0, pos = 0, neg_kept = 0;
#pragma unroll
  for (int k = 0; k < DS_PER_THREAD; ++k) {
    const int64_t i = base + (int64_t)k * DS_THREADS + threadIdx.x;
    if (i < N) {
      const uint64_t draw = ds_mix((uint64_t)uid[i] ^ seed_mixed) >> 32;
      const bool positive = y[i] > 0.5f;
      const bool kept = (negatives_only && positive) || draw < T;
      keep[i] = kept ? 1 : 0;
      pos += positive ? 1 : 0;
      if (kept) {
        rows += 1;
        nnz += row_nnz_ptr[i + 1] - row_nnz_ptr[i];
        neg_kept += positive ? 0 : 1;
      }
    }
  }
  rows = ds_wave_sum(rows); nnz = ds_wave_sum(nnz); pos = ds_wave_sum(pos); neg_kept = ds_wave_sum(neg_kept);
  if ((threadIdx.x & 63) == 0) {
    const int w = threadIdx.x >> 6;
    part[0][w] = rows; part[1][w] = nnz; part[2][w] = pos; part[3][w] = neg_kept;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    long long s[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) s[q] = part[q][0] + part[q][1] + part[q][2] + part[q][3];
    chunk_rows[blockIdx.x] = s[0];
    chunk_nnz[blockIdx.x] = s[1];
    if (s[2]) atomicAdd(&totals[DS_TOT_POS], (unsigned long long)s[2]);
    if (s[3]) atomicAdd(&totals[DS_TOT_NEG_KEPT], (unsigned long long)s[3]);
  }
}

// thread i < N: row i, when kept, to its output slot; thread e <= E: ent_row_ptr. A caller whose (N_out, Z_out) are not the plan's
// totals gets nothing written (its arrays have another size).
__global__ __launch_bounds__(DS_THREADS) void ds_rows_kernel(int64_t E, int64_t N, const int64_t* __restrict__ ent_row_ptr, const float* __restrict__ y,
                                                             const float* __restrict__ offset, const float* __restrict__ weight, double rate,
                                                             int negatives_only, const uint8_t* __restrict__ keep, const int32_t* __restrict__ row_scan,
                                                             const int64_t* __restrict__ nnz_scan, const unsigned long long* __restrict__ totals,
                                                             int32_t* __restrict__ src_row, int32_t* __restrict__ kept_rows, DsOut o) {
  if ((int64_t)totals[DS_TOT_ROWS] != o.N_out || (int64_t)totals[DS_TOT_NNZ] != o.Z_out) return;
  const int64_t i = (int64_t)blockIdx.x * DS_THREADS + threadIdx.x;
  if (i <= E) {
    int64_t r = ent_row_ptr[i];
    r = r < 0 ? 0 : (r > N ? N : r);
    o.ent_row_ptr[i] = row_scan[r];
  }
  if (i == 0) o.row_nnz_ptr[o.N_out] = o.Z_out;
  if (i >= N || !keep[i]) return;
  const int64_t k = row_scan[i];
  if (k >= o.N_out) return;
  const float yi = y[i];
  const float w = weight ? weight[i] : 1.0f;
  const bool subject = !(negatives_only && yi > 0.5f);
  o.y[k] = yi;
  o.offset[k] = offset[i];
  o.weight[k] = subject ? (float)((double)w / rate) : w;
  o.row_nnz_ptr[k] = nnz_scan[i];
  src_row[k] = (int32_t)i;
  if (kept_rows) kept_rows[k] = (int32_t)i;
}

static int ds_check(const char* who, const gdmix_re_ctx* ctx, const gdmix_re_raw_batch* raw, const gdmix_re_downsample_opts* opts,
                    const void* workspace, size_t workspace_bytes) {
  if (!ctx || !raw || !opts || !workspace) { set_error("%s: NULL argument", who); return GDMIX_RE_EINVAL; }
  if (!(opts->rate > 0.0 && opts->rate <= 1.0)) {   // (a NaN compares false)
    set_error("%s: the rate must lie in (0, 1], not %g", who, opts->rate);
    return GDMIX_RE_EINVAL;
  }
  if (raw->E < 0 || raw->N < 0 || raw->Z < 0) { set_error("%s: negative batch dimension", who); return GDMIX_RE_EINVAL; }
  if (raw->N >= ((int64_t)1 << 31)) {
    set_error("%s: %lld rows; a down-sampling pass takes fewer than 2^31", who, (long long)raw->N);
    return GDMIX_RE_ERANGE;
  }
  if (!raw->ent_row_ptr || !raw->row_nnz_ptr || (raw->N > 0 && (!raw->y || !raw->offset)) || (raw->Z > 0 && (!raw->col_global || !raw->val))) {
    set_error("%s: the raw batch has NULL arrays", who);
    return GDMIX_RE_EINVAL;
  }
  const size_t need = ds_layout(raw->N).total;
  if (workspace_bytes < need) { set_error("%s: workspace too small: %zu < %zu", who, workspace_bytes, need); return GDMIX_RE_ENOMEM; }
  return GDMIX_RE_OK;
}

}  // namespace gdmix

using namespace gdmix;

extern "C" {

GDMIX_API size_t gdmix_re_downsample_workspace_bytes(int64_t E, int64_t N) {
  if (E < 0 || N < 0 || N >= ((int64_t)1 << 31)) return 0;
  return ds_layout(N).total;
}

GDMIX_API int gdmix_re_downsample_plan(gdmix_re_ctx* ctx, const gdmix_re_raw_batch* raw, const int64_t* uid, const gdmix_re_downsample_opts* opts,
                                       void* workspace, size_t workspace_bytes, gdmix_re_downsample_counts* counts, void* stream) {
  const int rc = ds_check("gdmix_re_downsample_plan", ctx, raw, opts, workspace, workspace_bytes);
  if (rc != GDMIX_RE_OK) return rc;
  if (!counts || (raw->N > 0 && !uid)) { set_error("gdmix_re_downsample_plan: NULL argument"); return GDMIX_RE_EINVAL; }
  const int64_t N = raw->N;
  const DsLayout L = ds_layout(N);
  HIP_TRY(hipSetDevice(ctx->impl.device));
  hipStream_t s = static_cast<hipStream_t>(stream);
  char* base = static_cast<char*>(workspace);
  uint8_t* keep = reinterpret_cast<uint8_t*>(base + L.keep);
  int32_t* row_scan = reinterpret_cast<int32_t*>(base + L.row_scan);
  int64_t* nnz_scan = reinterpret_cast<int64_t*>(base + L.nnz_scan);
  long long* chunk_rows = reinterpret_cast<long long*>(base + L.chunk_rows);
  long long* chunk_nnz = reinterpret_cast<long long*>(base + L.chunk_nnz);
  unsigned long long* totals = reinterpret_cast<unsigned long long*>(base + L.totals);
  const uint64_t T = (uint64_t)(opts->rate * 4294967296.0);   // exact: a scaling by 2^32, then truncation
  HIP_TRY(hipMemsetAsync(totals, 0, DS_TOT_WORDS * 8, s));
  HIP_TRY(hipMemsetAsync(row_scan, 0, 4, s));   // N == 0: the single entry of each scan
  HIP_TRY(hipMemsetAsync(nnz_scan, 0, 8, s));
  if (N > 0) {
    const int nb = (int)((N + DS_CHUNK - 1) / DS_CHUNK);
    hipLaunchKernelGGL(ds_flag_kernel, dim3(nb), dim3(DS_THREADS), 0, s, N, raw->row_nnz_ptr, uid, raw->y, ds_mix(opts->seed), T,
                       opts->negatives_only ? 1 : 0, keep, chunk_rows, chunk_nnz, totals);
    hipLaunchKernelGGL(ds_chunk_scan_kernel, dim3(1), dim3(1024), 0, s, chunk_rows, chunk_nnz, nb, totals);
    hipLaunchKernelGGL(ds_row_scan_kernel, dim3(nb), dim3(DS_THREADS), 0, s, N, raw->row_nnz_ptr, (const uint8_t*)keep, (const long long*)chunk_rows,
                       (const long long*)chunk_nnz, row_scan, nnz_scan);
    HIP_TRY(hipGetLastError());
  }
  unsigned long long host[DS_TOT_WORDS];
  HIP_TRY(hipMemcpyAsync(host, totals, sizeof(host), hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  counts->rows = N;
  counts->kept = (int64_t)host[DS_TOT_ROWS];
  counts->kept_nnz = (int64_t)host[DS_TOT_NNZ];
  counts->positives = (int64_t)host[DS_TOT_POS];
  counts->negatives_kept = (int64_t)host[DS_TOT_NEG_KEPT];
  if (counts->kept < 0 || counts->kept > N || counts->kept_nnz < 0 || counts->kept_nnz > raw->Z) {
    set_error("gdmix_re_downsample_plan: the row pointers do not describe %lld non-zeros (kept %lld rows, %lld non-zeros)", (long long)raw->Z,
              (long long)counts->kept, (long long)counts->kept_nnz);
    return GDMIX_RE_EINVAL;
  }
  ctx->impl.ds_plan_ws = workspace;
  ctx->impl.ds_plan_rows = N;
  ctx->impl.ds_plan_kept = counts->kept;
  ctx->impl.ds_plan_nnz = counts->kept_nnz;
  return GDMIX_RE_OK;
}

GDMIX_API int gdmix_re_downsample_apply(gdmix_re_ctx* ctx, const gdmix_re_raw_batch* raw, const gdmix_re_downsample_opts* opts, void* workspace,
                                        size_t workspace_bytes, const gdmix_re_downsample_out* out, int32_t* kept_rows, void* stream) {
  const int rc = ds_check("gdmix_re_downsample_apply", ctx, raw, opts, workspace, workspace_bytes);
  if (rc != GDMIX_RE_OK) return rc;
  if (!out || out->N < 0 || out->Z < 0 || out->N > raw->N || out->Z > raw->Z) { set_error("gdmix_re_downsample_apply: bad output counts"); return GDMIX_RE_EINVAL; }
  if (!out->ent_row_ptr || !out->row_nnz_ptr || (out->N > 0 && (!out->y || !out->offset || !out->weight)) || (out->Z > 0 && (!out->col_global || !out->val))) {
    set_error("gdmix_re_downsample_apply: the output has NULL arrays");
    return GDMIX_RE_EINVAL;
  }
  const int64_t N = raw->N, E = raw->E;
  // the context's last plan is the one this workspace holds: counts that are not its totals are an error here (the kernels' own
  // comparison with the totals in the workspace only keeps a stale caller from writing past its arrays)
  if (ctx->impl.ds_plan_ws != workspace || ctx->impl.ds_plan_rows != N) {
    set_error("gdmix_re_downsample_apply: the workspace does not hold this context's last gdmix_re_downsample_plan of %lld rows", (long long)N);
    return GDMIX_RE_EINVAL;
  }
  if (ctx->impl.ds_plan_kept != out->N || ctx->impl.ds_plan_nnz != out->Z) {
    set_error("gdmix_re_downsample_apply: the output is sized for %lld rows / %lld non-zeros, the plan kept %lld / %lld", (long long)out->N,
              (long long)out->Z, (long long)ctx->impl.ds_plan_kept, (long long)ctx->impl.ds_plan_nnz);
    return GDMIX_RE_EINVAL;
  }
  const DsLayout L = ds_layout(N);
  HIP_TRY(hipSetDevice(ctx->impl.device));
  hipStream_t s = static_cast<hipStream_t>(stream);
  char* base = static_cast<char*>(workspace);
  const uint8_t* keep = reinterpret_cast<const uint8_t*>(base + L.keep);
  const int32_t* row_scan = reinterpret_cast<const int32_t*>(base + L.row_scan);
  const int64_t* nnz_scan = reinterpret_cast<const int64_t*>(base + L.nnz_scan);
  int32_t* src_row = reinterpret_cast<int32_t*>(base + L.src_row);
  const unsigned long long* totals = reinterpret_cast<const unsigned long long*>(base + L.totals);
  DsOut o{out->N, out->Z, out->ent_row_ptr, out->row_nnz_ptr, out->col_global, out->val, out->y, out->offset, out->weight};
  const int64_t threads = (N > E + 1 ? N : E + 1);
  hipLaunchKernelGGL(ds_rows_kernel, dim3((unsigned)((threads + DS_THREADS - 1) / DS_THREADS)), dim3(DS_THREADS), 0, s, E, N, raw->ent_row_ptr, raw->y,
                     raw->offset, raw->weight, opts->rate, opts->negatives_only ? 1 : 0, keep, row_scan, nnz_scan, totals, src_row, kept_rows, o);
  if (out->Z > 0) {
    const int64_t tiles = (out->Z + DS_TILE - 1) / DS_TILE;
    if (tiles > 0x7fffffffll) { set_error("gdmix_re_downsample_apply: %lld non-zeros are more than one launch copies", (long long)out->Z); return GDMIX_RE_ERANGE; }
    const int wide = (((uintptr_t)out->col_global | (uintptr_t)out->val) & 15) == 0;
    const int wide_in = (((uintptr_t)raw->col_global | (uintptr_t)raw->val) & 15) == 0;
    hipLaunchKernelGGL(ds_nnz_kernel, dim3((unsigned)tiles), dim3(DS_THREADS), 0, s, out->N, out->Z, raw->row_nnz_ptr, raw->col_global, raw->val,
                       (const int32_t*)src_row, (const int64_t*)out->row_nnz_ptr, totals, out->col_global, out->val, wide, wide_in);
  }
  HIP_TRY(hipGetLastError());
  return GDMIX_RE_OK;
}

}  // extern "C"
