// re_cap.hip — the active-data cap of a random-effect stage on the device (include/gdmix_re.h, "active-data cap", ABI 25).
//
// A row-subsetting pass over a gdmix_re_raw_batch in front of gdmix_re_pack, of which no pack or solve kernel knows: an entity of more than
// K rows keeps the K rows smallest by (key(seed, uid), row), in their order, each with its weight times n_e / K; every other entity keeps
// all its rows as they are.
//
//   plan    (two fills)          keep = 1 and row_ne = 0 for every row: what holds for the rows of an entity that is not capped
//           cap_list_kernel      the capped entities (n_e > K), those of at most small_max rows in one list and the others in another, in
//                                any order: an entity's flags depend on its own rows alone; the largest n_e
//           cap_small_kernel     a wavefront per listed entity: the keys hashed once into LDS, row i kept iff #{j : (key_j, j) < (key_i, i)} < K
//           cap_large_kernel     a workgroup per listed entity: exact radix select of the K-th smallest key, most significant byte first, a
//                                256-bin LDS histogram per pass, the key re-hashed from the uid on every pass; then key < tau is kept, and
//                                key == tau in row order until K is reached, by an ordered count across the workgroup
//           cap_chunk_kernel     per chunk of DS_CHUNK rows the kept rows / their non-zeros
//           ds_chunk_scan_kernel, ds_row_scan_kernel   the scans down-sampling has (re_rowsubset.hpp)
//   apply   cap_rows_kernel      the row arrays and ent_row_ptr, by input row; the weight multiplier is the entity's: row_ne / K, or none
//           ds_nnz_kernel        the non-zeros, by output position (re_rowsubset.hpp)
// Both entity kernels write keep and row_ne (= n_e) for every row of their entity. Histograms, ranks and scans are integers: the flags do
// not depend on the launch geometry or on the order of the lists.
#include "re_rowsubset.hpp"
#include "re_device.hpp"

#include <algorithm>

namespace gdmix {

constexpr int CAP_THREADS = 256;
constexpr int CAP_WAVES = CAP_THREADS / 64;        // entities per workgroup and turn of cap_small_kernel
constexpr int CAP_SMALL_MAX = 1024;                // most rows of an entity that may rank by counting: its keys are 8 KB of LDS
// ... and where the paths part by default. Counting is n^2 / 64 dependent steps of ONE wavefront: measured on a C5-shaped batch
// (profiles/active_data.txt) it wins up to a hundred or two rows (8.2 ms against 12.7 ms for the whole pass at K = 10) and loses above
// 256 (6.3 ms against 3.9 ms at K = 100 with the limit at 1024).
constexpr int CAP_SMALL_DEFAULT = 128;
constexpr int CAP_BIG_THREADS = 1024;              // the one workgroup of a large entity: 16 wavefronts keep one CU's loads in flight
constexpr int CAP_BIG_WAVES = CAP_BIG_THREADS / 64;
constexpr int CAP_BIG_PER_THREAD = 4;              // consecutive rows per lane in the ordered pass
constexpr int CAP_BIG_TILE = CAP_BIG_THREADS * CAP_BIG_PER_THREAD;
constexpr int CAP_MAX_GRID = 2048;                 // the entity kernels walk their list with this many workgroups at most
enum { CAP_TOT_SMALL = 0, CAP_TOT_LARGE = 1, CAP_TOT_LARGEST = 2, CAP_TOT_WORDS = 8 };

__device__ __forceinline__ uint64_t cap_key(uint64_t seed_mixed, int64_t uid) { return ds_mix((uint64_t)uid ^ seed_mixed); }

// the rows of entity e, inside [0, N] whatever the pointers say
__device__ __forceinline__ void cap_rows_of(const int64_t* __restrict__ ent_row_ptr, int64_t e, int64_t N, int64_t* r0, int64_t* n) {
  int64_t a = ent_row_ptr[e], b = ent_row_ptr[e + 1];
  a = a < 0 ? 0 : (a > N ? N : a);
  b = b < 0 ? 0 : (b > N ? N : b);
  *r0 = a;
  *n = b > a ? b - a : 0;
}

// thread e < E: entity e into the list of its path when n_e > K; tot[LARGEST] = max n_e by one atomic per wavefront
__global__ __launch_bounds__(CAP_THREADS) void cap_list_kernel(int64_t E, int64_t N, const int64_t* __restrict__ ent_row_ptr, int64_t K, int small_max,
                                                               int32_t* __restrict__ list_small, int32_t* __restrict__ list_large,
                                                               unsigned long long* __restrict__ tot) {
  const int64_t e = (int64_t)blockIdx.x * CAP_THREADS + threadIdx.x;
  int64_t r0 = 0, n = 0;
  if (e < E) cap_rows_of(ent_row_ptr, e, N, &r0, &n);
  if (n > K) {
    if (n <= small_max) list_small[atomicAdd(&tot[CAP_TOT_SMALL], 1ull)] = (int32_t)e;
    else list_large[atomicAdd(&tot[CAP_TOT_LARGE], 1ull)] = (int32_t)e;
  }
  long long m = n;
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const long long o = __shfl_xor(m, off, 64);
    m = o > m ? o : m;
  }
  if ((threadIdx.x & 63) == 0 && m > 0) atomicMax(&tot[CAP_TOT_LARGEST], (unsigned long long)m);
}

// One wavefront per listed entity (K < n <= small_max <= CAP_SMALL_MAX). The keys are hashed once into the wavefront's LDS row; a lane then
// counts, for each of its rows, the rows in front of it in the order (key, row): every lane reads the same word at a time.
__global__ __launch_bounds__(CAP_THREADS) void cap_small_kernel(int64_t N, const int64_t* __restrict__ ent_row_ptr, const int64_t* __restrict__ uid,
                                                                uint64_t seed_mixed, int K, const int32_t* __restrict__ list,
                                                                const unsigned long long* __restrict__ tot, uint8_t* __restrict__ keep,
                                                                int32_t* __restrict__ row_ne) {
  __shared__ uint64_t wave_keys[CAP_WAVES][CAP_SMALL_MAX];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  uint64_t* __restrict__ keys = wave_keys[wave];
  const int64_t count = (int64_t)tot[CAP_TOT_SMALL];
  for (int64_t idx = (int64_t)blockIdx.x * CAP_WAVES + wave; idx < count; idx += (int64_t)gridDim.x * CAP_WAVES) {   // (uniform over the wavefront)
    int64_t r0, n64;
    cap_rows_of(ent_row_ptr, list[idx], N, &r0, &n64);
    if (n64 <= K || n64 > CAP_SMALL_MAX) continue;
    const int n = (int)n64;
    for (int i = lane; i < n; i += 64) keys[i] = cap_key(seed_mixed, uid[r0 + i]);
    wave_lds_fence();
    for (int i = lane; i < n; i += 64) {
      const uint64_t mine = keys[i];
      int ahead = 0;
      for (int t = 0; t < n; ++t) {
        const uint64_t other = keys[t];
        ahead += (other < mine || (other == mine && t < i)) ? 1 : 0;
      }
      keep[r0 + i] = ahead < K ? 1 : 0;
      row_ne[r0 + i] = n;
    }
    wave_lds_fence();   // the next entity's keys go into the same row
  }
}

// One workgroup per listed entity (n > K, any size). Radix select: `prefix` holds the bytes of the K-th smallest key found so far, above
// bit `shift`; a pass counts, among the rows whose key agrees with it there, the next byte into 256 bins, the first wavefront finds the bin
// that holds the `remaining`-th of them, and the select ends early when that bin is taken whole. The last pass keeps key < tau and, of the
// rows with key == tau (compared above `shift`), the first `remaining` in row order: a lane takes CAP_BIG_PER_THREAD consecutive rows, so
// row order is lane order, and the count in front of a lane is a scan over the wavefront plus the sums of the wavefronts in front of it.
__global__ __launch_bounds__(CAP_BIG_THREADS) void cap_large_kernel(int64_t N, const int64_t* __restrict__ ent_row_ptr, const int64_t* __restrict__ uid,
                                                                    uint64_t seed_mixed, int K, const int32_t* __restrict__ list,
                                                                    const unsigned long long* __restrict__ tot, uint8_t* __restrict__ keep,
                                                                    int32_t* __restrict__ row_ne) {
  __shared__ uint32_t hist[256];
  __shared__ uint32_t sel[3];   // the bin, the rows in the bins in front of it, the rows in it
  __shared__ uint32_t wave_tot[CAP_BIG_WAVES];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int64_t count = (int64_t)tot[CAP_TOT_LARGE];
  for (int64_t idx = blockIdx.x; idx < count; idx += gridDim.x) {   // (uniform over the workgroup)
    int64_t r0, n;
    cap_rows_of(ent_row_ptr, list[idx], N, &r0, &n);
    if (n <= K) continue;
    const int64_t* __restrict__ u = uid + r0;
    uint64_t prefix = 0;
    uint32_t remaining = (uint32_t)K;
    int shift = 64;
    for (int pass = 0; pass < 8; ++pass) {
      shift -= 8;
      if (tid < 256) hist[tid] = 0;
      __syncthreads();
      for (int64_t i = tid; i < n; i += CAP_BIG_THREADS) {
        const uint64_t key = cap_key(seed_mixed, u[i]);
        if (pass == 0 || (key >> (shift + 8)) == (prefix >> (shift + 8))) atomicAdd(&hist[(uint32_t)(key >> shift) & 255u], 1u);
      }
      __syncthreads();
      if (wave == 0) {   // lane l: bins 4 l .. 4 l + 3
        uint32_t c[4], s = 0;
#pragma unroll
        for (int q = 0; q < 4; ++q) { c[q] = hist[4 * lane + q]; s += c[q]; }
        uint32_t incl = s;
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
          const uint32_t o = __shfl_up(incl, off, 64);
          if (lane >= off) incl += o;
        }
        uint32_t before = incl - s;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          if (before < remaining && remaining <= before + c[q]) { sel[0] = (uint32_t)(4 * lane + q); sel[1] = before; sel[2] = c[q]; }
          before += c[q];
        }
      }
      __syncthreads();
      const uint32_t bin = sel[0], before = sel[1], in_bin = sel[2];
      prefix |= (uint64_t)bin << shift;
      remaining -= before;
      if (in_bin == remaining) break;   // every row of the bin is kept: the bytes below do not matter
      // (the bins hold n >= K rows in the first pass and in_bin >= remaining >= 1 afterwards, so exactly one lane writes sel in every pass;
      // it is written again only behind the next pass's two barriers, which every thread reaches after these reads)
    }
    const uint64_t tau = prefix >> shift;
    uint32_t admitted = 0;   // rows with key == tau in front of this tile
    for (int64_t base = 0; base < n; base += CAP_BIG_TILE) {
      const int64_t i0 = base + (int64_t)tid * CAP_BIG_PER_THREAD;
      bool below[CAP_BIG_PER_THREAD], tie[CAP_BIG_PER_THREAD];
      uint32_t mine = 0;
#pragma unroll
      for (int q = 0; q < CAP_BIG_PER_THREAD; ++q) {
        below[q] = tie[q] = false;
        if (i0 + q < n) {
          const uint64_t hi = cap_key(seed_mixed, u[i0 + q]) >> shift;
          below[q] = hi < tau;
          tie[q] = hi == tau;
          mine += tie[q] ? 1u : 0u;
        }
      }
      uint32_t incl = mine;
#pragma unroll
      for (int off = 1; off < 64; off <<= 1) {
        const uint32_t o = __shfl_up(incl, off, 64);
        if (lane >= off) incl += o;
      }
      if (lane == 63) wave_tot[wave] = incl;
      __syncthreads();
      uint32_t in_front = 0, in_tile = 0;
#pragma unroll
      for (int w = 0; w < CAP_BIG_WAVES; ++w) {
        const uint32_t t = wave_tot[w];
        in_front += w < wave ? t : 0u;
        in_tile += t;
      }
      __syncthreads();   // wave_tot is written again in the next tile
      uint32_t pos = admitted + in_front + incl - mine;
#pragma unroll
      for (int q = 0; q < CAP_BIG_PER_THREAD; ++q) {
        if (i0 + q < n) {
          keep[r0 + i0 + q] = (below[q] || (tie[q] && pos < remaining)) ? 1 : 0;
          row_ne[r0 + i0 + q] = (int32_t)n;
          pos += tie[q] ? 1u : 0u;
        }
      }
      admitted += in_tile;
    }
    __syncthreads();   // the next entity's first pass writes hist and sel
  }
}

// per chunk the number of kept rows and of their non-zeros
__global__ __launch_bounds__(DS_THREADS) void cap_chunk_kernel(int64_t N, const int64_t* __restrict__ row_nnz_ptr, const uint8_t* __restrict__ keep,
                                                               long long* __restrict__ chunk_rows, long long* __restrict__ chunk_nnz) {
  __shared__ long long part[2][DS_THREADS / 64];
  const int64_t base = (int64_t)blockIdx.x * DS_CHUNK;
  long long rows = 0, nnz = 0;
#pragma unroll
  for (int k = 0; k < DS_PER_THREAD; ++k) {
    const int64_t i = base + (int64_t)k * DS_THREADS + threadIdx.x;
    if (i < N && keep[i]) {
      rows += 1;
      nnz += row_nnz_ptr[i + 1] - row_nnz_ptr[i];
    }
  }
  rows = ds_wave_sum(rows); nnz = ds_wave_sum(nnz);
  if ((threadIdx.x & 63) == 0) { part[0][threadIdx.x >> 6] = rows; part[1][threadIdx.x >> 6] = nnz; }
  __syncthreads();
  if (threadIdx.x == 0) {
    chunk_rows[blockIdx.x] = part[0][0] + part[0][1] + part[0][2] + part[0][3];
    chunk_nnz[blockIdx.x] = part[1][0] + part[1][1] + part[1][2] + part[1][3];
  }
}

// thread i < N: row i, when kept, to its output slot; thread e <= E: ent_row_ptr. A caller whose (N_out, Z_out) are not the plan's
// totals gets nothing written (its arrays have another size). row_ne[i] is n_e for a row of a capped entity and 0 for any other.
__global__ __launch_bounds__(DS_THREADS) void cap_rows_kernel(int64_t E, int64_t N, const int64_t* __restrict__ ent_row_ptr, const float* __restrict__ y,
                                                              const float* __restrict__ offset, const float* __restrict__ weight, int64_t K,
                                                              const uint8_t* __restrict__ keep, const int32_t* __restrict__ row_ne,
                                                              const int32_t* __restrict__ row_scan, const int64_t* __restrict__ nnz_scan,
                                                              const unsigned long long* __restrict__ totals, int32_t* __restrict__ src_row,
                                                              int32_t* __restrict__ kept_rows, DsOut o) {
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
  const float w = weight ? weight[i] : 1.0f;
  const int32_t ne = row_ne[i];
  o.y[k] = y[i];
  o.offset[k] = offset[i];
  o.weight[k] = ne > 0 ? (float)(((double)w * (double)ne) / (double)K) : w;
  o.row_nnz_ptr[k] = nnz_scan[i];
  src_row[k] = (int32_t)i;
  if (kept_rows) kept_rows[k] = (int32_t)i;
}

struct CapLayout { DsLayout ds; size_t row_ne, list_small, list_large, tot, total; };

static CapLayout cap_layout(int64_t E, int64_t N) {
  CapLayout L;
  L.ds = ds_layout(N);
  size_t off = L.ds.total;
  auto take = [&](size_t bytes) { size_t o = off; off += (bytes + 255) & ~(size_t)255; return o; };
  L.row_ne = take((size_t)(N + 1) * 4);
  L.list_small = take((size_t)(E + 1) * 4);
  L.list_large = take((size_t)(E + 1) * 4);
  L.tot = take(CAP_TOT_WORDS * 8);
  L.total = off;
  return L;
}

static int cap_check(const char* who, const gdmix_re_ctx* ctx, const gdmix_re_raw_batch* raw, const gdmix_re_cap_opts* opts, const void* workspace,
                     size_t workspace_bytes) {
  if (!ctx || !raw || !opts || !workspace) { set_error("%s: NULL argument", who); return GDMIX_RE_EINVAL; }
  if (opts->upper_bound < 1) {
    set_error("%s: the upper bound must be at least 1, not %lld", who, (long long)opts->upper_bound);
    return GDMIX_RE_EINVAL;
  }
  if (raw->E < 0 || raw->N < 0 || raw->Z < 0) { set_error("%s: negative batch dimension", who); return GDMIX_RE_EINVAL; }
  if (raw->N >= ((int64_t)1 << 31) || raw->E >= ((int64_t)1 << 31)) {
    set_error("%s: %lld rows of %lld entities; a cap pass takes fewer than 2^31 of either", who, (long long)raw->N, (long long)raw->E);
    return GDMIX_RE_ERANGE;
  }
  if (!raw->ent_row_ptr || !raw->row_nnz_ptr || (raw->N > 0 && (!raw->y || !raw->offset)) || (raw->Z > 0 && (!raw->col_global || !raw->val))) {
    set_error("%s: the raw batch has NULL arrays", who);
    return GDMIX_RE_EINVAL;
  }
  const size_t need = cap_layout(raw->E, raw->N).total;
  if (workspace_bytes < need) { set_error("%s: workspace too small: %zu < %zu", who, workspace_bytes, need); return GDMIX_RE_ENOMEM; }
  return GDMIX_RE_OK;
}

}  // namespace gdmix

using namespace gdmix;

extern "C" {

GDMIX_API size_t gdmix_re_cap_workspace_bytes(int64_t E, int64_t N) {
  if (E < 0 || N < 0 || N >= ((int64_t)1 << 31) || E >= ((int64_t)1 << 31)) return 0;
  return cap_layout(E, N).total;
}

GDMIX_API int gdmix_re_set_cap_small_max(gdmix_re_ctx* ctx, int small_max) {
  if (!ctx || small_max < 0 || small_max > CAP_SMALL_MAX) { set_error("gdmix_re_set_cap_small_max: 0 .. %d", CAP_SMALL_MAX); return GDMIX_RE_EINVAL; }
  ctx->impl.cap_small_set = 1;
  ctx->impl.cap_small_max = small_max;
  return GDMIX_RE_OK;
}

GDMIX_API int gdmix_re_cap_plan(gdmix_re_ctx* ctx, const gdmix_re_raw_batch* raw, const int64_t* uid, const gdmix_re_cap_opts* opts, void* workspace,
                                size_t workspace_bytes, gdmix_re_cap_counts* counts, void* stream) {
  const int rc = cap_check("gdmix_re_cap_plan", ctx, raw, opts, workspace, workspace_bytes);
  if (rc != GDMIX_RE_OK) return rc;
  if (!counts || (raw->N > 0 && !uid)) { set_error("gdmix_re_cap_plan: NULL argument"); return GDMIX_RE_EINVAL; }
  const int64_t N = raw->N, E = raw->E, K = opts->upper_bound;
  const CapLayout L = cap_layout(E, N);
  gdmix_ctx_impl* ci = &ctx->impl;
  ci->cap_plan_ws = nullptr;
  HIP_TRY(hipSetDevice(ci->device));
  hipStream_t s = static_cast<hipStream_t>(stream);
  char* base = static_cast<char*>(workspace);
  uint8_t* keep = reinterpret_cast<uint8_t*>(base + L.ds.keep);
  int32_t* row_scan = reinterpret_cast<int32_t*>(base + L.ds.row_scan);
  int64_t* nnz_scan = reinterpret_cast<int64_t*>(base + L.ds.nnz_scan);
  long long* chunk_rows = reinterpret_cast<long long*>(base + L.ds.chunk_rows);
  long long* chunk_nnz = reinterpret_cast<long long*>(base + L.ds.chunk_nnz);
  unsigned long long* totals = reinterpret_cast<unsigned long long*>(base + L.ds.totals);
  int32_t* row_ne = reinterpret_cast<int32_t*>(base + L.row_ne);
  int32_t* list_small = reinterpret_cast<int32_t*>(base + L.list_small);
  int32_t* list_large = reinterpret_cast<int32_t*>(base + L.list_large);
  unsigned long long* tot = reinterpret_cast<unsigned long long*>(base + L.tot);
  const int small_max = ci->cap_small_set ? ci->cap_small_max : CAP_SMALL_DEFAULT;
  HIP_TRY(hipMemsetAsync(totals, 0, DS_TOT_WORDS * 8, s));
  HIP_TRY(hipMemsetAsync(tot, 0, CAP_TOT_WORDS * 8, s));
  HIP_TRY(hipMemsetAsync(row_scan, 0, 4, s));   // N == 0: the single entry of each scan
  HIP_TRY(hipMemsetAsync(nnz_scan, 0, 8, s));
  if (N > 0) {
    const int nb = (int)((N + DS_CHUNK - 1) / DS_CHUNK);
    HIP_TRY(hipMemsetAsync(keep, 1, (size_t)N, s));
    HIP_TRY(hipMemsetAsync(row_ne, 0, (size_t)N * 4, s));
    if (E > 0)
      hipLaunchKernelGGL(cap_list_kernel, dim3((unsigned)((E + CAP_THREADS - 1) / CAP_THREADS)), dim3(CAP_THREADS), 0, s, E, N, raw->ent_row_ptr, K, small_max,
                         list_small, list_large, tot);
    if (E > 0 && K < N) {   // (no entity has more than N rows: at K >= N both lists are empty)
      const int Ki = (int)K;
      const uint64_t seed_mixed = ds_mix(opts->seed);
      // an entity of a list has more than K rows, one of the second list more than small_max as well
      const int64_t most_small = small_max > K ? N / (K + 1) : 0;
      const int64_t most_large = N / ((small_max > K ? (int64_t)small_max : K) + 1);
      const int64_t g_small = std::min<int64_t>(std::min<int64_t>((most_small + CAP_WAVES - 1) / CAP_WAVES, (E + CAP_WAVES - 1) / CAP_WAVES), CAP_MAX_GRID);
      const int64_t g_large = std::min<int64_t>(std::min<int64_t>(most_large, E), CAP_MAX_GRID);
      if (g_small > 0)
        hipLaunchKernelGGL(cap_small_kernel, dim3((unsigned)g_small), dim3(CAP_THREADS), 0, s, N, raw->ent_row_ptr, uid, seed_mixed, Ki,
                           (const int32_t*)list_small, (const unsigned long long*)tot, keep, row_ne);
      if (g_large > 0)
        hipLaunchKernelGGL(cap_large_kernel, dim3((unsigned)g_large), dim3(CAP_BIG_THREADS), 0, s, N, raw->ent_row_ptr, uid, seed_mixed, Ki,
                           (const int32_t*)list_large, (const unsigned long long*)tot, keep, row_ne);
    }
    hipLaunchKernelGGL(cap_chunk_kernel, dim3(nb), dim3(DS_THREADS), 0, s, N, raw->row_nnz_ptr, (const uint8_t*)keep, chunk_rows, chunk_nnz);
    hipLaunchKernelGGL(ds_chunk_scan_kernel, dim3(1), dim3(1024), 0, s, chunk_rows, chunk_nnz, nb, totals);
    hipLaunchKernelGGL(ds_row_scan_kernel, dim3(nb), dim3(DS_THREADS), 0, s, N, raw->row_nnz_ptr, (const uint8_t*)keep, (const long long*)chunk_rows,
                       (const long long*)chunk_nnz, row_scan, nnz_scan);
    HIP_TRY(hipGetLastError());
  }
  unsigned long long host[DS_TOT_WORDS], host_cap[CAP_TOT_WORDS];
  HIP_TRY(hipMemcpyAsync(host, totals, sizeof(host), hipMemcpyDeviceToHost, s));
  HIP_TRY(hipMemcpyAsync(host_cap, tot, sizeof(host_cap), hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  counts->entities = E;
  counts->capped = (int64_t)(host_cap[CAP_TOT_SMALL] + host_cap[CAP_TOT_LARGE]);
  counts->rows = N;
  counts->kept = (int64_t)host[DS_TOT_ROWS];
  counts->kept_nnz = (int64_t)host[DS_TOT_NNZ];
  counts->largest = (int64_t)host_cap[CAP_TOT_LARGEST];
  if (counts->kept < 0 || counts->kept > N || counts->kept_nnz < 0 || counts->kept_nnz > raw->Z) {
    set_error("gdmix_re_cap_plan: the row pointers do not describe %lld non-zeros (kept %lld rows, %lld non-zeros)", (long long)raw->Z,
              (long long)counts->kept, (long long)counts->kept_nnz);
    return GDMIX_RE_EINVAL;
  }
  ci->cap_plan_ws = workspace;
  ci->cap_plan_rows = N;
  ci->cap_plan_entities = E;
  ci->cap_plan_bound = K;
  ci->cap_plan_kept = counts->kept;
  ci->cap_plan_nnz = counts->kept_nnz;
  return GDMIX_RE_OK;
}

GDMIX_API int gdmix_re_cap_apply(gdmix_re_ctx* ctx, const gdmix_re_raw_batch* raw, const gdmix_re_cap_opts* opts, void* workspace, size_t workspace_bytes,
                                 const gdmix_re_downsample_out* out, int32_t* kept_rows, void* stream) {
  const int rc = cap_check("gdmix_re_cap_apply", ctx, raw, opts, workspace, workspace_bytes);
  if (rc != GDMIX_RE_OK) return rc;
  if (!out || out->N < 0 || out->Z < 0 || out->N > raw->N || out->Z > raw->Z) { set_error("gdmix_re_cap_apply: bad output counts"); return GDMIX_RE_EINVAL; }
  if (!out->ent_row_ptr || !out->row_nnz_ptr || (out->N > 0 && (!out->y || !out->offset || !out->weight)) || (out->Z > 0 && (!out->col_global || !out->val))) {
    set_error("gdmix_re_cap_apply: the output has NULL arrays");
    return GDMIX_RE_EINVAL;
  }
  const int64_t N = raw->N, E = raw->E;
  const gdmix_ctx_impl* ci = &ctx->impl;
  // the context's last plan is the one this workspace holds (the kernels' own comparison with the totals in the workspace only keeps a
  // stale caller from writing past its arrays)
  if (ci->cap_plan_ws != workspace || ci->cap_plan_rows != N || ci->cap_plan_entities != E || ci->cap_plan_bound != opts->upper_bound) {
    set_error("gdmix_re_cap_apply: the workspace does not hold this context's last gdmix_re_cap_plan of %lld rows at bound %lld", (long long)N,
              (long long)opts->upper_bound);
    return GDMIX_RE_EINVAL;
  }
  if (ci->cap_plan_kept != out->N || ci->cap_plan_nnz != out->Z) {
    set_error("gdmix_re_cap_apply: the output is sized for %lld rows / %lld non-zeros, the plan kept %lld / %lld", (long long)out->N, (long long)out->Z,
              (long long)ci->cap_plan_kept, (long long)ci->cap_plan_nnz);
    return GDMIX_RE_EINVAL;
  }
  const CapLayout L = cap_layout(E, N);
  HIP_TRY(hipSetDevice(ci->device));
  hipStream_t s = static_cast<hipStream_t>(stream);
  char* base = static_cast<char*>(workspace);
  const uint8_t* keep = reinterpret_cast<const uint8_t*>(base + L.ds.keep);
  const int32_t* row_scan = reinterpret_cast<const int32_t*>(base + L.ds.row_scan);
  const int64_t* nnz_scan = reinterpret_cast<const int64_t*>(base + L.ds.nnz_scan);
  int32_t* src_row = reinterpret_cast<int32_t*>(base + L.ds.src_row);
  const unsigned long long* totals = reinterpret_cast<const unsigned long long*>(base + L.ds.totals);
  const int32_t* row_ne = reinterpret_cast<const int32_t*>(base + L.row_ne);
  DsOut o{out->N, out->Z, out->ent_row_ptr, out->row_nnz_ptr, out->col_global, out->val, out->y, out->offset, out->weight};
  const int64_t threads = (N > E + 1 ? N : E + 1);
  hipLaunchKernelGGL(cap_rows_kernel, dim3((unsigned)((threads + DS_THREADS - 1) / DS_THREADS)), dim3(DS_THREADS), 0, s, E, N, raw->ent_row_ptr, raw->y,
                     raw->offset, raw->weight, opts->upper_bound, keep, row_ne, row_scan, nnz_scan, totals, src_row, kept_rows, o);
  if (out->Z > 0) {
    const int64_t tiles = (out->Z + DS_TILE - 1) / DS_TILE;
    if (tiles > 0x7fffffffll) { set_error("gdmix_re_cap_apply: %lld non-zeros are more than one launch copies", (long long)out->Z); return GDMIX_RE_ERANGE; }
    const int wide = (((uintptr_t)out->col_global | (uintptr_t)out->val) & 15) == 0;
    const int wide_in = (((uintptr_t)raw->col_global | (uintptr_t)raw->val) & 15) == 0;
    hipLaunchKernelGGL(ds_nnz_kernel, dim3((unsigned)tiles), dim3(DS_THREADS), 0, s, out->N, out->Z, raw->row_nnz_ptr, raw->col_global, raw->val,
                       (const int32_t*)src_row, (const int64_t*)out->row_nnz_ptr, totals, out->col_global, out->val, wide, wide_in);
  }
  HIP_TRY(hipGetLastError());
  return GDMIX_RE_OK;
}

}  // extern "C"
