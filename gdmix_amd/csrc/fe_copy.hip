// fe_copy.hip — the passes' copies of the non-zeros (fe_internal.hpp: FeCopy), built once when a problem is created: the kernels,
// and the build as a list of steps (fe_build_copy; fe_build_column_copy with the frequent columns under their virtual numbers).
// The only unit of the fixed effect that carries rocPRIM's sort and scans.
#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_scan.hpp>

#include "fe_internal.hpp"

#include <algorithm>
#include <utility>
#include <vector>

namespace gdmix {

// From the packed shard's CSR (for the column pass) and CSC (for the row pass) arrays: segment of every entry (flag + scan),
// stable sort by block of the entry's index (rocPRIM radix sort on the block number alone, so the source order — the order of
// the gathered vector — survives inside a block), units = the blocks' runs cut every `chunk` entries.
__global__ void fe_flag_kernel(const int32_t* __restrict__ ptr, int nseg, int64_t z, int32_t* __restrict__ flag) {
  for (int s = blockIdx.x * blockDim.x + threadIdx.x + 1; s < nseg; s += gridDim.x * blockDim.x) {
    const int p = ptr[s];
    if (p < z) atomicAdd(&flag[p], 1);   // empty segments pile up on the next entry
  }
}

struct FeEnt { int32_t seg, idx; float val; };   // an entry on its way through the sort

// sort key: the block, refined by the window of gathered elements (fe_internal.hpp: FE_SPAN_BITS)
__global__ void fe_ent_kernel(const int32_t* __restrict__ seg, const int32_t* __restrict__ idx, const float* __restrict__ val, int64_t z,
                              int nwin, int wbits, uint32_t* __restrict__ skey, FeEnt* __restrict__ ent) {
  for (int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; k < z; k += (int64_t)gridDim.x * blockDim.x) {
    const int i = idx[k], sg = seg[k];
    skey[k] = (uint32_t)(i / FE_B) * (uint32_t)nwin + (uint32_t)(sg >> wbits);
    ent[k] = FeEnt{sg, i, val[k]};
  }
}

// widest unit: key of its last entry - key of its first (keys ascend inside a unit)
__global__ void fe_span_kernel(const FeEnt* __restrict__ ent, const int32_t* __restrict__ ustart, int nunit, int32_t* __restrict__ kbase,
                               int32_t* __restrict__ max_span) {
  for (int u = blockIdx.x * blockDim.x + threadIdx.x; u < nunit; u += gridDim.x * blockDim.x) {
    const int k0 = ustart[u], k1 = ustart[u + 1];
    const int first = k1 > k0 ? ent[k0].seg : 0;
    kbase[u] = first;
    if (k1 > k0) atomicMax(max_span, ent[k1 - 1].seg - first);
  }
}

// the copy in the form the pass reads; one workgroup per unit
template <bool PACKED>
__global__ __launch_bounds__(256) void fe_pack_kernel(const FeEnt* __restrict__ ent, const int32_t* __restrict__ ustart,
                                                      const int32_t* __restrict__ kbase, uint2* __restrict__ out, int32_t* __restrict__ ckey,
                                                      float* __restrict__ cval, uint16_t* __restrict__ cloc) {
  const int u = blockIdx.x;
  const int k0 = ustart[u], k1 = ustart[u + 1], kb = kbase[u];
  for (int k = k0 + threadIdx.x; k < k1; k += 256) {
    const FeEnt e = ent[k];
    const int l = e.idx % FE_B;
    if (PACKED) {
      out[k] = make_uint2(((uint32_t)(e.seg - kb) << FE_LOC_BITS) | (uint32_t)l, __float_as_uint(e.val));
    } else {
      ckey[k] = e.seg;
      cval[k] = e.val;
      cloc[k] = (uint16_t)l;
    }
  }
}

// ---- the 6-byte form of a unit's entries --------------------------------------------------------------------------------------
// fillers an entry needs in front of it so that every key delta fits FE_CDELTA_MAX: a gap g > 31 takes (g - 1) / 31 fillers of
// delta 31 (value 0, accumulator 0) and leaves a delta in [1, 31] for the entry itself
__device__ __forceinline__ int fe_fillers(int gap) { return gap > FE_CDELTA_MAX ? (gap - 1) / FE_CDELTA_MAX : 0; }

// entries of unit u in the 6-byte form, fillers included (one workgroup per unit)
__global__ __launch_bounds__(256) void fe_ccount_kernel(const FeEnt* __restrict__ ent, const int32_t* __restrict__ ustart, const int32_t* __restrict__ kbase,
                                                        int32_t* __restrict__ cnt) {
  __shared__ int red[256 / WAVE];
  const int u = blockIdx.x, k0 = ustart[u], k1 = ustart[u + 1], kb = kbase[u];
  int f = 0;
  for (int k = k0 + threadIdx.x; k < k1; k += 256) f += fe_fillers(ent[k].seg - (k > k0 ? ent[k - 1].seg : kb));
  for (int sh = 32; sh > 0; sh >>= 1) f += __shfl_down(f, sh);
  if ((threadIdx.x & (WAVE - 1)) == 0) red[threadIdx.x >> 6] = f;
  __syncthreads();
  if (threadIdx.x == 0) cnt[u] = (k1 - k0) + red[0] + red[1] + red[2] + red[3];
}

__device__ __forceinline__ void fe_cput(unsigned char* base, int pos, float val, unsigned word) {
  const int t = pos / FE_CTRIP, w = pos % FE_CTRIP, q = w / WAVE, l = w % WAVE;
  unsigned char* tp = base + (size_t)t * FE_CTRIP_BYTES;
  *reinterpret_cast<float*>(tp + (q >> 2) * 1024 + l * 16 + (q & 3) * 4) = val;
  *reinterpret_cast<uint16_t*>(tp + 2048 + l * 16 + q * 2) = (uint16_t)word;
}

// the units that take the form (cbase[u] >= 0), written into a zeroed buffer: what stays zero is padding (delta 0, value 0)
__global__ __launch_bounds__(256) void fe_cpack_kernel(const FeEnt* __restrict__ ent, const int32_t* __restrict__ ustart, const int32_t* __restrict__ kbase,
                                                       const int64_t* __restrict__ cbase, unsigned char* __restrict__ cdata) {
  __shared__ int wsum[256 / WAVE];
  __shared__ int carry;
  const int u = blockIdx.x;
  if (cbase[u] < 0) return;
  const int k0 = ustart[u], k1 = ustart[u + 1], kb = kbase[u];
  unsigned char* base = cdata + cbase[u];
  const int tid = threadIdx.x, lane = tid & (WAVE - 1), wv = tid >> 6;
  if (tid == 0) carry = 0;
  __syncthreads();
  for (int c0 = k0; c0 < k1; c0 += 256) {
    const int k = c0 + tid;
    int gap = 0, f = 0;
    FeEnt e{0, 0, 0.0f};
    if (k < k1) {
      e = ent[k];
      gap = e.seg - (k > k0 ? ent[k - 1].seg : kb);
      f = fe_fillers(gap);
    }
    // exclusive prefix of f over the 256 entries of this chunk
    int incl = f;
    for (int sh = 1; sh < WAVE; sh <<= 1) {
      const int up = __shfl_up(incl, sh);
      if (lane >= sh) incl += up;
    }
    if (lane == WAVE - 1) wsum[wv] = incl;
    __syncthreads();
    int before = carry;
    for (int w2 = 0; w2 < wv; ++w2) before += wsum[w2];
    const int total = wsum[0] + wsum[1] + wsum[2] + wsum[3];
    if (k < k1) {
      const int first = (k - k0) + before + (incl - f);      // position of this entry's first filler (or of the entry)
      for (int j = 0; j < f; ++j) fe_cput(base, first + j, 0.0f, (unsigned)FE_CDELTA_MAX << FE_LOC_BITS);
      fe_cput(base, first + f, e.val, ((unsigned)(gap - FE_CDELTA_MAX * f) << FE_LOC_BITS) | (unsigned)(e.idx % FE_B));
    }
    __syncthreads();
    if (tid == 0) carry += total;
    __syncthreads();
  }
}

// bp[b] = first sorted entry of a block >= b
__global__ void fe_block_kernel(const uint32_t* __restrict__ sorted, int64_t z, int nblock, int32_t* __restrict__ bp) {
  for (int b = blockIdx.x * blockDim.x + threadIdx.x; b <= nblock; b += gridDim.x * blockDim.x) {
    int64_t lo = 0, hi = z;
    while (lo < hi) {
      const int64_t mid = (lo + hi) >> 1;
      if (sorted[mid] < (uint32_t)b) lo = mid + 1; else hi = mid;
    }
    bp[b] = (int32_t)lo;
  }
}

// Entries per unit of a (block, window) with len entries. A unit is one wavefront; where a block has fewer than four entries
// per 128-byte line of the gathered vector, nearly every gather is a line of its own out of the far cache and the unit crawls
// at a few microseconds per trip of 512 entries: 62 500 entries = 0.3 ms, the length of the whole pass (the rare features' blocks
// of a Zipf shard). Such blocks get units an eighth as long (sparse_chunk; 0 = never).
__device__ __forceinline__ int fe_block_chunk(int len, int chunk, int sparse_chunk, int extent) {
  return (sparse_chunk > 0 && (int64_t)len * 4 < (int64_t)extent) ? sparse_chunk : chunk;
}

// units of (block, window) b; the first window of a block keeps one even when empty: the block's outputs are still due
__global__ void fe_chunks_kernel(const int32_t* __restrict__ bp, int nblock, int nwin, int chunk, int sparse_chunk, int extent,
                                 int32_t* __restrict__ nch) {
  for (int b = blockIdx.x * blockDim.x + threadIdx.x; b <= nblock; b += gridDim.x * blockDim.x) {
    const int len = b < nblock ? bp[b + 1] - bp[b] : 0;
    const int c = fe_block_chunk(len, chunk, sparse_chunk, extent);
    nch[b] = b < nblock ? (len == 0 ? (b % nwin == 0 ? 1 : 0) : (len + c - 1) / c) : 0;
  }
}

// ufirst: first unit per (block, window); out: the units' first entries and blocks, and first unit per block
__global__ void fe_units_kernel(const int32_t* __restrict__ bp, const int32_t* __restrict__ ufirst, int nblock, int nwin, int chunk,
                                int sparse_chunk, int extent, int64_t z, int32_t* __restrict__ ustart, int32_t* __restrict__ ublock,
                                int32_t* __restrict__ block_first) {
  for (int b = blockIdx.x * blockDim.x + threadIdx.x; b < nblock; b += gridDim.x * blockDim.x) {
    const int u0 = ufirst[b], u1 = ufirst[b + 1];
    const int c = fe_block_chunk(bp[b + 1] - bp[b], chunk, sparse_chunk, extent);
    for (int u = u0; u < u1; ++u) {
      ustart[u] = bp[b] + (u - u0) * c;
      ublock[u] = b / nwin;
    }
    if (b % nwin == 0) block_first[b / nwin] = u0;
    if (b == nblock - 1) { ustart[u1] = (int32_t)z; block_first[nblock / nwin] = u1; }
  }
}

// the column pass's source columns with the frequent ones replaced by their virtual columns; one thread per row
__global__ void fe_hot_remap_kernel(const int32_t* __restrict__ ptr, int n, const int32_t* __restrict__ col, const int32_t* __restrict__ hotmap,
                                    int vbase, int32_t* __restrict__ col2) {
  for (int row = blockIdx.x * blockDim.x + threadIdx.x; row < n; row += gridDim.x * blockDim.x) {
    const int k1 = ptr[row + 1];
    for (int k = ptr[row]; k < k1; ++k) {
      const int c = col[k];
      const int h = hotmap[c];
      // the replica by the entry's POSITION, not by its row (round 4): a wavefront's 128 entries in flight are consecutive in row
      // order and span only ~4 rows of a 32-non-zero shard, so row % 32 sent all entries of all frequent columns of an instruction to
      // four replica slots = four LDS bank pairs (replicas of different columns 256 B apart share banks): SQ_LDS_BANK_CONFLICT + 62 %
      // against a uniform shard (profiles/r04_fe_counters.txt). The position spreads them over all 32; still a fixed assignment, so a
      // replica's terms are added in row order and two fits give the same bits.
      col2[k] = h >= 0 ? vbase + h * FE_HOT_REP + (k % FE_HOT_REP) : c;
    }
  }
}

// ---- the host side: a build as a list of steps --------------------------------------------------------------------------------------
// A step returns the first error of its calls and launches nothing behind it; every launch is checked where it is made.
#define FE_TRY(expr) do { const hipError_t rc_ = (expr); if (rc_ != hipSuccess) return rc_; } while (0)
#define FE_LAUNCH(kernel, grid, s, ...) do { hipLaunchKernelGGL(kernel, dim3(grid), dim3(256), 0, s, __VA_ARGS__); FE_TRY(hipGetLastError()); } while (0)

static bool fe_alloc(DevBuf& buf, size_t bytes) {
  const hipError_t rc = buf.alloc(bytes);
  if (rc != hipSuccess) set_error("hipMalloc(%zu) failed: %s", bytes, hipGetErrorString(rc));
  return rc == hipSuccess;
}

// Entries per unit. Blocks stay whole (a row block then finishes its rows itself) when that still gives the device enough
// units; otherwise every block is cut so that there are about eight wavefronts per CU.
static int fe_chunk_len(int64_t z, int nblock, int num_cus, const FeHooks& hooks) {
  const int64_t target = (z + (int64_t)num_cus * 8 - 1) / ((int64_t)num_cus * 8);
  const int64_t avg = (z + nblock - 1) / nblock;
  int64_t c = (avg <= 2 * target) ? 2 * avg : target;
  if (c < 8192) c = 8192;
  if (hooks.chunk) c = *hooks.chunk;
  if (c > (1 << 28)) c = 1 << 28;
  return (int)c;
}

// the work area of a build (released when the copy stands) and the copy's own memory, as byte offsets
struct FeWorkLayout { size_t a, seg, key, ent, ent2, bp, nch, uf, span, lib, bytes; };
struct FeTableLayout { size_t uf, us, ub, kb, ord, ent, bytes; };
struct FePlan {
  int nblock, chunk, wbits, nwin, nbw, extent, sparse_chunk;
  unsigned bits;                              // of the sort key
  size_t zz, max_units;                       // entries (at least one); upper bound of the unit count
  size_t sort_tmp, scan_tmp, scan2_tmp;       // rocPRIM's temporary storage
  FeWorkLayout w;
  FeTableLayout t;
};

// step 1: the sizes of everything, and where it lies. Host arithmetic (rocPRIM is only asked for its sizes): nothing is launched.
static int fe_plan(hipStream_t s, int num_cus, const FeHooks& hooks, const FeSource& src, FePlan* out) {
  FePlan& P = *out;
  const int nseg = src.nseg;
  P.nblock = src.len > 0 ? (src.len + FE_B - 1) / FE_B : 1;
  P.chunk = fe_chunk_len(src.z, P.nblock, num_cus, hooks);
  P.zz = (size_t)(src.z > 0 ? src.z : 1);
  P.wbits = hooks.window_bits.value_or(FE_SPAN_BITS);
  P.nwin = ((nseg > 0 ? nseg - 1 : 0) >> P.wbits) + 1;   // windows of the gathered vector (fe_ent_kernel)
  if ((int64_t)P.nblock * P.nwin > 0x7fffff00ll) { set_error("shard too large for the pass tables"); return GDMIX_RE_ERANGE; }
  P.nbw = P.nblock * P.nwin;
  P.extent = nseg < (1 << P.wbits) ? (nseg > 0 ? nseg : 1) : (1 << P.wbits);   // gathered elements per window
  P.sparse_chunk = src.cut_sparse ? (P.chunk / 8 > 4096 ? P.chunk / 8 : (P.chunk < 4096 ? P.chunk : 4096)) : 0;
  P.bits = 1;
  while (P.bits < 32 && (1u << P.bits) < (unsigned)P.nbw) ++P.bits;
  P.sort_tmp = P.scan_tmp = P.scan2_tmp = 0;
  hipError_t rc = rocprim::radix_sort_pairs(nullptr, P.sort_tmp, (uint32_t*)nullptr, (uint32_t*)nullptr, (FeEnt*)nullptr, (FeEnt*)nullptr,
                                            P.zz, 0u, P.bits, s);
  if (rc == hipSuccess) rc = rocprim::inclusive_scan(nullptr, P.scan_tmp, (int32_t*)nullptr, (int32_t*)nullptr, P.zz, rocprim::plus<int32_t>(), s);
  if (rc == hipSuccess) rc = rocprim::exclusive_scan(nullptr, P.scan2_tmp, (int32_t*)nullptr, (int32_t*)nullptr, 0, (size_t)P.nbw + 1, rocprim::plus<int32_t>(), s);
  if (rc != hipSuccess) { set_error("rocPRIM sizing failed: %s", hipGetErrorString(rc)); return GDMIX_RE_EHIP; }
  const size_t lib = std::max(P.sort_tmp, std::max(P.scan_tmp, P.scan2_tmp));
  // a block of len entries has at most len / chunk + 1 units
  P.max_units = (size_t)P.nbw + (size_t)(src.z / (P.sparse_chunk > 0 ? P.sparse_chunk : P.chunk)) + 1;
  const size_t zz = P.zz, nbw1 = (size_t)P.nbw + 1, mu = P.max_units;
  Arena work, tab;
  P.w.a = work.take(zz * 4);      // the flags, later the sorted keys
  P.w.seg = work.take(zz * 4);
  P.w.key = work.take(zz * 4);
  P.w.ent = work.take(zz * sizeof(FeEnt));
  P.w.ent2 = work.take(zz * sizeof(FeEnt));
  P.w.bp = work.take(nbw1 * 4);
  P.w.nch = work.take(nbw1 * 4);
  P.w.uf = work.take(nbw1 * 4);      // first unit per (block, window)
  P.w.span = work.take(64);
  P.w.lib = work.take(lib);
  P.w.bytes = work.off;
  // the unit tables, then the entries: 8 B per entry packed, 4 + 4 + 2 otherwise
  P.t.uf = tab.take(((size_t)P.nblock + 1) * 4);
  P.t.us = tab.take((mu + 1) * 4);
  P.t.ub = tab.take(mu * 4);
  P.t.kb = tab.take(mu * 4);
  P.t.ord = tab.take((mu + FE_XCDS) * 4);
  P.t.ent = tab.take(zz * 10 + 512);
  P.t.bytes = tab.off;
  return GDMIX_RE_OK;
}

// which units take the 6-byte form (cbase >= 0: the unit's byte offset, with its trips), what that comes to
struct FeCompressChoice {
  std::vector<int64_t> cbase;
  std::vector<int32_t> ctrip;
  size_t total = 0;       // bytes of the units that take it
  int64_t plain = 0;      // entries of the units that do not
  int taken = 0;
};

// a build under way: what the steps hand each other. The host vectors that asynchronous copies read or write live here, so that
// they outlast a step that ends early.
struct FeBuild {
  hipStream_t s;
  int num_cus;
  const FeHooks& hooks;
  const FeSource& src;
  FePlan P;
  DevBuf work, tables, cdata;
  FeCopy out;
  int nunit = 0;
  int32_t max_span = 0;
  bool packed = false;
  std::vector<int32_t> ufirst_h, ustart_h, cnt_h;
  FeCompressChoice choice;
};

// step 2: segment of every entry (flag + scan), then the entries sorted by (block, window); ent2 / the keys in `a` hold the result
static hipError_t fe_sort_step(FeBuild& B) {
  const FePlan& P = B.P;
  const FeSource& S = B.src;
  int32_t *flag = B.work.as<int32_t>(P.w.a), *seg = B.work.as<int32_t>(P.w.seg);
  uint32_t *skey = B.work.as<uint32_t>(P.w.key), *skey2 = B.work.as<uint32_t>(P.w.a);
  FeEnt *ent = B.work.as<FeEnt>(P.w.ent), *ent2 = B.work.as<FeEnt>(P.w.ent2);
  FE_TRY(hipMemsetAsync(B.work.as<int32_t>(P.w.span), 0, 64, B.s));
  if (S.z <= 0) return hipSuccess;
  FE_TRY(hipMemsetAsync(flag, 0, P.zz * 4, B.s));
  FE_LAUNCH(fe_flag_kernel, grid_for(S.nseg, 256, 4096), B.s, S.ptr, S.nseg, S.z, flag);
  size_t lt = P.scan_tmp;
  FE_TRY(rocprim::inclusive_scan(B.work.as<char>(P.w.lib), lt, flag, seg, (size_t)S.z, rocprim::plus<int32_t>(), B.s));
  FE_LAUNCH(fe_ent_kernel, B.num_cus * 16, B.s, seg, S.idx, S.val, S.z, P.nwin, P.wbits, skey, ent);
  lt = P.sort_tmp;
  return rocprim::radix_sort_pairs(B.work.as<char>(P.w.lib), lt, skey, skey2, ent, ent2, (size_t)S.z, 0u, P.bits, B.s);
}

// step 3: the sorted entries cut into units; their count comes back with the block -> unit table, then the widest unit's span
static hipError_t fe_cut_step(FeBuild& B) {
  const FePlan& P = B.P;
  const int64_t z = B.src.z;
  int32_t *bp = B.work.as<int32_t>(P.w.bp), *nch = B.work.as<int32_t>(P.w.nch), *ufw = B.work.as<int32_t>(P.w.uf);
  int32_t *span = B.work.as<int32_t>(P.w.span);
  int32_t *ufirst = B.tables.as<int32_t>(P.t.uf), *ustart = B.tables.as<int32_t>(P.t.us), *ublock = B.tables.as<int32_t>(P.t.ub);
  const int gb = grid_for(P.nbw + 1, 256, 4096);
  FE_LAUNCH(fe_block_kernel, gb, B.s, B.work.as<uint32_t>(P.w.a), z, P.nbw, bp);
  FE_LAUNCH(fe_chunks_kernel, gb, B.s, bp, P.nbw, P.nwin, P.chunk, P.sparse_chunk, P.extent, nch);
  size_t lt = P.scan2_tmp;
  FE_TRY(rocprim::exclusive_scan(B.work.as<char>(P.w.lib), lt, nch, ufw, 0, (size_t)P.nbw + 1, rocprim::plus<int32_t>(), B.s));
  FE_LAUNCH(fe_units_kernel, gb, B.s, bp, ufw, P.nbw, P.nwin, P.chunk, P.sparse_chunk, P.extent, z, ustart, ublock, ufirst);
  B.ufirst_h.resize((size_t)P.nblock + 1);
  FE_TRY(hipMemcpyAsync(B.ufirst_h.data(), ufirst, ((size_t)P.nblock + 1) * 4, hipMemcpyDeviceToHost, B.s));
  FE_TRY(hipStreamSynchronize(B.s));
  B.nunit = B.ufirst_h[(size_t)P.nblock];
  FE_LAUNCH(fe_span_kernel, grid_for(B.nunit, 256, 4096), B.s, B.work.as<FeEnt>(P.w.ent2), ustart, B.nunit, B.tables.as<int32_t>(P.t.kb), span);
  FE_TRY(hipMemcpyAsync(&B.max_span, span, 4, hipMemcpyDeviceToHost, B.s));
  return hipStreamSynchronize(B.s);
}

// Launch order. Workgroups go to the XCDs round robin and every XCD has its own L2: units that gather the same stretch of the
// vector should meet in one L2 rather than pull it over the fabric eight times (column pass on 4 M samples: 256 MB of
// residuals on top of 1 GB of entries). Units sorted by first gathered element, the sorted list cut into one run per XCD,
// run x dealt to the workgroups x, x + xcds, ...; -1 where a run is short.
static std::vector<int32_t> fe_xcd_order(const std::vector<int32_t>& kbase, int nunit, int xcds) {
  std::vector<int32_t> by((size_t)nunit);
  for (int u = 0; u < nunit; ++u) by[(size_t)u] = u;
  std::stable_sort(by.begin(), by.end(), [&](int32_t a, int32_t b) { return kbase[(size_t)a] < kbase[(size_t)b]; });
  const int per = (nunit + xcds - 1) / xcds;
  std::vector<int32_t> order((size_t)per * xcds, -1);
  for (int x = 0; x < xcds; ++x)
    for (int j = 0; j < per && x * per + j < nunit; ++j) order[(size_t)j * xcds + x] = by[(size_t)x * per + j];
  return order;
}

// step 4: the units dealt to the XCDs
static hipError_t fe_order_step(FeBuild& B) {
  std::vector<int32_t> kb((size_t)B.nunit);
  if (B.nunit) FE_TRY(hipMemcpy(kb.data(), B.tables.as<int32_t>(B.P.t.kb), (size_t)B.nunit * 4, hipMemcpyDeviceToHost));
  const std::vector<int32_t> order = fe_xcd_order(kb, B.nunit, FE_XCDS);
  if (!order.empty()) FE_TRY(hipMemcpy(B.tables.as<int32_t>(B.P.t.ord), order.data(), order.size() * 4, hipMemcpyHostToDevice));
  B.out.nlaunch = (int)order.size();
  return hipSuccess;
}

// step 5: the entries in the form the pass reads: one packed word and the value, or three arrays where a unit's keys span too much
static hipError_t fe_emit_step(FeBuild& B) {
  const FePlan& P = B.P;
  B.packed = GDMIX_FE_PACK && B.max_span < (1 << (32 - FE_LOC_BITS)) && B.hooks.pack.value_or(true);
  uint2* pent = B.tables.as<uint2>(P.t.ent);
  int32_t* ckey = B.tables.as<int32_t>(P.t.ent);
  float* cval = B.tables.as<float>(P.t.ent + up256(P.zz * 4));
  uint16_t* cloc = B.tables.as<uint16_t>(P.t.ent + 2 * up256(P.zz * 4));
  B.out.ent = B.packed ? pent : nullptr;
  B.out.key = ckey; B.out.val = cval; B.out.loc = cloc;
  B.out.stream_bytes = (int64_t)B.src.z * (B.packed ? 8 : 10);
  if (B.nunit <= 0 || B.src.z <= 0) return hipSuccess;
  const FeEnt* ent2 = B.work.as<FeEnt>(P.w.ent2);
  with_flag(B.packed, [&](auto PK) { hipLaunchKernelGGL((fe_pack_kernel<decltype(PK)::value>), dim3(B.nunit), dim3(256), 0, B.s, ent2, B.out.ustart, B.out.kbase, pent, ckey, cval, cloc); });
  FE_TRY(hipGetLastError());
  return hipStreamSynchronize(B.s);
}

// The form pays for a unit when it is shorter than 8 bytes per entry with room to spare (fillers of sparse blocks, padding of short
// units). ustart [nunit + 1]; cnt [nunit]: a unit's entries in the form, fillers included (fe_ccount_kernel).
static FeCompressChoice fe_choose_compressed(const std::vector<int32_t>& ustart, const std::vector<int32_t>& cnt) {
  const size_t nunit = cnt.size();
  FeCompressChoice c;
  c.cbase.assign(nunit, -1);
  c.ctrip.assign(nunit, 0);
  for (size_t u = 0; u < nunit; ++u) {
    const int64_t nu = (int64_t)ustart[u + 1] - ustart[u];
    const int64_t trips = ((int64_t)cnt[u] + FE_CTRIP - 1) / FE_CTRIP;
    if (nu > 0 && trips * FE_CTRIP_BYTES * 10 <= nu * 8 * 9) { c.cbase[u] = (int64_t)c.total; c.ctrip[u] = (int32_t)trips; c.total += (size_t)trips * FE_CTRIP_BYTES; ++c.taken; }
    else c.plain += nu;
  }
  return c;
}

// every unit's entry count in the 6-byte form, and the units' first entries, on the host
static hipError_t fe_count_compressed(FeBuild& B) {
  const size_t nunit = (size_t)B.nunit;
  DevBuf cnt;
  FE_TRY(cnt.alloc(nunit * 4));
  B.cnt_h.resize(nunit);
  B.ustart_h.resize(nunit + 1);
  FE_LAUNCH(fe_ccount_kernel, B.nunit, B.s, B.work.as<FeEnt>(B.P.w.ent2), B.out.ustart, B.out.kbase, cnt.as<int32_t>());
  FE_TRY(hipMemcpyAsync(B.cnt_h.data(), cnt.get(), nunit * 4, hipMemcpyDeviceToHost, B.s));
  FE_TRY(hipMemcpyAsync(B.ustart_h.data(), B.out.ustart, (nunit + 1) * 4, hipMemcpyDeviceToHost, B.s));
  return hipStreamSynchronize(B.s);
}

// step 6: the 6-byte form for the units it shortens (round 5), written into a zeroed buffer
static hipError_t fe_compress_step(FeBuild& B) {
  if (!B.src.compress || B.nunit <= 0 || B.src.z <= 0) return hipSuccess;
  FE_TRY(fe_count_compressed(B));
  B.choice = fe_choose_compressed(B.ustart_h, B.cnt_h);
  const FeCompressChoice& c = B.choice;
  if (c.taken == 0) return hipSuccess;
  const size_t nunit = (size_t)B.nunit;
  const size_t o_cb = 0, o_ct = up256(nunit * 8), o_data = o_ct + up256(nunit * 4);
  FE_TRY(B.cdata.alloc(o_data + c.total + 256));
  FE_TRY(hipMemsetAsync(B.cdata.as<char>(o_data), 0, c.total, B.s));
  FE_TRY(hipMemcpyAsync(B.cdata.as<char>(o_cb), c.cbase.data(), nunit * 8, hipMemcpyHostToDevice, B.s));
  FE_TRY(hipMemcpyAsync(B.cdata.as<char>(o_ct), c.ctrip.data(), nunit * 4, hipMemcpyHostToDevice, B.s));
  FE_LAUNCH(fe_cpack_kernel, B.nunit, B.s, B.work.as<FeEnt>(B.P.w.ent2), B.out.ustart, B.out.kbase, B.cdata.as<const int64_t>(o_cb),
            B.cdata.as<unsigned char>(o_data));
  FE_TRY(hipStreamSynchronize(B.s));      // the last reader of the work area
  B.out.stream_bytes = (int64_t)c.total + c.plain * (B.packed ? 8 : 10);
  B.out.cdata = B.cdata.as<const unsigned char>(o_data);
  B.out.cbase = B.cdata.as<const int64_t>(o_cb);
  B.out.ctrip = B.cdata.as<const int32_t>(o_ct);
  return hipSuccess;
}

int fe_build_copy(hipStream_t s, int num_cus, const FeHooks& hooks, const FeSource& src, FeCopy* out, DevBuf* tables, DevBuf* cdata,
                  std::vector<int32_t>* ufirst_host) {
  tables->reset();
  cdata->reset();
  FeBuild B{s, num_cus, hooks, src};
  const int rc = fe_plan(s, num_cus, hooks, src, &B.P);
  if (rc != GDMIX_RE_OK) return rc;
  const FePlan& P = B.P;
  if (!fe_alloc(B.work, P.w.bytes) || !fe_alloc(B.tables, P.t.bytes)) return GDMIX_RE_ENOMEM;
  B.out = FeCopy{};      // (part: the problem's pool, once the unit counts of both copies are known)
  B.out.ufirst = B.tables.as<int32_t>(P.t.uf); B.out.ustart = B.tables.as<int32_t>(P.t.us); B.out.ublock = B.tables.as<int32_t>(P.t.ub);
  B.out.kbase = B.tables.as<int32_t>(P.t.kb); B.out.order = B.tables.as<int32_t>(P.t.ord);
  B.out.nblock = P.nblock;
  hipError_t h = hipSuccess;
  for (auto step : {fe_sort_step, fe_cut_step, fe_order_step, fe_emit_step, fe_compress_step})
    if ((h = step(B)) != hipSuccess) break;
  if (h != hipSuccess) {
    (void)hipStreamSynchronize(s);      // what the steps before have enqueued still reads the work area and B's vectors
    set_error("building a pass's copy failed: %s", hipGetErrorString(h));
    return GDMIX_RE_EHIP;
  }
  // every reader of the work area has been waited for (fe_cut_step, fe_emit_step, fe_compress_step): it goes with B
  B.out.nunit = B.nunit;
  *out = B.out;
  *tables = std::move(B.tables);
  *cdata = std::move(B.cdata);
  if (ufirst_host) ufirst_host->swap(B.ufirst_h);
  return GDMIX_RE_OK;
}

// ---- the column pass's copy, frequent columns under their virtual numbers (fe_internal.hpp: FeHot) ----------------------------------
// the FE_HOT_MAX most frequent of the columns with at least hot_min entries, ascending; cp: the shard's column pointers [d + 1]
static std::vector<int32_t> fe_pick_hot(const std::vector<int32_t>& cp, int d, long hot_min) {
  std::vector<std::pair<int32_t, int32_t>> cand;   // (-count, column): most frequent first, ties by column
  for (int c = 0; c < d; ++c)
    if (cp[(size_t)c + 1] - cp[(size_t)c] >= hot_min) cand.emplace_back(-(cp[(size_t)c + 1] - cp[(size_t)c]), c);
  std::sort(cand.begin(), cand.end());
  if (cand.size() > (size_t)FE_HOT_MAX) cand.resize(FE_HOT_MAX);
  std::vector<int32_t> hot_cols;
  for (auto& q : cand) hot_cols.push_back(q.second);
  std::sort(hot_cols.begin(), hot_cols.end());
  return hot_cols;
}

// col2 = the shard's csr_col with the frequent columns replaced; hot_list = the frequent columns on the device
static hipError_t fe_hot_remap(hipStream_t s, int num_cus, const gdmix_re_packed* b, int n, const std::vector<int32_t>& hotmap,
                               const std::vector<int32_t>& hot_cols, int vbase, int32_t* hotmap_dev, int32_t* hot_list, int32_t* col2) {
  FE_TRY(hipMemcpyAsync(hotmap_dev, hotmap.data(), hotmap.size() * 4, hipMemcpyHostToDevice, s));
  FE_TRY(hipMemcpyAsync(hot_list, hot_cols.data(), hot_cols.size() * 4, hipMemcpyHostToDevice, s));
  FE_LAUNCH(fe_hot_remap_kernel, grid_for(n, 256, num_cus * 32), s, b->row_ptr, n, b->csr_col, hotmap_dev, vbase, col2);
  return hipStreamSynchronize(s);                      // (also: the host vectors are done with)
}

// Entry counts per column come from the packed shard's column pointers (one read-back at creation).
int fe_build_column_copy(hipStream_t s, int num_cus, const FeHooks& hooks, const gdmix_re_packed* b, int n, int d, int64_t z, FeCopy* out,
                         FeHot* hot, DevBuf* tables, DevBuf* cdata, DevBuf* hot_mem) {
  *hot = FeHot{0, 0, nullptr};
  FeSource src{b->row_ptr, n, b->csr_col, b->csr_val, z, d, true, (hooks.compress.value_or(FE_COMPRESS_DEFAULT) & 2) != 0};
  const long hot_min = hooks.hot_min.value_or(FE_HOT_MIN);
  std::vector<int32_t> hot_cols;
  if (hot_min > 0 && d > 0 && z > 0) {
    std::vector<int32_t> cp((size_t)d + 1);
    HIP_TRY(hipMemcpyAsync(cp.data(), b->col_ptr, ((size_t)d + 1) * 4, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    hot_cols = fe_pick_hot(cp, d, hot_min);
  }
  if (hot_cols.empty()) return fe_build_copy(s, num_cus, hooks, src, out, tables, cdata, nullptr);
  const int nh = (int)hot_cols.size();
  const int vbase = (d + FE_B - 1) / FE_B * FE_B;
  std::vector<int32_t> hotmap((size_t)d, -1);
  for (int h = 0; h < nh; ++h) hotmap[(size_t)hot_cols[(size_t)h]] = h;
  Arena a;
  const size_t o_map = a.take((size_t)d * 4), o_col2 = a.take((size_t)z * 4);
  DevBuf remap, list;
  if (!fe_alloc(remap, a.off) || !fe_alloc(list, (size_t)nh * 4)) return GDMIX_RE_ENOMEM;
  const hipError_t rc = fe_hot_remap(s, num_cus, b, n, hotmap, hot_cols, vbase, remap.as<int32_t>(o_map), list.as<int32_t>(), remap.as<int32_t>(o_col2));
  if (rc != hipSuccess) {
    (void)hipStreamSynchronize(s);
    set_error("frequent-column tables: %s", hipGetErrorString(rc));
    return GDMIX_RE_EHIP;
  }
  src.idx = remap.as<int32_t>(o_col2);
  src.len = vbase + nh * FE_HOT_REP;
  const int rc2 = fe_build_copy(s, num_cus, hooks, src, out, tables, cdata, nullptr);      // (synchronises: col2 is done with)
  if (rc2 != GDMIX_RE_OK) return rc2;
  *hot = FeHot{nh, vbase, list.as<const int32_t>()};
  *hot_mem = std::move(list);
  return GDMIX_RE_OK;
}

}  // namespace gdmix
