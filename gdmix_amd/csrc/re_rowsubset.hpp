// re_rowsubset.hpp — what the row-subsetting passes over a raw batch share (re_downsample.hip: down-sampling; re_cap.hip: the active-data
// cap): the hash, the exclusive scans of the keep flags, the output-position-driven copy of the non-zeros and the workspace layout.
//
//   plan    <the pass's own>     a keep flag per row, per chunk of DS_CHUNK rows the kept rows / their non-zeros
//           ds_chunk_scan_kernel exclusive scan of the chunk sums by one workgroup, the totals
//           ds_row_scan_kernel   exclusive scans inside every chunk: kept rows (int32) and kept non-zeros (int64) in front of each row
//   apply   <the pass's own>     the row arrays (y, offset, weight, row_nnz_ptr, the source row) and ent_row_ptr, by input row
//           ds_nnz_kernel        the non-zeros (col_global, val), by OUTPUT position: the only pass that moves real bytes
// The scans are integer sums: the same bits whatever the launch geometry. The kernels are static: each unit that includes this file
// launches its own copy.
#ifndef GDMIX_RE_ROWSUBSET_HPP_
#define GDMIX_RE_ROWSUBSET_HPP_
#include "re_internal.hpp"

namespace gdmix {

constexpr int DS_THREADS = 256;
constexpr int DS_PER_THREAD = 8;
constexpr int DS_CHUNK = DS_THREADS * DS_PER_THREAD;   // rows per workgroup of the plan kernels
constexpr int DS_NNZ_PER_THREAD = 4;                   // one float4 / two longlong2 stores per lane
constexpr int DS_TILE = DS_THREADS * DS_NNZ_PER_THREAD;   // output non-zeros per workgroup of ds_nnz_kernel
enum { DS_TOT_ROWS = 0, DS_TOT_NNZ = 1, DS_TOT_POS = 2, DS_TOT_NEG_KEPT = 3, DS_TOT_WORDS = 8 };

// splitmix64's output function (the header states it)
__host__ __device__ __forceinline__ uint64_t ds_mix(uint64_t x) {
  x += 0x9E3779B97F4A7C15ull;
  x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
  x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
  return x ^ (x >> 31);
}

__device__ __forceinline__ long long ds_wave_sum(long long v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
  return v;   // lane 0 holds the sum
}

// exclusive scan of both chunk arrays by one workgroup; the grand totals go to totals[ROWS] / totals[NNZ]
static __global__ __launch_bounds__(1024) void ds_chunk_scan_kernel(long long* __restrict__ chunk_rows, long long* __restrict__ chunk_nnz, int nb,
                                                                    unsigned long long* __restrict__ totals) {
  __shared__ long long ra[1024], za[1024];
  const int tid = threadIdx.x;
  const int per = (nb + 1023) / 1024;
  const int b0 = tid * per < nb ? tid * per : nb, b1 = (b0 + per < nb) ? b0 + per : nb;
  long long mr = 0, mz = 0;
  for (int b = b0; b < b1; ++b) { mr += chunk_rows[b]; mz += chunk_nnz[b]; }
  ra[tid] = mr; za[tid] = mz;
  __syncthreads();
  for (int off = 1; off < 1024; off <<= 1) {
    const long long vr = (tid >= off) ? ra[tid - off] : 0, vz = (tid >= off) ? za[tid - off] : 0;
    __syncthreads();
    ra[tid] += vr; za[tid] += vz;
    __syncthreads();
  }
  long long rr = ra[tid] - mr, rz = za[tid] - mz;
  for (int b = b0; b < b1; ++b) {
    const long long vr = chunk_rows[b], vz = chunk_nnz[b];
    chunk_rows[b] = rr; chunk_nnz[b] = rz;
    rr += vr; rz += vz;
  }
  if (tid == 1023) { totals[DS_TOT_ROWS] = (unsigned long long)ra[1023]; totals[DS_TOT_NNZ] = (unsigned long long)za[1023]; }
}

// row_scan[i] = kept rows in front of row i, nnz_scan[i] = their non-zeros; entry N holds the totals
static __global__ __launch_bounds__(DS_THREADS) void ds_row_scan_kernel(int64_t N, const int64_t* __restrict__ row_nnz_ptr, const uint8_t* __restrict__ keep,
                                                                        const long long* __restrict__ chunk_rows, const long long* __restrict__ chunk_nnz,
                                                                        int32_t* __restrict__ row_scan, int64_t* __restrict__ nnz_scan) {
  __shared__ long long ra[DS_THREADS], za[DS_THREADS];
  const int64_t base = (int64_t)blockIdx.x * DS_CHUNK + (int64_t)threadIdx.x * DS_PER_THREAD;
  int kf[DS_PER_THREAD];
  long long kz[DS_PER_THREAD], sr = 0, sz = 0;
#pragma unroll
  for (int k = 0; k < DS_PER_THREAD; ++k) {
    const int64_t i = base + k;
    kf[k] = 0; kz[k] = 0;
    if (i < N && keep[i]) { kf[k] = 1; kz[k] = row_nnz_ptr[i + 1] - row_nnz_ptr[i]; }
    sr += kf[k]; sz += kz[k];
  }
  ra[threadIdx.x] = sr; za[threadIdx.x] = sz;
  __syncthreads();
  for (int off = 1; off < DS_THREADS; off <<= 1) {
    const long long vr = (threadIdx.x >= off) ? ra[threadIdx.x - off] : 0, vz = (threadIdx.x >= off) ? za[threadIdx.x - off] : 0;
    __syncthreads();
    ra[threadIdx.x] += vr; za[threadIdx.x] += vz;
    __syncthreads();
  }
  long long rr = chunk_rows[blockIdx.x] + ra[threadIdx.x] - sr, rz = chunk_nnz[blockIdx.x] + za[threadIdx.x] - sz;
#pragma unroll
  for (int k = 0; k < DS_PER_THREAD; ++k) {
    const int64_t i = base + k;
    if (i < N) { row_scan[i] = (int32_t)rr; nnz_scan[i] = rz; }
    rr += kf[k]; rz += kz[k];
    if (i == N - 1) { row_scan[N] = (int32_t)rr; nnz_scan[N] = rz; }
  }
}

struct DsOut {
  int64_t N_out, Z_out;
  int64_t* ent_row_ptr; int64_t* row_nnz_ptr; int64_t* col_global; float* val; float* y; float* offset; float* weight;
};

// The copy of the non-zeros, by output position. A workgroup takes DS_TILE consecutive output positions, a lane DS_NNZ_PER_THREAD of
// them. The tile's first and last kept row come from one bisection each of the output row pointers (uniform over the workgroup: scalar
// loads); a lane then bisects only between those two for its first position and walks from there, skipping kept rows without
// non-zeros. Stores are one float4 and two longlong2 per lane (a tile starts at a multiple of DS_TILE, the arrays come from an
// allocator: 16-byte aligned, checked by the host). Loads are runs of a source row, 4 - 8 non-zeros in click-shaped data, whose
// alignment is the source's: a lane whose four positions lie in one row at a source position that is a multiple of four loads them as
// one float4 and two longlong2, the others element by element.
static __global__ __launch_bounds__(DS_THREADS) void ds_nnz_kernel(int64_t N_out, int64_t Z_out, const int64_t* __restrict__ in_row_nnz_ptr,
                                                                   const int64_t* __restrict__ in_col, const float* __restrict__ in_val,
                                                                   const int32_t* __restrict__ src_row, const int64_t* __restrict__ out_row_nnz_ptr,
                                                                   const unsigned long long* __restrict__ totals, int64_t* __restrict__ out_col,
                                                                   float* __restrict__ out_val, int wide, int wide_in) {
  if ((int64_t)totals[DS_TOT_ROWS] != N_out || (int64_t)totals[DS_TOT_NNZ] != Z_out || N_out <= 0) return;
  const int64_t tile0 = (int64_t)blockIdx.x * DS_TILE;
  if (tile0 >= Z_out) return;
  const int64_t tile_last = (tile0 + DS_TILE < Z_out ? tile0 + DS_TILE : Z_out) - 1;
  // the last kept row k with out_row_nnz_ptr[k] <= p (a row that holds p is never empty, and empty rows in front of it compare equal)
  auto row_of = [&](int64_t p, int64_t lo, int64_t hi) {   // invariant: ptr[lo] <= p, ptr[hi + 1] > p
    while (lo < hi) {
      const int64_t mid = lo + (hi - lo + 1) / 2;
      if (out_row_nnz_ptr[mid] <= p) lo = mid; else hi = mid - 1;
    }
    return lo;
  };
  const int64_t k_first = row_of(tile0, 0, N_out - 1);
  const int64_t k_last = row_of(tile_last, k_first, N_out - 1);
  const int64_t p0 = tile0 + (int64_t)threadIdx.x * DS_NNZ_PER_THREAD;
  if (p0 >= Z_out) return;
  int64_t k = row_of(p0, k_first, k_last);
  int64_t row_end = out_row_nnz_ptr[k + 1];
  int64_t shift = in_row_nnz_ptr[src_row[k]] - out_row_nnz_ptr[k];   // source position = output position + shift inside row k
  long long c[DS_NNZ_PER_THREAD];
  float v[DS_NNZ_PER_THREAD];
  // the lane's four positions lie in one source row at a source position that is a multiple of four: one float4 and two longlong2 loads
  if (wide_in && p0 + DS_NNZ_PER_THREAD <= row_end && ((p0 + shift) & 3) == 0) {
    const longlong2 a = *reinterpret_cast<const longlong2*>(in_col + p0 + shift), b = *reinterpret_cast<const longlong2*>(in_col + p0 + shift + 2);
    const float4 f = *reinterpret_cast<const float4*>(in_val + p0 + shift);
    c[0] = a.x; c[1] = a.y; c[2] = b.x; c[3] = b.y;
    v[0] = f.x; v[1] = f.y; v[2] = f.z; v[3] = f.w;
  } else {
#pragma unroll
  for (int j = 0; j < DS_NNZ_PER_THREAD; ++j) {
    const int64_t p = p0 + j;
    c[j] = 0; v[j] = 0.0f;
    if (p < Z_out) {
      while (p >= row_end && k < k_last) {
        ++k;
        row_end = out_row_nnz_ptr[k + 1];
        shift = in_row_nnz_ptr[src_row[k]] - out_row_nnz_ptr[k];
      }
      c[j] = in_col[p + shift];
      v[j] = in_val[p + shift];
    }
  }
  }
  if (wide && p0 + DS_NNZ_PER_THREAD <= Z_out) {
    longlong2 a, b;
    a.x = c[0]; a.y = c[1]; b.x = c[2]; b.y = c[3];
    *reinterpret_cast<longlong2*>(out_col + p0) = a;
    *reinterpret_cast<longlong2*>(out_col + p0 + 2) = b;
    *reinterpret_cast<float4*>(out_val + p0) = make_float4(v[0], v[1], v[2], v[3]);
  } else {
#pragma unroll
    for (int j = 0; j < DS_NNZ_PER_THREAD; ++j)
      if (p0 + j < Z_out) { out_col[p0 + j] = c[j]; out_val[p0 + j] = v[j]; }
  }
}

struct DsLayout { size_t keep, row_scan, nnz_scan, src_row, chunk_rows, chunk_nnz, totals, total; };

static DsLayout ds_layout(int64_t N) {
  DsLayout L;
  size_t off = 0;
  auto take = [&](size_t bytes) { size_t o = off; off += (bytes + 255) & ~(size_t)255; return o; };
  const size_t nb = (size_t)(N / DS_CHUNK + 2);
  L.keep = take((size_t)N + 1);
  L.row_scan = take((size_t)(N + 1) * 4);
  L.nnz_scan = take((size_t)(N + 1) * 8);
  L.src_row = take((size_t)(N + 1) * 4);
  L.chunk_rows = take(nb * 8);
  L.chunk_nnz = take(nb * 8);
  L.totals = take(DS_TOT_WORDS * 8);
  L.total = off;
  return L;
}

}  // namespace gdmix
#endif
