// re_solve_quad.hpp — FOUR ENTITIES PER WAVEFRONT: each DPP row (16 lanes) solves one entity.
//
// Why: the register-resident wave kernel is VALU-issue bound (rocprof: SQ_ACTIVE_INST_VALU ~ 90% of the
// SIMD cycles) and about half of its VALU instructions are the fp64 cross-lane reductions of the two-loop
// recursion (6 DPP stages + readlane for every dot product, ~25 per iteration). With one entity per
// 16-lane row, a reduction is 4 within-row DPP stages (quad_perm x2, row_half_mirror, row_mirror), needs
// no cross-row traffic and no readlane, and — because every VALU instruction serves four entities — its
// cost per entity drops ~6x; all other per-wave work is shared by four entities as well.
//
// Coefficient j of an entity lives in lane (j mod 16) of its row, slot (j div 16); EPL slots per lane
// hold p <= 16*EPL coefficients. Values that are uniform per ENTITY (f, step, line-search state, ...) are
// ordinary per-lane values that happen to be equal inside a row: the butterfly reductions below give
// bit-identical results to all 16 lanes, so every branch on them takes whole rows. The four entities
// of a wave advance independently, one function evaluation per trip of the main loop; an entity that is
// still line-searching simply sits out the direction update of that trip.
//
// Register diet (the (s, y) history alone is 40*EPL VGPRs): x, g, d and the history live in VGPRs;
// x_old, g_old and the per-entity scalars that are only needed between evaluations are parked in the
// row's LDS block. LDS offsets are the same for all four rows (capacity-based layout) so addressing
// needs one base VGPR. Row/column extents of the CSR/CSC copies are cached as packed (start | len << 16)
// registers, and the gathers are issued four at a time before the ordered FMA chain, so that an
// evaluation costs ~3 dependent LDS round trips instead of ~2 per non-zero.
//
// Same algorithm, stopping rules and accumulation order inside X~theta and X'r as re_solve_core.hpp /
// oracle/re_oracle.c (fit(), binary_logistic_regression.py:191-239).
#pragma once
#include "re_solve_wreg.hpp"

namespace gdmix {

constexpr int ROW = 16;   // lanes per entity

template <int CTRL>
__device__ __forceinline__ double dpp_row(double v) {
  int lo = __builtin_amdgcn_mov_dpp(__double2loint(v), CTRL, 0xf, 0xf, true);
  int hi = __builtin_amdgcn_mov_dpp(__double2hiint(v), CTRL, 0xf, 0xf, true);
  return __hiloint2double(hi, lo);
}

// (The butterfly moves through the LDS crossbar, ds_swizzle, instead of DPP: measured slower, rejected in round 6: profiles/r06_c2_ab.txt.)

// dpp_ctrl: quad_perm:[1,0,3,2] = 0xB1, quad_perm:[2,3,0,1] = 0x4E, row_half_mirror = 0x141, row_mirror = 0x140
// Butterfly: every lane of the row ends with the same bits (each stage adds the same two partial sums).
__device__ __forceinline__ double row_sum(double v) {
  v += dpp_row<0xB1>(v);
  v += dpp_row<0x4E>(v);
  v += dpp_row<0x141>(v);
  v += dpp_row<0x140>(v);
  return v;
}

__device__ __forceinline__ void row_sum2(double& a, double& b) {
#define GDMIX_RSTEP2(CTRL)              \
  {                                     \
    const double ta = dpp_row<CTRL>(a); \
    const double tb = dpp_row<CTRL>(b); \
    a += ta;                            \
    b += tb;                            \
  }
  GDMIX_RSTEP2(0xB1) GDMIX_RSTEP2(0x4E) GDMIX_RSTEP2(0x141) GDMIX_RSTEP2(0x140)
#undef GDMIX_RSTEP2
}

__device__ __forceinline__ double max_nn(double a, double b) { return (a > b) ? a : b; }

// ---- 32-lane groups (two DPP rows per entity): one more butterfly stage across the row pair ----------
// v_permlane16_swap (gfx950) swaps the odd rows of its first operand with the even rows of the second;
// fed with two copies of v it leaves {r0, r0, r2, r2} and {r1, r1, r3, r3}, whose sum is the pair total
// in all 32 lanes of each pair (same operand order in both rows -> bit-identical).
__device__ __forceinline__ void rowpair_split(double v, double& even, double& odd) {
  const unsigned lo = (unsigned)__double2loint(v), hi = (unsigned)__double2hiint(v);
  const auto l = __builtin_amdgcn_permlane16_swap(lo, lo, false, false);
  const auto h = __builtin_amdgcn_permlane16_swap(hi, hi, false, false);
  even = __hiloint2double((int)h[0], (int)l[0]);
  odd = __hiloint2double((int)h[1], (int)l[1]);
}

// v_permlane32_swap swaps the upper half of its first operand with the lower half of the second: fed with two
// copies of v it leaves {lo, lo} and {hi, hi}; their sum is the wave total in all 64 lanes.
__device__ __forceinline__ void half_split(double v, double& lower, double& upper) {
  const unsigned lo = (unsigned)__double2loint(v), hi = (unsigned)__double2hiint(v);
  const auto l = __builtin_amdgcn_permlane32_swap(lo, lo, false, false);
  const auto h = __builtin_amdgcn_permlane32_swap(hi, hi, false, false);
  lower = __hiloint2double((int)h[0], (int)l[0]);
  upper = __hiloint2double((int)h[1], (int)l[1]);
}

// Scratch of the cross-wave stage of groups wider than a wavefront (G = 64*NW): NW partials per value, double
// buffered so that one barrier per reduction suffices (a wave cannot be more than one reduction ahead).
struct XWave {
  double* buf;   // LDS [2][3][NW]
  int phase;
};

template <int G>
__device__ __forceinline__ double xwave_combine(XWave& X, double v, int slot, bool is_max) {
  constexpr int NW = G / WAVE;
  double* b = X.buf + (X.phase * 3 + slot) * NW;
  if ((threadIdx.x & (WAVE - 1)) == 0) b[threadIdx.x >> 6] = v;
  __syncthreads();
  double r = b[0];
#pragma unroll
  for (int w = 1; w < NW; ++w) r = is_max ? max_nn(r, b[w]) : r + b[w];
  return r;
}

// Sum over the G lanes of an entity; every lane of the group receives the same bits.
template <int G>
__device__ __forceinline__ double grp_sum(double v, XWave& X) {
  v = row_sum(v);
  if (G >= 32) { double a, b; rowpair_split(v, a, b); v = a + b; }
  if (G >= 64) { double a, b; half_split(v, a, b); v = a + b; }
  if (G > 64) { v = xwave_combine<G>(X, v, 0, false); X.phase ^= 1; }
  return v;
}

template <int G>
__device__ __forceinline__ void grp_sum2(double& a, double& b, XWave& X) {
  row_sum2(a, b);
  if (G >= 32) {
    double a0, a1, b0, b1;
    rowpair_split(a, a0, a1);
    rowpair_split(b, b0, b1);
    a = a0 + a1;
    b = b0 + b1;
  }
  if (G >= 64) {
    double a0, a1, b0, b1;
    half_split(a, a0, a1);
    half_split(b, b0, b1);
    a = a0 + a1;
    b = b0 + b1;
  }
  if (G > 64) {
    constexpr int NW = G / WAVE;
    double* pa = X.buf + (X.phase * 3 + 0) * NW;
    double* pb = X.buf + (X.phase * 3 + 1) * NW;
    if ((threadIdx.x & (WAVE - 1)) == 0) { pa[threadIdx.x >> 6] = a; pb[threadIdx.x >> 6] = b; }
    __syncthreads();
    a = pa[0]; b = pb[0];
#pragma unroll
    for (int w = 1; w < NW; ++w) { a += pa[w]; b += pb[w]; }
    X.phase ^= 1;
  }
}

__device__ __forceinline__ void row_sum3(double& a, double& b, double& c) {
#define GDMIX_RSTEP3S(CTRL)             \
  {                                     \
    const double ta = dpp_row<CTRL>(a); \
    const double tb = dpp_row<CTRL>(b); \
    const double tc = dpp_row<CTRL>(c); \
    a += ta;                            \
    b += tb;                            \
    c += tc;                            \
  }
  GDMIX_RSTEP3S(0xB1) GDMIX_RSTEP3S(0x4E) GDMIX_RSTEP3S(0x141) GDMIX_RSTEP3S(0x140)
#undef GDMIX_RSTEP3S
}

// three sums over the G lanes of an entity in one pass
template <int G>
__device__ __forceinline__ void grp_sum3(double& a, double& b, double& c, XWave& X) {
  row_sum3(a, b, c);
  if (G >= 32) {
    double a0, a1, b0, b1, c0, c1;
    rowpair_split(a, a0, a1);
    rowpair_split(b, b0, b1);
    rowpair_split(c, c0, c1);
    a = a0 + a1;
    b = b0 + b1;
    c = c0 + c1;
  }
  if (G >= 64) {
    double a0, a1, b0, b1, c0, c1;
    half_split(a, a0, a1);
    half_split(b, b0, b1);
    half_split(c, c0, c1);
    a = a0 + a1;
    b = b0 + b1;
    c = c0 + c1;
  }
  if (G > 64) {
    constexpr int NW = G / WAVE;
    double* pa = X.buf + (X.phase * 3 + 0) * NW;
    double* pb = X.buf + (X.phase * 3 + 1) * NW;
    double* pc = X.buf + (X.phase * 3 + 2) * NW;
    if ((threadIdx.x & (WAVE - 1)) == 0) { pa[threadIdx.x >> 6] = a; pb[threadIdx.x >> 6] = b; pc[threadIdx.x >> 6] = c; }
    __syncthreads();
    a = pa[0]; b = pb[0]; c = pc[0];
#pragma unroll
    for (int w = 1; w < NW; ++w) { a += pa[w]; b += pb[w]; c += pc[w]; }
    X.phase ^= 1;
  }
}

__device__ __forceinline__ void row_sum2_max(double& a, double& b, double& c) {
#define GDMIX_RSTEP3(CTRL)              \
  {                                     \
    const double ta = dpp_row<CTRL>(a); \
    const double tb = dpp_row<CTRL>(b); \
    const double tc = dpp_row<CTRL>(c); \
    a += ta;                            \
    b += tb;                            \
    c = max_nn(c, tc);                  \
  }
  GDMIX_RSTEP3(0xB1) GDMIX_RSTEP3(0x4E) GDMIX_RSTEP3(0x141) GDMIX_RSTEP3(0x140)
#undef GDMIX_RSTEP3
}

template <int G>
__device__ __forceinline__ void grp_sum2_max(double& a, double& b, double& c, XWave& X) {
  row_sum2_max(a, b, c);
  if (G >= 32) {
    double a0, a1, b0, b1, c0, c1;
    rowpair_split(a, a0, a1);
    rowpair_split(b, b0, b1);
    rowpair_split(c, c0, c1);
    a = a0 + a1;
    b = b0 + b1;
    c = max_nn(c0, c1);
  }
  if (G >= 64) {
    double a0, a1, b0, b1, c0, c1;
    half_split(a, a0, a1);
    half_split(b, b0, b1);
    half_split(c, c0, c1);
    a = a0 + a1;
    b = b0 + b1;
    c = max_nn(c0, c1);
  }
  if (G > 64) {
    constexpr int NW = G / WAVE;
    double* pa = X.buf + (X.phase * 3 + 0) * NW;
    double* pb = X.buf + (X.phase * 3 + 1) * NW;
    double* pc = X.buf + (X.phase * 3 + 2) * NW;
    if ((threadIdx.x & (WAVE - 1)) == 0) { pa[threadIdx.x >> 6] = a; pb[threadIdx.x >> 6] = b; pc[threadIdx.x >> 6] = c; }
    __syncthreads();
    a = pa[0]; b = pb[0]; c = pc[0];
#pragma unroll
    for (int w = 1; w < NW; ++w) { a += pa[w]; b += pb[w]; c = max_nn(c, pc[w]); }
    X.phase ^= 1;
  }
}

// ordering point between LDS writes and reads of different lanes of one entity
template <int G>
__device__ __forceinline__ void grp_fence() {
  if (G > 64) __syncthreads();
  else wave_lds_fence();
}

// ---- capacity-based LDS layout of one row (entity) ---------------------------------------------------
// Offsets depend only on (PCAP = 16*EPL, NCAP, ZCAP), i.e. they are wave-uniform.
struct QuadLayout {
  int xs, xo, go, rs, csr, csc, row_ptr, col_ptr, y, o, w, bytes;
};

// (The history split by age of round 3 — the oldest pairs of an EPL = 4 kernel in LDS instead of spilled VGPRs — lost 4 - 38 % on
// <16,4> and was deleted in round 4: profiles/r03_c2_history_by_age.txt.)
constexpr int QUAD_HDR_BYTES = 8 * (2 * M_REG + 16 + 8);   // rho, alpha, LineSearch slot, 8 scalars (one per wavefront of the group)

// (The rows of a wavefront padded to start 32 LDS banks apart: fewer bank conflicts, same time, rejected in round 6: profiles/r06_c2_ab.txt.)
__host__ __device__ inline QuadLayout quad_layout(int pcap, int ncap, int zcap, int waves = 1) {
  QuadLayout q;
  // groups wider than a wavefront keep one private copy of the uniform solver state per wavefront (all
  // copies hold the same values; sharing one would race between a fast wave's write and a slow wave's read)
  // plus the cross-wave reduction scratch
  int off = QUAD_HDR_BYTES * waves + (waves > 1 ? 8 * 2 * 3 * waves : 0);
  q.xs = off; off += 8 * pcap;
  q.xo = off; off += 8 * pcap;
  q.go = off; off += 8 * pcap;
  q.rs = off; off += 8 * ncap;
  q.csr = off; off += 8 * zcap;
  q.csc = off; off += 8 * zcap;
  q.row_ptr = off; off += 4 * (ncap + 1);
  q.col_ptr = off; off += 4 * (pcap + 1);
  q.y = off; off += 4 * ncap;
  q.o = off; off += 4 * ncap;
  q.w = off; off += 4 * ncap;
  q.bytes = (off + 15) & ~15;
  return q;
}

// Pointers into one row's LDS block (derived from one per-lane base + uniform offsets).
struct QuadLds {
  unsigned char* base;   // the entity's LDS block
  unsigned char* hdr;    // this wavefront's private header inside it
  QuadLayout q;
  bool has_w;
  __device__ __forceinline__ double* rho() const { return reinterpret_cast<double*>(hdr); }
  __device__ __forceinline__ double* alpha() const { return reinterpret_cast<double*>(hdr) + M_REG; }
  __device__ __forceinline__ LineSearch* ls() const { return reinterpret_cast<LineSearch*>(hdr + 16 * M_REG); }
  __device__ __forceinline__ double* scal() const { return reinterpret_cast<double*>(hdr + 16 * M_REG + 128); }
  __device__ __forceinline__ double* xs() const { return reinterpret_cast<double*>(base + q.xs); }
  __device__ __forceinline__ double* xo() const { return reinterpret_cast<double*>(base + q.xo); }
  __device__ __forceinline__ double* go() const { return reinterpret_cast<double*>(base + q.go); }
  __device__ __forceinline__ double* rs() const { return reinterpret_cast<double*>(base + q.rs); }
  __device__ __forceinline__ int2* csr() const { return reinterpret_cast<int2*>(base + q.csr); }
  __device__ __forceinline__ int2* csc() const { return reinterpret_cast<int2*>(base + q.csc); }
  __device__ __forceinline__ int32_t* row_ptr() const { return reinterpret_cast<int32_t*>(base + q.row_ptr); }
  __device__ __forceinline__ int32_t* col_ptr() const { return reinterpret_cast<int32_t*>(base + q.col_ptr); }
  __device__ __forceinline__ float* y() const { return reinterpret_cast<float*>(base + q.y); }
  __device__ __forceinline__ float* o() const { return reinterpret_cast<float*>(base + q.o); }
  __device__ __forceinline__ float* w() const { return reinterpret_cast<float*>(base + q.w); }
};
static_assert(sizeof(LineSearch) <= 128, "LineSearch must fit its LDS slot");

enum { SC_FOLD = 0, SC_GDOLD = 1, SC_THETA = 2, SC_MOVED = 3 };

// Which kernels keep the bounds test j < p on every coefficient slot of the trip (quad_eval, "dead slots"): those of several wavefronts
// per entity with four slots per lane. Their register allocation is the tightest of all (60 to 90 spilled registers) and comes out 5 to
// 17 registers worse without the masked regions; they are the code they were. Every other kernel runs the trip without the tests.
constexpr bool grp_slot_tests(int g, int epl) { return g > WAVE && epl >= 4; }

// (The per-entity rho, alpha and scalars in the lanes of a register pair instead of LDS: slower, rejected in round 6: profiles/r06_c2_ab.txt.)

// Is `v` true in any lane of the entity's group? G <= 64: from the wavefront's ballot (all lanes of a group are active
// together). Wider groups: this wavefront's part only (quad_eval collects the wavefronts' parts behind its first fence).
template <int G>
__device__ __forceinline__ bool grp_any(bool v) {
  const unsigned long long m = __ballot(v);
  if (G >= WAVE) return m != 0ull;
  const int sh = (int)threadIdx.x & (WAVE - 1) & ~(G - 1);
  return ((m >> sh) & ((1ull << G) - 1ull)) != 0ull;
}

// sum_k val[k] * vec[idx[k]] over `len` packed {idx, float bits} pairs starting at `pairs`, added to acc
// in index order. Gathers are issued four at a time; the FMA chain keeps the sequential order (masked
// tail entries multiply by an exact 0).
__device__ __forceinline__ double gather_dot(const int2* pairs, int len, const double* vec, double acc) {
  for (int c = 0; c < len; c += 4) {
    const int r = len - c;   // >= 1
    const int2 p0 = pairs[c];
    const int2 p1 = pairs[c + (r > 1 ? 1 : 0)];
    const int2 p2 = pairs[c + (r > 2 ? 2 : 0)];
    const int2 p3 = pairs[c + (r > 3 ? 3 : 0)];
    const double v0 = vec[p0.x], v1 = vec[p1.x], v2 = vec[p2.x], v3 = vec[p3.x];
    acc += (double)__int_as_float(p0.y) * v0;
    acc += (r > 1 ? (double)__int_as_float(p1.y) : 0.0) * v1;
    acc += (r > 2 ? (double)__int_as_float(p2.y) : 0.0) * v2;
    acc += (r > 3 ? (double)__int_as_float(p3.y) : 0.0) * v3;
  }
  return acc;
}

// The EPL columns of a lane in ONE loop, two entries of each per trip: every trip issues all its pair loads, then all its
// gathers (2 EPL in flight) — EPL loops one after the other were 2 EPL dependent LDS round trips per trip of each and a loop
// branch per column, with two wavefronts per SIMD to hide them. A column's products are added in its own order as before;
// a column that has ended adds exact zeros (gathered from the residual's slot 0, always finite).
template <int EPL>
__device__ __forceinline__ void gather_dot2_cols(const int2* csc, const unsigned (&colc)[EPL], const double* vec, double (&acc)[EPL]) {
  int len[EPL], mx = 0;
  const int2* pairs[EPL];
#pragma unroll
  for (int s = 0; s < EPL; ++s) {
    len[s] = (int)(colc[s] >> 16);
    pairs[s] = csc + (colc[s] & 0xffffu);
    mx = max(mx, len[s]);
  }
  for (int c = 0; c < mx; c += 2) {
    int2 p0[EPL], p1[EPL];
#pragma unroll
    for (int s = 0; s < EPL; ++s) {
      const int r = len[s] - c;
      p0[s] = pairs[s][r > 0 ? c : 0];
      p1[s] = pairs[s][r > 1 ? c + 1 : 0];
      if (r <= 0) p0[s] = make_int2(0, 0);
      if (r <= 1) p1[s] = make_int2(0, 0);
    }
    double v0[EPL], v1[EPL];
#pragma unroll
    for (int s = 0; s < EPL; ++s) { v0[s] = vec[p0[s].x]; v1[s] = vec[p1[s].x]; }
#pragma unroll
    for (int s = 0; s < EPL; ++s) {
      acc[s] += (double)__int_as_float(p0[s].y) * v0[s];
      acc[s] += (double)__int_as_float(p1[s].y) * v1[s];
    }
  }
}

// The same with ONE entry of each column per trip (EPL = 4: two per trip spill).
template <int EPL>
__device__ __forceinline__ void gather_dot1_cols(const int2* csc, const unsigned (&colc)[EPL], const double* vec, double (&acc)[EPL]) {
  int len[EPL], mx = 0;
  const int2* pairs[EPL];
#pragma unroll
  for (int s = 0; s < EPL; ++s) {
    len[s] = (int)(colc[s] >> 16);
    pairs[s] = csc + (colc[s] & 0xffffu);
    mx = max(mx, len[s]);
  }
  for (int c = 0; c < mx; ++c) {
    int2 p0[EPL];
#pragma unroll
    for (int s = 0; s < EPL; ++s) {
      p0[s] = pairs[s][c < len[s] ? c : 0];
      if (c >= len[s]) p0[s] = make_int2(0, 0);
    }
    double v0[EPL];
#pragma unroll
    for (int s = 0; s < EPL; ++s) v0[s] = vec[p0[s].x];
#pragma unroll
    for (int s = 0; s < EPL; ++s) acc[s] += (double)__int_as_float(p0[s].y) * v0[s];
  }
}

// f and g at xt. rowc: packed (start | len << 16) of the lane's first sample; colc[s]: same for the
// lane's coefficient slots (len = 0 for the intercept / unused slots).
// LOSS: the loss code (re_device.hpp, loss_terms).
// DEAD SLOTS (docs/kernels.md, "Dead slots"): a slot j = gl + G s >= p has no column (colc[s] == 0), starts at x = +0.0 and has zeros
// in xs, xo and go (quad_solve writes them once per entity), so the per-slot loops here and in quad_solve's trip do not test j < p
// (`live`; what is left of the tests and why is said where it stands: two sites, and the kernels of grp_slot_tests). A dead slot's gradient
// is inv_n * (0 + l2 * 0) = +0.0, its d, s and y are zeros of either sign, it adds exact zeros to every sum and |0| to the maximum, and
// x stays +0.0: the bits the selects gave. That holds while inv_n, l2 and the residual of sample 0 (what an ended column of the fused
// gathers multiplies by 0) are finite; the two cases where they are not on finite input are kept apart below.
// EMPTY: the class can hold an entity without samples (n == 0: inv_n = inf). Such an entity has no column either (p = ic <= 1) and fits
// every cap, so the first-fit rule sends it to the FIRST group class and to no other: only that class's kernel carries the guard.
template <int G, int EPL, bool LONG_COLS = true, int LOSS = LOSS_LOGISTIC, bool EMPTY = true>
__device__ __forceinline__ double quad_eval(const QuadLds& L, const SolveParams& o, int gl, int n, int p, int ic,
                                            unsigned rowc, const unsigned (&colc)[EPL], const double (&xt)[EPL],
                                            double (&g)[EPL], XWave& X, bool first, bool& counted) {
  double* const xs = L.xs();
  double* const rs = L.rs();
  constexpr bool TESTS = grp_slot_tests(G, EPL);
  const auto live = [&](int j) { return !TESTS || j < p; };
  // xs still holds the point of the previous evaluation: scipy's ScalarFunction serves an equal point from its cache without
  // counting it (nfev is its funcalls; a step too small to move x, _differentiable_functions.py)
  bool mv = first;
#pragma unroll
  for (int s = 0; s < EPL; ++s) {
    const int j = gl + G * s;
    if (live(j)) {
      mv = mv || (xs[j] != xt[s]);   // (a dead slot: 0 != 0)
      xs[j] = xt[s];
    }
  }
  counted = grp_any<G>(mv);
  if (G > WAVE) L.scal()[SC_MOVED] = counted ? 1.0 : 0.0;   // this wavefront's part; the others' behind the fence
  grp_fence<G>();
  if (G > WAVE) {
    constexpr int NWG = G / WAVE;
    bool any = false;
#pragma unroll
    for (int w = 0; w < NWG; ++w) any = any || reinterpret_cast<const double*>(L.base + w * QUAD_HDR_BYTES + 16 * M_REG + 128)[SC_MOVED] != 0.0;
    counted = any;
  }
  double part = 0.0, rpart = 0.0;
  const double x0 = ic ? xs[0] : 0.0;
  if (gl < n) {
    const double z = gather_dot(L.csr() + (rowc & 0xffffu), (int)(rowc >> 16), xs + ic, x0) + (double)L.o()[gl];
    double ri;
    part = loss_terms<LOSS>(z, (double)L.y()[gl], L.has_w ? (double)L.w()[gl] : 1.0, ri);
    rs[gl] = ri;
    rpart = ri;
  }
  for (int i = gl + G; i < n; i += G) {   // entities with more samples than lanes
    const int k0 = L.row_ptr()[i], k1 = L.row_ptr()[i + 1];
    const double z = gather_dot(L.csr() + k0, k1 - k0, xs + ic, x0) + (double)L.o()[i];
    double ri;
    part += loss_terms<LOSS>(z, (double)L.y()[i], L.has_w ? (double)L.w()[i] : 1.0, ri);
    rs[i] = ri;
    rpart += ri;
  }
  const int first_reg = (ic && !o.regularize_bias) ? 1 : 0;
  double sq = 0.0;
#pragma unroll
  for (int s = 0; s < EPL; ++s) {
    const int j = gl + G * s;
    if (j >= first_reg && live(j)) sq += xt[s] * xt[s];   // (j < first_reg: slot 0 of lane 0 alone)
  }
  // cost.sum() and the regulariser are summed separately and added once, as the reference writes it
  // (binary_logistic_regression.py:105-108): spreading (l2/2) x_j^2 over the lanes' loss partials rounds differently, which
  // decides line searches on entities whose loss is ~1e13 (tests/golden exit_extreme_02)
  grp_sum3<G>(part, rpart, sq, X);
  part += 0.5 * o.l2 * sq;
  grp_fence<G>();
  const double inv_n = 1.0 / (double)n;
  // An entity without samples (the pack takes one) has inv_n = inf, and inf * 0 is no zero: its dead slots (every slot s >= 1, and slot 0
  // of every lane but an intercept's) take the factor 0 instead, two selects per evaluation outside the slot loops. For n > 0, and in
  // every kernel but the first class's, both are inv_n.
  const double inv_hi = (!EMPTY || n > 0) ? inv_n : 0.0;
  const double inv_lo = (!EMPTY || gl < p) ? inv_n : inv_hi;
  if (EPL <= 3 || LONG_COLS) {
    double acc[EPL];
#pragma unroll
    for (int s = 0; s < EPL; ++s) {
      const int j = gl + G * s;
      acc[s] = (ic && j == 0) ? rpart : 0.0;
    }
    if (EPL <= 3) gather_dot2_cols<EPL>(L.csc(), colc, rs, acc);   // (a dead slot's colc is 0: an ended column from the start)
    else gather_dot1_cols<EPL>(L.csc(), colc, rs, acc);
#pragma unroll
    for (int s = 0; s < EPL; ++s) {
      const int j = gl + G * s;
      const double reg = (j < first_reg) ? 0.0 : o.l2 * xt[s];
      double gj = (s == 0 ? inv_lo : inv_hi) * (acc[s] + reg);
      // The product is rounded HERE, as it was when a select stood between it and its uses: left open, the compiler contracts it into
      // the subtraction g - g_old of quad_solve (one fused multiply-add, one rounding fewer) and a trip in twenty changes its last bit.
      asm("" : "+v"(gj));
      // exp(z) of sample 0 overflows to inf at a trial point too far out (the line search comes back from f = inf), and an ended
      // column has added 0 * inf: the Poisson kernels keep the select
      if constexpr (LOSS == LOSS_POISSON || TESTS) g[s] = (j < p) ? gj : 0.0;
      else g[s] = gj;
    }
    return inv_n * part;
  }
#pragma unroll
  for (int s = 0; s < EPL; ++s) {
    const int j = gl + G * s;
    double gj = 0.0;
    // (a dead slot's loop takes no trip and its gj is +0.0 either way, but this path is the EPL = 4 kernels' alone, and they spill a
    // register more without the region)
    if (j < p) {
      double acc = (ic && j == 0) ? rpart : 0.0;
      acc = gather_dot(L.csc() + (colc[s] & 0xffffu), (int)(colc[s] >> 16), rs, acc);
      const double reg = (j < first_reg) ? 0.0 : o.l2 * xt[s];
      gj = (s == 0 ? inv_lo : inv_hi) * (acc + reg);
    }
    g[s] = gj;
  }
  return inv_n * part;
}

template <int EPL>
struct QuadState {
  double x[EPL], g[EPL], d[EPL];
};

// The solve of the (up to) four entities of a wave. `valid` marks rows that own an entity.
// LONG_COLS: the class holds entities with more samples than the group has lanes (columns of several entries are the rule): the
// EPL = 4 kernels then gather their four columns in one loop too, an entry of each per trip (C5-shaped classes - 1 to - 3 %); where
// columns mostly hold one entry (C2's <16,4>: n <= 16) the four short loops are as fast and spill less (+ 0.5 % with the fused loop)
// KR: how many of the M_REG pairs live in the register shift register. KR < M_REG (the EPL = 5 kernel: ten pairs of five slots would
// be 200 VGPRs) splits the history by age: the newest KR pairs in registers as ever, and a pair that ages out of them is written ONCE
// into a per-lane ring of M_REG - KR pairs (a private array indexed by a per-row slot, i.e. scratch memory). A push moves no old pair;
// the ring is read only by the two-loop steps of rows whose history is longer than KR. Same pairs, same order of the steps, same
// arithmetic: where a pair lives changes no bit. KR == M_REG is the code as it was (no ring, every `if constexpr` below folds away).
template <int G, int EPL, bool LONG_COLS = true, int LOSS = LOSS_LOGISTIC, int KR = M_REG, bool EMPTY = true>
__device__ __forceinline__ void quad_solve(const QuadLds& L, const SolveParams& o, int gl, int n, int p, int ic,
                                           bool valid, unsigned rowc, const unsigned (&colc)[EPL], QuadState<EPL>& V,
                                           XWave& X, SolveStats& out) {
  // pair a of M_REG, newest last: the last KR in a register shift register (every index a compile-time constant), pair a < RN in the ring
  static_assert(KR >= 1 && KR <= M_REG, "register-resident pairs");
  constexpr int RN = M_REG - KR;
  double S[KR][EPL], Y[KR][EPL];
  double RS[RN > 0 ? RN : 1][EPL], RY[RN > 0 ? RN : 1][EPL];   // the ring; `head`: the slot the next aged pair goes to (per row)
  int head = 0;
#pragma unroll
  for (int a = 0; a < KR; ++a) {
#pragma unroll
    for (int s = 0; s < EPL; ++s) { S[a][s] = 0.0; Y[a][s] = 0.0; }
  }
  double* const rho = L.rho();      // per-entity uniform state: every lane of the row stores the same value
  double* const alpha = L.alpha();
  double* const scal = L.scal();
  double* const xo = L.xo();
  double* const go = L.go();
  constexpr bool TESTS = grp_slot_tests(G, EPL);
  const auto live = [&](int j) { return !TESTS || j < p; };
  const int m = o.m;
  int cnt = 0;
  int nit = 0, nfev = 0, ifun = 0;
  int status = valid ? -1 : 0;
  bool iter0 = true, first = true;
  // nfev is scipy's funcalls: an evaluation at the point of the previous evaluation is not counted (quad_eval)
  double f = 0.0, gd = 0.0, rr = 0.0, stp = 0.0, sbgnrm = 0.0;
  if (valid) {
    scal[SC_FOLD] = 0.0; scal[SC_GDOLD] = 0.0; scal[SC_THETA] = 1.0;
    // every slot of the row's G * EPL, the dead ones (j >= p) included: what lets the trip below touch xs, xo and go without a bounds
    // test (quad_eval, "dead slots"). The lanes' slots tile [0, G * EPL), the extent of the three arrays (quad_layout).
    double* const xs = L.xs();
#pragma unroll
    for (int s = 0; s < EPL; ++s) {
      const int j = gl + G * s;
      if (!TESTS) xs[j] = 0.0;
      if (live(j)) { xo[j] = 0.0; go[j] = 0.0; }
    }
  }
  while (__any(status < 0)) {
    bool need_dir = false, restart = false;
    if (status < 0) {
      // ---- f, g at the trial point; g'd, y'y and max|g| in one reduction pass ------------------------
      bool counted;
      f = quad_eval<G, EPL, LONG_COLS, LOSS, EMPTY>(L, o, gl, n, p, ic, rowc, colc, V.x, V.g, X, first, counted);
      nfev += counted ? 1 : 0;
      {
        double a = 0.0, b = 0.0, c = 0.0;
#pragma unroll
        for (int s = 0; s < EPL; ++s) {
          const int j = gl + G * s;
          // (a bounds test that stays in every kernel: this is the trip's register peak, and EPL unconditional loads in flight together made every
          // EPL = 4 kernel spill 10 to 25 registers more; the masked loads come one after the other)
          const double gold = (j < p) ? go[j] : 0.0;
          a += V.g[s] * V.d[s];
          const double yj = V.g[s] - gold;
          b += yj * yj;
          c = max_nn(c, fabs(V.g[s]));
        }
        grp_sum2_max<G>(a, b, c, X);
        gd = a; rr = b; sbgnrm = c;
      }
      if (first) {
        first = false;
        if (sbgnrm <= o.pgtol) status = 0;
        else need_dir = true;
      } else {
        // the first trial is accepted 95 % of the time: three numbers of the search's state decide that (dcsrch_converged); the rest
        // of the state is read — and, when the search goes on, written back — only when a row of the wave needs it (an accepted or
        // abandoned search is started afresh by dcsrch_start: nothing reads its state again). LDS traffic is what a trip of these
        // kernels waits for: the 15 stores alone were 2 % of the C2 step.
        int task = LS_CONV;
        {
          const LineSearch* const lsp = L.ls();
          const bool conv = dcsrch_converged(lsp->finit, lsp->gtest, lsp->ginit, f, gd, stp);
          if (__any(!conv)) {
            if (!conv) {
              LineSearch LS = *L.ls();
              task = dcsrch_step(LS, f, gd, stp);
              if (task == LS_FG) *L.ls() = LS;
            }
          }
        }
        if (task == LS_FG) {
          ++ifun;
          if (ifun - 1 < o.maxls) {
#pragma unroll
            for (int s = 0; s < EPL; ++s) {
              const int j = gl + G * s;
              if (live(j)) V.x[s] = stp * V.d[s] + xo[j];   // stp == 1: exactly xo + d
            }
          } else {
            restart = true;   // iback >= maxls
            need_dir = true;
          }
        } else {
          // ---- NEW_X: scipy's python loop first (nit / maxiter / maxfun), then mainlb's own tests ---
          ++nit;
          iter0 = false;
          const double fold = scal[SC_FOLD];
          const double dmx = fmax(fabs(fold), fmax(fabs(f), 1.0));
          if (nit >= o.max_iter) status = 2;
          else if (nfev > o.maxfun) status = 3;
          else if (sbgnrm <= o.pgtol) status = 0;
          else if (fold - f <= o.ftol * dmx) status = 1;
          else {
            need_dir = true;
            const double gdold = scal[SC_GDOLD];
            double dr, ddum;
            if (stp == 1.0) { dr = gd - gdold; ddum = -gdold; }
            else { dr = (gd - gdold) * stp; ddum = -gdold * stp; }
            if (dr > EPSMCH * ddum) {
              // push (s, y): the history shifts down by one, newest at KR-1
              // (Appending at the wavefront's next free slot instead: three times slower, rejected in round 6: profiles/r06_c2_ab.txt.)
#pragma unroll
              for (int a = 0; a < M_REG - 1; ++a) rho[a] = rho[a + 1];
              if constexpr (RN > 0) {
                // the oldest register pair ages into the ring; one that no direction can use again (cnt < KR: it has never been
                // within the row's last cnt pairs and every later push moves it further away; m <= KR) is not worth the stores
                if (cnt >= KR && m > KR) {
#pragma unroll
                  for (int s = 0; s < EPL; ++s) { RS[head][s] = S[0][s]; RY[head][s] = Y[0][s]; }
                }
                head = (head + 1 == RN) ? 0 : head + 1;
              }
#pragma unroll
              for (int a = 0; a < KR - 1; ++a) {
#pragma unroll
                for (int s = 0; s < EPL; ++s) { S[a][s] = S[a + 1][s]; Y[a][s] = Y[a + 1][s]; }
              }
#pragma unroll
              for (int s = 0; s < EPL; ++s) {
                const int j = gl + G * s;
                S[KR - 1][s] = stp * V.d[s];   // exact for stp == 1
                Y[KR - 1][s] = V.g[s] - (live(j) ? go[j] : 0.0);
              }
              rho[M_REG - 1] = 1.0 / dr;
              scal[SC_THETA] = rr / dr;
              if (cnt < m) ++cnt;
            }
          }
        }
      }
    }
    // ---- new search direction for the rows that need one (again after a line-search restart) ---------
    while (__any(need_dir)) {
      if (need_dir && restart) {
#pragma unroll
        for (int s = 0; s < EPL; ++s) {
          const int j = gl + G * s;
          if (live(j)) { V.x[s] = xo[j]; V.g[s] = go[j]; }
        }
        f = scal[SC_FOLD];
        restart = false;
        if (cnt == 0) { status = 4; need_dir = false; }
        else {
          cnt = 0;
          scal[SC_THETA] = 1.0;
        }
      }
      if (need_dir) {
#pragma unroll
        for (int s = 0; s < EPL; ++s) V.d[s] = -V.g[s];
      }
      // two-loop recursion over each row's last cnt pairs (indices M_REG-cnt .. M_REG-1, newest last). The pairs any row of the wave
      // uses are M_REG-cmax .. M_REG-1 with cmax uniform: the first loop leaves at its lower end, the second enters at it (a switch
      // that falls through) — until round 5 every one of the 2 M_REG steps was skipped on its own (`if (__any(use))`: a compare, an
      // exec save and a taken branch each, ~11 of 20 skipped at C2's mean history of 4.5 pairs).
      // (Zero-multiplier steps for the rows that do not use a pair, instead of masked ones: slower, rejected in round 6: profiles/r06_c2_ab.txt.)
      const int cmax = wave_max_nonneg_i32(need_dir ? cnt : 0);
      const int a0 = M_REG - cmax;
      // ring slot of pair a < RN: the pair that aged last (a = RN - 1) sits at head - 1, the one before it at head - 2, ...
      const auto ring_slot = [&](int a) { const int sl = head - (RN - a); return sl < 0 ? sl + RN : sl; };
      (void)ring_slot;
#define QUAD_FIRST_LOOP_STEP(a)                                                   \
      {                                                                           \
        if ((a) < a0) goto first_loop_done;                                       \
        const bool use = need_dir && ((a) >= M_REG - cnt);                        \
        if (use) {                                                                \
          if constexpr ((a) >= RN) {                                              \
            double t = 0.0;                                                       \
            _Pragma("unroll") for (int s = 0; s < EPL; ++s) t += S[(a) - RN][s] * V.d[s];  \
            const double al = rho[a] * grp_sum<G>(t, X);                          \
            alpha[a] = al;                                                        \
            _Pragma("unroll") for (int s = 0; s < EPL; ++s) V.d[s] -= al * Y[(a) - RN][s]; \
          } else {                                                                \
            const int sl = ring_slot(a);                                          \
            double t = 0.0;                                                       \
            _Pragma("unroll") for (int s = 0; s < EPL; ++s) t += RS[sl][s] * V.d[s];       \
            const double al = rho[a] * grp_sum<G>(t, X);                          \
            alpha[a] = al;                                                        \
            _Pragma("unroll") for (int s = 0; s < EPL; ++s) V.d[s] -= al * RY[sl][s];      \
          }                                                                       \
        }                                                                         \
      }
      static_assert(M_REG == 10, "the steps below are written out for ten pairs");
      QUAD_FIRST_LOOP_STEP(9) QUAD_FIRST_LOOP_STEP(8) QUAD_FIRST_LOOP_STEP(7) QUAD_FIRST_LOOP_STEP(6) QUAD_FIRST_LOOP_STEP(5)
      QUAD_FIRST_LOOP_STEP(4) QUAD_FIRST_LOOP_STEP(3) QUAD_FIRST_LOOP_STEP(2) QUAD_FIRST_LOOP_STEP(1) QUAD_FIRST_LOOP_STEP(0)
#undef QUAD_FIRST_LOOP_STEP
    first_loop_done:;
      if (need_dir && cnt > 0) {
        const double h0 = 1.0 / scal[SC_THETA];
#pragma unroll
        for (int s = 0; s < EPL; ++s) V.d[s] *= h0;
      }
#define QUAD_SECOND_LOOP_STEP(a)                                                  \
      {                                                                           \
        const bool use = need_dir && ((a) >= M_REG - cnt);                        \
        if (use) {                                                                \
          if constexpr ((a) >= RN) {                                              \
            double t = 0.0;                                                       \
            _Pragma("unroll") for (int s = 0; s < EPL; ++s) t += Y[(a) - RN][s] * V.d[s];  \
            const double c = alpha[a] - rho[a] * grp_sum<G>(t, X);                \
            _Pragma("unroll") for (int s = 0; s < EPL; ++s) V.d[s] += c * S[(a) - RN][s];  \
          } else {                                                                \
            const int sl = ring_slot(a);                                          \
            double t = 0.0;                                                       \
            _Pragma("unroll") for (int s = 0; s < EPL; ++s) t += RY[sl][s] * V.d[s];       \
            const double c = alpha[a] - rho[a] * grp_sum<G>(t, X);                \
            _Pragma("unroll") for (int s = 0; s < EPL; ++s) V.d[s] += c * RS[sl][s];       \
          }                                                                       \
        }                                                                         \
      }
      switch (a0) {
        case 0: QUAD_SECOND_LOOP_STEP(0) [[fallthrough]];
        case 1: QUAD_SECOND_LOOP_STEP(1) [[fallthrough]];
        case 2: QUAD_SECOND_LOOP_STEP(2) [[fallthrough]];
        case 3: QUAD_SECOND_LOOP_STEP(3) [[fallthrough]];
        case 4: QUAD_SECOND_LOOP_STEP(4) [[fallthrough]];
        case 5: QUAD_SECOND_LOOP_STEP(5) [[fallthrough]];
        case 6: QUAD_SECOND_LOOP_STEP(6) [[fallthrough]];
        case 7: QUAD_SECOND_LOOP_STEP(7) [[fallthrough]];
        case 8: QUAD_SECOND_LOOP_STEP(8) [[fallthrough]];
        case 9: QUAD_SECOND_LOOP_STEP(9) [[fallthrough]];
        default: break;
      }
#undef QUAD_SECOND_LOOP_STEP
      if (need_dir) {
        // z = x + d ; d = z - x (mainlb re-derives d from the subspace point); save x, g
        double dd = 0.0, gdp = 0.0;
#pragma unroll
        for (int s = 0; s < EPL; ++s) {
          const int j = gl + G * s;
          const double xj = V.x[s];
          const double z = xj + V.d[s];
          const double dj = z - xj;
          V.d[s] = dj;
          if (live(j)) { xo[j] = xj; go[j] = V.g[s]; }
          dd += dj * dj;
          gdp += V.g[s] * dj;
        }
        grp_sum2<G>(dd, gdp, X);
        gd = gdp;
        scal[SC_GDOLD] = gd;
        scal[SC_FOLD] = f;
        if (gd >= 0.0) {
          restart = true;   // lnsrlb info = -4: stay in this loop
        } else {
          stp = iter0 ? fmin(1.0 / sqrt(dd), LS_STPMAX) : 1.0;
          LineSearch LS;
          dcsrch_start(LS, f, gd, stp);
          *L.ls() = LS;
          ifun = 1;
#pragma unroll
          for (int s = 0; s < EPL; ++s) V.x[s] = stp * V.d[s] + V.x[s];   // V.x still holds x_old here
          need_dir = false;
        }
      }
    }
  }
  if (status == 4) {   // abnormal stop: report the restored gradient's norm
    double mx = 0.0;
#pragma unroll
    for (int s = 0; s < EPL; ++s) mx = max_nn(mx, fabs(V.g[s]));
    double d0 = 0.0, d1 = 0.0;
    grp_sum2_max<G>(d0, d1, mx, X);
    sbgnrm = mx;
  }
  out.f = f;
  out.gnorm = sbgnrm;
  out.nit = nit;
  out.nfev = nfev;
  out.status = status;
}

}  // namespace gdmix
