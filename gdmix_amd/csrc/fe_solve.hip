// fe_solve.hip — fixed-effect trainer (include/gdmix_fe.h): one worker's shard resident in HBM, one L-BFGS
// evaluation = two streaming passes over it + a handful of small kernels; the L-BFGS driver is the same resumable
// compact-form step the team kernels use (re_lbfgs_compact.hpp), here with its state in HBM between kernels so
// that the caller can all-reduce [gradient, value] across workers in between
// (fixed_effect_lr_lbfgs_model.py:309-392: _train_model_fn; :394-430 _compute_loss_and_gradients; :635-643).
//
// The two passes (fe_scatter_kernel) are written for HBM: no gather may cost an L2 request per entry, and no sum may
// depend on the launch. Each pass has its own copy of the non-zeros, grouped by block of FE_B consecutive *outputs* (rows
// for X theta, columns for X'r) and, inside a block, in the order of the *gathered* vector (columns for X theta, rows for
// X'r): one wavefront owns a block's FE_B accumulators in LDS, streams the block's entries (8 B each, every byte once:
// fp32 value + one word holding the accumulator index and the gathered element's index relative to the unit's first;
// three arrays and 10 B when a unit spans more than 2^21 gathered elements), reads the gathered vector almost
// sequentially (a 128-byte line serves all the entries that fall into it, ~20 here, instead of one) and adds the
// products into LDS with ds_add_f64. A block with many entries is cut into chunks of equal entry count, one wavefront
// each, whose partial sums a second small kernel adds in chunk order. One wavefront per accumulator set and in-order
// LDS atomics: a row's terms are added one by one in column order, a column's in row order, whatever the launch.
#include <cstdlib>
#include <cstring>

#include "fe_internal.hpp"
#include "re_lbfgs_compact.hpp"
#include "../../include/gdmix_fe.h"

#include <memory>
#include <new>
#include <vector>

namespace gdmix {

// theta_j of the coefficient whose solver variable is xj: phi_j with a prior installed (W.x holds phi then), itself otherwise
template <bool PRIOR>
__device__ __forceinline__ double fe_theta_of(const FeDev& F, int64_t j, double xj) {
  return PRIOR ? __builtin_fma(F.sc[j], xj, F.mu[j]) : xj;      // one rounding, the same at every site
}

template <bool PRIOR = false>
__global__ void fe_prepare_kernel(FeDev F) {
  for (int j = blockIdx.x * blockDim.x + threadIdx.x; j < F.d; j += gridDim.x * blockDim.x) {
    const int64_t g = F.umap[j];
    F.xl[j] = fe_theta_of<PRIOR>(F, g, F.W.x[g]);
  }
}

// ---- the data term's VALUE, added up error-free (round 6) ----------------------------------------------------------------------------
// The value of a shard is a sum of millions of losses: f ~ 5e5 has an ulp of 5.8e-11, and a line search near the optimum asks for
// decreases of that size (tools/fuzz_fe.py case 6100134: five features, 726 k samples, expected decrease of the fifth iteration
// ~ 1.4 ulp). Added over a tree of fp64 sums the value carries a few ulps of noise, every trial of the search fails the
// sufficient-decrease test and the fit ends ABNORMAL where scipy on an accurately summed objective (and the oracle, which adds in
// long double) takes the step and stops on the projected gradient. So the value is added up as (hi, lo) pairs combined with TwoSum
// at EVERY level — a lane's rows, the unit's wavefront, the ranges of fe_finish_kernel, its wavefronts, the final 64 — and rounded
// once at the end: f is the correctly rounded sum of the fp64 loss terms (first version: from the per-unit sums up only; case
// 6500120, 294 k samples, still searched two evaluations longer than the oracle on the per-unit sums' noise). Six more flops per row in
// passes whose vector units idle 90 % of the time; the gradient is not touched.
__device__ __forceinline__ void dd_add(double& hi, double& lo, double x) {      // (hi, lo) += x, Knuth's TwoSum: no error term lost
  const double s = hi + x, bb = s - hi;
  lo += (hi - (s - bb)) + (x - bb);
  hi = s;
}
__device__ __forceinline__ void dd_add2(double& hi, double& lo, double xh, double xl) { dd_add(hi, lo, xh); lo += xl; }
// (hi, lo) of all 64 lanes -> lane 63 holds the total pair (the shift pattern of wave_sum; an invalid source reads 0)
__device__ __forceinline__ void wave_sum_dd(double& hi, double& lo) {
#define GDMIX_DD_STEP(CTRL, MASK)                                                     \
  {                                                                                   \
    const double oh = dpp_get0<CTRL, MASK>(hi), ol = dpp_get0<CTRL, MASK>(lo);        \
    dd_add2(hi, lo, oh, ol);                                                          \
  }
  GDMIX_DD_STEP(0x111, 0xf) GDMIX_DD_STEP(0x112, 0xf) GDMIX_DD_STEP(0x114, 0xf) GDMIX_DD_STEP(0x118, 0xf) GDMIX_DD_STEP(0x142, 0xa) GDMIX_DD_STEP(0x143, 0xc)
#undef GDMIX_DD_STEP
  hi = readlane63(hi);
  lo = readlane63(lo);
}

// what becomes of a finished row sum
// HESS: the pass computes the diagonal of X~' D X~ instead of the gradient (fixed_effect_lr_lbfgs_model.py:271-296): the row pass
// leaves d_i = w_i rho_i (1 - rho_i), rho = sigmoid(logit), the column pass sums val^2 d_i
template <bool HESS>
__device__ __forceinline__ void fe_emit_row(const FeDev& F, const SolveParams& o, int s, double sum, double xb, double& loss, double& loss_lo, double& rsum) {
  const double zi = sum + xb + (double)F.o[s];
  const double yi = (double)F.y[s];
  const double wi = F.w ? (double)F.w[s] : 1.0;
  double ri;
  // The test stays "Poisson, else non-zero, else logistic": it is sound because every entry point refuses a code outside the three
  // (loss_code_ok), and spelling it == LOSS_SQUARED moves the code of the scatter and row kernels.
  if (HESS && o.loss == LOSS_POISSON) {
    ri = wi * exp_any(zi);      // d_i = w_i exp(z_i) (include/gdmix_fe.h, "poisson")
  } else if (HESS) {
    const double rho = sigmoid_full(zi);
    ri = wi * rho * (1.0 - rho);
  } else if (o.loss == LOSS_POISSON) {
    dd_add(loss, loss_lo, poisson_terms(zi, yi, wi, ri));
  } else if (o.loss) {
    const double e = zi - yi;
    dd_add(loss, loss_lo, wi * e * e);
    ri = 2.0 * wi * e;
  } else {
    dd_add(loss, loss_lo, logistic_terms(zi, yi, wi, ri));
  }
  F.rs[s] = ri;
  rsum += ri;
}

// The HV variant's emit (include/gdmix_fe.h, "(ABI 24) TRON"). A product: rs_i = D_i (x_i . d + d_b) with the curvature weights the
// evaluation of the accepted point left, no loss term. An evaluation: the residual and loss of fe_emit_row<false>, and next to them the
// curvature weight of this point — w rho (1 - rho), 2 w or w exp(z) — for the products that follow if the point is accepted.
__device__ __forceinline__ void fe_emit_row_hv(const FeDev& F, const SolveParams& o, int mode, double* __restrict__ cw, int s, double sum, double xb,
                                               double& loss, double& loss_lo, double& rsum) {
  double ri;
  if (mode & 1) {
    ri = cw[s] * (sum + xb);
  } else {
    const double zi = sum + xb + (double)F.o[s];
    const double yi = (double)F.y[s];
    const double wi = F.w ? (double)F.w[s] : 1.0;
    double ci;
    if (o.loss == LOSS_POISSON) {
      dd_add(loss, loss_lo, poisson_terms(zi, yi, wi, ri));
      ci = wi * exp_any(zi);
    } else if (o.loss) {
      const double e = zi - yi;
      dd_add(loss, loss_lo, wi * e * e);
      ri = 2.0 * wi * e;
      ci = 2.0 * wi;
    } else {
      dd_add(loss, loss_lo, logistic_terms(zi, yi, wi, ri));
      const double rho = sigmoid_full(zi);
      ci = wi * rho * (1.0 - rho);
    }
    cw[s] = ci;
  }
  F.rs[s] = ri;
  rsum += ri;
}

// what the HV variant of a row kernel reads at entry (uniform): the mode, the gathered vector, the intercept's entry, the curvature array
struct FeHvEntry { int mode; bool run; const double* vec; double xb; double* cw; };
__device__ __forceinline__ FeHvEntry fe_hv_entry(const FeDev& F) {
  const FeTron T = fe_tron_of(F);
  FeHvEntry e;
  e.mode = T.st->mode;
  e.run = e.mode >= FE_TM_CURVATURE || F.state->status < 0;      // the stop flag makes the solver's own pass pairs no-ops
  e.vec = (e.mode & 1) ? T.vl : F.xl;
  const bool second = (e.mode == FE_TM_PRODUCT) == (T.st->cur != 0);      // c[cur] for the solver's product, c[1 - cur] otherwise
  e.cw = second ? T.c[1] : T.c[0];      // (a select, not an index: an array indexed at run time lives in scratch)
  e.xb = 0.0;
  if (F.ic) e.xb = e.mode == FE_TM_EVAL ? T.xt[F.D] : e.mode == FE_TM_PRODUCT ? T.d[F.D] : e.mode == FE_TM_CURVATURE ? F.W.x[F.D] : T.st->vb;
  return e;
}

// acc[loc] += term, in LDS, nothing returned
__device__ __forceinline__ void lds_add(double* acc, int loc, double term) {
  __hip_atomic_fetch_add(acc + loc, term, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}

// inclusive prefix sums over the 64 lanes of two 16-bit counters packed in one word (no carry between the halves: sums < 65 536)
__device__ __forceinline__ unsigned wave_iscan_pair(unsigned v) {
  v += (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0x111, 0xf, 0xf, false);   // row_shr:1 (lanes without a source keep 0)
  v += (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0x112, 0xf, 0xf, false);   // row_shr:2
  v += (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0x114, 0xf, 0xf, false);   // row_shr:4
  v += (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0x118, 0xf, 0xf, false);   // row_shr:8: prefix within each row of 16
  v += (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0x142, 0xa, 0xf, false);   // row_bcast:15 into rows 1, 3
  v += (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0x143, 0xc, 0xf, false);   // row_bcast:31 into rows 2, 3
  return v;
}


// One unit in the 6-byte form. Trip t: lane l holds entries q * 64 + l, q = 0..7 — every gather instruction covers 64 consecutive
// entries (~100 consecutive elements of the gathered vector), and the adds of one accumulator happen in exact key order.
template <bool ROWS, bool HESS>
__device__ __forceinline__ void fe_scatter_compressed(double* acc, const unsigned char* __restrict__ base, int trips, const double* __restrict__ vec, int lane) {
  int key0 = 0;     // key of the entry before this trip's first, relative to the unit's first (uniform)
  for (int t = 0; t < trips; ++t) {
    const unsigned char* tp = base + (size_t)t * FE_CTRIP_BYTES;
    uint4 v0, v1, ix;
    __builtin_memcpy(&v0, tp + lane * 16, 16);
    __builtin_memcpy(&v1, tp + 1024 + lane * 16, 16);
    __builtin_memcpy(&ix, tp + 2048 + lane * 16, 16);
    const unsigned w[4] = {ix.x, ix.y, ix.z, ix.w};
    const float vq[8] = {__uint_as_float(v0.x), __uint_as_float(v0.y), __uint_as_float(v0.z), __uint_as_float(v0.w),
                         __uint_as_float(v1.x), __uint_as_float(v1.y), __uint_as_float(v1.z), __uint_as_float(v1.w)};
    int kq[8], lq[8];
    double xq[8];
#pragma unroll
    for (int h = 0; h < 4; ++h) {
      const unsigned pre = wave_iscan_pair((w[h] >> FE_LOC_BITS) & 0x001f001fu);      // rows 2h (low half) and 2h + 1 (high half)
      const unsigned tot = (unsigned)__builtin_amdgcn_readlane((int)pre, 63);
      kq[2 * h] = key0 + (int)(pre & 0xffffu);
      key0 += (int)(tot & 0xffffu);
      kq[2 * h + 1] = key0 + (int)(pre >> 16);
      key0 += (int)(tot >> 16);
      lq[2 * h] = (int)(w[h] & ((1u << FE_LOC_BITS) - 1));
      lq[2 * h + 1] = (int)((w[h] >> 16) & ((1u << FE_LOC_BITS) - 1));
    }
#pragma unroll
    for (int q = 0; q < 8; ++q) xq[q] = vec[kq[q]];
#pragma unroll
    for (int q = 0; q < 8; ++q) {
      const double v = (double)vq[q];
      // a filler (value 0: it only carries a key delta too large for five bits) must not turn a non-finite x into a NaN sum
      lds_add(acc, lq[q], vq[q] == 0.0f ? 0.0 : ((HESS && !ROWS) ? v * v * xq[q] : v * xq[q]));
    }
  }
}

// HV (include/gdmix_fe.h, "(ABI 24) TRON"): the row pass of a TRON problem — an evaluation or a Hessian-vector product, whichever the
// record says (fe_hv_entry); the column pass behind a product of gdmix_fe_hessian_vec, which runs whatever the status.
template <bool ROWS, bool HESS, bool PACKED, bool PRIOR = false, bool HV = false>
__global__ __launch_bounds__(WAVE) void fe_scatter_kernel(FeDev F, SolveParams o) {
  static_assert(ROWS || !PRIOR, "the column pass gathers residuals: it has no prior variant");
  static_assert(!HV || (!HESS && !PRIOR), "the product has no Hessian-diagonal and no prior variant");
  // exactly 16 KiB: ten wavefronts per CU (160 KiB of LDS). Round 5: a spare accumulator for the lanes beyond the end of the last
  // trip made it 16 400 B = nine; those lanes now add 0.0 to accumulator 0 (x + 0.0 == x bit for bit; an accumulator that is still
  // -0.0 cannot occur: they start at +0.0). Measured: nine or ten makes no difference (0.556 ms either way, three runs each):
  // the passes are bound by the CU's vector-memory path, not by occupancy (docs/rounds/r05.md)
  __shared__ double acc[FE_B];
  const int lane = threadIdx.x;
  const FeCopy& C = ROWS ? F.rc : F.cc;
  const int u = C.order[blockIdx.x];
  if (u < 0) return;
  if (!HESS && !HV && F.state->status >= 0) return;   // the driver has stopped: evaluations enqueued ahead of the status are no-ops
  FeHvEntry hv{};
  if constexpr (HV && ROWS) {
    hv = fe_hv_entry(F);
    if (!hv.run) return;
  }
  const int k0 = C.ustart[u], k1 = C.ustart[u + 1], b = C.ublock[u];
  const int kb = PACKED ? C.kbase[u] : 0;
  const bool whole = ROWS && (C.ufirst[b + 1] - C.ufirst[b] == 1);
  const double xb = (HV && ROWS) ? hv.xb : (ROWS && F.ic) ? fe_theta_of<PRIOR>(F, F.D, F.W.x[F.D]) : 0.0;
  const double* __restrict__ gathered = (HV && ROWS) ? hv.vec : (ROWS ? F.xl : F.rs);
  const uint2* __restrict__ ent = C.ent;
  const int32_t* __restrict__ key = C.key;
  const float* __restrict__ val = C.val;
  const uint16_t* __restrict__ loc = C.loc;
  const double* __restrict__ vec = gathered + kb;
#pragma unroll
  for (int i = 0; i < FE_B / WAVE; i += 2) *reinterpret_cast<double2*>(acc + (i * WAVE + 2 * lane)) = make_double2(0.0, 0.0);
  const int64_t cb = C.cbase ? C.cbase[u] : -1;      // uniform
  if (cb >= 0) {
    fe_scatter_compressed<ROWS, HESS>(acc, C.cdata + cb, C.ctrip[u], gathered + C.kbase[u], lane);   // (keys are relative to the unit's first in this form, always)
  } else {
  // full trips without a guard in sight (a load under a branch is waited for inside the branch); the last, partial trip
  // reads clamped addresses and sends what is beyond the end to a spare accumulator.
  // (Round 5, measured and removed: the entry stream two trips ahead of the gathers — prefetch issued BEHIND the gathers so that
  // the in-order return of loads does not make the gathers wait for it, two register sets, clean ISA: row pass 0.232 -> 0.262 ms,
  // column pass 0.247 -> 0.255. More bytes in flight per wavefront make this stream slower, not faster: docs/rounds/r05.md.)
  int base = k0;
  for (; base + WAVE * FE_U <= k1; base += WAVE * FE_U) {
    int kq[FE_U], lq[FE_U];
    float vq[FE_U];
    double xq[FE_U];
#pragma unroll
    for (int q = 0; q < FE_U; ++q) {
      const int k = base + q * WAVE + lane;
      if (PACKED) {
        // two consecutive entries per lane and 16-byte load; the adds keep entry order within a pair, pairs in lane order
        if ((q & 1) == 0) {
          uint4 e2;
          __builtin_memcpy(&e2, ent + (base + (q >> 1) * 2 * WAVE + 2 * lane), 16);
          kq[q] = (int)(e2.x >> FE_LOC_BITS); lq[q] = (int)(e2.x & ((1u << FE_LOC_BITS) - 1)); vq[q] = __uint_as_float(e2.y);
          kq[q + 1] = (int)(e2.z >> FE_LOC_BITS); lq[q + 1] = (int)(e2.z & ((1u << FE_LOC_BITS) - 1)); vq[q + 1] = __uint_as_float(e2.w);
        }
      } else {
        kq[q] = key[k];
        vq[q] = val[k];
        lq[q] = (int)loc[k];
      }
    }
#pragma unroll
    for (int q = 0; q < FE_U; ++q) xq[q] = vec[kq[q]];
#pragma unroll
    for (int q = 0; q < FE_U; ++q) {
      const double v = (double)vq[q];
      lds_add(acc, lq[q], (HESS && !ROWS) ? v * v * xq[q] : v * xq[q]);
    }
  }
  if (base < k1) {
    int kq[FE_U], lq[FE_U];
    float vq[FE_U];
    double xq[FE_U];
    unsigned live = 0u;
#pragma unroll
    for (int q = 0; q < FE_U; ++q) {
      const int k = base + q * WAVE + lane;
      const int kc = k < k1 ? k : k1 - 1;
      int l;
      if (PACKED) {
        const uint2 e = ent[kc];
        kq[q] = (int)(e.x >> FE_LOC_BITS);
        l = (int)(e.x & ((1u << FE_LOC_BITS) - 1));
        vq[q] = __uint_as_float(e.y);
      } else {
        kq[q] = key[kc];
        vq[q] = val[kc];
        l = (int)loc[kc];
      }
      lq[q] = k < k1 ? l : 0;
      live |= (k < k1 ? 1u : 0u) << q;
    }
#pragma unroll
    for (int q = 0; q < FE_U; ++q) xq[q] = vec[kq[q]];
#pragma unroll
    for (int q = 0; q < FE_U; ++q) {
      const double v = (double)vq[q];
      const double term = (HESS && !ROWS) ? v * v * xq[q] : v * xq[q];
      lds_add(acc, lq[q], ((live >> q) & 1u) ? term : 0.0);
    }
  }
  }   // (the 8-byte / three-array forms)
  __builtin_amdgcn_s_waitcnt(0xc07f);   // lgkmcnt(0): the adds have landed
  __builtin_amdgcn_wave_barrier();
  if (whole) {
    double loss = 0.0, loss_lo = 0.0, rsum = 0.0;
    const int r0 = b * FE_B;
    const int nr = (F.n - r0 < FE_B) ? F.n - r0 : FE_B;
    for (int i = lane; i < nr; i += WAVE) {
      if constexpr (HV) fe_emit_row_hv(F, o, hv.mode, hv.cw, r0 + i, acc[i], xb, loss, loss_lo, rsum);
      else fe_emit_row<HESS>(F, o, r0 + i, acc[i], xb, loss, loss_lo, rsum);
    }
    wave_sum_dd(loss, loss_lo);
    rsum = wave_sum(rsum);
    if (lane == 0) { F.loss_part[u] = loss; F.loss_lo_part[u] = loss_lo; F.rsum_part[u] = rsum; }
  } else {
    double* __restrict__ out = C.part + (size_t)u * FE_B;
#pragma unroll
    for (int i = 0; i < FE_B / WAVE; i += 2)
      *reinterpret_cast<double2*>(out + (i * WAVE + 2 * lane)) = *reinterpret_cast<const double2*>(acc + (i * WAVE + 2 * lane));
    if (ROWS && lane == 0) { F.loss_part[u] = 0.0; F.loss_lo_part[u] = 0.0; F.rsum_part[u] = 0.0; }
  }
}

// Partial sums of one output over the units [u0, u1) of its block. A frequent feature's block can have a thousand units: FE_STRANDS
// threads take every FE_STRANDS-th unit each (several loads in flight), then thread 0 of the output adds the strands in order.
// Fixed shape; with a single unit the result is that unit's value exactly.
constexpr int FE_STRANDS = 16;
constexpr int FE_RED_OUT = FE_THREADS / FE_STRANDS;   // outputs per workgroup; consecutive, so their loads share a line
static_assert(FE_B % FE_RED_OUT == 0, "a workgroup's outputs lie in one block");

__device__ __forceinline__ double fe_strand_sum(const double* __restrict__ part, int u0, int u1, int i, int strand, double (*lds)[FE_RED_OUT],
                                                int out) {
  double t = 0.0;
  int u = u0 + strand;
  for (; u + 3 * FE_STRANDS < u1; u += 4 * FE_STRANDS) {
    const double a0 = part[(size_t)u * FE_B + i], a1 = part[(size_t)(u + FE_STRANDS) * FE_B + i];
    const double a2 = part[(size_t)(u + 2 * FE_STRANDS) * FE_B + i], a3 = part[(size_t)(u + 3 * FE_STRANDS) * FE_B + i];
    t += a0; t += a1; t += a2; t += a3;
  }
  for (; u < u1; u += FE_STRANDS) t += part[(size_t)u * FE_B + i];
  lds[strand][out] = t;
  __syncthreads();
  double g = 0.0;
  if (strand == 0) {
    g = lds[0][out];
#pragma unroll
    for (int k = 1; k < FE_STRANDS; ++k) g += lds[k][out];
  }
  return g;
}

// rows of the blocks that were cut into several units
constexpr int FE_FIX_PER_BLOCK = FE_B / FE_RED_OUT;   // workgroups of fe_rows_fix_kernel per block
template <bool HESS = false, bool PRIOR = false, bool HV = false>
__global__ __launch_bounds__(FE_THREADS) void fe_rows_fix_kernel(FeDev F, SolveParams o) {
  __shared__ double lds[FE_STRANDS][FE_RED_OUT];
  if (!HESS && !HV && F.state->status >= 0) return;
  FeHvEntry hv{};
  if constexpr (HV) {
    hv = fe_hv_entry(F);
    if (!hv.run) return;      // (uniform over the grid)
  }
  const int tid = threadIdx.x, out = tid % FE_RED_OUT, strand = tid / FE_RED_OUT;
  const int b = F.multi[blockIdx.x / FE_FIX_PER_BLOCK];
  const int i = (blockIdx.x % FE_FIX_PER_BLOCK) * FE_RED_OUT + out;
  const int row = b * FE_B + i;
  const double xb = HV ? hv.xb : F.ic ? fe_theta_of<PRIOR>(F, F.D, F.W.x[F.D]) : 0.0;
  const double t = fe_strand_sum(F.rc.part, F.rc.ufirst[b], F.rc.ufirst[b + 1], i, strand, lds, out);
  double loss = 0.0, loss_lo = 0.0, rsum = 0.0;
  if (strand == 0 && row < F.n) {
    if constexpr (HV) fe_emit_row_hv(F, o, hv.mode, hv.cw, row, t, xb, loss, loss_lo, rsum);
    else fe_emit_row<HESS>(F, o, row, t, xb, loss, loss_lo, rsum);
  }
  if (tid < WAVE) {   // the outputs' threads are the first FE_RED_OUT lanes of wavefront 0
    wave_sum_dd(loss, loss_lo);
    rsum = wave_sum(rsum);
    if (tid == 0) {
      F.loss_part[F.rc.nunit + blockIdx.x] = loss;
      F.loss_lo_part[F.rc.nunit + blockIdx.x] = loss_lo;
      F.rsum_part[F.rc.nunit + blockIdx.x] = rsum;
    }
  }
}

// ---- frequent columns: FE_HOT_REP accumulators each (fe_internal.hpp: FeHot) -------------------------------------------------------------
// next to fe_finish_kernel's own workgroups (which find 0 for a frequent column — the copy holds no entry under its own number — and
// write nothing then: the buffer is clear before an evaluation). One workgroup per
// frequent column: replica r's sum over the virtual block's units by 8 strands, strands in order, then the replicas in order.
// (Round 6: the workgroups of this step are the FIRST F.hot.n workgroups of fe_finish_kernel's grid, not a launch of their own — one
// launch boundary (~6 us on this device) and 10 us of a nearly empty device less per evaluation of a shard with frequent columns.)
__device__ __forceinline__ void fe_hot_finish_block(const FeDev& F, int h) {
  constexpr int STR = FE_THREADS / FE_HOT_REP;
  __shared__ double lds[STR][FE_HOT_REP];
  __shared__ double rep[FE_HOT_REP];
  const FeHot& H = F.hot;
  const int tid = threadIdx.x, r = tid % FE_HOT_REP, strand = tid / FE_HOT_REP;
  const int b = H.vbase / FE_B, i = h * FE_HOT_REP + r;
  const int u0 = F.cc.ufirst[b], u1 = F.cc.ufirst[b + 1];
  const double* __restrict__ part = F.cc.part;
  double t = 0.0;
  int u = u0 + strand;
  for (; u + 3 * STR < u1; u += 4 * STR) {
    const double a0 = part[(size_t)u * FE_B + i], a1 = part[(size_t)(u + STR) * FE_B + i];
    const double a2 = part[(size_t)(u + 2 * STR) * FE_B + i], a3 = part[(size_t)(u + 3 * STR) * FE_B + i];
    t += a0; t += a1; t += a2; t += a3;
  }
  for (; u < u1; u += STR) t += part[(size_t)u * FE_B + i];
  lds[strand][r] = t;
  __syncthreads();
  if (strand == 0) {
    double g = lds[0][r];
#pragma unroll
    for (int k = 1; k < STR; ++k) g += lds[k][r];
    rep[r] = g;
  }
  __syncthreads();
  if (tid == 0) {
    double g = rep[0];
#pragma unroll
    for (int k = 1; k < FE_HOT_REP; ++k) g += rep[k];
    F.fg[F.umap[H.col[h]]] = g;
  }
}

// local gradient (the column blocks' partial sums) into the global coefficient space; the first FE_FIN_BLOCKS workgroups also add
// up a contiguous range of the per-unit value / residual sums each
template <bool HESS = false>
__global__ __launch_bounds__(FE_THREADS) void fe_finish_kernel(FeDev F) {
  __shared__ double lds[FE_STRANDS][FE_RED_OUT];
  __shared__ double red[3][FE_WAVES];
  if (!HESS && F.state->status >= 0) return;
  // the frequent columns' workgroups come FIRST in the grid: each is a long chain (a thousand units' sums by eight strands) and must
  // start with the launch, not behind it
  if ((int)blockIdx.x < F.hot.n) { fe_hot_finish_block(F, (int)blockIdx.x); return; }
  const int bid = (int)blockIdx.x - F.hot.n;
  const int tid = threadIdx.x, out = tid % FE_RED_OUT, strand = tid / FE_RED_OUT;
  const int j0 = bid * FE_RED_OUT;
  if (j0 < F.d) {   // workgroup-uniform
    const int jj = j0 + out < F.d ? j0 + out : F.d - 1;
    const int b = jj / FE_B, i = jj % FE_B;
    const double g = fe_strand_sum(F.cc.part, F.cc.ufirst[b], F.cc.ufirst[b + 1], i, strand, lds, out);
    // (an exact 0 is not written: the buffer is clear before an evaluation — gdmix_fe_eval / the step's dots — and a frequent column's
    // own slot, which holds no entry here, belongs to the workgroup that adds up its replicas in this same launch)
    if (strand == 0 && j0 + out < F.d && g != 0.0) F.fg[F.umap[jj]] = g;
  }
  if (bid >= FE_FIN_BLOCKS) return;
  const int lane = tid & (WAVE - 1), wv = tid >> 6;
  const int chunk = (F.nred + FE_FIN_BLOCKS - 1) / FE_FIN_BLOCKS;
  const int b0 = bid * chunk;
  const int b1 = (b0 + chunk < F.nred) ? b0 + chunk : F.nred;
  double a = 0.0, al = 0.0, r = 0.0;
  for (int b = b0 + tid; b < b1; b += FE_THREADS) {
    dd_add2(a, al, F.loss_part[b], F.loss_lo_part[b]);
    r += F.rsum_part[b];
  }
  wave_sum_dd(a, al);
  r = wave_sum(r);
  if (lane == 0) { red[0][wv] = a; red[1][wv] = r; red[2][wv] = al; }
  __syncthreads();
  __shared__ int last;
  if (tid == 0) {
    double sa = red[0][0], sl = red[2][0], sr = red[1][0];
#pragma unroll
    for (int w = 1; w < FE_WAVES; ++w) { dd_add2(sa, sl, red[0][w], red[2][w]); sr += red[1][w]; }
    st_x<true>(F.fin_part + 3 * bid, sa);
    st_x<true>(F.fin_part + 3 * bid + 1, sr);
    st_x<true>(F.fin_part + 3 * bid + 2, sl);
    __threadfence();
    last = atomicAdd(F.fin_count, 1u) == FE_FIN_BLOCKS - 1;
  }
  __syncthreads();
  // the workgroup that finishes last adds the FE_FIN_BLOCKS range sums (in lane order, whichever workgroup it is) -> data value and
  // intercept gradient (HESS: fg[D] = sum_i d_i, the intercept's entry; fg[P] unused)
  if (last && tid < WAVE) {
    __threadfence();
    double a = tid < FE_FIN_BLOCKS ? ld_x<true>(F.fin_part + 3 * tid) : 0.0, al = tid < FE_FIN_BLOCKS ? ld_x<true>(F.fin_part + 3 * tid + 2) : 0.0;
    wave_sum_dd(a, al);
    const double r = wave_sum(tid < FE_FIN_BLOCKS ? ld_x<true>(F.fin_part + 3 * tid + 1) : 0.0);
    if (tid == 0) {
      if (F.ic) F.fg[F.D] = r;
      F.fg[F.P] = a + al;      // rounded once
      *F.fin_count = 0u;
    }
  }
}

// g = reduced data gradient + regulariser, and every product the driver needs (re_lbfgs_compact.hpp acc[] layout): the share of
// "virtual block" vb of nvb — coefficients (vb * 256 + tid) + k * nvb * 256 — into acc_part[vb]. The partition is a function of P
// alone (nvb = min(ceil(P / 256), FE_DOT_BLOCKS)), not of the launch: fe_dots_kernel runs one workgroup per virtual block,
// fe_tail_kernel deals them over fewer resident workgroups, and both give the same bits.
// the reduced data gradient of coefficient j in the solver's variable: with a prior, grad_phi = s (.) grad_theta. The product is rounded on
// its own — not fused into the sum with the regulariser behind it — so that a neutral prior (s = 1) leaves the bits of the plain path.
__device__ __forceinline__ double fe_mul_rounded(double a, double b) {
#pragma clang fp contract(off)
  return a * b;
}

template <bool SC1 = false, bool PRIOR = false>
__device__ __forceinline__ void fe_dots_block(const FeDev& F, const SolveParams& o, int vb, int nvb, double (*red)[COMPACT_KD]) {
  const int tid = threadIdx.x, lane = tid & (WAVE - 1), wv = tid >> 6;
  const int col = F.state->col, head = F.state->head, m = o.m, P = F.P;
  double acc[COMPACT_KD];   // ... and S'g, Y'g taken directly behind the TEAM_K products (re_lbfgs_compact.hpp: why)
#pragma unroll
  for (int k = 0; k < COMPACT_KD; ++k) acc[k] = 0.0;
  for (int j = vb * FE_THREADS + tid; j < P; j += nvb * FE_THREADS) {
    const bool reg = (j < F.D) || o.regularize_bias;   // the intercept is coefficient D
    const double xj = F.W.x[j];
    const double fj = PRIOR ? fe_mul_rounded(F.fg[j], F.sc[j]) : F.fg[j];
    const double gj = fj + (reg ? o.l2 * xj : 0.0);
    F.fg[j] = 0.0;   // consumed: the next evaluation starts from a clear buffer (gdmix_fe_eval)
    F.W.g[j] = gj;
    const double dj = F.W.d[j], rj = F.W.r[j];
    if (reg) acc[0] += xj * xj;
    acc[1] += gj * dj;
    acc[2] += gj * gj;
    const double yj = gj - rj;
    acc[3] += yj * yj;
    acc[4] += yj * gj;
    acc[TEAM_RD] += rj * dj;
    acc[TEAM_K - 1] = fmax(acc[TEAM_K - 1], fabs(gj));
    double2 h[TEAM_MCAP];   // all pairs requested before the first is used (see team_eval)
#pragma unroll
    for (int i = 0; i < TEAM_MCAP; ++i) {
      int sl = head + i;
      if (sl >= m) sl -= m;
      if (i >= m) sl = 0;
      h[i] = compact_hist(F.W, m, j)[sl * COMPACT_HIST_STRIDE];
    }
#pragma unroll
    for (int i = 0; i < TEAM_MCAP; ++i) {
      const double hx = i < col ? h[i].x : 0.0, hy = i < col ? h[i].y : 0.0;
      acc[5 + i] += hx * yj;
      acc[5 + TEAM_MCAP + i] += hy * yj;
      acc[TEAM_K + i] += hx * gj;
      acc[TEAM_K + TEAM_MCAP + i] += hy * gj;
    }
  }
  static_assert(COMPACT_KD <= WAVE, "one lane per value");
  double mine = 0.0;
#pragma unroll
  for (int k = 0; k < COMPACT_KD; ++k) {
    const double t = (k == TEAM_K - 1) ? wave_max_nonneg(acc[k]) : wave_sum(acc[k]);
    if (lane == k) mine = t;
  }
  if (lane < COMPACT_KD) red[wv][lane] = mine;
  __syncthreads();
  if (tid < COMPACT_KD) {
    double s = red[0][tid];
#pragma unroll
    for (int w = 1; w < FE_WAVES; ++w) s = (tid == TEAM_K - 1) ? fmax(s, red[w][tid]) : s + red[w][tid];
    st_x<SC1>(F.acc_part + (size_t)vb * COMPACT_KD + tid, s);   // SC1 (fe_tail_kernel): written through, read by another workgroup of the same launch
  }
}

template <bool PRIOR = false>
__global__ __launch_bounds__(FE_THREADS) void fe_dots_kernel(FeDev F, SolveParams o) {
  __shared__ double red[FE_WAVES][COMPACT_KD];
  if (F.state->status >= 0) return;     // a step enqueued behind the stop (gdmix_fe_step_async) is a no-op
  fe_dots_block<false, PRIOR>(F, o, blockIdx.x, gridDim.x, red);
}

// one workgroup: totals of the products (the virtual blocks' shares, in a fixed order), then the driver's decision
template <bool SC1 = false>
__device__ __forceinline__ void fe_step_body(const FeDev& F, const SolveParams& o, int dot_blocks, int32_t* status_out, double* tot /* LDS [COMPACT_KD] */,
                                             CompactMats& mats /* LDS */, double (*part4)[WAVE] /* LDS [4][64] */) {
  const int tid = threadIdx.x;
  {
    // value v of block b by thread (b % 4) * 64 + v, four partial totals per value, combined in order
    static_assert(FE_THREADS == 4 * WAVE && COMPACT_KD <= WAVE, "four groups of one lane per value");
    const int v = tid & (WAVE - 1), g = tid >> 6;
    if (v < COMPACT_KD) {
      double s = 0.0;
      int b = g;
      for (; b + 60 < dot_blocks; b += 64) {   // sixteen loads in flight (four groups take the blocks where eight did: the chain is twice as long)
        double t[16];
#pragma unroll
        for (int q = 0; q < 16; ++q) t[q] = ld_x<SC1>(F.acc_part + (size_t)(b + 4 * q) * COMPACT_KD + v);
#pragma unroll
        for (int q = 0; q < 16; ++q) s = (v == TEAM_K - 1) ? fmax(s, t[q]) : s + t[q];
      }
      for (; b + 28 < dot_blocks; b += 32) {   // eight
        double t[8];
#pragma unroll
        for (int q = 0; q < 8; ++q) t[q] = ld_x<SC1>(F.acc_part + (size_t)(b + 4 * q) * COMPACT_KD + v);
#pragma unroll
        for (int q = 0; q < 8; ++q) s = (v == TEAM_K - 1) ? fmax(s, t[q]) : s + t[q];
      }
      for (; b < dot_blocks; b += 4) {
        const double t = ld_x<SC1>(F.acc_part + (size_t)b * COMPACT_KD + v);
        s = (v == TEAM_K - 1) ? fmax(s, t) : s + t;
      }
      part4[g][v] = s;
    }
    __syncthreads();
    if (tid < COMPACT_KD) {
      double s = part4[0][tid];
#pragma unroll
      for (int k = 1; k < 4; ++k) s = (tid == TEAM_K - 1) ? fmax(s, part4[k][tid]) : s + part4[k][tid];
      tot[tid] = s;
    }
  }
  {
    const double* src = reinterpret_cast<const double*>(F.mats);
    double* dst = reinterpret_cast<double*>(&mats);
    for (int k = tid; k < (int)(sizeof(CompactMats) / sizeof(double)); k += FE_THREADS) dst[k] = src[k];
  }
  __syncthreads();
  double acc[COMPACT_KD];
#pragma unroll
  for (int k = 0; k < COMPACT_KD; ++k) acc[k] = tot[k];
  CompactState S = *F.state;
  CompactPlan plan;
  plan.action = CA_STOP; plan.col = S.col; plan.head = S.head; plan.stp = S.stp; plan.gamma = 1.0;
  const double f_new = F.fg[F.P] + 0.5 * o.l2 * acc[0];
  // The data term is a sum of non-negative losses: - infinity is the mark a worker whose step was ABORTED leaves in its value slot
  // (fe_tail_kernel's watchdog), and the all-reduce has carried it to every worker — all of them stop in the same evaluation, none
  // is left alone in a collective (fixed_effect.run_stepping_loop raises on every worker).
  if (F.fg[F.P] == -__builtin_inf()) S.status = GDMIX_RE_ST_ABORTED_PEER;
  else compact_advance(S, acc, f_new, o, mats, plan, true, acc + TEAM_K);
  __syncthreads();
  {
    double* dst = reinterpret_cast<double*>(F.mats);
    const double* src = reinterpret_cast<const double*>(&mats);
    for (int k = tid; k < (int)(sizeof(CompactMats) / sizeof(double)); k += FE_THREADS) st_x<SC1>(dst + k, src[k]);
  }
  if (tid == 0) {
    *F.state = S;        // (read by later launches only)
    if (SC1) {           // the plan is read by the other workgroups of this launch: word by word, written through
      static_assert(sizeof(CompactPlan) % 4 == 0, "plan copied as 32-bit words");
      const unsigned* src = reinterpret_cast<const unsigned*>(&plan);
      unsigned* dst = reinterpret_cast<unsigned*>(F.plan);
      for (int k = 0; k < (int)(sizeof(CompactPlan) / 4); ++k) __hip_atomic_store(dst + k, src[k], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    } else {
      *F.plan = plan;
    }
    *status_out = (plan.action == CA_STOP || plan.action == CA_STOP_RESTORE) ? S.status : -1;
  }
}

__global__ __launch_bounds__(FE_THREADS) void fe_step_kernel(FeDev F, SolveParams o, int dot_blocks, int32_t* status_out) {
  __shared__ double tot[COMPACT_KD];
  __shared__ CompactMats mats;
  __shared__ double part4[4][WAVE];
  if (F.state->status >= 0) return;     // (status_out keeps the status of the stop; fe_update_kernel repeats the stop's plan: idempotent)
  fe_step_body(F, o, dot_blocks, status_out, tot, mats, part4);
}

// the elementwise part of a step for coefficient j; the shard's copy of x in local order follows it (the row pass gathers from xl)
template <bool PRIOR = false>
__device__ __forceinline__ void fe_update_one(const FeDev& F, const CompactPlan& plan, const CompactMats& mats, int m, int j) {
  if (plan.action == CA_STOP_RESTORE) F.W.x[j] = F.W.t[j];
  else compact_update(plan, mats, F.W, F.P, m, j);
  const int jl = F.inv[j];
  if (jl >= 0) F.xl[jl] = fe_theta_of<PRIOR>(F, j, F.W.x[j]);
}

// ---- the whole step in ONE launch (round 5) ----------------------------------------------------------------------------------------
// dots -> decision -> update were three launches (9.4 + 8.4 + 5.9 us and two boundaries) plus fe_prepare_kernel ahead of the next
// evaluation. Here: at most one workgroup per CU (all resident: the wait below cannot starve anyone), each takes its virtual blocks'
// share of the products; the workgroup that arrives last adds the shares up in the fixed order and takes the driver's decision;
// the others wait for its generation stamp, then every workgroup updates the coefficients of its own virtual blocks — the ones
// whose gradient it wrote itself, so the only data crossing workgroups are the shares (to the last arriver) and state / plan / the
// m x m matrices (back). Hand-off per MI355X_MICROARCH.md: plain stores, one lane's agent-scope release + drained store queue,
// relaxed agent atomics for ticket and stamp, one lane's agent-scope acquire, workgroup barrier, plain loads.
// A stopped problem (status >= 0 from an earlier launch) makes this and every pass kernel return at once: the host may enqueue
// evaluations ahead of the status it has read (gdmix_fe_step_async).

template <bool PRIOR = false>
__global__ __launch_bounds__(FE_THREADS) void fe_tail_kernel(FeDev F, SolveParams o, int dot_blocks, int32_t* status_out, unsigned seq) {
  __shared__ double red[FE_WAVES][COMPACT_KD];
  __shared__ double tot[COMPACT_KD];
  __shared__ CompactMats mats;
  __shared__ double part4[4][WAVE];
  __shared__ CompactPlan plan_s;
  __shared__ int last, timed_out;
  if (F.state->status >= 0) return;     // written by an earlier launch: uniform over the grid
  if (threadIdx.x == 0) timed_out = 0;
  const int tid = threadIdx.x;
  for (int vb = blockIdx.x; vb < dot_blocks; vb += gridDim.x) {
    fe_dots_block<true, PRIOR>(F, o, vb, dot_blocks, red);
    __syncthreads();                     // red is reused
  }
  // What crosses workgroups inside this launch — the shares, then plan and matrices — is written with write-through (sc1) stores
  // and read with sc1 loads, so the hand-off needs a drained store queue and the counters only: no L2 write-back, no L1 invalidate
  // (MI355X_MICROARCH.md, "valid forms": sc1 stores and loads on both sides). The first version used plain accesses with an
  // agent-scope release / acquire pair on either side of both hand-offs: the kernel took 36 - 45 us for 24 us of work
  // (profiles/r05_fe_counters.txt).
  if (tid == 0) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    last = __hip_atomic_fetch_add(&F.sync->arrive, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == gridDim.x - 1;
  }
  __syncthreads();                       // (the shares are stored by threads of wavefront 0, whose queue thread 0 has just drained)
  if (last) {
    fe_step_body<true>(F, o, dot_blocks, status_out, tot, mats, part4);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");      // every wavefront: its part of the matrices is at the memory side
    __syncthreads();
    if (tid == 0) {
      // a waiter of this launch gave up before this workgroup arrived: its ABORTED must survive the state / status this
      // workgroup has just written — the coefficients of the workgroups that left are not updated, the fit is invalid
      if (__hip_atomic_load(&F.sync->aborted, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0u) {
        __hip_atomic_store(reinterpret_cast<int*>(&F.state->status), GDMIX_RE_ST_ABORTED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_store(status_out, (int32_t)GDMIX_RE_ST_ABORTED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      }
      __hip_atomic_store(&F.sync->arrive, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      __hip_atomic_store(&F.sync->gen, seq, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
  }
  if (tid == 0) {
    if (!last) {
      // bounded: a workgroup of this launch that never arrives (it cannot happen while at most one workgroup per CU is launched on an
      // otherwise progressing device) must not hang the GPU — after ~4 s the problem is marked ABORTED, which also stops every later launch
      unsigned spins = 0;
      uint64_t t0 = 0;
      while (__hip_atomic_load(&F.sync->gen, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != seq) {
        __builtin_amdgcn_s_sleep(2);
        if ((++spins & 1023u) == 0) {
          const uint64_t now = wall_clock64();
          if (t0 == 0) t0 = now;
          else if (now - t0 > 400000000ull) {   // 4 s at 100 MHz
            __hip_atomic_store(&F.sync->aborted, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);      // first: the last arriver reads it
            F.fg[F.P] = -__builtin_inf();      // what this worker contributes to the next all-reduce: every worker stops (fe_step_body)
            __hip_atomic_store(reinterpret_cast<int*>(&F.state->status), GDMIX_RE_ST_ABORTED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __hip_atomic_store(status_out, (int32_t)GDMIX_RE_ST_ABORTED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            timed_out = 1;
            break;
          }
        }
      }
    }
    const unsigned* src = reinterpret_cast<const unsigned*>(F.plan);
    unsigned* dst = reinterpret_cast<unsigned*>(&plan_s);
    for (int k = 0; k < (int)(sizeof(CompactPlan) / 4); ++k) dst[k] = __hip_atomic_load(src + k, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  __syncthreads();
  if (timed_out) return;
  if (!last) {
    const double* src = reinterpret_cast<const double*>(F.mats);
    double* dst = reinterpret_cast<double*>(&mats);
    for (int k = tid; k < (int)(sizeof(CompactMats) / sizeof(double)); k += FE_THREADS) dst[k] = ld_x<true>(src + k);
    __syncthreads();
  }
  const CompactPlan plan = plan_s;
  if (plan.action == CA_STOP) return;
  for (int vb = blockIdx.x; vb < dot_blocks; vb += gridDim.x)
    for (int j = vb * FE_THREADS + tid; j < F.P; j += dot_blocks * FE_THREADS) fe_update_one<PRIOR>(F, plan, mats, o.m, j);
}

template <bool PRIOR = false>
__global__ void fe_update_kernel(FeDev F, int m) {
  const CompactPlan plan = *F.plan;
  if (plan.action == CA_STOP) return;
  for (int j = blockIdx.x * blockDim.x + threadIdx.x; j < F.P; j += gridDim.x * blockDim.x) fe_update_one<PRIOR>(F, plan, *F.mats, m, j);
}

// the start point in the solver's variable: theta0 itself, or with a prior phi0 = (theta0 - mu) / s (theta0 NULL: phi0 = 0, theta = mu)
template <bool PRIOR>
__device__ __forceinline__ double fe_start_of(const FeDev& F, const double* __restrict__ theta0, int64_t j) {
  if (!theta0) return 0.0;
  return PRIOR ? (theta0[j] - F.mu[j]) / F.sc[j] : theta0[j];
}

template <bool PRIOR = false>
__global__ void fe_init_kernel(FeDev F, const double* __restrict__ theta0) {
  for (int j = blockIdx.x * blockDim.x + threadIdx.x; j < F.P; j += gridDim.x * blockDim.x) {
    F.W.x[j] = fe_start_of<PRIOR>(F, theta0, j);
    F.W.d[j] = 0.0;
    F.W.r[j] = 0.0;
    F.W.g[j] = 0.0;
    F.W.t[j] = 0.0;
  }
  // the shard's local copy of the start point (afterwards the update keeps it current: fe_update_one)
  for (int jl = blockIdx.x * blockDim.x + threadIdx.x; jl < F.d; jl += gridDim.x * blockDim.x) {
    const int64_t j = F.umap[jl];      // (widened: an index into the global coefficient space)
    F.xl[jl] = fe_theta_of<PRIOR>(F, j, fe_start_of<PRIOR>(F, theta0, j));
    F.inv[j] = jl;
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    CompactState S;
    compact_init(S);
    *F.state = S;
  }
}

// ---- incremental training: what only a problem with a prior launches ------------------------------------------------------------------
// *bad = 1 if a scale is not finite or not > 0 (gdmix_fe_set_prior reads it back before anything of the problem is touched)
__global__ void fe_prior_check_kernel(const double* __restrict__ scale, int P, int32_t* __restrict__ bad) {
  for (int j = blockIdx.x * blockDim.x + threadIdx.x; j < P; j += gridDim.x * blockDim.x) {
    const double s = scale[j];
    if (!(s > 0.0) || s == __builtin_inf()) *bad = 1;      // (every writer stores the same value)
  }
}

// gdmix_fe_result with a prior: theta = mu + s (.) phi, the expression the passes gathered from
__global__ void fe_prior_theta_kernel(FeDev F, double* __restrict__ theta) {
  for (int j = blockIdx.x * blockDim.x + threadIdx.x; j < F.P; j += gridDim.x * blockDim.x) theta[j] = fe_theta_of<true>(F, j, F.W.x[j]);
}


}  // namespace gdmix

using namespace gdmix;

// ---- scoring ----------------------------------------------------------------------------------------------------------
// logits of every sample of a raw shard under a global coefficient vector (intercept last): one thread per sample straight
// off the sample-major arrays the reader produced — no pack, no column copy; the coefficient vector (8 B x features) is
// gathered from L2. Sums in row order, starting from the intercept, as the packed scoring pass does.
__global__ __launch_bounds__(256) void fe_score_kernel(int64_t n, const int64_t* __restrict__ row_nnz_ptr,
                                                       const int64_t* __restrict__ col_global, const float* __restrict__ val,
                                                       const float* __restrict__ offset, const double* __restrict__ theta,
                                                       int64_t D, int ic, float* __restrict__ score, float* __restrict__ per_coord) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  double acc = ic ? theta[D] : 0.0;
  if (row_nnz_ptr) {
    int64_t k = row_nnz_ptr[i];
    const int64_t k1 = row_nnz_ptr[i + 1];
    for (; k + 4 <= k1; k += 4) {
      const float v0 = val[k], v1 = val[k + 1], v2 = val[k + 2], v3 = val[k + 3];
      const double t0 = theta[col_global[k]], t1 = theta[col_global[k + 1]], t2 = theta[col_global[k + 2]], t3 = theta[col_global[k + 3]];
      acc += (double)v0 * t0;
      acc += (double)v1 * t1;
      acc += (double)v2 * t2;
      acc += (double)v3 * t3;
    }
    for (; k < k1; ++k) acc += (double)val[k] * theta[col_global[k]];
  }
  const double off = offset ? (double)offset[i] : 0.0;
  const double z = acc + off;
  score[i] = (float)z;
  per_coord[i] = (float)(z - off);
}


constexpr int FE_RING = 8;

struct gdmix_fe_problem {
  gdmix_re_ctx* ctx = nullptr;
  FeDev F{};
  SolveParams o{};
  DevBuf pool;           // one device allocation carved into the vectors and partial sums
  size_t pool_bytes = 0, pool_multi = 0, pool_multi_end = 0, pool_inv = 0;   // its size; the part gdmix_fe_restart keeps (F.multi); where F.inv lies
  DevBuf copies[2];      // the row pass's and the column pass's copy of the non-zeros, with their unit tables
  DevBuf ccopies[2];     // ... and their units in the 6-byte form
  DevBuf hot_mem;        // the frequent columns' list
  DevBuf prior_mem;      // [2 P] the problem's copy of the prior mean and scale, then the check's flag (gdmix_fe_set_prior); empty until the first prior
  double l1 = 0.0;       // weight of the L1 term (gdmix_fe_set_l1); > 0: the step is OWL-QN's (fe_qn.hip)
  DevBuf tron_mem;       // the TRON buffer (fe_internal.hpp: FeTron); empty until TRON is first selected or gdmix_fe_hessian_vec first called
  int optimizer = GDMIX_FE_OPT_LBFGS;      // gdmix_fe_set_optimizer; TRON: the pass pairs are the HV variant's, the step fe_tron.hip's
  DevBuf box_mem;        // [2 P] the problem's copy of the lower and upper bounds, then the check's flags (gdmix_fe_set_bounds); empty until the first bounds
  bool box = false;      // bounds are installed: the step is the projected L-BFGS of fe_qn.hip
  const double* box_lo() const { return box_mem.as<double>(); }
  const double* box_hi() const { return box_mem.as<double>() + F.P; }
  int32_t* status_dev = nullptr;
  hipEvent_t ev[3] = {};
  bool timed = false;
  bool dirty = false;        // the reduce buffer holds a result no step has consumed (and cleared) yet
  bool fused_tail = true;    // the step is one launch (fe_tail_kernel); GDMIX_FE_FUSED_TAIL=0: dots / step / update as three (A/B)
  unsigned gen = 0;      // launches of fe_tail_kernel so far (its generation stamp)
  int64_t evals = 0;     // gdmix_fe_eval calls so far
  int64_t seq = 0;       // steps enqueued so far; step k's status lands in status_ring[k % FE_RING] behind ring_ev[k % FE_RING]
  PinnedBuf status_ring; // [FE_RING] int32_t
  hipEvent_t ring_ev[FE_RING] = {};

  ~gdmix_fe_problem() {
    for (auto& e : ev) if (e) (void)hipEventDestroy(e);
    for (auto& e : ring_ev) if (e) (void)hipEventDestroy(e);
  }
};

// The test hooks of include/gdmix_fe.h, read once per problem (the top of gdmix_fe_create); a value out of range is no value.
static FeHooks fe_hooks_from_env() {
  FeHooks h;
  if (const char* e = getenv("GDMIX_FE_CHUNK")) { const long v = atol(e); if (v >= 64) h.chunk = v; }
  if (const char* e = getenv("GDMIX_FE_WINDOW_BITS")) { const int v = atoi(e); if (v >= 1 && v < FE_SPAN_BITS) h.window_bits = v; }
  if (const char* e = getenv("GDMIX_FE_PACK")) h.pack = atoi(e) != 0;
  if (const char* e = getenv("GDMIX_FE_HOT_MIN")) h.hot_min = atol(e);
  if (const char* e = getenv("GDMIX_FE_COMPRESS")) h.compress = atoi(e) & 3;
  if (const char* e = getenv("GDMIX_FE_FUSED_TAIL")) h.fused_tail = e[0] != '0';
  return h;
}

// prior: x of F is phi (a prior is installed and the pass runs at the solver's point): the row pass reads theta = mu + s (.) phi
template <bool HESS>
static int fe_passes(gdmix_fe_problem* p, const FeDev& F, hipStream_t s, bool timed, bool prior) {
  // features absent from this shard must read 0 in the reduce buffer; fe_dots_kernel leaves it cleared behind a step
  if (p->dirty) HIP_TRY(hipMemsetAsync(F.fg, 0, ((size_t)F.P + 1) * 8, s));
  p->dirty = true;
  // xl (x in the shard's local order) is kept current by the step's update (fe_update_one); the Hessian passes may run at
  // another point: they gather it themselves and put the solver's back afterwards
  const auto prepare = [&](const FeDev& G, bool with_prior) {
    with_flag(with_prior, [&](auto PR) { hipLaunchKernelGGL(fe_prepare_kernel<decltype(PR)::value>, dim3(grid_for(G.d, 256, 2048)), dim3(256), 0, s, G); });
  };
  if (HESS) prepare(F, prior);
  if (timed) HIP_TRY(hipEventRecord(p->ev[0], s));
  with_flag(prior, [&](auto PR) {
    constexpr bool PRIOR = decltype(PR)::value;
    with_flag(F.rc.ent != nullptr, [&](auto PK) { hipLaunchKernelGGL((fe_scatter_kernel<true, HESS, decltype(PK)::value, PRIOR>), dim3(F.rc.nlaunch), dim3(WAVE), 0, s, F, p->o); });
    if (F.nmulti) hipLaunchKernelGGL((fe_rows_fix_kernel<HESS, PRIOR>), dim3(F.nmulti * FE_FIX_PER_BLOCK), dim3(FE_THREADS), 0, s, F, p->o);
  });
  if (timed) HIP_TRY(hipEventRecord(p->ev[1], s));
  // (the column pass gathers residuals: it has no prior variant)
  with_flag(F.cc.ent != nullptr, [&](auto PK) { hipLaunchKernelGGL((fe_scatter_kernel<false, HESS, decltype(PK)::value>), dim3(F.cc.nlaunch), dim3(WAVE), 0, s, F, p->o); });
  if (timed) HIP_TRY(hipEventRecord(p->ev[2], s));
  int gf = (F.d + FE_RED_OUT - 1) / FE_RED_OUT;
  hipLaunchKernelGGL(fe_finish_kernel<HESS>, dim3((gf < FE_FIN_BLOCKS ? FE_FIN_BLOCKS : gf) + F.hot.n), dim3(FE_THREADS), 0, s, F);
  if (HESS) prepare(p->F, p->F.mu != nullptr);      // the solver's point back into xl
  HIP_TRY(hipGetLastError());
  return GDMIX_RE_OK;
}

// The row pass of the HV variant: what it computes is the record's business (fe_hv_entry).
static void fe_rows_hv(const FeDev& F, const SolveParams& o, hipStream_t s) {
  with_flag(F.rc.ent != nullptr, [&](auto PK) { hipLaunchKernelGGL((fe_scatter_kernel<true, false, decltype(PK)::value, false, true>), dim3(F.rc.nlaunch), dim3(WAVE), 0, s, F, o); });
  if (F.nmulti) hipLaunchKernelGGL((fe_rows_fix_kernel<false, false, true>), dim3(F.nmulti * FE_FIX_PER_BLOCK), dim3(FE_THREADS), 0, s, F, o);
}

// A pass pair of a TRON problem: the HV row pass, then the column pass and the finish of an evaluation, unchanged — they gather and add
// up whatever the row pass left in rs, and stop on the same flag.
static int fe_passes_tron(gdmix_fe_problem* p, hipStream_t s, bool timed) {
  const FeDev& F = p->F;
  if (p->dirty) HIP_TRY(hipMemsetAsync(F.fg, 0, ((size_t)F.P + 1) * 8, s));
  p->dirty = true;
  if (timed) HIP_TRY(hipEventRecord(p->ev[0], s));
  fe_rows_hv(F, p->o, s);
  if (timed) HIP_TRY(hipEventRecord(p->ev[1], s));
  with_flag(F.cc.ent != nullptr, [&](auto PK) { hipLaunchKernelGGL((fe_scatter_kernel<false, false, decltype(PK)::value>), dim3(F.cc.nlaunch), dim3(WAVE), 0, s, F, p->o); });
  if (timed) HIP_TRY(hipEventRecord(p->ev[2], s));
  const int gf = (F.d + FE_RED_OUT - 1) / FE_RED_OUT;
  hipLaunchKernelGGL(fe_finish_kernel<false>, dim3((gf < FE_FIN_BLOCKS ? FE_FIN_BLOCKS : gf) + F.hot.n), dim3(FE_THREADS), 0, s, F);
  HIP_TRY(hipGetLastError());
  return GDMIX_RE_OK;
}

// The TRON buffer, allocated on first need (the pool's size and layout do not depend on the optimiser).
static int fe_tron_alloc(gdmix_fe_problem* p, hipStream_t s) {
  if (p->tron_mem) return GDMIX_RE_OK;
  const size_t bytes = fe_tron_bytes(p->F.P, p->F.d, p->F.n);
  const hipError_t rc = p->tron_mem.alloc(bytes);
  if (rc != hipSuccess) { set_error("hipMalloc(%zu) failed: %s", bytes, hipGetErrorString(rc)); return GDMIX_RE_ENOMEM; }
  HIP_TRY(hipMemsetAsync(p->tron_mem.get(), 0, bytes, s));
  p->F.W.part = p->tron_mem.as<double>();      // (fe_internal.hpp: fe_tron_state)
  return GDMIX_RE_OK;
}

// The problem as gdmix_fe_create leaves it, at its current options and prior, from start point theta0 (gdmix_fe_restart, gdmix_fe_set_prior):
// the pool is zeroed again but for the list of row blocks with several units, F.inv refilled, the start point and a fresh L-BFGS state
// written by the same fe_init_kernel, the host's counters put back. Everything is enqueued behind whatever the stream still holds.
static int fe_reset(gdmix_fe_problem* p, const double* theta0, hipStream_t s) {
  const FeDev& F = p->F;
  char* base = p->pool.as<char>();
  HIP_TRY(hipMemsetAsync(base, 0, p->pool_multi, s));
  HIP_TRY(hipMemsetAsync(base + p->pool_multi_end, 0, p->pool_bytes - p->pool_multi_end, s));
  HIP_TRY(hipMemsetAsync(base + p->pool_inv, 0xff, (size_t)F.P * 4, s));
  with_flag(F.mu != nullptr, [&](auto PR) { hipLaunchKernelGGL(fe_init_kernel<decltype(PR)::value>, dim3(grid_for(F.P, 256, 1024)), dim3(256), 0, s, F, theta0); });
  if (fe_tron_state(F)) fe_tron_enqueue_reset(F, theta0, s);      // (also on a problem set back to L-BFGS-B: the record is what gdmix_fe_hessian_vec finds)
  if (p->box) fe_box_enqueue_start(F, p->box_lo(), p->box_hi(), s);      // the start point is the clamped one, zeros included
  HIP_TRY(hipGetLastError());
  p->timed = false;
  p->dirty = false;
  p->gen = 0u;
  p->seq = 0;
  p->evals = 0;
  return GDMIX_RE_OK;
}

// The pool: every vector and partial sum of the problem in one allocation, zeroed (F.inv: -1, the coefficient is not a column of this
// shard), F's pointers into it, the list of the row blocks with several units. Needs the unit counts of both copies.
static int fe_make_pool(gdmix_fe_problem* p, const std::vector<int32_t>& multi, int m, hipStream_t s) {
  FeDev& F = p->F;
  const size_t P = (size_t)F.P;
  Arena a;
  const size_t o_xl = a.take((size_t)(F.d + 1) * 8), o_rs = a.take((size_t)(F.n + 1) * 8), o_fg = a.take((P + 1) * 8);
  const size_t o_pr = a.take((size_t)F.rc.nunit * FE_B * 8), o_pc = a.take((size_t)F.cc.nunit * FE_B * 8);
  const size_t o_multi = a.take((multi.size() + 1) * 4), o_red = a.take((size_t)F.nred * 3 * 8 + 16);
  const size_t o_acc = a.take((size_t)FE_DOT_BLOCKS * COMPACT_KD * 8), o_fin = a.take((size_t)FE_FIN_BLOCKS * 3 * 8 + 64);
  const size_t o_state = a.take(sizeof(CompactState)), o_plan = a.take(sizeof(CompactPlan)), o_mats = a.take(sizeof(CompactMats));
  const size_t o_vec = a.take(((size_t)5 * P + compact_hist_doubles((int64_t)P, m)) * 8 + 16), o_status = a.take(64);
  const size_t o_inv = a.take(P * 4), o_sync = a.take(sizeof(FeSync));
  const hipError_t rc = p->pool.alloc(a.off);
  if (rc != hipSuccess) { set_error("hipMalloc(%zu) failed: %s", a.off, hipGetErrorString(rc)); return GDMIX_RE_ENOMEM; }
  p->pool_bytes = a.off; p->pool_multi = o_multi; p->pool_multi_end = o_red; p->pool_inv = o_inv;
  const DevBuf& pool = p->pool;
  HIP_TRY(hipMemsetAsync(pool.get(), 0, a.off, s));
  HIP_TRY(hipMemsetAsync(pool.as<char>(o_inv), 0xff, P * 4, s));
  F.xl = pool.as<double>(o_xl); F.rs = pool.as<double>(o_rs);
  F.fg = pool.as<double>(o_fg);
  F.rc.part = pool.as<double>(o_pr); F.cc.part = pool.as<double>(o_pc);
  F.multi = pool.as<const int32_t>(o_multi);
  F.loss_part = pool.as<double>(o_red); F.rsum_part = F.loss_part + F.nred; F.loss_lo_part = F.rsum_part + F.nred;
  F.acc_part = pool.as<double>(o_acc);
  F.fin_part = pool.as<double>(o_fin);
  F.fin_count = pool.as<unsigned>(o_fin + (size_t)FE_FIN_BLOCKS * 3 * 8);
  F.state = pool.as<CompactState>(o_state);
  F.plan = pool.as<CompactPlan>(o_plan);
  F.mats = pool.as<CompactMats>(o_mats);
  double* v = pool.as<double>(o_vec);
  F.W.x = v; F.W.g = v + P; F.W.d = v + 2 * P; F.W.t = v + 3 * P; F.W.r = v + 4 * P;
  F.W.ws = v + 5 * P + ((5 * P) & 1);   // 16-byte aligned: the interleaved history (re_lbfgs_compact.hpp) is read with 16-byte loads
  F.W.wy = F.W.ws + (size_t)m * P;
  F.W.rs = F.rs; F.W.alpha = nullptr; F.W.rho = nullptr; F.W.part = nullptr;
  p->status_dev = pool.as<int32_t>(o_status);
  F.inv = pool.as<int32_t>(o_inv);
  F.sync = pool.as<FeSync>(o_sync);
  return GDMIX_RE_OK;
}

extern "C" {

GDMIX_API int gdmix_fe_create(gdmix_re_ctx* ctx, const gdmix_re_packed* b, int64_t num_features, const gdmix_re_opts* opts,
                              const double* theta0, gdmix_fe_problem** out, void* stream) {
  if (!out) { set_error("out is NULL"); return GDMIX_RE_EINVAL; }
  *out = nullptr;
  if (!ctx || !b || !opts) { set_error("NULL argument"); return GDMIX_RE_EINVAL; }
  if (b->E != 1) { set_error("the shard must be packed as one entity (E = %lld)", (long long)b->E); return GDMIX_RE_EINVAL; }
  if (opts->m < 1 || opts->m > TEAM_MCAP) { set_error("1 <= m <= %d", TEAM_MCAP); return GDMIX_RE_EINVAL; }
  if (!loss_code_ok(opts->loss, "gdmix_fe_create")) return GDMIX_RE_EINVAL;
  if (opts->regularize_bias && !opts->has_intercept) { set_error("regularize_bias requires has_intercept"); return GDMIX_RE_EINVAL; }
  if (num_features < 1 || num_features > 0x7ffffff0ll) { set_error("bad num_features"); return GDMIX_RE_EINVAL; }
  if (b->Z > 0x7ffffff0ll || b->N > 0x7ffffff0ll) { set_error("shard exceeds 2^31 samples or non-zeros"); return GDMIX_RE_ERANGE; }
  const FeHooks hooks = fe_hooks_from_env();
  hipStream_t s = static_cast<hipStream_t>(stream);
  gdmix_ctx_impl* ci = &ctx->impl;
  HIP_TRY(hipSetDevice(ci->device));
  HIP_TRY(join_unique(ci, s));   // the shard's unique_global is read here
  std::unique_ptr<gdmix_fe_problem> p(new (std::nothrow) gdmix_fe_problem());
  if (!p) { set_error("out of host memory"); return GDMIX_RE_ENOMEM; }
  p->ctx = ctx;
  // the one-launch step has workgroups waiting for the last arriver: next to ANOTHER process's persistent grid neither might get
  // all its workgroups placed (re_internal.hpp: why this kernel is not behind the inter-process lock). A device that another
  // process is present on gets the three-launch step; GDMIX_FE_FUSED_TAIL=0 / 1 decides whatever the device looks like.
  p->fused_tail = hooks.fused_tail ? *hooks.fused_tail : !device_has_another_process(ci->device);
  FeDev& F = p->F;
  const int ic = opts->has_intercept ? 1 : 0;
  F.n = (int)b->N; F.z = b->Z; F.d = (int)b->D; F.ic = ic; F.D = num_features; F.P = (int)num_features + ic; F.m = opts->m;
  F.y = b->y; F.o = b->offset; F.w = b->weight; F.umap = b->unique_global;
  p->o = fe_solve_params(*opts);
  // row pass: outputs = rows, gathered = x by local column: from the column-major arrays. Column pass: the other way round,
  // the frequent columns apart.
  const int compress = hooks.compress.value_or(FE_COMPRESS_DEFAULT);
  const FeSource rows{b->col_ptr, F.d, b->csc_row, b->csc_val, F.z, F.n, false, (compress & 1) != 0};
  std::vector<int32_t> uf_r;
  int rc = fe_build_copy(s, ci->num_cus, hooks, rows, &F.rc, &p->copies[0], &p->ccopies[0], &uf_r);
  if (rc == GDMIX_RE_OK) rc = fe_build_column_copy(s, ci->num_cus, hooks, b, F.n, F.d, F.z, &F.cc, &F.hot, &p->copies[1], &p->ccopies[1], &p->hot_mem);
  if (rc != GDMIX_RE_OK) return rc;
  std::vector<int32_t> multi;
  for (int rb = 0; rb < F.rc.nblock; ++rb) if (uf_r[(size_t)rb + 1] - uf_r[(size_t)rb] > 1) multi.push_back(rb);
  F.nmulti = (int)multi.size();
  F.nred = F.rc.nunit + F.nmulti * FE_FIX_PER_BLOCK;
  rc = fe_make_pool(p.get(), multi, opts->m, s);
  if (rc != GDMIX_RE_OK) return rc;
  HIP_TRY(p->status_ring.alloc(FE_RING * sizeof(int32_t)));
  for (auto& e : p->ring_ev) HIP_TRY(hipEventCreateWithFlags(&e, hipEventDisableTiming));
  if (!multi.empty()) {
    HIP_TRY(hipMemcpyAsync(p->pool.as<char>(p->pool_multi), multi.data(), multi.size() * 4, hipMemcpyHostToDevice, s));
    HIP_TRY(hipStreamSynchronize(s));   // `multi` goes out of scope
  }
  hipLaunchKernelGGL(fe_init_kernel<false>, dim3(grid_for(F.P, 256, 1024)), dim3(256), 0, s, F, theta0);
  HIP_TRY(hipGetLastError());
  *out = p.release();
  return GDMIX_RE_OK;
}

// The problem as gdmix_fe_create leaves it, for other options and another start point (include/gdmix_fe.h): fe_reset above.
GDMIX_API int gdmix_fe_restart(gdmix_fe_problem* p, const gdmix_re_opts* opts, const double* theta0, void* stream) {
  if (!p || !opts) { set_error("NULL argument"); return GDMIX_RE_EINVAL; }
  const FeDev& F = p->F;
  if ((opts->has_intercept ? 1 : 0) != F.ic || opts->m != F.m || opts->loss != p->o.loss) {
    set_error("gdmix_fe_restart: has_intercept, loss and m must be the creation's (%d, %d, %d), not (%d, %d, %d): the pool is sized by them",
              F.ic, p->o.loss, F.m, opts->has_intercept ? 1 : 0, opts->loss, opts->m);
    return GDMIX_RE_EINVAL;
  }
  if (opts->regularize_bias && !opts->has_intercept) { set_error("regularize_bias requires has_intercept"); return GDMIX_RE_EINVAL; }
  hipStream_t s = static_cast<hipStream_t>(stream);
  HIP_TRY(hipSetDevice(p->ctx->impl.device));
  p->o = fe_solve_params(*opts);      // (has_intercept, m and loss are the creation's: checked above)
  return fe_reset(p, theta0, s);
}

GDMIX_API int gdmix_fe_set_prior(gdmix_fe_problem* p, const double* mean, const double* scale, void* stream) {
  if (!p) { set_error("problem is NULL"); return GDMIX_RE_EINVAL; }
  if ((mean == nullptr) != (scale == nullptr)) { set_error("gdmix_fe_set_prior: mean and scale are given together, or both NULL"); return GDMIX_RE_EINVAL; }
  hipStream_t s = static_cast<hipStream_t>(stream);
  HIP_TRY(hipSetDevice(p->ctx->impl.device));
  FeDev& F = p->F;
  if (mean && p->l1 > 0.0) { set_error("gdmix_fe_set_prior: the problem has an L1 term (gdmix_fe_set_l1), which does not compose with a prior"); return GDMIX_RE_EINVAL; }
  if (mean && p->optimizer == GDMIX_FE_OPT_TRON) {
    set_error("gdmix_fe_set_prior: the problem's optimiser is TRON (gdmix_fe_set_optimizer), whose product has no prior variant yet");
    return GDMIX_RE_EINVAL;
  }
  if (mean && p->box) {
    set_error("gdmix_fe_set_prior: the problem has bounds (gdmix_fe_set_bounds), which are not carried through the prior's change of variables yet");
    return GDMIX_RE_EINVAL;
  }
  if (!mean) {
    F.mu = nullptr; F.sc = nullptr;      // (the copy stays allocated: kernels of an earlier solve may still be queued on it)
    return fe_reset(p, nullptr, s);
  }
  const size_t P = (size_t)F.P;
  if (!p->prior_mem) {
    const hipError_t rc = p->prior_mem.alloc(2 * P * 8 + 64);
    if (rc != hipSuccess) { set_error("hipMalloc(%zu) failed: %s", 2 * P * 8 + 64, hipGetErrorString(rc)); return GDMIX_RE_ENOMEM; }
  }
  double* prior = p->prior_mem.as<double>();
  // the caller's scale is checked before the problem's copy — a prior an earlier call installed — is overwritten
  int32_t* bad_dev = reinterpret_cast<int32_t*>(prior + 2 * P);
  HIP_TRY(hipMemsetAsync(bad_dev, 0, sizeof(int32_t), s));
  hipLaunchKernelGGL(fe_prior_check_kernel, dim3(grid_for(F.P, 256, 1024)), dim3(256), 0, s, scale, F.P, bad_dev);
  HIP_TRY(hipGetLastError());
  int32_t bad = 0;
  HIP_TRY(hipMemcpyAsync(&bad, bad_dev, sizeof(int32_t), hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));      // the one wait of this call
  if (bad) { set_error("gdmix_fe_set_prior: every scale must be finite and > 0"); return GDMIX_RE_EINVAL; }
  HIP_TRY(hipMemcpyAsync(prior, mean, P * 8, hipMemcpyDeviceToDevice, s));
  HIP_TRY(hipMemcpyAsync(prior + P, scale, P * 8, hipMemcpyDeviceToDevice, s));
  F.mu = prior; F.sc = prior + P;
  return fe_reset(p, nullptr, s);
}

GDMIX_API int gdmix_fe_set_l1(gdmix_fe_problem* p, double l1, void* stream) {
  if (!p) { set_error("problem is NULL"); return GDMIX_RE_EINVAL; }
  if (!(l1 >= 0.0) || l1 == __builtin_inf()) { set_error("gdmix_fe_set_l1: l1 must be finite and >= 0"); return GDMIX_RE_EINVAL; }
  if (p->F.mu) { set_error("gdmix_fe_set_l1: the problem has a prior (gdmix_fe_set_prior), which does not compose with an L1 term"); return GDMIX_RE_EINVAL; }
  if (l1 > 0.0 && p->optimizer == GDMIX_FE_OPT_TRON) {
    set_error("gdmix_fe_set_l1: the problem's optimiser is TRON (gdmix_fe_set_optimizer), which minimises a smooth objective: no L1 term");
    return GDMIX_RE_EINVAL;
  }
  if (l1 > 0.0 && p->box) {
    set_error("gdmix_fe_set_l1: the problem has bounds (gdmix_fe_set_bounds), whose step minimises a smooth objective: no L1 term");
    return GDMIX_RE_EINVAL;
  }
  HIP_TRY(hipSetDevice(p->ctx->impl.device));
  p->l1 = l1;
  return fe_reset(p, nullptr, static_cast<hipStream_t>(stream));
}

GDMIX_API int gdmix_fe_set_optimizer(gdmix_fe_problem* p, int optimizer, void* stream) {
  if (!p) { set_error("problem is NULL"); return GDMIX_RE_EINVAL; }
  if (optimizer != GDMIX_FE_OPT_LBFGS && optimizer != GDMIX_FE_OPT_TRON) {
    set_error("gdmix_fe_set_optimizer: unknown optimiser %d (GDMIX_FE_OPT_LBFGS = %d, GDMIX_FE_OPT_TRON = %d)", optimizer, GDMIX_FE_OPT_LBFGS, GDMIX_FE_OPT_TRON);
    return GDMIX_RE_EINVAL;
  }
  if (optimizer == GDMIX_FE_OPT_TRON && p->l1 > 0.0) {
    set_error("gdmix_fe_set_optimizer: the problem has an L1 term (gdmix_fe_set_l1); TRON minimises a smooth objective");
    return GDMIX_RE_EINVAL;
  }
  if (optimizer == GDMIX_FE_OPT_TRON && p->F.mu) {
    set_error("gdmix_fe_set_optimizer: the problem has a prior (gdmix_fe_set_prior); TRON's product has no prior variant yet");
    return GDMIX_RE_EINVAL;
  }
  if (optimizer == GDMIX_FE_OPT_TRON && p->box) {
    set_error("gdmix_fe_set_optimizer: the problem has bounds (gdmix_fe_set_bounds); TRON minimises without constraints");
    return GDMIX_RE_EINVAL;
  }
  hipStream_t s = static_cast<hipStream_t>(stream);
  HIP_TRY(hipSetDevice(p->ctx->impl.device));
  if (optimizer == GDMIX_FE_OPT_TRON) {
    const int rc = fe_tron_alloc(p, s);
    if (rc != GDMIX_RE_OK) return rc;
  }
  p->optimizer = optimizer;
  return fe_reset(p, nullptr, s);
}

GDMIX_API int gdmix_fe_set_bounds(gdmix_fe_problem* p, const double* lower, const double* upper, void* stream) {
  if (!p) { set_error("problem is NULL"); return GDMIX_RE_EINVAL; }
  if ((lower == nullptr) != (upper == nullptr)) { set_error("gdmix_fe_set_bounds: lower and upper are given together, or both NULL"); return GDMIX_RE_EINVAL; }
  hipStream_t s = static_cast<hipStream_t>(stream);
  HIP_TRY(hipSetDevice(p->ctx->impl.device));
  if (!lower) {
    p->box = false;      // (the copy stays allocated: kernels of an earlier solve may still be queued on it)
    return fe_reset(p, nullptr, s);
  }
  if (p->l1 > 0.0) { set_error("gdmix_fe_set_bounds: the problem has an L1 term (gdmix_fe_set_l1); the bounded step minimises a smooth objective"); return GDMIX_RE_EINVAL; }
  if (p->optimizer == GDMIX_FE_OPT_TRON) {
    set_error("gdmix_fe_set_bounds: the problem's optimiser is TRON (gdmix_fe_set_optimizer), which minimises without constraints");
    return GDMIX_RE_EINVAL;
  }
  if (p->F.mu) {
    set_error("gdmix_fe_set_bounds: the problem has a prior (gdmix_fe_set_prior); bounds are not carried through its change of variables yet");
    return GDMIX_RE_EINVAL;
  }
  const size_t P = (size_t)p->F.P;
  if (!p->box_mem) {
    const hipError_t rc = p->box_mem.alloc(2 * P * 8 + 64);
    if (rc != hipSuccess) { set_error("hipMalloc(%zu) failed: %s", 2 * P * 8 + 64, hipGetErrorString(rc)); return GDMIX_RE_ENOMEM; }
  }
  double* box = p->box_mem.as<double>();
  // the caller's bounds are checked before the problem's copy — bounds an earlier call installed — is overwritten
  int32_t* bad_dev = reinterpret_cast<int32_t*>(box + 2 * P);
  HIP_TRY(hipMemsetAsync(bad_dev, 0, 3 * sizeof(int32_t), s));
  fe_box_enqueue_check(lower, upper, p->F.P, p->F.ic, bad_dev, s);
  HIP_TRY(hipGetLastError());
  int32_t bad[3] = {0, 0, 0};
  HIP_TRY(hipMemcpyAsync(bad, bad_dev, sizeof(bad), hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));      // the one wait of this call
  if (bad[0]) { set_error("gdmix_fe_set_bounds: a bound is not a number"); return GDMIX_RE_EINVAL; }
  if (bad[1]) { set_error("gdmix_fe_set_bounds: a lower bound exceeds its upper bound"); return GDMIX_RE_EINVAL; }
  if (bad[2]) { set_error("gdmix_fe_set_bounds: the intercept is never bounded: its bounds must be -inf and +inf"); return GDMIX_RE_EINVAL; }
  HIP_TRY(hipMemcpyAsync(box, lower, P * 8, hipMemcpyDeviceToDevice, s));
  HIP_TRY(hipMemcpyAsync(box + P, upper, P * 8, hipMemcpyDeviceToDevice, s));
  p->box = true;
  return fe_reset(p, nullptr, s);
}

GDMIX_API int gdmix_fe_products(gdmix_fe_problem* p, int64_t* nhv, void* stream) {
  if (!p || !nhv) { set_error("NULL argument"); return GDMIX_RE_EINVAL; }
  *nhv = 0;
  if (!fe_tron_state(p->F)) return GDMIX_RE_OK;      // never a TRON problem: no product taken
  hipStream_t s = static_cast<hipStream_t>(stream);
  FeTronState st;
  HIP_TRY(hipMemcpyAsync(&st, fe_tron_state(p->F), sizeof(st), hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  *nhv = (int64_t)st.nhv;
  return GDMIX_RE_OK;
}

GDMIX_API void gdmix_fe_destroy(gdmix_fe_problem* p) {
  delete p;
}

GDMIX_API double* gdmix_fe_reduce_buffer(gdmix_fe_problem* p, int64_t* count) {
  if (!p) return nullptr;
  if (count) *count = (int64_t)p->F.P + 1;
  return p->F.fg;
}

GDMIX_API int gdmix_fe_eval(gdmix_fe_problem* p, void* stream) {
  if (!p) { set_error("problem is NULL"); return GDMIX_RE_EINVAL; }
  if (!p->ev[0]) for (auto& e : p->ev) HIP_TRY(hipEventCreate(&e));
  // the first two evaluations of a problem are timed (gdmix_fe_last_eval_ms reports the second): with the status read a few steps
  // late the LAST evaluations of a solve are no-ops
  const bool timed = p->evals < 2;
  const int rc = p->optimizer == GDMIX_FE_OPT_TRON ? fe_passes_tron(p, static_cast<hipStream_t>(stream), timed)
                                                   : fe_passes<false>(p, p->F, static_cast<hipStream_t>(stream), timed, p->F.mu != nullptr);
  if (rc == GDMIX_RE_OK) { if (timed) p->timed = true; ++p->evals; }
  return rc;
}

GDMIX_API int gdmix_fe_hessian_diag(gdmix_fe_problem* p, const double* theta, void* stream) {
  if (!p) { set_error("problem is NULL"); return GDMIX_RE_EINVAL; }
  FeDev F = p->F;
  if (theta) F.W.x = const_cast<double*>(theta);   // the passes only read x
  p->dirty = true;   // (a step enqueued behind the stop leaves the buffer as it was)
  // theta is in theta units whatever the problem holds: only the current point of a problem with a prior is phi
  return fe_passes<true>(p, F, static_cast<hipStream_t>(stream), false, !theta && F.mu != nullptr);
}

GDMIX_API int gdmix_fe_hessian_vec(gdmix_fe_problem* p, const double* theta, const double* v, void* stream) {
  if (!p || !v) { set_error("NULL argument"); return GDMIX_RE_EINVAL; }
  hipStream_t s = static_cast<hipStream_t>(stream);
  HIP_TRY(hipSetDevice(p->ctx->impl.device));
  int rc = fe_tron_alloc(p, s);
  if (rc != GDMIX_RE_OK) return rc;
  FeDev F = p->F;
  const bool prior = !theta && F.mu != nullptr;      // theta is in theta units; only the current point of a problem with a prior is phi
  // the current accepted point of a TRON problem is W.x as well (fe_tron.hip); under the OWL-QN step it is W.t
  if (theta) F.W.x = const_cast<double*>(theta);
  else if (p->l1 > 0.0 || p->box) F.W.x = F.W.t;
  HIP_TRY(hipMemsetAsync(F.fg, 0, ((size_t)F.P + 1) * 8, s));
  p->dirty = true;
  const auto prepare = [&](const FeDev& G, bool with_prior) {
    with_flag(with_prior, [&](auto PR) { hipLaunchKernelGGL(fe_prepare_kernel<decltype(PR)::value>, dim3(grid_for(G.d, 256, 2048)), dim3(256), 0, s, G); });
  };
  if (prior) {
    // the HV row pass has no prior variant: theta = mu + s (.) phi is formed once, in the buffer's trial-point slot (a TRON problem has no prior)
    double* th = fe_tron_of(F).xt;
    hipLaunchKernelGGL(fe_prior_theta_kernel, dim3(grid_for(F.P, 256, 1024)), dim3(256), 0, s, F, th);
    F.W.x = th;
  }
  prepare(F, false);
  fe_tron_enqueue_hv_begin(F, s);
  fe_rows_hv(F, p->o, s);                 // the curvature weights at theta
  fe_tron_enqueue_hv_vector(F, v, s);
  fe_rows_hv(F, p->o, s);                 // rs = D (X~ v)
  with_flag(F.cc.ent != nullptr, [&](auto PK) { hipLaunchKernelGGL((fe_scatter_kernel<false, false, decltype(PK)::value, false, true>), dim3(F.cc.nlaunch), dim3(WAVE), 0, s, F, p->o); });
  const int gf = (F.d + FE_RED_OUT - 1) / FE_RED_OUT;
  hipLaunchKernelGGL(fe_finish_kernel<true>, dim3((gf < FE_FIN_BLOCKS ? FE_FIN_BLOCKS : gf) + F.hot.n), dim3(FE_THREADS), 0, s, F);
  fe_tron_enqueue_hv_end(F, s);
  // the solver's point back into xl: the trial point of a TRON problem, x otherwise
  if (p->optimizer == GDMIX_FE_OPT_TRON) { FeDev G = p->F; G.W.x = fe_tron_of(G).xt; prepare(G, false); }
  else prepare(p->F, p->F.mu != nullptr);
  HIP_TRY(hipGetLastError());
  return GDMIX_RE_OK;
}

GDMIX_API size_t gdmix_fe_hessian_dense_scratch_bytes(const gdmix_re_packed* shard) {
  return shard ? hessian_dense_scratch_doubles(shard->N) * 8 : 0;
}

static int fe_hessian_dense(gdmix_re_ctx* ctx, const gdmix_re_packed* b, int has_intercept, int loss, const double* theta_local, double* H,
                            int64_t ld, void* scratch, size_t scratch_bytes, void* stream) {
  if (!ctx || !b || !theta_local || !H || !scratch) { set_error("NULL argument"); return GDMIX_RE_EINVAL; }
  if (b->E != 1) { set_error("gdmix_fe_hessian_dense takes a one-entity batch (a worker's shard)"); return GDMIX_RE_EINVAL; }
  const int ic = has_intercept ? 1 : 0;
  if (b->D + ic > VAR_FULL_BIG_MAX_P) { set_error("dense Hessian of %lld coefficients: at most %lld", (long long)(b->D + ic), (long long)VAR_FULL_BIG_MAX_P); return GDMIX_RE_ERANGE; }
  if (ld < b->D + ic || ld % 64) { set_error("ld must be d + has_intercept rounded up to a multiple of 64"); return GDMIX_RE_EINVAL; }
  if (scratch_bytes < hessian_dense_scratch_doubles(b->N) * 8) { set_error("scratch too small"); return GDMIX_RE_ENOMEM; }
  HIP_TRY(hipSetDevice(ctx->impl.device));
  const BatchDev B = batch_dev(b);
  HIP_TRY(launch_hessian_dense(&ctx->impl, B, b->N, b->D, ic, theta_local, H, ld, static_cast<double*>(scratch), static_cast<hipStream_t>(stream), loss));
  return GDMIX_RE_OK;
}

GDMIX_API int gdmix_fe_hessian_dense(gdmix_re_ctx* ctx, const gdmix_re_packed* b, int has_intercept, const double* theta_local, double* H,
                                     int64_t ld, void* scratch, size_t scratch_bytes, void* stream) {
  return fe_hessian_dense(ctx, b, has_intercept, GDMIX_RE_LOSS_LOGISTIC, theta_local, H, ld, scratch, scratch_bytes, stream);
}

GDMIX_API int gdmix_fe_hessian_dense_loss(gdmix_re_ctx* ctx, const gdmix_re_packed* b, int has_intercept, int loss, const double* theta_local,
                                          double* H, int64_t ld, void* scratch, size_t scratch_bytes, void* stream) {
  if (!loss_code_ok(loss, "gdmix_fe_hessian_dense_loss")) return GDMIX_RE_EINVAL;
  return fe_hessian_dense(ctx, b, has_intercept, loss, theta_local, H, ld, scratch, scratch_bytes, stream);
}

GDMIX_API int gdmix_fe_variance_of_hessian(gdmix_re_ctx* ctx, double* H, int64_t p, int64_t ld, double l2, int64_t unregularised_index,
                                           double* work, double* variance, void* stream) {
  if (!ctx || !H || !work || !variance) { set_error("NULL argument"); return GDMIX_RE_EINVAL; }
  if (p < 1 || p > VAR_FULL_BIG_MAX_P || ld < p || ld % 64) { set_error("bad matrix dimensions (p = %lld, ld = %lld)", (long long)p, (long long)ld); return GDMIX_RE_EINVAL; }
  HIP_TRY(hipSetDevice(ctx->impl.device));
  HIP_TRY(launch_variance_of_hessian(&ctx->impl, H, work, p, ld, l2, unregularised_index, variance, static_cast<hipStream_t>(stream)));
  return GDMIX_RE_OK;
}

static int fe_enqueue_step(gdmix_fe_problem* p, hipStream_t s) {
  const FeDev& F = p->F;
  const int dot_blocks = grid_for(F.P, 256, FE_DOT_BLOCKS);
  const int tail_blocks = grid_for(dot_blocks, 1, p->ctx->impl.num_cus);      // at most one workgroup per CU: all resident, the wait inside cannot starve one
  if (p->fused_tail && !(p->l1 > 0.0) && !p->box && p->optimizer != GDMIX_FE_OPT_TRON) {
    ++p->gen;
    if (p->gen == 0u) ++p->gen;
  }
  if (p->optimizer == GDMIX_FE_OPT_TRON) fe_tron_enqueue_step(F, p->o, p->status_dev, s);      // (never with a prior or an L1 term: gdmix_fe_set_optimizer)
  else if (p->l1 > 0.0) fe_owlqn_enqueue_step(F, p->o, p->l1, p->status_dev, s);      // (never with a prior: gdmix_fe_set_l1)
  else if (p->box) fe_box_enqueue_step(F, p->o, p->box_lo(), p->box_hi(), p->status_dev, s);      // (never with a prior or an L1 term: gdmix_fe_set_bounds)
  else with_flag(F.mu != nullptr, [&](auto PR) {
    constexpr bool PRIOR = decltype(PR)::value;
    if (p->fused_tail) {
      hipLaunchKernelGGL(fe_tail_kernel<PRIOR>, dim3(tail_blocks), dim3(FE_THREADS), 0, s, F, p->o, dot_blocks, p->status_dev, p->gen);
    } else {
      hipLaunchKernelGGL(fe_dots_kernel<PRIOR>, dim3(dot_blocks), dim3(FE_THREADS), 0, s, F, p->o);
      hipLaunchKernelGGL(fe_step_kernel, dim3(1), dim3(FE_THREADS), 0, s, F, p->o, dot_blocks, p->status_dev);
      hipLaunchKernelGGL(fe_update_kernel<PRIOR>, dim3(grid_for(F.P, 256, 1024)), dim3(256), 0, s, F, p->o.m);
    }
  });
  p->dirty = false;
  HIP_TRY(hipGetLastError());
  const int slot = (int)(p->seq % FE_RING);
  HIP_TRY(hipMemcpyAsync(p->status_ring.as<int32_t>() + slot, p->status_dev, sizeof(int32_t), hipMemcpyDeviceToHost, s));
  HIP_TRY(hipEventRecord(p->ring_ev[slot], s));
  ++p->seq;
  return GDMIX_RE_OK;
}

GDMIX_API int gdmix_fe_step(gdmix_fe_problem* p, void* stream, int32_t* status) {
  if (!p || !status) { set_error("NULL argument"); return GDMIX_RE_EINVAL; }
  const int rc = fe_enqueue_step(p, static_cast<hipStream_t>(stream));
  if (rc != GDMIX_RE_OK) return rc;
  return gdmix_fe_step_status(p, p->seq - 1, status);
}

GDMIX_API int gdmix_fe_step_async(gdmix_fe_problem* p, void* stream, int64_t* seq) {
  if (!p) { set_error("problem is NULL"); return GDMIX_RE_EINVAL; }
  const int rc = fe_enqueue_step(p, static_cast<hipStream_t>(stream));
  if (rc == GDMIX_RE_OK && seq) *seq = p->seq - 1;
  return rc;
}

GDMIX_API int gdmix_fe_step_status(gdmix_fe_problem* p, int64_t seq, int32_t* status) {
  if (!p || !status) { set_error("NULL argument"); return GDMIX_RE_EINVAL; }
  if (seq < 0 || seq >= p->seq || seq + FE_RING <= p->seq) {
    set_error("step %lld: only the last %d of the %lld enqueued steps can be asked for", (long long)seq, FE_RING, (long long)p->seq);
    return GDMIX_RE_EINVAL;
  }
  const int slot = (int)(seq % FE_RING);
  HIP_TRY(hipEventSynchronize(p->ring_ev[slot]));
  *status = p->status_ring.as<int32_t>()[slot];
  return GDMIX_RE_OK;
}

GDMIX_API int gdmix_fe_solve(gdmix_fe_problem* p, void* stream, int32_t lookahead, int64_t max_evals, int32_t* status, int64_t* evals) {
  if (!p || !status) { set_error("NULL argument"); return GDMIX_RE_EINVAL; }
  if (lookahead < 0 || lookahead >= FE_RING) { set_error("0 <= lookahead < %d", FE_RING); return GDMIX_RE_EINVAL; }
  int32_t st = -1;
  int64_t k = 0;
  for (; k < max_evals + lookahead; ++k) {
    int rc = gdmix_fe_eval(p, stream);
    if (rc == GDMIX_RE_OK) rc = fe_enqueue_step(p, static_cast<hipStream_t>(stream));
    if (rc != GDMIX_RE_OK) return rc;
    if (k >= lookahead) {
      rc = gdmix_fe_step_status(p, p->seq - 1 - lookahead, &st);
      if (rc != GDMIX_RE_OK) return rc;
      if (st >= 0) break;
    }
  }
  // the steps behind the one that stopped were no-ops and report the same status; wait for them so that nothing of this solve is
  // still in flight when the caller reads the result
  if (st >= 0) {
    const int rc = gdmix_fe_step_status(p, p->seq - 1, &st);
    if (rc != GDMIX_RE_OK) return rc;
  }
  *status = st;
  if (evals) *evals = k + 1;
  return GDMIX_RE_OK;
}

GDMIX_API int gdmix_fe_result(gdmix_fe_problem* p, double* theta, double* fval, double* gnorm, int32_t* nit, int32_t* nfev,
                              void* stream) {
  if (!p) { set_error("problem is NULL"); return GDMIX_RE_EINVAL; }
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (theta && p->F.mu) {
    hipLaunchKernelGGL(fe_prior_theta_kernel, dim3(grid_for(p->F.P, 256, 1024)), dim3(256), 0, s, p->F, theta);
    HIP_TRY(hipGetLastError());
  } else if (theta) {
    // under the OWL-QN step and the bounded step W.x is the trial point and W.t the last accepted one (fe_qn.hip)
    HIP_TRY(hipMemcpyAsync(theta, (p->l1 > 0.0 || p->box) ? p->F.W.t : p->F.W.x, (size_t)p->F.P * 8, hipMemcpyDeviceToDevice, s));
  }
  CompactState S;
  HIP_TRY(hipMemcpyAsync(&S, p->F.state, sizeof(S), hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  if (fval) *fval = S.f;
  if (gnorm) *gnorm = S.sbgnrm;
  if (nit) *nit = S.nit;
  if (nfev) *nfev = S.nfev;
  return GDMIX_RE_OK;
}

GDMIX_API int gdmix_fe_score(gdmix_re_ctx* ctx, int64_t n, const int64_t* row_nnz_ptr, const int64_t* col_global, const float* val,
                             const float* offset, const double* theta, int64_t num_features, int has_intercept, float* score,
                             float* per_coord, void* stream) {
  if (!ctx || n < 0 || !theta || !score || !per_coord || num_features < 0) { set_error("bad argument"); return GDMIX_RE_EINVAL; }
  if (row_nnz_ptr && (!col_global || !val)) { set_error("row_nnz_ptr without col_global / val"); return GDMIX_RE_EINVAL; }
  if (n == 0) return GDMIX_RE_OK;
  HIP_TRY(hipSetDevice(ctx->impl.device));
  const int64_t blocks = (n + 255) / 256;
  if (blocks > 0x7fffffffLL) { set_error("too many samples for one launch"); return GDMIX_RE_ERANGE; }
  hipLaunchKernelGGL(fe_score_kernel, dim3((unsigned)blocks), dim3(256), 0, static_cast<hipStream_t>(stream), n, row_nnz_ptr,
                     col_global, val, offset, theta, num_features, has_intercept ? 1 : 0, score, per_coord);
  HIP_TRY(hipGetLastError());
  return GDMIX_RE_OK;
}

GDMIX_API int gdmix_fe_stream_bytes(gdmix_fe_problem* p, int64_t* rows_pass, int64_t* cols_pass) {
  if (!p) { set_error("problem is NULL"); return GDMIX_RE_EINVAL; }
  if (rows_pass) *rows_pass = p->F.rc.stream_bytes;
  if (cols_pass) *cols_pass = p->F.cc.stream_bytes;
  return GDMIX_RE_OK;
}

GDMIX_API int gdmix_fe_last_eval_ms(gdmix_fe_problem* p, float* rows_ms, float* cols_ms) {
  if (!p || !p->timed) { set_error("no evaluation has been timed"); return GDMIX_RE_EINVAL; }
  HIP_TRY(hipEventSynchronize(p->ev[2]));
  if (rows_ms) HIP_TRY(hipEventElapsedTime(rows_ms, p->ev[0], p->ev[1]));
  if (cols_ms) HIP_TRY(hipEventElapsedTime(cols_ms, p->ev[1], p->ev[2]));
  return GDMIX_RE_OK;
}

}  // extern "C"
