// re_tron.hpp — the per-entity trust-region Newton solve (include/gdmix_re.h, "TRON"): the algorithm section of include/gdmix_fe.h,
// "(ABI 24) TRON", applied to one entity's objective (divided by n, intercept first). Written once against the thread-group policy of
// re_solve_core.hpp, as owlqn_solve is: TronWave (one wavefront per entity, block and state in LDS) and TronBlock (one workgroup per
// entity, state in a global scratch slot, X streamed). tests/re_tron_helpers.py restates it in numpy.
//
//   F(theta) = (1/n) ( sum_i w_i l(z_i, y_i) + (l2/2) |theta_R|^2 ),   H v = (1/n) ( X~' (D o X~ v) + l2 v_R )
//
// No history: seven coefficient vectors (x g xt gt s r d; the product's Hd lives in gt, which is free while CG runs) and three sample
// vectors (the residuals of the last evaluation — the product's t_i = D_i (x_i . d) while CG runs —, the accepted point's curvature
// weights D, and the trial point's). An evaluation writes the trial's D beside the residual; acceptance swaps the two D pointers, so a
// rejected trial leaves the accepted point's D in force.
//
// Order of the sums (nothing depends on where in a batch an entity sits or on how many entities the batch has): a row's x_i . v runs over
// the row's CSR entries in storage order from the intercept's term; a column's sum runs over its CSC entries in storage order; thread t of
// the NT cooperating threads adds the samples (coefficients) t, t + NT, ... in that order, the 64 lanes of a wavefront are added by the
// fixed DPP tree of wave_sum, and a workgroup's wavefronts in wavefront order.
//
// Synchronisation: element j of every p-vector is only ever touched by thread j mod NT, so the elementwise passes need no barrier between
// them; a vector is synced before a row pass gathers it across threads (the trial point, the CG direction), and the sample vector between
// a row pass and the column pass that gathers it.
#pragma once
#include "re_solve_core.hpp"

namespace gdmix {

constexpr int RE_TRON_MAX_CG = 50;   // GDMIX_FE_TRON_MAX_CG
constexpr int TRON_P_VECTORS = 7, TRON_N_VECTORS = 3;
constexpr int TRON_PCG_P_VECTORS = TRON_P_VECTORS + 2;   // M and 1/M
constexpr double TRON_PCG_M_FLOOR = 1.0e-12;             // M_j >= this (a = 1, an empty column nothing regularises)

// SolveParams with the preconditioner's weight behind it: what the PCG kernels take where the others take SolveParams
struct TronPcgParams : SolveParams {
  double a;
};

struct TronWork {
  double* x;    // [p] accepted point (the result on exit)
  double* g;    // [p] gradient at x
  double* xt;   // [p] trial point (holds the start point on entry)
  double* gt;   // [p] gradient at xt; Hd while CG runs
  double* s;    // [p] CG iterate: the step
  double* r;    // [p] CG residual
  double* d;    // [p] CG direction
  double* rs;   // [n] per-sample residuals of the last evaluation; t_i of a product
  double* dc;   // [n] D at the accepted point
  double* dt;   // [n] D of the last evaluation (the trial point's)
  double* m;    // [p] PCG only: M at the accepted point
  double* im;   // [p] PCG only: 1 / M
};

struct TronStats {
  double f, gnorm;
  int nit, nfev, nhv, status;
};

// ---- several sums in one reduction ---------------------------------------------------------------------------------------------------
// The DPP steps of wave_sum, taken for N values side by side: the N dependent chains overlap instead of following each other.
template <int N>
__device__ __forceinline__ void wave_sums(double (&v)[N]) {
#pragma unroll
  for (int k = 0; k < N; ++k) v[k] += dpp_get0<0x111, 0xf>(v[k]);
#pragma unroll
  for (int k = 0; k < N; ++k) v[k] += dpp_get0<0x112, 0xf>(v[k]);
#pragma unroll
  for (int k = 0; k < N; ++k) v[k] += dpp_get0<0x114, 0xf>(v[k]);
#pragma unroll
  for (int k = 0; k < N; ++k) v[k] += dpp_get0<0x118, 0xf>(v[k]);
#pragma unroll
  for (int k = 0; k < N; ++k) v[k] += dpp_get0<0x142, 0xa>(v[k]);
#pragma unroll
  for (int k = 0; k < N; ++k) v[k] += dpp_get0<0x143, 0xc>(v[k]);
#pragma unroll
  for (int k = 0; k < N; ++k) v[k] = readlane63(v[k]);
}

constexpr int TRON_SUMS = 6;   // the most values one reduction carries

// PCG keeps the sums of both kernels in ONE order, the workgroup kernel's: thread t of 256 adds the elements t, t + 256, ..., a wavefront's
// 64 threads are added by the tree, the four wavefronts in order. A lane of the wavefront kernel therefore keeps PARTS partial sums — the
// w-th for the elements lane + 64 w + 256 k, what thread 64 w + lane of the workgroup kernel adds — and sums_parts puts each through
// the tree and adds the four as ((0 + 1) + 2) + 3. Up to 64 elements only partial 0 holds any, the others are the +0.0 a wavefront
// without elements contributes. v is [PARTS][N], flat; the totals end in v[0, N).
struct TronWave : WaveGroup {
  static constexpr int PARTS = 4;
  template <int N>
  __device__ __forceinline__ void sums(double (&v)[N]) const { wave_sums(v); }
  template <int N>
  __device__ __forceinline__ void sums_parts(double (&v)[N * PARTS], int count) const {
    if (count <= WAVE) {
      double u[N];
#pragma unroll
      for (int k = 0; k < N; ++k) u[k] = v[k];
      wave_sums(u);
#pragma unroll
      for (int k = 0; k < N; ++k) v[k] = ((u[k] + 0.0) + 0.0) + 0.0;
    } else {
      wave_sums(v);
#pragma unroll
      for (int k = 0; k < N; ++k) v[k] = ((v[k] + v[N + k]) + v[2 * N + k]) + v[3 * N + k];
    }
  }
};

// BlockGroup with a second, wider exchange buffer of its own (double-buffered like `red`: one barrier per reduction).
struct TronBlock : BlockGroup<BLOCK_NW> {
  static constexpr int PARTS = 1;
  double* red_n;   // LDS, 2 * BLOCK_NW * TRON_SUMS doubles
  int phase_n;
  template <int N>
  __device__ __forceinline__ void sums_parts(double (&v)[N], int) { sums(v); }
  template <int N>
  __device__ __forceinline__ void sums(double (&v)[N]) {
    static_assert(N <= TRON_SUMS, "the exchange buffer holds TRON_SUMS values per wavefront");
    wave_sums(v);
    double* buf = red_n + phase_n * (BLOCK_NW * TRON_SUMS);
    phase_n ^= 1;
    if ((tid & (WAVE - 1)) == 0) {
#pragma unroll
      for (int k = 0; k < N; ++k) buf[(tid >> 6) * TRON_SUMS + k] = v[k];
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < N; ++k) {
      double a = buf[k];
#pragma unroll
      for (int w = 1; w < BLOCK_NW; ++w) a += buf[w * TRON_SUMS + k];
      v[k] = a;
    }
  }
};

// ---- the evaluation: eval_fg's two passes, with the curvature weight left beside the residual -------------------------------------------
// returns w l(z, y), writes r = dl/dz and D = d2l/dz2 (both times w). The loss and the residual are loss_terms<LOSS>'s expressions.
template <int LOSS>
__device__ __forceinline__ double tron_terms(double z, double yi, double wi, double& ri, double& di) {
  if constexpr (LOSS == LOSS_SQUARED) {
    di = 2.0 * wi;
    return loss_terms<LOSS>(z, yi, wi, ri);
  } else if constexpr (LOSS == LOSS_POISSON) {
    const double e = exp_any(z);
    ri = wi * (e - yi);
    di = wi * e;
    return wi * (e - yi * z);
  } else {
    const double e = exp_neg(fabs(z));
    const double u = 1.0 + e;
    const double ce = fmax(z, 0.0) - z * yi + log_1_2(u);
    const double ru = rcp_nr(u);
    const double sig = (z >= 0.0) ? ru : e * ru;
    ri = wi * (sig - yi);
    di = wi * ((e * ru) * ru);   // rho (1 - rho) = e / (1 + e)^2 for either sign of z: no cancellation
    return wi * ce;
  }
}

// f at x; the gradient in g, the residuals in rs, the curvature weights in dw.
template <int LOSS, class G>
__device__ __forceinline__ double tron_eval(G& grp, const EntityView& P, const SolveParams& o, const double* __restrict__ x, double* g, double* rs,
                                            double* dw) {
  const int n = P.n, p = P.p, ic = P.ic;
  double part = 0.0, rpart = 0.0;
  const double x0 = ic ? x[0] : 0.0;
  for (int i = grp.tid; i < n; i += grp.NT) {
    double acc = x0;
    const int k1 = P.row_ptr[i + 1];
    for (int k = P.row_ptr[i]; k < k1; ++k) acc += (double)P.csr_val[k] * x[ic + P.csr_col[k]];
    const double z = acc + (double)P.o[i];
    const double wi = P.w ? (double)P.w[i] : 1.0;
    double ri, di;
    part += tron_terms<LOSS>(z, (double)P.y[i], wi, ri, di);
    rs[i] = ri;
    dw[i] = di;
    rpart += ri;
  }
  const int first_reg = (ic && !o.regularize_bias) ? 1 : 0;
  double sq = 0.0;
  for (int j = first_reg + grp.tid; j < p; j += grp.NT) sq += x[j] * x[j];
  const double inv_n = 1.0 / (double)n;
  double v[3] = {part, sq, rpart};
  grp.sums(v);
  const double f = inv_n * (v[0] + 0.5 * o.l2 * v[1]);
  grp.sync();   // the column pass gathers rs across threads
  for (int j = grp.tid; j < p; j += grp.NT) {
    double acc;
    if (ic && j == 0) {
      acc = v[2];
    } else {
      acc = 0.0;
      const int c = j - ic;
      const int k1 = P.col_ptr[c + 1];
      for (int k = P.col_ptr[c]; k < k1; ++k) acc += (double)P.csc_val[k] * rs[P.csc_row[k]];
    }
    g[j] = inv_n * (acc + ((j < first_reg) ? 0.0 : o.l2 * x[j]));
  }
  grp.sync();
  return f;
}

// tron_eval for PCG: the sum of the curvature weights (the intercept's diagonal entry) in *dsum, a fourth value of the evaluation's own
// reduction, and the sums in sums_parts' order.
template <int LOSS, class G>
__device__ __forceinline__ double tron_pcg_eval(G& grp, const EntityView& P, const SolveParams& o, const double* __restrict__ x, double* g, double* rs,
                                            double* dw, double* dsum) {
  const int n = P.n, p = P.p, ic = P.ic;
  constexpr int PW = G::PARTS;   // partial sums a thread keeps (TronWave::sums_parts)
  double part[PW] = {}, rpart[PW] = {};
  double dpart[PW] = {};
  const double x0 = ic ? x[0] : 0.0;
#pragma unroll
  for (int w = 0; w < PW; ++w)
  for (int i = grp.tid + w * grp.NT; i < n; i += PW * grp.NT) {
    double acc = x0;
    const int k1 = P.row_ptr[i + 1];
    for (int k = P.row_ptr[i]; k < k1; ++k) acc += (double)P.csr_val[k] * x[ic + P.csr_col[k]];
    const double z = acc + (double)P.o[i];
    const double wi = P.w ? (double)P.w[i] : 1.0;
    double ri, di;
    part[w] += tron_terms<LOSS>(z, (double)P.y[i], wi, ri, di);
    rs[i] = ri;
    dw[i] = di;
    rpart[w] += ri;
    dpart[w] += di;
  }
  const int first_reg = (ic && !o.regularize_bias) ? 1 : 0;
  double sq[PW] = {};
#pragma unroll
  for (int w = 0; w < PW; ++w)
    for (int j = first_reg + grp.tid + w * grp.NT; j < p; j += PW * grp.NT) sq[w] += x[j] * x[j];
  const double inv_n = 1.0 / (double)n;
  double v[4 * PW];
#pragma unroll
  for (int w = 0; w < PW; ++w) { v[4 * w] = part[w]; v[4 * w + 1] = sq[w]; v[4 * w + 2] = rpart[w]; v[4 * w + 3] = dpart[w]; }
  grp.template sums_parts<4>(v, n > p ? n : p);
  *dsum = v[3];
  const double f = inv_n * (v[0] + 0.5 * o.l2 * v[1]);
  grp.sync();   // the column pass gathers rs across threads
  for (int j = grp.tid; j < p; j += grp.NT) {
    double acc;
    if (ic && j == 0) {
      acc = v[2];
    } else {
      acc = 0.0;
      const int c = j - ic;
      const int k1 = P.col_ptr[c + 1];
      for (int k = P.col_ptr[c]; k < k1; ++k) acc += (double)P.csc_val[k] * rs[P.csc_row[k]];
    }
    g[j] = inv_n * (acc + ((j < first_reg) ? 0.0 : o.l2 * x[j]));
  }
  grp.sync();
  return f;
}

// h = H d: a row pass t_i = D_i (x_i . d) over the CSR copy, a column pass h_j = sum_i t_i x_ij over the CSC copy — no exp, no log, no
// reciprocal. d must be synced before; h[j] is written by thread j mod NT and needs no sync for the elementwise passes behind it.
template <class G>
__device__ __forceinline__ void tron_product(G& grp, const EntityView& P, const SolveParams& o, const double* __restrict__ d, const double* dw, double* t,
                                             double* h) {
  const int n = P.n, p = P.p, ic = P.ic;
  const double d0 = ic ? d[0] : 0.0;
  double tpart = 0.0;
  for (int i = grp.tid; i < n; i += grp.NT) {
    double acc = d0;
    const int k1 = P.row_ptr[i + 1];
    for (int k = P.row_ptr[i]; k < k1; ++k) acc += (double)P.csr_val[k] * d[ic + P.csr_col[k]];
    const double ti = dw[i] * acc;
    t[i] = ti;
    tpart += ti;
  }
  const double tsum = ic ? grp.sum(tpart) : 0.0;   // the intercept's column is all ones
  grp.sync();
  const int first_reg = (ic && !o.regularize_bias) ? 1 : 0;
  const double inv_n = 1.0 / (double)n;
  for (int j = grp.tid; j < p; j += grp.NT) {
    double acc;
    if (ic && j == 0) {
      acc = tsum;
    } else {
      acc = 0.0;
      const int c = j - ic;
      const int k1 = P.col_ptr[c + 1];
      for (int k = P.col_ptr[c]; k < k1; ++k) acc += (double)P.csc_val[k] * t[P.csc_row[k]];
    }
    h[j] = inv_n * (acc + ((j < first_reg) ? 0.0 : o.l2 * d[j]));
  }
}

// tron_product for PCG (the sums in sums_parts' order): a row pass t_i = D_i (x_i . d) over the CSR copy, a column pass h_j = sum_i t_i x_ij over the CSC copy — no exp, no log, no
// reciprocal. d must be synced before; h[j] is written by thread j mod NT and needs no sync for the elementwise passes behind it.
template <class G>
__device__ __forceinline__ void tron_pcg_product(G& grp, const EntityView& P, const SolveParams& o, const double* __restrict__ d, const double* dw, double* t,
                                             double* h) {
  const int n = P.n, p = P.p, ic = P.ic;
  const double d0 = ic ? d[0] : 0.0;
  constexpr int PW = G::PARTS;
  double tpart[PW] = {};
#pragma unroll
  for (int w = 0; w < PW; ++w)
  for (int i = grp.tid + w * grp.NT; i < n; i += PW * grp.NT) {
    double acc = d0;
    const int k1 = P.row_ptr[i + 1];
    for (int k = P.row_ptr[i]; k < k1; ++k) acc += (double)P.csr_val[k] * d[ic + P.csr_col[k]];
    const double ti = dw[i] * acc;
    t[i] = ti;
    tpart[w] += ti;
  }
  double tsum = 0.0;   // the intercept's column is all ones
  if (ic) { grp.template sums_parts<1>(tpart, n); tsum = tpart[0]; }
  grp.sync();
  const int first_reg = (ic && !o.regularize_bias) ? 1 : 0;
  const double inv_n = 1.0 / (double)n;
  for (int j = grp.tid; j < p; j += grp.NT) {
    double acc;
    if (ic && j == 0) {
      acc = tsum;
    } else {
      acc = 0.0;
      const int c = j - ic;
      const int k1 = P.col_ptr[c + 1];
      for (int k = P.col_ptr[c]; k < k1; ++k) acc += (double)P.csc_val[k] * t[P.csc_row[k]];
    }
    h[j] = inv_n * (acc + ((j < first_reg) ? 0.0 : o.l2 * d[j]));
  }
}

// |g|_inf and g'g of the accepted point
template <class G>
__device__ __forceinline__ void tron_gradient_norms(G& grp, int p, const double* g, double& gmax, double& gg) {
  double mx = 0.0, sq = 0.0;
  for (int j = grp.tid; j < p; j += grp.NT) {
    const double gj = g[j];
    mx = fmax(mx, fabs(gj));
    sq += gj * gj;
  }
  gmax = grp.max_nonneg(mx);
  gg = grp.sum(sq);
}

// The preconditioner at the accepted point, and the point's norms in it: M_j = max((1 - a) + a H_jj, floor), H_jj = (1/n) ( sum_k D_row(k)
// x_k^2 over column j's CSC entries in storage order + l2 [j in R] ), the intercept's column all ones (dsum, from the evaluation). A
// column pass: thread j mod NT owns column j, reads D by row index, writes M_j and its one reciprocal and adds its g_j^2 / M_j — no
// row pass, no exp, nothing per sample but a multiply-add. dw was synced by the evaluation that wrote it; m and im need no sync (their
// element j is thread j mod NT's). -> |g|_inf and g' M^-1 g.
template <class G>
__device__ __forceinline__ void tron_pcg_diagonal(G& grp, const EntityView& P, const TronPcgParams& o, const double* dw, double dsum, const double* g,
                                                  double* m, double* im, double& gmax, double& gmg) {
  const int n = P.n, p = P.p, ic = P.ic;
  const int first_reg = (ic && !o.regularize_bias) ? 1 : 0;
  const double inv_n = 1.0 / (double)n, a = o.a, b = 1.0 - o.a;
  double mx = 0.0, sq[G::PARTS] = {};
#pragma unroll
  for (int w = 0; w < G::PARTS; ++w)
  for (int j = grp.tid + w * grp.NT; j < p; j += G::PARTS * grp.NT) {
    double acc;
    if (ic && j == 0) {
      acc = dsum;
    } else {
      acc = 0.0;
      const int c = j - ic;
      const int k1 = P.col_ptr[c + 1];
      for (int k = P.col_ptr[c]; k < k1; ++k) {
        const double xv = (double)P.csc_val[k];
        acc += (xv * xv) * dw[P.csc_row[k]];
      }
    }
    const double hjj = inv_n * (acc + ((j < first_reg) ? 0.0 : o.l2));
    const double mj = fmax(b + a * hjj, TRON_PCG_M_FLOOR);
    const double imj = 1.0 / mj;
    m[j] = mj;
    im[j] = imj;
    const double gj = g[j];
    mx = fmax(mx, fabs(gj));
    sq[w] += (gj * gj) * imj;
  }
  gmax = grp.max_nonneg(mx);
  grp.template sums_parts<1>(sq, p);
  gmg = sq[0];
}

// The whole solve of one entity. On entry W.xt holds the start point; on exit W.x is the last accepted point (never a rejected trial),
// W.dc its curvature weights, and W.rs is free.
// PCG (PT = TronPcgParams): gg is g' M^-1 g, rr is r'z, every |.|^2 of s and d is taken in M, and M follows the accepted point.
template <int LOSS, bool PCG = false, class G, class PT>
__device__ void tron_solve(G& grp, const EntityView& P, const PT& o, TronWork& W, TronStats& st) {
  const int p = P.p;
  [[maybe_unused]] double dsum = 0.0;   // sum of D at the last evaluated point
  double F;
  if constexpr (PCG) F = tron_pcg_eval<LOSS>(grp, P, o, W.xt, W.gt, W.rs, W.dt, &dsum);
  else F = tron_eval<LOSS>(grp, P, o, W.xt, W.gt, W.rs, W.dt);
  { double* t = W.x; W.x = W.xt; W.xt = t; t = W.g; W.g = W.gt; W.gt = t; t = W.dc; W.dc = W.dt; W.dt = t; }
  int nfev = 1, nit = 0, nhv = 0, status = -1, rejected = 0;
  bool moved = false;
  double gmax, gg;
  if constexpr (PCG) tron_pcg_diagonal(grp, P, o, W.dc, dsum, W.g, W.m, W.im, gmax, gg);
  else tron_gradient_norms(grp, p, W.g, gmax, gg);
  if (gmax <= o.pgtol) status = 0;
  double delta = sqrt(gg);

  while (status < 0) {
    // Steihaug CG on the model at (x, g, D): s = 0, r = -g, d = r
    const double gnorm = sqrt(gg);
    for (int j = grp.tid; j < p; j += grp.NT) {
      const double gj = W.g[j];
      W.s[j] = 0.0;
      W.r[j] = -gj;
      if constexpr (PCG) W.d[j] = -gj * W.im[j];
      else W.d[j] = -gj;
    }
    grp.sync();   // the product gathers d across threads
    double rr = gg;
    double* const h = W.gt;
    for (int ncg = 1;; ++ncg) {
      if constexpr (PCG) tron_pcg_product(grp, P, o, W.d, W.dc, W.rs, h);
      else tron_product(grp, P, o, W.d, W.dc, W.rs, h);
      ++nhv;
      double v[PCG ? 6 * G::PARTS : 6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};   // d'Hd r'Hd |Hd|^2 s'd |s|^2 |d|^2
      if constexpr (PCG) {   // d'Hd z'Hd |Hd|^2 in 1/M; s'Md s'Ms d'Md: the same six sums, one reduction, in sums_parts' order
#pragma unroll
        for (int w = 0; w < G::PARTS; ++w)
          for (int j = grp.tid + w * grp.NT; j < p; j += G::PARTS * grp.NT) {
            const double dj = W.d[j], hj = h[j], sj = W.s[j];
            const double mj = W.m[j], hz = hj * W.im[j], md = mj * dj;
            v[6 * w] += dj * hj;
            v[6 * w + 1] += W.r[j] * hz;
            v[6 * w + 2] += hj * hz;
            v[6 * w + 3] += sj * md;
            v[6 * w + 4] += (sj * sj) * mj;
            v[6 * w + 5] += dj * md;
          }
        grp.template sums_parts<6>(v, p);
      } else {
        for (int j = grp.tid; j < p; j += grp.NT) {
          const double dj = W.d[j], hj = h[j], sj = W.s[j];
          v[0] += dj * hj;
          v[1] += W.r[j] * hj;
          v[2] += hj * hj;
          v[3] += sj * dj;
          v[4] += sj * sj;
          v[5] += dj * dj;
        }
        grp.sums(v);
      }
      const double dhd = v[0], rh = v[1], hh = v[2], sd = v[3], ss = v[4], dd = v[5];
      const double alpha = rr / dhd;
      if (!(dhd > 0.0) || ss + 2.0 * alpha * sd + alpha * alpha * dd > delta * delta) {
        // to the boundary: the non-negative root of |s + tau d| = Delta, in the form without cancellation for either sign of s'd
        const double gap = fmax(delta * delta - ss, 0.0);
        const double rad = sqrt(sd * sd + dd * gap);
        const double tau = sd >= 0.0 ? gap / (sd + rad) : (rad - sd) / dd;
        for (int j = grp.tid; j < p; j += grp.NT) {
          W.s[j] += tau * W.d[j];
          W.r[j] -= tau * h[j];
        }
        break;
      }
      const double rr_new = fmax(rr - 2.0 * alpha * rh + alpha * alpha * hh, 0.0);
      const bool last = sqrt(rr_new) <= 0.1 * gnorm || ncg >= RE_TRON_MAX_CG;
      const double beta = rr_new / rr;   // known before the update: one pass moves s, r and d
      for (int j = grp.tid; j < p; j += grp.NT) {
        const double dj = W.d[j];
        const double rj = W.r[j] - alpha * h[j];
        W.s[j] += alpha * dj;
        W.r[j] = rj;
        if constexpr (PCG) {
          if (!last) W.d[j] = rj * W.im[j] + beta * dj;
        } else {
          if (!last) W.d[j] = rj + beta * dj;
        }
      }
      if (last) break;
      rr = rr_new;
      grp.sync();
    }

    // the trial point, g's, |s|^2 and s'r: one pass, one reduction
    double v[PCG ? 3 * G::PARTS : 3] = {0.0, 0.0, 0.0};
    if constexpr (PCG) {
#pragma unroll
      for (int w = 0; w < G::PARTS; ++w)
        for (int j = grp.tid + w * grp.NT; j < p; j += G::PARTS * grp.NT) {
          const double sj = W.s[j];
          W.xt[j] = W.x[j] + sj;
          v[3 * w] += W.g[j] * sj;
          v[3 * w + 1] += (sj * sj) * W.m[j];
          v[3 * w + 2] += sj * W.r[j];
        }
      grp.template sums_parts<3>(v, p);
    } else {
      for (int j = grp.tid; j < p; j += grp.NT) {
        const double sj = W.s[j];
        W.xt[j] = W.x[j] + sj;
        v[0] += W.g[j] * sj;
        v[1] += sj * sj;
        v[2] += sj * W.r[j];
      }
      grp.sums(v);
    }
    const double gs = v[0], snorm = sqrt(v[1]);
    const double prered = -0.5 * (gs - v[2]);
    grp.sync();   // the evaluation gathers xt across threads
    [[maybe_unused]] double dsum_t = 0.0;
    double Ft_;
    if constexpr (PCG) Ft_ = tron_pcg_eval<LOSS>(grp, P, o, W.xt, W.gt, W.rs, W.dt, &dsum_t);
    else Ft_ = tron_eval<LOSS>(grp, P, o, W.xt, W.gt, W.rs, W.dt);
    const double Ft = Ft_;
    ++nfev;
    const double actred = F - Ft;
    if (!moved) delta = fmin(delta, snorm);
    const double curv = Ft - F - gs;
    const double ah = curv <= 0.0 ? 4.0 : fmax(0.25, -0.5 * (gs / curv));
    if (!(actred >= 1.0e-4 * prered)) delta = fmin(fmax(ah, 0.25) * snorm, 0.5 * delta);
    else if (actred < 0.25 * prered) delta = fmax(0.25 * delta, fmin(ah * snorm, 0.5 * delta));
    else if (actred < 0.75 * prered) delta = fmax(0.25 * delta, fmin(ah * snorm, 4.0 * delta));
    else delta = fmax(delta, fmin(ah * snorm, 4.0 * delta));
    if (actred > 1.0e-4 * prered) {
      { double* t = W.x; W.x = W.xt; W.xt = t; t = W.g; W.g = W.gt; W.gt = t; t = W.dc; W.dc = W.dt; W.dt = t; }
      const double Fold = F;
      F = Ft;
      ++nit;
      moved = true;
      rejected = 0;
      if constexpr (PCG) tron_pcg_diagonal(grp, P, o, W.dc, dsum_t, W.g, W.m, W.im, gmax, gg);
      else tron_gradient_norms(grp, p, W.g, gmax, gg);
      if (gmax <= o.pgtol) status = 0;
      else if (Fold - F <= o.ftol * fmax(fabs(Fold), fmax(fabs(F), 1.0))) status = 1;
      else if (nit >= o.max_iter) status = 2;
      else if (nfev > o.maxfun) status = 3;
    } else {
      ++rejected;
      if (nfev > o.maxfun) status = 3;
      else if (rejected >= o.maxls) status = 4;
    }
  }
  grp.sync();
  st.f = F;
  st.gnorm = gmax;
  st.nit = nit;
  st.nfev = nfev;
  st.nhv = nhv;
  st.status = status;
}

// SIMPLE variance at the returned theta: variance_simple's arithmetic (duplicates of one matrix cell summed before squaring) on the
// curvature weights the solve left in D — no second pass over exp.
template <class G>
__device__ __forceinline__ void tron_variance_simple(G& grp, const EntityView& P, const SolveParams& o, const double* D, double* var_out) {
  const int n = P.n, p = P.p, ic = P.ic;
  double dpart = 0.0;
  for (int i = grp.tid; i < n; i += grp.NT) dpart += D[i];
  const double dsum = grp.sum(dpart);
  const int first_reg = (ic && !o.regularize_bias) ? 1 : 0;
  for (int j = grp.tid; j < p; j += grp.NT) {
    double h;
    if (ic && j == 0) {
      h = dsum;
    } else {
      h = 0.0;
      const int c = j - ic;
      const int k1 = P.col_ptr[c + 1];
      int k = P.col_ptr[c];
      while (k < k1) {
        const int row = P.csc_row[k];
        double v = (double)P.csc_val[k];
        ++k;
        while (k < k1 && P.csc_row[k] == row) { v += (double)P.csc_val[k]; ++k; }
        h += v * v * D[row];
      }
    }
    h += (j < first_reg) ? 0.0 : o.l2;
    var_out[j] = 1.0 / (h + 1.0e-12);
  }
  grp.sync();
}

}  // namespace gdmix
