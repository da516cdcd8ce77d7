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

struct TronWave : WaveGroup {
  template <int N>
  __device__ __forceinline__ void sums(double (&v)[N]) const { wave_sums(v); }
};

// BlockGroup with a second, wider exchange buffer of its own (double-buffered like `red`: one barrier per reduction).
struct TronBlock : BlockGroup<BLOCK_NW> {
  double* red_n;   // LDS, 2 * BLOCK_NW * TRON_SUMS doubles
  int phase_n;
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

// The whole solve of one entity. On entry W.xt holds the start point; on exit W.x is the last accepted point (never a rejected trial),
// W.dc its curvature weights, and W.rs is free.
template <int LOSS, class G>
__device__ void tron_solve(G& grp, const EntityView& P, const SolveParams& o, TronWork& W, TronStats& st) {
  const int p = P.p;
  double F = tron_eval<LOSS>(grp, P, o, W.xt, W.gt, W.rs, W.dt);
  { double* t = W.x; W.x = W.xt; W.xt = t; t = W.g; W.g = W.gt; W.gt = t; t = W.dc; W.dc = W.dt; W.dt = t; }
  int nfev = 1, nit = 0, nhv = 0, status = -1, rejected = 0;
  bool moved = false;
  double gmax, gg;
  tron_gradient_norms(grp, p, W.g, gmax, gg);
  if (gmax <= o.pgtol) status = 0;
  double delta = sqrt(gg);

  while (status < 0) {
    // Steihaug CG on the model at (x, g, D): s = 0, r = -g, d = r
    const double gnorm = sqrt(gg);
    for (int j = grp.tid; j < p; j += grp.NT) {
      const double gj = W.g[j];
      W.s[j] = 0.0;
      W.r[j] = -gj;
      W.d[j] = -gj;
    }
    grp.sync();   // the product gathers d across threads
    double rr = gg;
    double* const h = W.gt;
    for (int ncg = 1;; ++ncg) {
      tron_product(grp, P, o, W.d, W.dc, W.rs, h);
      ++nhv;
      double v[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};   // d'Hd r'Hd |Hd|^2 s'd |s|^2 |d|^2
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
        if (!last) W.d[j] = rj + beta * dj;
      }
      if (last) break;
      rr = rr_new;
      grp.sync();
    }

    // the trial point, g's, |s|^2 and s'r: one pass, one reduction
    double v[3] = {0.0, 0.0, 0.0};
    for (int j = grp.tid; j < p; j += grp.NT) {
      const double sj = W.s[j];
      W.xt[j] = W.x[j] + sj;
      v[0] += W.g[j] * sj;
      v[1] += sj * sj;
      v[2] += sj * W.r[j];
    }
    grp.sums(v);
    const double gs = v[0], snorm = sqrt(v[1]);
    const double prered = -0.5 * (gs - v[2]);
    grp.sync();   // the evaluation gathers xt across threads
    const double Ft = tron_eval<LOSS>(grp, P, o, W.xt, W.gt, W.rs, W.dt);
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
      tron_gradient_norms(grp, p, W.g, gmax, gg);
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
