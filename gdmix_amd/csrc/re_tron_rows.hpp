// re_tron_rows.hpp — the trust-region Newton solve with FOUR ENTITIES PER WAVEFRONT: each DPP row (16 lanes) solves one entity
// (re_tron_rows_kernel of re_tron_rows.hip; include/gdmix_re.h, "TRON"). For the entities whose whole TRON footprint is a few KB — 16 samples
// and ~63 coefficients on the C2 shape — the one-entity wavefront kernel leaves 48 lanes of a row pass idle and pays six DPP stages and a
// v_readlane per reduction; here a reduction is the four within-row stages of re_solve_quad.hpp and every instruction serves four entities.
//
// Work split: sample i and coefficient j of an entity belong to lane (i mod 16) and (j mod 16) of its row; every loop strides by 16, so
// n and p are bounded by the LDS footprint alone. A row's LDS block has the carve-up of re_tron_wave_kernel (solver_lds_bytes at m = 0);
// the row's pointers are per-lane values that happen to be equal inside a row, as is everything uniform per entity: the butterflies give
// all 16 lanes the same bits, so a branch on such a value takes whole rows.
//
// Control: tron_solve (re_tron.hpp) cut at its two pass kinds, as lbfgs_advance cuts L-BFGS. A trip of the main loop is ONE pass pair for
// every live row at once — a row pass over the CSR copy, a column pass over the CSC copy — whether the row needs an evaluation (gathers
// the trial point, tron_terms per sample, the gradient into gt) or a product (gathers d, t_i = D_i (x_i . d), Hd into gt): the loops and
// the arrays are the same, only the gathered vector and the per-sample function differ. tron_rows_advance then runs the row's scalar
// logic — the CG update, the boundary exit, the 0.1 |g| exit and the cap; the predicted against the actual reduction, acceptance, the
// radius and the stops — until the row needs its next pass pair or has stopped.
//
// Order of the sums: that of the one-entity wavefront kernel, so an entity's bits do not depend on which of the two kernels solves it.
// There thread t of 64 adds the elements t, t + 64, ... and the lanes are added by the tree of wave_sum: within a DPP row pairs, quads,
// halves, the row; then (row 3 + row 2) + (row 1 + row 0). Here lane l of a row keeps four partials, one per k = 0..3 for the elements
// l + 16 k, l + 16 k + 64, ... — the partial of that kernel's lane 16 k + l — each is summed over the row by the butterfly (the same
// tree: an addition's operands commute), and the four row sums are added as (k3 + k2) + (k1 + k0). A partial that no element reaches is
// +0.0 as the idle lane's was. Where no row of the wavefront has more than 16 elements only k = 0 is carried (x + 0.0 is x: no partial
// is ever -0.0, each starts at +0.0).
#pragma once
#include "re_solve_quad.hpp"
#include "re_tron.hpp"

namespace gdmix {

constexpr int TRON_ROWS = WAVE / ROW;   // entities per wavefront

// ---- reductions -------------------------------------------------------------------------------------------------------------------------
// The butterfly of row_sum for N values side by side: the N dependent chains overlap.
template <int N>
__device__ __forceinline__ void row_sums(double (&v)[N]) {
#define GDMIX_ROWS_STAGE(CTRL)                                 \
  {                                                            \
    double t[N];                                               \
    _Pragma("unroll") for (int a = 0; a < N; ++a) t[a] = dpp_row<CTRL>(v[a]); \
    _Pragma("unroll") for (int a = 0; a < N; ++a) v[a] += t[a];               \
  }
  GDMIX_ROWS_STAGE(0xB1) GDMIX_ROWS_STAGE(0x4E) GDMIX_ROWS_STAGE(0x141) GDMIX_ROWS_STAGE(0x140)
#undef GDMIX_ROWS_STAGE
}

// N sums in the wavefront kernel's order from the four partials per lane (the header). one: no row of the wavefront has more than 16
// elements of this kind (wavefront-uniform).
template <int N>
__device__ __forceinline__ void rows_wave_sums(double (&q)[N][TRON_ROWS], bool one, double (&v)[N]) {
#pragma unroll
  for (int a = 0; a < N; ++a) v[a] = q[a][0];
  row_sums(v);
  if (one) return;
  double k1[N], k2[N], k3[N];
#pragma unroll
  for (int a = 0; a < N; ++a) { k1[a] = q[a][1]; k2[a] = q[a][2]; k3[a] = q[a][3]; }
  row_sums(k1);
  row_sums(k2);
  row_sums(k3);
#pragma unroll
  for (int a = 0; a < N; ++a) v[a] = (k3[a] + k2[a]) + (k1[a] + v[a]);
}

__device__ __forceinline__ double row_max_nonneg(double v) {
  v = fmax(v, dpp_row<0xB1>(v));
  v = fmax(v, dpp_row<0x4E>(v));
  v = fmax(v, dpp_row<0x141>(v));
  v = fmax(v, dpp_row<0x140>(v));
  return v;
}

// f(j, k) for the lane's elements j of [start, end), k the partial j belongs to: j = start + rl + 16 k + 64 t, t ascending per k
template <class F>
__device__ __forceinline__ void rows_each(int start, int end, int rl, F&& f) {
  for (int j0 = start + rl; j0 < end; j0 += WAVE) {
#pragma unroll
    for (int k = 0; k < TRON_ROWS; ++k) {
      const int j = j0 + ROW * k;
      if (j < end) f(j, k);
    }
  }
}

// ---- the state machine ------------------------------------------------------------------------------------------------------------------
enum { TRON_ROW_FIRST = 0, TRON_ROW_PRODUCT = 1, TRON_ROW_TRIAL = 2, TRON_ROW_DONE = 3 };   // what the row's next pass pair is for

// tron_solve's locals: per-lane values, equal inside a row
struct TronRowState {
  int phase, ncg, nit, nfev, nhv, status, rejected;
  bool moved;
  double F, delta, gg, gmax, gnorm, rr, gs, snorm, prered;
};

// one row's entity: per-lane values, equal inside a row
struct TronRowView {
  EntityView P;
  TronWork W;
  bool has_w;
};

// |g|_inf and g'g of the accepted point (tron_gradient_norms)
__device__ __forceinline__ void tron_rows_norms(const TronRowView& V, int rl, bool p_one, double& gmax, double& gg) {
  double mx = 0.0, q[1][TRON_ROWS] = {};
  rows_each(0, V.P.p, rl, [&](int j, int k) {
    const double gj = V.W.g[j];
    mx = fmax(mx, fabs(gj));
    q[0][k] += gj * gj;
  });
  double v[1];
  rows_wave_sums(q, p_one, v);
  gmax = row_max_nonneg(mx);
  gg = v[0];
}

// The row pass and the column pass of every live row: an evaluation at xt (n f returned: the loss and the regulariser before the 1/n;
// residuals in rs, curvature weights in dt, the gradient in gt) or a product of d (t in rs, Hd in gt). tron_eval and tron_product of
// re_tron.hpp, one loop nest for both.
template <int LOSS>
__device__ __forceinline__ double tron_rows_pass(const TronRowView& V, const SolveParams& o, int rl, int phase, bool n_one, bool p_one) {
  const EntityView& P = V.P;
  const TronWork& W = V.W;
  const int n = P.n, p = P.p, ic = P.ic;
  const bool live = phase != TRON_ROW_DONE, isev = phase != TRON_ROW_PRODUCT;
  const double* const vec = isev ? W.xt : W.d;
  const int first_reg = (ic && !o.regularize_bias) ? 1 : 0;
  double qn[2][TRON_ROWS] = {}, qp[1][TRON_ROWS] = {};   // the loss and the residuals (the product's t) over the samples; |x_R|^2
  if (live) {
    const double v0 = ic ? vec[0] : 0.0;
    int k = 0;
    for (int i = rl; i < n; i += ROW, k = (k + 1) & (TRON_ROWS - 1)) {
      double acc = v0;
      const int k1 = P.row_ptr[i + 1];
      for (int c = P.row_ptr[i]; c < k1; ++c) acc += (double)P.csr_val[c] * vec[ic + P.csr_col[c]];
      // the partials this sample belongs to, picked before and put back behind the additions: the additions themselves are written as
      // tron_eval and tron_product write them, so that the compiler contracts the same products into them
      double part = qn[0][0], rpart = qn[1][0];
#pragma unroll
      for (int a = 1; a < TRON_ROWS; ++a) {
        part = (a == k) ? qn[0][a] : part;
        rpart = (a == k) ? qn[1][a] : rpart;
      }
      if (isev) {
        const double z = acc + (double)P.o[i];
        const double wi = V.has_w ? (double)P.w[i] : 1.0;
        double ri, di;
        part += tron_terms<LOSS>(z, (double)P.y[i], wi, ri, di);
        W.rs[i] = ri;
        W.dt[i] = di;
        rpart += ri;
      } else {
        const double ti = W.dc[i] * acc;
        W.rs[i] = ti;
        rpart += ti;
      }
#pragma unroll
      for (int a = 0; a < TRON_ROWS; ++a) {
        qn[0][a] = (a == k) ? part : qn[0][a];
        qn[1][a] = (a == k) ? rpart : qn[1][a];
      }
    }
    if (isev) {
      rows_each(first_reg, p, rl, [&](int j, int a) { qp[0][a] += vec[j] * vec[j]; });
    }
  }
  double vn[2], vp[1];
  rows_wave_sums(qn, n_one, vn);
  rows_wave_sums(qp, p_one, vp);
  const double inv_n = 1.0 / (double)n;
  const double nf = vn[0] + 0.5 * o.l2 * vp[0];
  wave_lds_fence();   // the column pass gathers rs across the row's lanes
  if (live) {
    for (int j = rl; j < p; j += ROW) {
      double acc;
      if (ic && j == 0) {
        acc = vn[1];
      } else {
        acc = 0.0;
        const int c = j - ic;
        const int k1 = P.col_ptr[c + 1];
        for (int a = P.col_ptr[c]; a < k1; ++a) acc += (double)P.csc_val[a] * W.rs[P.csc_row[a]];
      }
      W.gt[j] = inv_n * (acc + ((j < first_reg) ? 0.0 : o.l2 * vec[j]));
    }
  }
  return nf;
}

// The row's scalar logic behind a pass pair, until it needs the next one or has stopped. nf: what tron_rows_pass returned.
// Element j of every p-vector is only ever touched by lane j mod 16 of the row, so the elementwise passes here need no fence; the
// caller fences before the next row pass gathers xt or d.
__device__ __forceinline__ void tron_rows_advance(TronRowView& V, const SolveParams& o, int rl, bool p_one, double nf, TronRowState& S) {
  TronWork& W = V.W;
  const int p = V.P.p;
  if (S.phase == TRON_ROW_PRODUCT) {
    // ---- a CG step on the model at (x, g, D): Hd is in gt
    double* const h = W.gt;
    ++S.nhv;
    double q[6][TRON_ROWS] = {};   // d'Hd r'Hd |Hd|^2 s'd |s|^2 |d|^2
    rows_each(0, p, rl, [&](int j, int k) {
      const double dj = W.d[j], hj = h[j], sj = W.s[j];
      q[0][k] += dj * hj;
      q[1][k] += W.r[j] * hj;
      q[2][k] += hj * hj;
      q[3][k] += sj * dj;
      q[4][k] += sj * sj;
      q[5][k] += dj * dj;
    });
    double v[6];
    rows_wave_sums(q, p_one, v);
    const double dhd = v[0], rh = v[1], hh = v[2], sd = v[3], ss = v[4], dd = v[5];
    const double delta = S.delta, rr = S.rr;
    const double alpha = rr / dhd;
    bool ended;
    if (!(dhd > 0.0) || ss + 2.0 * alpha * sd + alpha * alpha * dd > delta * delta) {
      // to the boundary: the non-negative root of |s + tau d| = Delta, in the form without cancellation for either sign of s'd
      const double gap = fmax(delta * delta - ss, 0.0);
      const double rad = sqrt(sd * sd + dd * gap);
      const double tau = sd >= 0.0 ? gap / (sd + rad) : (rad - sd) / dd;
      for (int j = rl; j < p; j += ROW) {
        W.s[j] += tau * W.d[j];
        W.r[j] -= tau * h[j];
      }
      ended = true;
    } else {
      const double rr_new = fmax(rr - 2.0 * alpha * rh + alpha * alpha * hh, 0.0);
      const bool last = sqrt(rr_new) <= 0.1 * S.gnorm || S.ncg >= RE_TRON_MAX_CG;
      const double beta = rr_new / rr;   // known before the update: one pass moves s, r and d
      for (int j = rl; j < p; j += ROW) {
        const double dj = W.d[j];
        const double rj = W.r[j] - alpha * h[j];
        W.s[j] += alpha * dj;
        W.r[j] = rj;
        if (!last) W.d[j] = rj + beta * dj;
      }
      ended = last;
      S.rr = rr_new;
      ++S.ncg;
    }
    if (ended) {
      // the trial point, g's, |s|^2 and s'r: one pass, one reduction
      double t[3][TRON_ROWS] = {};
      rows_each(0, p, rl, [&](int j, int k) {
        const double sj = W.s[j];
        W.xt[j] = W.x[j] + sj;
        t[0][k] += W.g[j] * sj;
        t[1][k] += sj * sj;
        t[2][k] += sj * W.r[j];
      });
      double u[3];
      rows_wave_sums(t, p_one, u);
      S.gs = u[0];
      S.snorm = sqrt(u[1]);
      S.prered = -0.5 * (u[0] - u[2]);
      S.phase = TRON_ROW_TRIAL;
    }
    return;
  }
  if (S.phase == TRON_ROW_DONE) return;
  // ---- behind an evaluation: the first one, or a trial point's
  bool accepted;
  const bool first = S.phase == TRON_ROW_FIRST;
  // f = (1/n) nf, rounded here. In tron_solve the compiler contracts that product into Ft - F of `curv` (one rounding fewer) and into
  // nothing else; the radius an iteration leaves depends on it, so the same is written out below.
  const double inv_n = 1.0 / (double)V.P.n;
  double f = inv_n * nf;
  asm("" : "+v"(f));
  double Fold = 0.0;
  if (first) {
    S.F = f;
    S.nfev = 1;
    accepted = true;
  } else {
    const double F = S.F, Ft = f, gs = S.gs, snorm = S.snorm, prered = S.prered;
    double delta = S.delta;
    ++S.nfev;
    const double actred = F - Ft;
    if (!S.moved) delta = fmin(delta, snorm);
    const double curv = fma(inv_n, nf, -F) - gs;
    const double ah = curv <= 0.0 ? 4.0 : fmax(0.25, -0.5 * (gs / curv));
    if (!(actred >= 1.0e-4 * prered)) delta = fmin(fmax(ah, 0.25) * snorm, 0.5 * delta);
    else if (actred < 0.25 * prered) delta = fmax(0.25 * delta, fmin(ah * snorm, 0.5 * delta));
    else if (actred < 0.75 * prered) delta = fmax(0.25 * delta, fmin(ah * snorm, 4.0 * delta));
    else delta = fmax(delta, fmin(ah * snorm, 4.0 * delta));
    S.delta = delta;
    accepted = actred > 1.0e-4 * prered;
    if (accepted) {
      Fold = F;
      S.F = Ft;
      ++S.nit;
      S.moved = true;
      S.rejected = 0;
    } else {
      ++S.rejected;
      if (S.nfev > o.maxfun) S.status = 3;
      else if (S.rejected >= o.maxls) S.status = 4;
    }
  }
  if (accepted) {
    { double* t = W.x; W.x = W.xt; W.xt = t; t = W.g; W.g = W.gt; W.gt = t; t = W.dc; W.dc = W.dt; W.dt = t; }
    tron_rows_norms(V, rl, p_one, S.gmax, S.gg);
    if (first) {
      if (S.gmax <= o.pgtol) S.status = 0;
      S.delta = sqrt(S.gg);
    } else {
      const double F = S.F;
      if (S.gmax <= o.pgtol) S.status = 0;
      else if (Fold - F <= o.ftol * fmax(fabs(Fold), fmax(fabs(F), 1.0))) S.status = 1;
      else if (S.nit >= o.max_iter) S.status = 2;
      else if (S.nfev > o.maxfun) S.status = 3;
    }
  }
  if (S.status >= 0) {
    S.phase = TRON_ROW_DONE;
    return;
  }
  // Steihaug CG on the model at (x, g, D): s = 0, r = -g, d = r
  S.gnorm = sqrt(S.gg);
  for (int j = rl; j < p; j += ROW) {
    const double gj = W.g[j];
    W.s[j] = 0.0;
    W.r[j] = -gj;
    W.d[j] = -gj;
  }
  S.rr = S.gg;
  S.ncg = 1;
  S.phase = TRON_ROW_PRODUCT;
}

// SIMPLE variance at the returned theta: tron_variance_simple on a row
__device__ __forceinline__ void tron_rows_variance_simple(const TronRowView& V, const SolveParams& o, int rl, bool n_one, const double* D, double* var_out) {
  const EntityView& P = V.P;
  const int n = P.n, p = P.p, ic = P.ic;
  double q[1][TRON_ROWS] = {};
  rows_each(0, n, rl, [&](int i, int k) { q[0][k] += D[i]; });
  double dsum[1];
  rows_wave_sums(q, n_one, dsum);
  const int first_reg = (ic && !o.regularize_bias) ? 1 : 0;
  for (int j = rl; j < p; j += ROW) {
    double h;
    if (ic && j == 0) {
      h = dsum[0];
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
}

}  // namespace gdmix
