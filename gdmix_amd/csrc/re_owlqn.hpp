// re_owlqn.hpp — the per-entity projected quasi-Newton solve, one solve driven by a rule (as fe_qn.hip is one step driven by a rule):
//   ReOwlRule  OWL-QN (Andrew & Gao 2007) for the elastic net   (include/gdmix_re.h, "elastic net"),
//   ReBoxRule  projected L-BFGS inside a box lo <= theta <= hi  (include/gdmix_re.h, "box constraints").
// Written once against the thread-group policy of re_solve_core.hpp (WaveGroup: one wavefront per entity, state in LDS; BlockGroup: one
// workgroup per entity, state in a global scratch slot). The statements it follows are the steps of include/gdmix_fe.h, "(ABI 23)" and
// "(ABI 26)", applied to the per-entity objective: divided by n, intercept first; tests/re_l1_helpers.py and tests/re_box_helpers.py restate
// them in numpy.
//
//   elastic net   F(theta) = f(theta) + lam |theta_R|_1,   f = eval_fg<LOSS> (data term and l2 term, divided by n),   lam = l1 / n
//   box           F(theta) = f(theta)   on  lo <= theta <= hi
//
// A rule answers only what differs per coefficient: the reduced gradient q (the pseudo-gradient; g off the binding set), the vector of
// the Armijo term, the stopping measure, the steepest-descent entry, the direction fix-up, the trial point, and whether F has an L1 sum.
//
// Synchronisation: element j of every p-vector — the bounds included — is only ever touched by thread j mod NT, so the elementwise passes
// need no barrier between them; the trial point is synced before an evaluation gathers it across threads, and eval_fg ends on a sync.
#pragma once
#include "box_rule.hpp"
#include "re_solve_core.hpp"

namespace gdmix {

// Working vectors of one solve: Work's, and what the rule keeps per coefficient. OWL-QN keeps the pseudo-gradient of the accepted point
// (it lives through the whole line search: the Armijo term is pg'(x(t) - x)); the bounded step keeps the entity's bounds and derives q from
// (g, x, lo, hi) where it needs it. The accepted pair (x, g) and the trial pair (xt, gt) change places on acceptance: no copy.
struct QnWork {
  double* x;    // [p] accepted point (the result on exit)
  double* g;    // [p] smooth gradient at x
  double* pg;   // [p] pseudo-gradient at x                     (ReOwlRule only)
  double* d;    // [p] direction
  double* xt;   // [p] trial point (holds the start point on entry)
  double* gt;   // [p] smooth gradient at xt
  double* lo;   // [p] lower bounds, -inf at the intercept      (ReBoxRule only)
  double* hi;   // [p] upper bounds, +inf at the intercept      (ReBoxRule only)
  double* ws;   // [m*p] s history, a slot-major ring
  double* wy;   // [m*p] y history
  double* rs;   // [n] per-sample residuals of the last evaluation
  double* alpha;  // [m] two-loop coefficients (uniform; every thread stores the same value)
  double* rho;    // [m] 1 / (s'y) per ring slot (uniform)
};

constexpr double OWL_ARMIJO_C = 1.0e-4;
constexpr double OWL_PAIR_EPS = 2.2e-16;   // a pair is stored iff s'y > OWL_PAIR_EPS y'y

// ---- the rules -------------------------------------------------------------------------------------------------------------------------
// A rule travels by value as a kernel argument; Rule::Ent is what it becomes for one entity. Of a rule:
//   P_VECTORS                        coefficient vectors of its QnWork (Work has five)
//   L1_TERM                          whether F carries lam |theta_R|_1
//   carve(W, dp, stride)             its coefficient vectors out of dp, `stride` doubles each -> the first double behind them
//   stage(W, j, ic, f0, v)           called once per coefficient by thread j mod NT while the block is staged: what the rule keeps of
//                                    coefficient j, and the start value from the caller's v
//   entity(n, first_reg)             -> Ent
// Of an Ent, per coefficient j (xj, gj: the accepted point and its gradient):
//   reduced(W, j, xj, gj)            q_j at the accepted point (OWL-QN stores it)
//   measure(W, j, xj, gj, q)         the entry of the stopping measure, a maximum
//   q(W, j)                          q_j again, for the two-loop recursion
//   armijo(W, j)                     the entry of the Armijo term's vector
//   descent(W, j)                    the entry of the steepest-descent direction
//   direction(W, j, dj)              the two-loop direction's entry as it is used
//   trial(W, j, xj, aj, dj, t)       the entry of the trial point along d
//   keeps(W, j)                      theta_thr keeps the value whatever the threshold
struct ReOwlRule {
  double l1;
  static constexpr int P_VECTORS = 6;   // x g pg d xt gt
  static constexpr bool L1_TERM = true;
  __device__ __forceinline__ static double* carve(QnWork& W, double* dp, size_t stride) {
    W.x = dp; dp += stride;
    W.g = dp; dp += stride;
    W.pg = dp; dp += stride;
    W.d = dp; dp += stride;
    W.xt = dp; dp += stride;
    W.gt = dp; dp += stride;
    W.lo = nullptr; W.hi = nullptr;
    return dp;
  }
  __device__ __forceinline__ double stage(const QnWork&, int, int, int64_t, double v) const { return v; }
  struct Ent {
    double lam;
    int first_reg;
    __device__ __forceinline__ double reduced(const QnWork& W, int j, double xj, double gj) const {
      double v = gj;
      if (j >= first_reg) {
        const double up = gj + lam, dn = gj - lam;
        v = xj > 0.0 ? up : (xj < 0.0 ? dn : (up < 0.0 ? up : (dn > 0.0 ? dn : 0.0)));
      }
      W.pg[j] = v;
      return v;
    }
    __device__ __forceinline__ double measure(const QnWork&, int, double, double, double q) const { return fabs(q); }
    __device__ __forceinline__ double q(const QnWork& W, int j) const { return W.pg[j]; }
    __device__ __forceinline__ double armijo(const QnWork& W, int j) const { return W.pg[j]; }
    __device__ __forceinline__ double descent(const QnWork& W, int j) const { return -W.pg[j]; }
    // the direction stays in the orthant the pseudo-gradient points into
    __device__ __forceinline__ double direction(const QnWork& W, int j, double dj) const { return (dj * W.pg[j] >= 0.0) ? 0.0 : dj; }
    // the projection on the orthant xi (sign(x_j), or sign(-pg_j) at x_j = 0): a coordinate that leaves it is exactly 0
    __device__ __forceinline__ double trial(const QnWork&, int, double xj, double pgj, double dj, double t) const {
      const int xi = xj != 0.0 ? ((xj > 0.0) - (xj < 0.0)) : ((pgj < 0.0) - (pgj > 0.0));
      double v = xj + t * dj;
      if (((v > 0.0) - (v < 0.0)) != xi) v = 0.0;
      return v;
    }
    __device__ __forceinline__ bool keeps(const QnWork&, int) const { return false; }
  };
  __device__ __forceinline__ Ent entity(int n, int first_reg) const { return Ent{l1 / (double)n, first_reg}; }
};

struct ReBoxRule {
  const double* lower;             // [num_features] by global feature id, or NULL: no lower bound
  const double* upper;             // [num_features], or NULL: no upper bound
  const int32_t* unique_global;    // the batch's local -> global feature index
  static constexpr int P_VECTORS = 7;   // x g d xt gt lo hi
  static constexpr bool L1_TERM = false;
  __device__ __forceinline__ static double* carve(QnWork& W, double* dp, size_t stride) {
    W.x = dp; dp += stride;
    W.g = dp; dp += stride;
    W.d = dp; dp += stride;
    W.xt = dp; dp += stride;
    W.gt = dp; dp += stride;
    W.lo = dp; dp += stride;
    W.hi = dp; dp += stride;
    W.pg = nullptr;
    return dp;
  }
  // the entity's bounds, gathered once: the intercept (coefficient 0 when ic) is free; the start point is clamped into the box
  __device__ __forceinline__ double stage(const QnWork& W, int j, int ic, int64_t f0, double v) const {
    double lo = -__builtin_inf(), hi = __builtin_inf();
    if (j >= ic) {
      const int32_t gid = unique_global[f0 + (j - ic)];
      if (lower) lo = lower[gid];
      if (upper) hi = upper[gid];
    }
    W.lo[j] = lo;
    W.hi[j] = hi;
    return box_clamp(v, lo, hi);
  }
  struct Ent {
    __device__ __forceinline__ double reduced(const QnWork& W, int j, double xj, double gj) const {
      return box_binding(gj, xj, W.lo[j], W.hi[j]) ? 0.0 : gj;
    }
    // the projected gradient
    __device__ __forceinline__ double measure(const QnWork& W, int j, double xj, double gj, double) const {
      return fabs(xj - box_clamp(xj - gj, W.lo[j], W.hi[j]));
    }
    __device__ __forceinline__ double q(const QnWork& W, int j) const { return reduced(W, j, W.x[j], W.g[j]); }
    __device__ __forceinline__ double armijo(const QnWork& W, int j) const { return W.g[j]; }      // the plain gradient at x
    __device__ __forceinline__ double descent(const QnWork& W, int j) const { return direction(W, j, -W.g[j]); }
    __device__ __forceinline__ double direction(const QnWork& W, int j, double dj) const {
      const double xj = W.x[j], lo = W.lo[j], hi = W.hi[j];
      return box_direction(dj, box_binding(W.g[j], xj, lo, hi), xj, lo, hi);
    }
    __device__ __forceinline__ double trial(const QnWork& W, int j, double xj, double, double dj, double t) const {
      return box_clamp(xj + t * dj, W.lo[j], W.hi[j]);
    }
    // a box that does not contain 0: the thresholded model stays inside it
    __device__ __forceinline__ bool keeps(const QnWork& W, int j) const { return W.lo[j] > 0.0 || W.hi[j] < 0.0; }
  };
  __device__ __forceinline__ Ent entity(int, int) const { return Ent{}; }
};

// q of the accepted point from (x, g), with the stopping measure and q'q: one pass, two reductions.
template <class G, class Ent>
__device__ __forceinline__ void qn_reduced_gradient(G& grp, int p, const Ent& r, const QnWork& W, double& qmax, double& qq) {
  double mx = 0.0, sq = 0.0;
  for (int j = grp.tid; j < p; j += grp.NT) {
    const double xj = W.x[j], gj = W.g[j];
    const double v = r.reduced(W, j, xj, gj);
    mx = fmax(mx, r.measure(W, j, xj, gj, v));
    sq += v * v;
  }
  qmax = grp.max_nonneg(mx);
  qq = grp.sum(sq);
}

// The whole solve of one entity. On entry W.xt holds the start point (staged by the rule: inside the box under ReBoxRule); on exit W.x is
// the last accepted point (never a rejected trial: coordinates the orthant projection set to zero are exactly 0.0, a clamped coordinate
// is the bound's double) and W.rs is free. o.l2 is the l2 of the objective.
template <int LOSS = LOSS_LOGISTIC, class Rule, class G>
__device__ void owlqn_solve(G& grp, const EntityView& P, const SolveParams& o, const Rule& R, QnWork& W, SolveStats& st) {
  const int p = P.p, m = o.m;
  const int first_reg = (P.ic && !o.regularize_bias) ? 1 : 0;
  const typename Rule::Ent r = R.entity(P.n, first_reg);
  Work E{};   // the evaluation's view: the trial pair
  E.rs = W.rs;

  // start point: evaluate, make it the accepted point
  double F;
  if constexpr (Rule::L1_TERM) {
    double l1p = 0.0;
    for (int j = first_reg + grp.tid; j < p; j += grp.NT) l1p += fabs(W.xt[j]);
    E.x = W.xt; E.g = W.gt;
    F = eval_fg<LOSS>(grp, P, o, E) + r.lam * grp.sum(l1p);
  } else {
    E.x = W.xt; E.g = W.gt;
    F = eval_fg<LOSS>(grp, P, o, E);
  }
  { double* t = W.x; W.x = W.xt; W.xt = t; t = W.g; W.g = W.gt; W.gt = t; }
  int nfev = 1, nit = 0, col = 0, head = 0, status = -1;
  double h0 = 1.0, qmax, qq;
  qn_reduced_gradient(grp, p, r, W, qmax, qq);
  if (qmax <= o.pgtol) status = 0;

  while (status < 0) {
    // direction: two-loop recursion on q over the ring (newest first, then oldest first), H0 from the newest pair, then the rule's
    // fix-up (OWL-QN: d_j pg_j >= 0 zeroed; box: the binding set, and where d points out of the box). No pair: the rule's steepest
    // descent, first step 1 / |q|_2.
    double t;
    if (col > 0) {
      for (int j = grp.tid; j < p; j += grp.NT) W.d[j] = r.q(W, j);
      for (int a = col - 1; a >= 0; --a) {
        int sl = head + a; if (sl >= m) sl -= m;
        const double* s = W.ws + (size_t)sl * p;
        const double* yv = W.wy + (size_t)sl * p;
        const double al = W.rho[sl] * dot(grp, s, W.d, p);
        W.alpha[a] = al;
        for (int j = grp.tid; j < p; j += grp.NT) W.d[j] -= al * yv[j];
      }
      for (int j = grp.tid; j < p; j += grp.NT) W.d[j] *= h0;
      for (int a = 0; a < col; ++a) {
        int sl = head + a; if (sl >= m) sl -= m;
        const double* s = W.ws + (size_t)sl * p;
        const double* yv = W.wy + (size_t)sl * p;
        const double beta = W.rho[sl] * dot(grp, yv, W.d, p);
        const double c = W.alpha[a] - beta;
        for (int j = grp.tid; j < p; j += grp.NT) W.d[j] += c * s[j];
      }
      for (int j = grp.tid; j < p; j += grp.NT) {
        const double dj = -W.d[j];
        W.d[j] = r.direction(W, j, dj);
      }
      t = 1.0;
    } else {
      for (int j = grp.tid; j < p; j += grp.NT) W.d[j] = r.descent(W, j);
      t = 1.0 / sqrt(qq);
    }

    // backtracking along the projected path
    int rejected = 0;
    double Ft = F;
    bool accepted = false;
    while (!accepted) {
      // trial point (projected on the orthant, or clamped into the box), a'(x(t) - x) and the L1 sum: one pass
      double pgd = 0.0, l1t = 0.0;
      for (int j = grp.tid; j < p; j += grp.NT) {
        const double xj = W.x[j], pgj = r.armijo(W, j);
        const double v = r.trial(W, j, xj, pgj, W.d[j], t);
        W.xt[j] = v;
        pgd += pgj * (v - xj);
        if constexpr (Rule::L1_TERM) l1t += (j >= first_reg) ? fabs(v) : 0.0;
      }
      const double pgdx = grp.sum(pgd);
      double l1s = 0.0;
      if constexpr (Rule::L1_TERM) l1s = grp.sum(l1t);
      grp.sync();   // the evaluation gathers xt across threads
      E.x = W.xt; E.g = W.gt;
      if constexpr (Rule::L1_TERM) Ft = eval_fg<LOSS>(grp, P, o, E) + r.lam * l1s;
      else Ft = eval_fg<LOSS>(grp, P, o, E);
      ++nfev;
      if (Ft <= F + OWL_ARMIJO_C * pgdx) { accepted = true; break; }
      ++rejected;
      if (rejected >= o.maxls) {
        if (col == 0) { status = 4; break; }
        // the memory is cleared and the search starts again along the steepest descent
        col = 0; head = 0; rejected = 0;
        for (int j = grp.tid; j < p; j += grp.NT) W.d[j] = r.descent(W, j);
        t = 1.0 / sqrt(qq);
      } else {
        t *= 0.5;
      }
    }
    if (!accepted) break;   // status 4 at x

    // s = xt - x, y = gt - g into the accepted pair's own vectors (they are the next trial pair), with s'y and y'y
    double syp = 0.0, yyp = 0.0;
    for (int j = grp.tid; j < p; j += grp.NT) {
      const double sj = W.xt[j] - W.x[j], yj = W.gt[j] - W.g[j];
      W.x[j] = sj;
      W.g[j] = yj;
      syp += sj * yj;
      yyp += yj * yj;
    }
    const double sy = grp.sum(syp);
    const double yy = grp.sum(yyp);
    if (sy > OWL_PAIR_EPS * yy) {
      int sl;
      if (col < m) { sl = head + col; if (sl >= m) sl -= m; ++col; }
      else { sl = head; ++head; if (head >= m) head = 0; }
      double* s = W.ws + (size_t)sl * p;
      double* yv = W.wy + (size_t)sl * p;
      for (int j = grp.tid; j < p; j += grp.NT) { s[j] = W.x[j]; yv[j] = W.g[j]; }
      W.rho[sl] = 1.0 / sy;
      h0 = sy / yy;
    }
    { double* q = W.x; W.x = W.xt; W.xt = q; q = W.g; W.g = W.gt; W.gt = q; }
    const double Fold = F;
    F = Ft;
    ++nit;
    qn_reduced_gradient(grp, p, r, W, qmax, qq);
    if (qmax <= o.pgtol) status = 0;
    else if (Fold - F <= o.ftol * fmax(fabs(Fold), fmax(fabs(F), 1.0))) status = 1;
    else if (nit >= o.max_iter) status = 2;
    else if (nfev > o.maxfun) status = 3;
  }
  grp.sync();
  st.f = F;
  st.gnorm = qmax;
  st.nit = nit;
  st.nfev = nfev;
  st.status = status;
}

}  // namespace gdmix
