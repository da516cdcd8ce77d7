// re_owlqn.hpp — the per-entity elastic-net solve (OWL-QN, Andrew & Gao 2007), written once against the thread-group policy of
// re_solve_core.hpp (WaveGroup: one wavefront per entity, state in LDS; BlockGroup: one workgroup per entity, state in a global
// scratch slot). The statement it follows is include/gdmix_re.h, "elastic net" (the step of include/gdmix_fe.h, "(ABI 23)", applied
// to the per-entity objective: divided by n, intercept first); tests/re_l1_helpers.py restates it in numpy.
//
//   F(theta) = f(theta) + lam |theta_R|_1,   f = eval_fg<LOSS> (data term and l2 term, divided by n),   lam = l1 / n
//
// Synchronisation: element j of every p-vector is only ever touched by thread j mod NT, so the elementwise passes need no barrier
// between them; the trial point is synced before an evaluation gathers it across threads, and eval_fg ends on a sync.
#pragma once
#include "re_solve_core.hpp"

namespace gdmix {

// Working vectors of one OWL-QN solve: Work's, and one p-vector more — the pseudo-gradient of the accepted point lives through the
// whole line search (the Armijo term is pg'(x(t) - x)). The accepted pair (x, g) and the trial pair (xt, gt) change places on
// acceptance: no copy.
struct OwlWork {
  double* x;    // [p] accepted point (the result on exit)
  double* g;    // [p] smooth gradient at x
  double* pg;   // [p] pseudo-gradient at x
  double* d;    // [p] direction
  double* xt;   // [p] trial point (holds theta0 on entry)
  double* gt;   // [p] smooth gradient at xt
  double* ws;   // [m*p] s history, a slot-major ring
  double* wy;   // [m*p] y history
  double* rs;   // [n] per-sample residuals of the last evaluation
  double* alpha;  // [m] two-loop coefficients (uniform; every thread stores the same value)
  double* rho;    // [m] 1 / (s'y) per ring slot (uniform)
};
constexpr int OWL_P_VECTORS = 6;   // x g pg d xt gt; Work has five

constexpr double OWL_ARMIJO_C = 1.0e-4;
constexpr double OWL_PAIR_EPS = 2.2e-16;   // a pair is stored iff s'y > OWL_PAIR_EPS y'y

// pg of the accepted point from (x, g), with |pg|_inf and pg'pg: one pass, two reductions.
template <class G>
__device__ __forceinline__ void owlqn_pseudo_gradient(G& grp, int p, int first_reg, double lam, const OwlWork& W, double& pgmax, double& pgpg) {
  double mx = 0.0, sq = 0.0;
  for (int j = grp.tid; j < p; j += grp.NT) {
    const double xj = W.x[j], gj = W.g[j];
    double v = gj;
    if (j >= first_reg) {
      const double up = gj + lam, dn = gj - lam;
      v = xj > 0.0 ? up : (xj < 0.0 ? dn : (up < 0.0 ? up : (dn > 0.0 ? dn : 0.0)));
    }
    W.pg[j] = v;
    mx = fmax(mx, fabs(v));
    sq += v * v;
  }
  pgmax = grp.max_nonneg(mx);
  pgpg = grp.sum(sq);
}

// The whole solve of one entity. On entry W.xt holds the start point; on exit W.x is the last accepted point (never a rejected
// trial: coordinates the orthant projection set to zero are exactly 0.0) and W.rs is free. o.l2 is the l2 of the elastic net.
template <int LOSS = LOSS_LOGISTIC, class G>
__device__ void owlqn_solve(G& grp, const EntityView& P, const SolveParams& o, double l1, OwlWork& W, SolveStats& st) {
  const int p = P.p, m = o.m;
  const int first_reg = (P.ic && !o.regularize_bias) ? 1 : 0;
  const double lam = l1 / (double)P.n;
  Work E{};   // the evaluation's view: the trial pair
  E.rs = W.rs;

  // start point: evaluate, make it the accepted point
  double l1p = 0.0;
  for (int j = first_reg + grp.tid; j < p; j += grp.NT) l1p += fabs(W.xt[j]);
  E.x = W.xt; E.g = W.gt;
  double F = eval_fg<LOSS>(grp, P, o, E) + lam * grp.sum(l1p);
  { double* t = W.x; W.x = W.xt; W.xt = t; t = W.g; W.g = W.gt; W.gt = t; }
  int nfev = 1, nit = 0, col = 0, head = 0, status = -1;
  double h0 = 1.0, pgmax, pgpg;
  owlqn_pseudo_gradient(grp, p, first_reg, lam, W, pgmax, pgpg);
  if (pgmax <= o.pgtol) status = 0;

  while (status < 0) {
    // direction: two-loop recursion on pg over the ring (newest first, then oldest first), H0 from the newest pair, then the
    // components with d_j pg_j >= 0 are zeroed. No pair: d = -pg, first step 1 / |pg|_2.
    double t;
    if (col > 0) {
      for (int j = grp.tid; j < p; j += grp.NT) W.d[j] = W.pg[j];
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
        W.d[j] = (dj * W.pg[j] >= 0.0) ? 0.0 : dj;
      }
      t = 1.0;
    } else {
      for (int j = grp.tid; j < p; j += grp.NT) W.d[j] = -W.pg[j];
      t = 1.0 / sqrt(pgpg);
    }

    // backtracking along the projected path
    int rejected = 0;
    double Ft = F;
    bool accepted = false;
    while (!accepted) {
      // trial point, its projection on the orthant xi (sign(x_j), or sign(-pg_j) at x_j = 0), pg'(x(t) - x) and the L1 sum: one pass
      double pgd = 0.0, l1t = 0.0;
      for (int j = grp.tid; j < p; j += grp.NT) {
        const double xj = W.x[j], pgj = W.pg[j];
        const int xi = xj != 0.0 ? ((xj > 0.0) - (xj < 0.0)) : ((pgj < 0.0) - (pgj > 0.0));
        double v = xj + t * W.d[j];
        if (((v > 0.0) - (v < 0.0)) != xi) v = 0.0;
        W.xt[j] = v;
        pgd += pgj * (v - xj);
        l1t += (j >= first_reg) ? fabs(v) : 0.0;
      }
      const double pgdx = grp.sum(pgd);
      const double l1s = grp.sum(l1t);
      grp.sync();   // the evaluation gathers xt across threads
      E.x = W.xt; E.g = W.gt;
      Ft = eval_fg<LOSS>(grp, P, o, E) + lam * l1s;
      ++nfev;
      if (Ft <= F + OWL_ARMIJO_C * pgdx) { accepted = true; break; }
      ++rejected;
      if (rejected >= o.maxls) {
        if (col == 0) { status = 4; break; }
        // the memory is cleared and the search starts again along -pg
        col = 0; head = 0; rejected = 0;
        for (int j = grp.tid; j < p; j += grp.NT) W.d[j] = -W.pg[j];
        t = 1.0 / sqrt(pgpg);
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
    owlqn_pseudo_gradient(grp, p, first_reg, lam, W, pgmax, pgpg);
    if (pgmax <= o.pgtol) status = 0;
    else if (Fold - F <= o.ftol * fmax(fabs(Fold), fmax(fabs(F), 1.0))) status = 1;
    else if (nit >= o.max_iter) status = 2;
    else if (nfev > o.maxfun) status = 3;
  }
  grp.sync();
  st.f = F;
  st.gnorm = pgmax;
  st.nit = nit;
  st.nfev = nfev;
  st.status = status;
}

}  // namespace gdmix
