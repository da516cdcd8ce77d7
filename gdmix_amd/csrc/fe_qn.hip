// fe_qn.hip — the fixed effect's two projected quasi-Newton steps, one step driven by a rule:
//   OwlRule  OWL-QN (Andrew & Gao 2007) for  F = smooth + l1 |theta_R|_1  (include/gdmix_fe.h, "(ABI 23) L1 / elastic net"; gdmix_fe_set_l1),
//   BoxRule  projected L-BFGS for the smooth objective inside a box  lo <= theta <= hi  ("(ABI 26) box constraints"; gdmix_fe_set_bounds).
// Either consumes the same all-reduced [gradient, value] buffer as the L-BFGS-B step of fe_solve.hip and lives in the same pool, state
// record, plan and m x m matrices. Three ordinary launches per evaluation — products, decision, update — and no kernel of this unit waits
// on another workgroup: a launch boundary is the only synchronisation. A rule travels by value as a kernel argument; the bounds are two
// vectors of the problem's own (fe_solve.hip: box_mem), so FeDev keeps its layout.
//
// The pool's vectors under these steps (Work of re_solve_core.hpp):
//     W.x  the TRIAL point, the one the passes evaluate (the row pass reads the intercept from W.x[D], the features from F.xl)
//     W.t  the last ACCEPTED point x (what gdmix_fe_result returns)
//     W.g  the smooth gradient at x            W.r  the smooth gradient at the trial (the products pass leaves it for the update)
//     W.d  the search direction as it is used  W.ws the (s, y) pairs, in re_lbfgs_compact.hpp's tile layout (compact_hist)
// What a rule derives — the pseudo-gradient and the orthant, or the binding set, the reduced and the projected gradient — is a function of
// (g_j, x_j) and the rule's own data alone and is formed where it is needed, never stored. The intercept's bounds are -inf / +inf
// (gdmix_fe_set_bounds checks it), so the bounded step does not treat it apart.
#include "box_rule.hpp"
#include "fe_step_shares.hpp"
#include "re_lbfgs_compact.hpp"
#include "../../include/gdmix_fe.h"

namespace gdmix {

// the products of one evaluation, per virtual block in F.acc_part and in total in the decision's LDS (fe_step_shares.hpp). q is the
// rule's reduced gradient (the pseudo-gradient; g off the binding set), q+ the one at the trial.
enum {
  QN_X2 = 0,      // sum over R of trial_j^2
  QN_ARM,         // a'(trial - x): the Armijo term, a the rule's vector at x
  QN_SY,          // s'y,  s = trial - x,  y = g(trial) - g(x)
  QN_YY,          // y'y
  QN_MAX,         // the stopping measure at the trial, a maximum
  QN_Q2,          // q+'q+
  QN_SQ,          // s'q+
  QN_YQ,          // y'q+
  QN_HSY,                            // S_i'y   (chronological i < col)
  QN_HYY = QN_HSY + TEAM_MCAP,       // Y_i'y
  QN_HSQ = QN_HYY + TEAM_MCAP,       // S_i'q+
  QN_HYQ = QN_HSQ + TEAM_MCAP,       // Y_i'q+
  QN_X1 = QN_HYQ + TEAM_MCAP         // sum over R of |trial_j|: last, and only under a rule with an L1 term
};
template <class Rule> constexpr int QN_K = QN_X1 + (Rule::L1_TERM ? 1 : 0);
constexpr int QN_BLOCKS = 480;      // virtual blocks at most: their shares fit the L-BFGS-B step's acc_part
static_assert(QN_BLOCKS * (QN_X1 + 1) <= FE_DOT_BLOCKS * COMPACT_KD, "the shares live in F.acc_part");

// CompactPlan.action under these steps. Both stops are idempotent: a step enqueued behind the stop repeats the plan.
enum {
  QA_STOP_ACCEPT = 0,   // the trial is the result: t := x
  QA_STOP_RESTORE,      // the last accepted point is the result: x := t
  QA_RETRY,             // backtrack: x := trial(t + stp d)
  QA_STEEPEST,          // the search failed with pairs stored: memory cleared, d := the rule's descent entry at t, x := trial(t + stp d)
  QA_ACCEPT             // the trial becomes x: pair (plan.store_pair), new direction, first trial along it; plan.restore: the start point (no pair to form)
};
constexpr double QN_ARMIJO = 1e-4;

// ---- the rules: what differs per coefficient ---------------------------------------------------------------------------------------------
// at(j, reg)               what the coefficient loads next to x and g
// reduced(g, x, a)         the reduced gradient q at a point
// armijo(g, x, a)          the entry of the Armijo term's vector at x
// measure(g, x, q, a)      the entry of the stopping measure
// descent(g, q, x, a)      the entry of the steepest-descent direction
// direction(d, g, q, x, a) the direction entry as it is used
// trial(x, d, q, stp, a)   the entry of the trial point along d
// retry(W, j, reg, stp)    the trial of a backtracking update, which never reads the stored pairs
__device__ __forceinline__ double owl_pseudo(double g, double x, double l1, bool reg) {
  if (!reg) return g;
  if (x > 0.0) return g + l1;
  if (x < 0.0) return g - l1;
  const double up = g + l1, dn = g - l1;
  return up < 0.0 ? up : (dn > 0.0 ? dn : 0.0);
}

// x + stp d kept inside the orthant xi = sign(x), or sign(-pg) where x is 0; a coordinate that leaves it is exactly 0
__device__ __forceinline__ double owl_trial(double x, double d, double pg, double stp) {
  const bool pos = x > 0.0 || (x == 0.0 && pg < 0.0), neg = x < 0.0 || (x == 0.0 && pg > 0.0);
  const double xn = x + stp * d;
  return ((pos && xn > 0.0) || (neg && xn < 0.0)) ? xn : 0.0;
}

struct OwlRule {
  double l1;
  static constexpr bool L1_TERM = true;
  using At = bool;      // whether the coefficient is regularised
  __device__ At at(int, bool reg) const { return reg; }
  __device__ double reduced(double g, double x, At reg) const { return owl_pseudo(g, x, l1, reg); }
  __device__ double armijo(double g, double x, At a) const { return reduced(g, x, a); }      // the pseudo-gradient at x
  __device__ double measure(double, double, double q, At) const { return fabs(q); }
  __device__ double descent(double, double q, double, At) const { return -q; }      // (already in the orthant it points into)
  // the direction stays in the orthant the pseudo-gradient points into
  __device__ double direction(double d, double, double q, double, At) const { return d * q >= 0.0 ? 0.0 : d; }
  __device__ double trial(double x, double d, double q, double stp, At) const { return owl_trial(x, d, q, stp); }
  __device__ double retry(const Work& W, int j, bool reg, double stp) const {      // reads x, g, d
    const double xa = W.t[j];
    return owl_trial(xa, W.d[j], owl_pseudo(W.g[j], xa, l1, reg), stp);
  }
};

// box_clamp, box_binding, box_direction: box_rule.hpp (shared with the random effect's bounded solve)
struct BoxRule {
  const double *lower, *upper;      // [P] device doubles
  static constexpr bool L1_TERM = false;
  struct At { double lo, hi; };
  __device__ At at(int j, bool) const { return {lower[j], upper[j]}; }
  __device__ double reduced(double g, double x, At a) const { return box_binding(g, x, a.lo, a.hi) ? 0.0 : g; }
  __device__ double armijo(double g, double, At) const { return g; }      // the plain gradient at x
  __device__ double measure(double g, double x, double, At a) const { return fabs(x - box_clamp(x - g, a.lo, a.hi)); }      // the projected gradient
  __device__ double descent(double g, double q, double x, At a) const { return direction(-g, g, q, x, a); }
  __device__ double direction(double d, double g, double, double x, At a) const { return box_direction(d, box_binding(g, x, a.lo, a.hi), x, a.lo, a.hi); }
  __device__ double trial(double x, double d, double, double stp, At a) const { return box_clamp(x + stp * d, a.lo, a.hi); }
  __device__ double retry(const Work& W, int j, bool, double stp) const {      // reads x, d and the bounds: never g
    return box_clamp(W.t[j] + stp * W.d[j], lower[j], upper[j]);
  }
};

// the ring's pairs of coefficient j in chronological order; all are requested before the first is used
__device__ __forceinline__ void qn_history(const Work& W, int m, int head, int j, double2 (&h)[TEAM_MCAP]) {
#pragma unroll
  for (int i = 0; i < TEAM_MCAP; ++i) {
    int sl = head + i;
    if (sl >= m) sl -= m;
    if (i >= m) sl = 0;
    h[i] = compact_hist(W, m, j)[sl * COMPACT_HIST_STRIDE];
  }
}

// ---- 1. products: one pass over the coefficients, one read of the history ------------------------------------------------------------
// The share of virtual block vb of nvb — coefficients (vb * 256 + tid) + k * nvb * 256 — into acc_part[vb]; nvb is a function of P alone.
template <class Rule>
__global__ __launch_bounds__(FE_THREADS) void fe_qn_products_kernel(FeDev F, SolveParams o, Rule R) {
  if (F.state->status >= 0) return;     // a step enqueued behind the stop is a no-op
  const int tid = threadIdx.x, vb = blockIdx.x, nvb = gridDim.x;
  const int col = F.state->col, head = F.state->head, m = o.m, P = F.P;
  double acc[QN_K<Rule>];
#pragma unroll
  for (int k = 0; k < QN_K<Rule>; ++k) acc[k] = 0.0;
  for (int j = vb * FE_THREADS + tid; j < P; j += nvb * FE_THREADS) {
    const bool reg = (j < F.D) || o.regularize_bias;   // the intercept is coefficient D
    const double xt = F.W.x[j], xa = F.W.t[j], go = F.W.g[j];
    const typename Rule::At a = R.at(j, reg);
    const double gn = F.fg[j] + (reg ? o.l2 * xt : 0.0);
    F.fg[j] = 0.0;   // consumed: the next evaluation starts from a clear buffer (gdmix_fe_eval)
    F.W.r[j] = gn;
    double2 h[TEAM_MCAP];
    qn_history(F.W, m, head, j, h);
    const double qn = R.reduced(gn, xt, a), ao = R.armijo(go, xa, a);
    const double sj = xt - xa, yj = gn - go;
    if (reg) {
      acc[QN_X2] += xt * xt;
      if constexpr (Rule::L1_TERM) acc[QN_X1] += fabs(xt);
    }
    acc[QN_ARM] += ao * sj;
    acc[QN_SY] += sj * yj;
    acc[QN_YY] += yj * yj;
    acc[QN_MAX] = fmax(acc[QN_MAX], R.measure(gn, xt, qn, a));
    acc[QN_Q2] += qn * qn;
    acc[QN_SQ] += sj * qn;
    acc[QN_YQ] += yj * qn;
#pragma unroll
    for (int i = 0; i < TEAM_MCAP; ++i) {
      const double hx = i < col ? h[i].x : 0.0, hy = i < col ? h[i].y : 0.0;
      acc[QN_HSY + i] += hx * yj;
      acc[QN_HYY + i] += hy * yj;
      acc[QN_HSQ + i] += hx * qn;
      acc[QN_HYQ + i] += hy * qn;
    }
  }
  fe_shares_store<QN_K<Rule>, QN_MAX>(acc, F.acc_part, vb);
}

// ---- 2. decision: one workgroup ----------------------------------------------------------------------------------------------------
// The m x m part by thread 0 on the replica in LDS: with R = triu(S'Y), D = diag(S'Y), gamma = s'y / y'y of the newest pair,
//     c = R^-1 S'q,   u = R^-T ((D + gamma Y'Y) c - gamma Y'q),   d = -H q = gamma (Y c - q) - S u      (Byrd, Nocedal & Schnabel)
__device__ __forceinline__ void qn_direction_coefficients(CompactMats& L, int col, double gamma, const double* a, const double* b) {
  constexpr int LD = TEAM_MCAP;
  double c[TEAM_MCAP], w[TEAM_MCAP];
  for (int k = col - 1; k >= 0; --k) {
    double s = a[k];
    for (int e = k + 1; e < col; ++e) s -= L.SY[k * LD + e] * c[e];
    c[k] = s / L.SY[k * LD + k];
  }
  for (int i = 0; i < col; ++i) {
    double s = L.SY[i * LD + i] * c[i] - gamma * b[i];
    for (int k = 0; k < col; ++k) s += gamma * L.YY[i * LD + k] * c[k];
    w[i] = s;
  }
  for (int k = 0; k < col; ++k) {
    double s = w[k];
    for (int r = 0; r < k; ++r) s -= L.SY[r * LD + k] * L.u[r];
    L.u[k] = s / L.SY[k * LD + k];
    L.q[k] = c[k];
  }
}

template <class Rule>
__global__ __launch_bounds__(FE_THREADS) void fe_qn_decide_kernel(FeDev F, SolveParams o, Rule R, int nvb, int32_t* status_out) {
  __shared__ double tot[QN_K<Rule>];
  __shared__ CompactMats mats;
  if (F.state->status >= 0) return;     // (status_out keeps the status of the stop; the update repeats the stop's plan: idempotent)
  const int tid = threadIdx.x;
  fe_shares_total<QN_K<Rule>, QN_MAX>(F.acc_part, nvb, tot);
  {
    const double* src = reinterpret_cast<const double*>(F.mats);
    double* dst = reinterpret_cast<double*>(&mats);
    for (int k = tid; k < (int)(sizeof(CompactMats) / sizeof(double)); k += FE_THREADS) dst[k] = src[k];
  }
  __syncthreads();
  if (tid == 0) {
    constexpr int LD = TEAM_MCAP;
    const int m = o.m;
    CompactState S = *F.state;
    CompactPlan plan;
    plan.action = QA_STOP_ACCEPT; plan.store_pair = 0; plan.restore = 0; plan.slot = 0; plan.cnew = 0; plan.col = S.col; plan.head = S.head;
    plan.shift = 0; plan.phantom = 0; plan.stp = S.stp; plan.stp_prev = S.stp; plan.gamma = S.theta;
    const double fdata = F.fg[F.P];
    double f_new;
    if constexpr (Rule::L1_TERM) f_new = fdata + 0.5 * o.l2 * tot[QN_X2] + R.l1 * tot[QN_X1];
    else f_new = fdata + 0.5 * o.l2 * tot[QN_X2];
    if (fdata == -__builtin_inf()) {
      // the mark of a worker whose step was aborted, carried here by the all-reduce (fe_step_body): every worker stops in this evaluation
      S.status = GDMIX_RE_ST_ABORTED_PEER;
      plan.action = S.first ? QA_STOP_ACCEPT : QA_STOP_RESTORE;
    } else if (S.first) {
      S.first = 0;
      ++S.nfev;
      S.f = f_new; S.fold = f_new;
      S.sbgnrm = tot[QN_MAX];
      S.gg_k = tot[QN_Q2];
      if (S.sbgnrm <= o.pgtol) {
        S.status = 0;
      } else {
        S.stp = 1.0 / sqrt(S.gg_k);
        S.ifun = 0;
        plan.action = QA_ACCEPT; plan.restore = 1; plan.col = 0; plan.head = 0; plan.stp = S.stp;
      }
    } else if (f_new <= S.f + QN_ARMIJO * tot[QN_ARM]) {
      ++S.nfev;
      ++S.nit;
      S.iter0 = 0;
      S.fold = S.f;
      S.f = f_new;
      S.ifun = 0;
      S.sbgnrm = tot[QN_MAX];
      S.gg_k = tot[QN_Q2];
      const double ddum = fmax(fabs(S.fold), fmax(fabs(S.f), 1.0));
      if (S.sbgnrm <= o.pgtol) S.status = 0;
      else if (S.fold - S.f <= o.ftol * ddum) S.status = 1;
      else if (S.nit >= o.max_iter) S.status = 2;
      else if (S.nfev > o.maxfun) S.status = 3;
      else {
        const double sy = tot[QN_SY], yy = tot[QN_YY];
        const bool store = sy > EPSMCH * yy;
        int col = S.col, head = S.head, off = 0, slot = 0;
        double a[TEAM_MCAP], b[TEAM_MCAP];
        if (store) {
          if (col < m) {
            slot = head + col;
            if (slot >= m) slot -= m;
            ++col;
          } else {      // drop the oldest pair: (r, c) <- (r + 1, c + 1), the ring's head moves on
            slot = head;
            head = head + 1 < m ? head + 1 : 0;
            off = 1;
            for (int r = 0; r + 1 < m; ++r)
              for (int c = 0; c + 1 < m; ++c) {
                mats.SY[r * LD + c] = mats.SY[(r + 1) * LD + c + 1];
                mats.YY[r * LD + c] = mats.YY[(r + 1) * LD + c + 1];
              }
          }
          const int cnew = col - 1;
          for (int i = 0; i < cnew; ++i) {
            mats.SY[i * LD + cnew] = tot[QN_HSY + i + off];
            mats.YY[i * LD + cnew] = tot[QN_HYY + i + off];
            mats.YY[cnew * LD + i] = tot[QN_HYY + i + off];
            a[i] = tot[QN_HSQ + i + off];
            b[i] = tot[QN_HYQ + i + off];
          }
          mats.SY[cnew * LD + cnew] = sy;
          mats.YY[cnew * LD + cnew] = yy;
          a[cnew] = tot[QN_SQ];
          b[cnew] = tot[QN_YQ];
          S.theta = sy / yy;      // gamma of H0, from the newest pair
          plan.store_pair = 1; plan.slot = slot; plan.cnew = cnew; plan.shift = off;
        } else {
          for (int i = 0; i < col; ++i) { a[i] = tot[QN_HSQ + i]; b[i] = tot[QN_HYQ + i]; }
        }
        if (col > 0) qn_direction_coefficients(mats, col, S.theta, a, b);
        S.col = col; S.head = head;
        S.stp = col > 0 ? 1.0 : 1.0 / sqrt(S.gg_k);
        plan.action = QA_ACCEPT; plan.col = col; plan.head = head; plan.stp = S.stp; plan.gamma = S.theta;
      }
    } else {
      ++S.nfev;
      ++S.ifun;      // rejected trials of this iteration
      if (S.ifun < o.maxls) {
        S.stp *= 0.5;
        plan.action = QA_RETRY; plan.stp = S.stp;
      } else if (S.col > 0) {
        S.col = 0; S.head = 0; S.ifun = 0;
        S.stp = 1.0 / sqrt(S.gg_k);
        plan.action = QA_STEEPEST; plan.col = 0; plan.head = 0; plan.stp = S.stp;
      } else {
        S.status = 4;
        plan.action = QA_STOP_RESTORE;
      }
    }
    *F.state = S;        // (read by later launches only)
    *F.plan = plan;
    *status_out = S.status;
  }
  __syncthreads();
  {
    double* dst = reinterpret_cast<double*>(F.mats);
    const double* src = reinterpret_cast<const double*>(&mats);
    for (int k = tid; k < (int)(sizeof(CompactMats) / sizeof(double)); k += FE_THREADS) dst[k] = src[k];
  }
}

// ---- 3. update: elementwise ----------------------------------------------------------------------------------------------------------
template <class Rule>
__global__ __launch_bounds__(256) void fe_qn_update_kernel(FeDev F, SolveParams o, Rule R) {
  const CompactPlan plan = *F.plan;
  const CompactMats& L = *F.mats;
  const int m = o.m;
  for (int j = blockIdx.x * blockDim.x + threadIdx.x; j < F.P; j += gridDim.x * blockDim.x) {
    const bool reg = (j < F.D) || o.regularize_bias;
    double xn;
    if (plan.action == QA_STOP_ACCEPT) {
      F.W.t[j] = F.W.x[j];
      continue;      // (the trial is already what the passes read)
    } else if (plan.action == QA_STOP_RESTORE) {
      xn = F.W.t[j];
    } else if (plan.action == QA_RETRY) {
      xn = R.retry(F.W, j, reg, plan.stp);
    } else if (plan.action == QA_STEEPEST) {
      const double xa = F.W.t[j], ga = F.W.g[j];
      const typename Rule::At a = R.at(j, reg);
      const double q = R.reduced(ga, xa, a);
      const double dj = R.descent(ga, q, xa, a);
      F.W.d[j] = dj;
      xn = R.trial(xa, dj, q, plan.stp, a);
    } else {
      const double xt = F.W.x[j], gn = F.W.r[j];
      const typename Rule::At a = R.at(j, reg);
      const double sn = xt - F.W.t[j], yn = gn - F.W.g[j];
      if (plan.store_pair) compact_hist(F.W, m, j)[plan.slot * COMPACT_HIST_STRIDE] = make_double2(sn, yn);
      F.W.t[j] = xt;
      F.W.g[j] = gn;
      const double q = R.reduced(gn, xt, a);
      double dj = -q;
      if (plan.col > 0) {
        double2 h[TEAM_MCAP];
        qn_history(F.W, m, plan.head, j, h);
        double su = 0.0, yc = 0.0;
#pragma unroll
        for (int i = 0; i < TEAM_MCAP; ++i) {
          if (i < plan.col) {
            const bool fresh = plan.store_pair && i == plan.cnew;
            su += L.u[i] * (fresh ? sn : h[i].x);
            yc += L.q[i] * (fresh ? yn : h[i].y);
          }
        }
        dj = plan.gamma * (yc - q) - su;
      }
      dj = R.direction(dj, gn, q, xt, a);
      F.W.d[j] = dj;
      xn = R.trial(xt, dj, q, plan.stp, a);
    }
    F.W.x[j] = xn;
    const int jl = F.inv[j];
    if (jl >= 0) F.xl[jl] = xn;
  }
}

template <class Rule>
static void qn_enqueue_step(const FeDev& F, const SolveParams& o, const Rule& R, int32_t* status_dev, hipStream_t s) {
  const int nvb = grid_for(F.P, FE_THREADS, QN_BLOCKS);
  hipLaunchKernelGGL(fe_qn_products_kernel<Rule>, dim3(nvb), dim3(FE_THREADS), 0, s, F, o, R);
  hipLaunchKernelGGL(fe_qn_decide_kernel<Rule>, dim3(1), dim3(FE_THREADS), 0, s, F, o, R, nvb, status_dev);
  hipLaunchKernelGGL(fe_qn_update_kernel<Rule>, dim3(grid_for(F.P, 256, 1024)), dim3(256), 0, s, F, o, R);
}

void fe_owlqn_enqueue_step(const FeDev& F, const SolveParams& o, double l1, int32_t* status_dev, hipStream_t s) {
  qn_enqueue_step(F, o, OwlRule{l1}, status_dev, s);
}

void fe_box_enqueue_step(const FeDev& F, const SolveParams& o, const double* lower, const double* upper, int32_t* status_dev, hipStream_t s) {
  qn_enqueue_step(F, o, BoxRule{lower, upper}, status_dev, s);
}

// ---- gdmix_fe_set_bounds' check and the start point ------------------------------------------------------------------------------------
// bad[0]: a NaN bound; bad[1]: lo_j > hi_j; bad[2]: a finite bound on the intercept (coefficient P - 1 when ic). Every writer stores 1.
__global__ void fe_box_check_kernel(const double* __restrict__ lower, const double* __restrict__ upper, int P, int ic, int32_t* __restrict__ bad) {
  for (int j = blockIdx.x * blockDim.x + threadIdx.x; j < P; j += gridDim.x * blockDim.x) {
    const double lo = lower[j], hi = upper[j];
    if (lo != lo || hi != hi) bad[0] = 1;
    else if (lo > hi) bad[1] = 1;
    else if (ic && j == P - 1 && (lo != -__builtin_inf() || hi != __builtin_inf())) bad[2] = 1;
  }
}

// behind fe_init_kernel: the start point clamped into the box, in W.x (what the passes evaluate), W.t (what gdmix_fe_result returns) and xl
__global__ void fe_box_start_kernel(FeDev F, const double* __restrict__ lower, const double* __restrict__ upper) {
  for (int j = blockIdx.x * blockDim.x + threadIdx.x; j < F.P; j += gridDim.x * blockDim.x) {
    const double x = box_clamp(F.W.x[j], lower[j], upper[j]);
    F.W.x[j] = x;
    F.W.t[j] = x;
    const int jl = F.inv[j];
    if (jl >= 0) F.xl[jl] = x;
  }
}

void fe_box_enqueue_check(const double* lower, const double* upper, int P, int ic, int32_t* bad_dev, hipStream_t s) {
  hipLaunchKernelGGL(fe_box_check_kernel, dim3(grid_for(P, 256, 1024)), dim3(256), 0, s, lower, upper, P, ic, bad_dev);
}

void fe_box_enqueue_start(const FeDev& F, const double* lower, const double* upper, hipStream_t s) {
  hipLaunchKernelGGL(fe_box_start_kernel, dim3(grid_for(F.P, 256, 1024)), dim3(256), 0, s, F, lower, upper);
}

}  // namespace gdmix
