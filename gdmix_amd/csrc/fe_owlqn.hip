// fe_owlqn.hip — the fixed effect's second step: OWL-QN (Andrew & Gao 2007) for  F = smooth + l1 |theta_R|_1  (include/gdmix_fe.h,
// "(ABI 23) L1 / elastic net"). It consumes the same all-reduced [gradient, value] buffer as the L-BFGS-B step of fe_solve.hip and
// lives in the same pool, state record, plan and m x m matrices; gdmix_fe_set_l1 selects it per problem. Three ordinary launches per
// evaluation — products, decision, update — and no kernel of this unit waits on another workgroup: a launch boundary is the only
// synchronisation.
//
// The pool's vectors under this step (Work of re_solve_core.hpp):
//     W.x  the TRIAL point, the one the passes evaluate (the row pass reads the intercept from W.x[D], the features from F.xl)
//     W.t  the last ACCEPTED point x (what gdmix_fe_result returns)
//     W.g  the smooth gradient at x            W.r  the smooth gradient at the trial (the products pass leaves it for the update)
//     W.d  the search direction, sign-fixed    W.ws the (s, y) pairs, in re_lbfgs_compact.hpp's tile layout (compact_hist)
// The pseudo-gradient and the orthant are functions of (g_j, x_j) alone and are formed where they are needed, never stored.
#include "fe_internal.hpp"
#include "re_lbfgs_compact.hpp"
#include "../../include/gdmix_fe.h"

namespace gdmix {

// the products of one evaluation, per virtual block in F.acc_part and in total in the decision's LDS
enum {
  OW_X2 = 0,      // sum over R of trial_j^2
  OW_X1,          // sum over R of |trial_j|
  OW_ARM,         // pg'(trial - x): the Armijo term, pg the pseudo-gradient at x
  OW_SY,          // s'y,  s = trial - x,  y = g(trial) - g(x)
  OW_YY,          // y'y
  OW_PGMAX,       // max |pg+_j|, pg+ the pseudo-gradient at the trial
  OW_PG2,         // pg+'pg+
  OW_SPG,         // s'pg+
  OW_YPG,         // y'pg+
  OW_HSY,                            // S_i'y   (chronological i < col)
  OW_HYY = OW_HSY + TEAM_MCAP,       // Y_i'y
  OW_HSPG = OW_HYY + TEAM_MCAP,      // S_i'pg+
  OW_HYPG = OW_HSPG + TEAM_MCAP,     // Y_i'pg+
  OWL_K = OW_HYPG + TEAM_MCAP
};
constexpr int OWL_BLOCKS = 480;      // virtual blocks at most: their shares fit the L-BFGS-B step's acc_part
static_assert(OWL_BLOCKS * OWL_K <= FE_DOT_BLOCKS * COMPACT_KD, "the shares live in F.acc_part");
static_assert(OWL_K <= WAVE, "one lane per value");

// CompactPlan.action under this step. Both stops are idempotent: a step enqueued behind the stop repeats the plan.
enum {
  OA_STOP_ACCEPT = 0,   // the trial is the result: t := x
  OA_STOP_RESTORE,      // the last accepted point is the result: x := t
  OA_RETRY,             // backtrack: x := project(t + stp d)
  OA_STEEPEST,          // the search failed with pairs stored: memory cleared, d := -pg at t, x := project(t + stp d)
  OA_ACCEPT             // the trial becomes x: pair (plan.store_pair), new direction, first trial along it; plan.restore: the start point (no pair to form)
};
constexpr double OWL_ARMIJO = 1e-4;

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

// ---- 1. products: one pass over the coefficients, one read of the history ------------------------------------------------------------
// The share of virtual block vb of nvb — coefficients (vb * 256 + tid) + k * nvb * 256 — into acc_part[vb]; nvb is a function of P alone.
__global__ __launch_bounds__(FE_THREADS) void fe_owl_products_kernel(FeDev F, SolveParams o, double l1) {
  __shared__ double red[FE_WAVES][OWL_K];
  if (F.state->status >= 0) return;     // a step enqueued behind the stop is a no-op
  const int tid = threadIdx.x, lane = tid & (WAVE - 1), wv = tid >> 6;
  const int vb = blockIdx.x, nvb = gridDim.x;
  const int col = F.state->col, head = F.state->head, m = o.m, P = F.P;
  double acc[OWL_K];
#pragma unroll
  for (int k = 0; k < OWL_K; ++k) acc[k] = 0.0;
  for (int j = vb * FE_THREADS + tid; j < P; j += nvb * FE_THREADS) {
    const bool reg = (j < F.D) || o.regularize_bias;   // the intercept is coefficient D
    const double xt = F.W.x[j], xa = F.W.t[j], go = F.W.g[j];
    const double gn = F.fg[j] + (reg ? o.l2 * xt : 0.0);
    F.fg[j] = 0.0;   // consumed: the next evaluation starts from a clear buffer (gdmix_fe_eval)
    F.W.r[j] = gn;
    double2 h[TEAM_MCAP];   // all pairs requested before the first is used
#pragma unroll
    for (int i = 0; i < TEAM_MCAP; ++i) {
      int sl = head + i;
      if (sl >= m) sl -= m;
      if (i >= m) sl = 0;
      h[i] = compact_hist(F.W, m, j)[sl * COMPACT_HIST_STRIDE];
    }
    const double pgn = owl_pseudo(gn, xt, l1, reg), pgo = owl_pseudo(go, xa, l1, reg);
    const double sj = xt - xa, yj = gn - go;
    if (reg) { acc[OW_X2] += xt * xt; acc[OW_X1] += fabs(xt); }
    acc[OW_ARM] += pgo * sj;
    acc[OW_SY] += sj * yj;
    acc[OW_YY] += yj * yj;
    acc[OW_PGMAX] = fmax(acc[OW_PGMAX], fabs(pgn));
    acc[OW_PG2] += pgn * pgn;
    acc[OW_SPG] += sj * pgn;
    acc[OW_YPG] += yj * pgn;
#pragma unroll
    for (int i = 0; i < TEAM_MCAP; ++i) {
      const double hx = i < col ? h[i].x : 0.0, hy = i < col ? h[i].y : 0.0;
      acc[OW_HSY + i] += hx * yj;
      acc[OW_HYY + i] += hy * yj;
      acc[OW_HSPG + i] += hx * pgn;
      acc[OW_HYPG + i] += hy * pgn;
    }
  }
  double mine = 0.0;
#pragma unroll
  for (int k = 0; k < OWL_K; ++k) {
    const double t = (k == OW_PGMAX) ? wave_max_nonneg(acc[k]) : wave_sum(acc[k]);
    if (lane == k) mine = t;
  }
  if (lane < OWL_K) red[wv][lane] = mine;
  __syncthreads();
  if (tid < OWL_K) {
    double s = red[0][tid];
#pragma unroll
    for (int w = 1; w < FE_WAVES; ++w) s = (tid == OW_PGMAX) ? fmax(s, red[w][tid]) : s + red[w][tid];
    F.acc_part[(size_t)vb * OWL_K + tid] = s;
  }
}

// ---- 2. decision: one workgroup ----------------------------------------------------------------------------------------------------
// The m x m part by thread 0 on the replica in LDS: with R = triu(S'Y), D = diag(S'Y), gamma = s'y / y'y of the newest pair,
//     q = R^-1 S'pg,   u = R^-T ((D + gamma Y'Y) q - gamma Y'pg),   d = -H pg = gamma (Y q - pg) - S u      (Byrd, Nocedal & Schnabel)
__device__ __forceinline__ void owl_direction(CompactMats& L, int col, double gamma, const double* a, const double* b) {
  constexpr int LD = TEAM_MCAP;
  double q[TEAM_MCAP], w[TEAM_MCAP];
  for (int k = col - 1; k >= 0; --k) {
    double s = a[k];
    for (int c = k + 1; c < col; ++c) s -= L.SY[k * LD + c] * q[c];
    q[k] = s / L.SY[k * LD + k];
  }
  for (int i = 0; i < col; ++i) {
    double s = L.SY[i * LD + i] * q[i] - gamma * b[i];
    for (int k = 0; k < col; ++k) s += gamma * L.YY[i * LD + k] * q[k];
    w[i] = s;
  }
  for (int k = 0; k < col; ++k) {
    double s = w[k];
    for (int r = 0; r < k; ++r) s -= L.SY[r * LD + k] * L.u[r];
    L.u[k] = s / L.SY[k * LD + k];
    L.q[k] = q[k];
  }
}

__global__ __launch_bounds__(FE_THREADS) void fe_owl_decide_kernel(FeDev F, SolveParams o, double l1, int nvb, int32_t* status_out) {
  __shared__ double tot[OWL_K];
  __shared__ double part4[4][WAVE];
  __shared__ CompactMats mats;
  if (F.state->status >= 0) return;     // (status_out keeps the status of the stop; the update repeats the stop's plan: idempotent)
  const int tid = threadIdx.x;
  {
    // value v of block b by thread (b % 4) * 64 + v: four partial totals per value, combined in order
    static_assert(FE_THREADS == 4 * WAVE, "four groups of one lane per value");
    const int v = tid & (WAVE - 1), g = tid >> 6;
    if (v < OWL_K) {
      double s = 0.0;
      int b = g;
      for (; b + 28 < nvb; b += 32) {   // eight loads in flight
        double t[8];
#pragma unroll
        for (int q = 0; q < 8; ++q) t[q] = F.acc_part[(size_t)(b + 4 * q) * OWL_K + v];
#pragma unroll
        for (int q = 0; q < 8; ++q) s = (v == OW_PGMAX) ? fmax(s, t[q]) : s + t[q];
      }
      for (; b < nvb; b += 4) {
        const double t = F.acc_part[(size_t)b * OWL_K + v];
        s = (v == OW_PGMAX) ? fmax(s, t) : s + t;
      }
      part4[g][v] = s;
    }
    __syncthreads();
    if (tid < OWL_K) {
      double s = part4[0][tid];
#pragma unroll
      for (int k = 1; k < 4; ++k) s = (tid == OW_PGMAX) ? fmax(s, part4[k][tid]) : s + part4[k][tid];
      tot[tid] = s;
    }
  }
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
    plan.action = OA_STOP_ACCEPT; plan.store_pair = 0; plan.restore = 0; plan.slot = 0; plan.cnew = 0; plan.col = S.col; plan.head = S.head;
    plan.shift = 0; plan.phantom = 0; plan.stp = S.stp; plan.stp_prev = S.stp; plan.gamma = S.theta;
    const double fdata = F.fg[F.P];
    const double f_new = fdata + 0.5 * o.l2 * tot[OW_X2] + l1 * tot[OW_X1];
    if (fdata == -__builtin_inf()) {
      // the mark of a worker whose step was aborted, carried here by the all-reduce (fe_step_body): every worker stops in this evaluation
      S.status = GDMIX_RE_ST_ABORTED_PEER;
      plan.action = S.first ? OA_STOP_ACCEPT : OA_STOP_RESTORE;
    } else if (S.first) {
      S.first = 0;
      ++S.nfev;
      S.f = f_new; S.fold = f_new;
      S.sbgnrm = tot[OW_PGMAX];
      S.gg_k = tot[OW_PG2];
      if (S.sbgnrm <= o.pgtol) {
        S.status = 0;
      } else {
        S.stp = 1.0 / sqrt(S.gg_k);
        S.ifun = 0;
        plan.action = OA_ACCEPT; plan.restore = 1; plan.col = 0; plan.head = 0; plan.stp = S.stp;
      }
    } else if (f_new <= S.f + OWL_ARMIJO * tot[OW_ARM]) {
      ++S.nfev;
      ++S.nit;
      S.iter0 = 0;
      S.fold = S.f;
      S.f = f_new;
      S.ifun = 0;
      S.sbgnrm = tot[OW_PGMAX];
      S.gg_k = tot[OW_PG2];
      const double ddum = fmax(fabs(S.fold), fmax(fabs(S.f), 1.0));
      if (S.sbgnrm <= o.pgtol) S.status = 0;
      else if (S.fold - S.f <= o.ftol * ddum) S.status = 1;
      else if (S.nit >= o.max_iter) S.status = 2;
      else if (S.nfev > o.maxfun) S.status = 3;
      else {
        const double sy = tot[OW_SY], yy = tot[OW_YY];
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
            mats.SY[i * LD + cnew] = tot[OW_HSY + i + off];
            mats.YY[i * LD + cnew] = tot[OW_HYY + i + off];
            mats.YY[cnew * LD + i] = tot[OW_HYY + i + off];
            a[i] = tot[OW_HSPG + i + off];
            b[i] = tot[OW_HYPG + i + off];
          }
          mats.SY[cnew * LD + cnew] = sy;
          mats.YY[cnew * LD + cnew] = yy;
          a[cnew] = tot[OW_SPG];
          b[cnew] = tot[OW_YPG];
          S.theta = sy / yy;      // gamma of H0, from the newest pair
          plan.store_pair = 1; plan.slot = slot; plan.cnew = cnew; plan.shift = off;
        } else {
          for (int i = 0; i < col; ++i) { a[i] = tot[OW_HSPG + i]; b[i] = tot[OW_HYPG + i]; }
        }
        if (col > 0) owl_direction(mats, col, S.theta, a, b);
        S.col = col; S.head = head;
        S.stp = col > 0 ? 1.0 : 1.0 / sqrt(S.gg_k);
        plan.action = OA_ACCEPT; plan.col = col; plan.head = head; plan.stp = S.stp; plan.gamma = S.theta;
      }
    } else {
      ++S.nfev;
      ++S.ifun;      // rejected trials of this iteration
      if (S.ifun < o.maxls) {
        S.stp *= 0.5;
        plan.action = OA_RETRY; plan.stp = S.stp;
      } else if (S.col > 0) {
        S.col = 0; S.head = 0; S.ifun = 0;
        S.stp = 1.0 / sqrt(S.gg_k);
        plan.action = OA_STEEPEST; plan.col = 0; plan.head = 0; plan.stp = S.stp;
      } else {
        S.status = 4;
        plan.action = OA_STOP_RESTORE;
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
__global__ __launch_bounds__(256) void fe_owl_update_kernel(FeDev F, SolveParams o, double l1) {
  const CompactPlan plan = *F.plan;
  const CompactMats& L = *F.mats;
  const int m = o.m;
  for (int j = blockIdx.x * blockDim.x + threadIdx.x; j < F.P; j += gridDim.x * blockDim.x) {
    const bool reg = (j < F.D) || o.regularize_bias;
    double xn;
    if (plan.action == OA_STOP_ACCEPT) {
      F.W.t[j] = F.W.x[j];
      continue;      // (the trial is already what the passes read)
    } else if (plan.action == OA_STOP_RESTORE) {
      xn = F.W.t[j];
    } else if (plan.action == OA_RETRY) {      // reads x, g, d only: never the stored pairs
      const double xa = F.W.t[j];
      xn = owl_trial(xa, F.W.d[j], owl_pseudo(F.W.g[j], xa, l1, reg), plan.stp);
    } else if (plan.action == OA_STEEPEST) {
      const double xa = F.W.t[j];
      const double pg = owl_pseudo(F.W.g[j], xa, l1, reg);
      F.W.d[j] = -pg;
      xn = owl_trial(xa, -pg, pg, plan.stp);
    } else {
      const double xt = F.W.x[j], gn = F.W.r[j];
      const double sn = xt - F.W.t[j], yn = gn - F.W.g[j];
      if (plan.store_pair) compact_hist(F.W, m, j)[plan.slot * COMPACT_HIST_STRIDE] = make_double2(sn, yn);
      F.W.t[j] = xt;
      F.W.g[j] = gn;
      const double pg = owl_pseudo(gn, xt, l1, reg);
      double dj = -pg;
      if (plan.col > 0) {
        double2 h[TEAM_MCAP];   // every pair is requested before the first is used
#pragma unroll
        for (int i = 0; i < TEAM_MCAP; ++i) {
          int sl = plan.head + i;
          if (sl >= m) sl -= m;
          if (i >= m) sl = 0;
          h[i] = compact_hist(F.W, m, j)[sl * COMPACT_HIST_STRIDE];
        }
        double su = 0.0, yq = 0.0;
#pragma unroll
        for (int i = 0; i < TEAM_MCAP; ++i) {
          if (i < plan.col) {
            const bool fresh = plan.store_pair && i == plan.cnew;
            su += L.u[i] * (fresh ? sn : h[i].x);
            yq += L.q[i] * (fresh ? yn : h[i].y);
          }
        }
        dj = plan.gamma * (yq - pg) - su;
      }
      if (dj * pg >= 0.0) dj = 0.0;      // the direction stays in the orthant the pseudo-gradient points into
      F.W.d[j] = dj;
      xn = owl_trial(xt, dj, pg, plan.stp);
    }
    F.W.x[j] = xn;
    const int jl = F.inv[j];
    if (jl >= 0) F.xl[jl] = xn;
  }
}

void fe_owlqn_enqueue_step(const FeDev& F, const SolveParams& o, double l1, int32_t* status_dev, hipStream_t s) {
  const int nvb = grid_for(F.P, FE_THREADS, OWL_BLOCKS);
  hipLaunchKernelGGL(fe_owl_products_kernel, dim3(nvb), dim3(FE_THREADS), 0, s, F, o, l1);
  hipLaunchKernelGGL(fe_owl_decide_kernel, dim3(1), dim3(FE_THREADS), 0, s, F, o, l1, nvb, status_dev);
  hipLaunchKernelGGL(fe_owl_update_kernel, dim3(grid_for(F.P, 256, 1024)), dim3(256), 0, s, F, o, l1);
}

}  // namespace gdmix
