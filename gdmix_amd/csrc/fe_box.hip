// fe_box.hip — the fixed effect's fourth step: projected L-BFGS for the smooth objective inside a box  lo <= theta <= hi  (include/gdmix_fe.h,
// "(ABI 26) box constraints"). It consumes the same all-reduced [gradient, value] buffer as the other steps and lives in the same pool,
// state record, plan and m x m matrices; gdmix_fe_set_bounds selects it per problem. Modelled on fe_owlqn.hip: three ordinary launches per
// evaluation — products, decision, update — and no kernel of this unit waits on another workgroup: a launch boundary is the only
// synchronisation. The bounds are two vectors of the problem's own (fe_solve.hip: box_mem) and arrive as kernel arguments: FeDev keeps its
// layout.
//
// The pool's vectors under this step (Work of re_solve_core.hpp), as under OWL-QN:
//     W.x  the TRIAL point, the one the passes evaluate (the row pass reads the intercept from W.x[D], the features from F.xl)
//     W.t  the last ACCEPTED point x (what gdmix_fe_result returns)
//     W.g  the gradient at x                   W.r  the gradient at the trial (the products pass leaves it for the update)
//     W.d  the search direction, zero on the binding set      W.ws the (s, y) pairs, in re_lbfgs_compact.hpp's tile layout (compact_hist)
// The binding set, the reduced gradient and the projected gradient are functions of (g_j, x_j, lo_j, hi_j) alone and are formed where they
// are needed, never stored. The intercept's bounds are -inf / +inf (gdmix_fe_set_bounds checks it), so no kernel treats it apart.
#include "fe_internal.hpp"
#include "re_lbfgs_compact.hpp"
#include "../../include/gdmix_fe.h"

namespace gdmix {

// the products of one evaluation, per virtual block in F.acc_part and in total in the decision's LDS. q+ is the reduced gradient at the trial.
enum {
  BX_X2 = 0,      // sum over R of trial_j^2
  BX_ARM,         // g'(trial - x): the Armijo term, g the gradient at x
  BX_SY,          // s'y,  s = trial - x,  y = g(trial) - g(x)
  BX_YY,          // y'y
  BX_PGMAX,       // max |trial_j - clamp(trial_j - g+_j)|: the projected gradient at the trial
  BX_Q2,          // q+'q+
  BX_SQ,          // s'q+
  BX_YQ,          // y'q+
  BX_HSY,                            // S_i'y   (chronological i < col)
  BX_HYY = BX_HSY + TEAM_MCAP,       // Y_i'y
  BX_HSQ = BX_HYY + TEAM_MCAP,       // S_i'q+
  BX_HYQ = BX_HSQ + TEAM_MCAP,       // Y_i'q+
  BOX_K = BX_HYQ + TEAM_MCAP
};
constexpr int BOX_BLOCKS = 480;      // virtual blocks at most: their shares fit the L-BFGS-B step's acc_part
static_assert(BOX_BLOCKS * BOX_K <= FE_DOT_BLOCKS * COMPACT_KD, "the shares live in F.acc_part");
static_assert(BOX_K <= WAVE, "one lane per value");

// CompactPlan.action under this step: OWL-QN's. Both stops are idempotent: a step enqueued behind the stop repeats the plan.
enum {
  BA_STOP_ACCEPT = 0,   // the trial is the result: t := x
  BA_STOP_RESTORE,      // the last accepted point is the result: x := t
  BA_RETRY,             // backtrack: x := clamp(t + stp d)
  BA_STEEPEST,          // the search failed with pairs stored: memory cleared, d := -q at t, x := clamp(t + stp d)
  BA_ACCEPT             // the trial becomes x: pair (plan.store_pair), new direction, first trial along it
};
constexpr double BOX_ARMIJO = 1e-4;

__device__ __forceinline__ double box_clamp(double v, double lo, double hi) { return v < lo ? lo : (v > hi ? hi : v); }      // exactly the bound's double
// j is in the binding set: at a bound with the gradient pushing out of the box, or pinned
__device__ __forceinline__ bool box_binding(double g, double x, double lo, double hi) {
  return (x <= lo && g > 0.0) || (x >= hi && g < 0.0) || lo == hi;
}
// the direction entry as it is used: 0 on the binding set, and where x sits at a bound and d points out of the box
__device__ __forceinline__ double box_direction(double d, bool binding, double x, double lo, double hi) {
  return (binding || (x <= lo && d < 0.0) || (x >= hi && d > 0.0)) ? 0.0 : d;
}

// ---- 1. products: one pass over the coefficients, one read of the history ------------------------------------------------------------
// The share of virtual block vb of nvb — coefficients (vb * 256 + tid) + k * nvb * 256 — into acc_part[vb]; nvb is a function of P alone.
__global__ __launch_bounds__(FE_THREADS) void fe_box_products_kernel(FeDev F, SolveParams o, const double* __restrict__ lower,
                                                                     const double* __restrict__ upper) {
  __shared__ double red[FE_WAVES][BOX_K];
  if (F.state->status >= 0) return;     // a step enqueued behind the stop is a no-op
  const int tid = threadIdx.x, lane = tid & (WAVE - 1), wv = tid >> 6;
  const int vb = blockIdx.x, nvb = gridDim.x;
  const int col = F.state->col, head = F.state->head, m = o.m, P = F.P;
  double acc[BOX_K];
#pragma unroll
  for (int k = 0; k < BOX_K; ++k) acc[k] = 0.0;
  for (int j = vb * FE_THREADS + tid; j < P; j += nvb * FE_THREADS) {
    const bool reg = (j < F.D) || o.regularize_bias;   // the intercept is coefficient D
    const double xt = F.W.x[j], xa = F.W.t[j], go = F.W.g[j], lo = lower[j], hi = upper[j];
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
    const double qn = box_binding(gn, xt, lo, hi) ? 0.0 : gn;
    const double sj = xt - xa, yj = gn - go;
    if (reg) acc[BX_X2] += xt * xt;
    acc[BX_ARM] += go * sj;
    acc[BX_SY] += sj * yj;
    acc[BX_YY] += yj * yj;
    acc[BX_PGMAX] = fmax(acc[BX_PGMAX], fabs(xt - box_clamp(xt - gn, lo, hi)));
    acc[BX_Q2] += qn * qn;
    acc[BX_SQ] += sj * qn;
    acc[BX_YQ] += yj * qn;
#pragma unroll
    for (int i = 0; i < TEAM_MCAP; ++i) {
      const double hx = i < col ? h[i].x : 0.0, hy = i < col ? h[i].y : 0.0;
      acc[BX_HSY + i] += hx * yj;
      acc[BX_HYY + i] += hy * yj;
      acc[BX_HSQ + i] += hx * qn;
      acc[BX_HYQ + i] += hy * qn;
    }
  }
  double mine = 0.0;
#pragma unroll
  for (int k = 0; k < BOX_K; ++k) {
    const double t = (k == BX_PGMAX) ? wave_max_nonneg(acc[k]) : wave_sum(acc[k]);
    if (lane == k) mine = t;
  }
  if (lane < BOX_K) red[wv][lane] = mine;
  __syncthreads();
  if (tid < BOX_K) {
    double s = red[0][tid];
#pragma unroll
    for (int w = 1; w < FE_WAVES; ++w) s = (tid == BX_PGMAX) ? fmax(s, red[w][tid]) : s + red[w][tid];
    F.acc_part[(size_t)vb * BOX_K + tid] = s;
  }
}

// ---- 2. decision: one workgroup ----------------------------------------------------------------------------------------------------
// The m x m part by thread 0 on the replica in LDS, as under OWL-QN with the reduced gradient q in the pseudo-gradient's place: with
// R = triu(S'Y), D = diag(S'Y), gamma = s'y / y'y of the newest pair,
//     c = R^-1 S'q,   u = R^-T ((D + gamma Y'Y) c - gamma Y'q),   d = -H q = gamma (Y c - q) - S u      (Byrd, Nocedal & Schnabel)
__device__ __forceinline__ void box_direction_coefficients(CompactMats& L, int col, double gamma, const double* a, const double* b) {
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

__global__ __launch_bounds__(FE_THREADS) void fe_box_decide_kernel(FeDev F, SolveParams o, int nvb, int32_t* status_out) {
  __shared__ double tot[BOX_K];
  __shared__ double part4[4][WAVE];
  __shared__ CompactMats mats;
  if (F.state->status >= 0) return;     // (status_out keeps the status of the stop; the update repeats the stop's plan: idempotent)
  const int tid = threadIdx.x;
  {
    // value v of block b by thread (b % 4) * 64 + v: four partial totals per value, combined in order
    static_assert(FE_THREADS == 4 * WAVE, "four groups of one lane per value");
    const int v = tid & (WAVE - 1), g = tid >> 6;
    if (v < BOX_K) {
      double s = 0.0;
      int b = g;
      for (; b + 28 < nvb; b += 32) {   // eight loads in flight
        double t[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) t[e] = F.acc_part[(size_t)(b + 4 * e) * BOX_K + v];
#pragma unroll
        for (int e = 0; e < 8; ++e) s = (v == BX_PGMAX) ? fmax(s, t[e]) : s + t[e];
      }
      for (; b < nvb; b += 4) {
        const double t = F.acc_part[(size_t)b * BOX_K + v];
        s = (v == BX_PGMAX) ? fmax(s, t) : s + t;
      }
      part4[g][v] = s;
    }
    __syncthreads();
    if (tid < BOX_K) {
      double s = part4[0][tid];
#pragma unroll
      for (int k = 1; k < 4; ++k) s = (tid == BX_PGMAX) ? fmax(s, part4[k][tid]) : s + part4[k][tid];
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
    plan.action = BA_STOP_ACCEPT; plan.store_pair = 0; plan.restore = 0; plan.slot = 0; plan.cnew = 0; plan.col = S.col; plan.head = S.head;
    plan.shift = 0; plan.phantom = 0; plan.stp = S.stp; plan.stp_prev = S.stp; plan.gamma = S.theta;
    const double fdata = F.fg[F.P];
    const double f_new = fdata + 0.5 * o.l2 * tot[BX_X2];
    if (fdata == -__builtin_inf()) {
      // the mark of a worker whose step was aborted, carried here by the all-reduce (fe_step_body): every worker stops in this evaluation
      S.status = GDMIX_RE_ST_ABORTED_PEER;
      plan.action = S.first ? BA_STOP_ACCEPT : BA_STOP_RESTORE;
    } else if (S.first) {
      S.first = 0;
      ++S.nfev;
      S.f = f_new; S.fold = f_new;
      S.sbgnrm = tot[BX_PGMAX];
      S.gg_k = tot[BX_Q2];
      if (S.sbgnrm <= o.pgtol) {
        S.status = 0;
      } else {
        S.stp = 1.0 / sqrt(S.gg_k);
        S.ifun = 0;
        plan.action = BA_ACCEPT; plan.restore = 1; plan.col = 0; plan.head = 0; plan.stp = S.stp;
      }
    } else if (f_new <= S.f + BOX_ARMIJO * tot[BX_ARM]) {
      ++S.nfev;
      ++S.nit;
      S.iter0 = 0;
      S.fold = S.f;
      S.f = f_new;
      S.ifun = 0;
      S.sbgnrm = tot[BX_PGMAX];
      S.gg_k = tot[BX_Q2];
      const double ddum = fmax(fabs(S.fold), fmax(fabs(S.f), 1.0));
      if (S.sbgnrm <= o.pgtol) S.status = 0;
      else if (S.fold - S.f <= o.ftol * ddum) S.status = 1;
      else if (S.nit >= o.max_iter) S.status = 2;
      else if (S.nfev > o.maxfun) S.status = 3;
      else {
        const double sy = tot[BX_SY], yy = tot[BX_YY];
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
            mats.SY[i * LD + cnew] = tot[BX_HSY + i + off];
            mats.YY[i * LD + cnew] = tot[BX_HYY + i + off];
            mats.YY[cnew * LD + i] = tot[BX_HYY + i + off];
            a[i] = tot[BX_HSQ + i + off];
            b[i] = tot[BX_HYQ + i + off];
          }
          mats.SY[cnew * LD + cnew] = sy;
          mats.YY[cnew * LD + cnew] = yy;
          a[cnew] = tot[BX_SQ];
          b[cnew] = tot[BX_YQ];
          S.theta = sy / yy;      // gamma of H0, from the newest pair
          plan.store_pair = 1; plan.slot = slot; plan.cnew = cnew; plan.shift = off;
        } else {
          for (int i = 0; i < col; ++i) { a[i] = tot[BX_HSQ + i]; b[i] = tot[BX_HYQ + i]; }
        }
        if (col > 0) box_direction_coefficients(mats, col, S.theta, a, b);
        S.col = col; S.head = head;
        S.stp = col > 0 ? 1.0 : 1.0 / sqrt(S.gg_k);
        plan.action = BA_ACCEPT; plan.col = col; plan.head = head; plan.stp = S.stp; plan.gamma = S.theta;
      }
    } else {
      ++S.nfev;
      ++S.ifun;      // rejected trials of this iteration
      if (S.ifun < o.maxls) {
        S.stp *= 0.5;
        plan.action = BA_RETRY; plan.stp = S.stp;
      } else if (S.col > 0) {
        S.col = 0; S.head = 0; S.ifun = 0;
        S.stp = 1.0 / sqrt(S.gg_k);
        plan.action = BA_STEEPEST; plan.col = 0; plan.head = 0; plan.stp = S.stp;
      } else {
        S.status = 4;
        plan.action = BA_STOP_RESTORE;
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
__global__ __launch_bounds__(256) void fe_box_update_kernel(FeDev F, SolveParams o, const double* __restrict__ lower,
                                                            const double* __restrict__ upper) {
  const CompactPlan plan = *F.plan;
  const CompactMats& L = *F.mats;
  const int m = o.m;
  for (int j = blockIdx.x * blockDim.x + threadIdx.x; j < F.P; j += gridDim.x * blockDim.x) {
    double xn;
    if (plan.action == BA_STOP_ACCEPT) {
      F.W.t[j] = F.W.x[j];
      continue;      // (the trial is already what the passes read)
    } else if (plan.action == BA_STOP_RESTORE) {
      xn = F.W.t[j];
    } else if (plan.action == BA_RETRY) {      // reads x, d and the bounds only: never the stored pairs
      xn = box_clamp(F.W.t[j] + plan.stp * F.W.d[j], lower[j], upper[j]);
    } else if (plan.action == BA_STEEPEST) {
      const double xa = F.W.t[j], ga = F.W.g[j], lo = lower[j], hi = upper[j];
      const bool binding = box_binding(ga, xa, lo, hi);
      const double dj = box_direction(-ga, binding, xa, lo, hi);
      F.W.d[j] = dj;
      xn = box_clamp(xa + plan.stp * dj, lo, hi);
    } else {
      const double xt = F.W.x[j], gn = F.W.r[j], lo = lower[j], hi = upper[j];
      const double sn = xt - F.W.t[j], yn = gn - F.W.g[j];
      if (plan.store_pair) compact_hist(F.W, m, j)[plan.slot * COMPACT_HIST_STRIDE] = make_double2(sn, yn);
      F.W.t[j] = xt;
      F.W.g[j] = gn;
      const bool binding = box_binding(gn, xt, lo, hi);
      const double qj = binding ? 0.0 : gn;
      double dj = -qj;
      if (plan.col > 0) {
        double2 h[TEAM_MCAP];   // every pair is requested before the first is used
#pragma unroll
        for (int i = 0; i < TEAM_MCAP; ++i) {
          int sl = plan.head + i;
          if (sl >= m) sl -= m;
          if (i >= m) sl = 0;
          h[i] = compact_hist(F.W, m, j)[sl * COMPACT_HIST_STRIDE];
        }
        double su = 0.0, yc = 0.0;
#pragma unroll
        for (int i = 0; i < TEAM_MCAP; ++i) {
          if (i < plan.col) {
            const bool fresh = plan.store_pair && i == plan.cnew;
            su += L.u[i] * (fresh ? sn : h[i].x);
            yc += L.q[i] * (fresh ? yn : h[i].y);
          }
        }
        dj = plan.gamma * (yc - qj) - su;
      }
      dj = box_direction(dj, binding, xt, lo, hi);
      F.W.d[j] = dj;
      xn = box_clamp(xt + plan.stp * dj, lo, hi);
    }
    F.W.x[j] = xn;
    const int jl = F.inv[j];
    if (jl >= 0) F.xl[jl] = xn;
  }
}

void fe_box_enqueue_step(const FeDev& F, const SolveParams& o, const double* lower, const double* upper, int32_t* status_dev, hipStream_t s) {
  const int nvb = grid_for(F.P, FE_THREADS, BOX_BLOCKS);
  hipLaunchKernelGGL(fe_box_products_kernel, dim3(nvb), dim3(FE_THREADS), 0, s, F, o, lower, upper);
  hipLaunchKernelGGL(fe_box_decide_kernel, dim3(1), dim3(FE_THREADS), 0, s, F, o, nvb, status_dev);
  hipLaunchKernelGGL(fe_box_update_kernel, dim3(grid_for(F.P, 256, 1024)), dim3(256), 0, s, F, o, lower, upper);
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
