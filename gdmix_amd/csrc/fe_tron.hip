// fe_tron.hip — the fixed effect's third step: trust-region Newton (Lin, Weng & Keerthi 2008; LIBLINEAR's tron) for the smooth objective
// F = data + (l2/2) |theta_R|^2 (include/gdmix_fe.h, "(ABI 24) TRON", is the definition). gdmix_fe_set_optimizer selects it per problem.
// It consumes the same all-reduced buffer as the other two steps, through the same status ring, lookahead and stop flag; what differs
// is that a pass pair of a TRON problem is either an evaluation at the trial point or a Hessian-vector product with the CG direction
// (the HV variant of the row kernels, fe_solve.hip), and that this step says which comes next: it writes FeTronState.mode. Three
// ordinary launches per pass pair — products, decision, update — and a launch boundary is the only synchronisation.
//
// Vectors: W.x (the pool's) is the ACCEPTED point, what gdmix_fe_result returns; everything else lives in the TRON buffer
// (fe_internal.hpp: FeTron): s, r, d of Steihaug's CG, h = what the last pass pair left with the regulariser added (H d after a
// product, the gradient at the trial after an evaluation), xt the trial point x + s, g the gradient at x, vl the direction in the
// shard's local order, c[2] the curvature weights of the accepted point and of the trial.
#include "fe_step_shares.hpp"
#include "re_lbfgs_compact.hpp"
#include "../../include/gdmix_fe.h"

namespace gdmix {

// the sums of one step, per virtual block in F.acc_part and in total in the decision's LDS (fe_step_shares.hpp)
enum {
  // after an evaluation                        after a product
  TS_X2 = 0,      // sum over R of xt_j^2       d'Hd
  TS_GG = 1,      // gn'gn, gn = h              r'Hd
  TS_GS = 2,      // g's                        Hd'Hd
  TS_SR = 3,      // s'r                        s'd
  TS_SS = 4,      // s's                        s's
  TS_DD = 5,      // -                          d'd
  TS_GMAX = 6,    // max |gn_j|                 -
  TRON_K = 7
};
static_assert(TRON_K <= WAVE && FE_DOT_BLOCKS * TRON_K <= FE_DOT_BLOCKS * COMPACT_KD, "the shares live in F.acc_part");

// FeTronState.action: what the update does. Every stop is idempotent: a step enqueued behind the stop returns in its first two launches
// and repeats the plan in the third.
enum {
  TA_NONE = 0,          // stopped where the accepted point is the result (the start point, a rejected trial): nothing moves
  TA_STOP_ACCEPT,       // stopped on an accepted trial: x := xt, g := h
  TA_CG_ACCEPT,         // the trial is accepted: x := xt, g := h, then CG starts: s = 0, r = d = -g
  TA_CG_AGAIN,          // the trial is rejected (or this is the start point, whose gradient the products pass left in g): CG starts at x again
  TA_CG_NEXT,           // s += coef d, r -= coef h, d = r + beta d
  TA_TRIAL              // s += coef d, r -= coef h, xt = x + s: CG has ended, an evaluation comes next
};
constexpr double TRON_ETA0 = 1e-4, TRON_ETA1 = 0.25, TRON_ETA2 = 0.75;
constexpr double TRON_SIGMA1 = 0.25, TRON_SIGMA2 = 0.5, TRON_SIGMA3 = 4.0;
constexpr double TRON_CG_TOL = 0.1;

// ---- 1. products: one pass over the coefficients -------------------------------------------------------------------------------------
// The share of virtual block vb of nvb — coefficients (vb * 256 + tid) + k * nvb * 256 — into acc_part[vb]; nvb is a function of P alone.
__global__ __launch_bounds__(FE_THREADS) void fe_tron_products_kernel(FeDev F, SolveParams o) {
  if (F.state->status >= 0) return;     // a step enqueued behind the stop is a no-op
  const FeTron T = fe_tron_of(F);
  const int tid = threadIdx.x, vb = blockIdx.x, nvb = gridDim.x, P = F.P;
  const bool product = T.st->mode == FE_TM_PRODUCT;      // uniform
  const bool first = F.state->first != 0;
  double acc[TRON_K];
#pragma unroll
  for (int k = 0; k < TRON_K; ++k) acc[k] = 0.0;
  for (int j = vb * FE_THREADS + tid; j < P; j += nvb * FE_THREADS) {
    const bool reg = (j < F.D) || o.regularize_bias;   // the intercept is coefficient D
    const double fj = F.fg[j];
    F.fg[j] = 0.0;   // consumed: the next pass pair starts from a clear buffer (gdmix_fe_eval)
    const double sj = T.s[j];
    if (product) {
      const double dj = T.d[j], rj = T.r[j];
      const double hj = fj + (reg ? o.l2 * dj : 0.0);      // l2 d_R is added once, here, behind the reduce
      T.h[j] = hj;
      acc[TS_X2] += dj * hj;
      acc[TS_GG] += rj * hj;
      acc[TS_GS] += hj * hj;
      acc[TS_SR] += sj * dj;
      acc[TS_SS] += sj * sj;
      acc[TS_DD] += dj * dj;
    } else {
      const double xj = T.xt[j];
      const double gn = fj + (reg ? o.l2 * xj : 0.0);
      if (first) T.g[j] = gn;      // the start point is accepted as it is: its gradient goes where the update finds it
      else T.h[j] = gn;
      if (reg) acc[TS_X2] += xj * xj;
      acc[TS_GG] += gn * gn;
      acc[TS_GS] += T.g[j] * sj;      // (s = 0 at the start point)
      acc[TS_SR] += sj * T.r[j];
      acc[TS_SS] += sj * sj;
      acc[TS_GMAX] = fmax(acc[TS_GMAX], fabs(gn));
    }
  }
  fe_shares_store<TRON_K, TS_GMAX>(acc, F.acc_part, vb);
}

// ---- 2. decision: one workgroup ------------------------------------------------------------------------------------------------------
// CG starts at the accepted point: s = 0, r = d = -g (the update forms them), r'r = g'g
__device__ __forceinline__ void tron_start_cg(FeTronState& R, int action) {
  R.rr = R.gg;
  R.ncg = 0;
  R.action = action;
  R.mode = FE_TM_PRODUCT;
}

__global__ __launch_bounds__(FE_THREADS) void fe_tron_decide_kernel(FeDev F, SolveParams o, int nvb, int32_t* status_out) {
  __shared__ double tot[TRON_K];
  if (F.state->status >= 0) return;     // (status_out keeps the status of the stop; the update repeats the stop's plan: idempotent)
  const int tid = threadIdx.x;
  fe_shares_total<TRON_K, TS_GMAX>(F.acc_part, nvb, tot);
  __syncthreads();
  if (tid != 0) return;
  const FeTron T = fe_tron_of(F);
  CompactState S = *F.state;
  FeTronState R = *T.st;
  const double fdata = F.fg[F.P];
  if (fdata == -__builtin_inf()) {
    // the mark of a worker whose step was aborted, carried here by the all-reduce (fe_step_body): every worker stops in this pass pair
    S.status = GDMIX_RE_ST_ABORTED_PEER;
    R.action = TA_NONE;
  } else if (R.mode == FE_TM_PRODUCT) {
    ++R.ncg;
    ++R.nhv;
    const double dhd = tot[TS_X2], rh = tot[TS_GG], hh = tot[TS_GS], sd = tot[TS_SR], ss = tot[TS_SS], dd = tot[TS_DD];
    const double alpha = R.rr / dhd;
    const double dsq = R.delta * R.delta;
    R.mode = FE_TM_EVAL;
    R.action = TA_TRIAL;
    if (!(dhd > 0.0) || ss + 2.0 * alpha * sd + alpha * alpha * dd > dsq) {
      // to the boundary: the non-negative root of |s + tau d| = delta, in the form without cancellation
      const double gap = fmax(dsq - ss, 0.0);
      const double rad = sqrt(sd * sd + dd * gap);
      R.coef = sd >= 0.0 ? gap / (sd + rad) : (rad - sd) / dd;
    } else {
      R.coef = alpha;
      const double rr_new = fmax(R.rr - 2.0 * alpha * rh + alpha * alpha * hh, 0.0);      // |r - alpha Hd|^2
      if (!(sqrt(rr_new) <= TRON_CG_TOL * R.gnorm) && R.ncg < GDMIX_FE_TRON_MAX_CG) {
        R.beta = rr_new / R.rr;
        R.rr = rr_new;
        R.mode = FE_TM_PRODUCT;
        R.action = TA_CG_NEXT;
      }
    }
  } else {
    const double f_new = fdata + 0.5 * o.l2 * tot[TS_X2];
    ++S.nfev;
    if (S.first) {
      S.first = 0;
      S.f = f_new; S.fold = f_new;
      S.sbgnrm = tot[TS_GMAX];
      R.gg = tot[TS_GG];
      R.gnorm = sqrt(R.gg);
      R.cur ^= 1;      // the curvature weights this evaluation wrote are the accepted point's
      if (S.sbgnrm <= o.pgtol) {
        S.status = 0;
        R.action = TA_NONE;
      } else {
        R.delta = R.gnorm;
        tron_start_cg(R, TA_CG_AGAIN);
      }
    } else {
      const double gs = tot[TS_GS], snorm = sqrt(tot[TS_SS]);
      const double prered = -0.5 * (gs - tot[TS_SR]);
      const double actred = S.f - f_new;
      if (!R.moved) R.delta = fmin(R.delta, snorm);
      const double curv = f_new - S.f - gs;
      const double ah = curv <= 0.0 ? TRON_SIGMA3 : fmax(TRON_SIGMA1, -0.5 * (gs / curv));
      // (a value that is not a number takes the first branch and is rejected)
      if (!(actred >= TRON_ETA0 * prered)) R.delta = fmin(fmax(ah, TRON_SIGMA1) * snorm, TRON_SIGMA2 * R.delta);
      else if (actred < TRON_ETA1 * prered) R.delta = fmax(TRON_SIGMA1 * R.delta, fmin(ah * snorm, TRON_SIGMA2 * R.delta));
      else if (actred < TRON_ETA2 * prered) R.delta = fmax(TRON_SIGMA1 * R.delta, fmin(ah * snorm, TRON_SIGMA3 * R.delta));
      else R.delta = fmax(R.delta, fmin(ah * snorm, TRON_SIGMA3 * R.delta));
      if (actred > TRON_ETA0 * prered) {
        ++S.nit;
        R.moved = 1;
        R.nrej = 0;
        R.cur ^= 1;
        S.fold = S.f;
        S.f = f_new;
        S.sbgnrm = tot[TS_GMAX];
        R.gg = tot[TS_GG];
        R.gnorm = sqrt(R.gg);
        const double ddum = fmax(fabs(S.fold), fmax(fabs(S.f), 1.0));
        if (S.sbgnrm <= o.pgtol) S.status = 0;
        else if (S.fold - S.f <= o.ftol * ddum) S.status = 1;
        else if (S.nit >= o.max_iter) S.status = 2;
        else if (S.nfev > o.maxfun) S.status = 3;
        if (S.status >= 0) R.action = TA_STOP_ACCEPT;
        else tron_start_cg(R, TA_CG_ACCEPT);
      } else {
        ++R.nrej;
        if (S.nfev > o.maxfun) S.status = 3;
        else if (R.nrej >= o.maxls) S.status = 4;
        if (S.status >= 0) R.action = TA_NONE;
        else tron_start_cg(R, TA_CG_AGAIN);
      }
    }
  }
  *F.state = S;        // (read by later launches only)
  *T.st = R;
  *status_out = S.status;
}

// ---- 3. update: elementwise ------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void fe_tron_update_kernel(FeDev F) {
  const FeTron T = fe_tron_of(F);
  const int action = T.st->action;
  if (action == TA_NONE) return;
  const double coef = T.st->coef, beta = T.st->beta;
  for (int j = blockIdx.x * blockDim.x + threadIdx.x; j < F.P; j += gridDim.x * blockDim.x) {
    const int jl = F.inv[j];
    if (action == TA_STOP_ACCEPT || action == TA_CG_ACCEPT) {
      F.W.x[j] = T.xt[j];
      T.g[j] = T.h[j];
    }
    if (action == TA_STOP_ACCEPT) continue;
    if (action == TA_CG_ACCEPT || action == TA_CG_AGAIN) {
      const double nj = -T.g[j];
      T.s[j] = 0.0;
      T.r[j] = nj;
      T.d[j] = nj;
      if (jl >= 0) T.vl[jl] = nj;
      continue;
    }
    const double dj = T.d[j];
    const double sj = T.s[j] + coef * dj, rj = T.r[j] - coef * T.h[j];
    T.s[j] = sj;
    T.r[j] = rj;
    if (action == TA_CG_NEXT) {
      const double dn = rj + beta * dj;
      T.d[j] = dn;
      if (jl >= 0) T.vl[jl] = dn;
    } else {      // TA_TRIAL
      const double xn = F.W.x[j] + sj;
      T.xt[j] = xn;
      if (jl >= 0) F.xl[jl] = xn;
    }
  }
}

void fe_tron_enqueue_step(const FeDev& F, const SolveParams& o, int32_t* status_dev, hipStream_t s) {
  const int nvb = grid_for(F.P, FE_THREADS, FE_DOT_BLOCKS);
  hipLaunchKernelGGL(fe_tron_products_kernel, dim3(nvb), dim3(FE_THREADS), 0, s, F, o);
  hipLaunchKernelGGL(fe_tron_decide_kernel, dim3(1), dim3(FE_THREADS), 0, s, F, o, nvb, status_dev);
  hipLaunchKernelGGL(fe_tron_update_kernel, dim3(grid_for(F.P, 256, 1024)), dim3(256), 0, s, F);
}

// ---- restart, and the two mode changes of gdmix_fe_hessian_vec -------------------------------------------------------------------------
__global__ void fe_tron_reset_kernel(FeDev F, const double* __restrict__ theta0) {
  const FeTron T = fe_tron_of(F);
  for (int j = blockIdx.x * blockDim.x + threadIdx.x; j < F.P; j += gridDim.x * blockDim.x) {
    T.s[j] = 0.0; T.r[j] = 0.0; T.d[j] = 0.0; T.h[j] = 0.0; T.g[j] = 0.0;
    T.xt[j] = theta0 ? theta0[j] : 0.0;      // (fe_init_kernel has put the same point into W.x and xl)
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    FeTronState R{};      // mode FE_TM_EVAL: an evaluation at the start point comes first
    *T.st = R;
  }
}

__global__ void fe_tron_hv_mode_kernel(FeDev F, int begin) {
  FeTronState* st = fe_tron_state(F);
  if (begin) { st->saved_mode = st->mode; st->mode = FE_TM_CURVATURE; }
  else st->mode = st->saved_mode;
}

// vl from a vector in the global coefficient space, the way fe_prepare_kernel fills xl; v NULL: from the CG direction (put back)
__global__ void fe_tron_fill_vl_kernel(FeDev F, const double* __restrict__ v) {
  const FeTron T = fe_tron_of(F);
  const double* __restrict__ src = v ? v : T.d;
  for (int jl = blockIdx.x * blockDim.x + threadIdx.x; jl < F.d; jl += gridDim.x * blockDim.x) T.vl[jl] = src[F.umap[jl]];
  if (v && blockIdx.x == 0 && threadIdx.x == 0) {
    T.st->vb = F.ic ? v[F.D] : 0.0;
    T.st->mode = FE_TM_VECTOR;
  }
}

void fe_tron_enqueue_reset(const FeDev& F, const double* theta0, hipStream_t s) {
  hipLaunchKernelGGL(fe_tron_reset_kernel, dim3(grid_for(F.P, 256, 1024)), dim3(256), 0, s, F, theta0);
}
void fe_tron_enqueue_hv_begin(const FeDev& F, hipStream_t s) { hipLaunchKernelGGL(fe_tron_hv_mode_kernel, dim3(1), dim3(1), 0, s, F, 1); }
void fe_tron_enqueue_hv_vector(const FeDev& F, const double* v, hipStream_t s) {
  hipLaunchKernelGGL(fe_tron_fill_vl_kernel, dim3(grid_for(F.d, 256, 2048)), dim3(256), 0, s, F, v);
}
void fe_tron_enqueue_hv_end(const FeDev& F, hipStream_t s) {
  hipLaunchKernelGGL(fe_tron_hv_mode_kernel, dim3(1), dim3(1), 0, s, F, 0);
  hipLaunchKernelGGL(fe_tron_fill_vl_kernel, dim3(grid_for(F.d, 256, 2048)), dim3(256), 0, s, F, static_cast<const double*>(nullptr));
}

}  // namespace gdmix
