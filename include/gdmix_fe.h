/* gdmix_fe.h — C ABI of the fixed-effect trainer in libgdmix_re.so.
 *
 * Replaces the body of FixedEffectLRModelLBFGS's training step
 *   _train_model_fn / _compute_loss_and_gradients / fmin_l_bfgs_b call
 *   gdmix-trainer/src/gdmix/models/custom/fixed_effect_lr_lbfgs_model.py:309-392, 394-430, 635-643
 * for one worker's shard resident in HBM:
 *
 *   f(theta) = sum_i w_i loss(y_i, x_i.w + b + offset_i) + (l2/2) |theta_reg|^2     theta = [w (num_features), b]
 *
 * (intercept LAST, :340-342; not divided by n; theta_reg excludes b unless regularize_bias, :367-369). The
 * reference evaluates value and gradient with TensorFlow on every worker, all-reduces both across workers
 * (two collectives, keys 0/1, each worker adding l2 |theta|^2 / (2 R), :375-381) and hands them to scipy's
 * fmin_l_bfgs_b, which runs replicated on every worker. Here one evaluation is
 *
 *   gdmix_fe_eval    local part of [gradient (num_features + 1), value] into one device buffer
 *   <caller>         ONE all-reduce (sum) of that buffer across workers (RCCL through torch.distributed);
 *                    nothing to do for a single worker
 *   gdmix_fe_step    adds the regulariser once, advances L-BFGS (replicated: every worker computes the same
 *                    step from the same reduced buffer), returns the solver status (-1 = evaluate again)
 *
 * so the host loop is `do { eval; all_reduce; } while (step() < 0)`. All arithmetic fp64 on fp32 data. The shard is
 * a one-entity batch packed by gdmix_re_pack (CSR + CSC copy, local feature ids + unique_global map); the
 * L-BFGS vectors live in the global coefficient space, which is common to all workers.
 *
 * Same conventions as gdmix_re.h: 0 / negative return codes, gdmix_re_last_error(), no exceptions, caller-owned
 * input buffers (which must stay alive until gdmix_fe_destroy), one context per device, calls serialised.
 */
#ifndef GDMIX_FE_H
#define GDMIX_FE_H

#include "gdmix_re.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct gdmix_fe_problem gdmix_fe_problem;

/* shard: a packed batch with E == 1 (gdmix_re_pack; has_intercept of the pack must equal opts->has_intercept).
 * num_features: size of the global feature space D; coefficients are [D + has_intercept], intercept last.
 * opts: l2, regularize_bias, has_intercept, m (<= 10), max_iter, maxfun, maxls, ftol, pgtol, loss are used.
 * theta0: device pointer [D + has_intercept] or NULL (zeros).
 * ---- poisson (ABI 19) ---- opts->loss is the loss code of include/gdmix_re.h (GDMIX_RE_LOSS_*; any other value is refused, also by
 * gdmix_fe_restart, whose code must be the creation's). GDMIX_RE_LOSS_POISSON: the objective of gdmix_re.h's section "poisson" summed, not
 * divided by n: f = sum_i w_i (exp(z_i) - y_i z_i) + (l2/2) |theta_reg|^2, g = X~' (w (exp(z) - y)) + l2 theta_reg, labels y >= 0
 * real-valued; gdmix_fe_hessian_diag leaves sum_i X~_ij^2 w_i exp(z_i). The value is added up error-free as for the other losses, exp
 * is the library's own (<= 0.98 ulp) and IEEE at the ends; gdmix_fe_score is unchanged (the margin z, never exp(z)).
 * The problem builds its own two copies of the non-zeros (8 B per non-zero each, 10 B when a unit of a pass spans more than 2^21
 * elements; temporary: 40 B per non-zero) and keeps reading the shard's y / offset / weight / unique_global, which must outlive it.
 * Synchronises the stream. Test hooks (environment; read when a problem is created and at no other time — a problem keeps what it
 * was created under, whatever the environment holds when it is restarted or solved): GDMIX_FE_CHUNK = entries per unit of a pass,
 * GDMIX_FE_PACK=0 = the three-array form of the entries, GDMIX_FE_COMPRESS = which passes may read units in the 6-byte form (bit 0
 * rows, bit 1 columns; default 2); GDMIX_FE_WINDOW_BITS, GDMIX_FE_HOT_MIN and GDMIX_FE_FUSED_TAIL likewise. */
GDMIX_API int gdmix_fe_create(gdmix_re_ctx* ctx, const gdmix_re_packed* shard, int64_t num_features,
                              const gdmix_re_opts* opts, const double* theta0, gdmix_fe_problem** out, void* stream);
GDMIX_API void gdmix_fe_destroy(gdmix_fe_problem* p);

/* Local [gradient of the data term (D + has_intercept), value of the data term] at the current trial point. */
GDMIX_API int gdmix_fe_eval(gdmix_fe_problem* p, void* stream);

/* The buffer gdmix_fe_eval fills and gdmix_fe_step consumes: *count = D + has_intercept + 1 doubles. */
GDMIX_API double* gdmix_fe_reduce_buffer(gdmix_fe_problem* p, int64_t* count);

/* Diagonal of the data term's Hessian X~' D X~ of the shard at theta (device pointer [D + has_intercept], intercept last;
 * NULL = the current point), D_i = w_i rho_i (1 - rho_i), rho = sigmoid(x_i . w + b + offset_i) — what
 * fixed_effect_lr_lbfgs_model.py:271-296 accumulates batch by batch for fixed_effect_variance_mode = SIMPLE. Written to the
 * reduce buffer in place of the gradient (entries [0, D + has_intercept); the last entry is unused): the same all-reduce as
 * an evaluation makes it the whole data set's, and variance_j = 1 / (H_j + l2 [j regularised] + 1e-12) (:451-456). The
 * reference does this arithmetic in float32, this library in float64. Two more streaming passes over the shard. */
GDMIX_API int gdmix_fe_hessian_diag(gdmix_fe_problem* p, const double* theta, void* stream);

/* fixed_effect_variance_mode = FULL with several workers, on the device (round 4). The reference sums the workers' dense Hessians
 * and inverts the sum (fixed_effect_lr_lbfgs_model.py:291-305, 384-389, 457-463). Stage 1, per worker: the curvature part X~' D X~ of
 * the shard — `shard` is the one-entity packed batch gdmix_fe_create took — at theta_local ([d + has_intercept], the shard's LOCAL
 * order: intercept first, then its features in ascending global index, packed->unique_global) as a dense symmetric matrix H
 * [ld x ld] row-major, ld = d + has_intercept rounded up to a multiple of 64, no regulariser, zero on the padding. The caller
 * scatters H into the common (global) index space and all-reduces it (RCCL through torch.distributed). Stage 2: variance [p] =
 * diag((H + (l2 + 1e-12) I - l2 e_u e_u' [u = unregularised_index, -1: none])^-1) of the summed matrix H [ld x ld] (overwritten),
 * work = another ld x ld doubles. Tiled Cholesky + inverse on the whole device (csrc/re_variance_big.hip), p <= 16 384. */
GDMIX_API size_t gdmix_fe_hessian_dense_scratch_bytes(const gdmix_re_packed* shard);
GDMIX_API int gdmix_fe_hessian_dense(gdmix_re_ctx* ctx, const gdmix_re_packed* shard, int has_intercept, const double* theta_local,
                                     double* H, int64_t ld, void* scratch, size_t scratch_bytes, void* stream);
/* (ABI 19) The same with the curvature weight of a loss code (GDMIX_RE_LOSS_*, include/gdmix_re.h): D_i = w_i rho_i (1 - rho_i) for the
 * logistic loss (what gdmix_fe_hessian_dense computes, whatever the problem's loss), 2 w_i for the squared, w_i exp(z_i) for the Poisson loss. */
GDMIX_API int gdmix_fe_hessian_dense_loss(gdmix_re_ctx* ctx, const gdmix_re_packed* shard, int has_intercept, int loss, const double* theta_local,
                                          double* H, int64_t ld, void* scratch, size_t scratch_bytes, void* stream);
GDMIX_API int gdmix_fe_variance_of_hessian(gdmix_re_ctx* ctx, double* H, int64_t p, int64_t ld, double l2, int64_t unregularised_index,
                                           double* work, double* variance, void* stream);

/* Consumes the (all-reduced) buffer. *status: -1 = evaluate again, else GDMIX_RE_ST_*. Synchronises the stream. */
GDMIX_API int gdmix_fe_step(gdmix_fe_problem* p, void* stream, int32_t* status);

/* The same, stream-ordered (round 5): the step is enqueued, nothing is waited for; *seq (may be NULL) = the number of this step,
 * counted from 0 over the life of the problem. gdmix_fe_step_status(p, seq, &status) waits for THAT step only and returns its
 * status (the last 8 enqueued steps can be asked for). Once the driver has stopped, every later gdmix_fe_eval / step on the
 * problem is a no-op on the device (the kernels return on the stop flag) and reports the status of the stop, so a host loop may
 * run `lookahead` evaluations ahead of the status it has read and the device never idles between evaluations:
 *     for k = 0, 1, ...: eval; all_reduce; step_async -> k; if (k >= lookahead and step_status(k - lookahead) >= 0) break;
 * With several workers every worker takes the same decisions from the same reduced buffer, so all of them enqueue the same
 * number of all-reduces. gdmix_fe_solve is that loop for ONE worker (no all-reduce), inside the library: *status = the status
 * of the stop (-1: max_evals evaluations without one), *evals (may be NULL) = evaluations enqueued, no-ops included. */
GDMIX_API int gdmix_fe_step_async(gdmix_fe_problem* p, void* stream, int64_t* seq);
GDMIX_API int gdmix_fe_step_status(gdmix_fe_problem* p, int64_t seq, int32_t* status);
GDMIX_API int gdmix_fe_solve(gdmix_fe_problem* p, void* stream, int32_t lookahead, int64_t max_evals, int32_t* status, int64_t* evals);

/* Result after status >= 0: theta [D + has_intercept] (device pointer, may be NULL) and scalars (host, may be NULL). */
GDMIX_API int gdmix_fe_result(gdmix_fe_problem* p, double* theta, double* fval, double* gnorm, int32_t* nit,
                              int32_t* nfev, void* stream);

/* Scores of a raw shard under a global coefficient vector: replaces _predict / the scoring after training
 *   gdmix-trainer/src/gdmix/models/custom/fixed_effect_lr_lbfgs_model.py:214-306,406-440
 * score_i = x_i . w + b + offset_i, per_coord_i = score_i - offset_i, stored as float (the reference's Avro `float`). All
 * pointers are device pointers: row_nnz_ptr [n+1] / col_global / val are the sample-major arrays of the reader (NULL,
 * NULL, NULL for a model without a feature bag), offset [n] or NULL, theta [num_features + has_intercept] with the
 * intercept last. No pack is needed: the pass reads the shard once. Feature indices must lie in [0, num_features). */
GDMIX_API int gdmix_fe_score(gdmix_re_ctx* ctx, int64_t n, const int64_t* row_nnz_ptr, const int64_t* col_global, const float* val,
                             const float* offset, const double* theta, int64_t num_features, int has_intercept, float* score,
                             float* per_coord, void* stream);

/* ---- a sweep over l2 inside one stage (ABI 15; gdmix_amd/fe_model.py: --l2_reg_weights) ----
 *
 * gdmix_fe_restart puts an existing problem back into exactly the state gdmix_fe_create leaves it in, for new l2, regularize_bias,
 * max_iter, maxfun, maxls, ftol, pgtol and a new start point (theta0: device pointer [D + has_intercept] or NULL = zeros; read by a
 * kernel on the stream, so it must stay alive until the stream has passed this call). Cleared and re-armed: the L-BFGS state, history,
 * plan and vectors, the shard-local copy of x, the reduce buffer (and the library's note that it is dirty), every partial sum, the
 * finishing counters, the sync words of the one-launch step, the status ring and the counts of steps / evaluations / launches, and with
 * the state the stop flag — which made every kernel of the stopped problem a no-op: a restart may come right behind a gdmix_fe_solve
 * that left `lookahead` no-op evaluations queued after the stop. Kept as they are: both copies of the non-zeros, their unit tables, the
 * frequent-column tables and the list of row blocks with several units — everything gdmix_fe_create sorted, split and synchronised for.
 * opts->has_intercept, opts->loss and opts->m must equal the creation's (the pool is sized and the copies are read by them):
 * GDMIX_RE_EINVAL otherwise. Stream-ordered, no synchronisation. The definition of the call: a solve after a restart gives the same
 * bits as gdmix_fe_create with those options and that start point followed by the same solve. */
GDMIX_API int gdmix_fe_restart(gdmix_fe_problem* p, const gdmix_re_opts* opts, const double* theta0, void* stream);

/* ---- (ABI 17) incremental training: the L2 term centred on a prior model and weighted by its precisions ---------------------------
 * The fixed-effect half of gdmix_re.h's section of the same name (--incremental_training True, gdmix_amd/fe_model.py; the reference
 * leaves it open: fixed_effect_lr_lbfgs_model.py:361-367). A warm start alone forgets the prior model once it converges: with l2 > 0 the
 * optimum does not depend on the start point.
 *
 * Definition. theta = [w (D), b], intercept last; coefficient j has a prior mean mu_j and a prior variance v_j, s_j = sqrt(v_j); R = the
 * regularised coefficients: every j < D, and the intercept iff regularize_bias:
 *     F(theta) = sum_i w_i l(y_i, x_i . w + b + offset_i) + (l2/2) sum_{j in R} (theta_j - mu_j)^2 / v_j
 * not divided by n (the fixed effect's convention), l the logistic or the squared loss (opts->loss) as without a prior.
 * The prior is global. It applies to every coefficient of the model, whether or not this worker's shard holds a non-zero in that
 * column: a coefficient no worker has data for stays at its prior mean, exactly.
 * Defaults (the caller's, gdmix_amd/fe_model.py; those of the random effect). mu_j = 0 where the prior file has no mean for j — a
 * coefficient thresholded out of the file counts as missing —, v_j = 1 where the variance is missing, not finite or <= 0. A prior file
 * without variances gives (l2/2) |theta_R - mu_R|^2.
 * The intercept. Unlike the random effect's kernels, nothing here pins the intercept column: a regularised intercept's prior variance is
 * honoured like any other. An unregularised intercept has no penalty: the caller passes s_D = 1, and mu_D is only where it starts.
 * Substitution. The optimiser works in phi_j = (theta_j - mu_j) / s_j, from phi = 0:
 *     penalty (l2/2) |phi_R|^2,   grad_phi = s (.) grad_theta,   theta_j = mu_j + s_j phi_j
 * The shard is NOT transformed (as csrc/re_prior.hip does for the random effect: a rounding per non-zero and a second copy of the
 * values). The problem already keeps the trial point in two places — the global x and the shard-local copy the row pass gathers from
 * — and consumes the reduced data gradient coefficient by coefficient, so the change of variables costs work per coefficient, none per
 * non-zero, and rounds no data:
 *     x holds phi; wherever the shard-local copy of coefficient j is written it gets mu_j + s_j phi_j (one fma);
 *     the row pass's intercept is mu_D + s_D phi_D;
 *     the step scales the reduced data gradient, fg[j] * s_j (rounded on its own), before it adds the regulariser l2 phi_j. The
 *       all-reduce between evaluation and step is untouched and carries the theta-space data gradient: every worker scales after the
 *       reduce and computes the same step;
 *     gdmix_fe_result returns theta = mu + s (.) phi.
 * Each is a compile-time variant of its kernel; a problem without a prior runs the instantiations without, instruction for instruction
 * what it ran before. mu = 0, s = 1 makes every added operation exact: the bits of a problem without a prior.
 * Consequences.
 *   stop tests  pgtol, ftol and every other stop test of L-BFGS-B apply in phi-space: |s (.) grad_theta F|_inf <= pgtol; gdmix_fe_result's
 *               gnorm is |grad_phi|_inf. fval is F; nit, nfev and status are those of the solve in phi.
 *   threshold   the sparsity threshold (the caller's) applies to theta, not to phi.
 *   variances   gdmix_fe_hessian_diag takes theta (NULL: the current point, mapped) and returns theta-space curvature, as before. The
 *               caller maps: Var(theta_j) = s_j^2 Var'(phi_j), Var' the stage's variance mode applied to H' = S H S —
 *               SIMPLE  s_j^2 / (s_j^2 H_jj + l2 [j in R] + 1e-12),
 *               FULL    s_j^2 diag((S H S + (l2 + 1e-12) I - l2 e_u e_u')^-1)_j, u an unregularised intercept.
 *
 * gdmix_fe_set_prior: mean / scale device pointers [D + has_intercept], intercept last; `scale` arrives computed (the host takes the
 *   square root: caller and device use the same bits). Both are copied into the problem: the caller may free them once the stream has
 *   passed the call. NULL, NULL removes the prior. Either way the call leaves the problem in the state of a gdmix_fe_restart with its
 *   current options at phi = 0 (theta = mu; without a prior: zeros). Stream-ordered. Every scale must be finite and > 0: a kernel checks
 *   the caller's array and the host reads its verdict back — the one place the call waits — before anything of the problem is touched;
 *   GDMIX_RE_EINVAL otherwise, the problem as it was.
 *   While a prior is installed gdmix_fe_restart's theta0 is in theta units: NULL means mu, otherwise phi0 = (theta0 - mu) / s. */
GDMIX_API int gdmix_fe_set_prior(gdmix_fe_problem* p, const double* mean, const double* scale, void* stream);

/* ---- (ABI 18) feature normalisation ---------------------------------------------------------------------------------------------------
 * The fixed-effect half of gdmix_re.h's section of the same name (--feature_normalization, gdmix_amd/fe_model.py): the statistics, their
 * definitions, bounds and kernels are stated there (gdmix_re_feature_extent / gdmix_re_feature_moments take the reader arrays gdmix_fe_score
 * takes). Here the data are the training samples of ALL workers: count_j and N are all-reduced with SUM and the bit patterns of max |x| with
 * MAX after pass 1, every worker derives the same shifts, and the four limb sums per feature are all-reduced with SUM after pass 2 — int64
 * tensors, exact on any backend — so every worker derives the same factors s_j from the same integers. A worker whose shard is empty still
 * takes part in the collectives.
 * Objective. F of the incremental section with mu = 0 and v_j = s_j^2: the penalty is (l2/2) sum_{j in R} (theta_j / s_j)^2. s_D = 1 for the
 * intercept, regularised or not: this feature's own choice. The caller installs it with gdmix_fe_set_prior(mean = 0, scale = [s, 1]) after
 * gdmix_fe_create; a warm start follows as gdmix_fe_restart(theta0), which takes theta units while a prior is installed. Everything the
 * incremental section states for a prior holds: the stop tests apply in phi = theta / s, the threshold to theta, Var(theta_j) = s_j^2 Var'(phi_j).
 * No entry point is added to this header. */

/* ---- (ABI 21) down-sampling ---------------------------------------------------------------------------------------------------------------
 * --down_sampling_rate / --down_sampling_seed (gdmix_amd/fe_model.py; Photon-ML's downSamplingRate): the stage's training shard is
 * down-sampled in HBM before it is packed, by gdmix_re.h's section "down-sampling", which holds the definition (the hash of (seed, uid), the
 * threshold, the weight 1 / rate of a kept row, every positive kept under the logistic loss). The problem of this header is then created on
 * the packed sample as on any shard: no kernel of this header knows of it, and the variances are those of the sampled, re-weighted
 * objective. Each worker samples its own shard with the same seed; the union of the kept rows does not depend on the number of workers. A
 * worker whose sample has no row or no non-zero trains on the weight-0 sample of an empty shard. Scoring, metrics, feature statistics and
 * validation data see every row. The random-effect stage has no such flag (an entity could lose all its rows; a follow-up). No entry point
 * is added to this header. */

/* ---- (ABI 23) L1 / elastic net ------------------------------------------------------------------------------------------------------------
 * --l1_reg_weight (gdmix_amd/fe_model.py; Photon-ML's regularizationType = L1 / ELASTIC_NET, solved there by OWL-QN as well):
 *     F(theta) = sum_i w_i l(y_i, x_i . w + b + offset_i) + (l2/2) |theta_R|^2 + l1 |theta_R|_1
 * R the regularised set of the options (every feature; the intercept iff regularize_bias), l any of the three losses, the sum not divided by
 * n. Photon-ML's elastic net (lambda, alpha) is l1 = alpha lambda, l2 = (1 - alpha) lambda.
 * gdmix_fe_set_l1: l1 must be finite and >= 0 (GDMIX_RE_EINVAL otherwise). l1 > 0 makes the problem take the OWL-QN step (csrc/fe_qn.hip)
 *   from its next step on; l1 == 0 puts it back on the L-BFGS-B step. Either way the call leaves the problem in the state of a
 *   gdmix_fe_restart with its current options at zeros. Stream-ordered; it waits for nothing. gdmix_fe_restart keeps the problem's l1; its
 *   theta0 is the OWL-QN start point. While a prior is installed the call is refused (GDMIX_RE_EINVAL), and so is gdmix_fe_set_prior with a
 *   prior while l1 > 0: the L1 term is not invariant under the diagonal substitution phi = (theta - mu) / s.
 * Every other entry point keeps its contract: gdmix_fe_eval is the same two passes, gdmix_fe_step / _step_async / _step_status / _solve, the
 * status ring, the lookahead and the stop flag work as before, the step leaves the reduce buffer cleared, and the -inf mark of an aborted
 * peer in the value slot stops every worker with GDMIX_RE_ST_ABORTED_PEER.
 * The step (Andrew & Gao 2007). g is the gradient of the smooth part (data + l2 theta_R) at the accepted point x.
 *   pseudo-gradient  j in R: pg_j = g_j + l1 (x_j > 0), g_j - l1 (x_j < 0); at x_j = 0: g_j + l1 if that is < 0, g_j - l1 if that is > 0, else 0.
 *                    j not in R: pg_j = g_j.
 *   direction        d = -H pg, H the L-BFGS inverse-Hessian approximation over the last <= m stored pairs s = x+ - x, y = g+ - g (smooth
 *                    gradients), H0 = (s'y / y'y) I from the newest pair; then d_j = 0 wherever d_j pg_j >= 0. No pair stored: d = -pg.
 *   orthant          xi_j = sign(x_j) if x_j != 0, else sign(-pg_j).
 *   trial            x(t)_j = x_j + t d_j if its sign equals xi_j, else exactly 0.0.
 *   search           t = 1 / |pg|_2 while no pair is stored, else 1; accepted when F(x(t)) <= F(x) + 1e-4 pg'(x(t) - x), else t is halved.
 *                    After maxls rejected trials in one iteration: the memory is cleared and the search starts again along -pg if a pair
 *                    was stored, else the solve stops with status 4 at x.
 *   pair storage     only if s'y > 2.2e-16 y'y.
 *   stops            after each accepted iterate, in this order: |pg|_inf <= pgtol -> 0 (also tested at the start point);
 *                    F_old - F <= ftol max(|F_old|, |F|, 1) -> 1; nit >= max_iter -> 2; nfev > maxfun -> 3. Every evaluation counts in nfev.
 * gdmix_fe_result returns the last accepted point, never a rejected trial: coordinates the orthant projection set to zero are exactly 0.0.
 * fval = F with the L1 term, gnorm = |pg|_inf, nit, nfev as above.
 * Variances are those of the smooth part at the returned theta: gdmix_fe_hessian_diag plus l2, as without an L1 term. A coefficient at
 * exactly 0 gets one too: this feature's own choice (the L1 term has no curvature; the variance says how well the data determine the
 * coefficient, not whether it was selected). */
GDMIX_API int gdmix_fe_set_l1(gdmix_fe_problem* p, double l1, void* stream);

/* ---- (ABI 24) TRON: trust-region Newton ------------------------------------------------------------------------------------------------------
 * --optimizer=TRON (gdmix_amd/fe_model.py; Photon-ML's OptimizerType = TRON; Lin, Weng & Keerthi 2008, LIBLINEAR's tron) minimises the smooth
 *     F(theta) = sum_i w_i l(y_i, x_i . w + b + offset_i) + (l2/2) |theta_R|^2
 * of any of the three losses by Newton steps inside a trust region, each found by conjugate gradients on Hessian-vector products
 *     H v = X~' D X~ v + l2 v_R,   D_i = w_i rho_i (1 - rho_i) | 2 w_i | w_i exp(z_i)   (logistic | squared | Poisson).
 * A product is the same two streaming passes as an evaluation: the row pass gathers v instead of theta and a finished row leaves
 * D_i (x_i . v + v_b) instead of the residual; the column pass is the evaluation's. It needs no exp and no log: D_i is written by the
 * evaluation of the point it belongs to. An evaluation runs at a trial point, so there are two arrays of weights and a word that says which
 * is the accepted point's; the step flips it on acceptance, and a rejected trial leaves the accepted point's weights in force.
 * gdmix_fe_set_optimizer: GDMIX_FE_OPT_LBFGS (the default of gdmix_fe_create) or GDMIX_FE_OPT_TRON; stream-ordered; leaves the problem in the
 *   state of a gdmix_fe_restart with its current options at zeros, like gdmix_fe_set_l1. gdmix_fe_restart keeps the optimiser; its theta0 is
 *   the start point. The first selection of TRON allocates a buffer of the problem's own (6 P + d + 2 n doubles); the pool does not change.
 *   Refused with GDMIX_RE_EINVAL: TRON while l1 > 0, and gdmix_fe_set_l1 > 0 on a TRON problem (the objective must be smooth); TRON while a
 *   prior is installed, and gdmix_fe_set_prior with a prior on a TRON problem. The substitution phi = (theta - mu) / s for TRON is a
 *   follow-up, per-coefficient work only: gather s_j d_j and scale the reduced product by s_j. A refused call leaves the problem as it was.
 * What a pass pair of a TRON problem computes — an evaluation at the trial point or a product with the CG direction — is decided on the
 * device: the step writes a mode word, the row kernels read it at entry. gdmix_fe_eval therefore launches the same kernels every time, the
 * loop "eval; all-reduce; step" with its lookahead, status ring and stop flag is the one of the other steps, the step leaves the reduce
 * buffer cleared, and -inf in the value slot stops every worker with GDMIX_RE_ST_ABORTED_PEER. After a product the buffer holds
 * [X~' D X~ d, 0]; l2 d_R is added once, in the step, behind the reduce.
 * The step. g, f: gradient and value of F (with the l2 term) at the accepted point x; norms are 2-norms unless marked.
 *   start     evaluate at x0 (nfev = 1). |g|_inf <= pgtol -> status 0 with nit = 0. Delta = |g|.
 *   CG        (Steihaug) s = 0, r = -g, d = r. Per product: Hd; alpha = r'r / d'Hd. If d'Hd <= 0 or |s + alpha d| > Delta (taken as
 *             s's + 2 alpha s'd + alpha^2 d'd > Delta^2): go to the boundary with the non-negative root tau of |s + tau d| = Delta,
 *             rad = sqrt((s'd)^2 + d'd (Delta^2 - s's)), tau = (Delta^2 - s's) / (s'd + rad) if s'd >= 0, else (rad - s'd) / d'd;
 *             s += tau d, r -= tau Hd, and CG ends. Else s += alpha d, r -= alpha Hd with r'r_new taken as
 *             max(0, r'r - 2 alpha r'Hd + alpha^2 Hd'Hd); CG ends if |r_new| <= 0.1 |g| or after GDMIX_FE_TRON_MAX_CG products in this outer
 *             iteration (this feature's own cap); else d = r + (r'r_new / r'r) d.
 *   trial     prered = -(g's - s'r) / 2. Evaluate at x + s; actred = f - f_new. On every trial before the first accepted step
 *             Delta = min(Delta, |s|). ah = 4 if f_new - f - g's <= 0, else max(0.25, -(g's / (f_new - f - g's)) / 2).
 *   radius    actred < 1e-4 prered (or not a number): Delta = min(max(ah, 0.25) |s|, Delta / 2); else if actred < prered / 4:
 *             Delta = max(Delta / 4, min(ah |s|, Delta / 2)); else if actred < 3 prered / 4: Delta = max(Delta / 4, min(ah |s|, 4 Delta));
 *             else Delta = max(Delta, min(ah |s|, 4 Delta)).
 *   accept    iff actred > 1e-4 prered: x, f, g move, the curvature word flips, nit += 1. A rejected trial starts CG again from the same
 *             x, g with the new Delta.
 *   stops     after an accepted step, in this order: |g|_inf <= pgtol -> 0; f_old - f <= ftol max(|f_old|, |f|, 1) -> 1; nit >= max_iter -> 2;
 *             nfev > maxfun -> 3. After a rejected trial: nfev > maxfun -> 3; maxls consecutive rejections -> 4, at the accepted point.
 * nfev counts evaluations only; products are counted apart (gdmix_fe_products). gdmix_fe_result returns the last accepted point, fval = F,
 * gnorm = |g|_inf, nit, nfev. gdmix_fe_last_eval_ms: on a TRON problem the timed second pass pair is the first product.
 * gdmix_fe_hessian_vec, the sibling of gdmix_fe_hessian_diag: leaves the data term's X~' D X~ v of the shard at theta (device pointers
 *   [D + has_intercept], intercept last; theta NULL: the current accepted point) in the reduce buffer — the intercept's entry last of the
 *   coefficients, the value slot 0, no regulariser; the same all-reduce as an evaluation makes it the whole data set's. On any problem,
 *   TRON or not (it allocates the buffer if need be and computes the weights at theta itself: two row passes, one column pass), between a
 *   step and the next gdmix_fe_eval; it puts the solver's point and mode back, so that a solve gives the bits it gives without the call. */
#define GDMIX_FE_OPT_LBFGS 0
#define GDMIX_FE_OPT_TRON 1
#define GDMIX_FE_TRON_MAX_CG 50
GDMIX_API int gdmix_fe_set_optimizer(gdmix_fe_problem* p, int optimizer, void* stream);
GDMIX_API int gdmix_fe_products(gdmix_fe_problem* p, int64_t* nhv, void* stream);
GDMIX_API int gdmix_fe_hessian_vec(gdmix_fe_problem* p, const double* theta, const double* v, void* stream);

/* ---- (ABI 26) box constraints: projected L-BFGS ----------------------------------------------------------------------------------------------
 * --coefficient_constraints (gdmix_amd/fe_model.py; Photon-ML's coefficient box constraints) minimises the smooth
 *     F(theta) = sum_i w_i l(y_i, x_i . w + b + offset_i) + (l2/2) |theta_R|^2     subject to  lo_j <= theta_j <= hi_j
 * of any of the three losses. lo_j may be -inf, hi_j may be +inf, lo_j == hi_j pins a coefficient; the intercept is never bounded.
 * gdmix_fe_set_bounds: lower, upper are device pointers to [D + has_intercept] doubles, intercept last (copied by the library: 2 P doubles of
 *   the problem's own, allocated at the first selection; the pool does not change). Bounds make the problem take the projected L-BFGS step
 *   (csrc/fe_qn.hip) from its next step on; both NULL puts it back on the L-BFGS-B step. Either way the call leaves the problem in the state
 *   of a gdmix_fe_restart with its current options at the clamped zeros. Stream-ordered but for one wait, on the check of the caller's arrays.
 *   gdmix_fe_restart keeps the bounds; its theta0 (NULL: zeros) is clamped into the box and that is the start point.
 *   Refused with GDMIX_RE_EINVAL, the problem left as it was: a NaN bound; lo_j > hi_j; a bound on the intercept other than -inf / +inf;
 *   bounds while l1 > 0, on a TRON problem, or while a prior is installed — and the mirror calls gdmix_fe_set_l1 > 0,
 *   gdmix_fe_set_optimizer(TRON) and gdmix_fe_set_prior with a prior on a problem that has bounds. (Bounds under the substitution
 *   phi = (theta - mu) / s are per-coefficient work, (lo - mu) / s and (hi - mu) / s: a follow-up.)
 * Every other entry point keeps its contract: gdmix_fe_eval is the same two passes, gdmix_fe_step / _step_async / _step_status / _solve, the
 * status ring, the lookahead and the stop flag work as before, the step leaves the reduce buffer cleared, and the -inf mark of an aborted
 * peer in the value slot stops every worker with GDMIX_RE_ST_ABORTED_PEER.
 * The step. g is the gradient of F (with the l2 term) at the accepted point x; clamp(v)_j = min(max(v_j, lo_j), hi_j), exactly the bound's
 * double where it clamps.
 *   binding set      B = { j : (x_j <= lo_j and g_j > 0) or (x_j >= hi_j and g_j < 0) or lo_j == hi_j }. Reduced gradient: q_j = 0 on B, g_j off B.
 *   direction        d = -H q, H the L-BFGS inverse-Hessian approximation over the last <= m stored pairs s = x+ - x, y = g+ - g,
 *                    H0 = (s'y / y'y) I from the newest pair; then d_j = 0 on B, and wherever x_j <= lo_j and d_j < 0 or x_j >= hi_j and
 *                    d_j > 0. No pair stored: d = -q.
 *   trial            x(t) = clamp(x + t d).
 *   search           t = 1 / |q|_2 while no pair is stored, else 1; accepted when F(x(t)) <= F(x) + 1e-4 g'(x(t) - x), else t is halved.
 *                    After maxls rejected trials in one iteration: the memory is cleared and the search starts again along -q if a pair
 *                    was stored, else the solve stops with status 4 at x.
 *   pair storage     only if s'y > 2.2e-16 y'y.
 *   stops            after each accepted iterate, in this order: max_j |x_j - clamp(x - g)_j| <= pgtol -> 0 (scipy's projected gradient; also
 *                    tested at the start point); F_old - F <= ftol max(|F_old|, |F|, 1) -> 1; nit >= max_iter -> 2; nfev > maxfun -> 3. Every
 *                    evaluation counts in nfev.
 *   start point      clamp(theta0); zeros are clamped too.
 * gdmix_fe_result returns the last accepted point, never a rejected trial: lo <= theta <= hi holds exactly and a coefficient at a bound is
 * the bound's double. fval = F, gnorm = the projected-gradient norm above, nit, nfev as above.
 * gdmix_fe_hessian_diag and the FULL variance path are unchanged. Variances are those of the smooth objective at the returned theta,
 * gdmix_fe_hessian_diag plus l2, as without bounds. A coefficient at a bound gets one too: this feature's own choice (the variance says how
 * well the data determine the coefficient, not whether a constraint holds it). */
GDMIX_API int gdmix_fe_set_bounds(gdmix_fe_problem* p, const double* lower, const double* upper, void* stream);

/* gdmix_fe_score under K coefficient vectors in ONE pass over the shard's non-zeros (csrc/fe_sweep.hip). thetas: HOST array of K device
 * pointers, each [num_features + has_intercept] with the intercept last; score / per_coord: [K][n] float, row k for thetas[k]
 * (per_coord may be NULL). Defined by equivalence: row k is bit for bit what gdmix_fe_score writes for thetas[k] — a row's products
 * are added in the row's order, each step one fused multiply-add into one fp64 accumulator that starts at the intercept. (col, val) of a
 * non-zero are loaded once and feed up to GDMIX_RE_SWEEP_MODELS_PER_PASS accumulators: 12 B per non-zero per pass instead of per model; a
 * longer list takes several passes. workspace (device, gdmix_fe_score_models_workspace_bytes(num_features, K) bytes; may be NULL): each
 * pass first copies its coefficient vectors into one slot-major array [num_features + 1][models of the pass], so that a non-zero's
 * coefficients are one contiguous read; without it they are read from the K arrays. Same arguments otherwise as gdmix_fe_score; n = 0 is
 * legal and does nothing. */
GDMIX_API size_t gdmix_fe_score_models_workspace_bytes(int64_t num_features, int K);
GDMIX_API int gdmix_fe_score_models(gdmix_re_ctx* ctx, int64_t n, const int64_t* row_nnz_ptr, const int64_t* col_global, const float* val,
                                    const float* offset, const double* const* thetas, int K, int64_t num_features, int has_intercept,
                                    float* score, float* per_coord, void* workspace, size_t workspace_bytes, void* stream);

/* Bytes of non-zero entries one row pass / one column pass of this problem reads (its own copies of the shard: 8 B per entry, 10 in the
 * three-array form; units in the 6-byte form of round 5 — values + 16-bit {key delta, accumulator} words — with their fillers and
 * padding). What the passes stream, next to the algorithmic 8 B per entry and pass the bench's roofline figure is quoted on. */
GDMIX_API int gdmix_fe_stream_bytes(gdmix_fe_problem* p, int64_t* rows_pass, int64_t* cols_pass);

/* Optional timing (HIP events on the launch stream): ms of the row pass (X theta) and the column pass (X'r) of the problem's SECOND
 * gdmix_fe_eval (its first, if there was only one) — not the last: with the status read a few steps late the last evaluations of a
 * solve are no-ops. */
GDMIX_API int gdmix_fe_last_eval_ms(gdmix_fe_problem* p, float* rows_ms, float* cols_ms);

#ifdef __cplusplus
}
#endif
#endif /* GDMIX_FE_H */
