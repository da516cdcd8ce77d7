/*
 * gdmix_re.h — C ABI of libgdmix_re.so, the MI355X-native random-effect (RE) trainer hot path.
 *
 * The reference (linkedin/gdmix, Python/TF/scipy, CPU only) has no FFI; the boundary this library
 * replaces is the body of three Python call sites (paths relative to the reference checkout):
 *
 *   prepare_jobs            gdmix-trainer/src/gdmix/models/custom/scipy/job_consumers.py:161-296
 *        -> gdmix_re_pack       (per-entity np.unique / local indexing / COO build, :243-250)
 *   BinaryLogisticRegressionTrainer.fit
 *                           gdmix-trainer/src/gdmix/models/custom/binary_logistic_regression.py:191-239
 *        -> gdmix_re_solve      (_loss :84-110, _gradient :121-131, scipy fmin_l_bfgs_b :223-231,
 *                                _compute_variance :144-189, threshold model_utils.py:4-12)
 *   BinaryLogisticRegressionTrainer.predict_proba(return_logits=True)
 *                           binary_logistic_regression.py:241-262, job_consumers.py:138-152
 *        -> gdmix_re_score
 *   Math.abs(id.toString.hashCode) % numPartitions
 *                           gdmix-data/src/main/scala/com/linkedin/gdmix/utils/PartitionUtils.scala:31-37
 *        -> gdmix_java_partition_id / gdmix_java_string_hash
 *
 * Conventions
 *   - every function returns 0 on success or a negative GDMIX_RE_E* code; nothing throws or aborts;
 *     gdmix_re_last_error() returns a thread-local NUL-terminated message for the last failure.
 *   - the caller owns every buffer. Device buffers may come from any allocator bound to the context's
 *     HIP device (the Python host passes torch tensor data_ptr()s). The library never frees or
 *     retains caller memory after the work enqueued on `stream` has completed.
 *   - all device work is enqueued on the caller's `stream` (a hipStream_t passed as void*; NULL = the
 *     default stream) and is asynchronous with respect to the host unless stated otherwise.
 *   - a context is bound to one HIP device; calls on one context must be serialised by the caller.
 *   - all arithmetic of the solver is IEEE fp64 on fp32-valued inputs, as in the reference.
 */
#ifndef GDMIX_RE_H_
#define GDMIX_RE_H_

#include <stdint.h>
#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GDMIX_RE_ABI_VERSION 27

#if defined(__GNUC__)
#define GDMIX_API __attribute__((visibility("default")))
#else
#define GDMIX_API
#endif

/* error codes */
#define GDMIX_RE_OK          0
#define GDMIX_RE_EINVAL    (-1)   /* bad argument */
#define GDMIX_RE_EHIP      (-2)   /* a HIP runtime call failed (no device, launch failure, ...) */
#define GDMIX_RE_ENOMEM    (-3)   /* workspace too small */
#define GDMIX_RE_ERANGE    (-4)   /* an entity exceeds an int32 per-entity limit; an evaluation of 2^31 samples or entities or more */

/* per-entity solver status, mirrors scipy fmin_l_bfgs_b's task/warnflag */
#define GDMIX_RE_ST_PGTOL     0   /* CONVERGENCE: NORM OF PROJECTED GRADIENT <= PGTOL      */
#define GDMIX_RE_ST_FACTR     1   /* CONVERGENCE: REL_REDUCTION_OF_F <= FACTR*EPSMCH         */
#define GDMIX_RE_ST_MAXITER   2   /* STOP: TOTAL NO. of ITERATIONS REACHED LIMIT             */
#define GDMIX_RE_ST_MAXFUN    3   /* STOP: TOTAL NO. of f AND g EVALUATIONS EXCEEDS LIMIT    */
#define GDMIX_RE_ST_ABNORMAL  4   /* ABNORMAL_TERMINATION_IN_LNSRCH                          */
#define GDMIX_RE_ST_ABORTED   9   /* device-wide kernel gave up waiting at a barrier (never expected; the result is invalid) */
#define GDMIX_RE_ST_ABORTED_PEER 10 /* fixed effect with several workers: ANOTHER worker's step was aborted; its mark came with the
                                     * all-reduce and every worker stops in the same evaluation (the result is invalid) */
/* "converged" for the entities/sec metric = status in {PGTOL, FACTR, MAXITER}: the reference treats
 * all three as a finished model (job_consumers.py:36-63 never looks at warnflag). */

#define GDMIX_RE_VAR_NONE    0
#define GDMIX_RE_VAR_SIMPLE  1    /* 1/(diag(X'DX) + l2 + 1e-12), binary_logistic_regression.py:175-180 */
#define GDMIX_RE_VAR_FULL    2    /* diag(inv(X'DX + (l2+1e-12)I)),                         :181-187 */

typedef struct gdmix_re_ctx gdmix_re_ctx;

/* ---- raw entity-grouped batch: exactly what prepare_jobs slices per entity ------------------------
 * E entities, N samples, Z non-zeros, entity-major then sample-major (the order of the TF sparse
 * tensors in job_consumers.py:176-199). Pointers are DEVICE pointers for gdmix_re_pack and HOST
 * pointers for the oracle. */
typedef struct {
  int64_t E, N, Z;
  const int64_t* ent_row_ptr;   /* [E+1] sample offsets of each entity                              */
  const int64_t* row_nnz_ptr;   /* [N+1] non-zero offsets of each sample                            */
  const int64_t* col_global;    /* [Z]   global feature index ("<bag>_indices")                     */
  const float*   val;           /* [Z]   feature value        ("<bag>_values")                      */
  const float*   y;             /* [N]   label, exactly 0.0f or 1.0f (fit() asserts this, :208)     */
  const float*   offset;        /* [N]   fixed-effect score (offset_column_name)                    */
  const float*   weight;        /* [N]   sample weight, or NULL => ones (job_consumers.py:255-256)  */
} gdmix_re_raw_batch;

/* ---- the same batch in its 32-bit hand-over form (what crosses PCIe) -------------------------------
 * Counts instead of pointers, int32 or uint16 feature ids (gdmix_re_pack requires them below 2^31 anyway), byte
 * labels: 0.47 of the bytes of the raw form for C2. gdmix_re_widen rebuilds the raw arrays in HBM; val / offset / weight
 * are used in place. The counts must add up: sum(ent_n) == N, sum(row_nnz) == Z. DEVICE pointers. */
typedef struct {
  int64_t E, N, Z;
  const int32_t* ent_n;         /* [E] samples of each entity                                          */
  const void*    row_nnz;       /* [N] non-zeros of each sample, unsigned, row_nnz_width bytes each     */
  int32_t        row_nnz_width; /* 1, 2 or 4                                                            */
  int32_t        y_width;       /* 1: y is uint8 0/1 (logistic labels); 4: y is float                   */
  int32_t        col_width;     /* 4: col_global is int32; 2: uint16 (feature spaces of at most 65536)  */
  int32_t        reserved;
  const void*    col_global;    /* [Z]                                                                  */
  const float*   val;           /* [Z]                                                                  */
  const void*    y;             /* [N]                                                                  */
  const float*   offset;        /* [N]                                                                  */
  const float*   weight;        /* [N] or NULL                                                          */
} gdmix_re_wire_batch;

/* ---- packed ragged CSR(+CSC) batch in HBM, produced by gdmix_re_pack ------------------------------
 * All pointers point into the caller-provided workspace (or alias the raw batch for y/offset/weight).
 * Entity e owns
 *   samples       [ent_row_ptr[e],  ent_row_ptr[e+1])            n_e
 *   non-zeros     [ent_nnz_ptr[e],  ent_nnz_ptr[e+1])            z_e  (must be < 2^31)
 *   features      [ent_feat_ptr[e], ent_feat_ptr[e+1])           d_e  distinct global indices
 *   coefficients  [ent_feat_ptr[e] + e*has_intercept, +p_e)      p_e = d_e + has_intercept
 *   row_ptr       [ent_row_ptr[e] + e,  + n_e + 1)   entity-relative nnz offsets (CSR)
 *   col_ptr       [ent_nnz_ptr[e] + e,  + d_e + 1)   entity-relative nnz offsets (CSC); addressed by the
 *                 entity's non-zero offset (d_e <= z_e) so that packing does not wait for the prefix sum of d_e
 * unique_global is sorted ascending inside an entity (np.unique, job_consumers.py:243); csr_col are
 * local indices 0..d_e-1; the CSC copy is sorted by (local col, sample) so that the transposed
 * product X'r is an ordered, atomic-free per-coefficient sum. */
typedef struct {
  int64_t E, N, Z, D;           /* D = sum of d_e; valid on the host once the pack stream is synced */
  const int64_t* ent_row_ptr;   /* [E+1] */
  int64_t*       ent_nnz_ptr;   /* [E+1] */
  int64_t*       ent_feat_ptr;  /* [E+1] */
  int32_t*       row_ptr;       /* [N+E] */
  int32_t*       csr_col;       /* [Z]   */
  float*         csr_val;       /* [Z]   */
  int32_t*       col_ptr;       /* [Z+E] sparse: d_e + 1 entries at ent_nnz_ptr[e] + e */
  int32_t*       csc_row;       /* [Z]   entity-relative sample index */
  float*         csc_val;       /* [Z]   */
  int32_t*       unique_global; /* [D]   (allocated Z) local -> global feature index; int32 since ABI 12 (was int64: global feature
                                 *       indices are below 2^31 on this path, and the array is written, copied to the host and read there
                                 *       once per partition — half the bytes each time) */
  const float*   y;             /* [N]   */
  const float*   offset;        /* [N]   */
  const float*   weight;        /* [N] or NULL */
  /* solver-owned scratch inside the workspace (written by gdmix_re_solve) */
  int32_t*       order;         /* [E]   entity ids grouped by size class (solver launch order)     */
  int32_t*       cls_tmp;       /* [E]   size class of each entity                                  */
  int32_t*       class_count;   /* [6*NUM_CLASSES] per-class counts / bases / cursors / largest nnz / total nnz (u64) (device) */
  void*          scratch;       /* pack-time sort scratch, free for reuse once pack has returned    */
  size_t         scratch_bytes;
  int32_t        max_p, max_n, max_nnz;  /* per-entity maxima over the batch (host, after pack)     */
} gdmix_re_packed;

#define GDMIX_RE_NUM_CLASSES 40

/* ---- solver options (defaults = REParams/LRParams defaults + scipy defaults) ----------------------
 * base_lr_params.py:22-27, binary_logistic_regression.py:223-231 (pgtol/maxfun/maxls are scipy's). */
typedef struct {
  double  l2;               /* l2_reg_weight                          default 1.0   */
  int32_t regularize_bias;  /*                                        default 1     */
  int32_t has_intercept;    /*                                        default 1     */
  int32_t m;                /* num_of_lbfgs_curvature_pairs           default 10    */
  int32_t max_iter;         /* num_of_lbfgs_iterations                default 100   */
  int32_t maxfun;           /* scipy default                          15000         */
  int32_t maxls;            /* scipy default                          20            */
  double  ftol;             /* = factr*eps = lbfgs_tolerance          default 1e-12 */
  double  pgtol;            /* scipy default                          1e-5          */
  int32_t variance_mode;    /* GDMIX_RE_VAR_*                         default NONE  */
  double  threshold;        /* sparsity_threshold applied to theta_thr, default 1e-4 (model_utils.py:4-12) */
  /* The two switches below together turn the per-entity objective into the fixed-effect one
   * (fixed_effect_lr_lbfgs_model.py:309-392): a batch with one "entity" = one worker's shard. Defaults 0.
   * sum_loss != 0 routes every entity to the device-wide team kernel, needs m <= 10 and refuses a variance mode. */
  int32_t sum_loss;         /* 1: f = sum_i w_i l_i + (l2/2)|theta_reg|^2, not divided by n (:363-381)            */
  int32_t loss;             /* the loss code, GDMIX_RE_LOSS_* below (ABI 19; until then a flag: 0 logistic, non-zero squared). 1: l_i = (y_i - z_i)^2
                             * (linear regression, :356-358), 2: l_i = exp(z_i) - y_i z_i (section "poisson" below). Any other value is refused.
                             * (The field was called `linear` until the third loss; position and type are unchanged.) */
  /* loss == GDMIX_RE_LOSS_SQUARED with sum_loss == 0 is the random effect's linear regression (--model_type=linear_regression; the reference has none: this
   * is its per-entity objective with its fixed-effect loss put in). For one entity of n samples, theta in local index space, intercept
   * first, labels y real-valued:
   *     z_i = x_i . theta + offset_i
   *     f(theta) = (1/n) ( sum_i w_i (y_i - z_i)^2 + (l2/2) |theta_reg|^2 )
   *     g        = (1/n) ( X~' (2 w (z - y)) + l2 theta_reg )
   * Everything else is as for the logistic loss: the same L-BFGS-B loop, theta0, m, max_iter, ftol, pgtol, maxls, every stop and status
   * code, thresholding into theta_thr, and the same size classes (classification goes by LDS footprint): every solve kernel has an
   * instantiation of its own for this loss. Variance is _compute_variance (binary_logistic_regression.py:144-189) with the curvature
   * weight D_i = 2 w_i in place of rho_i (1 - rho_i) w_i — it does not depend on theta:
   *     SIMPLE  1 / (sum_i D_i X~_ij^2 + l2 [- l2 for an unregularised intercept] + 1e-12)
   *     FULL    diag((X~' D X~ + (l2 + 1e-12) I [- l2 e0 e0'])^-1)      (gdmix_re_variance_full takes the loss from opts->loss too)
   * neither divided by n, as in the reference. gdmix_re_score is the same for every loss: x . theta + offset.
   *
   * ---- poisson (ABI 19) ----
   * loss == GDMIX_RE_LOSS_POISSON is Poisson regression (--model_type=poisson_regression; Photon-ML's PoissonLossFunction). For one
   * entity of n samples, theta in local index space, the intercept first, labels y >= 0 real-valued:
   *     z_i = x_i . theta + offset_i
   *     f   = (1/n) ( sum_i w_i (exp(z_i) - y_i z_i) + (l2/2) |theta_reg|^2 )
   *     g   = (1/n) ( X~' (w (exp(z) - y)) + l2 theta_reg )
   *     D_i = w_i exp(z_i)            curvature weight for SIMPLE / FULL variance, at the returned theta
   * The constant log(y!) is dropped. Everything else is exactly as for the other two losses (the loop, every stop and status code,
   * thresholding, the size classes: a batch lands in the classes it lands in with the logistic loss), and every solve kernel has an
   * instantiation of its own for this loss. The variances are those above with this D_i, not divided by n. With SIMPLE variance the
   * classes of the team kernels need out->theta (D is evaluated at it by a kernel that follows them). gdmix_re_score is unchanged: the
   * score is the margin z, never exp(z), which is what lets a stage's scores be the next stage's offsets.
   * exp is the library's own (one range reduction, a degree-13 polynomial, ldexp: <= 0.98 ulp on normal results, gradual underflow) and
   * IEEE at the ends: +inf past z ~ 709.78, NaN for NaN. The solver does nothing special about either: every loop is bounded by maxls,
   * max_iter and maxfun, so such an entity ends with a status code. Keeping negative and non-finite labels out is the host's business. */
} gdmix_re_opts;

#define GDMIX_RE_LOSS_LOGISTIC 0
#define GDMIX_RE_LOSS_SQUARED  1
#define GDMIX_RE_LOSS_POISSON  2

/* fills *o with the defaults above */
GDMIX_API void gdmix_re_default_opts(gdmix_re_opts* o);

/* ---- per-entity / per-coefficient outputs of a solve (device pointers; any may be NULL) ----------- */
typedef struct {
  double*  theta;      /* [P]  raw L-BFGS result (result[0] of fmin_l_bfgs_b), local index space     */
  double*  theta_thr;  /* [P]  after threshold_coefficients(|x|<=threshold -> 0)                     */
  double*  variance;   /* [P]  when opts.variance_mode != NONE                                       */
  double*  fval;       /* [E]  final objective                                                       */
  double*  gnorm;      /* [E]  max|g| at the returned point                                          */
  int32_t* nit;        /* [E]                                                                        */
  int32_t* nfev;       /* [E]                                                                        */
  int32_t* status;     /* [E]  GDMIX_RE_ST_*                                                         */
} gdmix_re_result;

GDMIX_API int  gdmix_re_abi_version(void);
/* (ABI 12) Hash (16 hex digits) of the sources this binary was compiled from — the .hip units, csrc/*.hpp and the two C headers;
 * gdmix_amd/build.py: source_id(). The library travels prebuilt next to its sources; the Python loader refuses a binary whose id is
 * not the hash of the sources beside it, and build.needs_build() compares this id, not modification times. */
GDMIX_API const char* gdmix_re_build_id(void);
GDMIX_API const char* gdmix_re_last_error(void);

/* (ABI 12) Two PROCESSES on one device — the reference starts num_of_consumers processes per worker
 * (random_effect_lr_lbfgs_model.py:103,214-217) and TF_CONFIG may list more workers than the box has GPUs. The solver's persistent grids
 * (team tiers, tall teams) need all their workgroups resident; two of them from two processes can starve each other. They are chained by a
 * file lock per device (<GDMIX_RE_LOCK_DIR or /tmp>/gdmix_re_grid_<pci bus id>.lock, held while a process has such a grid in flight; a
 * turnstile file keeps two processes alternating; GDMIX_RE_GRID_LOCK=0 turns it off). These three entry points are that lock for a named
 * key, host only — what tests/test_grid_lock.py drives from several processes. acquire blocks until this process may launch (it counts:
 * one release per acquire); stats returns how often the process took the file lock and how often a launch rode on a lock it already held. */
/* 1 if ANOTHER process has a context on this context's device right now (each process holds a record lock on a per-device file from its
 * first gdmix_re_create on; same directory and switch as above), 0 if not, < 0 on error. What gdmix_fe_create asks before it chooses the
 * one-launch step (whose workgroups wait for each other: next to another process's persistent grid it takes the three-launch form). */
GDMIX_API int gdmix_re_device_shared(gdmix_re_ctx* ctx);
GDMIX_API int gdmix_re_grid_lock_acquire(const char* key);
GDMIX_API int gdmix_re_grid_lock_release(const char* key);
GDMIX_API int gdmix_re_grid_lock_stats(const char* key, int64_t* takes, int64_t* rides);

GDMIX_API int  gdmix_re_create(int hip_device, gdmix_re_ctx** out);
GDMIX_API void gdmix_re_destroy(gdmix_re_ctx* ctx);

/* Bytes of device workspace gdmix_re_pack needs for a batch of this shape (upper bound; host-only). */
GDMIX_API size_t gdmix_re_pack_workspace_bytes(int64_t E, int64_t N, int64_t Z);

/* Pack: per entity, unique-sort the global feature indices, re-index the non-zeros locally, build the
 * CSR and CSC copies and the size-class launch order — all on the device. Fills *out (a host struct
 * of device pointers into `workspace`). Synchronises `stream` once to read back D and the class
 * counts. replaces job_consumers.py:209-258 (enable_local_indexing=True form; the reference's
 * global-indexing form yields identical coefficients on the entity's support). */
GDMIX_API int gdmix_re_pack(gdmix_re_ctx* ctx, const gdmix_re_raw_batch* raw_dev, int has_intercept,
                  void* workspace, size_t workspace_bytes, gdmix_re_packed* out, void* stream);

/* (ABI 11) The last kernel of a pack compacts every entity's unique feature ids into `unique_global` — the one output no solve
 * kernel reads (it names the coefficients for the model table, job_consumers.py:243, and maps a fixed-effect shard's columns). With
 * `enabled` != 0 gdmix_re_pack queues that kernel on a side stream of the context and returns without waiting for it, so it runs
 * NEXT to the gdmix_re_solve the caller queues behind the pack: a copy-shaped kernel beside kernels bound by their arithmetic.
 * Every other member of gdmix_re_packed is ordered on `stream` as before. `unique_global` is ordered on the stream of the next of
 * these calls on the same context: gdmix_re_solve (on return the stream is behind the compaction as it is behind the solve),
 * gdmix_re_solve_box (before its first kernel: it reads the array), gdmix_re_score, gdmix_re_variance_full, gdmix_fe_create, gdmix_re_pack (the next batch), gdmix_re_pack_join, gdmix_re_join_features,
 * gdmix_re_score_models. A caller that reads
 * unique_global itself, or frees / reuses the workspace, without one of them in between calls gdmix_re_pack_join(ctx, stream)
 * first. Default off (everything stream-ordered when gdmix_re_pack returns); gdmix_amd/solver.py switches it on. Results are the
 * same bits either way. A context without side streams ignores the request. */
GDMIX_API int gdmix_re_set_defer_unique(gdmix_re_ctx* ctx, int enabled);
GDMIX_API int gdmix_re_pack_join(gdmix_re_ctx* ctx, void* stream);

/* Wire form -> raw form on the device (two prefix sums and two widening copies, ~0.3 ms for C2), enqueued on
 * `stream`; fills *out (a host struct of device pointers into `workspace` and into the wire arrays). The result
 * feeds gdmix_re_pack on the same stream. */
GDMIX_API size_t gdmix_re_widen_workspace_bytes(int64_t E, int64_t N, int64_t Z);
GDMIX_API int gdmix_re_widen(gdmix_re_ctx* ctx, const gdmix_re_wire_batch* wire_dev, void* workspace, size_t workspace_bytes,
                   gdmix_re_raw_batch* out, void* stream);

/* Solve every entity of the packed batch: the whole L-BFGS loop runs on the device, one wavefront
 * (or workgroup, for entities that do not fit a wavefront's LDS budget) per entity.
 * theta0: [P] warm-start coefficients in local index space, or NULL => zeros (fit():220-221). */
GDMIX_API int gdmix_re_solve(gdmix_re_ctx* ctx, const gdmix_re_packed* batch, const gdmix_re_opts* opts,
                   const double* theta0, const gdmix_re_result* out, void* stream);

/* Bytes of device scratch gdmix_re_solve needs beyond the pack workspace (0 if none). */
GDMIX_API size_t gdmix_re_solve_scratch_bytes(const gdmix_re_packed* batch, const gdmix_re_opts* opts);
GDMIX_API int    gdmix_re_set_scratch(gdmix_re_ctx* ctx, void* scratch, size_t bytes);

/* variance_mode FULL on its own: diag((X~' D X~ + (l2 + 1e-12) I - l2 e0 e0' [intercept unregularised])^-1) of every entity of the
 * batch at `theta` ([P], local index space), D = rho (1 - rho) w (binary_logistic_regression.py:181-187) -> variance [P].
 * Entities up to 16 384 coefficients (a dense p x p matrix per entity, as the reference builds). Needs the scratch of
 * gdmix_re_solve_scratch_bytes with variance_mode FULL. Also what the fixed-effect stage uses for its FULL variances on one
 * worker (fixed_effect_lr_lbfgs_model.py:296-305, 457-463: the same matrix, intercept last instead of first). */
GDMIX_API int gdmix_re_variance_full(gdmix_re_ctx* ctx, const gdmix_re_packed* batch, const gdmix_re_opts* opts, const double* theta,
                                     double* variance, void* stream);

/* ---- elastic net: per-entity models with an L1 term, solved by OWL-QN on the device (no ABI bump: two new symbols, nothing else moves) ----
 * --elastic_net_alpha (gdmix_amd/params.py, REParams; Photon-ML's elastic net per random-effect coordinate). For one entity of n samples, in
 * the conventions of gdmix_re_opts (theta in local index space, the intercept first, f divided by n):
 *     F(theta) = (1/n) ( sum_i w_i l(y_i, x_i . theta + offset_i) + (l2/2) |theta_R|^2 + l1 |theta_R|_1 )
 * l any of the three losses (opts->loss), l2 = opts->l2, R the set l2 regularises: every feature, and the intercept iff regularize_bias.
 * Photon-ML's (lambda, alpha) is l1 = alpha lambda, l2 = (1 - alpha) lambda. With l1 = 0 this is gdmix_re_solve's objective.
 * The algorithm is the step of include/gdmix_fe.h, "(ABI 23) L1 / elastic net", applied to this F, per entity: the pseudo-gradient, the
 * two-loop direction on it with H0 from the newest pair, the zeroing where d_j pg_j >= 0, the orthant, the projected trial point with
 * exact 0.0, backtracking from t = 1 / |pg|_2 (no pair stored) or 1 with c = 1e-4 on pg'(x(t) - x) and halving, the memory cleared after
 * maxls rejections and then status 4, pair storage iff s'y > 2.2e-16 y'y, and the stops 0 / 1 / 2 / 3 in that order. What differs from that
 * section, and only this: every term carries the 1/n (g is the gradient of the smooth part divided by n, and the pseudo-gradient adds or
 * subtracts l1 / n), R is the set above, and the intercept is coefficient 0 of the entity, not the last one. m, max_iter, maxfun, maxls, ftol
 * and pgtol are those of gdmix_re_opts; gdmix_re_opts does not grow.
 * Results: theta is the last accepted point, never a rejected trial, so coordinates the orthant projection set to zero are exactly 0.0;
 * theta_thr is that point thresholded as by gdmix_re_solve; fval = F with the L1 term; gnorm = |pg|_inf; nit, nfev (every evaluation counts)
 * and status follow the statement. Variances are those of the smooth part at the returned theta — SIMPLE inside the solve kernels, FULL by
 * gdmix_re_variance_full with the same l2 — for a coefficient at 0 too, as in the fixed effect.
 * gdmix_re_solve_l1: l1 must be finite and >= 0 (GDMIX_RE_EINVAL otherwise). l1 == 0 forwards to gdmix_re_solve: the plain fit, bit for bit.
 *   sum_loss != 0 is refused (GDMIX_RE_EINVAL: the fixed effect's elastic net is gdmix_fe_set_l1). An empty batch returns right behind the
 *   argument checks. theta0 is the OWL-QN start point (NULL: zeros).
 * Routing. The size classes of gdmix_re_solve are not involved (GDMIX_RE_NUM_CLASSES and the class table are untouched). An entity is solved
 *   by re_owlqn_wave_kernel — one wavefront, the entity's block and the whole solver state in LDS — iff its OWL-QN LDS footprint (the plain
 *   wavefront kernel's plus one coefficient vector, rounded up to 16 bytes) is within the context's wave_lds_limit
 *   (gdmix_re_set_wave_lds_limit; 0: no entity), and otherwise, whatever its size, by re_owlqn_block_kernel: one workgroup per entity, the
 *   state in a global scratch slot per workgroup, X streamed. One kernel writes the two lists into the batch's solver-owned `order` (the
 *   first from the front, the second from the back); after the call the first two words of class_count hold their lengths (a later
 *   gdmix_re_solve overwrites the record). The wavefront kernel's workgroup is one wavefront and its LDS bounds how many a CU holds, so its
 *   entities within 20 KB are launched apart from the others, with that much LDS (their list is in the solver-owned cls_tmp). The two launches run side by side where the context has side streams. No workgroup waits for
 *   another. Limits: one workgroup per large entity (no team, device-wide, tall or several-entities-per-wavefront variants: the head of a
 *   Zipf distribution runs one workgroup per entity); no l2 sweep, no prior, no normalisation and no re-balancing compose with it on the
 *   host (gdmix_amd/params.py).
 * gdmix_re_solve_l1_scratch_bytes: device scratch the call needs beyond the pack workspace (gdmix_re_set_scratch), never less than
 *   gdmix_re_solve_scratch_bytes of the same arguments. With less, the workgroup kernel runs on as many slots as fit (at least one). */
GDMIX_API int gdmix_re_solve_l1(gdmix_re_ctx* ctx, const gdmix_re_packed* batch, const gdmix_re_opts* opts, double l1,
                                const double* theta0, const gdmix_re_result* out, void* stream);
GDMIX_API size_t gdmix_re_solve_l1_scratch_bytes(const gdmix_re_packed* batch, const gdmix_re_opts* opts);

/* ---- box constraints: per-entity models inside a box, solved by projected L-BFGS on the device (no ABI bump: two new symbols, nothing else moves) ----
 * --entity_coefficient_constraints (gdmix_amd/params.py, REParams; Photon-ML's coefficient box constraints per random-effect coordinate). For
 * one entity of n samples, in the conventions of gdmix_re_opts (theta in local index space, the intercept first, everything divided by n):
 *     F(theta) = (1/n) ( sum_i w_i l(y_i, x_i . theta + offset_i) + (l2/2) |theta_R|^2 )      subject to  lo_j <= theta_j <= hi_j
 * l any of the three losses (opts->loss), l2 = opts->l2, R the set l2 regularises: every feature, and the intercept iff regularize_bias.
 * lo_j may be -inf, hi_j may be +inf, lo_j == hi_j pins a coefficient; the intercept is never bounded. One box per global feature id, the
 * same for every entity that has the feature.
 * The algorithm is the step of include/gdmix_fe.h, "(ABI 26) box constraints", applied to this F, per entity. With g the gradient of F
 * (l2 term included) at the accepted point x and clamp(v)_j = min(max(v_j, lo_j), hi_j), exactly the bound's double where it clamps:
 *   binding set      B = { j : (x_j <= lo_j and g_j > 0) or (x_j >= hi_j and g_j < 0) or lo_j == hi_j }; reduced gradient q_j = 0 on B, g_j off B.
 *   direction        the two-loop recursion on q over the last <= m stored pairs s = x+ - x, y = g+ - g, H0 = (s'y / y'y) I from the newest
 *                    pair, negated; then d_j = 0 on B and wherever x_j <= lo_j and d_j < 0 or x_j >= hi_j and d_j > 0. No pair stored: d = -q.
 *   trial            x(t) = clamp(x + t d).
 *   search           t = 1 / |q|_2 while no pair is stored, else 1; accepted when F(x(t)) <= F(x) + 1e-4 g'(x(t) - x), else t is halved. After
 *                    maxls rejected trials in one iteration: the memory is cleared and the search starts again along -q if a pair was
 *                    stored, else the solve stops with status 4 at x.
 *   pair storage     only if s'y > 2.2e-16 y'y.
 *   stops            after each accepted iterate, in this order: gnorm = max_j |x_j - clamp(x - g)_j| <= pgtol -> 0 (the projected-gradient
 *                    norm; also tested at the start point); F_old - F <= ftol max(|F_old|, |F|, 1) -> 1; nit >= max_iter -> 2;
 *                    nfev > maxfun -> 3. Every evaluation counts in nfev.
 *   start point      clamp(theta0); zeros (theta0 NULL) are clamped too.
 * What differs from the fixed effect's section, and only this: every term carries the 1/n, R is the set above, and the intercept is
 * coefficient 0 of the entity, not the last one. m, max_iter, maxfun, maxls, ftol and pgtol are those of gdmix_re_opts; gdmix_re_opts does
 * not grow.
 * gdmix_re_solve_box: lower, upper are device pointers to num_features doubles each, indexed by GLOBAL feature id — the ids unique_global
 *   holds — and shared by every entity; they are not expanded to the batch's P coefficients (16 B per coefficient of extra HBM and a pass to
 *   build it, against two tables of D doubles that stay in L2). A solve kernel gathers lower[unique_global[f0 + j]] once per entity while it
 *   stages the block and keeps lo and hi next to the solver state; the intercept's slot gets -inf / +inf. Either pointer may be NULL: no
 *   bound on that side. Both NULL forwards to gdmix_re_solve: the plain fit, bit for bit. unique_global may come from a deferred compaction
 *   (gdmix_re_set_defer_unique): the call orders `stream` behind it before its first kernel reads the array (it is one of the calls listed
 *   there).
 *   Refused with GDMIX_RE_EINVAL, the results untouched: a NaN bound; lo_j > hi_j; num_features not above the largest id of the batch (or
 *   negative); sum_loss != 0 (the fixed effect's box is gdmix_fe_set_bounds); a loss code outside the three. The caller's arrays are checked
 *   on the device and the verdict comes back with the read-back the call waits for anyway (the list lengths): one host wait per solve. An
 *   empty batch returns right behind the host-side argument checks.
 * Results: theta is the last accepted point, never a rejected trial: lo <= theta <= hi holds exactly and a clamped coordinate is the bound's
 *   double. theta_thr is that point thresholded as by gdmix_re_solve, except that a coefficient whose box does not contain 0 (lo_j > 0 or
 *   hi_j < 0) keeps its value: the written model lies in the box too. fval = F, gnorm = the projected-gradient norm above; nit, nfev and status
 *   follow the statement. Variances are those of the smooth objective at the returned theta — SIMPLE inside the solve kernels, FULL by
 *   gdmix_re_variance_full, unchanged — for a coefficient at a bound too (the fixed effect's choice).
 * Routing is the elastic net's: the size classes are not involved; an entity is solved by re_owlqn_wave_kernel iff its footprint is within
 *   the context's wave_lds_limit, otherwise by re_owlqn_block_kernel (one workgroup, a scratch slot); the lists, the first two words of
 *   class_count and the two launches split at 20 KB are as there. The bounded step keeps x, g, d, xt, gt, lo and hi — seven coefficient vectors
 *   where OWL-QN has six; it needs no pseudo-gradient, q being a function of (g, x, lo, hi) — so its LDS footprint is the plain wavefront
 *   kernel's plus two coefficient vectors, rounded up to 16 bytes, and a scratch slot holds one vector more than the elastic net's. Limits
 *   as there: one workgroup per large entity; no L1 term, no prior, no normalisation, no l2 sweep and no re-balancing compose with it on the
 *   host (gdmix_amd/params.py).
 * gdmix_re_solve_box_scratch_bytes: device scratch the call needs beyond the pack workspace, never less than gdmix_re_solve_scratch_bytes of
 *   the same arguments. With less, the workgroup kernel runs on as many slots as fit (at least one). */
GDMIX_API int gdmix_re_solve_box(gdmix_re_ctx* ctx, const gdmix_re_packed* batch, const gdmix_re_opts* opts, const double* lower,
                                 const double* upper, int64_t num_features, const double* theta0, const gdmix_re_result* out, void* stream);
GDMIX_API size_t gdmix_re_solve_box_scratch_bytes(const gdmix_re_packed* batch, const gdmix_re_opts* opts);

/* ---- TRON: per-entity models by trust-region Newton on the device (no ABI bump: two new symbols, nothing else moves) ----
 * --entity_optimizer=TRON (gdmix_amd/params.py, REParams; Photon-ML's OptimizerType = TRON per random-effect coordinate). For one entity of n
 * samples, in the conventions of gdmix_re_opts (theta in local index space, the intercept first, everything divided by n):
 *     F(theta) = (1/n) ( sum_i w_i l(y_i, x_i . theta + offset_i) + (l2/2) |theta_R|^2 )
 * l any of the three losses (opts->loss), l2 = opts->l2, R the set l2 regularises: every feature, and the intercept iff regularize_bias. This
 * is gdmix_re_solve's objective, scaling and regularised set.
 * The algorithm is the section "(ABI 24) TRON" of include/gdmix_fe.h, applied to this F, per entity: Delta = |g|_2 at the start; Steihaug CG
 * with the boundary root in its cancellation-free form; |r - alpha Hd|^2 = r'r - 2 alpha r'Hd + alpha^2 |Hd|^2, clamped at 0; CG ends at
 * |r| <= 0.1 |g| or after GDMIX_FE_TRON_MAX_CG = 50 products in an outer iteration; eta = (1e-4, 0.25, 0.75), sigma = (0.25, 0.5, 4); every
 * trial before the first accepted step clamps Delta to |s|; a trial is accepted iff actred > 1e-4 prered. The stops, in that section's
 * order, with this solver's status codes: after an accepted step |g|_inf <= pgtol -> 0; f_old - f <= ftol max(|f_old|, |f|, 1) -> 1;
 * nit >= max_iter -> 2; nfev > maxfun -> 3; after a rejected trial nfev > maxfun -> 3; maxls (20 by default) rejected trials in a row -> 4,
 * at the accepted point. What differs from that section, and only this: every term carries the 1/n, R is the set above, and the intercept
 * is coefficient 0 of the entity, not the last one:
 *     H v = (1/n) ( X~' (D o X~ v) + l2 v_R ),   D_i = w_i rho_i (1 - rho_i) | 2 w_i | w_i exp(z_i)   (logistic | squared | Poisson)
 * with D taken at the accepted point: an evaluation leaves the trial point's D beside the residual in an array of its own, acceptance
 * exchanges the two arrays, and a rejected trial leaves the accepted point's D in force. A product is a row pass t_i = D_i (x_i . v) over
 * the entity's CSR copy and a column pass h_j = sum_i t_i x_ij over its CSC copy: no exp, no log, no reciprocal. max_iter, maxfun, maxls,
 * ftol and pgtol are those of gdmix_re_opts; m is ignored (there is no history); gdmix_re_opts does not grow.
 * Order of the sums. A row's x_i . v runs over the row's CSR entries in storage order, from the intercept's term; a column's sum runs over
 * its CSC entries in storage order. Of the NT threads that share an entity (64, or 256 in the workgroup kernel), thread t adds the samples
 * (coefficients) t, t + NT, ... in that order; the 64 lanes of a wavefront are added by one fixed tree, a workgroup's four wavefronts in
 * wavefront order. No atomics. A result therefore depends on the entity's own data, the options and the kernel that solves it, never on
 * where in the batch the entity sits or on how many entities the batch has.
 * Results: theta is the last accepted point, never a rejected trial; theta_thr is that point thresholded as by gdmix_re_solve; fval = F,
 * gnorm = |g|_inf; nit counts accepted iterations, nfev evaluations only, nhv ([E] int32, device, may be NULL) products. Variances are at the
 * returned theta — SIMPLE inside the solve kernels, from the D the solve holds (variance_simple's arithmetic, no second pass over exp), FULL
 * by gdmix_re_variance_full. theta0 is the start point (NULL: zeros), as in gdmix_re_solve.
 * gdmix_re_solve_tron refuses with GDMIX_RE_EINVAL: a NULL ctx, batch, opts or out; sum_loss != 0 (the fixed effect's TRON is
 *   gdmix_fe_set_optimizer); a loss code outside the three; max_iter < 0 or maxls < 1; variance outputs missing as for gdmix_re_solve. An
 *   empty batch returns right behind the argument checks.
 * Routing is the elastic net's shape: the size classes are not involved. An entity is solved by re_tron_wave_kernel — one wavefront, the
 *   entity's block and the whole solver state in LDS — iff its TRON LDS footprint is within the context's wave_lds_limit
 *   (gdmix_re_set_wave_lds_limit; 0: no entity), and otherwise, whatever its size, by re_tron_block_kernel: one workgroup per entity, the
 *   state in a global scratch slot per workgroup (7 max_p + 3 max_n + 8 doubles), X streamed. The footprint is the plain wavefront kernel's
 *   without its 2 m p + 2 m doubles of history, plus two coefficient vectors and two sample vectors:
 *   8 (7 p + 3 n) + 4 (4 nnz + (n + 1) + (d + 1) + (2 | 3) n) bytes, rounded up to 16 (seven coefficient vectors x g xt gt s r d — Hd lives
 *   in gt —, the residuals / t, and D of the accepted and of the trial point). One kernel writes the two lists into the batch's solver-owned
 *   `order`; after the call the first two words of class_count hold their lengths (a later solve overwrites the record). The wavefront
 *   kernel's entities within 20 KB are launched apart from the others, with that much LDS (eight one-wavefront workgroups per CU; their list
 *   is in the solver-owned cls_tmp). Limits: one workgroup per large entity (no size-class, tall, team or device-wide variants); no L1 term,
 *   no box, no prior, no normalisation, no l2 sweep and no re-balancing compose with it on the host (gdmix_amd/params.py).
 * gdmix_re_solve_tron_scratch_bytes: device scratch the call needs beyond the pack workspace (gdmix_re_set_scratch), never less than
 *   gdmix_re_solve_scratch_bytes of the same arguments. With less, the workgroup kernel runs on as many slots as fit (at least one). */
GDMIX_API int gdmix_re_solve_tron(gdmix_re_ctx* ctx, const gdmix_re_packed* batch, const gdmix_re_opts* opts, const double* theta0,
                                  const gdmix_re_result* out, int32_t* nhv, void* stream);
GDMIX_API size_t gdmix_re_solve_tron_scratch_bytes(const gdmix_re_packed* batch, const gdmix_re_opts* opts);

/* Score: logit[i] = x_i . theta_e + offset[i] (fp64 accumulate, stored fp32 as the score Avro
 * does, io_utils.py:367-375), logit_per_coord[i] = logit[i] - offset[i] (job_consumers.py:145-150).
 * has_model: [E] uint8, 0 => entity has no model and logit = offset (job_consumers.py:145-146);
 * NULL => all entities have one. theta is in the batch's local index space [P]. */
GDMIX_API int gdmix_re_score(gdmix_re_ctx* ctx, const gdmix_re_packed* batch, int has_intercept,
                   const double* theta, const uint8_t* has_model,
                   float* logit, float* logit_per_coord, void* stream);

/* Tuning/testing knob: entities whose LDS footprint exceeds `bytes` are solved by the
 * workgroup-per-entity kernel (0 => every entity). Default and maximum 65536. */
GDMIX_API int gdmix_re_set_wave_lds_limit(gdmix_re_ctx* ctx, int bytes);

/* Tuning/testing knob: which per-entity kernels the solver may use. bit 1 = LDS-resident wavefront kernel (any m), bit 2 = the
 * group kernels (several entities per wavefront); the tall kernel and the team kernels are always available. Default 7. Bit 0 was
 * round 1's register-resident one-entity-per-wavefront kernel: unreachable under default routing once the group kernels covered
 * p <= 2048 (tests/test_gpu_parity.py::test_default_routing_reaches_only_these_classes), removed in round 4 with its thirteen size
 * classes (ABI 8, GDMIX_RE_NUM_CLASSES 38; 39 since the tall team class of ABI 9); the bit is accepted and ignored. (Round 2's bit 3, team kernels with the history in
 * registers, went in round 3 - profiles/r03_zipf_register_team_kernels.txt.) */
GDMIX_API int gdmix_re_set_kernel_mask(gdmix_re_ctx* ctx, int mask);

/* The head of a Zipf-distributed partition is solved by a persistent kernel (one workgroup per CU) split into teams
 * of CUs, every team taking the next entity of its tier as it becomes free, largest first. Tiers by non-zeros:
 *   [team_nnz, 8 team_nnz)        128 teams of 2 CUs
 *   [8 team_nnz, 128 team_nnz)     32 teams of 8 CUs
 *   [128 team_nnz, giant_nnz)       8 teams of 32 CUs
 *   >= giant_nnz                    the whole device, one entity after another
 * (these entities are bound by synchronisation and memory latency, not by throughput: small teams, many at a time).
 * Smaller entities: one workgroup each. Defaults team_nnz 16384, giant_nnz 16777216; 0 disables the tiers above /
 * the device-wide tier. Results do not depend on the thresholds beyond summation order. */
GDMIX_API int gdmix_re_set_giant_nnz(gdmix_re_ctx* ctx, int64_t giant_nnz);
GDMIX_API int gdmix_re_set_team_nnz(gdmix_re_ctx* ctx, int64_t team_nnz);

/* Tall and skinny entities — at most 64 coefficients and at least `min_n` samples (MovieLens per-user / per-movie random
 * effects: up to ~54 k samples for 25 coefficients) — are solved by one workgroup each, the samples over all its lanes, the
 * L-BFGS driver replicated in every wavefront's registers (csrc/re_solve_tall.hip). 0 = never. Results do not depend on the
 * threshold beyond summation order. */
#define GDMIX_RE_TALL_MIN_N_DEFAULT 32
GDMIX_API int gdmix_re_set_tall_min_n(gdmix_re_ctx* ctx, int min_n);
/* Tall entities of at least `split_n` samples get a CU each (a workgroup of eight wavefronts); smaller ones share a CU,
 * eight single-wavefront workgroups at a time, so that one entity's L-BFGS driver (a latency-bound chain in one
 * wavefront) runs while the others' passes over their samples do. Until this is called the split is the default, lowered per
 * batch to 2 048 / 1 024 / 512 when the eight-wavefront class stays small that way; a split set by the caller is kept as it is,
 * also when it equals the default (the way to switch the per-batch choice off); split_n = 0 returns to the adaptive default. */
#define GDMIX_RE_TALL_SPLIT_N_DEFAULT 4096
GDMIX_API int gdmix_re_set_tall_split_n(gdmix_re_ctx* ctx, int split_n);
/* The tallest entities of a batch get a TEAM of four workgroups (four CUs of one XCD) that share the pass over one entity's
 * samples: a share of a strongly scaled MovieLens job lasts as long as ONE workgroup needs for its most rated title
 * (ABI 9, GDMIX_RE_NUM_CLASSES 39). `team_n` > 0: eight-wavefront tall entities of at least team_n, 2 team_n or 4 team_n samples
 * - the lowest of the three that keeps the class within one round of teams on the device (a quarter of its CUs' worth of entities); a batch with
 * more entities than that above 4 team_n has no team class (it is bound by throughput, not by one entity's chain).
 * `team_n` < 0: every tall entity of at least -team_n samples (at least 64), no limit. 0 = never. The split of an entity's samples
 * over the four workgroups depends on its size alone, and a team's result agrees with the one-workgroup kernel's to rounding
 * (another summation order) — but WHICH of the two kernels an entity gets depends on the batch when team_n > 0 (and likewise
 * for the per-batch split below gdmix_re_set_tall_split_n's default): the same entity can come out with other last bits in
 * another batch. A caller that needs results independent of the batching (entity re-balancing, comparisons across partitionings)
 * pins both: gdmix_re_set_tall_split_n(ctx, GDMIX_RE_TALL_SPLIT_N_DEFAULT) and gdmix_re_set_tall_team_n(ctx,
 * -GDMIX_RE_TALL_TEAM_N_DEFAULT) (gdmix_amd/solver.py: pin_routing). A device with fewer than 32 CUs never gets the class. */
#define GDMIX_RE_TALL_TEAM_N_DEFAULT 8192
GDMIX_API int gdmix_re_set_tall_team_n(gdmix_re_ctx* ctx, int team_n);
/* (ABI 12, GDMIX_RE_NUM_CLASSES 40) The MID tall class: in a SMALL batch (a share of a strongly scaled job) the largest one-wavefront tall
 * entities below the split get a workgroup of four wavefronts with half a CU's LDS (they stay resident there; on one wavefront they are
 * streamed, and the share lasts as long as that one wavefront's chain: random_effect_driver.py:60-68 splits the partitions over the
 * workers, BASELINE config 3). OFF by default: measured, it makes those shares slower (the one-wavefront launch is bound by the
 * throughput of its many small entities, not by its longest chain, and a mid workgroup takes LDS away from four of them:
 * profiles/r06_ml20m_mid.txt); kept, parity-tested, for devices where that balance differs. mid_n < 0: chosen per batch on the device — the lowest of 256 / 384 / 512 / 768 / 1 024 / 1 536
 * samples that keeps the class within one round of its launch (two workgroups per CU), only when the one-wavefront class is small and the
 * split is not pinned; mid_n > 0: every one-wavefront tall entity of at least mid_n samples, whatever the batch (tests); 0: never. Same
 * caveat as the teams: the kernel an entity gets depends on the batch, its sums are added in another order (agreement to rounding);
 * gdmix_re_set_tall_split_n(ctx, default) pins this choice too. GDMIX_RE_TALL_MID=1 in the environment switches the per-batch class on. */
GDMIX_API int gdmix_re_set_tall_mid_n(gdmix_re_ctx* ctx, int mid_n);

/* (ABI 20) The NARROW kernel. Entities of the class "re_solve_grp_kernel<32,3> n<=32 nnz<=128" with at most 80 coefficients, 24 samples
 * and 96 non-zeros are solved four to a wavefront by re_solve_grp_kernel<16,5,24,96> (five coefficients per lane; the older half of the
 * L-BFGS history in a per-lane ring instead of registers) instead of two to a wavefront. They stay entities of that class: its index,
 * name, count (gdmix_re_packed::class_count) and time (gdmix_re_last_solve_ms) are the class's; how many of them the narrow kernel took
 * is word GDMIX_RE_NARROW_COUNT_WORD of row 3 of class_count. Which kernel an entity gets depends on its own (p, n, nnz) alone, so its
 * result does not depend on the batch; the two kernels agree to rounding (a coefficient sum folds over 16 lanes instead of 32).
 * on = 0 switches the kernel off (every entity of the class as before ABI 20); GDMIX_RE_NARROW=0 in the environment sets that default
 * for new contexts. */
#define GDMIX_RE_NARROW_COUNT_WORD 15
GDMIX_API int gdmix_re_set_narrow(gdmix_re_ctx* ctx, int on);

/* Launch schedule of a solve. Size classes too small to fill the device always run next to the others on the context's side streams
 * (three, created with the context). `queues` > 1 (default 4 = the caller's stream + the three side streams; GDMIX_RE_SPREAD in the
 * environment sets the default of new contexts): the LARGE classes are dealt over that many streams in launch order as well, so that the
 * tail of one class launch (the entities with the most iterations) overlaps with the next class instead of idling the device; every
 * side stream is joined back into the caller's stream before gdmix_re_solve returns. 0 or 1: large classes one after another on the
 * caller's stream. A schedule changes the time, never a bit of the result; per-class durations (gdmix_re_last_solve_ms) of overlapped
 * launches stretch each other. */
GDMIX_API int gdmix_re_set_spread(gdmix_re_ctx* ctx, int queues);

/* Optional kernel timing: when enabled, gdmix_re_solve brackets each size class's kernel launch with
 * HIP events on the caller's stream; gdmix_re_last_solve_ms waits for them and returns the elapsed
 * milliseconds per class ([GDMIX_RE_NUM_CLASSES] floats, 0 for classes that were not launched). */
GDMIX_API int gdmix_re_set_timing(gdmix_re_ctx* ctx, int enabled);
GDMIX_API int gdmix_re_last_solve_ms(gdmix_re_ctx* ctx, float* ms_out);

/* Name of the kernel variant that solved size class c (for profiling reports), or NULL. */
GDMIX_API const char* gdmix_re_class_kernel_name(int c);

/* ---- (ABI 13) evaluation: the stage metric on the device — exact AUC and MSE, per entity and over a whole stage ------------------
 * What gdmix-data's Evaluator.scala computes in a Spark job of its own (Spark's BinaryClassificationMetrics / RegressionMetrics on
 * (score, label), unweighted), and the AUC per entity, which the reference cannot report. csrc/re_evaluate.hip.
 *
 * Definitions
 *   score       the fp32 predictionScore (what gdmix_re_score writes to `logit`). -0.0f equals +0.0f. Label positive <=> label > 0.5f.
 *   key         fp32 score -> uint32 that orders as the floats do (-0 canonicalised to +0; sign bit set for non-negative scores, all bits
 *               complemented for negative ones), the label in the low bit below it: a 33-bit key in which the negatives of a tie group
 *               sort in front of its positives. gdmix_amd/metrics.py: sortable_key is the host statement of the 32-bit part.
 *   twoU        sum over positives i of (2 #{negatives j: s_j < s_i} + #{negatives j: s_j == s_i}), an unsigned 64-bit integer.
 *               AUC = twoU / (2 n_pos n_neg), undefined (NaN) when n_pos == 0 or n_neg == 0: ties at half weight, what Spark's
 *               trapezoid over the distinct thresholds gives.
 *   SSE         sum of (label - score)^2 in fp64, both widened from fp32 first; MSE = SSE / n, n = n_pos + n_neg. Added in trees of a
 *               fixed shape (at most 2 048 terms in a row per lane; csrc/re_eval_sum.hpp states the shape): relative error below
 *               2.5e-13, the same bits from run to run.
 *   NaN         a NaN score is counted (n_nan) and left out of every sum and count; gdmix_amd/metrics.py reports AUC and MSE as NaN
 *               when n_nan > 0. Infinities order as usual.
 *   limits      fewer than 2^31 samples per evaluation and fewer than 2^31 entities: more is refused with GDMIX_RE_ERANGE and a
 *               message, never approximated.
 * The device returns the INTEGERS and the fp64 SSE; the global division is the caller's, from exact integers. Per entity the device also
 * writes auc[e] = (double)twoU / (2.0 * (double)n_pos * (double)n_neg), one division of exactly converted integers: exact (correctly
 * rounded) for entities below 2^26 samples — a caller redoes the division for larger ones.
 * Out of scope: sample weights in the metric; AUPR and RMSE (the Poisson loss, precision@k and the logistic loss have sections of their own
 * below); combining the accumulators of several workers (each worker
 * finishes its own; from the counts a caller can combine MSE exactly and AUC not at all). */
typedef struct {          /* device pointers, [E] each; any may be NULL */
  uint64_t* two_u;
  int32_t*  n_pos;
  int32_t*  n_neg;
  int32_t*  n_nan;
  double*   sse;
  double*   auc;
} gdmix_re_eval_out;

typedef struct {          /* host */
  uint64_t two_u;
  int64_t  n;             /* samples added, NaN scores included */
  int64_t  n_pos, n_neg, n_nan;
  double   sse;
} gdmix_re_eval_totals;

/* Per entity, for a scored batch: ent_row_ptr [E+1] (gdmix_re_packed.ent_row_ptr), score / label [N], all on the device. Entities of
 * at most 64 samples are evaluated in registers, without a sort (1, 2 or 4 per wavefront pass); larger ones by a radix sort of
 * (entity, key) and a rank-sum pass over the sorted keys. Results do not depend on which of the two an entity takes. Synchronises
 * `stream` once (to learn how many entities take the sort path). Workspace: gdmix_re_eval_workspace_bytes (host only; 0 beyond the
 * limits); too small a workspace is GDMIX_RE_ENOMEM. rocPRIM's temporary storage is the context's own (grow-only). */
GDMIX_API size_t gdmix_re_eval_workspace_bytes(int64_t E, int64_t N);
GDMIX_API int gdmix_re_eval_entities(gdmix_re_ctx* ctx, const int64_t* ent_row_ptr, int64_t E, int64_t N, const float* score, const float* label,
                                     const gdmix_re_eval_out* out, void* workspace, size_t workspace_bytes, void* stream);
/* Testing knob: entities of more than `small_max` samples take the sort path (0 => every entity that has a sample). 0 .. 64, default 64. */
GDMIX_API int gdmix_re_set_eval_small_max(gdmix_re_ctx* ctx, int small_max);

/* The metric of a whole stage, which scores partition after partition (and training next to validation data): an accumulator, a host
 * struct of the caller's. `keys` ([capacity] uint64 on the device: a sample's 33-bit key takes 8 bytes) and `state`
 * (GDMIX_RE_EVAL_ACC_STATE_BYTES on the device) are the caller's buffers; `count` is kept by the library. `reset` empties it; `add`
 * appends a batch's keys and adds up its SSE in one read of the samples; `finish` sorts once, runs the rank-sum pass with a single
 * segment, synchronises `stream` and fills *host_out — the accumulator stays as it is, more batches may follow. A key buffer too small
 * for count + N is GDMIX_RE_ENOMEM and nothing is added (the caller may move the keys to a larger buffer and set keys / capacity). The
 * integers do not depend on how the samples were split into batches or on the order of the batches. */
#define GDMIX_RE_EVAL_ACC_STATE_BYTES 33024
typedef struct {
  uint64_t* keys;
  int64_t   capacity;
  int64_t   count;
  void*     state;
} gdmix_re_eval_acc;
GDMIX_API int gdmix_re_eval_acc_reset(gdmix_re_ctx* ctx, gdmix_re_eval_acc* acc, void* stream);
GDMIX_API int gdmix_re_eval_acc_add(gdmix_re_ctx* ctx, gdmix_re_eval_acc* acc, const float* score, const float* label, int64_t N, void* stream);
GDMIX_API size_t gdmix_re_eval_acc_workspace_bytes(int64_t N);      /* N = acc->count */
GDMIX_API int gdmix_re_eval_acc_finish(gdmix_re_ctx* ctx, const gdmix_re_eval_acc* acc, void* workspace, size_t workspace_bytes,
                                       gdmix_re_eval_totals* host_out, void* stream);

/* ---- (ABI 19) poisson evaluation: the Poisson loss of a scored set, per entity and over a whole stage ---------------------------
 * The metric of a --model_type=poisson_regression stage, where a linear stage reports MSE. csrc/re_evaluate_poisson.hip. The structs and
 * entry points above are not involved.
 *   PL          sum_i (exp(s_i) - y_i s_i) in fp64, the fp32 score s and label y widened first (log(y!) dropped, as in training); the mean
 *               poisson_loss = PL / n is the caller's division. Unweighted, as the other metrics are.
 *   trees       added in the trees SSE is added in: both units take the shape from csrc/re_eval_sum.hpp, which states it. The same bits from
 *               run to run. The accumulator adds the sums of its batches to a (hi, lo) pair without losing the additions' rounding errors: the
 *               total is the rounded exact sum of the batches' sums, so it does not depend on the order the batches came in (two orders could
 *               differ only if that exact sum lay within 2^-100 of the midpoint of two doubles). The terms have either sign, so the bound is
 *               relative to the sum of magnitudes: |PL - exact| <= 3e-13 * sum_i (exp(s_i) + |y_i s_i|) — SSE's 2.5e-13 for the longest
 *               chain of additions (< 2 211 roundings) plus exp (<= 0.98 ulp) and the one rounding of exp(s) - y s (a fused multiply-add).
 *   NaN         a NaN score is counted (n_nan) and left out of the sum and of n. exp is IEEE: a score past ~88.7 (fp32) stays finite in fp64.
 *   infinities  an infinite score is a score like any other: it is counted in n and its term is what IEEE arithmetic makes of the statement.
 *               s = +inf: exp(s) = +inf, so the term is +inf for y < 0 and NaN (inf - inf, or 0 * inf) for y >= 0. s = -inf: exp(s) = 0 and
 *               the term is -y s: +inf for y > 0, -inf for y < 0, NaN for y = 0. A finite score past ~709.78 gives +inf (y s is finite), one
 *               below ~-745.13 gives -y s. (The log loss of an infinite score is exactly 0 on the label's side and +inf on the other.)
 *   limits      fewer than 2^31 samples per evaluation and fewer than 2^31 entities (GDMIX_RE_ERANGE).
 * Entities of at most 64 samples are summed in registers (four entities per wavefront, as gdmix_re_eval_entities does), larger ones by a
 * workgroup each; gdmix_re_set_eval_small_max moves the limit for both evaluations. No workspace, no synchronisation per entity call. */
typedef struct {          /* device pointers, [E] each; any may be NULL */
  double*  pl;
  int32_t* n;             /* samples with a score that is not NaN */
  int32_t* n_nan;
} gdmix_re_eval_pl_out;
typedef struct {          /* host */
  double  pl;
  int64_t n;              /* samples added whose score is not NaN */
  int64_t n_nan;
} gdmix_re_eval_pl_totals;
GDMIX_API int gdmix_re_eval_pl_entities(gdmix_re_ctx* ctx, const int64_t* ent_row_ptr, int64_t E, int64_t N, const float* score, const float* label,
                                        const gdmix_re_eval_pl_out* out, void* stream);
/* The accumulator of a stage: `state` (GDMIX_RE_EVAL_PL_STATE_BYTES on the device) is the caller's buffer, `count` is kept by the library.
 * `finish` synchronises `stream` and fills *host_out; the accumulator stays as it is, more batches may follow. */
#define GDMIX_RE_EVAL_PL_STATE_BYTES 33024
typedef struct {
  void*   state;
  int64_t count;
} gdmix_re_eval_pl_acc;
GDMIX_API int gdmix_re_eval_pl_acc_reset(gdmix_re_ctx* ctx, gdmix_re_eval_pl_acc* acc, void* stream);
GDMIX_API int gdmix_re_eval_pl_acc_add(gdmix_re_ctx* ctx, gdmix_re_eval_pl_acc* acc, const float* score, const float* label, int64_t N, void* stream);
GDMIX_API int gdmix_re_eval_pl_acc_finish(gdmix_re_ctx* ctx, const gdmix_re_eval_pl_acc* acc, gdmix_re_eval_pl_totals* host_out, void* stream);

/* ---- (ABI 27) ranking evaluation: per-entity precision@k as exact integers, and the logistic loss of a scored set -----------------------
 * What Photon-ML's multi-evaluators (AUC:<id>, PRECISION@K:<id>) and its LOGISTIC_LOSS evaluator report; the reference's Evaluator has
 * neither. csrc/re_evaluate.hip (precision@k), csrc/re_evaluate_poisson.hip (the logistic loss, the Poisson unit's second term).
 *
 * Definitions, per entity over its VALID samples
 *   valid       a sample whose score is not NaN. Label positive <=> label > 0.5f. Scores compare by the key of "evaluation" above: -0 equals
 *               +0, infinities order as usual.
 *   counts      n = n_pos + n_neg valid samples, an integer k >= 1.
 *               n <= k:  hits_sure = n_pos, slots = tie_pos = tie_size = 0.
 *               n > k:   c = the k-th largest score; `above` = the samples with score > c (a < k of them), `tie` = those with score == c
 *                        (tie_size >= k - a >= 1); hits_sure = positives in `above`, slots = k - a, tie_pos = positives in `tie`.
 *   H           expected hits = hits_sure + slots * tie_pos / tie_size (the last term 0 when tie_size == 0): the expectation of "sort
 *               descending, take k, count the positives" under a uniformly random order inside tie groups — for precision what "ties at
 *               half weight" is for AUC.
 *   precision@k H / k. The denominator is k also for an entity of fewer than k samples.
 * The device returns the four INTEGERS; the division is the caller's (gdmix_amd/metrics.py: precision_from_counts, correctly rounded).
 * Aggregates over a data set (the mean of per-entity AUC or precision@k) are the caller's too: an exact sum of the per-entity values.
 *
 * One call does ONE sort. Entities of at most 64 samples are ranked in registers, four per wavefront as in gdmix_re_eval_entities (a lane
 * counts the keys below and not above its own through LDS; the integers are sums of flags over the entity's lanes); larger ones go through
 * the (entity, key) radix sort of gdmix_re_eval_entities, then a workgroup per entity finds the cut key at position n - k of the valid part
 * of its sorted segment, the tie group by binary searches, and counts the positives above it. The two paths give identical integers;
 * gdmix_re_set_eval_small_max moves the limit for this call too. With auc_out non-NULL the call also fills what gdmix_re_eval_entities
 * fills, bit for bit (the same integers; sse from the same tree), so a stage that wants both pays one pass.
 *   ks          host, nk of them, 1 <= nk <= 4, distinct, each >= 1: anything else is GDMIX_RE_EINVAL (checked before anything is launched,
 *               also for an empty batch).
 *   out         device, [nk][E] each, k-major (the values of ks[j] at [j * E, (j + 1) * E)); any pointer may be NULL.
 * Limits, GDMIX_RE_ERANGE / GDMIX_RE_ENOMEM, the workspace and the single stream synchronisation are those of gdmix_re_eval_entities
 * (gdmix_re_eval_topk_workspace_bytes equals gdmix_re_eval_workspace_bytes). */
typedef struct {           /* device, [nk][E] each, k-major; any may be NULL */
  int32_t* hits_sure;
  int32_t* slots;
  int32_t* tie_pos;
  int32_t* tie_size;
} gdmix_re_eval_topk_out;
GDMIX_API size_t gdmix_re_eval_topk_workspace_bytes(int64_t E, int64_t N);
GDMIX_API int gdmix_re_eval_topk_entities(gdmix_re_ctx* ctx, const int64_t* ent_row_ptr, int64_t E, int64_t N, const float* score, const float* label,
                                          const int32_t* ks /* host */, int nk /* 1..4, distinct, each >= 1 */, const gdmix_re_eval_topk_out* out,
                                          const gdmix_re_eval_out* auc_out /* may be NULL */, void* workspace, size_t workspace_bytes, void* stream);

/* The logistic loss (log loss) of a scored set: LL = sum over valid samples of ce(s, y),
 *   ce(s, y) = max(s, 0) - s [y > 0.5] + log(1 + exp(-|s|)), in fp64 from the widened fp32 score; logistic_loss = LL / n is the caller's.
 * max(s, 0) - s [y > 0.5] is formed as max(-s, 0) for a positive and max(s, 0) for a negative (the same number, no rounding, no inf - inf);
 * exp and log are the library's own (csrc/re_device.hpp: exp_neg, log_1_2), and u = 1 + exp(-|s|) is rounded before the logarithm, as in the
 * solve kernels. That rounding is an ABSOLUTE error of the term, not a relative one. Measured against long double over every exponent of
 * fp32 scores and both labels (tools/logloss_check.c, 2^25 scores per label): |ce - exact| <= 2^-53 ce + eps with
 *   eps = GDMIX_RE_EVAL_LL_TERM_EPS,
 * so with the trees of csrc/re_eval_sum.hpp (the Poisson loss's shape, trees, TwoSum accumulator, NaN handling and limits; the same bits
 * from run to run; never a floating-point atomic):  |LL - exact| <= 2.5e-13 * sum_i ce_i + n * eps  (2.5e-13 covers the < 2 211 roundings of
 * the longest chain of additions and the one of the term).
 * The entry points mirror the gdmix_re_eval_pl_ family: the same structs (the field `pl` holds LL) and the same state size. */
#define GDMIX_RE_EVAL_LL_TERM_EPS 1.5e-16   /* measured 1.413e-16 (at s = 0.5575137); on an MI355X 1.306e-16 (at s = 0.5658179) over the grid of tests/eval_edges_helpers.py */
#define GDMIX_RE_EVAL_LL_STATE_BYTES GDMIX_RE_EVAL_PL_STATE_BYTES
typedef gdmix_re_eval_pl_out    gdmix_re_eval_ll_out;
typedef gdmix_re_eval_pl_totals gdmix_re_eval_ll_totals;
typedef gdmix_re_eval_pl_acc    gdmix_re_eval_ll_acc;
GDMIX_API int gdmix_re_eval_ll_entities(gdmix_re_ctx* ctx, const int64_t* ent_row_ptr, int64_t E, int64_t N, const float* score, const float* label,
                                        const gdmix_re_eval_ll_out* out, void* stream);
GDMIX_API int gdmix_re_eval_ll_acc_reset(gdmix_re_ctx* ctx, gdmix_re_eval_ll_acc* acc, void* stream);
GDMIX_API int gdmix_re_eval_ll_acc_add(gdmix_re_ctx* ctx, gdmix_re_eval_ll_acc* acc, const float* score, const float* label, int64_t N, void* stream);
GDMIX_API int gdmix_re_eval_ll_acc_finish(gdmix_re_ctx* ctx, const gdmix_re_eval_ll_acc* acc, gdmix_re_eval_ll_totals* host_out, void* stream);

/* ---- (ABI 14) sweep: K models trained on one batch score another batch in one pass over its non-zeros ----------------------------
 * A stage that sweeps l2_reg_weight (gdmix_amd/sweep.py) solves a training partition K times and scores the validation partition under
 * all K models. The models live in the TRAINING batch's coefficient index space (gdmix_re_result.theta_thr of K solves of one packed
 * batch); the validation partition is a packed batch of its own, with other entities and other features per entity. csrc/re_sweep.hip.
 *
 * gdmix_re_join_features: where in the training batch's coefficient array every coefficient slot of the evaluation batch finds its value.
 *   train_entity  [eval->E] int32, device: the training batch's row of the same entity, -1 if it has none (a value outside
 *                 [0, train->E) counts as none). The caller builds it from the two id lists; an id listed twice in the training batch
 *                 maps to its LAST row (the model a table built by dict.update keeps).
 *   coef_pos      [P_eval] int64, device, P_eval = eval->D + eval->E * has_intercept: for slot s of the evaluation batch (entity e, the
 *                 intercept or a global feature index g) the index in the training batch's [P_train] arrays of entity train_entity[e]'s
 *                 coefficient for the same thing: intercept -> intercept, g -> the slot whose unique_global is g; -1 where that entity
 *                 never saw g, or where e has no model.
 *   has_model     [eval->E] uint8, device: train_entity[e] names a row.
 *   Both unique_global lists are ascending inside an entity: a thread per evaluation feature bisects its entity's training list. Both
 *   batches need a valid D (the host struct after gdmix_re_pack). Reads unique_global of both batches: it orders a deferred compaction
 *   (gdmix_re_set_defer_unique) on `stream` first.
 *
 * gdmix_re_score_models: thetas = HOST array of K device pointers, each a [P_train] fp64 array in the training batch's index space.
 *   logit [K][N] (row k at logit + k * N), logit_per_coord [K][N] or NULL, fp32, N = eval->N. Defined by equivalence: with
 *       theta_mapped_k[s] = coef_pos[s] < 0 ? 0.0 : thetas[k][coef_pos[s]]
 *   row k is BIT FOR BIT what gdmix_re_score(eval, has_intercept, theta_mapped_k, has_model, ...) writes: the same products in the same
 *   order, every step one fused multiply-add acc = fma((double)v, t, acc) starting from the intercept (or +0.0 without one), a missing
 *   coefficient entering as +0.0 — so a zero logit has the sign it has there. has_model NULL: every entity has a model (every slot is
 *   then looked up; an intercept slot of -1 reads as +0.0). Every coef_pos entry must be -1 or below P_train (what
 *   gdmix_re_join_features writes); nothing else is checked on the device.
 *   One thread per sample, the entity search of gdmix_re_score; (value, column, coef_pos) of a non-zero are loaded once and feed the
 *   accumulators of up to GDMIX_RE_SWEEP_MODELS_PER_PASS models; a longer list takes several passes over the batch.
 *   workspace NULL: the K coefficients of a slot are gathered from the K arrays. workspace of at least
 *   gdmix_re_score_models_workspace_bytes(P_train, K) device bytes: each pass first copies its models into one slot-major array
 *   [P_train][models of the pass] there, and a slot's coefficients are one contiguous read. The same bits either way. */
#define GDMIX_RE_SWEEP_MODELS_PER_PASS 8
GDMIX_API int gdmix_re_join_features(gdmix_re_ctx* ctx, const gdmix_re_packed* eval, const gdmix_re_packed* train, int has_intercept,
                                     const int32_t* train_entity, int64_t* coef_pos, uint8_t* has_model, void* stream);
GDMIX_API size_t gdmix_re_score_models_workspace_bytes(int64_t P_train, int K);
GDMIX_API int gdmix_re_score_models(gdmix_re_ctx* ctx, const gdmix_re_packed* eval, int has_intercept, const double* const* thetas, int K,
                                    int64_t P_train, const int64_t* coef_pos, const uint8_t* has_model, float* logit, float* logit_per_coord,
                                    void* workspace, size_t workspace_bytes, void* stream);

/* ---- (ABI 16) incremental training: the L2 term centred on a prior model and weighted by its precisions ---------------------------
 * A warm start alone forgets the prior model once it converges: with l2 > 0 the optimum does not depend on the starting point. With
 * --incremental_training True (gdmix_amd/params.py; not in the reference, which leaves it open: random_effect_lr_lbfgs_model.py:155-160,
 * fixed_effect_lr_lbfgs_model.py:363-366) the prior model's means and variances (what --random_effect_variance_mode writes) define the
 * regulariser, as Photon-ML defines incremental training: a model trained on a new day's data alone is the Bayesian update of
 * yesterday's. csrc/re_prior.hip.
 *
 * Definition. One entity, theta in local index space, intercept first; coefficient j has a prior mean mu_j and a prior variance v_j,
 * s_j = sqrt(v_j):
 *     F(theta) = (1/n) ( sum_i w_i l(z_i, y_i) + (l2/2) sum_{j regularised} (theta_j - mu_j)^2 / v_j ),   z = X~ theta + offset
 * l the logistic or the squared loss (opts->loss) as without a prior.
 * Defaults. A coefficient has no prior when the entity is new, when the feature is new for the entity, when the coefficient was
 * thresholded out of the model file, when the record has no variances, or when its variance is missing, not finite or <= 0. Such a
 * coefficient gets mu_j = 0 where the mean is missing and v_j = 1 where the variance is missing: an entity without a prior has exactly
 * the objective of gdmix_re_opts.
 * The intercept. Every solve kernel's intercept column is the constant 1: it cannot be scaled, so s_0 = 1 for every intercept. An
 * unregularised intercept (regularize_bias 0) has no penalty anyway. A regularised one is penalised with v_0 = 1, (l2/2)(theta_0 -
 * mu_0)^2: its prior mean is honoured, its prior variance is not (F above with v_0 := 1), and its written variance is Var'(phi_0). mu_0
 * applies as the shift below either way.
 * Substitution. phi_j = (theta_j - mu_j) / s_j turns F into the objective of gdmix_re_opts in phi on a transformed batch:
 *     x'_ij     = x_ij s_j
 *     offset'_i = offset_i + sum_j x~_ij mu_j          (intercept included)
 *     penalty   = (l2/2) |phi_reg|^2,   phi0 = 0       (theta0 NULL: the solve starts at theta = mu)
 * and afterwards theta_j = mu_j + s_j phi_j, Var(theta_j) = v_j Var'(phi_j), Var' the variance mode (SIMPLE or FULL) of the transformed
 * batch, since H_theta^-1 = S H_phi^-1 S. No solve, pack, score or variance kernel knows about priors: gdmix_re_prior_apply makes the
 * transformed batch, gdmix_re_solve solves it, gdmix_re_prior_restore maps the result back.
 * Consequences.
 *   rounding    the transformed batch is held in the precision of every batch on this path: x' = (float)((double)x * s_j), one rounding
 *               per non-zero; offset' is the fp64 sum mu_0 + sum_j x_ij mu_j + offset_i rounded once to fp32 — what gdmix_re_score
 *               writes to `logit` for theta = mu (to the order of the sum). The problem solved is the one with these fp32 values; it
 *               differs from the exact-arithmetic F by a relative perturbation of the data of 2^-24.
 *   stop tests  pgtol, ftol and every other stop test of L-BFGS-B apply in phi-space: |s (.) grad_theta F|_inf <= pgtol. fval is F;
 *               nit, nfev and status are those of the transformed solve.
 *   threshold   the sparsity threshold applies to theta, not to phi.
 *
 * gdmix_re_prior_apply: mean / scale [P] fp64 on the device, P = packed->D + packed->E * has_intercept, in the batch's coefficient order;
 *   `scale` arrives computed (the host takes the square root: the caller and the device use the same bits). Writes new csr_val, csc_val and
 *   offset arrays into `workspace` (at least gdmix_re_prior_workspace_bytes(packed) device bytes; less is GDMIX_RE_ENOMEM) and fills *out
 *   as a copy of *packed that points at them. Index arrays, y, weight, order and the scratch are SHARED with *packed, not copied; *packed
 *   itself is left as it is (a stage scores it afterwards with theta). Work is dealt by sample rows and by non-zeros, never by entity (one
 *   batch holds entities of one non-zero next to a head of 2^20): the CSR pass gives a row to a lane, a row of more than 32 non-zeros to
 *   its whole wavefront, reads each non-zero once, gathers mu and s at (coefficient base + csr_col), writes x' and the row's offset';
 *   the CSC pass gives four consecutive non-zeros to a lane, which finds their column by bisection of the entity's col_ptr.
 * gdmix_re_prior_restore: phi [P] (gdmix_re_result.theta of the transformed solve), var_phi [P] or NULL ->
 *     theta[j]     = mean[j] + scale[j] * phi[j]                      (fp64, product and sum rounded separately)
 *     theta_thr[j] = |theta[j]| <= threshold ? 0.0 : theta[j]         (threshold_coefficients, as gdmix_re_solve applies it)
 *     variance[j]  = (scale[j] * scale[j]) * var_phi[j]               (when both variance and var_phi are given)
 *   theta, theta_thr, variance: any may be NULL; each may alias its input (phi, var_phi).
 * Both calls are stream-ordered, without a host synchronisation, and read nothing a deferred compaction writes (unique_global): they
 * need no gdmix_re_pack_join. */
GDMIX_API size_t gdmix_re_prior_workspace_bytes(const gdmix_re_packed* packed);
GDMIX_API int gdmix_re_prior_apply(gdmix_re_ctx* ctx, const gdmix_re_packed* packed, int has_intercept, const double* mean, const double* scale,
                                   void* workspace, size_t workspace_bytes, gdmix_re_packed* out, void* stream);
GDMIX_API int gdmix_re_prior_restore(gdmix_re_ctx* ctx, const gdmix_re_packed* packed, int has_intercept, const double* mean, const double* scale,
                                     double threshold, const double* phi, const double* var_phi, double* theta, double* theta_thr,
                                     double* variance, void* stream);

/* ---- (ABI 18) feature normalisation: exact column statistics on the device, factors, the expansion to coefficient order ---------------
 * --feature_normalization (gdmix_amd/params.py; Photon-ML's NormalizationType, not in the reference) penalises coefficients in normalised
 * units: the objective of gdmix_re_opts with the penalty (l2/2) sum_{j regularised} (theta_j / s_j)^2, which is the incremental section's F
 * with mu = 0 and v_j = s_j^2. gdmix_re_prior_apply / gdmix_re_solve / gdmix_re_prior_restore solve it as they stand (mean = 0, phi0 =
 * theta0 / s for a warm start); the stop tests apply in phi, the threshold to theta, Var(theta_j) = s_j^2 Var'(phi_j). What this section adds
 * is the column statistics the factors come from, csrc/feature_stats.hip.
 *
 * Data. The stage's training data: for the random effect the ACTIVE training samples of every partition in the partition list, for the
 * fixed effect the training samples of all workers. N is their number. Zeros are implicit; sample weights are not used (as in Photon's
 * summary). Statistics are taken over STORED ENTRIES: a (sample, feature) pair stored twice counts as two entries.
 * Per feature j of the bag, exact:
 *     count_j = the number of stored entries (int64),   a_j = max |x| (a float32, carried as its bit pattern)
 * and from these two alone
 *     E_j = floor(log2 a_j),  L_j = min(31, 62 - bit_length(count_j)),  shift1_j = 2 L_j - (E_j + 1),  shift2_j = 2 L_j - 2 (E_j + 1).
 * A feature with count_j = 0 or a_j = 0 is dead (limb_bits 0: it has no accumulator). L_j < 25 (more than 2^37 entries of one feature) is
 * an error naming the feature: below 25 the square of the column's largest value is no longer exact.
 * Moments, as exact integers:  I1_j = sum rint(x 2^shift1_j),  I2_j = sum rint(x^2 2^shift2_j): the float32 is widened to fp64, x x is exact,
 * the scaling is ldexp, the rounding ties-to-even. |x| <= a_j < 2^(E_j + 1), so each term is below 2^(2 L_j) in magnitude; it is split into
 * a high limb (arithmetic shift by L_j) and a low limb (mask), summed in separate int64 accumulators, which by the choice of L_j cannot
 * overflow. The host recombines I = hi 2^L + lo. Integer addition commutes: the four accumulators per feature do not depend on the order of
 * the entries, on how the data are cut into calls, on the launch geometry, on the path (LDS or global) or on the number of workers.
 * Bound per moment: |I1_j 2^-shift1_j - sum x| <= count_j 2^(E_j + 1 - 2 L_j) / 2, and |I2_j 2^-shift2_j - sum x^2| <= count_j 2^(2 (E_j + 1)
 * - 2 L_j) / 2 (half a unit of the last place of the scaled integer per entry).
 * Mean and variance (host, gdmix_amd/feature_stats.py), rounded to fp64 within 1 ulp of the exact rational value of
 *     mean_j = I1 2^-shift1 / N,     var_j = (I2 2^-shift2 - (I1 2^-shift1)^2 / N) / (N - 1)          (0 for N = 1)
 * Spark's unbiased variance with the zeros counted. var_j is exactly 0 when N I2 2^(2 L) = I1^2 (a constant dense column), and 0 where the
 * roundings of the terms leave that integer difference negative.
 * Factors. scale_with_standard_deviation: s_j = 1 / sqrt(var_j); scale_with_max_magnitude: s_j = 1 / a_j; s_j = 1 where the feature is
 * dead, where var_j = 0 or where the result is not finite; s = 1 for every intercept ("The intercept" above; for the fixed effect by this
 * feature's own choice, for regularised and unregularised intercepts alike).
 *
 * gdmix_re_feature_extent (pass 1) and gdmix_re_feature_moments (pass 2) are stream-ordered and ACCUMULATE into the caller's arrays (zeroed
 * before the first call; one call per partition or per chunk of a shard). col: Z column ids of col_width bytes (8: int64, 4: int32, 2:
 * uint16 — the raw batch's col_global, the wire form's narrower ids, the reader arrays gdmix_fe_score takes), val: Z floats.
 *   count [D] uint64, max_abs_bits [D] uint32 (the bit pattern of a non-negative float orders as the float does: an unsigned max)
 *   limb_bits / shift1 / shift2 [D] int32: L_j, shift1_j, shift2_j as derived from the (all-reduced) pass 1; limb_bits 0 for a dead feature
 *   limbs [D][4] int64: hi and lo of I1, hi and lo of I2
 *   bad [2]: the caller sets {0, -1}. bad[0] counts the entries of this call that are not finite, whose column is outside [0, D), or (pass 2)
 *            with |x| >= 2^(E_j + 1), the bound the shifts were made for (on a dead feature: any non-zero value); bad[1] is the smallest index
 *            of a bad entry within its call (an unsigned atomic min). A bad entry is left out of every accumulator: nothing wraps silently.
 * Paths. Up to 4 096 features (GDMIX_STATS_LDS_MAX_FEATURES in the environment: a test hook, at most 5 000) the table is private to a
 * workgroup in LDS, flushed with one global atomic per touched slot; above, global 64-bit integer atomics per entry. A wavefront whose
 * entries share one column adds them with shuffles first. The two paths give the same bits.
 * gdmix_re_feature_scale_expand: scale [P] fp64 in the batch's coefficient order from factor [num_features]: factor[unique_global] at the
 * feature slots, 1 at every intercept slot. Built on the device (P is tens of millions); waits for a deferred compaction itself. */
GDMIX_API int gdmix_re_feature_extent(gdmix_re_ctx* ctx, const void* col, int col_width, const float* val, int64_t Z, int64_t num_features,
                                      uint64_t* count, uint32_t* max_abs_bits, int64_t* bad, void* stream);
GDMIX_API int gdmix_re_feature_moments(gdmix_re_ctx* ctx, const void* col, int col_width, const float* val, int64_t Z, int64_t num_features,
                                       const int32_t* limb_bits, const int32_t* shift1, const int32_t* shift2, int64_t* limbs, int64_t* bad,
                                       void* stream);
GDMIX_API int gdmix_re_feature_scale_expand(gdmix_re_ctx* ctx, const gdmix_re_packed* packed, int has_intercept, const double* factor,
                                            int64_t num_features, double* scale, void* stream);

/* ---- (ABI 21) down-sampling: a row subset of a raw batch, chosen by a hash of (seed, uid), before gdmix_re_pack ------------------------
 * Photon-ML's downSamplingRate for the fixed-effect stage (--down_sampling_rate / --down_sampling_seed, gdmix_amd/fe_model.py; not in
 * the reference): the stage trains on a sample of its shard that keeps every positive (logistic loss) and a negative with probability
 * `rate`, kept negatives weighted 1 / rate, so that the objective stays an unbiased estimate of the full one and l2_reg_weight keeps its
 * meaning. csrc/re_downsample.hip; a pass over a gdmix_re_raw_batch (any E) in front of gdmix_re_pack, of which no pack or solve kernel
 * knows. The random-effect stage has no such flag (an entity could lose all its rows); what it has is a cap on every entity's rows, which
 * can never empty one: "(ABI 25) active-data cap" below.
 *
 * Definition. All arithmetic on unsigned 64-bit integers, wrapping.
 *     mix(x):  x += 0x9E3779B97F4A7C15;  x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9;  x = (x ^ (x >> 27)) * 0x94D049BB133111EB;
 *              return x ^ (x >> 31)                    (splitmix64's output function; mix(0) = 0xE220A8397B1DCDAF)
 *     draw(seed, uid) = mix((uint64)uid ^ mix(seed)) >> 32       the sample's int64 uid reinterpreted as unsigned
 *     T = (uint64)(rate * 4294967296.0),  0 < rate <= 1          the product is exact; T may be 0 and is 2^32 at rate 1
 * A row is SAMPLED if draw < T. With negatives_only (the logistic loss) a row with label > 0.5f is always kept, its weight unchanged, and
 * only the other rows are subject to sampling; without it (squared and Poisson loss) every row is. A row that was subject to sampling and
 * kept gets the weight (float)((double)w / rate), w = 1 where the batch has no weight array. Kept rows keep their order.
 * A row's fate is a pure function of (seed, uid): it does not depend on the partitioning, on the order of the rows or on the number of
 * workers, and rows with EQUAL uids share a fate. gdmix_amd/downsample.py is the numpy statement of this definition; the device gives the
 * same bits.
 *     draw(0, 0) = 2802244911   draw(1, 0) = 1581361928   draw(0, 1) = 146079144   draw(20240603, 123456789) = 3653550952
 *     draw(7, -1) = 2846452585  draw(7, -2^63) = 2118445982
 *
 * gdmix_re_downsample_plan: uid [N] int64 on the device. Writes into `workspace` (gdmix_re_downsample_workspace_bytes(E, N) device bytes;
 *   host only, 0 beyond the limits; less is GDMIX_RE_ENOMEM) a keep flag per row, the exclusive scan of the kept rows (int32) and the
 *   exclusive int64 scan of their non-zeros, synchronises `stream` once and fills *counts (host). The caller allocates the output arrays of
 *   exactly counts->kept rows and counts->kept_nnz non-zeros.
 * gdmix_re_downsample_apply: the same raw batch, options and workspace; fills the arrays of *out (out->N = kept, out->Z = kept_nnz):
 *     ent_row_ptr [E+1] = scan[ent_row_ptr_in[e]] (an entity may end with no rows), row_nnz_ptr [N_out+1] from 0, col_global, val [Z_out],
 *     y, offset [N_out], weight [N_out] (always written), and kept_rows [N_out] (optional, NULL: not wanted): the source row of each kept row.
 *   Stream-ordered. The workspace must hold the context's LAST plan, and out->N / out->Z must be its totals: anything else is
 *   GDMIX_RE_EINVAL and nothing is written. The copy of the non-zeros is driven by output position (a lane takes four consecutive ones; a
 *   workgroup finds its tile's rows by bisection of the output row pointers, a lane walks from there); stores are 16 bytes per lane where
 *   the output arrays are 16-byte aligned, and so are the loads of a lane whose four positions lie in one source row at a source position
 *   that is a multiple of four.
 * rate outside (0, 1] or not finite: GDMIX_RE_EINVAL. 2^31 rows or more: GDMIX_RE_ERANGE. All offsets are 64-bit. */
typedef struct {
  double   rate;
  uint64_t seed;
  int32_t  negatives_only;
  int32_t  reserved;
} gdmix_re_downsample_opts;
typedef struct {          /* host */
  int64_t rows;           /* N of the input                                                     */
  int64_t kept;           /* N_out                                                              */
  int64_t kept_nnz;       /* Z_out                                                              */
  int64_t positives;      /* input rows with label > 0.5f                                       */
  int64_t negatives_kept; /* kept rows with label <= 0.5f                                       */
} gdmix_re_downsample_counts;
typedef struct {          /* device pointers of the caller's arrays */
  int64_t  N, Z;          /* counts->kept, counts->kept_nnz */
  int64_t* ent_row_ptr;
  int64_t* row_nnz_ptr;
  int64_t* col_global;
  float*   val;
  float*   y;
  float*   offset;
  float*   weight;
} gdmix_re_downsample_out;
GDMIX_API size_t gdmix_re_downsample_workspace_bytes(int64_t E, int64_t N);
GDMIX_API int gdmix_re_downsample_plan(gdmix_re_ctx* ctx, const gdmix_re_raw_batch* raw_dev, const int64_t* uid_dev, const gdmix_re_downsample_opts* opts,
                                       void* workspace, size_t workspace_bytes, gdmix_re_downsample_counts* counts, void* stream);
GDMIX_API int gdmix_re_downsample_apply(gdmix_re_ctx* ctx, const gdmix_re_raw_batch* raw_dev, const gdmix_re_downsample_opts* opts, void* workspace,
                                        size_t workspace_bytes, const gdmix_re_downsample_out* out_dev, int32_t* kept_rows, void* stream);

/* ---- (ABI 22) feature selection: per entity, the features most correlated with the label, before gdmix_re_pack ----------------------------
 * Photon-ML's numFeaturesToSamplesRatioUpperBound for a random-effect stage (--features_to_samples_ratio=R, gdmix_amd/model.py; not in the
 * reference): before an entity is trained it keeps only the ceil(R n_e) features whose Pearson correlation with the label is largest in
 * magnitude. csrc/re_select.hip; a pass between two packs (pack -> plan on the packed CSC -> apply on the raw non-zeros -> pack again), of
 * which no pack or solve kernel knows: a dropped feature is from there on a feature the entity's data does not contain.
 *
 * Definition, for one entity with n samples, labels y_i (fp32 widened to fp64) and cells x_ij: a cell is the fp64 sum of the entity's
 * duplicates of (sample i, feature j), in CSC order, and zero where there is none. Unweighted; offsets are ignored; the intercept is not a
 * feature (it is kept apart and takes no slot — Photon-ML counts it as one of the kept features).
 *     Sy = sum y_i, Syy = sum y_i^2 over the samples in order; per feature, over its cells in sample order: Sx, Sxx, Sxy
 *     A = n Sxy - Sx Sy,  Bx = n Sxx - Sx^2,  By = n Syy - Sy^2
 *     q = A^2 / Bx  if Bx > 2^-30 n Sxx and By > 2^-30 n Syy, else 0   (a constant column, constant labels, n = 1)
 *     key = (float)q  (a NaN, from infinite sums, is 0.0f);  r^2 = q / By, and By is common to an entity's features, so it is dropped
 *     rank by key descending, then by feature index ascending; keep the first k_e = min(d_e, (int64)ceil(R (double)n_e))
 * A feature that occurs in one sample only has q = (n y_i - Sy)^2 / (n - 1) whatever its value: exact ties at the boundary are the rule,
 * which is why the rank is taken on the fp32 key with the index as the tie-break. A column's sums are plain fp64 sums by one lane, one term
 * after another; Sy and Syy are 64 partial sums over the samples i = l, l + 64, ... added by a butterfly, a shape that depends on n alone:
 * a key is a function of the entity's own data alone and has the same bits whichever ranking path takes the entity, wherever the entity
 * sits in the batch and however partitions are grouped. gdmix_amd/feature_selection.py is the numpy statement.
 *
 * Error of a key against the exact q (u = 2^-53; inputs are fp32, so x^2 and x y are exact in fp64 unless a cell is a sum of duplicates):
 * a sum of c <= n terms carries at most (c + 1) u sum|terms|; with M = n sum|x y| + |Sx| |Sy| the computed A is within
 * delta = (n + 4) 2^-52 M of the exact one (twice the first-order bound (n + 3) u M, for columns whose values share a sign, as sum|x| = |Sx|
 * there), so A^2 is within 2 M delta + delta^2, divided by Bx. The computed Bx is within (n + 4) 2^-52 (n Sxx + Sx^2) of the exact one: where
 * that is at most 2^-24 Bx its share stays inside the 2^-22 q that also holds the fp32 rounding (2^-24 q). So where the exact
 * Bx >= 2^-20 n Sxx and By >= 2^-20 n Syy:   |key - q| <= 2^-22 q + (2 M delta + delta^2) / Bx.
 * Where the exact Bx or By is 0 the computed one is at most (n + 4) 2^-51 n Sxx < 2^-30 n Sxx (n < 2^20) and the key is exactly 0.0f.
 *
 * gdmix_re_select_plan: `packed` is the pack of the raw batch (gdmix_re_pack, has_intercept either way). Column moments come from csc_val,
 *   csc_row and y, a wavefront per entity and a lane per column. Entities of at most 1024 features rank by counting,
 *   #{key_j > key_i or (== and j < i)} < k_e (up to 64 features across the lanes' registers, above that against the keys in LDS); larger ones by a segmented
 *   radix sort of (~key bits, local index). Both give the same mask. Writes the plan into `workspace`
 *   (gdmix_re_select_workspace_bytes(E, N, Z) device bytes; host only, 0 beyond the limits; less is GDMIX_RE_ENOMEM), keep_out [D] uint8 and,
 *   unless NULL, keys_out [D] float, both in the order of unique_global; synchronises `stream` once and fills *counts (host). rocPRIM's
 *   temporary storage is the context's own (grow-only).
 * gdmix_re_select_apply: the raw batch that was packed, the pack, the workspace; fills row_nnz_ptr [N+1], col_global and val [kept_nnz] of
 *   *out. A non-zero z is kept iff keep[ent_feat_ptr[e] + csr_col[z]]; kept non-zeros keep their order. Rows, y, offset and weight are not
 *   touched: the caller's raw batch keeps them. Stream-ordered. The workspace must hold the context's LAST plan, and out->Z must be its
 *   kept_nnz: anything else is GDMIX_RE_EINVAL and nothing is written.
 * R not finite or <= 0: GDMIX_RE_EINVAL. 2^31 entities, samples or non-zeros or more: GDMIX_RE_ERANGE. All offsets are 64-bit. */
typedef struct {          /* host */
  int64_t entities;       /* E                                                                  */
  int64_t affected;       /* entities with k_e < d_e                                            */
  int64_t features;       /* D, the sum of d_e                                                  */
  int64_t kept;           /* the sum of k_e                                                     */
  int64_t dropped;        /* features - kept                                                    */
  int64_t kept_nnz;       /* non-zeros of the kept features                                     */
} gdmix_re_select_counts;
typedef struct {          /* device pointers of the caller's arrays */
  int64_t  Z;             /* counts->kept_nnz */
  int64_t* row_nnz_ptr;   /* [N+1] */
  int64_t* col_global;    /* [Z]   */
  float*   val;           /* [Z]   */
} gdmix_re_select_out;
GDMIX_API size_t gdmix_re_select_workspace_bytes(int64_t E, int64_t N, int64_t Z);
GDMIX_API int gdmix_re_select_plan(gdmix_re_ctx* ctx, const gdmix_re_packed* packed, double R, void* workspace, size_t workspace_bytes, float* keys_out,
                                   uint8_t* keep_out, gdmix_re_select_counts* counts, void* stream);
GDMIX_API int gdmix_re_select_apply(gdmix_re_ctx* ctx, const gdmix_re_raw_batch* raw_dev, const gdmix_re_packed* packed, void* workspace,
                                    const gdmix_re_select_out* out_dev, void* stream);
/* Testing knob: entities of more than `small_max` features take the sort path (0 => every entity that has a feature). 0 .. 1024, default 1024. */
GDMIX_API int gdmix_re_set_select_small_max(gdmix_re_ctx* ctx, int small_max);

/* ---- (ABI 25) active-data cap: at most K rows of every entity, a uniform sample with rescaled weights, before gdmix_re_pack --------------
 * Photon-ML's activeDataUpperBound for a random-effect stage (--active_data_upper_bound=K / --active_data_seed, gdmix_amd/model.py; not in
 * the reference): an entity of more than K samples trains on a uniform sample of K of them, each weighted n_e / K, so that the objective
 * stays an unbiased estimate of the full one and l2_reg_weight keeps its meaning. The head of a skewed population is bounded; no entity
 * can lose all its rows. csrc/re_cap.hip; a pass over a gdmix_re_raw_batch in front of gdmix_re_pack, of which no pack or solve kernel
 * knows. Only the batch the solver sees is cut: scores and metrics are taken over every row.
 *
 * Definition, for one entity with rows i = 0 .. n_e - 1 in batch order and row uids u_i; mix is the function of the down-sampling section.
 *     key(seed, uid) = mix((uint64)uid ^ mix(seed))                all 64 bits (down-sampling's draw is key >> 32)
 *     n_e <= K :  every row is kept, its weight unchanged (1 where the batch has no weight array)
 *     n_e >  K :  kept = the K rows smallest by (key, i); kept rows keep their order;
 *                 weight of a kept row = (float)(((double)w * (double)n_e) / (double)K)
 * Every operation is a single IEEE fp64 step followed by one rounding to fp32: gdmix_amd/active_data.py, the numpy statement of this
 * definition, and the device give the same bits.
 *   - With distinct uids the kept set is a function of (seed, the entity's set of uids, K) alone: it does not depend on the order of the
 *     rows, on where the entity sits or on how partitions are grouped.
 *   - The kept set at K is a subset of the kept set at K' > K.
 *   - Rows with EQUAL uids tie on the key and are admitted in row order: the only place where the order matters.
 *     key(0, 0) = 0xa706dd2f4d197e6f   key(1, 0) = 0x5e41ab087439611e   key(0, 1) = 0x08b4fda8c892b50e
 *     key(20240603, 123456789) = 0xd9c4c3685399dfb6   key(7, -1) = 0xa9a96b699dc41760   key(7, -2^63) = 0x7e44eb9e75b86b14
 *     seed 5, one entity with uids 100 .. 111: K = 4 keeps rows {0, 5, 8, 10}, K = 5 keeps rows {0, 5, 8, 9, 10}.
 * The stage's objective, (1/n) ( sum w l + (l2/2) |theta_reg|^2 ), is divided by the number of rows the solver sees, which is K for a
 * capped entity and not n_e. That constant multiplies the whole objective and does not move the minimiser of sum w l + (l2/2) |theta|^2
 * (fval and the gradient norm the stopping tests see are scaled by n_e / K against an uncapped entity's).
 *
 * gdmix_re_cap_plan: uid [N] int64 on the device. Lists the capped entities (n_e > K; in any order, which no output depends on); those of at
 *   most 128 rows (gdmix_re_set_cap_small_max: up to 1024) take a wavefront each, hash their keys once into LDS and keep row i iff #{j : (key_j, j) < (key_i, i)} < K; larger ones
 *   take a workgroup each and find the K-th smallest key by an exact radix select, most significant byte first, with a 256-bin histogram
 *   in LDS per pass (at most eight passes over the entity's uids, the key hashed again from the uid each time: no key array in HBM), then
 *   keep key < tau and, of key == tau, the first rows in row order until K is reached, by an ordered count across the workgroup. Both give
 *   the same flags; all counts are integers. Then the exclusive scans of down-sampling. Writes into `workspace`
 *   (gdmix_re_cap_workspace_bytes(E, N) device bytes; host only, 0 beyond the limits; less is GDMIX_RE_ENOMEM), synchronises `stream` once
 *   and fills *counts (host). The caller allocates the output arrays of exactly counts->kept rows and counts->kept_nnz non-zeros.
 * gdmix_re_cap_apply: the same raw batch, options and workspace; fills the arrays of *out as gdmix_re_downsample_apply does (weight is
 *   always written) and kept_rows [N_out] (optional). Stream-ordered. The workspace must hold the context's LAST plan, and out->N / out->Z
 *   must be its totals: anything else is GDMIX_RE_EINVAL and nothing is written.
 * upper_bound < 1: GDMIX_RE_EINVAL. 2^31 rows or entities or more: GDMIX_RE_ERANGE. All offsets are 64-bit. */
typedef struct {
  int64_t  upper_bound;   /* K >= 1 */
  uint64_t seed;
} gdmix_re_cap_opts;
typedef struct {          /* host */
  int64_t entities;       /* E                                                                  */
  int64_t capped;         /* entities with n_e > K                                              */
  int64_t rows;           /* N of the input                                                     */
  int64_t kept;           /* N_out                                                              */
  int64_t kept_nnz;       /* Z_out                                                              */
  int64_t largest;        /* the largest n_e before the cap                                     */
} gdmix_re_cap_counts;
GDMIX_API size_t gdmix_re_cap_workspace_bytes(int64_t E, int64_t N);
GDMIX_API int gdmix_re_cap_plan(gdmix_re_ctx* ctx, const gdmix_re_raw_batch* raw_dev, const int64_t* uid_dev, const gdmix_re_cap_opts* opts, void* workspace,
                                size_t workspace_bytes, gdmix_re_cap_counts* counts, void* stream);
GDMIX_API int gdmix_re_cap_apply(gdmix_re_ctx* ctx, const gdmix_re_raw_batch* raw_dev, const gdmix_re_cap_opts* opts, void* workspace, size_t workspace_bytes,
                                 const gdmix_re_downsample_out* out_dev, int32_t* kept_rows, void* stream);
/* Where the two paths part: capped entities of more than `small_max` rows take the radix-select path (0 => every capped entity). 0 .. 1024;
 * the default, 128, is where counting stops paying on a C5-shaped batch (profiles/active_data.txt). The flags do not depend on it. */
GDMIX_API int gdmix_re_set_cap_small_max(gdmix_re_ctx* ctx, int small_max);

/* ---- (ABI 27) row grouping: a sample-major data set grouped by entity on the device, and per-row values moved between the two orders ----
 * What the partition job does between two stages of the coordinate chain, for coordinates that stay in HBM (gdmix_amd/descent.py, which
 * also states all of this in numpy: group_rows_host, offsets_combine_host). csrc/re_group.hip. The entry points are additions: no struct
 * and no entry point of ABI 27 changes, so the version number stays.
 *
 * Definition. Input: N rows of a CSR bag (row_nnz_ptr [N + 1], col_global [Z], val [Z]) and entity_index [N] int32; a row whose index is
 * outside [0, E) (-1 by convention) belongs to no entity and is left out. With keep = {i : 0 <= entity_index[i] < E} in ascending order:
 *     row_of      = keep reordered by a STABLE sort on entity_index: entities ascending, the rows of one entity in input order
 *                   ( keep[np.argsort(entity_index[keep], kind="stable")] )                                  [N'] grouped position -> source row
 *     present     = the distinct values of entity_index[keep], ascending                                     [E'] no empty entity
 *     ent_row_ptr = where each present entity's rows start in row_of, and N'                                  [E' + 1]
 *     row_nnz_ptr, col_global, val = the rows row_of[0], row_of[1], ... of the bag, one after another        [N' + 1], [Z'], [Z']
 * Every intermediate is an integer (a stable radix sort of (entity, row) pairs, integer prefix sums): the same bits on every run and for
 * every launch geometry.
 *
 * gdmix_re_group_rows: all array arguments are device pointers. The caller sizes the outputs by their upper bounds (below); the first
 *   N' / E' / Z' entries are the result, what lies behind them is unspecified. Work is queued on `stream`, which is synchronised once, in
 *   the middle, to read the counts back (the copy of the non-zeros is launched for exactly Z' positions); it returns with the copy queued.
 *   The non-zeros move by OUTPUT position, 16 bytes per lane and store (csrc/re_rowsubset.hpp, ds_nnz_kernel). Row pointers that do not
 *   describe Z non-zeros (a row outside [0, Z], or decreasing) are GDMIX_RE_EINVAL and no non-zero is copied. 2^31 rows or entities or
 *   more: GDMIX_RE_ERANGE. `workspace`: gdmix_re_group_workspace_bytes(N, E) device bytes (host only; 0 beyond the limits).
 *
 * Row values. row_of is the array above (or any int32 map into the source); an entry outside the source's rows reads as 0 / is skipped.
 *   gdmix_re_rows_gather_f32:   dst[i] = src[row_of[i]]                       i < n_dst            (labels, weights -> grouped order)
 *   gdmix_re_rows_scatter_f32:  dst[:] = 0 unless keep_rest;  dst[row_of[i]] = src[i]    i < n_src (a coordinate's scores -> sample order;
 *                                                                                                   rows that were left out keep 0, or, with
 *                                                                                                   keep_rest != 0, what dst held)
 *   gdmix_re_offsets_combine:   r = row_of ? row_of[i] : i
 *                               acc = base ? base[r] : +0.0f
 *                               for k = 0 .. K - 1, k != skip:  acc = acc + parts[k][r]            (fp32, in this order)
 *                               dst[i] = acc                                  i < n_dst
 *     Plain fp32 additions from left to right: no multiply (nothing to contract into an fma) and no reordering. This order is what makes
 *     the first pass of a resident descent the file chain: there a stage's offset is the previous stage's score, an Avro `float`, and
 *     float(double(a) + double(b)) is the fp32 sum of two floats. `parts` is a HOST array of K <= GDMIX_RE_COMBINE_MAX device pointers to
 *     [n_src] floats; skip = -1 (or any value outside [0, K)) leaves nothing out. Stream-ordered, no synchronisation. */
#define GDMIX_RE_COMBINE_MAX 8
typedef struct {           /* device arrays the caller allocates, by upper bound                                  */
  int32_t* row_of;         /* [N]                 the first N' entries                                            */
  int32_t* present;        /* [min(N, E)]         the first E'                                                    */
  int64_t* ent_row_ptr;    /* [min(N, E) + 1]     the first E' + 1                                                */
  int64_t* row_nnz_ptr;    /* [N + 1]             the first N' + 1                                                */
  int64_t* col_global;     /* [Z]                 the first Z'                                                    */
  float*   val;            /* [Z]                 the first Z'                                                    */
} gdmix_re_group_out;
typedef struct {           /* host */
  int64_t rows;            /* N of the input                                                                      */
  int64_t grouped;         /* N'                                                                                  */
  int64_t grouped_nnz;     /* Z'                                                                                  */
  int64_t entities;        /* E'                                                                                  */
  int64_t left_out;        /* N - N'                                                                              */
} gdmix_re_group_counts;
GDMIX_API size_t gdmix_re_group_workspace_bytes(int64_t N, int64_t E);
GDMIX_API int gdmix_re_group_rows(gdmix_re_ctx* ctx, int64_t N, int64_t Z, int64_t E, const int64_t* row_nnz_ptr, const int64_t* col_global, const float* val,
                                  const int32_t* entity_index, void* workspace, size_t workspace_bytes, const gdmix_re_group_out* out_dev,
                                  gdmix_re_group_counts* counts, void* stream);
GDMIX_API int gdmix_re_rows_gather_f32(gdmix_re_ctx* ctx, float* dst, int64_t n_dst, const float* src, int64_t n_src, const int32_t* row_of, void* stream);
GDMIX_API int gdmix_re_rows_scatter_f32(gdmix_re_ctx* ctx, float* dst, int64_t n_dst, const float* src, int64_t n_src, const int32_t* row_of, int keep_rest,
                                        void* stream);
GDMIX_API int gdmix_re_offsets_combine(gdmix_re_ctx* ctx, float* dst, int64_t n_dst, const float* base, const float* const* parts, int K, int skip,
                                       const int32_t* row_of, int64_t n_src, void* stream);

/* ---- B4: the upstream Spark partitioner's hash, bit-exact (host functions) ------------------------
 * hashCode over UTF-16 code units in wrapping int32; Math.abs(Int.MinValue) stays negative; Scala %
 * keeps the dividend's sign (PartitionUtils.scala:31-37). */
GDMIX_API int32_t gdmix_java_string_hash(const uint16_t* utf16, int64_t len);
GDMIX_API int32_t gdmix_java_partition_id(const uint16_t* utf16, int64_t len, int32_t num_partitions);
/* Batched device form for decimal int64 entity ids (id.toString of a Long): out[i] = partition id. */
GDMIX_API int gdmix_java_partition_ids_i64(gdmix_re_ctx* ctx, const int64_t* ids_dev, int64_t count,
                                 int32_t num_partitions, int32_t* out_dev, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* GDMIX_RE_H_ */
