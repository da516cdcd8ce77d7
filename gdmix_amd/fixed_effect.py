"""Fixed-effect linear / logistic regression on one MI355X (single-worker form).

The reference trains the fixed effect by scipy's fmin_l_bfgs_b over an objective TensorFlow evaluates on the
worker's shard (gdmix-trainer/src/gdmix/models/custom/fixed_effect_lr_lbfgs_model.py:309-392,635-643):

    f(theta) = sum_i w_i * loss(y_i, x_i . w + b + offset_i) + (l2 / 2) * |theta_reg|^2        (not divided by n)
    loss     = sigmoid cross entropy (logistic_regression) or (y - z)^2 (linear_regression)
    theta    = [w (num_features), b]: the intercept is the LAST coefficient (:340-342)
    theta_reg = theta if regularize_bias or no intercept, else theta[:-1] (:367-369)

That is the random-effect objective of one "entity" holding the whole shard, without the 1/n and with an optional
squared loss — two switches of the same device solver (gdmix_re_opts.sum_loss / .loss, include/gdmix_re.h): the
shard is packed as a one-entity batch and solved by the device-wide team kernel (csrc/re_solve_team.hpp), X
streaming from HBM twice per evaluation (CSR for the logits, the CSC copy for the gradient). This module maps
between the reference's coefficient layout (global feature index, intercept last) and the solver's (features
present in the shard, intercept first).

Two device paths, same arithmetic rules:
  * fit()           the whole solve inside the device-wide team kernel (one launch; single worker only);
  * fit_stepping()  include/gdmix_fe.h: streaming kernels for the two passes over the shard and the L-BFGS step as
                    separate launches, with ONE all-reduce of [gradient, value] across workers in between (the
                    reference does two, :375-381) — RCCL through torch.distributed on the GPU box. Every worker holds
                    its shard and runs the replicated step on the reduced buffer, like the reference's workers run scipy.
"""
import ctypes as C
import os

import numpy as np

from .batch import RawBatch
from .solver import REDeviceSolver, SolverOptions

LOGISTIC_REGRESSION = "logistic_regression"
LINEAR_REGRESSION = "linear_regression"
POISSON_REGRESSION = "poisson_regression"      # loss exp(z) - y z on count labels (include/gdmix_fe.h, "poisson")
LOSS_OF_MODEL_TYPE = {LOGISTIC_REGRESSION: "logistic", LINEAR_REGRESSION: "squared", POISSON_REGRESSION: "poisson"}
LBFGS, TRON = "LBFGS", "TRON"                  # --optimizer (Photon-ML's OptimizerType); include/gdmix_fe.h, "(ABI 24) TRON"
OPTIMIZER_CODE = {LBFGS: 0, TRON: 1}           # GDMIX_FE_OPT_LBFGS, GDMIX_FE_OPT_TRON


def check_optimizer(value):
    """'tron' -> 'TRON': one of Photon-ML's names, in any case."""
    name = str(value).strip().upper()
    if name not in OPTIMIZER_CODE:
        raise ValueError(f"--optimizer={value!r}: one of {', '.join(OPTIMIZER_CODE)}")
    return name


def shard_as_batch(row_nnz_ptr, col_global, val, y, offset=None, weight=None, has_intercept=True, binary_labels=True,
                   dummy=None):
    """The shard as a one-entity RawBatch.

    dummy=True: an intercept-only model (no feature bag configured) gets one dummy zero feature per sample, as the
    random-effect path does (job_consumers.py:213-218). dummy=None infers it from "no non-zeros at all", which is
    only right for callers that have no notion of a feature bag; the model class passes `feature_bag is None`.

    A bagged worker whose shard holds no non-zero (no samples at all — shard_input_files hands out [] when there are
    fewer files than workers, util/distribution_utils.py:41-44 — or only empty rows) still owns the full
    coefficient space: it gets one extra sample of weight 0 carrying a 0.0 at feature 0, which adds exactly 0 to the
    value and to every gradient entry, so it joins the all-reduce with a full-size buffer of zeros like the
    reference's empty worker does."""
    row_nnz_ptr = np.asarray(row_nnz_ptr, np.int64)
    n = row_nnz_ptr.size - 1
    col = np.asarray(col_global, np.int64)
    v = np.asarray(val, np.float32)
    y = np.asarray(y, np.float32)
    offset = np.zeros(n, np.float32) if offset is None else np.asarray(offset, np.float32)
    weight = None if weight is None else np.asarray(weight, np.float32)
    if dummy is None:
        dummy = col.size == 0
    if dummy:
        if not has_intercept:
            raise ValueError("a model without features needs an intercept")
        row_nnz_ptr = np.arange(n + 1, dtype=np.int64)
        col = np.zeros(n, np.int64)
        v = np.zeros(n, np.float32)
    if col.size == 0:   # bagged shard without a single non-zero (or a dummy shard without samples): the weight-0 sample
        row_nnz_ptr = np.concatenate([row_nnz_ptr, [row_nnz_ptr[-1] + 1]]).astype(np.int64)
        col = np.zeros(1, np.int64)
        v = np.zeros(1, np.float32)
        y = np.concatenate([y, np.zeros(1, np.float32)])
        offset = np.concatenate([offset, np.zeros(1, np.float32)])
        weight = np.concatenate([np.ones(n, np.float32) if weight is None else weight, np.zeros(1, np.float32)])
        n += 1
    b = RawBatch(ent_row_ptr=np.array([0, n], np.int64), row_nnz_ptr=row_nnz_ptr, col_global=col, val=v,
                 y=y, offset=offset, weight=weight, uid=np.arange(n, dtype=np.int64),
                 entity_ids=["fixed_effect"], has_label=True, binary_labels=binary_labels)
    return b, dummy


def to_local(theta_global, unique_global, num_features, has_intercept, dummy):
    """reference layout [w (num_features), b] -> solver layout [b, w of the features present]."""
    t = np.asarray(theta_global, np.float64)
    ic = 1 if has_intercept else 0
    out = np.zeros(unique_global.size + ic)
    if has_intercept:
        out[0] = t[num_features]
    if not dummy:
        out[ic:] = t[unique_global]
    return out


def to_global(theta_local, unique_global, num_features, has_intercept, dummy):
    ic = 1 if has_intercept else 0
    out = np.zeros(num_features + ic)
    if not dummy:
        out[unique_global] = theta_local[ic:]
    if has_intercept:
        out[num_features] = theta_local[0]
    return out


class FixedEffectDeviceSolver:
    """fit() = FixedEffectLRModelLBFGS's training step for one worker, on the device."""

    def __init__(self, device=0, solver=None):
        self.solver = solver or REDeviceSolver(device)

    def score(self, row_nnz_ptr, col_global, val, offset, theta, num_features, has_intercept=True):
        """-> (score, per-coordinate score) of every sample under theta (intercept last); see device_score."""
        return device_score(self.solver, row_nnz_ptr, col_global, val, offset, theta, num_features, has_intercept)

    def upload(self, row_nnz_ptr, col_global, val, offset, num_features, label=None):
        """The sample-major arrays of a raw shard on the device, once, for any number of score_device / score_models calls."""
        return DeviceShard(self.solver, row_nnz_ptr, col_global, val, offset, num_features, label)

    def score_device(self, shard, theta, has_intercept=True):
        """-> (score, per-coordinate score) of an uploaded shard as float32 DEVICE tensors (gdmix_fe_score); theta: numpy or device."""
        return device_score_shard(self.solver, shard, theta, has_intercept)

    def score_models(self, shard, thetas, has_intercept=True, per_coord=True, slot_major=True):
        """gdmix_fe_score_models: K coefficient vectors (numpy or float64 device tensors, intercept last) over an uploaded shard in one
        pass over its non-zeros -> (score [K, n], per_coord [K, n] | None) float32 device tensors; row k is bit for bit score_device's
        for thetas[k]. slot_major: each pass first copies its models into one [coefficient][model] array (a device temporary)."""
        return device_score_models(self.solver, shard, thetas, has_intercept, per_coord, slot_major)

    def file_scores(self, shard, per_coord):
        """The predictionScore the stage's score file holds for these per-coordinate scores — float32(float64(per_coord) + float64(offset)),
        as fe_model._score_and_write forms it on the host — without leaving the device (what the stage metric is computed on)."""
        t = self.solver.torch
        return (per_coord.to(t.float64) + shard.of.to(t.float64)).to(t.float32)

    @staticmethod
    def to_host(x):
        return x.cpu().numpy()

    def new_evaluator(self, metric=None):
        """An accumulator of the exact stage metric for scores that stay on the device (metrics.DeviceEvaluator; metrics.PoissonEvaluator
        for metric "poisson_loss")."""
        from . import metrics
        return metrics.PoissonEvaluator(self.solver) if metric == metrics.POISSON_LOSS else metrics.DeviceEvaluator(self.solver)

    def models_per_chunk(self, K, P, n_eval):
        """How many of K models are scored at once (sweep.models_per_chunk): a model is its coefficients and two rows of the output,
        score and per-coordinate score."""
        from .sweep import models_per_chunk
        return models_per_chunk(self.solver.torch, self.solver.device, K, 8 * P + 8 * n_eval + 1)

    def fit(self, row_nnz_ptr, col_global, val, y, num_features, offset=None, weight=None, has_intercept=True, l2=1.0,
            regularize_bias=True, model_type=LOGISTIC_REGRESSION, theta0=None, max_iter=100, m=10, tolerance=1e-12, dummy=None):
        """-> (theta [num_features + has_intercept], intercept last; info dict with f, nit, nfev, status, gnorm)."""
        opts = fit_options(has_intercept, l2, regularize_bias, model_type, max_iter, m, tolerance)
        batch, dummy = shard_as_batch(row_nnz_ptr, col_global, val, y, offset, weight, has_intercept, binary_labels=opts.loss_name() == "logistic", dummy=dummy)
        if not dummy and batch.col_global.size and (batch.col_global.min() < 0 or batch.col_global.max() >= num_features):
            raise ValueError(f"feature index outside [0, {num_features})")
        packed = self.solver.pack(batch, has_intercept=has_intercept)
        uniq = packed.unique_global().cpu().numpy()
        t0 = None if theta0 is None else to_local(theta0, uniq, num_features, has_intercept, dummy)
        res = self.solver.solve(packed, opts, theta0=t0).to_host()
        theta = to_global(res["theta"], uniq, num_features, has_intercept, dummy)
        info = {k: res[k][0] for k in ("fval", "nit", "nfev", "status", "gnorm")}
        if not 0 <= int(info["status"]) <= 4:
            raise RuntimeError(f"the fixed-effect solve did not finish (device status {int(info['status'])}: 9 = a device barrier timed out)")
        return theta, info

    def fit_stepping(self, row_nnz_ptr, col_global, val, y, num_features, offset=None, weight=None, has_intercept=True, l2=1.0,
                     regularize_bias=True, model_type=LOGISTIC_REGRESSION, theta0=None, max_iter=100, m=10, tolerance=1e-12,
                     group=None, return_problem=False, dummy=None, variance_mode=None, threshold=0.0, prior=None, feature_scale=None,
                     down_sampling=None, l1=0.0, optimizer=LBFGS, bounds=None):
        """Same contract as fit(), through include/gdmix_fe.h. With torch.distributed initialised (or `group` given) every
        worker calls this with its own shard; the coefficients returned are identical on all workers. dummy: True for a
        model without a feature bag (intercept only), False for a bagged model — also when this worker's shard happens to
        hold no non-zero, so that its all-reduce buffer has the same num_features + 2 entries as everyone else's.
        prior = (mean, variance), each in theta0's layout: incremental training (include/gdmix_fe.h, "incremental training") — the L2
        term is centred on `mean` and weighted by 1 / variance (1 where a variance is not finite or <= 0), the fit starts at `mean`
        (theta0 must be None), and the variances returned are the posterior's. Every worker passes the same prior.
        feature_scale = s [num_features]: feature normalisation (include/gdmix_re.h, "feature normalisation") — the penalty is
        (l2/2) sum (theta_j / s_j)^2, i.e. a prior of mean 0 and variance s^2 with s = 1 for the intercept; theta0, in theta units, is
        honoured; not together with `prior`. Every worker passes the same factors.
        down_sampling = (rate, seed, uid [n] int64): the fit is that of a sample of the shard, drawn on the device (include/gdmix_re.h,
        "down-sampling"; gdmix_amd/downsample.py states it): a row is kept when draw(seed, uid) < rate * 2^32 and then weighs w / rate; with
        the logistic loss every positive is kept as it is. Variances are those of the sampled, re-weighted objective; info["down_sampling"]
        holds the counts. Every worker passes the same rate and seed. Rate 1.0 is the plain fit.
        l1 > 0: the objective gains l1 |theta_R|_1 and the step is OWL-QN's (include/gdmix_fe.h, "(ABI 23) L1 / elastic net"); theta0 is its
        start point; not together with `prior` or `feature_scale`. Coefficients outside the support are exactly 0.0; info["nnz"] counts
        the others. l1 = 0 is the plain fit: set_l1 is never called.
        optimizer="TRON": the smooth objective is minimised by trust-region Newton on the device (include/gdmix_fe.h, "(ABI 24) TRON"); theta0
        is its start point; not together with l1 > 0, `prior` or `feature_scale`. info["nhv"] counts the Hessian-vector products (0 under
        "LBFGS", the plain fit: set_optimizer is never called), info["optimizer"] names the optimiser.
        bounds = (lower, upper), numpy arrays of num_features + has_intercept entries, intercept last and infinite: the smooth objective is
        minimised subject to lower <= theta <= upper by projected L-BFGS on the device (include/gdmix_fe.h, "(ABI 26) box constraints");
        theta0 is clamped into the box; not together with l1 > 0, TRON, `prior` or `feature_scale`. The coefficients returned lie in the box, a
        coefficient at a bound is the bound's double, info["at_bound"] counts those. Every worker passes the same bounds. None is the plain
        fit: set_bounds is never called."""
        optimizer = check_optimizer(optimizer)
        l1 = float(l1)
        if not (np.isfinite(l1) and l1 >= 0.0):
            raise ValueError(f"l1 must be finite and >= 0, not {l1}")
        if l1 > 0.0 and (prior is not None or feature_scale is not None):
            raise ValueError("the L1 term does not compose with a prior model or with feature normalisation")
        if optimizer == TRON and (l1 > 0.0 or prior is not None or feature_scale is not None):
            raise ValueError("TRON minimises the smooth objective in theta units: it does not run with an L1 term, a prior model or feature normalisation")
        if bounds is not None:
            if l1 > 0.0 or optimizer == TRON or prior is not None or feature_scale is not None:
                raise ValueError("bounds constrain the smooth objective in theta units under projected L-BFGS: they do not run with an L1 term, TRON, "
                                 "a prior model or feature normalisation")
            bounds = check_bounds(bounds, int(num_features) + (1 if has_intercept else 0), has_intercept)
        opts = fit_options(has_intercept, l2, regularize_bias, model_type, max_iter, m, tolerance)
        fit = _SteppingFit(self.solver, opts, row_nnz_ptr, col_global, val, y, num_features, offset, weight, theta0, group, dummy, variance_mode,
                           prior=prior, feature_scale=feature_scale, down_sampling=down_sampling)
        if l1 > 0.0 or optimizer == TRON or bounds is not None:
            t0 = fit.prob.theta0
            if l1 > 0.0:
                fit.prob.set_l1(l1)      # (leaves the problem at zeros)
            elif bounds is not None:
                fit.prob.set_bounds(*fit.device_bounds(bounds))      # (leaves the problem at the clamped zeros)
            else:
                fit.prob.set_optimizer(optimizer)
            if t0 is not None:
                fit.prob.restart(opts, t0)
        theta, info = fit.stage_result(*fit.run(), l2, threshold)
        info["l1"] = l1
        info["optimizer"] = optimizer
        info["nnz"] = int(np.count_nonzero(theta))
        if bounds is not None:
            info["at_bound"] = count_at_bound(theta, bounds)
        if return_problem:
            return theta, info, fit.prob
        fit.prob.close()
        return theta, info

    def fit_sweep(self, row_nnz_ptr, col_global, val, y, num_features, l2_grid, select, offset=None, weight=None, has_intercept=True,
                  regularize_bias=True, model_type=LOGISTIC_REGRESSION, max_iter=100, m=10, tolerance=1e-12, dummy=None, variance_mode=None,
                  threshold=0.0, down_sampling=None, optimizer=LBFGS, bounds=None):
        """One worker's fit for every weight of l2_grid on ONE problem: the shard is packed and gdmix_fe_create runs once; per weight, in the
        order given, gdmix_fe_restart (cold: zeros) + the same loop and status check as fit_stepping — by the restart's contract the bits
        of a fresh fit_stepping at that weight. select(thetas) — the K coefficient vectors as fit_stepping would have returned them — names
        the winner; -> (theta, info, best) of the winner as fit_stepping returns them, its variances (at its weight, for it alone) included.
        down_sampling: as fit_stepping takes it; the shard is sampled once, in front of the one pack. optimizer: as fit_stepping takes it;
        the restarts keep it. bounds: as fit_stepping takes them; the restarts keep them, every model of the sweep lies in the box."""
        import dataclasses
        optimizer = check_optimizer(optimizer)
        if bounds is not None:
            if optimizer == TRON:
                raise ValueError("bounds do not run with TRON, which minimises without constraints")
            bounds = check_bounds(bounds, int(num_features) + (1 if has_intercept else 0), has_intercept)
        if _world_size(None) > 1:
            raise ValueError("a sweep over l2_reg_weight runs on one worker")
        opts = fit_options(has_intercept, float(l2_grid[0]), regularize_bias, model_type, max_iter, m, tolerance)
        fit = _SteppingFit(self.solver, opts, row_nnz_ptr, col_global, val, y, num_features, offset, weight, None, None, dummy, variance_mode,
                           down_sampling=down_sampling)
        try:
            if optimizer == TRON:
                fit.prob.set_optimizer(optimizer)
            if bounds is not None:
                fit.prob.set_bounds(*fit.device_bounds(bounds))
            fits = []
            for w in l2_grid:
                fit.prob.restart(dataclasses.replace(opts, l2=float(w)), None)
                fits.append(fit.run())
            best = int(select([fit.strip_dummy(th) for th, _ in fits]))
            fits[best][1]["optimizer"] = optimizer
            theta, info = fit.stage_result(*fits[best], l2_grid[best], threshold)
            if bounds is not None:
                info["at_bound"] = count_at_bound(theta, bounds)
            return theta, info, best
        finally:
            fit.prob.close()


def check_bounds(bounds, P, has_intercept):
    """(lower, upper) of fit_stepping -> two contiguous float64 arrays of P entries: no NaN, lower <= upper, the intercept (last) infinite.
    (gdmix_fe_set_bounds refuses the same; here the message can name the coefficient.)"""
    try:
        lower, upper = (np.array(b, np.float64) for b in bounds)      # (copies: the caller's arrays may be read-only)
    except (TypeError, ValueError):
        raise ValueError("bounds are a pair (lower, upper) of arrays") from None
    if lower.shape != (P,) or upper.shape != (P,):
        raise ValueError(f"bounds: lower and upper hold {P} entries each (num_features + has_intercept, intercept last), not {lower.shape} and {upper.shape}")
    bad = np.flatnonzero(np.isnan(lower) | np.isnan(upper))
    if bad.size:
        raise ValueError(f"bounds: coefficient {int(bad[0])} has a bound that is not a number")
    bad = np.flatnonzero(lower > upper)
    if bad.size:
        raise ValueError(f"bounds: coefficient {int(bad[0])} has lower {lower[bad[0]]} > upper {upper[bad[0]]}")
    if has_intercept and (lower[-1] != -np.inf or upper[-1] != np.inf):
        raise ValueError("bounds: the intercept (the last entry) is never bounded: -inf and +inf")
    return lower, upper


def count_at_bound(theta, bounds):
    """How many coefficients equal one of their bounds."""
    return int(np.count_nonzero((theta == bounds[0]) | (theta == bounds[1])))


def fit_options(has_intercept, l2, regularize_bias, model_type, max_iter, m, tolerance):
    """The solver's options of a fixed-effect fit: the objective is not divided by n, the model is stored unthresholded."""
    if model_type not in LOSS_OF_MODEL_TYPE:
        raise ValueError(f"unknown model type {model_type!r}")
    return SolverOptions(l2=l2, regularize_bias=bool(regularize_bias) and bool(has_intercept), has_intercept=has_intercept, m=m,
                         max_iter=max_iter, ftol=tolerance, threshold=0.0, sum_loss=True, linear=(model_type == LINEAR_REGRESSION),
                         loss="poisson" if model_type == POISSON_REGRESSION else None)


class DeviceShard:
    """A raw shard's sample-major arrays in HBM: row_nnz_ptr [n + 1] / col_global / val (None, None, None for a model without a
    feature bag), offset [n], and the labels when given. Feature indices are checked against [0, num_features) once, here."""

    def __init__(self, solver, row_nnz_ptr, col_global, val, offset, num_features, label=None):
        t = solver.torch
        dev = solver.device
        up = lambda a, dt: None if a is None else t.from_numpy(np.ascontiguousarray(a, dt)).to(dev)
        self.n = (len(row_nnz_ptr) - 1) if row_nnz_ptr is not None else len(offset)
        self.rp, self.cg, self.vl = up(row_nnz_ptr, np.int64), up(col_global, np.int64), up(val, np.float32)
        if self.cg is not None and self.cg.numel() and (int(self.cg.min()) < 0 or int(self.cg.max()) >= num_features):
            raise ValueError(f"feature index outside [0, {num_features})")
        self.of = up(offset, np.float32)
        self.y = up(label, np.float32)
        self.num_features = int(num_features)

    def pointers(self):
        """(row_nnz_ptr, col_global, val, offset) as the library takes them: NULL for what is absent or empty."""
        ptr = lambda x: None if x is None or x.numel() == 0 else x.data_ptr()
        return (None if self.cg is None or self.cg.numel() == 0 else self.rp.data_ptr()), ptr(self.cg), ptr(self.vl), ptr(self.of)


def _theta_on_device(solver, theta, P):
    t = solver.torch
    th = theta if t.is_tensor(theta) else t.from_numpy(np.ascontiguousarray(theta, np.float64)).to(solver.device)
    if not th.is_cuda or th.dtype != t.float64 or not th.is_contiguous() or th.numel() != P:
        from .solver import GdmixReError
        raise GdmixReError(f"a coefficient vector is a contiguous float64 array of {P} entries (intercept last)")
    return th


def device_score_shard(solver, shard, theta, has_intercept):
    """(score, per-coordinate score) float32 DEVICE tensors of every sample of an uploaded shard (gdmix_fe_score)."""
    t = solver.torch
    th = _theta_on_device(solver, theta, shard.num_features + (1 if has_intercept else 0))
    score = t.empty(shard.n, dtype=t.float32, device=solver.device)
    per = t.empty(shard.n, dtype=t.float32, device=solver.device)
    if shard.n == 0:
        return score, per
    rc = solver.lib.gdmix_fe_score(solver._h, shard.n, *shard.pointers(), th.data_ptr(), shard.num_features, int(bool(has_intercept)),
                                   score.data_ptr(), per.data_ptr(), solver._stream())
    if rc != 0:
        from .solver import GdmixReError
        raise GdmixReError("gdmix_fe_score: " + solver.lib.gdmix_re_last_error().decode())
    return score, per


def device_score_models(solver, shard, thetas, has_intercept, per_coord=True, slot_major=True):
    """gdmix_fe_score_models over an uploaded shard -> (score [K, n], per_coord [K, n] | None) float32 device tensors."""
    from .solver import GdmixReError
    t = solver.torch
    K = len(thetas)
    if K < 1:
        raise GdmixReError("score_models: no model")
    P = shard.num_features + (1 if has_intercept else 0)
    ths = [_theta_on_device(solver, th, P) for th in thetas]
    n = shard.n
    score = t.empty((K, n), dtype=t.float32, device=solver.device)
    per = t.empty((K, n), dtype=t.float32, device=solver.device) if per_coord else None
    ptrs = (C.c_void_p * K)(*[th.data_ptr() for th in ths])
    ws, nbytes = None, 0
    if slot_major:
        nbytes = int(solver.lib.gdmix_fe_score_models_workspace_bytes(shard.num_features, K))
        ws = t.empty(max(nbytes, 1), dtype=t.uint8, device=solver.device)
    rc = solver.lib.gdmix_fe_score_models(solver._h, n, *shard.pointers(), ptrs, K, shard.num_features, int(bool(has_intercept)),
                                          score.data_ptr() if n else None, None if per is None or not n else per.data_ptr(),
                                          None if ws is None else ws.data_ptr(), nbytes, solver._stream())
    if rc != 0:
        raise GdmixReError("gdmix_fe_score_models: " + solver.lib.gdmix_re_last_error().decode())
    return score, per


def device_score(solver, row_nnz_ptr, col_global, val, offset, theta, num_features, has_intercept):
    """(score, per-coordinate score) float32 numpy arrays of every sample: x . w + b (+ offset). theta: [num_features +
    has_intercept], intercept last. The shard is read once off its sample-major arrays (gdmix_fe_score): no pack. Uploads the shard
    and downloads the scores on every call; DeviceShard + device_score_shard keep both in HBM."""
    shard = DeviceShard(solver, row_nnz_ptr, col_global, val, offset, num_features)
    score, per = device_score_shard(solver, shard, theta, has_intercept)
    return score.cpu().numpy(), per.cpu().numpy()


ST_ABORTED = 9      # GDMIX_RE_ST_ABORTED
ST_ABORTED_PEER = 10   # GDMIX_RE_ST_ABORTED_PEER: another worker's step was aborted (its mark came with the all-reduce)
FE_RING = 8         # status ring of the library (csrc/fe_solve.hip: FE_RING): a status can be read at most FE_RING - 1 steps late
LOOKAHEAD = int(os.environ.get("GDMIX_FE_LOOKAHEAD", "2"))   # evaluations enqueued ahead of the status the host has read


class _SteppingProblem:
    """gdmix_fe_problem handle; the packed shard and theta0 are kept alive with it."""

    def __init__(self, solver, packed, num_features, opts, theta0_dev):
        from .solver import GdmixReError
        self.solver, self.packed, self.theta0 = solver, packed, theta0_dev
        self.lib = solver.lib
        self._h = C.c_void_p()
        c_opts = opts.to_c()
        rc = self.lib.gdmix_fe_create(solver._h, C.byref(packed.c), int(num_features), C.byref(c_opts),
                                      None if theta0_dev is None else theta0_dev.data_ptr(), C.byref(self._h), solver._stream())
        if rc != 0:
            raise GdmixReError("gdmix_fe_create: " + self.lib.gdmix_re_last_error().decode())
        cnt = C.c_int64()
        ptr = self.lib.gdmix_fe_reduce_buffer(self._h, C.byref(cnt))
        self.count = int(cnt.value)
        self.buffer_ptr = ptr

    def _check(self, rc, what):
        from .solver import GdmixReError
        if rc != 0:
            raise GdmixReError(f"{what}: " + self.lib.gdmix_re_last_error().decode())

    def restart(self, opts, theta0_dev=None):
        """gdmix_fe_restart: the problem as creation left it, for other options (l2, regularize_bias, the limits and tolerances) and
        another start point (None: zeros); the copies of the non-zeros and their tables stay. Stream-ordered."""
        c_opts = opts.to_c()
        self._check(self.lib.gdmix_fe_restart(self._h, C.byref(c_opts), None if theta0_dev is None else theta0_dev.data_ptr(),
                                              self.solver._stream()), "gdmix_fe_restart")
        self.theta0 = theta0_dev      # kept alive: a kernel on the stream reads it

    def set_prior(self, mean_dev=None, scale_dev=None):
        """gdmix_fe_set_prior: float64 device tensors [D + has_intercept], intercept last (copied by the library); None, None removes the
        prior. Leaves the problem as a restart with its current options at phi = 0 does."""
        for x in (mean_dev, scale_dev):
            if x is not None and (not x.is_cuda or x.dtype != self.solver.torch.float64 or not x.is_contiguous() or x.numel() != self.count - 1):
                from .solver import GdmixReError
                raise GdmixReError(f"a prior vector is a contiguous float64 device array of {self.count - 1} entries (intercept last)")
        self._check(self.lib.gdmix_fe_set_prior(self._h, None if mean_dev is None else mean_dev.data_ptr(),
                                                None if scale_dev is None else scale_dev.data_ptr(), self.solver._stream()), "gdmix_fe_set_prior")
        self.theta0 = None

    def set_l1(self, l1):
        """gdmix_fe_set_l1: l1 > 0 puts the problem on the OWL-QN step, 0 back on the L-BFGS-B step. Leaves the problem as a restart with
        its current options at zeros does. Stream-ordered."""
        self._check(self.lib.gdmix_fe_set_l1(self._h, float(l1), self.solver._stream()), "gdmix_fe_set_l1")
        self.theta0 = None

    def set_bounds(self, lower_dev=None, upper_dev=None):
        """gdmix_fe_set_bounds: float64 device tensors [D + has_intercept], intercept last and infinite (copied by the library) put the problem
        on the projected L-BFGS step; None, None back on the L-BFGS-B step. Leaves the problem as a restart with its current options at the
        clamped zeros does; a restart keeps the bounds."""
        for x in (lower_dev, upper_dev):
            if x is not None and (not x.is_cuda or x.dtype != self.solver.torch.float64 or not x.is_contiguous() or x.numel() != self.count - 1):
                from .solver import GdmixReError
                raise GdmixReError(f"a bound vector is a contiguous float64 device array of {self.count - 1} entries (intercept last)")
        self._check(self.lib.gdmix_fe_set_bounds(self._h, None if lower_dev is None else lower_dev.data_ptr(),
                                                 None if upper_dev is None else upper_dev.data_ptr(), self.solver._stream()), "gdmix_fe_set_bounds")
        self.theta0 = None

    def set_optimizer(self, optimizer):
        """gdmix_fe_set_optimizer: "TRON" puts the problem on the trust-region Newton step, "LBFGS" back on the L-BFGS-B step. Leaves the
        problem as a restart with its current options at zeros does. Stream-ordered."""
        self._check(self.lib.gdmix_fe_set_optimizer(self._h, OPTIMIZER_CODE[check_optimizer(optimizer)], self.solver._stream()), "gdmix_fe_set_optimizer")
        self.theta0 = None

    def products(self):
        """Hessian-vector products the problem has taken since its last restart (gdmix_fe_products); 0 on a problem that never was TRON's."""
        n = C.c_int64(0)
        self._check(self.lib.gdmix_fe_products(self._h, C.byref(n), self.solver._stream()), "gdmix_fe_products")
        return int(n.value)

    def hessian_vec(self, theta_dev, v_dev):
        """X~' D X~ v of the shard at theta (device tensors [D + has_intercept], intercept last; theta None = the current accepted point)
        into the reduce buffer, no regulariser (gdmix_fe_hessian_vec)."""
        for x in (theta_dev, v_dev):
            if x is not None and (not x.is_cuda or x.dtype != self.solver.torch.float64 or not x.is_contiguous() or x.numel() != self.count - 1):
                from .solver import GdmixReError
                raise GdmixReError(f"a coefficient vector is a contiguous float64 device array of {self.count - 1} entries (intercept last)")
        if v_dev is None:
            from .solver import GdmixReError
            raise GdmixReError("hessian_vec: v is None")
        self._check(self.lib.gdmix_fe_hessian_vec(self._h, None if theta_dev is None else theta_dev.data_ptr(), v_dev.data_ptr(), self.solver._stream()),
                    "gdmix_fe_hessian_vec")

    def reduce_tensor(self):
        """The [gradient, value] buffer as a torch tensor view (no copy), for torch.distributed.all_reduce."""
        t = self.solver.torch
        return _device_view(t, self.buffer_ptr, self.count, self.solver.device)

    def eval(self):
        self._check(self.lib.gdmix_fe_eval(self._h, self.solver._stream()), "gdmix_fe_eval")

    def step(self):
        st = C.c_int32(-1)
        self._check(self.lib.gdmix_fe_step(self._h, self.solver._stream(), C.byref(st)), "gdmix_fe_step")
        return int(st.value)

    def step_async(self):
        """Enqueue the step; returns its number (gdmix_fe_step_async)."""
        seq = C.c_int64(-1)
        self._check(self.lib.gdmix_fe_step_async(self._h, self.solver._stream(), C.byref(seq)), "gdmix_fe_step_async")
        return int(seq.value)

    def step_status(self, seq):
        st = C.c_int32(-1)
        self._check(self.lib.gdmix_fe_step_status(self._h, int(seq), C.byref(st)), "gdmix_fe_step_status")
        return int(st.value)

    def solve(self, lookahead=LOOKAHEAD, max_evals=100000):
        """The whole single-worker loop inside the library (gdmix_fe_solve): the status is read `lookahead` steps late."""
        st, n = C.c_int32(-1), C.c_int64(0)
        self._check(self.lib.gdmix_fe_solve(self._h, self.solver._stream(), int(lookahead), int(max_evals), C.byref(st), C.byref(n)),
                    "gdmix_fe_solve")
        return int(st.value), int(n.value)

    def result(self):
        t = self.solver.torch
        theta = t.empty(self.count - 1, dtype=t.float64, device=self.solver.device)
        f, g, nit, nfev = C.c_double(), C.c_double(), C.c_int32(), C.c_int32()
        self._check(self.lib.gdmix_fe_result(self._h, theta.data_ptr(), C.byref(f), C.byref(g), C.byref(nit), C.byref(nfev),
                                             self.solver._stream()), "gdmix_fe_result")
        return theta.cpu().numpy(), dict(fval=f.value, gnorm=g.value, nit=int(nit.value), nfev=int(nfev.value))

    def hessian_diag(self, theta_dev=None):
        """diag(X~' D X~) of the shard at theta (device tensor [D + has_intercept], None = the current point) into the reduce
        buffer (gdmix_fe_hessian_diag)."""
        self._check(self.lib.gdmix_fe_hessian_diag(self._h, None if theta_dev is None else theta_dev.data_ptr(), self.solver._stream()),
                    "gdmix_fe_hessian_diag")

    def stream_bytes(self):
        """(bytes of entries the row pass reads, the column pass reads) — gdmix_fe_stream_bytes."""
        a, b = C.c_int64(), C.c_int64()
        self._check(self.lib.gdmix_fe_stream_bytes(self._h, C.byref(a), C.byref(b)), "gdmix_fe_stream_bytes")
        return int(a.value), int(b.value)

    def last_eval_ms(self):
        a, b = C.c_float(), C.c_float()
        self._check(self.lib.gdmix_fe_last_eval_ms(self._h, C.byref(a), C.byref(b)), "gdmix_fe_last_eval_ms")
        return float(a.value), float(b.value)

    def close(self):
        if self._h:
            self.lib.gdmix_fe_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _device_view(torch, ptr, count, device):
    """float64 tensor over `count` doubles of device memory owned by the library."""
    class _Holder:
        pass
    h = _Holder()
    h.__cuda_array_interface__ = {"shape": (count,), "typestr": "<f8", "data": (int(ptr), False), "version": 2}
    return torch.as_tensor(h, device=device)


def run_stepping_loop(problem, all_reduce=None, max_evals=100000, lookahead=None):
    """do { eval; all_reduce; } while (step() < 0)  — the loop gdmix_fe.h describes, with the status read `lookahead` steps late
    so that the device never waits for the host between evaluations (the kernels of a stopped problem return at once; every
    worker takes the same decisions, so all of them enqueue the same number of all-reduces). all_reduce(tensor) sums in place
    across workers (None: single worker, the loop runs inside the library). A collective that goes through the host (gloo) is
    synchronous anyway: lookahead 0 unless all_reduce.device_ordered is set (RCCL on the device buffer)."""
    if lookahead is None:
        lookahead = LOOKAHEAD if (all_reduce is None or getattr(all_reduce, "device_ordered", False)) else 0
    if not 0 <= int(lookahead) < FE_RING:      # the status ring of the library (gdmix_fe_step_status would fail mid-run, collectives queued)
        raise ValueError(f"lookahead must be in 0..{FE_RING - 1}, not {lookahead}")
    lookahead = int(lookahead)
    if all_reduce is None:
        status, _ = problem.solve(lookahead, max_evals)
        if status in (ST_ABORTED, ST_ABORTED_PEER):
            raise RuntimeError(f"the fixed-effect step gave up waiting for a workgroup of its own launch (status {status}): the result is invalid")
        if status >= 0:
            return status
        raise RuntimeError(f"the fixed-effect L-BFGS loop did not stop within {max_evals} evaluations")
    buf = problem.reduce_tensor()
    for k in range(max_evals + lookahead):
        problem.eval()
        all_reduce(buf)
        seq = problem.step_async()
        if k >= lookahead:
            status = problem.step_status(seq - lookahead)
            if status == ST_ABORTED:
                # The abort is a per-device timeout: the other workers have not seen it. This worker's value slot carries the mark
                # (csrc/fe_solve.hip), the next all-reduce hands it to everybody and their step stops with the same status — one
                # evaluation later, so this worker joins one more all-reduce before it raises: every worker has then enqueued the
                # same number of collectives and none hangs in RCCL.
                problem.eval()
                all_reduce(buf)
                raise RuntimeError("the fixed-effect step gave up waiting for a workgroup of its own launch (status 9): the result is invalid "
                                   "(every worker stops in the same evaluation)")
            if status == ST_ABORTED_PEER:      # one evaluation behind the worker it happened on: the collectives are even, nothing to add
                raise RuntimeError("another worker's fixed-effect step was aborted (status 10): the result is invalid")
            if status >= 0:
                return problem.step_status(seq)      # (the steps behind the stop are no-ops with the same status: nothing left in flight)
    raise RuntimeError(f"the fixed-effect L-BFGS loop did not stop within {max_evals} evaluations")


class _SteppingFit:
    """What a fit through include/gdmix_fe.h needs around its loop: the shard as a packed one-entity batch, the problem (gdmix_fe_create)
    and the all-reduce of this process group; then the loop, and the result as the stage takes it."""

    def __init__(self, solver, opts, row_nnz_ptr, col_global, val, y, num_features, offset, weight, theta0, group, dummy, variance_mode,
                 prior=None, feature_scale=None, down_sampling=None):
        ic = 1 if opts.has_intercept else 0
        if prior is not None and theta0 is not None:
            raise ValueError("a fit with a prior starts at the prior mean: theta0 must be None")
        if prior is not None and feature_scale is not None:
            raise ValueError("feature normalisation does not compose with a prior model")
        n_rows = np.asarray(row_nnz_ptr).size - 1
        shard, self.dummy = shard_as_batch(row_nnz_ptr, col_global, val, y, offset, weight, opts.has_intercept,
                                           binary_labels=opts.loss_name() == "logistic", dummy=dummy)
        if opts.loss_name() == "poisson":
            from .batch import check_count_labels
            check_count_labels(shard.y, "poisson_regression, the fixed effect's shard")
        D = 1 if self.dummy else int(num_features)   # the dummy zero feature of an intercept-only model occupies global index 0
        if not self.dummy and shard.col_global.size and (shard.col_global.min() < 0 or shard.col_global.max() >= D):
            raise ValueError(f"feature index outside [0, {D})")
        self.down_sampling = None      # the counts of the down-sampling pass, when there was one
        if down_sampling is not None:
            from .downsample import check_rate
            rate, seed, uid = check_rate(down_sampling[0]), int(down_sampling[1]), np.ascontiguousarray(down_sampling[2], np.int64)
            if uid.shape != (n_rows,):
                raise ValueError(f"down_sampling: one uid per row of the shard ({n_rows}), not {uid.shape}")
            if rate == 1.0:
                down_sampling = None   # the plain fit: not a call, not a bit of difference
        # whether the variances can be computed is decided before any training (a job that trains for its whole budget and
        # then dies on the variances loses the model)
        if variance_mode is not None:
            check_variance_request(str(variance_mode).upper(), D + ic, _world_size(group))
        self.solver, self.opts, self.D, self.group, self.variance_mode = solver, opts, D, group, variance_mode
        self._sample = None            # the down-sampled arrays in HBM while self.batch has not been asked for
        if down_sampling is None:
            self._batch = shard
            self.packed = solver.pack(shard, has_intercept=opts.has_intercept)
        else:
            self._batch, self.packed = self._pack_sample(shard, n_rows, rate, seed, uid)
        t0 = None
        if theta0 is not None:
            full = np.zeros(D + ic)
            th = np.asarray(theta0, np.float64)
            if self.dummy:
                full[D:] = th[-ic:] if ic else []
            else:
                full[:] = th
            t0 = solver.torch.from_numpy(full).to(solver.device)
        self.prob = _SteppingProblem(solver, self.packed, D, opts, None if (feature_scale is not None and not self.dummy) else t0)
        self.prior_scale = None
        if prior is not None:
            mean, self.prior_scale = prior_vectors(prior[0], prior[1], D, ic, self.dummy, opts.regularize_bias)
            up = lambda a: solver.torch.from_numpy(a).to(solver.device)
            self.prob.set_prior(up(mean), up(self.prior_scale))
        elif feature_scale is not None and not self.dummy:
            # mean 0, scale s, 1 for the intercept: created cold, the prior installed, then the start point in theta units
            # (gdmix_fe_set_prior leaves the problem at phi = 0; gdmix_fe_restart takes theta0 as theta while a prior is installed)
            sc = np.ones(D + ic)
            sc[:D] = np.asarray(feature_scale, np.float64)
            if sc.shape != (D + ic,) or not np.all(np.isfinite(sc) & (sc > 0)):
                raise ValueError(f"feature_scale holds {D} finite factors > 0")
            self.prior_scale = sc
            up = lambda a: solver.torch.from_numpy(a).to(solver.device)
            self.prob.set_prior(up(np.zeros(D + ic)), up(sc))
            if t0 is not None:
                self.prob.restart(opts, t0)
        self.all_reduce = None
        try:
            import torch.distributed as dist
            if dist.is_available() and dist.is_initialized() and dist.get_world_size(group) > 1:
                if dist.get_backend(group) == "nccl":          # RCCL, in place on the device buffer, ordered on the stream
                    def all_reduce(t):
                        dist.all_reduce(t, group=group)
                    all_reduce.device_ordered = True
                else:                                          # e.g. gloo: staged through the host
                    def all_reduce(t):
                        h = t.cpu()
                        dist.all_reduce(h, group=group)
                        t.copy_(h)
                self.all_reduce = all_reduce
        except ImportError:
            pass

    def device_bounds(self, bounds):
        """(lower, upper) of check_bounds as the device tensors set_bounds takes."""
        if self.dummy:
            raise ValueError("bounds name features: a model without a feature bag has none")
        return tuple(self.solver.torch.from_numpy(b).to(self.solver.device) for b in bounds)

    def _pack_sample(self, shard, n_rows, rate, seed, uid):
        """Upload the shard, down-sample it on the device, pack the sample -> (the host batch of the sample or None while it stays in HBM,
        the packed sample). A sample without a row or without a non-zero becomes the weight-0 sample shard_as_batch builds for an empty
        bagged shard: the worker still joins every all-reduce with a full-size buffer."""
        solver, opts = self.solver, self.opts
        logistic = opts.loss_name() == "logistic"
        if shard.N == n_rows + 1:
            # the shard held no non-zero and carries shard_as_batch's weight-0 sample at its end. Whatever uid that row gets, the outcome
            # is what sampling the shard's own rows first gives: kept, it is the same row (0 / rate = 0); dropped, the sample has no
            # non-zero and gets the row back below.
            uid = np.concatenate([uid, np.zeros(1, np.int64)])
        sample, counts = solver.downsample(solver.upload(shard), uid, rate, seed, negatives_only=logistic)
        self.down_sampling = dict(counts, rate=rate, seed=seed, rows=n_rows)      # (the shard's own rows: never the appended weight-0 sample)
        if shard.N == n_rows + 1 and bool(sample["kept_rows"][-1:].eq(n_rows).any()):
            self.down_sampling["kept"] -= 1      # ... which holds the sample's one non-zero and, label 0, counts as a negative when kept
            self.down_sampling["kept_nnz"] -= 1
            self.down_sampling["negatives_kept"] -= 1
        if counts["kept"] > 0 and counts["kept_nnz"] > 0:
            self._sample = sample
            return None, solver.pack(sample, has_intercept=opts.has_intercept)
        h = lambda k: sample[k].cpu().numpy()
        batch, _ = shard_as_batch(h("row_nnz_ptr"), [], [], h("y"), h("offset"), h("weight"), opts.has_intercept, binary_labels=logistic,
                                  dummy=self.dummy)
        return batch, solver.pack(batch, has_intercept=opts.has_intercept)

    @property
    def batch(self):
        """The host batch the problem was built from: the shard, or its sample — copied back from HBM when first asked for (the FULL
        variances of a small model are computed on the host from it: never from the full shard when the fit came from the sample)."""
        if self._batch is None:
            s = self._sample
            h = lambda k: s[k].cpu().numpy()
            self._batch = RawBatch(ent_row_ptr=h("ent_row_ptr"), row_nnz_ptr=h("row_nnz_ptr"), col_global=h("col_global"), val=h("val"), y=h("y"),
                                   offset=h("offset"), weight=h("weight"), uid=np.arange(int(s["N"]), dtype=np.int64),
                                   entity_ids=["fixed_effect"], has_label=True, binary_labels=self.opts.loss_name() == "logistic")
        return self._batch

    def run(self):
        """The loop on the problem as it stands -> (theta, info) in the problem's layout (the dummy feature still in front)."""
        status = run_stepping_loop(self.prob, self.all_reduce)
        theta, info = self.prob.result()
        info["status"] = status
        info["nhv"] = self.prob.products()
        return theta, info

    def strip_dummy(self, x):
        return x[self.D:] if self.dummy else x

    def stage_result(self, theta, info, l2, threshold):
        """(theta, info) of run() as fit_stepping returns them: with a variance mode, the variances of the thresholded model on the
        training data, as the reference's scoring pass after training computes them (fixed_effect_lr_lbfgs_model.py:648-661, 271-305,
        451-463); the dummy entry stripped from both."""
        if self.variance_mode is not None:
            th = np.where(np.abs(theta) <= threshold, 0.0, theta)
            o = self.opts
            info["variances"] = self.strip_dummy(_variances(self.solver, self.prob, self.batch, th, self.D, o.has_intercept, float(l2), o.regularize_bias,
                                                            str(self.variance_mode).upper(), self.all_reduce, self.group, packed=self.packed,
                                                            dummy=self.dummy, scale=self.prior_scale, poisson=o.loss_name() == "poisson"))
        if self.down_sampling is not None:
            info["down_sampling"] = dict(self.down_sampling)
        return self.strip_dummy(theta), info


# FULL densifies a (D + 1) x (D + 1) Hessian, as the reference does (fixed_effect_lr_lbfgs_model.py:291, 457: no limit there but
# memory). Up to FULL_VARIANCE_HOST_MAX coefficients the matrix is built and inverted on the host exactly as the reference does
# (several workers: summed with an all-reduce first); above that and up to FULL_VARIANCE_DEVICE_MAX on the device (tiled Cholesky
# and inverse over the whole MI355X, csrc/re_variance_big.hip). Several workers (round 4): every worker builds the dense curvature
# matrix of its shard on its device (gdmix_fe_hessian_dense), scatters it into the common index space, one all-reduce of the
# P x P matrix (RCCL), and every worker factors the sum (gdmix_fe_variance_of_hessian) — replicated, as scipy is in the reference.
FULL_VARIANCE_HOST_MAX = 4096
FULL_VARIANCE_DEVICE_MAX = 16384


def _world_size(group=None):
    try:
        import torch.distributed as dist
        if dist.is_available() and dist.is_initialized():
            return dist.get_world_size(group)
    except ImportError:
        pass
    return 1


def check_variance_request(mode, P, num_workers):
    """Raise before any training if the variances asked for cannot be computed for a model of P coefficients."""
    if mode == "SIMPLE":
        return
    if mode != "FULL":
        raise ValueError(f"unknown variance mode {mode!r}")
    if P > FULL_VARIANCE_DEVICE_MAX:
        raise ValueError(f"fixed_effect_variance_mode FULL inverts a dense {P} x {P} matrix; at most {FULL_VARIANCE_DEVICE_MAX} "
                         "coefficients (use SIMPLE for larger models)")


def usable_variance(v):
    """Prior variances with the default put in: 1 where the variance is missing (0 after the join), not finite or <= 0 (model.usable_variance)."""
    v = np.asarray(v, np.float64)
    return np.where(np.isfinite(v) & (v > 0.0), v, 1.0)


def prior_vectors(mean, variance, D, ic, dummy, regularize_bias):
    """(mean, scale = sqrt(variance)) [D + ic] as gdmix_fe_set_prior takes them, from a prior in theta0's layout (a dummy model's: the
    intercept alone; the dummy feature gets mean 0, scale 1). variance None: every variance 1. An unregularised intercept has no penalty:
    its scale is 1 and its mean is only where the fit starts (include/gdmix_fe.h, "The intercept")."""
    P = D + ic
    mu, v = np.zeros(P), np.ones(P)
    m_in = np.asarray(mean, np.float64)
    v_in = np.ones(m_in.size) if variance is None else usable_variance(variance)
    if m_in.size != (ic if dummy else P) or v_in.size != m_in.size:
        raise ValueError(f"a prior has {ic if dummy else P} means and as many variances (intercept last), not {m_in.size} and {v_in.size}")
    if dummy:
        mu[D:], v[D:] = m_in, v_in
    else:
        mu[:], v[:] = m_in, v_in
    if not np.all(np.isfinite(mu)):
        raise ValueError("a prior mean is not finite")
    if ic and not regularize_bias:
        v[D] = 1.0
    return mu, np.sqrt(v)


def simple_variances(H, l2, ic, regularize_bias, scale=None):
    """SIMPLE variances from the diagonal H of X~' D X~ (intercept last): 1 / (H_j + l2 [j regularised] + 1e-12); with a prior of scale s
    the same in phi-space mapped back, s_j^2 / (s_j^2 H_j + l2 [j regularised] + 1e-12)."""
    eps = 1.0e-12
    reg = np.full(H.size, float(l2))
    if ic and not regularize_bias:
        reg[-1] = 0.0
    if scale is None:
        return 1.0 / (H + reg + eps)
    s2 = np.asarray(scale, np.float64) ** 2
    return s2 / (s2 * H + reg + eps)


def full_variances_of(H, l2, ic, regularize_bias, scale=None):
    """FULL variances from the dense X~' D X~ (intercept last): diag((H + (l2 + 1e-12) I - l2 e_u e_u')^-1), u an unregularised intercept;
    with a prior of scale s, s_j^2 diag((S H S + (l2 + 1e-12) I - l2 e_u e_u')^-1)_j = diag((H + diag((l2 [regularised] + 1e-12) / v))^-1)."""
    eps = 1.0e-12
    P = H.shape[0]
    reg = np.full(P, float(l2) + eps)
    if ic and not regularize_bias:
        reg[-1] -= l2
    if scale is not None:
        reg = reg / (np.asarray(scale, np.float64) ** 2)
    return np.diagonal(np.linalg.inv(H + np.diag(reg))).copy()


def _variances(solver, prob, batch, theta, D, has_intercept, l2, regularize_bias, mode, all_reduce, group, packed=None, dummy=False, scale=None,
               poisson=False):
    """variance of every coefficient (intercept last). SIMPLE: 1 / (diag(X~' D X~) + l2 [regularised] + 1e-12), the diagonal by two
    more streaming passes on the device and the same all-reduce as an evaluation. FULL: diag((X~' D X~ + (l2 + 1e-12) I - l2
    [intercept unregularised])^-1): the dense matrix is built on the host from the shard (scipy), summed over the workers and
    inverted with numpy, exactly as the reference does (:296-305, 457-463) — only sensible for small feature spaces.
    scale: the prior scale [D + ic] of an incremental fit (include/gdmix_fe.h, "incremental training"): the same mode applied in phi-space
    to S H S and mapped back, Var(theta_j) = s_j^2 Var'(phi_j); theta is theta, and the curvature the device returns is theta-space's.
    poisson: the curvature weight is D_i = w_i exp(z_i) (include/gdmix_fe.h, "poisson"): SIMPLE takes it from the problem's loss, the FULL
    routes are told."""
    eps = 1.0e-12
    ic = 1 if has_intercept else 0
    P = D + ic
    if mode == "SIMPLE":
        t = solver.torch
        prob.hessian_diag(t.from_numpy(np.ascontiguousarray(theta, np.float64)).to(solver.device))
        buf = prob.reduce_tensor()
        if all_reduce is not None:
            all_reduce(buf)
        H = buf[:P].cpu().numpy().copy()
        if scale is not None:
            return simple_variances(H, l2, ic, regularize_bias, scale)
        H += l2
        if ic and not regularize_bias:
            H[-1] -= l2
        return 1.0 / (H + eps)
    if mode != "FULL":
        raise ValueError(f"unknown variance mode {mode!r}")
    check_variance_request(mode, P, _world_size(group))
    if P > FULL_VARIANCE_HOST_MAX and (_world_size(group) > 1 or scale is not None):
        # (with a prior any number of workers: the one-worker shortcut below, solver.variance_full, knows no prior)
        return _full_variances_several_workers(solver, packed, theta, D, has_intercept, l2, regularize_bias, group, dummy, scale=scale,
                                               loss="poisson" if poisson else None)
    if P > FULL_VARIANCE_HOST_MAX:
        # on the device, in the shard's local index space (intercept first): the random-effect FULL variance of a one-entity
        # batch is this very matrix (binary_logistic_regression.py:181-187 = fixed_effect_lr_lbfgs_model.py:296-305, 457-463).
        # Features without a non-zero in the shard have a zero row and column in X~' D X~: their variance is 1 / (l2 + 1e-12).
        uniq = packed.unique_global().cpu().numpy()
        local = to_local(theta, uniq, D, has_intercept, dummy)
        o = SolverOptions(l2=l2, regularize_bias=regularize_bias, has_intercept=has_intercept, loss="poisson" if poisson else None)
        v_local = solver.variance_full(packed, o, local).cpu().numpy()
        out = np.full(P, 1.0 / (l2 + eps))
        out[uniq] = v_local[ic:]
        if ic:
            out[D] = v_local[0]
        return out
    import scipy.sparse as sp
    n = batch.N
    X = sp.csr_matrix((batch.val.astype(np.float64), batch.col_global, batch.row_nnz_ptr), shape=(n, max(D, 1)))[:, :D]
    if ic:
        X = sp.hstack([X, sp.csr_matrix(np.ones((n, 1)))], format="csr")
    z = X @ theta + batch.offset.astype(np.float64)
    rho = 1.0 / (1.0 + np.exp(-z))
    d = (np.exp(z) if poisson else rho * (1.0 - rho)) * (1.0 if batch.weight is None else batch.weight.astype(np.float64))
    H = np.asarray((X.T @ X.multiply(d[:, None])).todense(), np.float64)
    try:
        import torch
        import torch.distributed as dist
        if dist.is_available() and dist.is_initialized() and dist.get_world_size(group) > 1:
            ht = torch.from_numpy(H)
            if dist.get_backend(group) == "nccl":
                hd = ht.to(solver.device)
                dist.all_reduce(hd, group=group)
                H = hd.cpu().numpy()
            else:
                dist.all_reduce(ht, group=group)
                H = ht.numpy()
    except ImportError:
        pass
    if scale is not None:
        return full_variances_of(H, l2, ic, regularize_bias, scale)
    H = H + np.diag([l2 + eps] * P)
    if ic and not regularize_bias:
        H[-1, -1] -= l2
    return np.diagonal(np.linalg.inv(H)).copy()


def _full_variances_several_workers(solver, packed, theta, D, has_intercept, l2, regularize_bias, group, dummy=False, scale=None, loss=None):
    """FULL variances on the device with the Hessian summed over the workers (fixed_effect_lr_lbfgs_model.py:291-305, 384-389,
    457-463). Coefficient order: features 0 .. D-1, intercept last. scale: the prior scale of an incremental fit — rows and columns of
    the summed matrix are scaled by it (S H S), the variances of that by s^2; with it also the route of a single worker."""
    import torch
    import torch.distributed as dist
    ic = 1 if has_intercept else 0
    P = D + ic
    uniq_dev = packed.unique_global()
    uniq = uniq_dev.cpu().numpy()
    p_l = uniq.size + ic
    ld = (P + 63) // 64 * 64
    # the summed matrix and the factorisation's work area are ld x ld doubles each, the local matrix another one at most: refuse with a
    # clear message rather than die in an allocation after the whole training
    need = 3 * ld * ld * 8 + (1 << 28)
    if solver.device.type == "cuda":
        # free = what the driver reports + what torch's caching allocator holds without using it (after a whole training run that can
        # be most of the HBM: ADVICE r5 — the driver's figure alone refused allocations that would have succeeded)
        free = torch.cuda.mem_get_info(solver.device)[0] + torch.cuda.memory_reserved(solver.device) - torch.cuda.memory_allocated(solver.device)
        if free < need:
            raise MemoryError(f"fixed_effect_variance_mode=FULL with {P} coefficients needs {need / 1e9:.1f} GB of free device memory "
                              f"({free / 1e9:.1f} GB free)")
    Hg = torch.zeros((ld, ld), dtype=torch.float64, device=solver.device)
    if not dummy and p_l > 0:     # (a worker without data trains on one weight-0 sample: its curvature is exactly zero — nothing to build or scatter)
        local = to_local(theta, uniq, D, has_intercept, dummy)
        Hl = solver.hessian_dense(packed, local, has_intercept, **({} if loss is None else {"loss": loss}))   # [ld_l, ld_l], local order: intercept first
        idx = torch.cat([torch.full((ic,), D, dtype=torch.int64, device=solver.device), uniq_dev.to(torch.int64)])   # local -> global coefficient
        Hg.index_put_((idx[:, None], idx[None, :]), Hl[:p_l, :p_l])       # one 2-D scatter into the common index space
        del Hl
    if _world_size(group) == 1:
        pass
    elif dist.get_backend(group) == "nccl":
        dist.all_reduce(Hg, group=group)
    else:      # (gloo: the two-worker tests on one device)
        h = Hg.cpu()
        dist.all_reduce(h, group=group)
        Hg = h.to(solver.device)
    unreg = D if (ic and not regularize_bias) else -1
    if scale is None:
        return solver.variance_of_hessian(Hg, P, l2, unreg).cpu().numpy()
    s = torch.from_numpy(np.ascontiguousarray(scale, np.float64)).to(solver.device)
    Hg[:P, :P] *= s[:, None]
    Hg[:P, :P] *= s[None, :]
    return (solver.variance_of_hessian(Hg, P, l2, unreg) * s * s).cpu().numpy()

