"""--l2_reg_weights: a random-effect stage sweeps l2_reg_weight itself and keeps the best model.

What the reference leaves to K runs of the stage and a Spark job that compares their evalSummary.json files (gdmix-data's
BestModelSelector) is pass 1 of ONE stage here: every partition of this worker is decoded, uploaded and packed once, solved once per
weight (cold start, no variances), its validation partition is scored under all the models in one pass over its non-zeros
(gdmix_re_join_features + gdmix_re_score_models, csrc/re_sweep.hip), and one exact stage metric per weight accumulates on the device
(metrics.DeviceEvaluator). No model and no score file is written. The winner's weight becomes model_params.l2_reg_weight and the stage
then runs as it always does (pass 2: driver.RandomEffectDriver.run_training), so its outputs are those of a plain run with that weight.

The selection uses pass 1's numbers, in which every partition is a device batch of its own; the stage's evalSummary.json is pass 2's,
where consecutive partitions may share a batch (GDMIX_PARTITIONS_PER_BATCH) and a team-tier entity may come out with other last bits.

Written under <metric_output_dir>/sweep/:
    model-<k>/evalSummary.json    {"auc" | "mse", "n", "n_pos", "n_neg", "n_nan", "two_u", "sse", "l2_reg_weight"}
    evals.json                    {"best model index", "model params": {"l2_reg_weight"}, "metric", "models": [{"index", "l2_reg_weight", <metric>}]}

Limits (refused with a message before any work): one worker; no prior model in output_model_dir (a sweep is a cold start); no entity
re-balancing; validation data and a metric directory are required. --action=inference ignores the flag.
"""
import dataclasses
import glob
import json
import logging
import math
import os

import numpy as np

from . import constants
from .metrics import SUMMARY_KEYS

logger = logging.getLogger(__name__)
logger.setLevel(logging.INFO)

SWEEP_DIR = "sweep"
EVALS_JSON = "evals.json"
BEST_MODEL_INDEX, MODEL_PARAMS = "best model index", "model params"      # BestModelSelector.scala's keys


class SweepError(ValueError):
    pass


# ---- the selection rule ------------------------------------------------------------------------------------------------------------
def select_best(metric, values):
    """Index of the best of `values` (one per weight, in the order of the list): the largest for "auc", the smallest for "mse"; a tie
    goes to the earlier index; NaN (or None) never wins; SweepError if nothing is left."""
    if metric not in ("auc", "mse"):
        raise SweepError(f"metric {metric!r}: the sweep compares auc or mse")
    best = None
    for k, v in enumerate(values):
        if v is None or (isinstance(v, float) and math.isnan(v)):
            continue
        v = float(v)
        if math.isnan(v):
            continue
        if best is None or (v > best[1] if metric == "auc" else v < best[1]):
            best = (k, v)
    if best is None:
        raise SweepError(f"the sweep has no model to choose: the validation {metric} of every weight is undefined "
                         "(one class only in the validation data, or a NaN score)")
    return best[0]


# ---- the files -----------------------------------------------------------------------------------------------------------------------
def _json_number(x):
    return None if isinstance(x, float) and x != x else x


def write_model_summary(out_dir, k, weight, metric, block):
    """<out_dir>/sweep/model-<k>/evalSummary.json from DeviceEvaluator.finish()'s dict."""
    d = os.path.join(out_dir, SWEEP_DIR, f"model-{k}")
    os.makedirs(d, exist_ok=True)
    out = {key: _json_number(block[key]) for key in (metric,) + SUMMARY_KEYS}
    out["l2_reg_weight"] = float(weight)
    with open(os.path.join(d, "evalSummary.json"), "w") as f:
        json.dump(out, f)
    return out


def write_evals(out_dir, metric, weights, values, best):
    d = os.path.join(out_dir, SWEEP_DIR)
    os.makedirs(d, exist_ok=True)
    out = {BEST_MODEL_INDEX: int(best), MODEL_PARAMS: {"l2_reg_weight": float(weights[best])}, "metric": metric,
           "models": [{"index": k, "l2_reg_weight": float(w), metric: _json_number(v)} for k, (w, v) in enumerate(zip(weights, values))]}
    with open(os.path.join(d, EVALS_JSON), "w") as f:
        json.dump(out, f)
    return out


def conclude(out_dir, metric, weights, blocks):
    """What both sweeps do with the K finished accumulators (DeviceEvaluator.finish()'s dicts): the per-model summaries, the selection,
    evals.json and the log line. -> the best index. (Every metric undefined: select_best raises, the summaries written before say why.)"""
    values = [b[metric] for b in blocks]
    for k, (w, b) in enumerate(zip(weights, blocks)):
        write_model_summary(out_dir, k, w, metric, b)
    best = select_best(metric, values)
    write_evals(out_dir, metric, weights, values, best)
    logger.info(f"sweep: validation {metric} {dict(zip(weights, values))}; best l2_reg_weight = {weights[best]} (index {best})")
    return best


# ---- the join, stated in numpy --------------------------------------------------------------------------------------------------------
def train_entity_map(eval_ids, train_ids):
    """[E_eval] int32: the training batch's row of the same entity id, -1 if it has none; an id listed twice in the training batch
    maps to its LAST row (the model ModelTable.update + lookup keep)."""
    if hasattr(eval_ids, "rows_in") and hasattr(train_ids, "all_different") and train_ids.all_different():
        return eval_ids.rows_in(train_ids).astype(np.int32)
    where = dict(zip(train_ids, range(len(train_ids))))      # a later row replaces an earlier one
    return np.fromiter((where.get(k, -1) for k in eval_ids), np.int32, count=len(eval_ids))


def join_features_host(eval_feat_ptr, eval_unique, train_feat_ptr, train_unique, train_entity, has_intercept):
    """What gdmix_re_join_features computes (include/gdmix_re.h): -> (coef_pos [P_eval] int64, has_model [E_eval] uint8)."""
    efp, tfp = np.asarray(eval_feat_ptr, np.int64), np.asarray(train_feat_ptr, np.int64)
    eu, tu = np.asarray(eval_unique, np.int64), np.asarray(train_unique, np.int64)
    te = np.asarray(train_entity, np.int64)
    E, Et, ic = efp.size - 1, tfp.size - 1, 1 if has_intercept else 0
    model = (te >= 0) & (te < Et)
    coef_pos = np.full(int(efp[-1]) + E * ic, -1, np.int64)
    te0 = np.where(model, te, 0)
    if ic:
        coef_pos[efp[:-1] + np.arange(E)] = np.where(model, tfp[te0] + te0, -1)
    d = np.diff(efp)
    ent = np.repeat(np.arange(E, dtype=np.int64), d)                 # entity of every evaluation feature
    if ent.size and tu.size:
        F = int(max(eu.max(initial=0), tu.max(initial=0))) + 1
        train_key = np.repeat(np.arange(Et, dtype=np.int64), np.diff(tfp)) * F + tu      # ascending: entity-major, features ascending
        want = te0[ent] * F + eu
        at = np.searchsorted(train_key, want)
        at_c = np.minimum(at, train_key.size - 1)
        hit = model[ent] & (at < train_key.size) & (train_key[at_c] == want)
        slot = np.arange(ent.size, dtype=np.int64) + ent * ic + ic
        coef_pos[slot[hit]] = at_c[hit] + te0[ent][hit] * ic + ic
    return coef_pos, model.astype(np.uint8)


# ---- refusals ------------------------------------------------------------------------------------------------------------------------
def refuse_several_workers(execution_context, flag="--l2_reg_weights"):
    if int(execution_context.get(constants.NUM_WORKERS) or 1) > 1:
        raise SweepError(f"{flag} runs on one worker: the AUC of several workers cannot be combined from their counts")


def refuse_poisson(model_type):
    if model_type == constants.POISSON_REGRESSION:
        raise SweepError("--l2_reg_weights does not run with --model_type=poisson_regression: the sweep compares auc or mse, not poisson_loss")


def refuse_blind_or_warm(mp, prior, prior_is=""):
    """No validation data, no metric directory, or a prior model (`prior`: the model files found where the stage would look for one)."""
    if not mp.validation_data_dir:
        raise SweepError("--l2_reg_weights needs --validation_data_dir: only validation data can choose a weight")
    if not mp.metric_output_dir:
        raise SweepError("--l2_reg_weights needs --metric_output_dir: the sweep writes its metrics there")
    if prior:
        raise SweepError(f"--l2_reg_weights is a cold start, and {prior[0]} is a prior model{prior_is}: warm-started sweeps are not implemented")


def validate(model, execution_context):
    """Everything a sweep does not do is refused here, before a partition is read or a solver created."""
    mp = model.model_params
    refuse_poisson(getattr(model, "model_type", None))
    refuse_blind_or_warm(mp, sorted(glob.glob(os.path.join(mp.output_model_dir, "part-*.avro"))))
    if mp.rebalance_entities:
        raise SweepError("--l2_reg_weights does not run with --rebalance_entities=True")
    refuse_several_workers(execution_context)


# ---- pass 1 --------------------------------------------------------------------------------------------------------------------------
def models_per_chunk(torch, device, K, bytes_per_model):
    """How many of K models are held at once: all of them if they fit into half of the free device memory (GDMIX_SWEEP_CHUNK sets
    it: tests)."""
    forced = int(os.environ.get("GDMIX_SWEEP_CHUNK", "0"))
    if forced > 0:
        return min(K, forced)
    free, _ = torch.cuda.mem_get_info(device)
    return int(max(1, min(K, (free // 2) // bytes_per_model)))


def _solve(model, solver, packed, opts, out):
    """One cold solve of the packed batch into `out`; every entity's status is checked as the stage checks it. A team barrier that
    timed out is answered as the stage answers it: once more without the tall team class, the knob put back."""
    out["status"].fill_(-1)
    solved = solver.solve(packed, opts, theta0=None, out=out)
    status = solved.status.cpu().numpy()
    if (status == model.ST_ABORTED).any() and getattr(solver, "tall_team_n", 0) != 0:
        logger.warning("sweep: entities timed out at a team barrier: solving the partition again without the tall team class")
        keep = solver.tall_team_n
        solver.set_tall_team_n(0)
        try:
            out["status"].fill_(-1)
            solved = solver.solve(packed, opts, theta0=None, out=out)
            status = solved.status.cpu().numpy()
        finally:
            solver.set_tall_team_n(keep)
    model._check_statuses(status, packed.E)
    return solved


def sweep_partition(model, solver, train_batch, eval_batch, weights, evaluators, slot_major=False):
    """Steps 1 - 5 for one partition: both batches packed once, K solves, one join, one scoring pass per chunk of models, K accumulators."""
    from .solver import VAR_NONE
    t = solver.torch
    if not train_batch.has_label:
        raise KeyError("the label column is missing from the training data")
    if eval_batch is not None and eval_batch.E > 0 and not eval_batch.has_label:
        raise SweepError("the validation data carries no labels: the sweep has nothing to compare")
    tp = model._pack(solver, train_batch)
    vp = coef_pos = has_model = labels = None
    if eval_batch is not None and eval_batch.E > 0:
        vp = model._pack(solver, eval_batch)
        coef_pos, has_model = solver.join_features(vp, tp, train_entity_map(eval_batch.entity_ids, train_batch.entity_ids))
        labels = vp._raw_dev["y"]
    K = len(weights)
    chunk = models_per_chunk(t, solver.device, K, 8 * tp.P + 4 * (0 if vp is None else vp.N) + 1)      # coefficients, and scores next to the batch
    base = solver.alloc_result(tp, variance=False)
    opts0 = model._solver_options()
    for first in range(0, K, chunk):
        thetas = []
        for w in weights[first:first + chunk]:
            out = dict(base, theta_thr=t.empty(tp.P, dtype=t.float64, device=solver.device))
            _solve(model, solver, tp, dataclasses.replace(opts0, l2=float(w), variance_mode=VAR_NONE), out)
            thetas.append(out["theta_thr"])
        if vp is None:
            continue
        logit, _ = solver.score_models(vp, thetas, coef_pos, has_model, per_coord=False, slot_major=slot_major)
        for j in range(len(thetas)):
            evaluators[first + j].add(logit[j], labels)


def run(driver, schema_params):
    """Pass 1 for the driver's partitions; sets the winner's weight on the model. -> (best index, best weight)."""
    from . import metrics
    from .io.metadata import DatasetMetadata, read_json_file
    model = driver.model
    mp = model.model_params
    weights = mp.l2_grid()
    validate(model, driver.execution_context)
    metric = metrics.metric_of_loss(model.loss)
    logger.info(f"sweeping l2_reg_weight over {list(weights)} by validation {metric}; --l2_reg_weight={mp.l2_reg_weight} is ignored")
    tensor_metadata = DatasetMetadata(read_json_file(model.metadata_file))
    num_features = 1 if model.feature_bag_name is None else tensor_metadata.get_feature_shape(model.feature_bag_name)[0]
    todo = []
    for p in driver._get_partition_list():
        tdir = driver._anchor_directory(model.training_data_dir, p)
        vdir = driver._anchor_directory(model.validation_data_dir, p)
        if os.path.isdir(tdir) and os.listdir(tdir):
            todo.append((tdir, vdir if os.path.isdir(vdir) and os.listdir(vdir) else None))
    solver = model._get_solver()
    evaluators = [metrics.DeviceEvaluator(solver) for _ in weights]
    from concurrent.futures import ThreadPoolExecutor
    read = lambda d: None if d is None else model._read_ahead(d, tensor_metadata, schema_params, num_features)
    with ThreadPoolExecutor(max_workers=2, thread_name_prefix="gdmix-sweep-read") as pool:     # the next partition is decoded while this one is solved
        ahead = [pool.submit(read, d) for d in todo[0]] if todo else None
        for i in range(len(todo)):
            train_batch, eval_batch = (f.result() for f in ahead)
            ahead = [pool.submit(read, d) for d in todo[i + 1]] if i + 1 < len(todo) else None
            if train_batch.E > 0:
                sweep_partition(model, solver, train_batch, eval_batch, weights, evaluators)
            del train_batch, eval_batch
    best = conclude(mp.metric_output_dir, metric, weights, [ev.finish() for ev in evaluators])
    mp.l2_reg_weight = float(weights[best])
    return best, weights[best]
