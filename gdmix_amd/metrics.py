"""The stage metric on the device: exact AUC and MSE, per entity and over a whole stage (include/gdmix_re.h, "evaluation";
csrc/re_evaluate.hip). What gdmix-data's Evaluator.scala computes in a Spark job of its own, plus the AUC per entity.

The device returns integers (twoU, n_pos, n_neg, n_nan) and the fp64 sum of squared errors; the divisions are done here, from exact
integers. Unweighted, as the Evaluator is. There is no CPU fallback: the host functions below state the key and the division, they do
not evaluate.
"""
import ctypes as C
import json
import logging
import os
from fractions import Fraction

import numpy as np

from . import solver as _solver

AUC, MSE = "auc", "mse"
POISSON_LOSS = "poisson_loss"        # mean of exp(s) - y s: the metric of a poisson_regression stage (include/gdmix_re.h, "poisson evaluation")
LOGISTIC_LOSS = "logistic_loss"      # mean of the logistic loss of a score (include/gdmix_re.h, "ranking evaluation"): --evaluators=LOGISTIC_LOSS


def metric_of_loss(loss) -> str:
    """The stage metric of a loss name of solver.LOSS_CODES."""
    return {"logistic": AUC, "squared": MSE, "poisson": POISSON_LOSS}[loss]


def poisson_loss_terms(score, label) -> np.ndarray:
    """The host statement of the device's Poisson-loss terms: exp(s) - y s in fp64, the fp32 score and label widened first. It states the
    definition (tests add the terms up with math.fsum); it does not evaluate a stage."""
    s = np.asarray(score, np.float32).astype(np.float64)
    return np.exp(s) - np.asarray(label, np.float32).astype(np.float64) * s


def logistic_loss_terms(score, label) -> np.ndarray:
    """The host statement of the device's log-loss terms: log(1 + exp(s)) - [y > 0.5] s in fp64, the fp32 score widened first. It states
    the definition (tests add the terms up with math.fsum); it does not evaluate a stage."""
    s = np.asarray(score, np.float32).astype(np.float64)
    return np.logaddexp(0.0, s) - (np.asarray(label, np.float32) > 0.5) * s


EXACT_DEVICE_DIVISION = 1 << 26      # entities below this many samples: auc[e] of the device is the correctly rounded quotient


def sortable_key(score) -> np.ndarray:
    """fp32 scores -> uint32 keys that order exactly as the floats do: -0 and +0 get one key; non-negative scores get the sign bit set,
    negative ones all bits complemented. (A NaN maps to some key above +inf's; the device counts NaN scores apart.)"""
    s = np.ascontiguousarray(score, np.float32)
    b = s.view(np.uint32).copy()
    b[s == 0.0] = 0
    neg = (b & np.uint32(0x80000000)) != 0
    return np.where(neg, ~b, b | np.uint32(0x80000000)).astype(np.uint32)


def auc_from_counts(two_u, n_pos, n_neg) -> float:
    """twoU / (2 n_pos n_neg) from exact integers, correctly rounded; NaN when one class is missing."""
    two_u, n_pos, n_neg = int(two_u), int(n_pos), int(n_neg)
    if n_pos == 0 or n_neg == 0:
        return float("nan")
    return float(Fraction(two_u, 2 * n_pos * n_neg))


def entities_to_host(res) -> dict:
    """The tensors of DeviceEvaluator.entities -> numpy arrays, with `n`, `mse` (sse / n, NaN for an entity without samples or with a
    NaN score) and `auc` (NaN with a NaN score; entities of 2^26 samples or more get the division from exact integers)."""
    h = {k: _solver.host_array(v) for k, v in res.items()}
    n_pos, n_neg, n_nan = h["n_pos"].astype(np.int64), h["n_neg"].astype(np.int64), h["n_nan"]
    n = n_pos + n_neg
    auc = h["auc"].copy()
    for e in np.flatnonzero(n >= EXACT_DEVICE_DIVISION):
        auc[e] = auc_from_counts(h["two_u"][e], n_pos[e], n_neg[e])
    with np.errstate(divide="ignore", invalid="ignore"):
        mse = h["sse"] / n.astype(np.float64)
    mse[n == 0] = np.nan
    auc[n_nan > 0] = np.nan
    mse[n_nan > 0] = np.nan
    h.update(n=n + n_nan, auc=auc, mse=mse)
    return h


def precision_from_counts(hits_sure, slots, tie_pos, tie_size, k) -> float:
    """precision@k = (hits_sure + slots tie_pos / tie_size) / k from the device's exact integers, correctly rounded (the tie term is 0
    when tie_size is 0): the expected share of positives among the k best under a uniformly random order inside tie groups."""
    hits_sure, slots, tie_pos, tie_size, k = int(hits_sure), int(slots), int(tie_pos), int(tie_size), int(k)
    if k < 1:
        raise ValueError(f"precision@{k}: k is at least 1")
    h = Fraction(hits_sure) + (Fraction(slots * tie_pos, tie_size) if tie_size else 0)
    return float(h / k)


def precision_key(k) -> str:
    """The per-entity field of precision@k (an Avro name)."""
    return f"precision_at_{int(k)}"


def ranking_entities_to_host(res, ks) -> dict:
    """The tensors of RankingEvaluator.entities -> numpy arrays: what entities_to_host gives, the four [nk, E] integer arrays, and per k
    `precision_at_<k>` [E] float64 — one fp64 division of exactly converted int64 numerator and denominator (exact for entities below
    2^26 samples: with ties n > k, so both stay below 2^53; larger entities go through Fraction). NaN with a NaN score, as auc is."""
    counts = ("hits_sure", "slots", "tie_pos", "tie_size")
    h = entities_to_host({k: v for k, v in res.items() if k not in counts})
    c = {k: _solver.host_array(res[k]).astype(np.int64) for k in counts}
    h.update({k: c[k].astype(np.int32) for k in counts})
    big = np.flatnonzero(h["n"] >= EXACT_DEVICE_DIVISION)
    for j, k in enumerate(ks):
        hs, sl, tp, ts = (c[name][j] for name in counts)
        tied = ts > 0
        num = np.where(tied, hs * ts + sl * tp, hs).astype(np.float64)
        den = np.where(tied, ts * np.int64(k), np.int64(k)).astype(np.float64)
        p = num / den
        for e in big:
            p[e] = precision_from_counts(hs[e], sl[e], tp[e], ts[e], k)
        p[h["n_nan"] > 0] = np.nan
        h[precision_key(k)] = p
    return h


def poisson_entities_to_host(res) -> dict:
    """The tensors of PoissonEvaluator.entities -> numpy arrays, with `n` (every sample, NaN scores included) and `poisson_loss`
    (pl / n, NaN for an entity without samples or with a NaN score)."""
    h = {k: _solver.host_array(v) for k, v in res.items()}
    n, n_nan = h["n"].astype(np.int64), h["n_nan"].astype(np.int64)
    with np.errstate(divide="ignore", invalid="ignore"):
        mean = h["pl"] / n.astype(np.float64)
    mean[(n == 0) | (n_nan > 0)] = np.nan
    h.update(n=n + n_nan, poisson_loss=mean)
    return h


# what a stage writes per evaluator (StageMetrics): the summary's keys next to the metric, and the per-entity records
PER_ENTITY_SCHEMA = {"type": "record", "name": "EntityMetricAvro", "namespace": "gdmix_amd", "fields": [
    {"name": "entityId", "type": "string"}, {"name": "n", "type": "long"}, {"name": "n_pos", "type": "long"},
    {"name": "auc", "type": ["null", "double"]}, {"name": "mse", "type": "double"}]}
PER_ENTITY_POISSON_SCHEMA = {"type": "record", "name": "EntityPoissonMetricAvro", "namespace": "gdmix_amd", "fields": [
    {"name": "entityId", "type": "string"}, {"name": "n", "type": "long"}, {"name": "poisson_loss", "type": "double"}]}
def ranking_entity_schema(ks) -> dict:
    """PER_ENTITY_SCHEMA with one nullable double per requested k behind it (null: a NaN score in the entity)."""
    return dict(PER_ENTITY_SCHEMA, fields=PER_ENTITY_SCHEMA["fields"] + [{"name": precision_key(k), "type": ["null", "double"]} for k in ks])


SUMMARY_KEYS = ("n", "n_pos", "n_neg", "n_nan", "two_u", "sse")
POISSON_SUMMARY_KEYS = ("n", "n_nan", "pl")


class _Evaluator:
    """What the evaluators share: the checks of their inputs. Each declares OUTPUTS (name and dtype of `entities`' tensors, in the order
    of its C struct OUT_STRUCT), SUMMARY_KEYS and ENTITY_SCHEMA (what a stage writes from `finish`, next to its metric, and per entity) and `to_host`."""

    def __init__(self, solver):
        self.solver = solver
        self.torch = solver.torch
        self.lib = solver.lib

    def _f32(self, x, what):
        t = self.torch
        if isinstance(x, np.ndarray):
            x = t.from_numpy(np.ascontiguousarray(x, np.float32)).to(self.solver.device)
        if not x.is_cuda or x.dtype != t.float32 or not x.is_contiguous():
            raise _solver.GdmixReError(f"{what} must be a contiguous float32 array on the solver's device")
        return x

    def _pair(self, score, label):
        """-> (score, label, N), checked"""
        score, label = self._f32(score, "score"), self._f32(label, "label")
        N = int(score.numel())
        if label.numel() != N:
            raise _solver.GdmixReError("score and label differ in length")
        return score, label, N

    def set_small_max(self, small_max: int):
        """Testing knob: entities of more than small_max samples take the path of the large ones (the sort path; for the Poisson loss a
        workgroup each). 0: every entity. Default 64."""
        with self.solver._ctx_lock:
            _solver._check(self.lib.gdmix_re_set_eval_small_max(self.solver._h, int(small_max)), "gdmix_re_set_eval_small_max")

    def _entities_args(self, packed_or_ent_row_ptr, score, label):
        """`entities`' arguments, checked -> (ent_row_ptr, score, label, E, N, the zeroed output tensors, their C struct).
        packed_or_ent_row_ptr: a PackedBatch (its labels are the default for `label`) or the [E+1] int64 sample offsets."""
        t, s = self.torch, self.solver
        if isinstance(packed_or_ent_row_ptr, _solver.PackedBatch):
            pb = packed_or_ent_row_ptr
            rp = pb._raw_dev["ent_row_ptr"]
            if label is None:
                label = pb._raw_dev["y"]
        else:
            rp = packed_or_ent_row_ptr
            if isinstance(rp, np.ndarray):
                rp = t.from_numpy(np.ascontiguousarray(rp, np.int64)).to(s.device)
        if label is None:
            raise _solver.GdmixReError("entities: no labels")
        if not rp.is_cuda or rp.dtype != t.int64 or rp.numel() < 1:
            raise _solver.GdmixReError("ent_row_ptr must be int64 on the solver's device, one entry more than entities")
        score, label, N = self._pair(score, label)
        E = int(rp.numel()) - 1
        if E > 0 and (int(rp[0]) != 0 or int(rp[-1]) != N):
            raise _solver.GdmixReError(f"ent_row_ptr runs from {int(rp[0])} to {int(rp[-1])}; the batch has {N} samples")
        res = {k: t.zeros(E, dtype=getattr(t, dtype), device=s.device) for k, dtype in self.OUTPUTS}
        return rp, score, label, E, N, res, self.OUT_STRUCT(*(res[k].data_ptr() if E else None for k, _ in self.OUTPUTS))

    @property
    def count(self) -> int:
        return int(self._acc.count)


class PoissonEvaluator(_Evaluator):
    """The Poisson loss on one MI355X through the solver's context, with DeviceEvaluator's interface: `entities` per entity of a scored
    batch, `add` ... `finish` over everything a stage scores. (LogLossEvaluator below is this class over the other family of entry
    points: FAMILY names it, METRIC the mean `finish` reports.)"""
    OUTPUTS = (("pl", "float64"), ("n", "int32"), ("n_nan", "int32"))
    OUT_STRUCT = _solver._EvalPlOut
    SUMMARY_KEYS = POISSON_SUMMARY_KEYS
    ENTITY_SCHEMA = PER_ENTITY_POISSON_SCHEMA
    to_host = staticmethod(poisson_entities_to_host)
    FAMILY, METRIC, SUM = "gdmix_re_eval_pl", POISSON_LOSS, "pl"

    def __init__(self, solver):
        super().__init__(solver)
        self._state = self.torch.empty(_solver.EVAL_PL_STATE_BYTES, dtype=self.torch.uint8, device=solver.device)
        self._acc = _solver._EvalPlAcc(self._state.data_ptr(), 0)
        self.reset()

    def _fn(self, call):
        return getattr(self.lib, f"{self.FAMILY}_{call}")

    def entities(self, packed_or_ent_row_ptr, score, label=None) -> dict:
        """-> {"pl" float64, "n", "n_nan" int32}: device tensors, one entry per entity (n: the samples whose score is not NaN)."""
        s = self.solver
        rp, score, label, E, N, res, c_out = self._entities_args(packed_or_ent_row_ptr, score, label)
        with s._ctx_lock:
            _solver._check(self._fn("entities")(s._h, rp.data_ptr(), E, N, score.data_ptr() if N else None, label.data_ptr() if N else None,
                                                              C.byref(c_out), s._stream()), self.FAMILY + "_entities")
        return res

    def reset(self):
        s = self.solver
        with s._ctx_lock:
            _solver._check(self._fn("acc_reset")(s._h, C.byref(self._acc), s._stream()), self.FAMILY + "_acc_reset")

    def add(self, score, label):
        score, label, N = self._pair(score, label)
        if N == 0:
            return
        s = self.solver
        with s._ctx_lock:
            _solver._check(self._fn("acc_add")(s._h, C.byref(self._acc), score.data_ptr(), label.data_ptr(), N, s._stream()),
                           self.FAMILY + "_acc_add")

    def finish(self) -> dict:
        """-> {"poisson_loss", "pl", "n", "n_nan"}: the mean (NaN when a score was NaN or nothing was added), the sum over the scores that
        are not NaN, every sample added, the NaN scores. The accumulator stays as it is: more batches may follow."""
        s = self.solver
        tot = _solver._EvalPlTotals()
        with s._ctx_lock:
            _solver._check(self._fn("acc_finish")(s._h, C.byref(self._acc), C.byref(tot), s._stream()), self.FAMILY + "_acc_finish")
        n, n_nan = int(tot.n), int(tot.n_nan)
        return {self.METRIC: float("nan") if n_nan > 0 or n == 0 else float(tot.pl) / n, self.SUM: float(tot.pl), "n": n + n_nan, "n_nan": n_nan}


def logloss_entities_to_host(res) -> dict:
    """The tensors of LogLossEvaluator.entities -> numpy arrays, with `n` (every sample, NaN scores included) and `logistic_loss`
    (ll / n, NaN for an entity without samples or with a NaN score)."""
    h = poisson_entities_to_host(res)
    h[LOGISTIC_LOSS] = h.pop(POISSON_LOSS)
    h["ll"] = h["pl"]
    return h


class LogLossEvaluator(PoissonEvaluator):
    """The logistic loss of (score, label) on the device, with PoissonEvaluator's interface (include/gdmix_re.h, "ranking evaluation": the
    gdmix_re_eval_ll_ entry points share the Poisson family's structs, so `entities` returns the per-entity sums under "pl"; `finish`
    -> {"logistic_loss", "ll", "n", "n_nan"})."""
    SUMMARY_KEYS = ("n", "n_nan", "ll")
    ENTITY_SCHEMA = None
    to_host = staticmethod(logloss_entities_to_host)
    FAMILY, METRIC, SUM = "gdmix_re_eval_ll", LOGISTIC_LOSS, "ll"


class DeviceEvaluator(_Evaluator):
    """AUC / MSE on one MI355X through the solver's context: `entities` per entity of a scored batch, `add` ... `finish` over everything
    a stage scores (one accumulator per object; a solver may serve several)."""
    OUTPUTS = (("two_u", "int64"), ("n_pos", "int32"), ("n_neg", "int32"), ("n_nan", "int32"), ("sse", "float64"), ("auc", "float64"))
    OUT_STRUCT = _solver._EvalOut
    SUMMARY_KEYS = SUMMARY_KEYS
    ENTITY_SCHEMA = PER_ENTITY_SCHEMA
    to_host = staticmethod(entities_to_host)

    def __init__(self, solver):
        super().__init__(solver)
        self._keys = None       # device int64 tensor behind the accumulator's uint64 keys
        self._state = None      # the accumulator's device state
        self._acc = _solver._EvalAcc(None, 0, 0, None)
        self.reset()

    # ---- per entity ----------------------------------------------------------------------------------------------------------------
    def entities(self, packed_or_ent_row_ptr, score, label=None, workspace_bytes=None) -> dict:
        """-> {"two_u" int64, "n_pos", "n_neg", "n_nan" int32, "sse", "auc" float64}: device tensors, one entry per entity.
        packed_or_ent_row_ptr: a PackedBatch (its labels are the default for `label`) or the [E+1] int64 sample offsets."""
        t, s = self.torch, self.solver
        rp, score, label, E, N, res, c_out = self._entities_args(packed_or_ent_row_ptr, score, label)
        nbytes = int(self.lib.gdmix_re_eval_workspace_bytes(E, N)) if workspace_bytes is None else int(workspace_bytes)
        ws = t.empty(max(nbytes, 1), dtype=t.uint8, device=s.device)
        with s._ctx_lock:
            _solver._check(self.lib.gdmix_re_eval_entities(s._h, rp.data_ptr(), E, N, score.data_ptr() if N else None, label.data_ptr() if N else None,
                                                           C.byref(c_out), ws.data_ptr(), nbytes, s._stream()), "gdmix_re_eval_entities")
        return res

    # ---- a whole stage -------------------------------------------------------------------------------------------------------------
    def reset(self):
        t, s = self.torch, self.solver
        if self._state is None:
            self._state = t.empty(_solver.EVAL_ACC_STATE_BYTES, dtype=t.uint8, device=s.device)
            self._acc.state = self._state.data_ptr()
        with s._ctx_lock:
            _solver._check(self.lib.gdmix_re_eval_acc_reset(s._h, C.byref(self._acc), s._stream()), "gdmix_re_eval_acc_reset")

    def reserve(self, samples: int):
        """Room for this many samples in the key buffer (8 bytes each). `add` grows it by itself; a stage that knows its size saves
        the copies."""
        t = self.torch
        if self._keys is None or self._keys.numel() < samples:
            new = t.empty(int(samples), dtype=t.int64, device=self.solver.device)
            if self._keys is not None and self.count:
                new[:self.count].copy_(self._keys[:self.count])
            self._keys = new
            self._acc.keys, self._acc.capacity = new.data_ptr(), int(new.numel())

    def add(self, score, label):
        score, label, N = self._pair(score, label)
        if N == 0:
            return
        if self._keys is None or self._keys.numel() < self.count + N:
            self.reserve(max(self.count + N, 2 * (self._keys.numel() if self._keys is not None else 0)))
        s = self.solver
        with s._ctx_lock:
            _solver._check(self.lib.gdmix_re_eval_acc_add(s._h, C.byref(self._acc), score.data_ptr(), label.data_ptr(), N, s._stream()),
                           "gdmix_re_eval_acc_add")

    def finish(self) -> dict:
        """-> {"auc", "mse", "n", "n_pos", "n_neg", "n_nan", "two_u", "sse"}; AUC and MSE are NaN when a score was NaN. The accumulator
        stays as it is: more batches may follow."""
        t, s = self.torch, self.solver
        nbytes = int(self.lib.gdmix_re_eval_acc_workspace_bytes(self.count))
        ws = t.empty(max(nbytes, 1), dtype=t.uint8, device=s.device)
        tot = _solver._EvalTotals()
        with s._ctx_lock:
            _solver._check(self.lib.gdmix_re_eval_acc_finish(s._h, C.byref(self._acc), ws.data_ptr(), nbytes, C.byref(tot), s._stream()),
                           "gdmix_re_eval_acc_finish")
        n_pos, n_neg, n_nan = int(tot.n_pos), int(tot.n_neg), int(tot.n_nan)
        n = n_pos + n_neg
        bad = n_nan > 0
        return {"auc": float("nan") if bad else auc_from_counts(tot.two_u, n_pos, n_neg),
                "mse": float("nan") if bad or n == 0 else float(tot.sse) / n,
                "n": int(tot.n), "n_pos": n_pos, "n_neg": n_neg, "n_nan": n_nan, "two_u": int(tot.two_u), "sse": float(tot.sse)}


class RankingEvaluator(_Evaluator):
    """precision@k per entity for up to four k, and DeviceEvaluator's per-entity outputs, from ONE device call and one sort
    (gdmix_re_eval_topk_entities). ks: distinct integers >= 1."""
    COUNTS = ("hits_sure", "slots", "tie_pos", "tie_size")
    OUTPUTS = DeviceEvaluator.OUTPUTS
    OUT_STRUCT = _solver._EvalOut

    def __init__(self, solver, ks):
        super().__init__(solver)
        self.ks = tuple(int(k) for k in ks)
        if not 1 <= len(self.ks) <= _solver.EVAL_TOPK_MAX or len(set(self.ks)) != len(self.ks) or min(self.ks) < 1 or max(self.ks) >= 1 << 31:
            raise _solver.GdmixReError(f"RankingEvaluator: ks = {list(ks)}; 1 .. {_solver.EVAL_TOPK_MAX} distinct integers, each in [1, 2^31)")

    def to_host(self, res):
        return ranking_entities_to_host(res, self.ks)

    def entities(self, packed_or_ent_row_ptr, score, label=None, workspace_bytes=None, with_auc=True) -> dict:
        """-> {"hits_sure", "slots", "tie_pos", "tie_size": int32 [nk, E]} and, with_auc, DeviceEvaluator.entities' tensors: all on the
        device."""
        t, s = self.torch, self.solver
        rp, score, label, E, N, res, c_auc = self._entities_args(packed_or_ent_row_ptr, score, label)
        nk = len(self.ks)
        counts = {k: t.zeros((nk, E), dtype=t.int32, device=s.device) for k in self.COUNTS}
        c_out = _solver._EvalTopkOut(*(counts[k].data_ptr() if E else None for k in self.COUNTS))
        c_ks = (C.c_int32 * nk)(*self.ks)
        nbytes = int(self.lib.gdmix_re_eval_topk_workspace_bytes(E, N)) if workspace_bytes is None else int(workspace_bytes)
        ws = t.empty(max(nbytes, 1), dtype=t.uint8, device=s.device)
        with s._ctx_lock:
            _solver._check(self.lib.gdmix_re_eval_topk_entities(s._h, rp.data_ptr(), E, N, score.data_ptr() if N else None, label.data_ptr() if N else None,
                                                                c_ks, nk, C.byref(c_out), C.byref(c_auc) if with_auc else None, ws.data_ptr(), nbytes,
                                                                s._stream()), "gdmix_re_eval_topk_entities")
        return dict(res, **counts) if with_auc else counts


EVALUATOR_OF_METRIC = {AUC: DeviceEvaluator, MSE: DeviceEvaluator, POISSON_LOSS: PoissonEvaluator}


# ---- a stage that reports its metric while it scores (REParams.metric_output_dir) ----------------------------------------------------
EVAL_SUMMARY_JSON = "evalSummary.json"
PER_ENTITY_DIR = "perEntity"
TRAINING, VALIDATION = "training", "validation"

logger = logging.getLogger(__name__)


def _json_number(x):
    return None if isinstance(x, float) and x != x else x      # NaN is not JSON


class StageMetrics:
    """What a random-effect stage keeps when it is asked for its metric: one accumulator for its training scores (active and passive)
    and one for its validation scores, fed with the scores while they are still in HBM, and the per-entity files of every scored
    partition. Layout under `out_dir`:
        evalSummary.json          {"<metric>": value, "n", "n_pos", "n_neg", "n_nan", "two_u", "sse", "data": "validation" | "training",
                                   "training": {the same keys}, "validation": {...}} — the top level repeats the validation block
                                   (the data the workflow's evaluator reads), or the training block of a stage without validation data
        perEntity/part-<data>-<partition directory>-<score file>.avro     records {entityId, n, n_pos, auc (null: one class), mse}
    A Poisson stage (metric "poisson_loss"): the summary's keys are {"poisson_loss", "n", "n_nan", "pl"}, the records {entityId, n, poisson_loss}.
    One worker, one summary: workers of a multi-process job need a directory each.
    With `spec` (--evaluators; params.EvaluatorSpec) every block of the summary gains
        "logistic_loss", "ll"                                  the mean and the sum of the logistic loss (LogLossEvaluator)
        "auc:<id>", "auc:<id>_records"                         the mean of auc over the per-entity RECORDS (what write_entities wrote for
                                                               that data: an entity with active and passive training data has two or more) that
                                                               have both classes, and how many those are
        "precision@K:<id>", "precision@K:<id>_records"         the mean of precision@K over the records with a sample, per requested K
    and the records one nullable double precision_at_K per K. Each mean is math.fsum of the records' values over their number: the sum is
    exact, so the value depends on no order or grouping of partitions. Any record with a NaN score makes it NaN (null), as the stage
    metric. Without `spec` every file is byte for byte what it was."""

    def __init__(self, solver, out_dir, metric_name, spec=None):
        self.solver, self.out_dir, self.metric = solver, out_dir, metric_name
        self.evaluator = EVALUATOR_OF_METRIC[metric_name]      # the class: it says what is summed, kept and written
        self.ev = {}
        self._warned = False
        self.spec = spec
        self.entity_schema = self.evaluator.ENTITY_SCHEMA
        self.ll = {}             # which -> LogLossEvaluator (spec.log_loss)
        self.ranking = None      # RankingEvaluator (spec.ranking): one device call gives the per-entity AUC outputs and precision@k
        self.records = {}        # which -> {"nan": records with a NaN score, "auc": [values], precision_key(k): [values]}
        if spec is not None and spec.ranking:
            self.ks = spec.ks if spec.ks else (1,)      # AUC:<id> alone still takes the one call; its k is not reported
            self.entity_schema = ranking_entity_schema(spec.ks)

    def add_log_loss(self, which, score, label):
        """--evaluators=LOGISTIC_LOSS: the scores of a batch (device) -> `which`'s log-loss accumulator. Nothing without it."""
        if self.spec is None or not self.spec.log_loss:
            return
        if which not in self.ll:
            self.ll[which] = LogLossEvaluator(self.solver)
        self.ll[which].add(score, label)

    def _evaluator(self, which):
        if which not in self.ev:
            self.ev[which] = self.evaluator(self.solver)
        return self.ev[which]

    def no_labels(self, what):
        if not self._warned:
            logger.info(f"{what} carries no labels: no metric is written to {self.out_dir}")
            self._warned = True

    def feed(self, which, packed, logit):
        """The scores of a packed batch (device) -> added to `which`'s accumulator; -> per-entity results on the host."""
        ev = self._evaluator(which)
        ev.add(logit, packed._raw_dev["y"])
        self.add_log_loss(which, logit, packed._raw_dev["y"])
        if self.spec is not None and self.spec.ranking:
            if self.ranking is None:
                self.ranking = RankingEvaluator(self.solver, self.ks)
            return self.ranking.to_host(self.ranking.entities(packed, logit))
        return ev.to_host(ev.entities(packed, logit))

    def _collect(self, which, host, e0, e1):
        """The records just written -> the values the aggregates of `which` are taken over."""
        r = self.records.setdefault(which, dict({"nan": 0, "auc": []}, **{precision_key(k): [] for k in self.spec.ks}))
        sl = slice(e0, e1)
        r["nan"] += int(np.count_nonzero(host["n_nan"][sl] > 0))
        both = (host["n_pos"][sl] > 0) & (host["n_neg"][sl] > 0) & (host["n_nan"][sl] == 0)
        r["auc"].extend(host["auc"][sl][both].tolist())
        some = (host["n"][sl] >= 1) & (host["n_nan"][sl] == 0)
        for k in self.spec.ks:
            r[precision_key(k)].extend(host[precision_key(k)][sl][some].tolist())

    def write_entities(self, which, output_file, entity_ids, host, e0=0, e1=None):
        from .io import avro
        e1 = len(entity_ids) + e0 if e1 is None else e1
        d = os.path.join(self.out_dir, PER_ENTITY_DIR)
        os.makedirs(d, exist_ok=True)
        stem = os.path.basename(output_file)
        stem = stem[len("part-"):] if stem.startswith("part-") else stem
        name = f"part-{which}-{os.path.basename(os.path.dirname(os.path.abspath(output_file)))}-{stem}"
        # a record per entity from the evaluator's schema: a long, a double, or a double that is null when it is NaN
        as_type = {"long": int, "double": float}
        nullable = lambda x: None if x != x else float(x)
        fields = [(f["name"], as_type[f["type"]] if isinstance(f["type"], str) else nullable) for f in self.entity_schema["fields"][1:]]
        recs = [dict({"entityId": str(entity_ids[i])}, **{k: conv(host[k][e0 + i]) for k, conv in fields}) for i in range(e1 - e0)]
        avro.write_file(os.path.join(d, name), self.entity_schema, recs)
        if self.spec is not None and self.spec.ranking:
            self._collect(which, host, e0, e1)

    def _aggregates(self, which) -> dict:
        """The block's keys of --evaluators for `which` (in a fixed order: the log loss, the mean AUC, precision@k as listed)."""
        import math
        out = {}
        if self.spec.log_loss and which in self.ll:
            r = self.ll[which].finish()
            out[LOGISTIC_LOSS], out["ll"] = _json_number(r[LOGISTIC_LOSS]), r["ll"]
        if self.spec.ranking:
            r = self.records.get(which, {"nan": 0, "auc": []})
            mean = lambda v: None if r["nan"] > 0 or not v else math.fsum(v) / len(v)
            if self.spec.auc:
                out[f"auc:{self.spec.entity}"], out[f"auc:{self.spec.entity}_records"] = mean(r["auc"]), len(r["auc"])
            for k in self.spec.ks:
                v = r.get(precision_key(k), [])
                out[f"precision@{k}:{self.spec.entity}"], out[f"precision@{k}:{self.spec.entity}_records"] = mean(v), len(v)
        return out

    def write_summary(self):
        if not self.ev:
            return None
        blocks = {}
        for which, ev in self.ev.items():
            r = ev.finish()
            blocks[which] = {k: _json_number(r[k]) for k in (self.metric,) + self.evaluator.SUMMARY_KEYS}
            if self.spec is not None:
                blocks[which].update(self._aggregates(which))
        top = VALIDATION if VALIDATION in blocks else TRAINING
        out = dict(blocks[top], data=top, **blocks)
        os.makedirs(self.out_dir, exist_ok=True)
        with open(os.path.join(self.out_dir, EVAL_SUMMARY_JSON), "w") as f:
            json.dump(out, f)
        return out
