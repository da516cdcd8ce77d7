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


def metric_of_loss(loss) -> str:
    """The stage metric of a loss name of solver.LOSS_CODES."""
    return {"logistic": AUC, "squared": MSE, "poisson": POISSON_LOSS}[loss]


def poisson_loss_terms(score, label) -> np.ndarray:
    """The host statement of the device's Poisson-loss terms: exp(s) - y s in fp64, the fp32 score and label widened first. It states the
    definition (tests add the terms up with math.fsum); it does not evaluate a stage."""
    s = np.asarray(score, np.float32).astype(np.float64)
    return np.exp(s) - np.asarray(label, np.float32).astype(np.float64) * s
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
    batch, `add` ... `finish` over everything a stage scores."""
    OUTPUTS = (("pl", "float64"), ("n", "int32"), ("n_nan", "int32"))
    OUT_STRUCT = _solver._EvalPlOut
    SUMMARY_KEYS = POISSON_SUMMARY_KEYS
    ENTITY_SCHEMA = PER_ENTITY_POISSON_SCHEMA
    to_host = staticmethod(poisson_entities_to_host)

    def __init__(self, solver):
        super().__init__(solver)
        self._state = self.torch.empty(_solver.EVAL_PL_STATE_BYTES, dtype=self.torch.uint8, device=solver.device)
        self._acc = _solver._EvalPlAcc(self._state.data_ptr(), 0)
        self.reset()

    def entities(self, packed_or_ent_row_ptr, score, label=None) -> dict:
        """-> {"pl" float64, "n", "n_nan" int32}: device tensors, one entry per entity (n: the samples whose score is not NaN)."""
        s = self.solver
        rp, score, label, E, N, res, c_out = self._entities_args(packed_or_ent_row_ptr, score, label)
        with s._ctx_lock:
            _solver._check(self.lib.gdmix_re_eval_pl_entities(s._h, rp.data_ptr(), E, N, score.data_ptr() if N else None, label.data_ptr() if N else None,
                                                              C.byref(c_out), s._stream()), "gdmix_re_eval_pl_entities")
        return res

    def reset(self):
        s = self.solver
        with s._ctx_lock:
            _solver._check(self.lib.gdmix_re_eval_pl_acc_reset(s._h, C.byref(self._acc), s._stream()), "gdmix_re_eval_pl_acc_reset")

    def add(self, score, label):
        score, label, N = self._pair(score, label)
        if N == 0:
            return
        s = self.solver
        with s._ctx_lock:
            _solver._check(self.lib.gdmix_re_eval_pl_acc_add(s._h, C.byref(self._acc), score.data_ptr(), label.data_ptr(), N, s._stream()),
                           "gdmix_re_eval_pl_acc_add")

    def finish(self) -> dict:
        """-> {"poisson_loss", "pl", "n", "n_nan"}: the mean (NaN when a score was NaN or nothing was added), the sum over the scores that
        are not NaN, every sample added, the NaN scores. The accumulator stays as it is: more batches may follow."""
        s = self.solver
        tot = _solver._EvalPlTotals()
        with s._ctx_lock:
            _solver._check(self.lib.gdmix_re_eval_pl_acc_finish(s._h, C.byref(self._acc), C.byref(tot), s._stream()), "gdmix_re_eval_pl_acc_finish")
        n, n_nan = int(tot.n), int(tot.n_nan)
        return {POISSON_LOSS: float("nan") if n_nan > 0 or n == 0 else float(tot.pl) / n, "pl": float(tot.pl), "n": n + n_nan, "n_nan": n_nan}


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
    One worker, one summary: workers of a multi-process job need a directory each."""

    def __init__(self, solver, out_dir, metric_name):
        self.solver, self.out_dir, self.metric = solver, out_dir, metric_name
        self.evaluator = EVALUATOR_OF_METRIC[metric_name]      # the class: it says what is summed, kept and written
        self.ev = {}
        self._warned = False

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
        return ev.to_host(ev.entities(packed, logit))

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
        fields = [(f["name"], as_type[f["type"]] if isinstance(f["type"], str) else nullable) for f in self.evaluator.ENTITY_SCHEMA["fields"][1:]]
        recs = [dict({"entityId": str(entity_ids[i])}, **{k: conv(host[k][e0 + i]) for k, conv in fields}) for i in range(e1 - e0)]
        avro.write_file(os.path.join(d, name), self.evaluator.ENTITY_SCHEMA, recs)

    def write_summary(self):
        if not self.ev:
            return None
        blocks = {}
        for which, ev in self.ev.items():
            r = ev.finish()
            blocks[which] = {k: _json_number(r[k]) for k in (self.metric,) + self.evaluator.SUMMARY_KEYS}
        top = VALIDATION if VALIDATION in blocks else TRAINING
        out = dict(blocks[top], data=top, **blocks)
        os.makedirs(self.out_dir, exist_ok=True)
        with open(os.path.join(self.out_dir, EVAL_SUMMARY_JSON), "w") as f:
            json.dump(out, f)
        return out
