"""Block coordinate descent with the coordinates resident on the device: several passes over (global fixed effect, per-entity random
effects, ...), every coordinate fitted against the scores of all the others (Photon-ML's coordinateDescentIterations).

gdmix_amd/chain.py runs the FIRST pass through the stages' files: every stage uploads, packs, solves and writes Avro scores, and a host
partition job regroups the rows for the next stage. Here a coordinate is uploaded, grouped by entity ON THE DEVICE
(include/gdmix_re.h, "row grouping"; csrc/re_group.hip) and packed ONCE. An update of coordinate c then
    1. rewrites the offset array its packed batch aliases:  offset = base + sum of the other coordinates' contributions, in its row order
       (gdmix_re_offsets_combine: fp32, left to right, the order the file chain's Avro `float` scores imply),
    2. solves, warm-started from its own previous coefficients (the first pass: the cold solve a stage makes, so one pass reproduces
       chain.run_chain without upper bounds; a fixed effect is re-armed with gdmix_fe_restart — nothing derived from the offsets is kept
       by gdmix_fe_create, csrc/fe_solve.hip reads them through the shard's pointer at every evaluation),
    3. scores the THRESHOLDED model and scatters its per-coordinate score back to sample order (contribution s_c [N], fp32).
After every update the stage metric (metrics.metric_of_loss: AUC / MSE / Poisson loss) of the accumulated score is taken with the
device evaluators, on training and validation data. The accumulated score after an update is the score the stage would write: the
updated coordinate's own score of its rows, float32(x . theta + offset) with the sum taken in fp64 (gdmix_re_score's logit; a fixed
effect: float32 of per-coordinate score + offset), not the fp32 sum of the contributions, which rounds x . theta first.

The grouping and the offset sum are stated in numpy below (group_rows_host, rows_gather_host, rows_scatter_host, offsets_combine_host):
the definitions the device kernels are held to, bit for bit.

Out of scope: several GPUs; active-data upper bounds; the per-stage options (--l2_reg_weights, incremental training, feature
normalisation, L1 / TRON / box constraints); a CLI over TFRecord inputs (tools/chain_demo.py --resident runs the synthetic MovieLens
shape). chain.run_chain, every stage's files, refusals and loss codes are what they were.
"""
import os
from dataclasses import dataclass, field
from typing import Optional

import numpy as np

from .constants import LINEAR_REGRESSION, LOGISTIC_REGRESSION, POISSON_REGRESSION

MAX_COORDINATES = 8      # GDMIX_RE_COMBINE_MAX: the parts one gdmix_re_offsets_combine call adds up
LOSS_OF_MODEL_TYPE = {LOGISTIC_REGRESSION: "logistic", LINEAR_REGRESSION: "squared", POISSON_REGRESSION: "poisson"}


# ---- the numpy statements ------------------------------------------------------------------------------------------------------------
def group_rows_host(row_nnz_ptr, col_global, val, entity_index, E):
    """What gdmix_re_group_rows computes (include/gdmix_re.h, "row grouping"). entity_index [N]: values in [0, E), anything else (-1) is a
    row of no entity. -> dict(row_of [N'] int32, present [E'] int32, ent_row_ptr [E' + 1] int64, row_nnz_ptr [N' + 1] int64,
    col_global [Z'] int64, val [Z'] float32, counts)."""
    ptr = np.asarray(row_nnz_ptr, np.int64)
    col, vl = np.asarray(col_global, np.int64), np.asarray(val, np.float32)
    idx = np.asarray(entity_index, np.int64)
    keep = np.flatnonzero((idx >= 0) & (idx < int(E)))
    row_of = keep[np.argsort(idx[keep], kind="stable")]
    present, counts = np.unique(idx[row_of], return_counts=True)
    k = np.diff(ptr)[row_of]
    out_ptr = np.concatenate([[0], np.cumsum(k)]).astype(np.int64)
    nz = np.repeat(ptr[:-1][row_of] - out_ptr[:-1], k) + np.arange(int(out_ptr[-1]), dtype=np.int64)
    return dict(row_of=row_of.astype(np.int32), present=present.astype(np.int32), ent_row_ptr=np.concatenate([[0], np.cumsum(counts)]).astype(np.int64),
                row_nnz_ptr=out_ptr, col_global=col[nz], val=vl[nz],
                counts=dict(rows=int(idx.size), grouped=int(row_of.size), grouped_nnz=int(out_ptr[-1]), entities=int(present.size),
                            left_out=int(idx.size - row_of.size)))


def rows_gather_host(src, row_of):
    """dst[i] = src[row_of[i]]."""
    return np.asarray(src, np.float32)[np.asarray(row_of, np.int64)]


def rows_scatter_host(src, row_of, n_dst):
    """dst = zeros(n_dst); dst[row_of[i]] = src[i]: rows no entry of row_of names keep 0."""
    out = np.zeros(int(n_dst), np.float32)
    out[np.asarray(row_of, np.int64)] = np.asarray(src, np.float32)
    return out


def offsets_combine_host(n_src, base, parts, skip=-1, row_of=None):
    """dst[i] = base[r] + parts[0][r] + parts[1][r] + ... with parts[skip] left out, r = row_of[i] (None: i): fp32 additions from left to
    right, starting from +0.0 when there is no base."""
    r = np.arange(int(n_src), dtype=np.int64) if row_of is None else np.asarray(row_of, np.int64)
    acc = np.zeros(r.size, np.float32) if base is None else np.asarray(base, np.float32)[r].copy()
    for k, p in enumerate(parts):
        if k != skip:
            acc = (acc + np.asarray(p, np.float32)[r]).astype(np.float32)
    return acc


def joint_objective(loss, label, weight, score, models):
    """F = sum_i w_i loss(y_i, score_i) + sum_c (l2_c / 2) |theta_c restricted to its regularised entries|^2 in fp64.
    models: [(theta, regularised mask, l2)]. The tests recompute the descent's objective with it."""
    z = np.asarray(score, np.float64)
    y = np.asarray(label, np.float64)
    w = np.ones_like(z) if weight is None else np.asarray(weight, np.float64)
    if loss == "logistic":
        terms = np.logaddexp(0.0, z) - (y > 0.5) * z
    elif loss == "squared":
        terms = (y - z) ** 2      # (no half: include/gdmix_re.h, GDMIX_RE_LOSS_SQUARED)
    elif loss == "poisson":
        terms = np.exp(z) - y * z
    else:
        raise ValueError(f"unknown loss {loss!r}")
    f = float(np.sum(w * terms))
    for theta, mask, l2 in models:
        t = np.asarray(theta, np.float64)[np.asarray(mask, bool)]
        f += 0.5 * float(l2) * float(t @ t)
    return f


# ---- the public objects ----------------------------------------------------------------------------------------------------------------
@dataclass
class DataSet:
    """The per-sample columns every coordinate shares. offset: the base offset of every sample (None: 0)."""
    label: np.ndarray
    uid: np.ndarray
    weight: Optional[np.ndarray] = None
    offset: Optional[np.ndarray] = None

    @property
    def n(self):
        return int(np.asarray(self.label).size)


@dataclass
class Coordinate:
    """One block of the model. bag = (row_nnz_ptr, col, val, dim): a CSR bag over the training samples; entity [N] int64: the entity id of
    every sample (None: a fixed effect). validation_bag / validation_entity: the same over the validation samples. features: the (name,
    term) of every column, for write_models (None: ("<name>_<j>", ""))."""
    name: str
    bag: tuple
    entity: Optional[np.ndarray] = None
    l2: float = 1.0
    regularize_bias: bool = True
    has_intercept: bool = True
    validation_bag: Optional[tuple] = None
    validation_entity: Optional[np.ndarray] = None
    features: Optional[list] = None

    @property
    def random_effect(self):
        return self.entity is not None

    @property
    def dim(self):
        return int(self.bag[3])


@dataclass
class CoordinateModel:
    """A coordinate's model after the last update. Random effect: theta / theta_thr [P] in the packed batch's order (per entity: the
    intercept, then its features in ascending global index), present [E] the entity ids in that order, unique_global [D] the feature of
    every slot, coef_ptr [E + 1] each entity's slice of theta, feat_ptr [E + 1] of unique_global. Fixed effect: theta / theta_thr
    [dim + 1], the intercept last; the other arrays are None."""
    name: str
    random_effect: bool
    dim: int
    has_intercept: bool
    theta: np.ndarray
    theta_thr: np.ndarray
    present: Optional[np.ndarray] = None
    unique_global: Optional[np.ndarray] = None
    coef_ptr: Optional[np.ndarray] = None
    feat_ptr: Optional[np.ndarray] = None
    features: Optional[list] = None


@dataclass
class DescentResult:
    """history: one dict per update, in order: {"pass", "coordinate", "train_<metric>", "validation_<metric>" (with validation data),
    "max_nit", "status"} and, with record=True, "offsets" (what the update trained on, in the coordinate's row order: grouped for a random
    effect), "validation_offsets" (the other coordinates' validation contributions added up, sample order), "theta0" (where it started;
    None: cold), "theta" / "theta_thr" (where it ended), "score" / "validation_score" (the accumulated score behind the metric, sample
    order) and "contribution" (the coordinate's new s_c, sample order).
    models: {name: CoordinateModel}; contributions / validation_contributions: {name: s_c [N] float32}; row_of: {name: [N'] int32} of the
    random effects; setup_s / pass_s / update_s: host clocks around device synchronises."""
    model_type: str
    metric: str
    history: list
    models: dict
    contributions: dict
    validation_contributions: dict
    row_of: dict
    setup_s: dict = field(default_factory=dict)
    pass_s: list = field(default_factory=list)
    update_s: list = field(default_factory=list)


def _check_bag(name, bag, n, what):
    if bag is None or len(bag) != 4:
        raise ValueError(f"coordinate {name!r}: {what} is (row_nnz_ptr, col, val, dim)")
    ptr, col, val, dim = bag
    ptr = np.ascontiguousarray(ptr, np.int64)
    col, val = np.ascontiguousarray(col, np.int64), np.ascontiguousarray(val, np.float32)
    if ptr.size != n + 1:
        raise ValueError(f"coordinate {name!r}: {what} has {ptr.size - 1} rows, the data set has {n}")
    if ptr[0] != 0 or ptr[-1] != col.size or col.size != val.size or (np.diff(ptr) < 0).any():
        raise ValueError(f"coordinate {name!r}: the row pointers of {what} do not describe its {col.size} non-zeros")
    if col.size and (col.min() < 0 or col.max() >= int(dim)):
        raise ValueError(f"coordinate {name!r}: feature index outside [0, {int(dim)}) in {what}")
    return ptr, col, val, int(dim)


def check_request(train, coordinates, passes, model_type, validation=None):
    """Everything fit() refuses, before any device work (no device is needed to call it)."""
    if model_type not in LOSS_OF_MODEL_TYPE:
        raise ValueError(f"model type {model_type!r}: one of {', '.join(LOSS_OF_MODEL_TYPE)}")
    if int(passes) < 1:
        raise ValueError(f"passes must be at least 1, not {passes}")
    if not coordinates:
        raise ValueError("a descent needs at least one coordinate")
    if len(coordinates) > MAX_COORDINATES:
        raise ValueError(f"{len(coordinates)} coordinates: one offset update adds up at most {MAX_COORDINATES}")
    names = [c.name for c in coordinates]
    for nm in names:
        if names.count(nm) > 1:
            raise ValueError(f"two coordinates are named {nm!r}")
    n = train.n
    for which, ds in (("training", train), ("validation", validation)):
        if ds is None:
            continue
        for col in ("uid", "weight", "offset"):
            a = getattr(ds, col)
            if a is not None and np.asarray(a).shape != (ds.n,):
                raise ValueError(f"the {which} data set's {col} has {np.asarray(a).shape} entries, its label {ds.n}")
        if model_type == POISSON_REGRESSION:
            from .batch import check_count_labels
            check_count_labels(ds.label, f"poisson_regression, the {which} labels")
    for c in coordinates:
        if c.entity is not None and np.asarray(c.entity).shape != (n,):
            raise ValueError(f"coordinate {c.name!r}: the entity array has {np.asarray(c.entity).shape} entries, the data set has {n} samples")
        if c.regularize_bias and not c.has_intercept:
            raise ValueError(f"coordinate {c.name!r}: regularize_bias needs an intercept")
        if validation is not None:
            if c.validation_bag is None or (c.random_effect and c.validation_entity is None):
                raise ValueError(f"coordinate {c.name!r}: validation data needs its validation_bag" + (" and validation_entity" if c.random_effect else ""))
            if c.random_effect and np.asarray(c.validation_entity).shape != (validation.n,):
                raise ValueError(f"coordinate {c.name!r}: the validation entity array has {np.asarray(c.validation_entity).shape} entries, "
                                 f"the validation set has {validation.n} samples")


# ---- a coordinate on the device ----------------------------------------------------------------------------------------------------------
class _RandomEffect:
    """Grouped and packed once; its packed batch aliases self.offsets (gdmix_re_packed shares y / offset / weight with the raw batch)."""

    def __init__(self, cd, c, train_dev, validation_dev):
        from .solver import SolverOptions
        s, t = cd.solver, cd.solver.torch
        self.c, self.solver = c, s
        self.opts = SolverOptions(l2=c.l2, regularize_bias=bool(c.regularize_bias) and bool(c.has_intercept), has_intercept=c.has_intercept, m=cd.m,
                                  max_iter=cd.max_iter, ftol=cd.tolerance, threshold=cd.threshold, loss=cd.loss)
        ptr, col, val, dim = _check_bag(c.name, c.bag, train_dev["n"], "the bag")
        self.ids, inv = np.unique(np.asarray(c.entity, np.int64), return_inverse=True)
        up = lambda a: t.from_numpy(np.ascontiguousarray(a)).to(s.device)
        g, self.counts = s.group_rows(up(ptr), up(col), up(val), up(inv.astype(np.int32)), self.ids.size)
        self.row_of, self.n = g["row_of"], train_dev["n"]
        self.offsets = t.zeros(g["N"], dtype=t.float32, device=s.device)
        g["y"] = s.rows_gather(train_dev["y"], self.row_of)
        g["weight"] = None if train_dev["weight"] is None else s.rows_gather(train_dev["weight"], self.row_of)
        g["offset"] = self.offsets
        self.packed = s.pack(g, has_intercept=c.has_intercept)
        self.present = self.ids[g["present"].cpu().numpy()]      # (every training entity owns a row: all of ids, in order)
        self.theta = None
        self.v = None
        if validation_dev is not None:
            vptr, vcol, vval, _ = _check_bag(c.name, tuple(c.validation_bag[:3]) + (dim,), validation_dev["n"], "the validation bag")
            vent = np.asarray(c.validation_entity, np.int64)
            at = np.minimum(np.searchsorted(self.ids, vent), max(self.ids.size - 1, 0))
            vidx = np.where(self.ids[at] == vent, at, -1).astype(np.int32) if self.ids.size else np.full(vent.size, -1, np.int32)
            vg, vcounts = s.group_rows(up(vptr), up(vcol), up(vval), up(vidx), self.ids.size)
            self.v = dict(n=validation_dev["n"], row_of=vg["row_of"], counts=vcounts, packed=None)
            if vg["N"] > 0:
                vg["y"] = s.rows_gather(validation_dev["y"], vg["row_of"])
                vg["weight"] = None
                vg["offset"] = t.zeros(vg["N"], dtype=t.float32, device=s.device)
                vp = s.pack(vg, has_intercept=c.has_intercept)
                # the training batch's entity e sits at row e (present = every id, ascending); an entity the training data lacks never
                # reaches the validation batch: its rows carry -1 and are left out, their contribution stays 0
                coef_pos, has_model = s.join_features(vp, self.packed, vg["present"])
                self.v.update(packed=vp, coef_pos=coef_pos, has_model=has_model)

    def rows(self):
        return self.row_of

    def update(self, warm):
        s = self.solver
        theta0 = self.theta if warm else None
        res = s.solve(self.packed, self.opts, theta0=theta0)
        status = res.status.cpu().numpy()
        if status.size and not ((status >= 0) & (status <= 4)).all():
            bad = int(np.flatnonzero((status < 0) | (status > 4))[0])
            raise RuntimeError(f"coordinate {self.c.name!r}: entity {bad} did not finish (device status {int(status[bad])})")
        self.theta, self.theta_thr = res.theta, res.theta_thr
        info = dict(max_nit=int(res.nit.max()) if status.size else 0, status=status)
        return theta0, info

    def score(self, out):
        """The thresholded model's contribution into `out` [N], sample order -> the accumulated score [N] (every training row is grouped)."""
        s = self.solver
        logit, per = s.score(self.packed, self.theta_thr)
        s.rows_scatter(per, self.row_of, self.n, out=out)
        return s.rows_scatter(logit, self.row_of, self.n)

    def validation_score(self, offsets, out):
        """offsets [Nv]: the other coordinates' accumulated contributions, sample order. The contribution into `out` -> the accumulated
        score; a row of an entity the training data lacks contributes 0 and keeps its offset."""
        s, v = self.solver, self.v
        if v["packed"] is None:
            out.zero_()
            return offsets
        s.rows_gather(offsets, v["row_of"], out=v["packed"].offset())
        logit, per = s.score_models(v["packed"], [self.theta_thr], v["coef_pos"], v["has_model"], per_coord=True)
        s.rows_scatter(per[0], v["row_of"], v["n"], out=out)
        return s.rows_scatter(logit[0], v["row_of"], v["n"], out=offsets, keep_rest=True)

    def model(self):
        h = lambda x: x.cpu().numpy()
        return CoordinateModel(self.c.name, True, self.c.dim, self.c.has_intercept, h(self.theta), h(self.theta_thr), present=self.present,
                               unique_global=h(self.packed.unique_global()).astype(np.int64), coef_ptr=self.packed.coef_ptr_host(),
                               feat_ptr=h(self.packed.ent_feat_ptr()), features=self.c.features)


class _FixedEffect:
    """The shard packed as fixed_effect.shard_as_batch does and its problem created once (gdmix_fe_create); the problem reads the offsets
    through the packed shard's pointer, so an update rewrites them in place and re-arms the problem with gdmix_fe_restart."""

    def __init__(self, cd, c, train, validation):
        from . import fixed_effect as fe
        s = cd.solver
        self.c, self.solver, self.threshold = c, s, cd.threshold
        ptr, col, val, dim = _check_bag(c.name, c.bag, train.n, "the bag")
        if col.size == 0:
            raise ValueError(f"coordinate {c.name!r}: a fixed effect needs at least one non-zero")
        self.opts = fe.fit_options(c.has_intercept, c.l2, c.regularize_bias, cd.model_type, cd.max_iter, cd.m, cd.tolerance)
        self.fit = fe._SteppingFit(s, self.opts, ptr, col, val, np.asarray(train.label, np.float32), dim, None, train.weight, None, None, False, None)
        self.offsets = self.fit.packed.offset()
        self.n = train.n
        self.shard = fe.DeviceShard(s, ptr, col, val, None, dim)
        self.vshard = None
        if validation is not None:
            vptr, vcol, vval, _ = _check_bag(c.name, tuple(c.validation_bag[:3]) + (dim,), validation.n, "the validation bag")
            self.vshard = fe.DeviceShard(s, vptr, vcol, vval, None, dim)
        self.theta = None

    def rows(self):
        return None

    def update(self, warm):
        t = self.solver.torch
        theta0 = self.theta if warm else None
        self.fit.prob.restart(self.opts, theta0)      # (cold: by the restart's contract the bits of a problem just created)
        theta, info = self.fit.run()
        if not 0 <= int(info["status"]) <= 4:
            raise RuntimeError(f"coordinate {self.c.name!r}: the fixed-effect solve did not finish (device status {int(info['status'])})")
        thr = np.where(np.abs(theta) <= self.threshold, 0.0, theta)
        self.theta = t.from_numpy(theta).to(self.solver.device)
        self.theta_thr = t.from_numpy(thr).to(self.solver.device)
        return theta0, dict(max_nit=int(info["nit"]), status=np.array([info["status"]], np.int32))

    def _score(self, shard, offsets, out):
        from .fixed_effect import device_score_shard
        _, per = device_score_shard(self.solver, shard, self.theta_thr, self.c.has_intercept)
        out.copy_(per)
        return self.solver.offsets_combine(shard.n, offsets, [out])      # float32(per-coordinate score + offset), as the stage's score file

    def score(self, out):
        return self._score(self.shard, self.offsets[:self.n], out)

    def validation_score(self, offsets, out):
        return self._score(self.vshard, offsets, out)

    def model(self):
        h = lambda x: x.cpu().numpy()
        return CoordinateModel(self.c.name, False, self.c.dim, self.c.has_intercept, h(self.theta), h(self.theta_thr), features=self.c.features)

    def close(self):
        self.fit.prob.close()


class CoordinateDescent:
    """fit(): the descent described in the module's docstring, on one MI355X. There is no CPU path: without a device, or without the
    library, construction raises."""

    def __init__(self, device=0, model_type=LOGISTIC_REGRESSION, m=10, max_iter=100, tolerance=1e-12, threshold=1e-4, solver=None):
        if model_type not in LOSS_OF_MODEL_TYPE:
            raise ValueError(f"model type {model_type!r}: one of {', '.join(LOSS_OF_MODEL_TYPE)}")
        self.device, self.model_type, self.loss = device, model_type, LOSS_OF_MODEL_TYPE[model_type]
        self.m, self.max_iter, self.tolerance, self.threshold = int(m), int(max_iter), float(tolerance), float(threshold)
        self._solver = solver

    @property
    def solver(self):
        if self._solver is None:
            from .solver import REDeviceSolver
            self._solver = REDeviceSolver(self.device)
        return self._solver

    def _evaluate(self, score, label):
        from . import metrics
        ev = metrics.PoissonEvaluator(self.solver) if self.metric == metrics.POISSON_LOSS else metrics.DeviceEvaluator(self.solver)
        ev.add(score, label)
        return ev.finish()[self.metric]

    def fit(self, train, coordinates, passes=1, validation=None, record=False):
        """train / validation: DataSet; coordinates: Coordinate objects, updated in this order in every pass -> DescentResult."""
        import time
        from . import metrics
        check_request(train, coordinates, passes, self.model_type, validation)
        s = self.solver
        t = s.torch
        self.metric = metrics.metric_of_loss(self.loss)
        sync = lambda: t.cuda.current_stream(s.device).synchronize()
        up = lambda a: None if a is None else t.from_numpy(np.ascontiguousarray(a, np.float32)).to(s.device)
        dev = lambda ds: None if ds is None else dict(n=ds.n, y=up(ds.label), weight=up(ds.weight), base=up(ds.offset))
        td, vd = dev(train), dev(validation)
        N = train.n
        setup_s, blocks = {}, []
        try:
            for c in coordinates:
                t0 = time.perf_counter()
                blocks.append(_RandomEffect(self, c, td, vd) if c.random_effect else _FixedEffect(self, c, train, validation))
                sync()
                setup_s[c.name] = time.perf_counter() - t0
            zeros = lambda n: t.zeros(n, dtype=t.float32, device=s.device)
            parts = [zeros(N) for _ in coordinates]
            vparts = [zeros(validation.n) for _ in coordinates] if validation is not None else None
            h = lambda x: None if x is None else x.cpu().numpy()
            history, pass_s, update_s = [], [], []
            for p in range(int(passes)):
                tp = time.perf_counter()
                for k, (c, b) in enumerate(zip(coordinates, blocks)):
                    tu = time.perf_counter()
                    s.offsets_combine(N, td["base"], parts, skip=k, row_of=b.rows(), out=b.offsets)
                    offsets = h(b.offsets) if record else None
                    theta0, info = b.update(warm=p > 0)
                    score = b.score(parts[k])
                    entry = {"pass": p, "coordinate": c.name, "max_nit": info["max_nit"], "status": info["status"]}
                    entry[f"train_{self.metric}"] = self._evaluate(score, td["y"])
                    vscore = voffsets = None
                    if validation is not None:
                        voff = s.offsets_combine(validation.n, vd["base"], vparts, skip=k)
                        voffsets = h(voff) if record else None
                        vscore = b.validation_score(voff, vparts[k])
                        entry[f"validation_{self.metric}"] = self._evaluate(vscore, vd["y"])
                    sync()
                    update_s.append(time.perf_counter() - tu)
                    if record:
                        entry.update(offsets=offsets, theta0=h(theta0), theta=h(b.theta), theta_thr=h(b.theta_thr), score=h(score), validation_score=h(vscore),
                                     contribution=h(parts[k]), validation_offsets=voffsets)
                    history.append(entry)
                pass_s.append(time.perf_counter() - tp)
            return DescentResult(self.model_type, self.metric, history, {c.name: b.model() for c, b in zip(coordinates, blocks)},
                                 {c.name: h(x) for c, x in zip(coordinates, parts)},
                                 {c.name: h(x) for c, x in zip(coordinates, vparts)} if vparts is not None else {},
                                 {c.name: h(b.rows()) for c, b in zip(coordinates, blocks) if b.rows() is not None}, setup_s, pass_s, update_s)
        finally:
            for b in blocks:
                if hasattr(b, "close"):
                    b.close()


# ---- the models as a stage writes them -------------------------------------------------------------------------------------------------------
def write_models(result, root):
    """<root>/<name>/models/part-00000.avro for every coordinate, through the writers the stages use (model._export_models_to_avro: the
    intercept always, a feature when |value| > 1e-4): what --action=inference of the stage loads. -> {name: path}."""
    from . import constants
    from .fe_model import GLOBAL_MODEL_ID, MODEL_CLASS
    from .model import ModelTable, _export_models_to_avro
    out = {}
    for name, m in result.models.items():
        d = os.path.join(root, name, "models")
        os.makedirs(d, exist_ok=True)
        path = os.path.join(d, "part-00000.avro")
        features = m.features if m.features is not None else [(f"{name}_{j}", "") for j in range(m.dim)]
        if len(features) != m.dim:
            raise ValueError(f"coordinate {name!r}: {len(features)} feature names for {m.dim} columns")
        ic = 1 if m.has_intercept else 0
        table = ModelTable()
        if m.random_effect:
            table.add_chunk([str(e) for e in m.present.tolist()], m.theta_thr, m.coef_ptr, m.unique_global, m.feat_ptr)
            model_class = constants.PHOTON_POISSON_MODEL_CLASS if result.model_type == POISSON_REGRESSION else None
        else:
            local = np.concatenate([m.theta_thr[m.dim:m.dim + ic], m.theta_thr[:m.dim]])      # intercept first, as the export helper expects
            table.add_chunk([GLOBAL_MODEL_ID], local, [0, local.size], np.arange(m.dim, dtype=np.int64), [0, m.dim])
            model_class = MODEL_CLASS[result.model_type]
        _export_models_to_avro(path, table, [tuple(f) for f in features], m.has_intercept, False, sparsity_threshold=1.0e-4, model_class=model_class)
        out[name] = path
    return out
