"""CPU restatement of the resident coordinate descent (gdmix_amd/descent.py) — test infrastructure, never imported by the product.
Every solve is the fp64 oracle's (oracle/re_oracle.c), every contribution is the per-coordinate score of the THRESHOLDED model
truncated to float32, every offset is descent.offsets_combine_host of the other coordinates' contributions, the rows of a random effect
are grouped by descent.group_rows_host. Logistic loss only (the oracle has no Poisson loss)."""
import numpy as np

from gdmix_amd import chain, descent
from gdmix_amd import fixed_effect as fe
from oracle import oracle

THRESHOLD = 1e-4


def _threshold(theta):
    return np.where(np.abs(theta) <= THRESHOLD, 0.0, theta)


def movielens_coordinates(data, re_regularize_bias, rows=None, vrows=None):
    """The three coordinates of chain.make_dataset's dict over `rows` (default: the training rows), with the validation rows' bags:
    descent.Coordinate objects, as chain.run_resident builds them."""
    return chain.resident_coordinates(data, re_regularize_bias=re_regularize_bias, rows=rows, vrows=vrows)


class Block:
    """One coordinate on the CPU: packed once (a random effect grouped first), solved from given offsets and a given start point."""

    def __init__(self, c, label, weight=None, m=10, max_iter=100, tolerance=1e-12):
        self.c = c
        ptr, col, val, dim = c.bag
        self.dim, self.n = int(dim), int(np.asarray(label).size)
        y = np.asarray(label, np.float32)
        if c.random_effect:
            self.ids, inv = np.unique(np.asarray(c.entity, np.int64), return_inverse=True)
            g = descent.group_rows_host(ptr, col, val, inv, self.ids.size)
            self.row_of = g["row_of"].astype(np.int64)
            self.pk = oracle.pack(g["ent_row_ptr"], g["row_nnz_ptr"], g["col_global"])
            self.val, self.y = g["val"], y[self.row_of]
            self.weight = None if weight is None else np.asarray(weight, np.float32)[self.row_of]
            self.opts = oracle.make_opts(l2=c.l2, regularize_bias=c.regularize_bias, has_intercept=True, m=m, max_iter=max_iter, ftol=tolerance,
                                         threshold=THRESHOLD)
        else:
            self.row_of = None
            batch, _ = fe.shard_as_batch(ptr, col, val, y, None, weight, True, dummy=False)
            self.pk = oracle.pack(batch.ent_row_ptr, batch.row_nnz_ptr, batch.col_global)
            self.val, self.y, self.weight = batch.val, batch.y, batch.weight
            self.opts = oracle.make_opts(l2=c.l2, regularize_bias=c.regularize_bias, has_intercept=True, m=m, max_iter=max_iter, ftol=tolerance,
                                         threshold=0.0, sum_loss=True)
        self.theta = None

    # the device's layout of a fixed effect is [w (dim), b]; the oracle's is the packed one, [b, w of the features present]
    def to_device_layout(self, theta):
        return theta if self.c.random_effect else fe.to_global(theta, self.pk["unique_global"], self.dim, True, False)

    def from_device_layout(self, theta):
        if theta is None:
            return None
        return theta if self.c.random_effect else fe.to_local(theta, self.pk["unique_global"], self.dim, True, False)

    def solve(self, offsets, theta0=None):
        """offsets in the block's row order (grouped for a random effect), theta0 in the oracle's layout -> (theta, theta_thr, result)."""
        res = oracle.solve(self.pk, self.val, self.y, np.asarray(offsets, np.float32), self.weight, self.opts, theta0=theta0)
        return res["theta"], _threshold(res["theta"]), res

    def contribution(self, theta_thr):
        """The per-coordinate score of every training sample under theta_thr, float32, sample order."""
        _, per = oracle.score(self.pk, self.val, np.zeros(self.pk["N"], np.float32), theta_thr, True)
        return per if self.row_of is None else descent.rows_scatter_host(per, self.row_of, self.n)

    def regularised(self):
        """The mask of the regularised entries of theta (the oracle's layout)."""
        mask = np.ones(self.pk["D"] + self.pk["E"], bool)
        if not self.c.regularize_bias:
            fp = self.pk["ent_feat_ptr"]
            mask[fp[:-1] + np.arange(self.pk["E"])] = False
        return mask

    def validation_contribution(self, theta_thr):
        """The thresholded model applied to the validation bag; an entity the training data lacks contributes 0."""
        ptr, col, val, _ = self.c.validation_bag
        ptr, col = np.asarray(ptr, np.int64), np.asarray(col, np.int64)
        n = ptr.size - 1
        rows = np.repeat(np.arange(n), np.diff(ptr))
        fp, uq = self.pk["ent_feat_ptr"], self.pk["unique_global"]
        E = self.pk["E"]
        coef = np.zeros((E, self.dim))
        ent = np.repeat(np.arange(E), np.diff(fp))
        coef[ent, uq] = np.delete(theta_thr, fp[:-1] + np.arange(E))
        icpt = theta_thr[fp[:-1] + np.arange(E)]
        if self.c.random_effect:
            vent = np.asarray(self.c.validation_entity, np.int64)
            at = np.minimum(np.searchsorted(self.ids, vent), E - 1)
            has = self.ids[at] == vent
        else:
            at, has = np.zeros(n, np.int64), np.ones(n, bool)
        z = np.where(has, icpt[at], 0.0) + np.bincount(rows, np.asarray(val, np.float64) * np.where(has[rows], coef[at[rows], col], 0.0), n)
        return z.astype(np.float32)


def objective(blocks, thetas_thr, label, weight, parts):
    """The joint objective in fp64 from the contributions and the thresholded models (descent.joint_objective)."""
    score = np.sum([p.astype(np.float64) for p in parts], axis=0)
    return descent.joint_objective("logistic", label, weight, score, [(th, b.regularised(), b.c.l2) for b, th in zip(blocks, thetas_thr) if th is not None])


def run(coordinates, label, passes, validation_label=None):
    """-> dict(F: [passes x C] the joint objective after every update, validation_auc: the same shape (with validation data), parts,
    thetas): the descent free-running on the CPU."""
    blocks = [Block(c, label) for c in coordinates]
    n = int(np.asarray(label).size)
    parts = [np.zeros(n, np.float32) for _ in blocks]
    vparts = None if validation_label is None else [np.zeros(int(np.asarray(validation_label).size), np.float32) for _ in blocks]
    thetas = [None] * len(blocks)
    thetas_thr = [None] * len(blocks)
    F, vauc, moved = [], [], []
    for p in range(passes):
        F.append([])
        vauc.append([])
        moved.append(0.0)
        for k, b in enumerate(blocks):
            off = descent.offsets_combine_host(n, None, parts, skip=k, row_of=b.row_of)
            theta, thr, _ = b.solve(off, thetas[k])
            if thetas[k] is not None:
                moved[-1] = max(moved[-1], float(np.abs(theta - thetas[k]).max()))
            thetas[k], thetas_thr[k] = theta, thr
            parts[k] = b.contribution(thr)
            F[-1].append(objective(blocks, thetas_thr, label, None, parts))
            if vparts is not None:
                vparts[k] = b.validation_contribution(thr)
                vauc[-1].append(chain.auc(validation_label, descent.offsets_combine_host(vparts[0].size, None, vparts)))
    return dict(F=np.array(F), validation_auc=np.array(vauc), parts=parts, thetas=thetas, thetas_thr=thetas_thr, blocks=blocks, moved=moved)
