"""The numpy statement of the evaluation contract (include/gdmix_re.h, "evaluation") that the metric tests lean on. Test
infrastructure: exact Python integers, no device. tests/test_metrics_host.py pins it against chain.auc and the O(n^2) definition."""
import math

import numpy as np


def two_u_reference(score, label):
    """-> (twoU, n_pos, n_neg, n_nan) as Python ints: twoU = sum over positives of 2 #{negatives below} + #{negatives equal}; a NaN
    score is counted and left out; -0 equals +0 (np.unique compares values)."""
    score = np.asarray(score, np.float32)
    pos_all = np.asarray(label, np.float32) > 0.5
    ok = ~np.isnan(score)
    n_nan = int((~ok).sum())
    s, pos = score[ok], pos_all[ok]
    n_pos, n_neg = int(pos.sum()), int((~pos).sum())
    if s.size == 0:
        return 0, 0, 0, n_nan
    _, inv = np.unique(s, return_inverse=True)
    groups = int(inv.max()) + 1
    negs = np.bincount(inv[~pos], minlength=groups).astype(np.int64)
    poss = np.bincount(inv[pos], minlength=groups).astype(np.int64)
    below = np.cumsum(negs) - negs          # negatives strictly below each distinct score
    assert s.size < (1 << 31)      # every product and the sum (at most n^2 / 2) fit an int64
    two_u = int(np.sum(poss * (2 * below + negs), dtype=np.int64))
    return two_u, n_pos, n_neg, n_nan


def auc_reference(score, label):
    from fractions import Fraction
    two_u, n_pos, n_neg, _ = two_u_reference(score, label)
    return float(Fraction(two_u, 2 * n_pos * n_neg)) if n_pos and n_neg else float("nan")


def sse_reference(score, label):
    """math.fsum of the fp64 terms (label - score)^2, NaN scores left out."""
    s = np.asarray(score, np.float32).astype(np.float64)
    y = np.asarray(label, np.float32).astype(np.float64)
    ok = ~np.isnan(s)
    d = y[ok] - s[ok]
    return math.fsum((d * d).tolist())


def per_entity_reference(ent_row_ptr, score, label):
    """-> dict of per-entity lists / arrays: two_u (object array of Python ints), n_pos, n_neg, n_nan (int64), auc (the same fp64
    division the device does, NaN for a single-class entity), sse (fsum)."""
    E = len(ent_row_ptr) - 1
    two_u = np.zeros(E, object)
    n_pos, n_neg, n_nan = np.zeros(E, np.int64), np.zeros(E, np.int64), np.zeros(E, np.int64)
    sse = np.zeros(E)
    for e in range(E):
        a, b = int(ent_row_ptr[e]), int(ent_row_ptr[e + 1])
        two_u[e], n_pos[e], n_neg[e], n_nan[e] = two_u_reference(score[a:b], label[a:b])
        sse[e] = sse_reference(score[a:b], label[a:b])
    with np.errstate(divide="ignore", invalid="ignore"):
        auc = two_u.astype(np.float64) / (2.0 * n_pos * n_neg)
    auc[(n_pos == 0) | (n_neg == 0)] = np.nan
    return dict(two_u=two_u, n_pos=n_pos, n_neg=n_neg, n_nan=n_nan, auc=auc, sse=sse)
