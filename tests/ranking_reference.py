"""The tests' own statement of the ranking evaluation (include/gdmix_re.h, "ranking evaluation"): the four integers of precision@k per
entity, precision@k and the aggregates as exact rationals (Python ints and Fraction), and the same expectation by exhaustive enumeration
of tie orders. Plain Python over numpy arrays, written from the definitions — nothing here shares code with gdmix_amd/metrics.py.

There is no counterpart in the reference project: its Evaluator reports a global AUC or MSE and nothing per entity. The definition is
Photon-ML's PrecisionAtK multi-evaluator with ties resolved in expectation, as the header states it on its own authority.
"""
import itertools
import math
from fractions import Fraction

import numpy as np


def _valid(score, label):
    """-> [(score as a Python float, positive?)] of the samples whose score is not NaN. Python floats compare as the header says scores do:
    -0.0 == 0.0, infinities order as usual."""
    return [(float(s), bool(y > 0.5)) for s, y in zip(np.asarray(score, np.float32).tolist(), np.asarray(label, np.float32).tolist()) if not math.isnan(s)]


def topk_counts(score, label, k):
    """One entity -> (hits_sure, slots, tie_pos, tie_size), Python ints."""
    k = int(k)
    assert k >= 1
    v = _valid(score, label)
    n = len(v)
    if n <= k:
        return sum(p for _, p in v), 0, 0, 0
    c = sorted((s for s, _ in v), reverse=True)[k - 1]      # the k-th largest score
    above = [p for s, p in v if s > c]
    tie = [p for s, p in v if s == c]
    assert len(above) < k <= len(above) + len(tie)
    return sum(above), k - len(above), sum(tie), len(tie)


def expected_hits(counts) -> Fraction:
    hits_sure, slots, tie_pos, tie_size = counts
    return Fraction(hits_sure) + (Fraction(slots * tie_pos, tie_size) if tie_size else 0)


def precision(score, label, k) -> Fraction:
    """precision@k of one entity, exact. The denominator is k whatever the entity's size."""
    return expected_hits(topk_counts(score, label, k)) / int(k)


def precision_by_enumeration(score, label, k) -> Fraction:
    """The same number the long way: every order of the valid samples that is sorted by descending score (that is every order inside the tie
    groups, each as likely as another), the positives among its first k, averaged; over k."""
    v = _valid(score, label)
    hits, orders = 0, 0
    for perm in itertools.permutations(range(len(v))):
        if all(v[perm[i]][0] >= v[perm[i + 1]][0] for i in range(len(perm) - 1)):
            orders += 1
            hits += sum(v[i][1] for i in perm[:k])
    return Fraction(hits, orders) / int(k)


def per_entity_counts(ent_row_ptr, score, label, ks) -> dict:
    """A batch -> {"hits_sure", "slots", "tie_pos", "tie_size": int64 [len(ks), E], "n": valid samples [E]}."""
    rp = np.asarray(ent_row_ptr, np.int64)
    E = rp.size - 1
    out = {name: np.zeros((len(ks), E), np.int64) for name in ("hits_sure", "slots", "tie_pos", "tie_size")}
    n = np.zeros(E, np.int64)
    for e in range(E):
        s, y = score[rp[e]:rp[e + 1]], label[rp[e]:rp[e + 1]]
        n[e] = len(_valid(s, y))
        for j, k in enumerate(ks):
            for name, v in zip(("hits_sure", "slots", "tie_pos", "tie_size"), topk_counts(s, y, k)):
                out[name][j, e] = v
    out["n"] = n
    return out


def auc_exact(score, label):
    """One entity -> its AUC as a Fraction (ties at half weight), or None when a class is missing."""
    v = _valid(score, label)
    pos, neg = [s for s, p in v if p], [s for s, p in v if not p]
    if not pos or not neg:
        return None
    neg.sort()
    two_u = 0
    import bisect
    for s in pos:
        lo, hi = bisect.bisect_left(neg, s), bisect.bisect_right(neg, s)
        two_u += 2 * lo + (hi - lo)
    return Fraction(two_u, 2 * len(pos) * len(neg))


def mean_of_records(values):
    """An aggregate as the stage writes it: the correctly rounded sum of the records' doubles over their number; None without a record."""
    values = list(values)
    return math.fsum(values) / len(values) if values else None


def log_loss_reference(score, label):
    """(math.fsum of log(1 + exp(s)) - [y > 0.5] s over the samples whose score is not NaN, the sum of the terms' magnitudes — the terms are
    non-negative, so the same number —, how many such samples). np.logaddexp(0, s) - y s is evaluated in numpy's long double and each term
    rounded to a double once: in fp64 the subtraction of s from logaddexp(0, s) alone would cost an ulp of s, more than the bound allows a
    single-sample entity with a confident score."""
    s = np.asarray(score, np.float32).astype(np.longdouble)
    ok = ~np.isnan(s)
    t = (np.logaddexp(np.longdouble(0.0), s[ok]) - (np.asarray(label, np.float32)[ok] > 0.5) * s[ok]).astype(np.float64)
    return math.fsum(t.tolist()), math.fsum(np.abs(t).tolist()), int(ok.sum())
