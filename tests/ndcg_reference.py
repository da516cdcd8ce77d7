"""NDCG@K of one entity as include/gdmix_re.h, "NDCG", defines it, in mpmath at 50 digits: the reference of tests/test_gpu_ndcg.py."""
import math

import mpmath
import numpy as np

mpmath.mp.dps = 50


def _key(s):
    """fp32 scores compare as floats with -0 equal to +0."""
    return 0.0 if s == 0.0 else float(s)


def dcg_idcg(scores, labels, k):
    """-> (dcg, idcg, n, n_nan, n_bad_label): mpf sums and integer counts over the valid samples (score not NaN). A label outside [0, 64]
    (NaN, infinite, negative, above 64) is counted and gains 0. A tie group of the ranks [a, b) adds its mean gain times the discounts of
    the ranks a .. min(b, k) - 1."""
    s, y = np.asarray(scores, np.float32), np.asarray(labels, np.float32)
    valid = ~np.isnan(s)
    n, n_nan = int(valid.sum()), int((~valid).sum())
    s, y = s[valid], y[valid].astype(np.float64)
    bad = ~((y >= 0.0) & (y <= 64.0))
    gain = [mpmath.mpf(0) if b else mpmath.power(2, mpmath.mpf(float(v))) - 1 for v, b in zip(y, bad)]
    disc = lambda r: 1 / mpmath.log(r + 2, 2)
    top = min(int(k), n)
    idcg = mpmath.fsum(g * disc(r) for r, g in enumerate(sorted(gain, reverse=True)[:top]))
    groups = {}
    for sc, g in zip(s, gain):
        groups.setdefault(_key(sc), []).append(g)
    dcg, a = mpmath.mpf(0), 0
    for sc in sorted(groups, reverse=True):
        b = a + len(groups[sc])
        if a < top:
            dcg += mpmath.fsum(groups[sc]) / (b - a) * mpmath.fsum(disc(r) for r in range(a, min(b, top)))
        a = b
    return dcg, idcg, n, n_nan, int(bad.sum())


def ndcg(scores, labels, k):
    """-> NDCG@k as a float, or None where it is null: no gain, a bad label, a NaN score."""
    dcg, idcg, _, n_nan, n_bad = dcg_idcg(scores, labels, k)
    return None if idcg == 0 or n_nan or n_bad else float(dcg / idcg)


def mean_of_records(values):
    return math.fsum(values) / len(values) if values else None
