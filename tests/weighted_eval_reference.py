"""The weighted evaluation as include/gdmix_re.h defines it ("weighted evaluation"), in exact rationals from the fp32 inputs, on the host
statement of the key (metrics.sortable_key). The log-loss term itself is libm's in fp64 (its error is far below the sums' bound); the
products and sums are exact."""
import math
from fractions import Fraction

import numpy as np

from gdmix_amd import metrics


def _kept(score, label, weight):
    """-> (scores, positive?, weights as Fractions) of the valid samples, n_nan, n_bad_weight. A bad weight is counted first."""
    s, y = np.asarray(score, np.float32), np.asarray(label, np.float32)
    w = np.ones(s.size, np.float32) if weight is None else np.asarray(weight, np.float32)
    bad = ~(w >= 0) | np.isinf(w)
    nan = ~bad & np.isnan(s)
    keep = ~bad & ~nan
    return s[keep], y[keep] > 0.5, [Fraction(float(x)) for x in w[keep]], int(nan.sum()), int(bad.sum())


def rank_sums_exact(score, label, weight=None):
    """-> (twoU_w, W_pos, W_neg as Fractions, n_nan, n_bad_weight): per tie group P_g (2 Nbefore_g + N_g)."""
    s, pos, w, n_nan, n_bad = _kept(score, label, weight)
    groups, of = np.unique(metrics.sortable_key(s).astype(np.int64), return_inverse=True)
    P, N = [Fraction(0)] * groups.size, [Fraction(0)] * groups.size
    for g, p, x in zip(of.tolist(), pos.tolist(), w):
        if p:
            P[g] += x
        else:
            N[g] += x
    two_u, before = Fraction(0), Fraction(0)
    for g in range(groups.size):      # ascending scores
        two_u += P[g] * (2 * before + N[g])
        before += N[g]
    return two_u, sum(P, Fraction(0)), before, n_nan, n_bad


def logloss_sums_exact(score, label, weight=None):
    """-> (LL_w, W as Fractions, n_nan, n_bad_weight); LL_w is math.inf with an infinite score on the wrong side of its label. Every term
    is >= 0, so LL_w is also the sum of magnitudes the header's bound is relative to."""
    s, pos, w, n_nan, n_bad = _kept(score, label, weight)
    ll = Fraction(0)
    for z, p, x in zip(s.astype(np.float64).tolist(), pos.tolist(), w):
        if x > 0:      # (a weight of 0 adds 0 whatever the score)
            ce = max(-z if p else z, 0.0) + math.log1p(math.exp(-abs(z)))
            if math.isinf(ce):      # an infinite score on the wrong side of its label: LL_w is +inf
                return math.inf, sum(w, Fraction(0)), n_nan, n_bad
            ll += x * Fraction(ce)
    return ll, sum(w, Fraction(0)), n_nan, n_bad
