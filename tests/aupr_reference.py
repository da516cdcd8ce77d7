"""AUPR as include/gdmix_re.h defines it ("AUPR"), in exact rationals on the host statement of the key (metrics.sortable_key)."""
from fractions import Fraction

import numpy as np

from gdmix_amd import metrics


def pr_sum_exact(score, label):
    """-> (pr_sum as a Fraction, n_pos, n_neg, n_nan) of one scored set. AUPR = pr_sum / n_pos."""
    s = np.asarray(score, np.float32)
    valid = ~np.isnan(s)
    key = metrics.sortable_key(s[valid]).astype(np.int64)
    pos = np.asarray(label, np.float32)[valid] > 0.5
    groups, of = np.unique(key, return_inverse=True)      # one threshold per tie group
    t_of, f_of = np.bincount(of, pos, groups.size).astype(np.int64), np.bincount(of, ~pos, groups.size).astype(np.int64)
    total, T, F, P_prev = Fraction(0), 0, 0, None
    for j in range(groups.size - 1, -1, -1):               # c_1 > c_2 > ...
        t = int(t_of[j])
        T, F = T + t, F + int(f_of[j])
        P = Fraction(T, T + F)
        total += t * (P + (P if P_prev is None else P_prev)) / 2      # P_0 := P_1
        P_prev = P
    return total, int(pos.sum()), int((~pos).sum()), int((~valid).sum())
