"""Shared by tests/test_feature_stats_host.py (CPU) and tests/test_gpu_feature_stats.py (GPU): the cases of the column-statistics
kernels and their reference in Python integers (include/gdmix_re.h, "feature normalisation"). Test infrastructure.

The reference: count and max |x| per feature by a sort; L, shift1, shift2 from Python's int.bit_length and math.frexp; every term
rint(x 2^shift) as an int64 through the IEEE operations (a sample of the terms is checked against Fractions by the CPU test), the sums
of the high limbs, of the low limbs and of the whole terms as Python integers (object arrays)."""
import math
from fractions import Fraction

import numpy as np


def reference(col, val, D):
    """-> dict(count [D] int64, bits [D] uint32, L / s1 / s2 [D] int32, limbs [D, 4] int64, I1 / I2: lists of Python ints). Every entry
    must be good (finite, column in range)."""
    col = np.asarray(col).astype(np.int64)
    val = np.asarray(val, np.float32)
    order = np.argsort(col, kind="stable")
    c, v = col[order], val[order]
    feats, starts, counts = np.unique(c, return_index=True, return_counts=True)
    count = np.zeros(D, np.int64)
    count[feats] = counts
    bits = np.zeros(D, np.uint32)
    if c.size:
        bits[feats] = np.maximum.reduceat(np.abs(v).view(np.uint32), starts)
    L, s1, s2 = np.zeros(D, np.int32), np.zeros(D, np.int32), np.zeros(D, np.int32)
    for j in feats.tolist():
        a = float(bits[j:j + 1].view(np.float32)[0])
        if a == 0.0:
            continue
        e = math.frexp(a)[1]                        # a = m 2^e, m in [0.5, 1): e = floor(log2 a) + 1
        L[j] = min(31, 62 - int(count[j]).bit_length())
        s1[j], s2[j] = 2 * L[j] - e, 2 * L[j] - 2 * e
    limbs = np.zeros((D, 4), np.int64)
    I1, I2 = [0] * D, [0] * D
    if c.size:
        x = v.astype(np.float64)
        Lc = L[c].astype(np.int64)
        t1 = np.where(Lc > 0, np.rint(np.ldexp(x, s1[c])), 0.0).astype(np.int64)
        t2 = np.where(Lc > 0, np.rint(np.ldexp(x * x, s2[c])), 0.0).astype(np.int64)
        m = (np.int64(1) << Lc) - 1
        for k, t in ((0, t1 >> Lc), (1, t1 & m), (2, t2 >> Lc), (3, t2 & m)):
            sums = np.add.reduceat(t.astype(object), starts)           # Python integers: no width to overflow
            assert all(-2 ** 63 <= int(s) < 2 ** 63 for s in sums)
            limbs[feats, k] = np.array([int(s) for s in sums], np.int64)
        for j, a, b in zip(feats.tolist(), np.add.reduceat(t1.astype(object), starts), np.add.reduceat(t2.astype(object), starts)):
            I1[j], I2[j] = int(a), int(b)
            assert int(limbs[j, 0]) * 2 ** int(L[j]) + int(limbs[j, 1]) == I1[j] and int(limbs[j, 2]) * 2 ** int(L[j]) + int(limbs[j, 3]) == I2[j]
    return dict(count=count, bits=bits, L=L, s1=s1, s2=s2, limbs=limbs, I1=I1, I2=I2, terms=(c, v, t1, t2) if c.size else None)


def rint_fraction(q):
    f = q.numerator // q.denominator
    r = q - f
    if r > Fraction(1, 2) or (r == Fraction(1, 2) and f % 2 == 1):
        f += 1
    return f


def check_terms_against_fractions(ref, how_many=2000, seed=0):
    """A sample of the reference's terms against exact rational arithmetic."""
    c, v, t1, t2 = ref["terms"]
    rng = np.random.default_rng(seed)
    for i in rng.choice(c.size, min(how_many, c.size), replace=False).tolist():
        j = int(c[i])
        if ref["L"][j] == 0:
            continue
        q = Fraction(float(v[i]))
        assert int(t1[i]) == rint_fraction(q * Fraction(2) ** int(ref["s1"][j]))
        assert int(t2[i]) == rint_fraction(q * q * Fraction(2) ** int(ref["s2"][j]))
        assert abs(int(t1[i])) < 2 ** (2 * int(ref["L"][j])) and int(t2[i]) < 2 ** (2 * int(ref["L"][j]))


# ---- the cases ------------------------------------------------------------------------------------------------------------------------------
def case_one_address():
    """D = 1, Z = 100 003: every add on one address, with an odd tail."""
    rng = np.random.default_rng(1)
    Z = 100003
    return np.zeros(Z, np.int64), (rng.standard_normal(Z) * 3).astype(np.float32), 1


def case_lds():
    """D = 24, Z = 300 000: the LDS path; MovieLens-like columns (0/1 flags next to release_date / 2000 and age / 100)."""
    rng = np.random.default_rng(2)
    Z, D = 300000, 24
    col = rng.integers(0, D, Z)
    val = np.ones(Z, np.float32)
    val[col == 0] = (0.97 + rng.integers(0, 30, Z)[col == 0] / 2000.0).astype(np.float32)
    val[col == 1] = (rng.integers(1, 80, Z)[col == 1] / 100.0).astype(np.float32)
    val[col == 2] = (rng.standard_normal(Z)[col == 2] * 1000).astype(np.float32)
    return col.astype(np.int64), val, D


def case_zipf(D=70001, Z=500000, seed=3):
    """Past uint16, past LDS: Zipf columns (a hot head, a large share of the features dead), per-column scales exp(U(-30, 30)), one nearly
    constant column, values 1e-20 times the rest inside a large column."""
    rng = np.random.default_rng(seed)
    col = np.minimum((D * rng.random(Z) ** 20).astype(np.int64), D - 1)
    scale = np.exp(rng.uniform(-30, 30, D))
    val = (rng.standard_normal(Z) * scale[col]).astype(np.float32)
    one = col == 1
    val[one] = (np.float32(0.97) + rng.integers(0, 3, Z)[one].astype(np.float32) * np.float32(2.0 ** -20)).astype(np.float32)
    tiny = (col == 0) & (rng.random(Z) < 0.3)
    val[tiny] *= np.float32(1e-20)
    return col, val, D


def case_4000():
    """4 000 features: above the 64 KiB of LDS a workgroup has without asking for more, below the CU's 160 KiB."""
    rng = np.random.default_rng(4)
    Z, D = 200000, 4000
    col = np.minimum((D * rng.random(Z) ** 3).astype(np.int64), D - 1)
    return col, (rng.standard_normal(Z) * np.exp(rng.uniform(-5, 5, D))[col]).astype(np.float32), D


def seven_chunks(Z, seed=5):
    """A permutation of the entries and the bounds of seven uneven chunks of it, one of them empty."""
    rng = np.random.default_rng(seed)
    cuts = np.sort(rng.integers(1, Z, 6))
    cuts[3] = cuts[2]
    return rng.permutation(Z), [0] + cuts.tolist() + [Z]
