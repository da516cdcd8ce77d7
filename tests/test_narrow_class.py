"""CPU checks of what tests/test_gpu_narrow_class.py stands on: the shaped generator gives entities of exactly the stated (p, n, nnz), and
the oracle's own runs of the history cases meet the conditions the GPU test needs (fits past ten pairs, memory wraps, a wavefront whose
entities finish iterations apart)."""
import numpy as np
import pytest

import narrow_helpers as nh
from oracle import oracle


def test_shaped_batch_has_the_stated_shapes():
    shapes = [(p - 1, n, z) for p in (64, 65, 80, 81) for n in (1, 17, 24, 25) for z in (96, 97)]
    b = nh.make_shaped_batch(shapes, seed=11)
    b.validate()
    pk = oracle.pack(b.ent_row_ptr, b.row_nnz_ptr, b.col_global)
    assert np.array_equal(np.diff(pk["ent_feat_ptr"]), [s[0] for s in shapes])
    assert np.array_equal(b.ent_n(), [s[1] for s in shapes]) and np.array_equal(b.ent_nnz(), [s[2] for s in shapes])
    assert int(nh.is_narrow(np.diff(pk["ent_feat_ptr"]) + 1, b.ent_n(), b.ent_nnz()).sum()) == 6
    for seed in (1, 2):
        for d, n, z in nh.narrow_shapes(np.random.default_rng(seed), 50):
            assert nh.is_narrow(d + 1, n, z)


@pytest.mark.parametrize("m,l2", sorted(nh.HISTORY_CASES))
def test_history_cases_meet_their_conditions_on_the_oracle(m, l2):
    kw = dict(l2=l2, regularize_bias=True, has_intercept=True, m=m, max_iter=100, ftol=1e-12)
    for E, seed in zip((4, 13), nh.HISTORY_CASES[(m, l2)]):
        ref, mx, spread, wraps = nh.history_conditions(nh.history_batch(E, seed), kw)
        assert mx >= 15 and wraps > 0 and (E != 4 or spread >= 5), (E, mx, spread, wraps)
        assert np.all(ref["status"] == 0)
