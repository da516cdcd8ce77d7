"""CPU: the resident coordinate descent (gdmix_amd/descent.py) without a device — its numpy statements of the row grouping and of the
offset sum against brute-force loops, the multi-pass descent restated on the fp64 oracle (tests/descent_oracle.py), the refusals, and
the new entry points in the header, the symbol list and the library."""
import os
import re

import numpy as np
import pytest

from gdmix_amd import chain, descent, solver
from gdmix_amd.descent import Coordinate, DataSet

import descent_oracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("gdmix_re_group_workspace_bytes", "gdmix_re_group_rows", "gdmix_re_rows_gather_f32", "gdmix_re_rows_scatter_f32", "gdmix_re_offsets_combine")


def random_bag(rng, n, dim, empty_front=0, empty_back=0):
    """A CSR bag of n rows with 0 .. 6 non-zeros each (some rows in between empty too), ascending columns."""
    k = rng.integers(0, 7, n)
    k[:empty_front] = 0
    if empty_back:
        k[n - empty_back:] = 0
    ptr = np.concatenate([[0], np.cumsum(k)]).astype(np.int64)
    col = np.concatenate([np.sort(rng.choice(dim, int(c), replace=False)) for c in k] + [np.zeros(0, np.int64)]).astype(np.int64)
    val = rng.standard_normal(int(ptr[-1])).astype(np.float32)
    return ptr, col, val


def group_brute(ptr, col, val, idx, E):
    """The definition with loops: entities ascending, an entity's rows in input order, rows outside [0, E) left out."""
    row_of, present, erp, out_ptr, out_col, out_val = [], [], [0], [0], [], []
    for e in range(E):
        mine = [i for i in range(len(idx)) if idx[i] == e]
        if not mine:
            continue
        present.append(e)
        for i in mine:
            row_of.append(i)
            out_col += list(col[ptr[i]:ptr[i + 1]])
            out_val += list(val[ptr[i]:ptr[i + 1]])
            out_ptr.append(len(out_col))
        erp.append(len(row_of))
    return dict(row_of=np.array(row_of, np.int32), present=np.array(present, np.int32), ent_row_ptr=np.array(erp, np.int64),
                row_nnz_ptr=np.array(out_ptr, np.int64), col_global=np.array(out_col, np.int64), val=np.array(out_val, np.float32))


@pytest.mark.parametrize("seed", range(6))
def test_group_rows_host_is_the_definition(seed):
    rng = np.random.default_rng(seed)
    n, E, dim = int(rng.integers(1, 90)), int(rng.integers(1, 12)), 9
    ptr, col, val = random_bag(rng, n, dim, empty_front=seed % 3, empty_back=(seed + 1) % 3 if n > 4 else 0)
    idx = rng.integers(-1, E, n)
    idx[idx == E // 2] = -1 if seed % 2 else E - 1      # an entity that owns no row: E' < E
    if seed == 5:
        idx[:] = -1                                      # nothing grouped
    got = descent.group_rows_host(ptr, col, val, idx, E)
    want = group_brute(ptr, col, val, idx, E)
    for k, w in want.items():
        assert got[k].dtype == w.dtype and np.array_equal(got[k], w), k
    c = got["counts"]
    assert c == dict(rows=n, grouped=want["row_of"].size, grouped_nnz=want["col_global"].size, entities=want["present"].size,
                     left_out=n - want["row_of"].size)
    assert np.array_equal(got["row_of"], np.flatnonzero(idx >= 0)[np.argsort(idx[idx >= 0], kind="stable")])


@pytest.mark.parametrize("K,skip,with_base,with_map", [(1, -1, False, False), (1, 0, True, True), (3, 1, True, False), (3, 0, False, True), (8, 7, True, True),
                                                       (8, -1, False, False), (8, 3, True, True)])
def test_offsets_combine_host_adds_in_fp32_from_left_to_right(K, skip, with_base, with_map):
    rng = np.random.default_rng(K * 10 + skip + 1)
    n = 57
    parts = [(rng.standard_normal(n) * 10.0 ** rng.integers(-3, 4)).astype(np.float32) for _ in range(K)]
    base = rng.standard_normal(n).astype(np.float32) if with_base else None
    row_of = rng.permutation(n)[:41].astype(np.int32) if with_map else None
    got = descent.offsets_combine_host(n, base, parts, skip, row_of)
    rows = range(n) if row_of is None else row_of
    want = []
    for r in rows:
        acc = np.float32(0.0) if base is None else base[r]
        for k in range(K):
            if k != skip:
                acc = np.float32(acc + parts[k][r])
        want.append(acc)
    assert got.dtype == np.float32 and np.array_equal(got.view(np.uint32), np.array(want, np.float32).view(np.uint32))
    # the order matters: the sum taken in fp64 and rounded once differs somewhere on these magnitudes (K >= 3)
    if K == 8 and skip == -1:
        once = np.sum([p.astype(np.float64) for p in parts], axis=0).astype(np.float32)
        assert not np.array_equal(once, got)


def test_gather_and_scatter_host():
    rng = np.random.default_rng(3)
    src = rng.standard_normal(20).astype(np.float32)
    row_of = np.array([7, 3, 19, 0], np.int32)
    assert np.array_equal(descent.rows_gather_host(src, row_of), src[[7, 3, 19, 0]])
    back = descent.rows_scatter_host(src[:4], row_of, 20)
    assert np.array_equal(np.flatnonzero(back), [0, 3, 7, 19]) and np.array_equal(back[row_of], src[:4])


@pytest.fixture(scope="module")
def restated():
    data = chain.make_dataset(120, 200, 8000)
    tr, va = np.flatnonzero(data["train"]), np.flatnonzero(~data["train"])
    y = data["response"].astype(np.float32)
    return descent_oracle.run(chain.resident_coordinates(data, re_regularize_bias=True), y[tr], 4, y[va])


def test_every_update_of_four_passes_lowers_the_joint_objective(restated):
    """make_dataset(120, 200, 8000), l2 = 1, intercepts regularised on the two random effects and not on the global model, 4 passes on
    the fp64 oracle: F falls at each of the 12 updates (the smallest fall is 0.311: no tolerance), and one pass is visibly unconverged —
    coefficients still move by more than 0.1 in pass 2."""
    F = restated["F"]
    assert F.shape == (4, 3)
    steps = -np.diff(np.concatenate([[np.inf], F.ravel()]))
    assert (steps > 0).all(), F
    assert restated["moved"][1] > 0.1 and restated["moved"][3] < restated["moved"][1]


def test_validation_auc_after_four_passes_is_at_least_that_after_one(restated):
    a = restated["validation_auc"]
    assert a[3, -1] >= a[0, -1] and a[0, 0] < a[0, 1] < a[0, 2]


def _request(n=6, coords=None, **kw):
    ptr = np.arange(n + 1, dtype=np.int64)
    bag = (ptr, np.zeros(n, np.int64), np.ones(n, np.float32), 2)
    train = DataSet(label=kw.pop("label", np.array([0, 1] * (n // 2), np.float32)), uid=np.arange(n, dtype=np.int64))
    coords = coords if coords is not None else [Coordinate("global", bag), Coordinate("per_user", bag, entity=np.arange(n, dtype=np.int64) % 3)]
    return (train, coords, kw.pop("passes", 1), kw.pop("model_type", chain.LOGISTIC))


def test_refusals():
    n = 6
    bag = (np.arange(n + 1, dtype=np.int64), np.zeros(n, np.int64), np.ones(n, np.float32), 2)
    descent.check_request(*_request())
    with pytest.raises(ValueError, match="passes must be at least 1"):
        descent.check_request(*_request(passes=0))
    with pytest.raises(ValueError, match="9 coordinates"):
        descent.check_request(*_request(coords=[Coordinate(f"c{i}", bag) for i in range(9)]))
    with pytest.raises(ValueError, match="two coordinates are named 'a'"):
        descent.check_request(*_request(coords=[Coordinate("a", bag), Coordinate("a", bag)]))
    with pytest.raises(ValueError, match=r"the entity array has \(5,\) entries, the data set has 6 samples"):
        descent.check_request(*_request(coords=[Coordinate("u", bag, entity=np.arange(5))]))
    with pytest.raises(ValueError, match="labels must be finite and >= 0"):
        descent.check_request(*_request(label=np.array([1, 2, -1, 0, 3, 1], np.float32), model_type=chain.POISSON))
    descent.check_request(*_request(label=np.array([1, 2, 0, 0, 3, 1], np.float32), model_type=chain.POISSON))
    with pytest.raises(ValueError, match="model type 'svm'"):
        descent.check_request(*_request(model_type="svm"))
    with pytest.raises(ValueError, match="validation data needs its validation_bag"):
        train, coords, passes, mt = _request()
        descent.check_request(train, coords, passes, mt, validation=train)
    with pytest.raises(ValueError, match="model type"):
        chain.run_resident({}, model_type="svm")


def test_the_header_the_symbol_list_and_the_library_hold_the_new_entry_points():
    hdr = open(os.path.join(ROOT, "include", "gdmix_re.h")).read()
    declared = set(re.findall(r"GDMIX_API[^;(]*?\b(gdmix_\w+)\s*\(", hdr + open(os.path.join(ROOT, "include", "gdmix_fe.h")).read()))
    assert declared == set(solver.EXPORTED_SYMBOLS) and set(NEW_SYMBOLS) <= declared
    assert "(ABI 27) row grouping" in hdr and f"#define GDMIX_RE_COMBINE_MAX {solver.COMBINE_MAX}" in hdr
    assert descent.MAX_COORDINATES == solver.COMBINE_MAX
    from gdmix_amd import build
    build.build_library()
    lib = solver.load_library()
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name), name
    assert 0 < lib.gdmix_re_group_workspace_bytes(10, 3) < lib.gdmix_re_group_workspace_bytes(100000, 3)
    assert lib.gdmix_re_group_workspace_bytes(1 << 31, 3) == 0
