"""CPU: --features_to_samples_ratio (include/gdmix_re.h, "feature selection") — the flag and its refusals, k_e, the numpy statement
(gdmix_amd/feature_selection.py) against exact rational arithmetic, the singleton identity, and the conditions under which
tests/test_gpu_feature_selection.py compares the device's keys (feature_selection_helpers.check_conditions), on the batches it uses."""
from fractions import Fraction

import numpy as np
import pytest

from gdmix_amd import feature_selection as fs
from gdmix_amd.batch import RawBatch
from gdmix_amd.params import REParams
import feature_selection_helpers as F

BASE = ["--metadata_file=m.json", "--output_model_dir=out", "--feature_bag=per_user"]


def test_the_flag_parses_and_is_off_by_default():
    assert REParams.__from_argv__(BASE).features_to_samples_ratio is None
    p = REParams.__from_argv__(BASE + ["--features_to_samples_ratio=0.5"])
    assert p.features_to_samples_ratio == 0.5 and isinstance(p.features_to_samples_ratio, float)
    assert REParams.__from_argv__(BASE + ["--features_to_samples_ratio=1e9"]).features_to_samples_ratio == 1e9


@pytest.mark.parametrize("value", ["0", "-0.5", "nan", "inf"])
def test_a_ratio_that_is_not_finite_and_positive_is_refused(value):
    with pytest.raises(ValueError, match="--features_to_samples_ratio=.*a finite ratio above 0"):
        REParams.__from_argv__(BASE + [f"--features_to_samples_ratio={value}"])


@pytest.mark.parametrize("flag,message", [
    ("--incremental_training=True", "--features_to_samples_ratio does not run with --incremental_training: a prior feature the selection drops"),
    ("--l2_reg_weights=1,0.1", "--features_to_samples_ratio does not run with --l2_reg_weights: a sweep over selected features is not implemented"),
    ("--feature_normalization=scale_with_standard_deviation", "--features_to_samples_ratio does not run with --feature_normalization: the correlation is taken"),
    ("--rebalance_entities=True", "--features_to_samples_ratio does not run with --rebalance_entities: the selection does not travel"),
])
def test_flags_the_selection_does_not_run_with_are_refused_at_parse_time(flag, message):
    with pytest.raises(ValueError) as err:
        REParams.__from_argv__(BASE + ["--features_to_samples_ratio=0.5", flag])
    assert message in str(err.value)
    REParams.__from_argv__(BASE + [flag])      # (each is fine without the ratio)


def test_feature_normalization_none_runs_with_the_ratio():
    assert REParams.__from_argv__(BASE + ["--features_to_samples_ratio=0.5", "--feature_normalization=none"]).features_to_samples_ratio == 0.5


def test_the_fixed_effect_has_no_such_flag():
    from gdmix_amd import fe_model
    import dataclasses
    for cls in vars(fe_model).values():
        if dataclasses.is_dataclass(cls) and isinstance(cls, type):
            assert "features_to_samples_ratio" not in {f.name for f in dataclasses.fields(cls)}, cls


def test_k_on_edge_values():
    assert fs.k_of(0.5, 16, 60) == 8
    assert fs.k_of(0.25, 1, 3) == 1          # ceil(0.25) = 1: an entity with a sample keeps a feature
    assert fs.k_of(0.5, 3, 60) == 2          # ceil(1.5)
    assert fs.k_of(0.5, 4, 2) == 2           # never more than d_e
    assert fs.k_of(0.5, 4, 0) == 0
    assert fs.k_of(0.5, 0, 7) == 0           # no samples: nothing is kept
    assert fs.k_of(1e9, 16, 60) == 60
    assert fs.k_of(1e300, 2 ** 31 - 1, 2 ** 31 - 1) == 2 ** 31 - 1      # the product exceeds int64: still d_e
    assert fs.k_of(0.1, 10, 5) == 1 and fs.k_of(0.1, 11, 5) == 2        # 0.1 * 10 rounds to exactly 1.0 in fp64, 0.1 * 11 lies above 1
    assert fs.k_of(1.0 / 3.0, 3, 5) == 1
    assert fs.k_of(5e-324, 1, 5) == 1
    n, d = np.array([16, 1, 3, 4, 0, 16]), np.array([60, 3, 60, 2, 7, 60])
    assert np.array_equal(fs.k_all(0.5, n, d), [fs.k_of(0.5, a, b) for a, b in zip(n, d)])
    assert np.array_equal(fs.k_all(1e300, n, d), np.where(n > 0, d, 0))
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            fs.k_of(bad, 4, 4)


def test_slots_are_the_oracle_packs():
    from oracle import oracle
    b = F.batch("edge")
    pk = oracle.pack(b.ent_row_ptr, b.row_nnz_ptr, b.col_global)
    fp, uniq, nnz_slot, _ = fs.slots(b)
    assert np.array_equal(fp, pk["ent_feat_ptr"]) and np.array_equal(uniq, pk["unique_global"])
    nnz_ent = np.repeat(np.arange(b.E), np.diff(b.row_nnz_ptr[b.ent_row_ptr]))
    assert np.array_equal(nnz_slot, fp[nnz_ent] + pk["csr_col"])
    names = F.edge_batch()[1]
    d = dict(zip(names, np.diff(fp)))
    assert (d["d_63"], d["d_64"], d["d_65"]) == (63, 64, 65)
    n = dict(zip(names, np.diff(b.ent_row_ptr)))
    assert n["n_is_1"] == 1 and fs.k_of(0.5, n["k_is_1"], d["k_is_1"]) == 1 and fs.k_of(0.25, n["k_is_1"], d["k_is_1"]) == 1
    assert fs.k_of(0.5, n["k_is_d_minus_1_at_0.5"], d["k_is_d_minus_1_at_0.5"]) == d["k_is_d_minus_1_at_0.5"] - 1
    assert fs.k_of(0.25, n["k_is_d_minus_1_at_0.25"], d["k_is_d_minus_1_at_0.25"]) == d["k_is_d_minus_1_at_0.25"] - 1


@pytest.mark.parametrize("name", F.NAMES)
def test_the_conditions_of_the_key_bound_hold_on_the_reference(name):
    got = F.check_conditions(F.reference(name))
    print(name, got)


@pytest.mark.parametrize("name", F.NAMES)
def test_the_numpy_statement_against_the_exact_reference(name):
    ref = F.reference(name)
    _, _, key = fs.keys(ref["batch"])
    assert key.dtype == np.float32 and key.size == ref["slots"][1].size and np.all(key >= 0)
    F.check_keys(ref, key)


def test_the_edge_batch_holds_what_it_says():
    b, names = F.edge_batch()
    ref = F.reference("edge")
    fp, uniq, key = fs.keys(b)
    e = {nm: k for k, nm in enumerate(names)}
    col = lambda nm, g: int(fp[e[nm]] + np.searchsorted(uniq[fp[e[nm]]:fp[e[nm] + 1]], g))
    for nm in ("n_is_1", "labels_all_equal"):
        assert np.all(key[fp[e[nm]]:fp[e[nm] + 1]] == 0.0)
        assert all(ref["cols"][f]["kind"] == "zero" for f in range(fp[e[nm]], fp[e[nm] + 1]))
    f = col("constant_column_0.1f_x40", 399)
    assert ref["cols"][f]["kind"] == "zero" and ref["cols"][f]["Bx"] == 0 and key[f] == 0.0
    m = fs.moments(b)
    assert key[col("identical_columns_and_a_double", 510)] == key[col("identical_columns_and_a_double", 511)] > 0
    assert key[col("identical_columns_and_a_double", 520)] == key[col("identical_columns_and_a_double", 521)] > 0      # a scaling by 2 is exact
    f = col("duplicated_cell", 450)
    assert m["Sx"][f] == (0.75 - 1.5) + (2.25 + 0.125) and m["Sxx"][f] == (0.75 - 1.5) ** 2 + (2.25 + 0.125) ** 2
    keep = fs.select(fp, np.diff(b.ent_row_ptr), key, 0.5)
    k = fp[e["n_is_1"]]
    assert list(keep[k:k + 3]) == [True, False, False]      # all keys 0: the lowest index wins
    a, c = col("identical_columns_and_a_double", 510), col("identical_columns_and_a_double", 511)
    assert keep[a] >= keep[c]


def test_the_singleton_identity():
    """A feature that occurs in one sample only: q = (n y_i - Sy)^2 / (n - 1), whatever its value — exactly, and so do the keys tie."""
    y = np.float32([1, 0, 0, 1, 1, 0, 1])
    n = y.size
    vals = np.float32([0.3, -7.0, 1e-3, 123.0, 1.0, 0.5, 2.0])
    b = RawBatch(np.array([0, n]), np.arange(n + 1), np.arange(n) + 10, vals, y, np.zeros(n, np.float32))
    ref = F.exact_entity(b, fs.slots(b), 0)
    Sy = int(y.sum())
    for i in range(n):
        assert ref[i]["q"] == Fraction((n * int(y[i]) - Sy) ** 2, n - 1)
    _, _, key = fs.keys(b)
    want = np.float32([(n * v - Sy) ** 2 / (n - 1) for v in y.astype(np.float64)])
    assert np.allclose(key, want, rtol=2.0 ** -22, atol=0.0)
    keep = fs.select(np.array([0, n]), np.array([n]), want, 0.5)      # k = 4: the labels 0 score 16/6, the labels 1 score 9/6
    assert list(np.flatnonzero(keep)) == [0, 1, 2, 5]      # ... and of the four tied features with label 1 the lowest index


@pytest.mark.parametrize("ratio", F.RATIOS)
def test_filtering_keeps_rows_and_drops_only_dropped_features(ratio):
    b = F.batch("edge")
    fb, keep, key, counts = fs.select_batch(b, ratio)
    fp, uniq, nnz_slot, _ = fs.slots(b)
    assert fb.N == b.N and fb.E == b.E and np.array_equal(fb.y, b.y) and np.array_equal(fb.offset, b.offset)
    assert counts["kept_nnz"] == fb.Z and counts["kept"] + counts["dropped"] == counts["features"] == uniq.size
    assert np.array_equal(fb.col_global, b.col_global[keep[nnz_slot]]) and np.array_equal(fb.val, b.val[keep[nnz_slot]])
    k = fs.k_all(ratio, np.diff(b.ent_row_ptr), np.diff(fp))
    assert np.array_equal(np.add.reduceat(keep.astype(np.int64), fp[:-1]), k)
    fp2, uniq2, _, _ = fs.slots(fb)
    assert np.array_equal(np.diff(fp2), k) and np.array_equal(uniq2, uniq[keep])
    assert counts["affected"] == int((k < np.diff(fp)).sum())
    again, keep1, _, counts1 = fs.select_batch(b, 1e9)
    assert keep1.all() and counts1["affected"] == 0 and np.array_equal(again.col_global, b.col_global) and np.array_equal(again.row_nnz_ptr, b.row_nnz_ptr)
