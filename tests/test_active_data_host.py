"""CPU: the active-data cap as gdmix_amd/active_data.py states it (include/gdmix_re.h, "active-data cap") — the known answers of the key and
of the selection, the properties the header promises (order-free for distinct uids, nested in K, exact weights, consistent pointers), and
the two flags at parse time."""
import dataclasses

import numpy as np
import pytest

from gdmix_amd import active_data as ad
from gdmix_amd import downsample as ds
from gdmix_amd import solver as S
from gdmix_amd.params import REParams
import active_data_helpers as A

KEYS = [(0, 0, 0xa706dd2f4d197e6f), (1, 0, 0x5e41ab087439611e), (0, 1, 0x08b4fda8c892b50e), (20240603, 123456789, 0xd9c4c3685399dfb6),
        (7, -1, 0xa9a96b699dc41760), (7, -2 ** 63, 0x7e44eb9e75b86b14)]


@pytest.mark.parametrize("seed,uid,want", KEYS)
def test_key_known_answers(seed, uid, want):
    k = ad.key(seed, np.array([uid], np.int64))
    assert k.dtype == np.uint64 and int(k[0]) == want
    assert int(k[0]) >> 32 == int(ds.draw(seed, np.array([uid], np.int64))[0])


def test_key_is_the_draw_with_its_low_half():
    uid = np.random.default_rng(1).integers(-2 ** 63, 2 ** 63 - 1, 1000, dtype=np.int64)
    assert np.array_equal(ad.key(9, uid) >> np.uint64(32), ds.draw(9, uid))


@pytest.mark.parametrize("K,rows", [(4, [0, 5, 8, 10]), (5, [0, 5, 8, 9, 10])])
def test_selection_known_answer(K, rows):
    uid = np.arange(100, 112, dtype=np.int64)
    kept = ad.keep_mask([0, 12], uid, K, 5)
    assert np.flatnonzero(kept).tolist() == rows


@pytest.mark.parametrize("K", A.KS)
def test_kept_uids_do_not_depend_on_the_order_of_an_entitys_rows(K):
    rng = np.random.default_rng(K)
    erp = np.array([0, 40, 40 + 3 * K + 7, 40 + 3 * K + 7 + 2000], np.int64)
    uid = rng.permutation(10 ** 6)[:erp[-1]].astype(np.int64) - 500_000
    kept = ad.keep_mask(erp, uid, K, 11)
    shuffled = uid.copy()
    for e in range(3):
        shuffled[erp[e]:erp[e + 1]] = rng.permutation(uid[erp[e]:erp[e + 1]])
    kept_s = ad.keep_mask(erp, shuffled, K, 11)
    for e in range(3):
        s = slice(erp[e], erp[e + 1])
        assert set(uid[s][kept[s]]) == set(shuffled[s][kept_s[s]])
        assert kept[s].sum() == min(K, erp[e + 1] - erp[e])
    assert not np.array_equal(kept, ad.keep_mask(erp, uid, K, 12))      # another seed, another sample


def test_the_kept_set_is_nested_in_K():
    b = A.edge_batch(64)
    prev = None
    for K in (1, 2, 3, 63, 64, 65, 100, 1024, 1025, 6000):
        kept = ad.keep_mask(b.ent_row_ptr, b.uid, K, A.SEED)
        assert np.array_equal(np.add.reduceat(kept.astype(np.int64), b.ent_row_ptr[:-1]), np.minimum(b.ent_n(), K))      # (no entity of this batch is empty)
        if prev is not None:
            assert not (prev & ~kept).any()
        prev = kept
    assert prev.all()


@pytest.mark.parametrize("with_weight", [True, False])
@pytest.mark.parametrize("K", A.KS)
def test_weights_are_one_fp64_product_and_quotient_rounded_once(K, with_weight):
    b = A.edge_batch(K, with_weight)
    h = A.host_cap(b, K)
    n = np.repeat(b.ent_n(), b.ent_n())[h["kept_rows"]]
    w = (np.ones(b.N, np.float32) if b.weight is None else b.weight)[h["kept_rows"]]
    want = np.where(n > K, ((w.astype(np.float64) * n.astype(np.float64)) / np.float64(K)).astype(np.float32), w)
    assert h["weight"].dtype == np.float32 and np.array_equal(h["weight"].view(np.uint32), want.view(np.uint32))
    assert (n > K).any() and (n <= K).any()
    full = ad.scaled_weight(b.ent_row_ptr, b.weight, K)
    untouched = np.repeat(b.ent_n(), b.ent_n()) <= K
    assert np.array_equal(full[untouched], (np.ones(b.N, np.float32) if b.weight is None else b.weight)[untouched])


@pytest.mark.parametrize("K", A.KS)
def test_apply_host_gives_consistent_pointers(K):
    b = A.edge_batch(K)
    h = A.host_cap(b, K)
    kept, kept_nnz = h["y"].size, h["val"].size
    assert h["ent_row_ptr"][0] == 0 and h["ent_row_ptr"][-1] == kept == h["kept_rows"].size == h["offset"].size == h["weight"].size
    assert h["row_nnz_ptr"][0] == 0 and h["row_nnz_ptr"][-1] == kept_nnz == h["col_global"].size
    assert np.array_equal(np.diff(h["ent_row_ptr"]), np.minimum(b.ent_n(), K))
    assert np.all(np.diff(h["kept_rows"]) > 0)                                            # kept rows keep their order
    assert np.array_equal(np.diff(h["row_nnz_ptr"]), np.diff(b.row_nnz_ptr)[h["kept_rows"]])
    r = int(h["kept_rows"][kept // 2])
    k = kept // 2
    assert np.array_equal(h["col_global"][h["row_nnz_ptr"][k]:h["row_nnz_ptr"][k + 1]], b.col_global[b.row_nnz_ptr[r]:b.row_nnz_ptr[r + 1]])
    A.capped_batch(b, K).validate()


def test_an_empty_batch_and_a_bound_above_every_entity():
    h = A.host_cap(A.empty_batch(), 3)
    assert h["ent_row_ptr"].tolist() == [0] and h["row_nnz_ptr"].tolist() == [0] and h["y"].size == 0
    b = A.edge_batch(2, with_weight=False)
    h = A.host_cap(b, 5000)
    assert np.array_equal(h["ent_row_ptr"], b.ent_row_ptr) and np.array_equal(h["col_global"], b.col_global)
    assert np.array_equal(h["weight"], np.ones(b.N, np.float32))


# ---- the flags ----------------------------------------------------------------------------------------------------------------------
BASE = ["--metadata_file=m.json", "--output_model_dir=out", "--feature_bag=per_user", "--partition_entity=user_id"]


def test_flag_defaults_and_values():
    p = REParams.__from_argv__(BASE)
    assert p.active_data_upper_bound is None and p.active_data_seed == 0
    p = REParams.__from_argv__(BASE + ["--active_data_upper_bound=1000", "--active_data_seed=7"])
    assert p.active_data_upper_bound == 1000 and p.active_data_seed == 7 and isinstance(p.active_data_upper_bound, int)
    assert REParams.__from_argv__(BASE + ["--active_data_upper_bound", "1"]).active_data_upper_bound == 1
    assert ad.check_upper_bound(1) == 1 and ad.check_upper_bound("12") == 12


@pytest.mark.parametrize("bad", ["0", "-1", "1.5", "nan", "many"])
def test_bad_bounds_are_refused_at_parse_time(bad):
    with pytest.raises(ValueError):
        REParams.__from_argv__(BASE + [f"--active_data_upper_bound={bad}"])
    with pytest.raises(ValueError):
        ad.check_upper_bound(bad)


@pytest.mark.parametrize("bad", [0, -1, 1.5, float("nan"), float("inf"), True])
def test_bad_bounds_are_refused_when_the_parameters_are_built_directly(bad):
    with pytest.raises(ValueError, match="active_data_upper_bound"):
        REParams(metadata_file="m.json", output_model_dir="out", feature_bag="per_user", active_data_upper_bound=bad)


REFUSED = [("--l2_reg_weights=1,0.1", "--l2_reg_weights"), ("--rebalance_entities=True", "--rebalance_entities"),
           ("--incremental_training=True", "--incremental_training"), ("--feature_normalization=scale_with_standard_deviation", "--feature_normalization"),
           ("--feature_normalization=scale_with_max_magnitude", "--feature_normalization")]


@pytest.mark.parametrize("flag,name", REFUSED)
def test_what_the_bound_does_not_run_with(flag, name):
    with pytest.raises(ValueError) as err:
        REParams.__from_argv__(BASE + ["--active_data_upper_bound=10", flag])
    assert str(err.value).startswith(f"--active_data_upper_bound does not run with {name}: ")
    REParams.__from_argv__(BASE + [flag])                                                  # the flag alone stays valid


@pytest.mark.parametrize("extra", [["--feature_normalization=none"], ["--random_effect_variance_mode=full"], ["--metric_output_dir=m"],
                                   ["--features_to_samples_ratio=0.5"], ["--disable_random_effect_scoring_after_training=True"]])
def test_what_the_bound_runs_with(extra):
    p = REParams.__from_argv__(BASE + ["--active_data_upper_bound=10"] + extra)
    assert p.active_data_upper_bound == 10


def test_the_fixed_effect_has_no_such_flag():
    from gdmix_amd.fe_model import FixedLRParams
    from gdmix_amd.params import LRParams, Params, SchemaParams
    for cls in (FixedLRParams, LRParams, Params, SchemaParams):
        names = {f.name for f in dataclasses.fields(cls)}
        assert "active_data_upper_bound" not in names and "active_data_seed" not in names, cls


def test_the_new_symbols_are_exported():
    for name in ("gdmix_re_cap_workspace_bytes", "gdmix_re_cap_plan", "gdmix_re_cap_apply", "gdmix_re_set_cap_small_max"):
        assert name in S.EXPORTED_SYMBOLS
    assert hasattr(S.REDeviceSolver, "cap_samples") and hasattr(S.REDeviceSolver, "set_cap_small_max")
