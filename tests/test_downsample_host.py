"""Host: the numpy statement of down-sampling (gdmix_amd/downsample.py; include/gdmix_re.h, "down-sampling") against the known answers of
the definition, and the stage's two flags (--down_sampling_rate / --down_sampling_seed) at parse time."""
import numpy as np
import pytest

from gdmix_amd import constants
from gdmix_amd import downsample as ds
from gdmix_amd.fe_model import FixedEffectLRModelLBFGS, FixedLRParams

DRAWS = [(0, 0, 2802244911), (1, 0, 1581361928), (0, 1, 146079144), (20240603, 123456789, 3653550952), (7, -1, 2846452585),
         (7, -2 ** 63, 2118445982)]


def test_mix_and_draw_known_answers():
    assert ds.mix(0) == 0xE220A8397B1DCDAF
    assert int(ds.mix(np.zeros(1, np.uint64))[0]) == 0xE220A8397B1DCDAF
    for seed, uid, want in DRAWS:
        assert int(ds.draw(seed, np.array([uid], np.int64))[0]) == want, (seed, uid)
    together = ds.draw(7, np.array([-1, -2 ** 63], np.int64))
    assert together.dtype == np.uint64 and together.tolist() == [2846452585, 2118445982]


def test_threshold_is_the_exact_product_truncated():
    assert [ds.threshold(r) for r in (0.1, 0.25, 0.5, 1.0, 2.0 ** -33)] == [429496729, 1 << 30, 1 << 31, 1 << 32, 0]
    for bad in (0.0, -0.5, 1.0000001, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            ds.threshold(bad)


def _ten_rows():
    uid = np.array([5, -3, 17, 17, 0, 123456789, -2 ** 63, 2 ** 62, 44, 9], np.int64)      # (rows 2 and 3 share a uid)
    y = np.array([1, 0, 0, 0, 1, 0, 0, 1, 0, 0], np.float32)
    w = np.array([0.5, 1.5, 2.0, 0.25, 3.0, 1.0, 0.7, 1.25, 0.1, 4.0], np.float32)
    return uid, y, w


def test_keep_mask_and_scaled_weight_on_ten_rows():
    uid, y, w = _ten_rows()
    seed, rate = 11, 0.25
    sampled = np.array([int(ds.draw(seed, uid[i:i + 1])[0]) < (1 << 30) for i in range(10)])
    assert 0 < sampled.sum() < 10 and sampled[2] == sampled[3]                            # equal uids share a fate
    assert np.array_equal(ds.keep_mask(uid, y, rate, seed, False), sampled)
    with_pos = ds.keep_mask(uid, y, rate, seed, True)
    assert np.array_equal(with_pos, sampled | (y > 0.5)) and with_pos[[0, 4, 7]].all()    # positives survive
    assert not sampled[[0, 4, 7]].all()                                                  # ... and at least one of them only for that reason
    scaled = ds.scaled_weight(w, y, rate, False)
    assert scaled.dtype == np.float32 and np.array_equal(scaled, np.float32(np.float64(w) / rate))
    neg_only = ds.scaled_weight(w, y, rate, True)
    assert np.array_equal(neg_only[y > 0.5], w[y > 0.5]) and np.array_equal(neg_only[y <= 0.5], scaled[y <= 0.5])
    assert np.array_equal(ds.scaled_weight(None, y, 0.1, False), np.full(10, np.float32(np.float64(1.0) / 0.1)))
    assert np.array_equal(ds.scaled_weight(None, y, 0.1, True), np.where(y > 0.5, np.float32(1.0), np.float32(np.float64(1.0) / 0.1)))
    # the filtered arrays: kept rows in their order, non-zeros of the kept rows, entity pointers through the scan
    rp = np.array([0, 2, 2, 5, 6, 6, 9, 10, 12, 12, 15], np.int64)
    col, val = np.arange(15, dtype=np.int64) * 3, np.arange(15, dtype=np.float32) / 4
    out = ds.apply_host(np.array([0, 4, 4, 10]), rp, col, val, y, None, w, uid, rate, seed, True)
    rows = np.flatnonzero(with_pos)
    assert np.array_equal(out["kept_rows"], rows) and np.array_equal(out["y"], y[rows]) and np.array_equal(out["weight"], neg_only[rows])
    assert np.array_equal(out["offset"], np.zeros(rows.size, np.float32))
    assert np.array_equal(out["col_global"], np.concatenate([col[rp[i]:rp[i + 1]] for i in rows]))
    assert np.array_equal(out["val"], np.concatenate([val[rp[i]:rp[i + 1]] for i in rows]))
    assert np.array_equal(np.diff(out["row_nnz_ptr"]), np.diff(rp)[rows]) and out["row_nnz_ptr"][0] == 0
    assert out["ent_row_ptr"].tolist() == [0, int(with_pos[:4].sum()), int(with_pos[:4].sum()), rows.size]


def test_mask_does_not_depend_on_shards_or_row_order():
    rng = np.random.default_rng(4)
    uid = rng.integers(-2 ** 63, 2 ** 63 - 1, 5000, dtype=np.int64)
    y = (rng.random(5000) < 0.1).astype(np.float32)
    whole = ds.keep_mask(uid, y, 0.25, 9, True)
    kept = set(uid[whole].tolist())
    perm = rng.permutation(5000)
    assert np.array_equal(ds.keep_mask(uid[perm], y[perm], 0.25, 9, True), whole[perm])
    for shards in (2, 3, 7):
        got = set()
        for r in range(shards):
            rows = np.arange(r, 5000, shards)
            got |= set(uid[rows][ds.keep_mask(uid[rows], y[rows], 0.25, 9, True)].tolist())
        assert got == kept
    assert set(uid[ds.keep_mask(uid, y, 0.25, 10, True)].tolist()) != kept      # (another seed, another sample)


@pytest.mark.parametrize("n", [600, 20_000, 100_000])
@pytest.mark.parametrize("rate", [0.1, 0.25, 0.5])
def test_kept_count_within_four_sigma(n, rate):
    """A cap on the hash, not a measurement: the nine cases lie between -2.01 and +0.82 sigma (9 809 of 100 000 at 0.1)."""
    uid = 3 * np.arange(n, dtype=np.int64) + 11
    kept = int(ds.keep_mask(uid, np.zeros(n, np.float32), rate, 5, False).sum())
    sigma = np.sqrt(n * rate * (1.0 - rate))
    print(f"n {n} rate {rate}: kept {kept}, {(kept - n * rate) / sigma:+.2f} sigma")
    assert abs(kept - n * rate) <= 4.0 * sigma
    if (n, rate) == (100_000, 0.1):
        assert kept == 9809


# ---- the flags -----------------------------------------------------------------------------------------------------------------------
BASE = ["--metadata_file=md.json", "--output_model_dir=models"]


def test_params_default_and_parse():
    p = FixedLRParams.__from_argv__(BASE)
    assert p.down_sampling_rate == 1.0 and p.down_sampling_seed == 0 and not p.down_sampling_given()
    p = FixedLRParams.__from_argv__(BASE + ["--down_sampling_rate=0.25", "--down_sampling_seed=3"])
    assert p.down_sampling_rate == 0.25 and p.down_sampling_seed == 3 and p.down_sampling_given()
    assert FixedLRParams.__from_argv__(BASE + ["--down_sampling_rate=1"]).down_sampling_rate == 1.0


@pytest.mark.parametrize("text", ["0", "0.0", "-0.1", "1.5", "nan", "inf", "abc", ""])
def test_params_refuse_a_bad_rate_at_parse_time(text):
    with pytest.raises(ValueError):
        FixedLRParams.__from_argv__(BASE + [f"--down_sampling_rate={text}"])


def test_params_refuse_a_bad_rate_given_directly():
    for bad in (0, -1.0, 2, float("nan"), "x", None):
        with pytest.raises(ValueError):
            FixedLRParams(metadata_file="md.json", output_model_dir="models", down_sampling_rate=bad)
    with pytest.raises(ValueError):
        FixedLRParams.__from_argv__(BASE + ["--down_sampling_seed=1.5"])


def _model(extra):
    m = FixedEffectLRModelLBFGS.__new__(FixedEffectLRModelLBFGS)      # check_request reads the parameters alone
    m.model_params = FixedLRParams.__from_argv__(BASE + extra)
    m.model_type = constants.LOGISTIC_REGRESSION
    return m


def test_flags_are_refused_for_inference():
    ctx = {constants.NUM_WORKERS: 1, constants.TASK_INDEX: 0, constants.IS_CHIEF: True}
    for extra in (["--down_sampling_rate=0.5"], ["--down_sampling_seed=4"]):
        with pytest.raises(ValueError, match="down_sampling"):
            _model(extra).check_request(ctx, constants.ACTION_INFERENCE)
        _model(extra).check_request(ctx, constants.ACTION_TRAIN)
    _model([]).check_request(ctx, constants.ACTION_INFERENCE)
    _model(["--down_sampling_rate=1.0"]).check_request(ctx, constants.ACTION_INFERENCE)
