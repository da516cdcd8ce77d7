"""Feature normalisation, host side (gdmix_amd/feature_stats.py): shifts and finish against exact rationals, the numpy stand-in of the two
kernels, the statistics file, every refusal, and two gloo ranks against one."""
import json
import os
import subprocess
import sys
from fractions import Fraction

import numpy as np
import pytest

from gdmix_amd import feature_stats as fs
from gdmix_amd.fe_model import FixedLRParams
from gdmix_amd.params import REParams

HERE = os.path.dirname(os.path.abspath(__file__))


# ---- an exact reference: Python integers and Fractions ------------------------------------------------------------------------------------
def rint_fraction(q):
    """Round a Fraction to the nearest integer, ties to even."""
    f = q.numerator // q.denominator
    r = q - f
    if r > Fraction(1, 2) or (r == Fraction(1, 2) and f % 2 == 1):
        f += 1
    return f


def exact_moments(col, val, D, count=None):
    """-> count, max_abs, L, s1, s2, I1, I2 per feature by the header's definitions, in Python integers. count: forged counts (tests)."""
    cnt = [0] * D
    a = [0.0] * D
    for c, x in zip(col.tolist(), val.tolist()):
        cnt[c] += 1
        a[c] = max(a[c], abs(x))
    if count is not None:
        cnt = list(count)
    L, s1, s2, I1, I2 = [0] * D, [0] * D, [0] * D, [0] * D, [0] * D
    for j in range(D):
        if cnt[j] == 0 or a[j] == 0:
            continue
        E = int(np.floor(np.log2(a[j])))
        assert 2.0 ** E <= a[j] < 2.0 ** (E + 1)
        L[j] = min(31, 62 - int(cnt[j]).bit_length())
        s1[j] = 2 * L[j] - (E + 1)
        s2[j] = 2 * L[j] - 2 * (E + 1)
    for c, x in zip(col.tolist(), val.tolist()):
        if L[c] == 0:
            continue
        q = Fraction(x)
        I1[c] += rint_fraction(q * Fraction(2) ** s1[c])
        I2[c] += rint_fraction(q * q * Fraction(2) ** s2[c])
    return cnt, a, L, s1, s2, I1, I2


def exact_mean_var(N, L, s1, s2, I1, I2):
    mean, var = [], []
    for j in range(len(L)):
        if L[j] == 0:
            mean.append(Fraction(0))
            var.append(Fraction(0))
            continue
        m1 = Fraction(I1[j]) / Fraction(2) ** s1[j]
        m2 = Fraction(I2[j]) / Fraction(2) ** s2[j]
        mean.append(m1 / N)
        var.append(max(Fraction(0), (m2 - m1 * m1 / N) / (N - 1)) if N > 1 else Fraction(0))
    return mean, var


def ulps(x, q):
    """|x - q| in units of the last place of the double nearest to q."""
    if q == 0:
        return 0.0 if x == 0 else np.inf
    ref = float(q)
    return float(abs(Fraction(x) - q) / Fraction(np.spacing(abs(ref))))


def run_standin(D, chunks, kind=fs.SCALE_WITH_STANDARD_DEVIATION, N=None):
    acc = fs.NumpyAccumulator(D)
    return fs.collect(acc, lambda a: [a.add(c, v) for c, v in chunks], N, kind), acc


def small_case(seed=0, D=70, N=900):
    """Dense-ish data with every difficulty of the header: per-column scales over 26 decades, a constant dense column, a nearly constant
    one, a dead feature, negative values, tiny values inside a large column."""
    rng = np.random.default_rng(seed)
    rows = np.repeat(np.arange(N), 8)
    col = rng.integers(0, D - 4, rows.size)
    scale = np.exp(rng.uniform(-30, 30, D))
    val = (rng.standard_normal(rows.size) * scale[col]).astype(np.float32)
    tiny = (col == 3) & (rng.random(rows.size) < 0.3)
    val[tiny] *= np.float32(1e-20)
    # D-4: constant dense; D-3: nearly constant dense; D-2: dead; D-1: stored zeros only
    col = np.concatenate([col, np.full(N, D - 4), np.full(N, D - 3), np.full(5, D - 1)])
    near = np.float32(0.97) + (rng.integers(0, 3, N) * np.float32(2.0 ** -20)).astype(np.float32)
    val = np.concatenate([val, np.full(N, np.float32(0.3)), near, np.zeros(5, np.float32)]).astype(np.float32)
    return col.astype(np.int64), val, D, N


# ---- shifts and finish --------------------------------------------------------------------------------------------------------------------
def test_moments_mean_and_variance_against_exact_rationals():
    col, val, D, N = small_case()
    stats, acc = run_standin(D, [(col, val)], N=N)
    cnt, a, L, s1, s2, I1, I2 = exact_moments(col, val, D)
    assert stats.count.tolist() == cnt and stats.max_abs.tolist() == [np.float32(x) for x in a]
    assert acc.limb_bits.tolist() == L and acc.shift1.tolist() == s1 and acc.shift2.tolist() == s2
    limbs = stats.limbs
    got1 = [int(limbs[j, 0]) * 2 ** L[j] + int(limbs[j, 1]) for j in range(D)]
    got2 = [int(limbs[j, 2]) * 2 ** L[j] + int(limbs[j, 3]) for j in range(D)]
    assert got1 == I1 and got2 == I2
    mean, var = exact_mean_var(N, L, s1, s2, I1, I2)
    worst = max(max(ulps(stats.mean[j], mean[j]), ulps(stats.variance[j], var[j])) for j in range(D))
    print("worst error of mean / variance in ulps:", worst)
    assert worst <= 1.0
    # the constant dense column: exactly zero variance, factor 1; the dead feature and the stored zeros: factor 1
    assert stats.variance[D - 4] == 0.0 and stats.mean[D - 4] == float(np.float32(0.3))
    s = fs.factors(fs.SCALE_WITH_STANDARD_DEVIATION, stats)
    assert s[D - 4] == 1.0 and s[D - 2] == 1.0 and s[D - 1] == 1.0
    assert stats.variance[D - 3] > 0 and s[D - 3] == 1.0 / np.sqrt(stats.variance[D - 3])
    live = [j for j in range(D - 4) if cnt[j] > 0]
    assert np.array_equal(s[live], 1.0 / np.sqrt(stats.variance[live]))
    m = fs.factors(fs.SCALE_WITH_MAX_MAGNITUDE, stats)
    assert np.array_equal(m[live], 1.0 / stats.max_abs[live].astype(np.float64)) and m[D - 2] == 1.0 and m[D - 1] == 1.0
    assert np.array_equal(fs.factors(fs.NONE, stats), np.ones(D))


def test_one_sample_and_negative_values():
    col = np.array([0, 1, 2], np.int64)
    val = np.array([-3.5, 2.0, -1e-3], np.float32)
    stats, _ = run_standin(4, [(col, val)], N=1)
    assert stats.variance.tolist() == [0.0] * 4 and fs.factors(fs.SCALE_WITH_STANDARD_DEVIATION, stats).tolist() == [1.0] * 4
    assert stats.mean[:3].tolist() == val.astype(np.float64).tolist()
    # negative values: the arithmetic shift splits them so that hi 2^L + lo is the term
    col = np.zeros(5, np.int64)
    val = np.array([-1.5, -0.75, 0.5, -1.0e-7, 1.25], np.float32)
    stats, acc = run_standin(1, [(col, val)], N=7)
    cnt, a, L, s1, s2, I1, I2 = exact_moments(col, val, 1)
    assert int(stats.limbs[0, 0]) * 2 ** L[0] + int(stats.limbs[0, 1]) == I1[0] and I1[0] < 0
    mean, var = exact_mean_var(7, L, s1, s2, I1, I2)
    assert ulps(stats.mean[0], mean[0]) <= 1.0 and ulps(stats.variance[0], var[0]) <= 1.0


def test_a_forged_count_of_2_to_the_36_is_exact_and_2_to_the_37_is_refused():
    a = np.array([0.97, 3.0], np.float32)
    L, s1, s2 = fs.shifts(np.array([2 ** 36, 5], np.int64), a)
    assert L.tolist() == [25, 31] and s1.tolist() == [50, 60] and s2.tolist() == [50, 58]
    # with L = 25 the square of the column's largest value is still exact
    x = float(a[0])
    assert Fraction(np.rint(np.ldexp(x * x, int(s2[0])))) == Fraction(x) ** 2 * 2 ** int(s2[0])
    # finish from limbs as large as such a count allows: N = count = 2^36 entries of the value a
    t1 = int(np.rint(np.ldexp(x, int(s1[0]))))
    t2 = int(np.rint(np.ldexp(x * x, int(s2[0]))))
    n = 2 ** 36
    limbs = np.array([[(t1 >> 25) * n, (t1 & (2 ** 25 - 1)) * n, (t2 >> 25) * n, (t2 & (2 ** 25 - 1)) * n], [0, 0, 0, 0]], np.int64)
    mean, var = fs.finish(np.array([n, 5]), a, L, s1, s2, limbs, n)
    assert mean[0] == x and var[0] == 0.0
    with pytest.raises(fs.FeatureStatsError, match=r"feature 0 has 137438953472 stored entries"):
        fs.shifts(np.array([2 ** 37, 5], np.int64), a)


# ---- the stand-in -----------------------------------------------------------------------------------------------------------------------
def test_chunked_and_permuted_equals_a_single_call():
    col, val, D, N = small_case(seed=3)
    whole, _ = run_standin(D, [(col, val)], N=N)
    rng = np.random.default_rng(5)
    perm = rng.permutation(col.size)
    cuts = np.sort(rng.integers(0, col.size, 6))
    cuts[2] = cuts[1]                                                    # one empty chunk
    chunks = [(col[p], val[p]) for p in np.split(perm, cuts)]
    assert len(chunks) == 7 and any(c.size == 0 for c, _ in chunks)
    parts, _ = run_standin(D, chunks, N=N)
    assert np.array_equal(parts.limbs, whole.limbs) and parts.equal_bits(whole)
    # multiplying a column by 8 leaves the integers unchanged and scales sigma by exactly 8
    v8 = val.copy()
    v8[col == 5] *= np.float32(8)
    times8, _ = run_standin(D, [(col, v8)], N=N)
    assert np.array_equal(times8.limbs, whole.limbs)
    assert times8.variance[5] == 64 * whole.variance[5] and times8.mean[5] == 8 * whole.mean[5]
    s, s8 = fs.factors(fs.SCALE_WITH_STANDARD_DEVIATION, whole), fs.factors(fs.SCALE_WITH_STANDARD_DEVIATION, times8)
    assert s8[5] * 8 == s[5]
    x = val[col == 5].astype(np.float64)
    assert np.array_equal((x * s[5]).astype(np.float32), (x * 8 * s8[5]).astype(np.float32))


def test_bad_entries_are_left_out_and_named():
    col, val, D, N = small_case(seed=4, D=20, N=50)
    c2, v2 = col.copy(), val.copy()
    v2[7], v2[11], c2[13], c2[17] = np.nan, np.inf, -1, D
    acc = fs.NumpyAccumulator(D)
    acc.add(c2, v2)
    assert acc.take_bad() == [(4, 7)]
    keep = np.ones(col.size, bool)
    keep[[7, 11, 13, 17]] = False
    ref = fs.NumpyAccumulator(D)
    ref.add(col[keep], val[keep])
    assert np.array_equal(acc.count, ref.count) and np.array_equal(acc.bits, ref.bits)
    with pytest.raises(fs.FeatureStatsError, match=r"pass 1: 4 bad entries in call 0, the first at index 7"):
        run_standin(D, [(c2, v2)], N=N)
    # pass 2: a value above the maximum the shifts were made for
    acc = fs.NumpyAccumulator(D)
    acc.add(col, val)
    acc.shifts()
    big = val.copy()
    j = int(np.flatnonzero(col == 2)[0])
    big[j] = np.float32(4) * np.abs(val[col == 2]).max()
    acc.add(col, big)
    assert acc.take_bad() == [(1, j)]


def test_the_stand_in_equals_the_python_integer_reference_on_the_kernel_cases():
    """The cases of tests/test_gpu_feature_stats.py on the CPU: the reference the kernels are held to is itself held to Fractions (a sample
    of its terms) and to the stand-in (every accumulator)."""
    import feature_stats_helpers as fh
    for make in (fh.case_one_address, fh.case_lds, fh.case_zipf, fh.case_4000):
        col, val, D = make()
        ref = fh.reference(col, val, D)
        fh.check_terms_against_fractions(ref, 500)
        acc = fs.NumpyAccumulator(D)
        acc.add(col, val)
        L, s1, s2 = acc.shifts()
        acc.add(col, val)
        assert acc.take_bad() == [(0, -1)]
        assert np.array_equal(acc.count, ref["count"]) and np.array_equal(acc.bits, ref["bits"])
        assert np.array_equal(L, ref["L"]) and np.array_equal(s1, ref["s1"]) and np.array_equal(s2, ref["s2"])
        assert np.array_equal(acc.limbs, ref["limbs"])
    col, val, D = fh.case_zipf()
    ref = fh.reference(col, val, D)
    dead = float((ref["count"] == 0).mean())
    print(f"zipf case: {dead:.2f} of the features dead, the hottest column holds {int(ref['count'].max())} of {col.size} entries")
    assert 0.25 <= dead <= 0.75 and ref["count"].max() > col.size // 5 and D > 0xffff


# ---- the file ---------------------------------------------------------------------------------------------------------------------------
def test_npz_round_trip_and_num_features_mismatch(tmp_path):
    col, val, D, N = small_case(seed=6)
    stats, _ = run_standin(D, [(col, val)], N=N)
    path = str(tmp_path / "sub" / "stats.npz")
    fs.save(path, stats)
    assert os.listdir(tmp_path / "sub") == ["stats.npz"]                 # written under a temporary name and renamed
    with np.load(path) as z:
        assert sorted(z.files) == sorted(["format_version", "num_features", "num_samples", "count", "max_abs", "mean", "variance"])
        assert int(z["num_features"]) == D and int(z["num_samples"]) == N
    back = fs.load(path, D)
    assert back.equal_bits(stats)
    assert np.array_equal(fs.factors(fs.SCALE_WITH_STANDARD_DEVIATION, back), fs.factors(fs.SCALE_WITH_STANDARD_DEVIATION, stats))
    with pytest.raises(fs.FeatureStatsError, match=rf"num_features {D}, the feature bag has {D + 1}"):
        fs.load(path, D + 1)
    # a file of the one-pass type holds no variances: the other type says so
    one, _ = run_standin(D, [(col, val)], kind=fs.SCALE_WITH_MAX_MAGNITUDE, N=N)
    fs.save(path, one)
    with pytest.raises(fs.FeatureStatsError, match="holds no variances"):
        fs.need_two_passes(fs.SCALE_WITH_STANDARD_DEVIATION, fs.load(path, D))


# ---- refusals -------------------------------------------------------------------------------------------------------------------------------
RE = dict(metadata_file="m", output_model_dir="o")
STD = "scale_with_standard_deviation"


def test_the_default_is_none_and_leaves_argv_as_it_was():
    for cls in (REParams, FixedLRParams):
        p = cls(**RE)
        assert p.normalization() == "none" and "--feature_normalization" not in p.__to_argv__()
        assert cls(**RE, feature_normalization="none").normalization() == "none"
        q = cls.__from_argv__(["--metadata_file=m", "--output_model_dir=o", f"--feature_normalization={STD}", "--feature_statistics_file=s.npz"])
        assert q.normalization() == STD and q.feature_statistics_file == "s.npz"
        assert cls.__from_argv__(q.__to_argv__()) == q


@pytest.mark.parametrize("cls", [REParams, FixedLRParams])
def test_refusals_at_parse_time(cls):
    with pytest.raises(ValueError, match="standardization is not implemented: the mean shift makes the penalty of a regularised intercept non-diagonal"):
        cls(**RE, feature_normalization="standardization")
    with pytest.raises(ValueError, match="--feature_normalization='zscore': one of none, scale_with_standard_deviation, scale_with_max_magnitude"):
        cls(**RE, feature_normalization="zscore")
    with pytest.raises(ValueError, match=f"--feature_normalization={STD} does not run with --incremental_training: prior variances are in the original"):
        cls(**RE, feature_normalization=STD, incremental_training=True)
    with pytest.raises(ValueError, match="--feature_normalization=scale_with_max_magnitude does not run with --l2_reg_weights: a sweep in normalised units"):
        cls(**RE, feature_normalization="scale_with_max_magnitude", l2_reg_weights="1,0.1")
    # none composes with everything
    cls(**RE, feature_normalization="none", incremental_training=True)


def test_rebalance_entities_is_refused():
    with pytest.raises(ValueError, match=f"--feature_normalization={STD} does not run with --rebalance_entities: the factors do not travel"):
        REParams(**RE, feature_normalization=STD, rebalance_entities=True)


def test_several_random_effect_workers_need_an_existing_file(tmp_path):
    class Model:
        pass
    m = Model()
    m.model_params = REParams(**RE, feature_normalization=STD)
    fs.validate(m, {"num_workers": 1})
    with pytest.raises(fs.FeatureStatsError, match="several random-effect workers needs an existing --feature_statistics_file"):
        fs.validate(m, {"num_workers": 2})
    m.model_params = REParams(**RE, feature_normalization=STD, feature_statistics_file=str(tmp_path / "absent.npz"))
    with pytest.raises(fs.FeatureStatsError, match="has no collective"):
        fs.validate(m, {"num_workers": 2})
    col, val, D, N = small_case(seed=8, D=12, N=30)
    stats, _ = run_standin(D, [(col, val)], N=N)
    fs.save(str(tmp_path / "there.npz"), stats)
    m.model_params = REParams(**RE, feature_normalization=STD, feature_statistics_file=str(tmp_path / "there.npz"))
    fs.validate(m, {"num_workers": 2})


# ---- two gloo ranks -------------------------------------------------------------------------------------------------------------------------
def test_two_gloo_ranks_reproduce_one_rank_bit_for_bit(tmp_path):
    root = os.path.dirname(HERE)
    env = dict(os.environ)
    env.pop("TF_CONFIG", None)
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2", "--master-addr", "127.0.0.1",
           "--master-port", "29641", os.path.join(root, "tests", "_feature_stats_dist_worker.py"), str(tmp_path)]
    subprocess.run(cmd, check=True, env=env, timeout=300, cwd=root)
    from _feature_stats_dist_worker import CASE
    col, val, D, N = small_case(**CASE)
    one, _ = run_standin(D, [(col, val)], N=N)
    for rank in (0, 1):
        got = fs.load(str(tmp_path / f"rank{rank}.npz"), D)
        assert got.equal_bits(one)
        assert np.array_equal(np.load(tmp_path / f"limbs{rank}.npy"), one.limbs)
    assert json.load(open(tmp_path / "result.json")) == {"world": 2, "backend": "gloo"}
