"""Incremental training on the host (include/gdmix_re.h, "incremental training"): the flag and its refusals, the mapping of a prior
model's means and variances into a batch with the defaults, the carry-over of prior features an entity's new data lacks, and — by the
CPU oracle alone — that solving the transformed batch and mapping back minimises the exact objective F. No GPU."""
import types

import numpy as np
import pytest

import prior_helpers as ph
from gdmix_amd import model as M
from gdmix_amd import synthetic
from gdmix_amd.io import native_reader
from gdmix_amd.model import ModelTable, RandomEffectLRLBFGSModel
from gdmix_amd.params import REParams
from oracle import oracle

BASE = ["--metadata_file", "meta.json", "--output_model_dir", "models", "--feature_bag", "bag", "--feature_file", "features.csv",
        "--partition_entity", "ent", "--regularize_bias", "False"]


# ---- 1. parsing --------------------------------------------------------------------------------------------------------------------
def test_the_flag_parses_and_defaults_to_off():
    assert REParams.__from_argv__(BASE).incremental_training is False
    assert REParams.__from_argv__(BASE + ["--incremental_training", "True"]).incremental_training is True
    assert REParams.__from_argv__(BASE + ["--incremental_training=False"]).incremental_training is False


@pytest.mark.parametrize("extra,other", [(["--l2_reg_weights", "1,10"], "--l2_reg_weights"), (["--rebalance_entities", "True"], "--rebalance_entities")])
def test_refused_at_parse_time_with_an_error_naming_both_flags(extra, other):
    with pytest.raises(ValueError) as err:
        REParams.__from_argv__(BASE + ["--incremental_training", "True"] + extra)
    assert "--incremental_training" in str(err.value) and other in str(err.value)
    REParams.__from_argv__(BASE + extra)        # each of them alone is accepted as before


def test_inference_is_refused_before_anything_is_read(tmp_path):
    m = RandomEffectLRLBFGSModel(BASE + ["--incremental_training", "True"])
    with pytest.raises(ValueError) as err:
        m.predict(str(tmp_path / "out"), str(tmp_path / "nothing"), str(tmp_path / "no_meta.json"), str(tmp_path), {"partition_index": 0}, None)
    assert "--incremental_training" in str(err.value) and "--action inference" in str(err.value)


# ---- 2. mapping --------------------------------------------------------------------------------------------------------------------
def _hand_table():
    """Prior models, has_intercept: "a" with variances (feature 7 with variance 0, feature 9 with nan, feature 4 absent from the data),
    "b" in a chunk without variances; "c" has none. Coefficients intercept first."""
    t = ModelTable()
    t.add_chunk(["a"], [0.5, 1.0, -2.0, 3.0, 0.25], [0, 5], [2, 4, 7, 9], [0, 4], variance=[0.04, 0.09, 0.16, 0.0, np.nan])
    t.add_chunk(["b"], [-0.3, 0.7], [0, 2], [3], [0, 1])
    plain = {"a": (np.array([0.5, 1.0, -2.0, 3.0, 0.25]), np.array([0.04, 0.09, 0.16, 0.0, np.nan]), np.array([2, 4, 7, 9])),
             "b": (np.array([-0.3, 0.7]), None, np.array([3]))}
    return t, plain


# the batch: "a" sees features 2, 5 (new for it), 7, 9; "c" (new) sees 1; "b" sees 3, 8
IDS = ["a", "c", "b"]
UNIQ = np.array([2, 5, 7, 9, 1, 3, 8], np.int64)
FEAT_PTR = np.array([0, 4, 5, 7], np.int64)
WANT_MEAN = np.array([0.5, 1.0, 0.0, 3.0, 0.25, 0.0, 0.0, -0.3, 0.7, 0.0])
WANT_VAR = np.array([0.04, 0.09, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0])


@pytest.mark.parametrize("native", [False, True])
def test_mapping_of_means_and_variances_with_the_defaults(native):
    if native and not native_reader.available():
        from gdmix_amd import build
        build.build_io_library()
    table, plain = _hand_table()
    mean, var = M.prior_for_batch(table, IDS, UNIQ, FEAT_PTR, True, 16, native=native)
    assert np.array_equal(mean, WANT_MEAN) and np.array_equal(var, WANT_VAR)
    pm, pv = ph.map_prior_plain(plain, IDS, UNIQ, FEAT_PTR, True)
    assert np.array_equal(pm, WANT_MEAN) and np.array_equal(pv, WANT_VAR)
    # the scale: sqrt, and 1 at every intercept (the intercept column cannot be scaled)
    scale = M.prior_scale(var, FEAT_PTR, True)
    want = np.sqrt(WANT_VAR)
    want[[0, 5, 7]] = 1.0
    assert np.array_equal(scale, want)
    assert np.array_equal(M.prior_scale(var, FEAT_PTR + np.arange(4), False), np.sqrt(WANT_VAR))


def test_mapping_without_a_prior_is_todays_objective():
    mean, var = M.prior_for_batch(ModelTable(), IDS, UNIQ, FEAT_PTR, True, 16)
    assert not mean.any() and np.array_equal(var, np.ones(10))


# ---- 3. carry-over -----------------------------------------------------------------------------------------------------------------
def _train_with(flag, tmp_path):
    """RandomEffectLRLBFGSModel._train on the hand-built prior with the read, the solve and the file writer replaced: what comes out is
    the merged table."""
    argv = BASE + ["--random_effect_variance_mode", "simple"] + (["--incremental_training", "True"] if flag else [])
    m = RandomEffectLRLBFGSModel(argv)
    table, _ = _hand_table()
    table.add_chunk(["gone"], [0.1, 0.2], [0, 2], [6], [0, 1], variance=[0.5, 0.6])     # an entity absent from the new data
    batch = types.SimpleNamespace(E=3, N=3, Z=7, entity_ids=IDS, has_label=True)
    theta = np.arange(1.0, 11.0)
    variance = np.arange(1.0, 11.0) / 100.0
    m._read = lambda *a, **k: batch
    m._read_key = lambda *a, **k: "key"
    m._solve_batch = lambda b, mw, nf: (theta, variance, UNIQ, FEAT_PTR, {}, None)
    m._write_behind = lambda *a, **k: None
    return m._train("in", None, table, 16, None, str(tmp_path / "model.avro")), theta, variance


def test_a_prior_feature_absent_from_the_new_data_keeps_its_mean_and_variance(tmp_path):
    out, theta, variance = _train_with(True, tmp_path)
    a = out.get("a")
    assert a.unique_global_indices.tolist() == [2, 4, 5, 7, 9]          # feature 4 is back, ascending
    assert a.theta.tolist() == [1.0, 2.0, -2.0, 3.0, 4.0, 5.0]          # intercept, f2, the carried f4 = -2.0, f5, f7, f9
    assert a.variance.tolist() == [0.01, 0.02, 0.16, 0.03, 0.04, 0.05]  # f4 keeps its prior variance
    c, b = out.get("c"), out.get("b")
    assert c.unique_global_indices.tolist() == [1] and c.theta.tolist() == [6.0, 7.0]
    assert b.unique_global_indices.tolist() == [3, 8] and b.theta.tolist() == [8.0, 9.0, 10.0]
    gone = out.get("gone")                                               # carried over whole, as today
    assert gone.theta.tolist() == [0.1, 0.2] and gone.variance.tolist() == [0.5, 0.6] and gone.unique_global_indices.tolist() == [6]
    assert list(out.keys()) == ["a", "b", "gone", "c"]


def test_without_the_flag_the_table_is_what_it_is_today(tmp_path):
    out, theta, variance = _train_with(False, tmp_path)
    a = out.get("a")
    assert a.unique_global_indices.tolist() == [2, 5, 7, 9] and a.theta.tolist() == [1.0, 2.0, 3.0, 4.0, 5.0]     # feature 4 is dropped
    assert out.get("gone").theta.tolist() == [0.1, 0.2]
    assert list(out.keys()) == ["a", "b", "gone", "c"]


def test_a_carried_feature_without_a_usable_variance_gets_the_default():
    t = ModelTable()
    t.add_chunk(["b"], [-0.3, 0.7, 0.9], [0, 3], [3, 11], [0, 2])        # no variances in the prior
    th, va, uq, fp = M.carry_over_prior_features(t, ["b"], np.array([1.0, 2.0]), np.array([0.1, 0.2]), np.array([3]), np.array([0, 1]), True)
    assert uq.tolist() == [3, 11] and fp.tolist() == [0, 2] and th.tolist() == [1.0, 2.0, 0.9] and va.tolist() == [0.1, 0.2, 1.0]


# ---- 4. the substitution is right, by the oracle alone -----------------------------------------------------------------------------
# Measured on the CPU over the eight cases below (40 ragged entities, seed 31): the largest |s (.) grad F|_inf of the EXACT objective at
# the restored solution of the transformed (fp32-rounded) problem is 2.55e-7 — the floor the rounding of the data sets, about 1e-7 |x| —
# and the largest distance to the closed-form ridge minimiser, in phi units |theta - theta*| / s, is 3.07e-6 (l2 = 0.1: the rounding of
# the data divided by the smallest curvature). The bounds are 4 x those.
GRAD_BOUND = 4 * 2.55e-7
RIDGE_BOUND = 4 * 3.07e-6


@pytest.fixture(scope="module")
def ragged():
    b = synthetic.make_ragged_batch(40, seed=31, D=30, max_n=40, max_k=9)
    return b, synthetic.with_real_labels(b, 31), oracle.pack(b.ent_row_ptr, b.row_nnz_ptr, b.col_global)


@pytest.mark.parametrize("regularize_bias", [True, False])
@pytest.mark.parametrize("l2", [0.1, 10.0])
@pytest.mark.parametrize("linear", [False, True])
def test_solving_the_transformed_batch_minimises_the_exact_objective(ragged, linear, l2, regularize_bias):
    b = ragged[1] if linear else ragged[0]
    pk = ragged[2]
    kw = dict(l2=l2, has_intercept=True, regularize_bias=regularize_bias)
    cp = ph.coef_ptr(pk, True)
    mean, var, scale = ph.draw_prior(int(cp[-1]), 5, cp, has_intercept=True)
    val2, off2 = ph.transform_raw(b, pk, mean, scale, True)
    o = oracle.make_opts(pgtol=1e-10, ftol=1e-16, max_iter=1000, linear=linear, **kw)
    res = oracle.solve(pk, val2, b.y, off2, b.weight, o)
    theta, _, _ = ph.restore(mean, scale, res["theta"])
    g = ph.scaled_gradient_norms(b, pk, theta, mean, var, scale, kw, linear)
    print(f"linear={linear} l2={l2} regularize_bias={regularize_bias}: max |s grad F| = {g.max():.3e}")
    assert g.max() <= GRAD_BOUND
    # the substitution matters: the same solve WITHOUT it (today's warm start from the prior) is not at the minimum of F
    plain = oracle.solve(pk, b.val, b.y, b.offset, b.weight, o, theta0=mean)
    assert ph.scaled_gradient_norms(b, pk, plain["theta"], mean, var, scale, kw, linear).max() > 1e3 * GRAD_BOUND
    if linear:
        worst = 0.0
        for e in range(b.E):
            a, c = int(cp[e]), int(cp[e + 1])
            star = ph.ridge_with_prior(b, pk, e, mean[a:c], var[a:c], l2, True, regularize_bias)
            worst = max(worst, float(np.max(np.abs(theta[a:c] - star) / scale[a:c])))
        print(f"    distance to the closed-form minimiser, phi units: {worst:.3e}")
        assert worst <= RIDGE_BOUND
