"""Host side of the ranking evaluation (include/gdmix_re.h, "ranking evaluation"): the tests' reference against exhaustive enumeration of
tie orders, the host division, the --evaluators flag and its refusals, the ABI. No device."""
import ctypes as C
import math
from fractions import Fraction

import numpy as np
import pytest

from gdmix_amd import constants, evaluate, metrics, params, solver
from gdmix_amd.fe_model import FixedLRParams
from gdmix_amd.params import REParams, Params

import ranking_reference as ref


def test_reference_equals_the_average_over_all_tie_orders():
    """n <= 6, k <= 7, scores rounded to integers (heavy ties): the closed form equals the average over every order inside the tie groups."""
    rng = np.random.default_rng(7)
    tied = 0
    for _ in range(200):
        n = int(rng.integers(0, 7))
        s = np.round(rng.standard_normal(n) * 1.5).astype(np.float32)
        y = (rng.random(n) < 0.5).astype(np.float32)
        for k in range(1, 8):
            c = ref.topk_counts(s, y, k)
            assert ref.precision(s, y, k) == ref.precision_by_enumeration(s, y, k), (s, y, k)
            tied += n > k and c[1] < c[3] and 0 < c[2] < c[3]
    assert tied > 100      # ties that cut a mixed group are common in these cases


def test_reference_with_signed_zeros_infinities_and_nan():
    """-0 ties with +0; infinities order as usual and tie with themselves; a NaN score is no sample."""
    cases = [([0.0, -0.0, 1.0], [1, 0, 0]), ([-0.0, 0.0, -0.0, 0.0], [1, 1, 0, 0]), ([np.inf, np.inf, 1.0, -np.inf], [1, 0, 1, 1]),
             ([-np.inf, -np.inf, -np.inf], [1, 0, 0]), ([np.inf, -np.inf, 0.0, -0.0, np.nan, 2.0], [0, 1, 1, 0, 1, 1]), ([np.nan, np.nan], [1, 0]),
             ([np.inf, np.inf, -0.0, 0.0, -np.inf, -np.inf], [0, 1, 0, 1, 0, 1])]
    for s, y in cases:
        s, y = np.array(s, np.float32), np.array(y, np.float32)
        for k in range(1, 8):
            assert ref.precision(s, y, k) == ref.precision_by_enumeration(s, y, k), (s, y, k)
    assert ref.topk_counts(np.array([0.0, -0.0, 1.0], np.float32), np.array([1, 0, 0], np.float32), 2) == (0, 1, 1, 2)
    assert ref.topk_counts(np.array([np.nan, 3.0], np.float32), np.array([1, 1], np.float32), 1) == (1, 0, 0, 0)      # n = 1 <= k
    assert ref.precision(np.array([1.0], np.float32), np.array([1.0], np.float32), 5) == Fraction(1, 5)              # the denominator is k


def test_precision_from_counts_is_the_correctly_rounded_quotient():
    rng = np.random.default_rng(11)
    cases = [(0, 0, 0, 0, 1), (3, 0, 0, 0, 5), (1, 2, 1, 3, 5), (0, 1, 1, 2, 1),
             # the product slots * tie_pos is above 2^53: no fp64 arithmetic on the way
             (5, (1 << 30) - 7, (1 << 30) + 11, (1 << 31) - 1, 1 << 30), (123456789, 987654321, 1234567891, 1999999999, 1111111110)]
    for _ in range(200):
        ts = int(rng.integers(1, 1 << 31))
        tp = int(rng.integers(0, ts + 1))
        sl = int(rng.integers(1, ts + 1))
        hs = int(rng.integers(0, 1 << 31))
        cases.append((hs, sl, tp, ts, hs + sl + int(rng.integers(0, 3))))
    assert any(c[1] * c[2] > 1 << 53 for c in cases)
    for hs, sl, tp, ts, k in cases:
        want = Fraction(hs) + (Fraction(sl * tp, ts) if ts else 0)
        assert metrics.precision_from_counts(hs, sl, tp, ts, k) == float(want / k), (hs, sl, tp, ts, k)
    with pytest.raises(ValueError):
        metrics.precision_from_counts(0, 0, 0, 0, 0)


def test_ranking_entities_to_host_divides_exact_integers():
    """The vectorised division on what a device call returns (here host tensors) equals precision_from_counts entity by entity;
    an entity with a NaN score reports NaN."""
    ks = (1, 3, 70)
    s = np.array([2, 2, 1, 1, 1, 0, 5, np.nan, 4, 4], np.float32)
    y = np.array([1, 0, 1, 1, 0, 1, 1, 1, 0, 1], np.float32)
    rp = np.array([0, 6, 6, 10], np.int64)
    want = ref.per_entity_counts(rp, s, y, ks)
    res = {k: want[k].astype(np.int32) for k in ("hits_sure", "slots", "tie_pos", "tie_size")}
    res.update(two_u=np.array([9, 0, 3], np.int64), n_pos=np.array([4, 0, 2], np.int32), n_neg=np.array([2, 0, 1], np.int32),
               n_nan=np.array([0, 0, 1], np.int32), sse=np.zeros(3), auc=np.array([0.5625, np.nan, 0.75]))
    import torch
    h = metrics.ranking_entities_to_host({k: torch.from_numpy(v) for k, v in res.items()}, ks)      # (host tensors stand for the device's)
    for j, k in enumerate(ks):
        got = h[metrics.precision_key(k)]
        for e in (0, 1):
            assert got[e] == float(ref.precision(s[rp[e]:rp[e + 1]], y[rp[e]:rp[e + 1]], k))
        assert math.isnan(got[2])
    assert h["n"].tolist() == [6, 0, 4]


RE = ["--metadata_file=m", "--output_model_dir=o", "--feature_bag=b", "--partition_entity=user_id"]
FE = ["--metadata_file=m", "--output_model_dir=o", "--feature_bag=b"]
DIR = ["--metric_output_dir=d"]


def test_evaluators_flag_is_parsed():
    p = REParams.__from_argv__(RE + DIR + ["--evaluators=logistic_loss, AUC:user_id,Precision@5:user_id,PRECISION@1:user_id"])
    spec = p.evaluator_spec()
    assert spec == params.EvaluatorSpec(True, True, (5, 1), "user_id") and spec.ranking
    assert REParams.__from_argv__(RE + DIR + ["--evaluators=LOGISTIC_LOSS"]).evaluator_spec() == params.EvaluatorSpec(True, False, (), "user_id")
    four = REParams.__from_argv__(RE + DIR + ["--evaluators=" + ",".join(f"PRECISION@{k}:user_id" for k in (1, 2, 3, 2**31 - 1))])
    assert four.evaluator_spec().ks == (1, 2, 3, 2**31 - 1)
    fe = FixedLRParams.__from_argv__(FE + DIR + ["--evaluators=Logistic_Loss"])
    assert fe.evaluator_spec() == params.EvaluatorSpec(True, False, (), None) and not fe.evaluator_spec().ranking


@pytest.mark.parametrize("flags,match", [
    (DIR + ["--evaluators=AUC:movie_id"], r"groups by 'movie_id'; this stage's entity is --partition_entity=user_id"),
    (DIR + ["--evaluators=PRECISION@5:queryId"], r"--partition_entity=user_id"),
    (DIR + ["--evaluators=AUC"], r"names no entity"),
    (DIR + ["--evaluators=PRECISION@0:user_id"], r"K is an integer >= 1"),
    (DIR + ["--evaluators=PRECISION@-1:user_id"], r"K is an integer >= 1"),
    (DIR + ["--evaluators=PRECISION@2.5:user_id"], r"K is an integer >= 1"),
    (DIR + ["--evaluators=PRECISION@:user_id"], r"K is an integer >= 1"),
    (DIR + ["--evaluators=PRECISION@five:user_id"], r"K is an integer >= 1"),
    (DIR + ["--evaluators=" + ",".join(f"PRECISION@{k}:user_id" for k in (1, 2, 3, 4, 5))], r"more than 4 distinct K"),
    (DIR + ["--evaluators=AUC:user_id,auc:user_id"], r"listed twice"),
    (DIR + ["--evaluators=PRECISION@5:user_id,precision@05:user_id"], r"listed twice"),
    (DIR + ["--evaluators=LOGISTIC_LOSS,LOGISTIC_LOSS"], r"listed twice"),
    (DIR + ["--evaluators=RMSE"], r"none of LOGISTIC_LOSS, AUC:<id>, PRECISION@K:<id>"),
    (DIR + ["--evaluators=AUC:user_id,"], r"an empty item"),
    (["--evaluators=LOGISTIC_LOSS"], r"--evaluators needs --metric_output_dir"),
    (DIR + ["--evaluators=LOGISTIC_LOSS", "--l2_reg_weights=1,10", "--validation_data_dir=v"], r"does not run with --l2_reg_weights"),
])
def test_evaluators_flag_refusals_of_a_random_effect_stage(flags, match):
    with pytest.raises(ValueError, match=match):
        REParams.__from_argv__(RE + flags)


@pytest.mark.parametrize("flags,match", [
    (DIR + ["--evaluators=AUC:user_id"], r"a fixed effect has no entities"),
    (DIR + ["--evaluators=LOGISTIC_LOSS,PRECISION@5:user_id"], r"a fixed effect has no entities"),
    (["--evaluators=LOGISTIC_LOSS"], r"--evaluators needs --metric_output_dir"),
    (DIR + ["--evaluators=LOGISTIC_LOSS", "--l2_reg_weights=1,10"], r"does not run with --l2_reg_weights"),
])
def test_evaluators_flag_refusals_of_a_fixed_effect_stage(flags, match):
    with pytest.raises(ValueError, match=match):
        FixedLRParams.__from_argv__(FE + flags)


@pytest.mark.parametrize("model_type", [constants.LINEAR_REGRESSION, constants.POISSON_REGRESSION])
def test_evaluators_need_a_logistic_stage(model_type):
    """The model type is the driver's flag, so the refusal comes from the model's constructor — before a solver or a file."""
    from gdmix_amd.model import RandomEffectLRLBFGSModel
    base = Params(uid_column_name="uid", label_column_name="response", stage=constants.RANDOM_EFFECT, model_type=model_type)
    with pytest.raises(ValueError, match=rf"--evaluators needs --model_type=logistic_regression: this stage is a {model_type}"):
        RandomEffectLRLBFGSModel(RE + DIR + ["--evaluators=AUC:user_id"], base_training_params=base)
    with pytest.raises(ValueError, match="--evaluators needs --model_type=logistic_regression"):
        params.check_evaluators_model_type(FixedLRParams.__from_argv__(FE + DIR + ["--evaluators=LOGISTIC_LOSS"]).evaluator_spec(), model_type)
    RandomEffectLRLBFGSModel(RE + DIR, base_training_params=base)      # without the flag the stage is what it was
    logistic = Params(uid_column_name="uid", label_column_name="response", stage=constants.RANDOM_EFFECT)
    assert RandomEffectLRLBFGSModel(RE + DIR + ["--evaluators=AUC:user_id"], base_training_params=logistic).evaluator_spec.auc


def test_parameters_without_the_flag_are_unchanged():
    for cls, argv in ((REParams, RE), (FixedLRParams, FE)):
        p = cls.__from_argv__(argv + DIR)
        assert p.evaluators is None and p.evaluator_spec() is None
        assert "--evaluators" not in p.__to_argv__()
        q = cls.__from_argv__(argv + DIR + ["--evaluators=LOGISTIC_LOSS"])
        a, b = p.__to_argv__(), q.__to_argv__()
        assert [x for x in b if x not in ("--evaluators", "LOGISTIC_LOSS")] == a
    from gdmix_amd import chain
    for stage in ("global", "per_user", "per_movie"):
        assert chain.stage_argv("r", stage, device_metrics=True) == chain.stage_argv("r", stage, device_metrics=True, evaluators=None)
        assert chain.stage_argv("r", stage, evaluators={"per_user": "AUC:user_id"}) == chain.stage_argv("r", stage) + (
            [f"--metric_output_dir={chain.metric_dir('r', stage)}", "--evaluators=AUC:user_id"] if stage == "per_user" else [])


def test_stage_metrics_schema_without_and_with_the_flag():
    sm = metrics.StageMetrics(None, "d", metrics.AUC)
    assert sm.entity_schema is metrics.PER_ENTITY_SCHEMA and sm.spec is None
    sm = metrics.StageMetrics(None, "d", metrics.AUC, params.EvaluatorSpec(False, True, (5, 1), "user_id"))
    assert [f["name"] for f in sm.entity_schema["fields"]] == ["entityId", "n", "n_pos", "auc", "mse", "precision_at_5", "precision_at_1"]
    assert sm.entity_schema["fields"][-1]["type"] == ["null", "double"]
    assert len(metrics.PER_ENTITY_SCHEMA["fields"]) == 5


def test_new_symbols_and_abi_version():
    new = ["gdmix_re_eval_topk_workspace_bytes", "gdmix_re_eval_topk_entities", "gdmix_re_eval_ll_entities", "gdmix_re_eval_ll_acc_reset",
           "gdmix_re_eval_ll_acc_add", "gdmix_re_eval_ll_acc_finish"]
    assert all(n in solver.EXPORTED_SYMBOLS for n in new)
    assert solver.EVAL_LL_STATE_BYTES == solver.EVAL_PL_STATE_BYTES and solver.EVAL_TOPK_MAX == 4
    import os
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "gdmix_re.h")).read()
    assert "#define GDMIX_RE_ABI_VERSION 27" in hdr and "(ABI 27) ranking evaluation" in hdr
    assert f"#define GDMIX_RE_EVAL_LL_TERM_EPS {solver.EVAL_LL_TERM_EPS!r}" in hdr


def test_evaluate_accepts_logistic_loss_and_still_refuses_rmse():
    argv = ["--metricsInputDir", "i", "--outputMetricFile", "o", "--labelColumnName", "response", "--predictionColumnName", "predictionScore"]
    assert evaluate.parse(argv + ["--metricName", "logistic_loss"])["metricName"] == "logistic_loss"
    with pytest.raises(ValueError, match=r"^Do not support metric rmse, currently only support 'auc' and 'mse'\.$"):
        evaluate.parse(argv + ["--metricName", "rmse"])
    for grouped in ("auc:user_id", "precision@5:user_id"):
        with pytest.raises(ValueError, match="Do not support metric"):
            evaluate.parse(argv + ["--metricName", grouped])


@pytest.fixture(scope="module")
def lib():
    from gdmix_amd import build
    build.build_library()
    return solver.load_library()


def test_argument_checks_of_the_new_entry_points(lib):
    """An empty batch (E = 0) returns right behind the argument checks, so no device and no real context is needed: the context is a zeroed
    buffer that is never read (as test_abi.py, test_loss_codes_at_the_entry_points). nk outside 1 .. 4, a NULL ks, a k below 1 and a k
    listed twice are GDMIX_RE_EINVAL; so is a NULL output struct of either family."""
    assert lib.gdmix_re_abi_version() == 27
    ctx = C.create_string_buffer(4096)
    out, auc = solver._EvalTopkOut(), solver._EvalOut()

    def call(ks, nk=None, out_ref=C.byref(out), auc_ref=None):
        arr = None if ks is None else (C.c_int32 * max(len(ks), 1))(*ks)
        return lib.gdmix_re_eval_topk_entities(C.addressof(ctx), None, 0, 0, None, None, arr, len(ks) if nk is None else nk, out_ref, auc_ref, None, 0, None)
    assert call([1, 5, 16, 64]) == 0 and call([2**31 - 1]) == 0 and call([3], auc_ref=C.byref(auc)) == 0
    for bad, nk, msg in (([1], 0, b"nk = 0"), ([1, 2, 3, 4, 5], None, b"nk = 5"), ([1], -1, b"nk = -1"), (None, 1, b"nk = 1"),
                         ([0], None, b"ks[0] = 0"), ([4, -2], None, b"ks[1] = -2"), ([7, 3, 7], None, b"ks[0] = ks[2] = 7")):
        assert call(bad, nk) == -1, (bad, nk)
        assert msg in lib.gdmix_re_last_error(), (bad, nk, lib.gdmix_re_last_error())
    assert call([1], out_ref=None) == -1
    assert lib.gdmix_re_eval_topk_entities(C.addressof(ctx), None, 0, -1, None, None, (C.c_int32 * 1)(1), 1, C.byref(out), None, None, 0, None) == -1
    assert lib.gdmix_re_eval_topk_entities(C.addressof(ctx), None, 0, 1 << 31, None, None, (C.c_int32 * 1)(1), 1, C.byref(out), None, None, 0, None) == -4
    assert lib.gdmix_re_eval_topk_workspace_bytes(10, 1 << 31) == 0
    assert lib.gdmix_re_eval_topk_workspace_bytes(10, 1000) == lib.gdmix_re_eval_workspace_bytes(10, 1000) > 0
    pl = solver._EvalPlOut()
    assert lib.gdmix_re_eval_ll_entities(C.addressof(ctx), None, 0, 0, None, None, C.byref(pl), None) == 0
    assert lib.gdmix_re_eval_ll_entities(C.addressof(ctx), None, 0, 0, None, None, None, None) == -1
    assert b"gdmix_re_eval_ll_entities" in lib.gdmix_re_last_error()
    assert lib.gdmix_re_eval_ll_entities(C.addressof(ctx), None, 1 << 31, 0, None, None, C.byref(pl), None) == -4
    acc = solver._EvalPlAcc(None, 0)
    tot = solver._EvalPlTotals()
    assert lib.gdmix_re_eval_ll_acc_reset(C.addressof(ctx), C.byref(acc), None) == -1 and b"gdmix_re_eval_ll_acc_reset" in lib.gdmix_re_last_error()
    assert lib.gdmix_re_eval_ll_acc_add(C.addressof(ctx), C.byref(acc), None, None, 0, None) == -1
    assert lib.gdmix_re_eval_ll_acc_finish(C.addressof(ctx), C.byref(acc), C.byref(tot), None) == -1
    assert lib.gdmix_re_eval_pl_acc_reset(C.addressof(ctx), C.byref(acc), None) == -1 and b"gdmix_re_eval_pl_acc_reset" in lib.gdmix_re_last_error()
