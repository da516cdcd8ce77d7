"""Host side of AUPR (include/gdmix_re.h, "AUPR"): the reference by hand, the --evaluators items, the ABI and argument checks. No device."""
import ctypes as C
import math
from fractions import Fraction as Fr

import numpy as np
import pytest

from gdmix_amd import evaluate, metrics, params, solver
from gdmix_amd.fe_model import FixedLRParams
from gdmix_amd.params import EvaluatorSpec, REParams

import aupr_reference as ref

RE = ["--metadata_file=m", "--output_model_dir=o", "--feature_bag=b", "--partition_entity=user_id", "--metric_output_dir=d"]
FE = ["--metadata_file=m", "--output_model_dir=o", "--feature_bag=b", "--metric_output_dir=d"]


@pytest.mark.parametrize("score,label,want", [
    ([0.5, 0.5, 0.5, 0.5], [1, 0, 0, 1], (Fr(2, 4) * 2, 2, 2, 0)),      # one tie group: AUPR = n_pos / n
    ([3, 2, 1, 0], [1, 1, 0, 0], (Fr(2), 2, 2, 0)),                     # a perfect ranking: AUPR = 1
    # [1, 0, 1] by descending score: the curve's points are (0, 1), (1/2, 1), (1/2, 1/2), (1, 2/3). The negative's threshold is a point
    # of its own, so the last trapezoid runs from precision 1/2, not from 1: AUPR = (1 + 1/2 (1/2 + 2/3)) / 2
    ([1, 2, 3], [1, 0, 1], (1 + Fr(1, 2) * (Fr(1, 2) + Fr(2, 3)), 2, 1, 0)),
])
def test_reference_on_hand_computed_cases(score, label, want):
    assert ref.pr_sum_exact(np.array(score, np.float32), np.array(label, np.float32)) == want


def test_the_two_items_are_parsed_and_older_specs_compare_equal():
    spec = REParams.__from_argv__(RE + ["--evaluators=aupr, AUPR:user_id"]).evaluator_spec()
    assert spec == EvaluatorSpec(False, False, (), "user_id", True, True) and not spec.ranking
    both = REParams.__from_argv__(RE + ["--evaluators=AUC:user_id,AUPR:user_id,PRECISION@5:user_id"]).evaluator_spec()
    assert both == EvaluatorSpec(False, True, (5,), "user_id", aupr_entity=True)
    assert REParams.__from_argv__(RE + ["--evaluators=LOGISTIC_LOSS,AUC:user_id"]).evaluator_spec() == EvaluatorSpec(True, True, (), "user_id")      # four fields
    fe = FixedLRParams.__from_argv__(FE + ["--evaluators=LOGISTIC_LOSS,AUPR"]).evaluator_spec()
    assert fe == EvaluatorSpec(True, False, (), None, True)
    sm = metrics.StageMetrics(None, "d", metrics.AUC, spec)
    assert [f["name"] for f in sm.entity_schema["fields"]] == ["entityId", "n", "n_pos", "auc", "mse", "aupr"]
    assert metrics.StageMetrics(None, "d", metrics.AUC, fe).entity_schema is metrics.PER_ENTITY_SCHEMA
    with pytest.raises(ValueError, match="--evaluators needs --model_type=logistic_regression"):
        params.check_evaluators_model_type(spec, "linear_regression")
    assert metrics.aupr_from_sum(1.75, 2) == 0.875 and metrics.aupr_from_sum(1.0, 3) == 1.0 / 3.0 and math.isnan(metrics.aupr_from_sum(0.0, 0))
    argv = ["--metricsInputDir", "i", "--outputMetricFile", "o", "--labelColumnName", "response", "--predictionColumnName", "predictionScore"]
    assert evaluate.parse(argv + ["--metricName", "aupr"])["metricName"] == "aupr"
    with pytest.raises(ValueError, match=r"^Do not support metric rmse, currently only support 'auc' and 'mse'\.$"):
        evaluate.parse(argv + ["--metricName", "rmse"])


@pytest.mark.parametrize("cls,flags,match", [
    (REParams, RE + ["--evaluators=AUPR,aupr"], r"listed twice"),
    (REParams, RE + ["--evaluators=AUPR:user_id,AUPR,Aupr:user_id"], r"listed twice"),
    (REParams, RE + ["--evaluators=AUPR:movie_id"], r"groups by 'movie_id'; this stage's entity is --partition_entity=user_id"),
    (REParams, RE + ["--evaluators=RMSE"], r"none of LOGISTIC_LOSS, AUC:<id>, PRECISION@K:<id>, AUPR, AUPR:<id>"),
    (REParams, RE[:-1] + ["--evaluators=AUPR"], r"--evaluators needs --metric_output_dir"),
    (REParams, RE + ["--evaluators=AUPR", "--l2_reg_weights=1,10", "--validation_data_dir=v"], r"does not run with --l2_reg_weights"),
    (FixedLRParams, FE + ["--evaluators=AUPR:user_id"], r"a fixed effect has no entities"),
])
def test_refusals(cls, flags, match):
    with pytest.raises(ValueError, match=match):
        cls.__from_argv__(flags)


def test_new_symbols_abi_version_and_argument_checks():
    """An empty batch returns right behind the argument checks, so the context is a zeroed buffer that is never read."""
    assert all("gdmix_re_eval_aupr_" + n in solver.EXPORTED_SYMBOLS for n in ("workspace_bytes", "entities", "acc_workspace_bytes", "acc_finish"))
    from gdmix_amd import build
    build.build_library()
    zeroed = C.create_string_buffer(4096)
    lib, ctx = solver.load_library(), C.addressof(zeroed)
    out, tot, acc = solver._EvalAuprOut(), solver._EvalAuprTotals(1.0, 1, 1, 1, 1), solver._EvalAcc(None, 0, 0, None)
    entities = lambda E, N, o: lib.gdmix_re_eval_aupr_entities(ctx, None, E, N, None, None, o, None, 0, None)
    finish = lambda a, t: lib.gdmix_re_eval_aupr_acc_finish(ctx, a, None, 0, t, None)
    assert lib.gdmix_re_abi_version() == 27 and entities(0, 0, C.byref(out)) == 0 and entities(0, 0, None) == -1 and b"gdmix_re_eval_aupr_entities" in lib.gdmix_re_last_error()
    assert entities(0, -1, C.byref(out)) == -1 and entities(0, 1 << 31, C.byref(out)) == -4 and entities(1 << 31, 0, C.byref(out)) == -4
    assert lib.gdmix_re_eval_aupr_workspace_bytes(10, 1 << 31) == 0 and lib.gdmix_re_eval_aupr_acc_workspace_bytes(1 << 31) == 0
    assert lib.gdmix_re_eval_aupr_acc_workspace_bytes(1000) >= lib.gdmix_re_eval_acc_workspace_bytes(1000) + 8 * 1000
    assert finish(C.byref(acc), C.byref(tot)) == 0 and (tot.pr_sum, tot.n, tot.n_pos, tot.n_neg, tot.n_nan) == (0.0, 0, 0, 0, 0)      # empty: zeros
    assert finish(C.byref(acc), None) == -1 and b"gdmix_re_eval_aupr_acc_finish" in lib.gdmix_re_last_error() and finish(None, C.byref(tot)) == -1
    acc.count = 5                                                                                       # keys without a workspace
    assert finish(C.byref(acc), C.byref(tot)) == -3
