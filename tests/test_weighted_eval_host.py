"""Host side of the weighted evaluation (include/gdmix_re.h, "weighted evaluation"): the --evaluators items, the ABI, the argument checks on
an empty batch and the division. No device."""
import ctypes as C
import math
import os
import re

import pytest

from gdmix_amd import build, metrics, solver
from gdmix_amd.fe_model import FixedLRParams
from gdmix_amd.params import EvaluatorSpec, REParams

RE = ["--metadata_file=m", "--output_model_dir=o", "--feature_bag=b", "--partition_entity=user_id", "--metric_output_dir=d"]
FE = ["--metadata_file=m", "--output_model_dir=o", "--feature_bag=b", "--metric_output_dir=d"]
NAMES = ["gdmix_re_eval_w_" + n for n in ("workspace_bytes", "entities", "acc_add", "acc_workspace_bytes", "acc_finish")] + \
        ["gdmix_re_eval_wll_" + n for n in ("entities", "acc_reset", "acc_add", "acc_finish")]


def test_the_three_items_are_parsed_in_any_case_on_both_stages():
    spec = REParams.__from_argv__(RE + ["--evaluators=weighted_auc, WEIGHTED_AUC:user_id,Weighted_Logistic_Loss"]).evaluator_spec()
    assert spec == EvaluatorSpec(entity="user_id", weighted_auc=True, weighted_auc_entity=True, weighted_log_loss=True) and not spec.ranking
    fe = FixedLRParams.__from_argv__(FE + ["--evaluators=WEIGHTED_AUC,WEIGHTED_LOGISTIC_LOSS"]).evaluator_spec()
    assert fe == EvaluatorSpec(weighted_auc=True, weighted_log_loss=True)
    sm = metrics.StageMetrics(None, "d", metrics.AUC, spec)
    assert [f["name"] for f in sm.entity_schema["fields"]] == ["entityId", "n", "n_pos", "auc", "mse", "weighted_auc"]
    assert metrics.StageMetrics(None, "d", metrics.AUC, fe).entity_schema is metrics.PER_ENTITY_SCHEMA


@pytest.mark.parametrize("cls,flags,match", [
    (REParams, RE + ["--evaluators=WEIGHTED_AUC:movie_id"], r"groups by 'movie_id'; this stage's entity is --partition_entity=user_id"),
    (FixedLRParams, FE + ["--evaluators=WEIGHTED_AUC:user_id"], r"a fixed effect has no entities"),
    (REParams, RE + ["--evaluators=WEIGHTED_AUC,weighted_auc"], r"listed twice"),
    (REParams, RE + ["--evaluators=WEIGHTED_AUC:user_id,WEIGHTED_AUC,weighted_auc:user_id"], r"listed twice"),
    (REParams, RE + ["--evaluators=WEIGHTED_LOGISTIC_LOSS:user_id"], r"names no entity"),
])
def test_refusals(cls, flags, match):
    with pytest.raises(ValueError, match=match):
        cls.__from_argv__(flags)


def test_symbols_are_declared_and_exported_and_an_empty_batch_is_checked_without_a_device():
    """An empty batch returns right behind the argument checks, so the context is a zeroed buffer that is never read."""
    with open(os.path.join(os.path.dirname(build.CSRC), os.pardir, "include", "gdmix_re.h")) as f:
        declared = set(re.findall(r"GDMIX_API\s+[\w\s\*]+?\b(gdmix_\w+)\s*\(", f.read()))
    assert all(n in declared and n in solver.EXPORTED_SYMBOLS for n in NAMES)
    build.build_library()
    zeroed = C.create_string_buffer(4096)
    lib, ctx = solver.load_library(), C.addressof(zeroed)
    assert all(hasattr(lib, n) for n in NAMES) and lib.gdmix_re_abi_version() == 27
    out = solver._EvalWOut()
    entities = lambda E, N, o: lib.gdmix_re_eval_w_entities(ctx, None, E, N, None, None, None, o, None, 0, None)
    assert entities(0, 0, C.byref(out)) == 0 and entities(0, 0, None) == -1 and b"gdmix_re_eval_w_entities" in lib.gdmix_re_last_error()
    assert entities(0, 1 << 31, C.byref(out)) == -4 and lib.gdmix_re_eval_w_workspace_bytes(10, 1 << 31) == 0
    assert lib.gdmix_re_eval_wll_entities(ctx, None, 0, 0, None, None, None, None, None) == -1 and b"gdmix_re_eval_wll_entities" in lib.gdmix_re_last_error()
    tot, acc = solver._EvalWTotals(1.0, 1.0, 1.0, 1, 1, 1), solver._EvalAcc(None, 0, 0, None)
    assert lib.gdmix_re_eval_w_acc_finish(ctx, C.byref(acc), None, 0, C.byref(tot), None) == 0      # empty: zeros, no workspace
    assert (tot.two_u_w, tot.w_pos, tot.w_neg, tot.n, tot.n_nan, tot.n_bad_weight) == (0.0, 0.0, 0.0, 0, 0, 0)
    assert lib.gdmix_re_eval_w_acc_workspace_bytes(1000) >= 16 * 1000 and solver.EVAL_W_SCAN_TILE == 4096


def test_weighted_auc_from_sums():
    assert metrics.weighted_auc_from_sums(3.0, 1.0, 2.0) == 0.75 and metrics.weighted_auc_from_sums(0.375, 0.5, 0.75) == 0.5
    assert math.isnan(metrics.weighted_auc_from_sums(0.0, 0.0, 2.0)) and math.isnan(metrics.weighted_auc_from_sums(0.0, 2.0, 0.0))
