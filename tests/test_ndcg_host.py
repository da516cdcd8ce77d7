"""Host side of NDCG@K (include/gdmix_re.h, "NDCG"): the --evaluators item, the model types it runs with, the ABI and the division.
No device."""
import ctypes as C
import math
import os
import re

import pytest

from gdmix_amd import build, metrics, solver
from gdmix_amd.fe_model import FixedLRParams
from gdmix_amd.params import EvaluatorSpec, REParams, check_evaluators_model_type

RE = ["--metadata_file=m", "--output_model_dir=o", "--feature_bag=b", "--partition_entity=user_id", "--metric_output_dir=d"]
FE = ["--metadata_file=m", "--output_model_dir=o", "--feature_bag=b", "--metric_output_dir=d"]
MODEL_TYPES = ("logistic_regression", "linear_regression", "poisson_regression")
NAMES = ["gdmix_re_eval_ndcg_workspace_bytes", "gdmix_re_eval_ndcg_entities"]


def test_the_item_is_parsed_in_any_case_and_the_spec_keeps_its_old_shape():
    spec = REParams.__from_argv__(RE + ["--evaluators=ndcg@3:user_id, NDCG@10:user_id,Ndcg@2147483647:user_id"]).evaluator_spec()
    assert spec == EvaluatorSpec(entity="user_id", ndcg_ks=(3, 10, 2**31 - 1)) and spec.ndcg_only and not spec.ranking
    mixed = REParams.__from_argv__(RE + ["--evaluators=PRECISION@1:user_id,PRECISION@2:user_id,PRECISION@3:user_id,PRECISION@4:user_id,"
                                         "NDCG@1:user_id,NDCG@2:user_id,NDCG@3:user_id,NDCG@4:user_id,AUC:user_id"]).evaluator_spec()      # four K of each
    assert mixed == EvaluatorSpec(False, True, (1, 2, 3, 4), "user_id", False, False, False, False, False, (1, 2, 3, 4)) and not mixed.ndcg_only
    assert EvaluatorSpec() == EvaluatorSpec(False, False, (), None, False, False, False, False, False) and EvaluatorSpec().ndcg_ks == ()
    assert [f["name"] for f in metrics.StageMetrics(None, "d", metrics.MSE, spec).entity_schema["fields"]] == \
        ["entityId", "n", "n_pos", "auc", "mse", "ndcg_at_3", "ndcg_at_10", "ndcg_at_2147483647"]
    assert [f["name"] for f in metrics.StageMetrics(None, "d", metrics.POISSON_LOSS, spec).entity_schema["fields"]] == \
        ["entityId", "n", "poisson_loss", "ndcg_at_3", "ndcg_at_10", "ndcg_at_2147483647"]


@pytest.mark.parametrize("cls,flags,match", [
    (REParams, RE + ["--evaluators=NDCG@0:user_id"], r"K is an integer >= 1"),
    (REParams, RE + ["--evaluators=NDCG@-1:user_id"], r"K is an integer >= 1"),
    (REParams, RE + ["--evaluators=NDCG@1.5:user_id"], r"K is an integer >= 1"),
    (REParams, RE + ["--evaluators=NDCG@:user_id"], r"K is an integer >= 1"),
    (REParams, RE + ["--evaluators=NDCG@2147483648:user_id"], r"K is below 2\^31"),
    (REParams, RE + ["--evaluators=NDCG@3:user_id,ndcg@3:user_id"], r"listed twice"),
    (REParams, RE + ["--evaluators=" + ",".join(f"NDCG@{k}:user_id" for k in range(1, 6))], r"more than 4 distinct K"),
    (REParams, RE + ["--evaluators=NDCG@3"], r"names no entity"),
    (REParams, RE + ["--evaluators=NDCG@3:movie_id"], r"groups by 'movie_id'; this stage's entity is --partition_entity=user_id"),
    (REParams, RE + ["--evaluators=NDCG:user_id"], r"is none of LOGISTIC_LOSS, AUC:<id>.*NDCG@K:<id>$"),
    (FixedLRParams, FE + ["--evaluators=NDCG@3:user_id"], r"a fixed effect has no entities"),
])
def test_refusals(cls, flags, match):
    with pytest.raises(ValueError, match=match):
        cls.__from_argv__(flags)


@pytest.mark.parametrize("model_type", MODEL_TYPES)
def test_ndcg_alone_runs_with_every_model_type_and_any_other_item_needs_a_logistic_stage(model_type):
    check_evaluators_model_type(EvaluatorSpec(entity="user_id", ndcg_ks=(3,)), model_type)
    assert REParams.__from_argv__(RE + ["--evaluators=NDCG@3:user_id", f"--model_type={model_type}"]).evaluator_spec().ndcg_ks == (3,)
    beside = EvaluatorSpec(auc=True, entity="user_id", ndcg_ks=(3,))
    if model_type == "logistic_regression":
        check_evaluators_model_type(beside, model_type)
    else:
        with pytest.raises(ValueError, match=rf"^--evaluators needs --model_type=logistic_regression: this stage is a {model_type}$"):
            check_evaluators_model_type(beside, model_type)


def test_symbols_are_declared_and_exported_and_the_ks_are_checked_without_a_device():
    """The argument checks, an empty batch included, return before the context is read: it is a zeroed buffer."""
    with open(os.path.join(os.path.dirname(build.CSRC), os.pardir, "include", "gdmix_re.h")) as f:
        header = f.read()
    declared = set(re.findall(r"GDMIX_API\s+[\w\s\*]+?\b(gdmix_\w+)\s*\(", header))
    assert all(n in declared and n in solver.EXPORTED_SYMBOLS for n in NAMES)
    assert float(re.search(r"#define GDMIX_RE_EVAL_NDCG_BOUND (\S+)", header).group(1)) == solver.EVAL_NDCG_BOUND <= 1e-12
    build.build_library()
    zeroed = C.create_string_buffer(4096)
    lib, ctx, out = solver.load_library(), C.addressof(zeroed), solver._EvalNdcgOut()
    assert all(hasattr(lib, n) for n in NAMES) and lib.gdmix_re_abi_version() == 27
    call = lambda ks, nk, N=0, o=C.byref(out): lib.gdmix_re_eval_ndcg_entities(ctx, None, 0, N, None, None, (C.c_int32 * len(ks))(*ks), nk, o, None, 0, None)
    assert call([1, 3], 2) == 0 and call([1], 1, o=None) == -1 and b"gdmix_re_eval_ndcg_entities" in lib.gdmix_re_last_error()
    assert call([1], 0) == -1 and call([1, 2, 3, 4, 5], 5) == -1 and call([2, 2], 2) == -1 and call([0], 1) == -1 and call([-3], 1) == -1
    assert call([1], 1, N=1 << 31) == -4 and lib.gdmix_re_eval_ndcg_workspace_bytes(10, 1 << 31) == 0
    assert lib.gdmix_re_eval_ndcg_workspace_bytes(10, 1000) >= 72 * 1000 and solver.EVAL_NDCG_SCAN_TILE == 4096


def test_ndcg_from_sums():
    assert metrics.ndcg_from_sums(1.5, 3.0) == 0.5 and metrics.ndcg_from_sums(0.0, 2.0) == 0.0 and metrics.ndcg_from_sums(7.0, 7.0) == 1.0
    for null in (metrics.ndcg_from_sums(0.0, 0.0), metrics.ndcg_from_sums(1.0, 2.0, n_nan=1), metrics.ndcg_from_sums(1.0, 2.0, n_bad_label=2)):
        assert math.isnan(null)
    assert metrics.ndcg_key(10) == "ndcg_at_10"
