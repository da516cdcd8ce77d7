"""--l2_reg_weights on the host (gdmix_amd/sweep.py, params.py, driver.py): the flag, the selection rule, the files, the numpy statement
of the join against the model table's own coefficient mapping, and everything the sweep refuses — none of which needs a device."""
import json
import math
import os

import numpy as np
import pytest

from gdmix_amd import sweep
from gdmix_amd.driver import RandomEffectDriver
from gdmix_amd.model import ModelTable, RandomEffectLRLBFGSModel, _model_coefficients_for_batch
from gdmix_amd.params import Params, REParams, SchemaParams, parse_l2_grid

BASE = ["--metadata_file=m.json", "--output_model_dir=out"]


# ---- the flag ----------------------------------------------------------------------------------------------------------------------
def test_flag_parses_both_spellings_and_round_trips():
    p = REParams.__from_argv__(BASE + ["--l2_reg_weights=10,1,0.1"])
    assert p.l2_grid() == (10.0, 1.0, 0.1)
    q = REParams.__from_argv__(BASE + ["--l2_reg_weights", "3"])
    assert q.l2_grid() == (3.0,)                                 # K = 1 is legal
    again = REParams.__from_argv__(p.__to_argv__())
    assert again == p and again.l2_grid() == (10.0, 1.0, 0.1)
    assert parse_l2_grid(" 100, 10 ,0") == (100.0, 10.0, 0.0)


def test_without_the_flag_the_parameters_are_todays():
    p = REParams.__from_argv__(BASE)
    assert p.l2_reg_weights is None and p.l2_grid() is None
    assert "--l2_reg_weights" not in p.__to_argv__()
    fields = {k: v for k, v in vars(p).items() if k != "l2_reg_weights"}
    assert fields == {k: v for k, v in vars(REParams(metadata_file="m.json", output_model_dir="out")).items() if k != "l2_reg_weights"}
    assert p.l2_reg_weight == 1.0


@pytest.mark.parametrize("bad", ["10,,1", "1,nan", "1,-0.5", "1,2,1", "1,1.0", "inf", "1,x", ","])
def test_bad_lists_are_errors_at_parse_time(bad):
    with pytest.raises(ValueError, match="l2_reg_weights"):
        REParams.__from_argv__(BASE + [f"--l2_reg_weights={bad}"])


# ---- the selection rule ------------------------------------------------------------------------------------------------------------
def test_selection_rule():
    nan = float("nan")
    assert sweep.select_best("auc", [0.7, 0.9, 0.8]) == 1
    assert sweep.select_best("mse", [0.7, 0.9, 0.2, 0.8]) == 2
    assert sweep.select_best("auc", [0.7, 0.9, 0.9]) == 1          # a tie goes to the earlier position
    assert sweep.select_best("mse", [0.5, 0.2, 0.2]) == 1
    assert sweep.select_best("auc", [nan, 0.1, nan]) == 1          # NaN never wins, in either direction
    assert sweep.select_best("mse", [nan, 5.0, None, 7.0]) == 1
    assert sweep.select_best("mse", [0.0]) == 0
    for metric in ("auc", "mse"):
        with pytest.raises(sweep.SweepError, match="undefined"):
            sweep.select_best(metric, [nan, nan])
    with pytest.raises(sweep.SweepError):
        sweep.select_best("rmse", [1.0])


def test_files_have_the_documented_keys(tmp_path):
    blk = dict(auc=0.75, mse=0.2, n=10, n_pos=4, n_neg=6, n_nan=0, two_u=36, sse=2.0)
    out = str(tmp_path)
    sweep.write_model_summary(out, 0, 10.0, "auc", blk)
    sweep.write_model_summary(out, 1, 0.5, "auc", dict(blk, auc=float("nan"), n_nan=1))
    sweep.write_evals(out, "auc", (10.0, 0.5), [0.75, float("nan")], 0)
    with open(os.path.join(out, "sweep", "model-0", "evalSummary.json")) as f:
        m0 = json.load(f)
    assert m0 == dict(auc=0.75, n=10, n_pos=4, n_neg=6, n_nan=0, two_u=36, sse=2.0, l2_reg_weight=10.0)
    with open(os.path.join(out, "sweep", "model-1", "evalSummary.json")) as f:
        m1 = json.load(f)
    assert m1["auc"] is None and m1["l2_reg_weight"] == 0.5 and set(m1) == set(m0)
    with open(os.path.join(out, "sweep", "evals.json")) as f:
        ev = json.load(f)
    assert ev == {"best model index": 0, "model params": {"l2_reg_weight": 10.0}, "metric": "auc",
                  "models": [{"index": 0, "l2_reg_weight": 10.0, "auc": 0.75}, {"index": 1, "l2_reg_weight": 0.5, "auc": None}]}
    sweep.write_model_summary(out, 2, 1.0, "mse", blk)
    with open(os.path.join(out, "sweep", "model-2", "evalSummary.json")) as f:
        assert set(json.load(f)) == {"mse", "n", "n_pos", "n_neg", "n_nan", "two_u", "sse", "l2_reg_weight"}


# ---- the join against the model table's coefficient mapping -------------------------------------------------------------------------
def _features(rng, counts, D):
    """Ascending distinct feature ids per entity -> (feat_ptr, unique)."""
    ptr = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    uniq = np.concatenate([np.sort(rng.choice(D, int(c), replace=False)) for c in counts] + [np.zeros(0, np.int64)]).astype(np.int64)
    return ptr, uniq


def _pair(seed, ic):
    rng = np.random.default_rng(seed)
    D = 40
    # training batch: "u7" listed twice (rows 2 and 9), "empty" has no feature
    train_ids = [f"u{i}" for i in range(9)] + ["u7", "empty", "big"]
    t_counts = np.array([3, 1, 5, 8, 2, 4, 6, 7, 3, 9, 0, 30])
    tfp, tu = _features(rng, t_counts, D)
    P = int(tfp[-1]) + len(train_ids) * ic
    theta = rng.standard_normal(P)
    theta[rng.integers(0, P, 10)] = 0.0
    theta[rng.integers(0, P, 5)] = -0.0
    # evaluation batch: entities unseen in training, features unseen in training, the duplicated id, an entity without features on either side
    eval_ids = ["u3", "nobody", "u7", "empty", "big", "u0", "stranger", "featureless", "u8"]
    e_counts = np.array([10, 4, 12, 3, 40, 6, 1, 0, 5])
    efp, eu = _features(rng, e_counts, D)
    return train_ids, tfp, tu, theta, eval_ids, efp, eu, D


@pytest.mark.parametrize("ic", [1, 0])
@pytest.mark.parametrize("native", [None, False])
def test_join_features_host_equals_the_model_tables_mapping(ic, native):
    train_ids, tfp, tu, theta, eval_ids, efp, eu, D = _pair(11, ic)
    table = ModelTable()
    coef_ptr = tfp + np.arange(len(train_ids) + 1, dtype=np.int64) * ic
    table.add_chunk(list(train_ids), theta, coef_ptr, tu, tfp)
    want_theta, want_has = _model_coefficients_for_batch(table, list(eval_ids), eu, efp, bool(ic), D, native=native)
    te = sweep.train_entity_map(eval_ids, train_ids)
    assert te.dtype == np.int32 and te.tolist() == [3, -1, 9, 10, 11, 0, -1, -1, 8]       # "u7" -> its LAST row
    pos, has = sweep.join_features_host(efp, eu, tfp, tu, te, bool(ic))
    assert pos.dtype == np.int64 and pos.size == int(efp[-1]) + len(eval_ids) * ic
    assert np.array_equal(has, want_has) and has.dtype == np.uint8
    got = np.where(pos >= 0, theta[np.maximum(pos, 0)], 0.0)
    assert np.array_equal(got, want_theta)
    assert (pos >= 0).sum() > 20 and (pos < 0).sum() > 20 and pos.max() < theta.size
    # entities without a model have no place at all; with an intercept, every entity with a model has its intercept
    ecp = efp + np.arange(len(eval_ids) + 1) * ic
    for e in range(len(eval_ids)):
        if not has[e]:
            assert (pos[ecp[e]:ecp[e + 1]] == -1).all()
        elif ic:
            assert pos[ecp[e]] == coef_ptr[te[e]]


def test_join_features_host_of_empty_batches():
    z = np.zeros(0, np.int64)
    pos, has = sweep.join_features_host(np.zeros(1, np.int64), z, np.array([0, 2]), np.array([1, 5]), np.zeros(0, np.int32), True)
    assert pos.size == 0 and has.size == 0
    pos, has = sweep.join_features_host(np.array([0, 2]), np.array([1, 5]), np.zeros(1, np.int64), z, np.array([-1], np.int32), True)
    assert pos.tolist() == [-1, -1, -1] and has.tolist() == [0]


# ---- refusals: before any work, before a solver exists ---------------------------------------------------------------------------------
def _driver(tmp_path, monkeypatch, extra, drop=(), workers=1):
    root = str(tmp_path)
    for d in ("train/active", "valid", "models", "metrics"):
        os.makedirs(os.path.join(root, d), exist_ok=True)
    with open(os.path.join(root, "partitionList.txt"), "w") as f:
        f.write("0")
    argv = ["gdmix", "--stage=random_effect", "--action=train", "--model_type=logistic_regression", f"--partition_list_file={root}/partitionList.txt",
            f"--training_data_dir={root}/train", f"--validation_data_dir={root}/valid", f"--metadata_file={root}/metadata.json",
            "--feature_bag=bag", f"--feature_file={root}/features", "--partition_entity=user_id", f"--output_model_dir={root}/models",
            f"--training_score_dir={root}/ts", f"--validation_score_dir={root}/vs", f"--metric_output_dir={root}/metrics",
            "--uid_column_name=uid", "--label_column_name=response", "--prediction_score_column_name=predictionScore", "--l2_reg_weights=10,1"]
    argv = [a for a in argv if not any(a.startswith(f"--{d}=") for d in drop)] + list(extra)
    monkeypatch.delenv("TF_CONFIG", raising=False)
    monkeypatch.setenv("RANK", "0")
    monkeypatch.setenv("WORLD_SIZE", str(workers))
    params = Params.__from_argv__(argv)
    model = RandomEffectLRLBFGSModel(raw_model_params=argv, base_training_params=params)

    def no_solver():
        raise AssertionError("a solver was asked for")
    monkeypatch.setattr(model, "_get_solver", no_solver)
    monkeypatch.setattr(model, "_read_files", lambda *a, **k: (_ for _ in ()).throw(AssertionError("a partition was read")))
    return RandomEffectDriver(params, model), SchemaParams.__from_argv__(argv), root


@pytest.mark.parametrize("case, message", [("no validation", "validation_data_dir"), ("no metric dir", "metric_output_dir"),
                                           ("prior model", "cold start"), ("rebalance", "rebalance_entities"), ("two workers", "one worker")])
def test_refusals_come_before_any_work(tmp_path, monkeypatch, case, message):
    kw = {"no validation": dict(extra=[], drop=["validation_data_dir"]), "no metric dir": dict(extra=[], drop=["metric_output_dir"]),
          "prior model": dict(extra=[]), "rebalance": dict(extra=["--rebalance_entities=True"]), "two workers": dict(extra=[], workers=2)}[case]
    driver, schema, root = _driver(tmp_path, monkeypatch, **kw)
    if case == "prior model":
        with open(os.path.join(root, "models", "part-00003.avro"), "wb") as f:
            f.write(b"x")
    with pytest.raises(sweep.SweepError, match=message):
        driver.run_training(schema)
    assert not os.path.exists(os.path.join(root, "metrics", "sweep"))
    assert driver.model.model_params.l2_reg_weight == 1.0


def test_inference_ignores_the_flag(tmp_path, monkeypatch):
    driver, schema, root = _driver(tmp_path, monkeypatch, extra=[])
    calls = []
    monkeypatch.setattr(sweep, "run", lambda *a, **k: (_ for _ in ()).throw(AssertionError("the sweep ran")))
    monkeypatch.setattr(driver.model, "predict", lambda **k: calls.append(k["input_data_path"]))
    os.makedirs(os.path.join(root, "train", "active", "partitionId=0"))
    with open(os.path.join(root, "train", "active", "partitionId=0", "part-0.tfrecord"), "wb") as f:
        f.write(b"")
    driver.run_inference(schema)
    assert len(calls) == 1 and driver.model.model_params.l2_reg_weight == 1.0      # (the validation directory is empty)


def test_without_the_flag_training_never_enters_the_sweep(tmp_path, monkeypatch):
    driver, schema, root = _driver(tmp_path, monkeypatch, extra=[], drop=["l2_reg_weights"])
    monkeypatch.setattr(sweep, "run", lambda *a, **k: (_ for _ in ()).throw(AssertionError("the sweep ran")))
    os.makedirs(os.path.join(root, "train", "active", "partitionId=0"))      # an empty partition: the stage has nothing to do
    driver.run_training(schema)
    assert not os.path.exists(os.path.join(root, "metrics", "sweep"))
    assert math.isclose(driver.model.model_params.l2_reg_weight, 1.0)
