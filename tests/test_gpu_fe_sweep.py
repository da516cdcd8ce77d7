"""The fixed-effect stage's --metric_output_dir and --l2_reg_weights on the device: the K-model scoring pass (csrc/fe_sweep.hip) against K
calls of gdmix_fe_score, gdmix_fe_restart against a fresh gdmix_fe_create, the stage through the command line against plain runs, the plain
stage's metric against the numpy reference and `python -m gdmix_amd.evaluate`, and the coordinate chain with a swept global stage.

"Byte for byte" between two runs' Avro files means every byte but the container's sync marker, 16 random bytes per file
(gdmix_amd/io/avro.py: os.urandom): avro_bytes() zeroes them where they stand and compares the rest, lengths included."""
import dataclasses
import json
import os
import shutil
import subprocess
import sys
from fractions import Fraction

import numpy as np
import pytest

from gdmix_amd import chain, sweep
from gdmix_amd import fixed_effect as fe
from gdmix_amd.solver import GdmixReError, SolverOptions
from metrics_reference import sse_reference, two_u_reference
from test_fe_sweep_host import avro_bytes

HERE = os.path.dirname(os.path.abspath(__file__))
GRID = (100.0, 30.0, 10.0, 3.0, 1.0, 0.1)
GRID_TEXT = "100,30,10,3,1,0.1"
WINNER = {chain.LOGISTIC: 3, chain.LINEAR: 1}      # l2 = 3 and l2 = 30 on the CPU oracle, by margins thousands of times the device's distance from it


def load(name):
    z = np.load(os.path.join(HERE, "golden", f"fe_{name}.npz"))
    return {k: z[k] for k in z.files}


# ---- the K-model pass -------------------------------------------------------------------------------------------------------------
def _raw_shard(case, seed=3):
    """-> (row_nnz_ptr, col, val, offset, D, has_intercept): rows of 0, 1 - 3 and >= 4 non-zeros in every bagged case."""
    rng = np.random.default_rng(seed)
    n, D = (0 if case == "empty" else 5000), 700
    k = rng.integers(0, 14, n)
    if n:
        k[:6] = [0, 1, 2, 3, 4, 9]
        k[-3:] = [0, 5, 0]
        k[rng.integers(0, n, 3)] = 900
    rp = np.concatenate([[0], np.cumsum(k)]).astype(np.int64)
    cols = np.minimum((float(D + 1) ** rng.random(rp[-1])).astype(np.int64) - 1, D - 1)
    vals = (rng.standard_normal(rp[-1]) * 0.4).astype(np.float32)
    vals[rng.random(rp[-1]) < 0.05] = 0.0
    off = None if case == "no_offset" else (0.3 * rng.standard_normal(n)).astype(np.float32)
    if case == "no_bag":
        return None, None, None, (0.3 * rng.standard_normal(n)).astype(np.float32), 0, True
    return rp, cols, vals, off, D, case != "no_intercept"


def _models(K, P, seed=5):
    rng = np.random.default_rng(seed)
    out = []
    for k in range(K):
        th = rng.standard_normal(P) * (0.5 + k)
        th[rng.random(P) < 0.2] = 0.0
        th[rng.random(P) < 0.05] = -0.0
        th[P - 1] = 0.25 * (k + 1) * (-1) ** k      # (the last place is the intercept: K intercept-only models stay K different models)
        out.append(th)
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("slot_major", [True, False])
@pytest.mark.parametrize("K", [1, 3, 8, 11])
@pytest.mark.parametrize("case", ["mixed", "no_offset", "no_intercept", "no_bag", "empty"])
def test_score_models_rows_are_the_bits_of_gdmix_fe_score(device_solver, case, K, slot_major):
    rp, cols, vals, off, D, ic = _raw_shard(case)
    s = fe.FixedEffectDeviceSolver(solver=device_solver)
    n = (rp.size - 1) if rp is not None else off.size
    shard = s.upload(rp, cols, vals, off, D)
    thetas = _models(K, D + (1 if ic else 0))
    score, per = s.score_models(shard, thetas, ic, per_coord=True, slot_major=slot_major)
    only_score, none = s.score_models(shard, thetas, ic, per_coord=False, slot_major=slot_major)
    assert none is None and tuple(score.shape) == (K, n) == tuple(per.shape)
    score, per, only_score = (x.cpu().numpy() for x in (score, per, only_score))
    seen = set()
    for k, th in enumerate(thetas):
        one_score, one_per = (x.cpu().numpy() for x in s.score_device(shard, th, ic))
        assert np.array_equal(score[k].view(np.uint32), one_score.view(np.uint32)), (case, K, k)
        assert np.array_equal(per[k].view(np.uint32), one_per.view(np.uint32)), (case, K, k)
        assert np.array_equal(only_score[k].view(np.uint32), one_score.view(np.uint32))
        seen.add(one_score.tobytes())
    if n:
        assert len(seen) == K and np.isfinite(score).all()      # K different models, K different rows
        if rp is not None:      # the shard has the three kinds of rows, and the scores are those of the definition
            lens = np.diff(rp)
            assert (lens == 0).any() and ((lens >= 1) & (lens <= 3)).any() and (lens >= 4).any()
            rows = np.repeat(np.arange(n), lens)
            want = np.bincount(rows, vals.astype(np.float64) * thetas[0][cols], n) + (thetas[0][D] if ic else 0.0)
            np.testing.assert_allclose(per[0], want, rtol=2e-6, atol=1e-6)


@pytest.mark.gpu
def test_score_models_in_forced_chunks_of_two(device_solver, monkeypatch):
    rp, cols, vals, off, D, ic = _raw_shard("mixed", seed=9)
    s = fe.FixedEffectDeviceSolver(solver=device_solver)
    shard = s.upload(rp, cols, vals, off, D)
    thetas = _models(7, D + 1)
    assert s.models_per_chunk(7, D + 1, shard.n) == 7                 # 7 x (coefficients + two rows) is nothing next to the HBM
    monkeypatch.setenv("GDMIX_SWEEP_CHUNK", "2")
    chunk = s.models_per_chunk(7, D + 1, shard.n)
    assert chunk == 2
    whole, _ = s.score_models(shard, thetas, ic, per_coord=False)
    rows = [s.score_models(shard, thetas[f:f + chunk], ic, per_coord=False)[0] for f in range(0, 7, chunk)]
    assert [int(r.shape[0]) for r in rows] == [2, 2, 2, 1]
    got = device_solver.torch.cat(rows).cpu().numpy()
    assert np.array_equal(got.view(np.uint32), whole.cpu().numpy().view(np.uint32))


@pytest.mark.gpu
def test_score_models_refuses_what_it_cannot_score(device_solver):
    rp, cols, vals, off, D, ic = _raw_shard("mixed")
    s = fe.FixedEffectDeviceSolver(solver=device_solver)
    shard = s.upload(rp, cols, vals, off, D)
    with pytest.raises(GdmixReError):
        s.score_models(shard, [], ic)
    with pytest.raises(GdmixReError):
        s.score_models(shard, _models(2, D), ic)                    # a vector without the intercept's place
    with pytest.raises(ValueError, match="feature index"):
        s.upload(rp, cols + 1, vals, off, D)


# ---- restart ----------------------------------------------------------------------------------------------------------------------
def _zipf_shard():
    """150 k samples x ~12 Zipf-distributed columns of 140 k features: row blocks of ~25 k entries are cut into several units of 8192,
    and feature 0 has more than the 65 536 entries from which a column gets its place in the frequent-column table."""
    rng = np.random.default_rng(17)
    n, D = 150_000, 140_000
    k = rng.integers(4, 21, n)
    rp = np.concatenate([[0], np.cumsum(k)]).astype(np.int64)
    cols = np.minimum((float(D + 1) ** rng.random(rp[-1])).astype(np.int64) - 1, D - 1)
    vals = (rng.standard_normal(rp[-1]) * 0.3).astype(np.float32)
    assert np.bincount(cols).max() >= (1 << 16) and rp[-1] / 8192 > 2 * ((n + 2047) // 2048)
    z = 0.2 * rng.standard_normal(n)
    return dict(row_nnz_ptr=rp, col_global=cols, val=vals, offset=(0.2 * rng.standard_normal(n)).astype(np.float32), num_features=D, has_intercept=True,
                y_logistic=(rng.random(n) < 0.3).astype(np.float32), y_linear=(3.0 + z).astype(np.float32))


def _problem_inputs(solver, c, linear):
    ic = bool(c["has_intercept"])
    y = c["y_linear" if linear else "y_logistic"] if "y_logistic" in c else c["y"]
    batch, _ = fe.shard_as_batch(c["row_nnz_ptr"], c["col_global"], c["val"], y, c["offset"], None, ic, binary_labels=not linear, dummy=False)
    return solver.pack(batch, has_intercept=ic), int(c["num_features"]), ic


def _opts(w, ic, linear, max_iter, **kw):
    return SolverOptions(**dict(dict(l2=w, regularize_bias=False, has_intercept=ic, m=10, max_iter=max_iter, threshold=0.0, sum_loss=True, linear=linear), **kw))


def _solve(prob, lookahead=None):
    status = fe.run_stepping_loop(prob, None, lookahead=lookahead)
    theta, info = prob.result()
    return theta, dict(info, status=status)


def _check_restart(solver, c, linear, weights, max_iter, with_start):
    packed, D, ic = _problem_inputs(solver, c, linear)
    t = solver.torch
    t0 = None
    if with_start:
        t0 = t.from_numpy(0.05 * np.random.default_rng(2).standard_normal(D + (1 if ic else 0))).to(solver.device)
    fresh = {}
    for w in weights:
        prob = fe._SteppingProblem(solver, packed, D, _opts(w, ic, linear, max_iter), t0)
        fresh[w] = _solve(prob)
        prob.close()
    assert len({th.tobytes() for th, _ in fresh.values()}) == len(weights)       # the weights do give different models
    assert all(info["nit"] >= 2 for _, info in fresh.values())
    for order in (weights, weights[::-1]):
        # created for ANOTHER weight and start point than any it is restarted for, and solved once before the first restart
        prob = fe._SteppingProblem(solver, packed, D, _opts(7.0, ic, linear, max_iter, regularize_bias=ic, ftol=1e-9), None)
        _solve(prob)
        for w in order:
            prob.restart(_opts(w, ic, linear, max_iter), t0)
            theta, info = _solve(prob)
            assert np.array_equal(theta, fresh[w][0]), (w, order)
            assert info == fresh[w][1], (w, order, info, fresh[w][1])            # fval, gnorm, nit, nfev, status
        prob.close()


@pytest.mark.gpu
@pytest.mark.parametrize("with_start", [False, True])
@pytest.mark.parametrize("name", ["logistic_wide", "linear_wide", "logistic_offset", "linear_offset"])
def test_restart_and_solve_give_the_bits_of_create_and_solve_on_golden_shards(device_solver, name, with_start):
    c = load(name)
    _check_restart(device_solver, c, bool(c["linear"]), (10.0, 1.0, 0.1), 100, with_start)


@pytest.mark.gpu
@pytest.mark.parametrize("with_start", [False, True])
@pytest.mark.parametrize("linear", [False, True])
def test_restart_on_a_shard_with_several_units_per_pass_and_frequent_columns(device_solver, linear, with_start):
    _check_restart(device_solver, _zipf_shard(), linear, (30.0, 3.0, 0.3), 25, with_start)


@pytest.mark.gpu
def test_restart_straight_after_a_solve_that_left_no_ops_behind_the_stop(device_solver):
    """gdmix_fe_solve with lookahead 2 enqueues two evaluations and steps behind the one that stopped; they return on the stop flag. The
    restart clears the flag behind them, on the stream: the next solve is a fresh one, and so is one after a solve cut short by max_evals."""
    c = load("logistic_wide")
    packed, D, ic = _problem_inputs(device_solver, c, False)
    ref = {}
    for w in (5.0, 0.5):
        prob = fe._SteppingProblem(device_solver, packed, D, _opts(w, ic, False, 100), None)
        ref[w] = _solve(prob, lookahead=0)
        prob.close()
    prob = fe._SteppingProblem(device_solver, packed, D, _opts(5.0, ic, False, 100), None)
    status, evals = prob.solve(lookahead=2)
    th, info = prob.result()
    assert status >= 0 and evals >= info["nfev"] + 2 and np.array_equal(th, ref[5.0][0])       # two no-ops were enqueued behind the stop
    prob.restart(_opts(0.5, ic, False, 100), None)
    status, evals = prob.solve(lookahead=2)
    th, info = prob.result()
    assert np.array_equal(th, ref[0.5][0]) and dict(info, status=status) == ref[0.5][1] and evals >= info["nfev"] + 2
    status, _ = prob.solve(lookahead=2, max_evals=1)      # a stopped problem: no-ops only, the status of the stop
    assert status == ref[0.5][1]["status"]
    prob.restart(_opts(5.0, ic, False, 100), None)
    status, _ = prob.solve(lookahead=2, max_evals=3)      # cut short: still running (-1) ...
    assert status == -1
    prob.restart(_opts(5.0, ic, False, 100), None)       # ... and restarted from the middle of a run
    assert _solve(prob, lookahead=5)[1] == ref[5.0][1]
    prob.close()


@pytest.mark.gpu
def test_restart_through_eval_and_step_as_three_launches(tmp_path):
    root = os.path.dirname(HERE)
    out = str(tmp_path / "result.json")
    env = dict(os.environ, GDMIX_FE_FUSED_TAIL="0")
    env.pop("TF_CONFIG", None)
    subprocess.run([sys.executable, os.path.join(HERE, "_fe_restart_worker.py"), "logistic_wide", out], check=True, env=env, timeout=600, cwd=root)
    with open(out) as f:
        res = json.load(f)
    assert [r["l2"] for r in res] == [10.0, 1.0, 0.1]
    for r in res:
        assert r["theta_equal"] and r["info_equal"] and r["nit"] >= 2 and r["status"] in (0, 1), r


@pytest.mark.gpu
def test_restart_refuses_what_the_pool_was_not_sized_for(device_solver):
    c = load("logistic_offset")
    packed, D, ic = _problem_inputs(device_solver, c, False)
    prob = fe._SteppingProblem(device_solver, packed, D, _opts(1.0, ic, False, 100), None)
    assert ic
    for other in (dict(m=5), dict(linear=True), dict(has_intercept=False)):
        with pytest.raises(GdmixReError, match="gdmix_fe_restart"):
            prob.restart(dataclasses.replace(_opts(1.0, ic, False, 100), **other), None)
    prob.restart(_opts(1.0, ic, False, 100), None)       # the refusals left the problem usable
    assert _solve(prob)[1]["status"] in (0, 1)
    prob.close()


# ---- the stage, through the command line, in process ------------------------------------------------------------------------------
def _json(*path):
    with open(os.path.join(*path)) as f:
        return json.load(f)


def _run_global(base, root, model_type, extra):
    """One fixed-effect stage under `root` on a copy of base's inputs; -> root."""
    shutil.copytree(os.path.join(base, "global"), os.path.join(root, "global"))
    chain.run_stage(chain.stage_argv(root, "global", model_type, False) + list(extra))
    return root


@pytest.fixture(scope="module")
def global_stages(tmp_path_factory, device_solver):
    """Per model type: the inputs (984 training samples, ~99 k validation samples), the sweep's root, a plain run with the metric per weight."""
    data = chain.make_dataset(943, 1682, 100_000, train_fraction=0.01)
    assert int(data["train"].sum()) == 984
    made = {}

    def get(model_type):
        if model_type not in made:
            tag = "lin" if model_type == chain.LINEAR else "log"
            base = str(tmp_path_factory.mktemp(f"fe_inputs_{tag}"))
            chain.write_global_inputs(base, data, model_type=model_type)
            swept = str(tmp_path_factory.mktemp(f"fe_sweep_{tag}"))
            shutil.copytree(os.path.join(base, "global"), os.path.join(swept, "global"))
            chain.run_stage(chain.stage_argv(swept, "global", model_type, False, l2_grids={"global": GRID_TEXT}))
            plain = []
            for k, w in enumerate(GRID):
                r = str(tmp_path_factory.mktemp(f"fe_plain_{tag}_{k}"))
                plain.append(_run_global(base, r, model_type, [f"--l2_reg_weight={w!r}", f"--metric_output_dir={chain.metric_dir(r, 'global')}"]))
            made[model_type] = dict(base=base, swept=swept, plain=plain, data=data)
        return made[model_type]
    return get


@pytest.mark.gpu
@pytest.mark.parametrize("model_type", [chain.LOGISTIC, chain.LINEAR])
def test_stage_sweep_is_six_plain_runs_and_the_plain_run_at_the_winner(global_stages, model_type):
    st = global_stages(model_type)
    metric = "mse" if model_type == chain.LINEAR else "auc"
    mdir = chain.metric_dir(st["swept"], "global")
    values = []
    for k, w in enumerate(GRID):
        got = _json(mdir, "sweep", f"model-{k}", "evalSummary.json")
        want = _json(chain.metric_dir(st["plain"][k], "global"), "evalSummary.json")["validation"]
        print(f"{model_type} l2 {w}: sweep {metric} {got[metric]!r}, plain run {want[metric]!r}, two_u {got['two_u']} / {want['two_u']}, sse {got['sse']!r} / {want['sse']!r}")
        assert got["l2_reg_weight"] == w and set(got) == {metric, "n", "n_pos", "n_neg", "n_nan", "two_u", "sse", "l2_reg_weight"}
        for key in ("two_u", "n_pos", "n_neg", "sse", metric, "n", "n_nan"):
            assert got[key] == want[key], (k, key)                       # exactly: the same coefficients, the same scores, one batch each
        assert got["n"] == int((~st["data"]["train"]).sum()) and got["n_nan"] == 0
        info = _json(chain.metric_dir(st["plain"][k], "global"), "evalSummary.json")
        assert info["data"] == "validation" and ("training" in info) == (model_type == chain.LOGISTIC)
        values.append(got[metric])
    evals = _json(mdir, "sweep", "evals.json")
    best = WINNER[model_type]
    assert evals["best model index"] == best == sweep.select_best(metric, values) and evals["model params"] == {"l2_reg_weight": GRID[best]}
    assert evals["metric"] == metric and [m["l2_reg_weight"] for m in evals["models"]] == list(GRID) and [m[metric] for m in evals["models"]] == values
    # the stage's own files: byte for byte the plain run's at the winning weight
    a, b = os.path.join(st["swept"], "global"), os.path.join(st["plain"][best], "global")
    files = [("models", "part-00000.avro"), ("validationScores", "part-00000.avro")] + ([("trainingScores", "part-00000.avro")] if model_type == chain.LOGISTIC else [])
    for d, fn in files:
        assert avro_bytes(os.path.join(a, d, fn)) == avro_bytes(os.path.join(b, d, fn)), (d, fn)
    if model_type == chain.LINEAR:      # (plain linear regression does not score its training data, with or without a sweep)
        assert not os.path.exists(os.path.join(a, "trainingScores", "part-00000.avro")) and not os.path.exists(os.path.join(b, "trainingScores", "part-00000.avro"))
    with open(os.path.join(a, "metrics", "evalSummary.json"), "rb") as f, open(os.path.join(b, "metrics", "evalSummary.json"), "rb") as g:
        assert f.read() == g.read()
    for root in [st["swept"]] + st["plain"]:
        assert not os.path.exists(os.path.join(chain.metric_dir(root, "global"), "perEntity"))
    assert sorted(os.listdir(mdir)) == ["evalSummary.json", "sweep"] and sorted(os.listdir(chain.metric_dir(st["plain"][best], "global"))) == ["evalSummary.json"]


@pytest.mark.gpu
def test_a_chunked_stage_sweep_writes_the_same_files(global_stages, tmp_path, monkeypatch):
    st = global_stages(chain.LOGISTIC)
    monkeypatch.setenv("GDMIX_SWEEP_CHUNK", "2")
    root = str(tmp_path / "chunked")
    shutil.copytree(os.path.join(st["base"], "global"), os.path.join(root, "global"))
    chain.run_stage(chain.stage_argv(root, "global", chain.LOGISTIC, False, l2_grids={"global": GRID_TEXT}))
    a, b = chain.metric_dir(root, "global"), chain.metric_dir(st["swept"], "global")
    for rel in [("evalSummary.json",), ("sweep", "evals.json")] + [("sweep", f"model-{k}", "evalSummary.json") for k in range(len(GRID))]:
        with open(os.path.join(a, *rel), "rb") as f, open(os.path.join(b, *rel), "rb") as g:
            assert f.read() == g.read(), rel


# ---- the plain stage's metric -----------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("model_type", [chain.LOGISTIC, chain.LINEAR])
def test_plain_stage_summary_is_the_exact_metric_of_its_score_files(global_stages, device_solver, tmp_path, model_type):
    from gdmix_amd import evaluate
    st = global_stages(model_type)
    metric = "mse" if model_type == chain.LINEAR else "auc"
    root = st["plain"][WINNER[model_type]]
    summary = _json(chain.metric_dir(root, "global"), "evalSummary.json")
    blocks = [("validation", "validationScores")] + ([("training", "trainingScores")] if model_type == chain.LOGISTIC else [])
    assert set(summary) == {metric, "n", "n_pos", "n_neg", "n_nan", "two_u", "sse", "data"} | {b for b, _ in blocks}
    assert summary["data"] == "validation" and {k: summary[k] for k in summary["validation"]} == summary["validation"]
    for block, d in blocks:
        _, sc, _, lab = chain.read_scores(os.path.join(root, "global", d))
        two_u, n_pos, n_neg, n_nan = two_u_reference(sc, lab)
        blk = summary[block]
        print(f"{model_type} {block}: {blk}")
        assert (blk["n"], blk["n_nan"], blk["two_u"], blk["n_pos"], blk["n_neg"]) == (sc.size, 0, two_u, n_pos, n_neg) and n_nan == 0
        if metric == "auc":
            assert blk["auc"] == float(Fraction(two_u, 2 * n_pos * n_neg))
        else:      # fp64 sums of ~1e5 terms in two orders (the device's, math.fsum's): 1e-12 relative, as tests/test_gpu_metrics.py takes it
            want = sse_reference(sc, lab)
            assert abs(blk["sse"] - want) <= 1e-12 * want and blk["mse"] == blk["sse"] / sc.size
    out = str(tmp_path / "evaluate")
    v = evaluate.run(["--metricsInputDir", os.path.join(root, "global", "validationScores"), "--outputMetricFile", out, "--labelColumnName", "response",
                      "--predictionColumnName", "predictionScore", "--metricName", metric], solver=device_solver)
    assert _json(out, "evalSummary.json") == {metric: v}
    assert summary[metric] == v if metric == "auc" else abs(summary[metric] - v) <= 1e-12 * v


@pytest.mark.gpu
def test_inference_reports_what_it_scores(global_stages, tmp_path):
    st = global_stages(chain.LOGISTIC)
    plain = st["plain"][WINNER[chain.LOGISTIC]]
    root = str(tmp_path / "inference")
    shutil.copytree(os.path.join(plain, "global"), os.path.join(root, "global"))
    shutil.rmtree(os.path.join(root, "global", "metrics"))
    os.remove(os.path.join(root, "global", "validationScores", "part-00000.avro"))
    argv = [a.replace("--action=train", "--action=inference") for a in chain.stage_argv(root, "global", chain.LOGISTIC, False)]
    chain.run_stage(argv + [f"--metric_output_dir={chain.metric_dir(root, 'global')}", "--l2_reg_weights=5,6"])      # (the grid is ignored)
    got = _json(chain.metric_dir(root, "global"), "evalSummary.json")
    _, sc, _, lab = chain.read_scores(os.path.join(root, "global", "validationScores"))
    two_u, n_pos, n_neg, n_nan = two_u_reference(sc, lab)
    assert set(got) == {"auc", "n", "n_pos", "n_neg", "n_nan", "two_u", "sse", "data", "validation"} and got["data"] == "validation"
    assert (got["n"], got["n_nan"], got["two_u"], got["n_pos"], got["n_neg"]) == (sc.size, n_nan, two_u, n_pos, n_neg)
    assert got["auc"] == float(Fraction(two_u, 2 * n_pos * n_neg)) and os.listdir(chain.metric_dir(root, "global")) == ["evalSummary.json"]


# ---- the chain --------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_chain_with_a_swept_global_stage(tmp_path):
    data = chain.make_dataset(300, 500, 20_000)
    bounds = {"per_user": 48}
    root = str(tmp_path / "swept")
    res = chain.run_chain(root, data, upper_bounds=bounds, l2_grids={"global": GRID_TEXT})
    w = res["global"]["l2_reg_weight"]
    assert w in GRID and w == _json(chain.metric_dir(root, "global"), "sweep", "evals.json")["model params"]["l2_reg_weight"]
    assert "l2_reg_weight" not in res["per_user"] and "l2_reg_weight" not in res["per_movie"]
    for stage in chain.STAGES:
        for which in ("train", "validation"):
            dev, host = res[stage][f"{which}_auc_device"], res[stage][f"{which}_auc"]
            print(f"{stage} {which}: device AUC {dev!r}, from the score files {host!r}")
            assert abs(dev - host) <= 1e-12                      # exact integers on the device, average ranks in fp64 on the host
    # the same chain with the global stage GIVEN the winner
    plain = str(tmp_path / "plain")
    chain.write_global_inputs(plain, data)
    prev = None
    for stage in chain.STAGES:
        if stage != "global":
            chain.partition_stage(plain, data, stage, os.path.join(plain, prev, "trainingScores"), os.path.join(plain, prev, "validationScores"), 4,
                                  upper_bound=bounds.get(stage))
        chain.run_stage(chain.stage_argv(plain, stage, chain.LOGISTIC, True) + ([f"--l2_reg_weight={w!r}"] if stage == "global" else []))
        prev = stage
    compared = 0
    for stage in chain.STAGES:
        for d in ("models", "trainingScores", "validationScores"):
            for r, _, fs in os.walk(os.path.join(root, stage, d)):
                for fn in fs:
                    other = os.path.join(plain, os.path.relpath(os.path.join(r, fn), root))
                    assert avro_bytes(os.path.join(r, fn)) == avro_bytes(other), other
                    compared += 1
            assert sorted(os.listdir(os.path.join(root, stage, d))) == sorted(os.listdir(os.path.join(plain, stage, d)))
    assert compared >= 3 + 2 * 3 * 4
    for stage in ("per_user", "per_movie"):
        with open(os.path.join(chain.metric_dir(root, stage), "evalSummary.json"), "rb") as f, open(os.path.join(chain.metric_dir(plain, stage), "evalSummary.json"), "rb") as g:
            assert f.read() == g.read()
