"""--l2_reg_weights on the device (include/gdmix_re.h "sweep", csrc/re_sweep.hip, gdmix_amd/sweep.py): gdmix_re_join_features against
its numpy statement, gdmix_re_score_models bit for bit against K calls of gdmix_re_score with host-mapped coefficients, and the stage —
pass 1's metrics against plain runs of the stage at every weight, the winner, and pass 2's files against a plain run at the winner."""
import dataclasses
import json
import os
import shutil

import numpy as np
import pytest

from gdmix_amd import chain, sweep, synthetic
from gdmix_amd.batch import RawBatch
from gdmix_amd.solver import PackedBatch, SolverOptions, _Packed

pytestmark = pytest.mark.gpu

GRID = (100.0, 10.0, 3.0, 1.0, 0.1)
GRID_FLAG = "--l2_reg_weights=100,10,3,1,0.1"
BOUND = 200          # the per-user bound of tests/test_gpu_metrics.py


# ---- pairs of batches ----------------------------------------------------------------------------------------------------------------
def _c2_pair():
    """C2-shaped: the evaluation batch a re-draw with 10 % new entities and shifted columns."""
    E = 20_000
    train = synthetic.make_survey_batch(E, seed=101)
    ev = synthetic.make_survey_batch(E, seed=202, entity_id_base=E // 10)
    return train, dataclasses.replace(ev, col_global=(ev.col_global + 3) % 1024)


def _zipf_batch(seed, E, id_base, D=65536):
    rng = np.random.default_rng(seed)
    n = synthetic.c5_entity_samples(rng, E, mean_nnz=4, k=1)      # two thirds of the entities have one sample (and a quarter of those one non-zero)
    n[E // 2] = 200_000                        # one entity that sees most of the feature space
    N = int(n.sum())
    k = rng.integers(1, 5, N)
    ptr = np.concatenate([[0], np.cumsum(k)]).astype(np.int64)
    Z = int(ptr[-1])
    return RawBatch(ent_row_ptr=np.concatenate([[0], np.cumsum(n)]).astype(np.int64), row_nnz_ptr=ptr,
                    col_global=rng.integers(0, D, Z, dtype=np.int64), val=rng.standard_normal(Z).astype(np.float32),
                    y=(rng.random(N) < 0.5).astype(np.float32), offset=rng.standard_normal(N).astype(np.float32), weight=None,
                    uid=None, entity_ids=[str(i) for i in range(id_base, id_base + E)])


def _zipf_pair():
    E = 12000
    return _zipf_batch(303, E, 0), _zipf_batch(404, E, E // 10)


@pytest.fixture(scope="module")
def chain_base(tmp_path_factory):
    """The chain's inputs up to the per-user partition job, once per model type: global stage trained, partitions written."""
    made = {}

    def get(model_type):
        if model_type not in made:
            data = chain.make_dataset()
            base = str(tmp_path_factory.mktemp("base_" + model_type))
            chain.write_global_inputs(base, data, model_type=model_type)
            chain.run_stage(chain.stage_argv(base, "global", model_type, False))
            if model_type == chain.LINEAR:
                chain.run_stage(chain.global_training_scores_argv(base))
            chain.partition_stage(base, data, "per_user", os.path.join(base, "global", "trainingScores"), os.path.join(base, "global", "validationScores"),
                                  upper_bound=BOUND, model_type=model_type)
            made[model_type] = base
        return made[model_type]
    return get


def _chain_pair(chain_base):
    """Partition 0 of the chain's per-user stage: active training data and validation data, as the stage reads them."""
    from gdmix_amd.io.metadata import DatasetMetadata, read_json_file
    from gdmix_amd.model import RandomEffectLRLBFGSModel
    from gdmix_amd.params import Params, SchemaParams
    base = chain_base(chain.LOGISTIC)
    argv = chain.stage_argv(base, "per_user", chain.LOGISTIC, False)
    model = RandomEffectLRLBFGSModel(raw_model_params=argv, base_training_params=Params.__from_argv__(argv))
    schema = SchemaParams.__from_argv__(argv)
    md = DatasetMetadata(read_json_file(model.metadata_file))
    nf = md.get_feature_shape(model.feature_bag_name)[0]
    with open(os.path.join(base, "per_user", "partition", "partitionList.txt")) as f:
        p = f.readline().split(",")[0]
    train = model._read_files(os.path.join(model.training_data_dir, f"partitionId={p}"), md, schema, nf)
    ev = model._read_files(os.path.join(model.validation_data_dir, f"partitionId={p}"), md, schema, nf)
    return train, ev


@pytest.fixture(scope="module")
def pairs(device_solver, chain_base):
    """name -> (training batch, evaluation batch, packed training batch, packed evaluation batch, host arrays of both)."""
    out = {}
    for name, (train, ev) in (("chain", _chain_pair(chain_base)), ("c2", _c2_pair()), ("zipf", _zipf_pair())):
        tp = device_solver.pack(train, has_intercept=True)
        vp = device_solver.pack(ev, has_intercept=True)
        host = dict(tfp=tp.ent_feat_ptr().cpu().numpy(), tu=tp.unique_global().cpu().numpy(), efp=vp.ent_feat_ptr().cpu().numpy(),
                    eu=vp.unique_global().cpu().numpy(), te=sweep.train_entity_map(ev.entity_ids, train.entity_ids))
        out[name] = (train, ev, tp, vp, host)
    return out


# ---- gdmix_re_join_features ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["chain", "c2", "zipf"])
@pytest.mark.parametrize("ic", [True, False])
def test_join_features_equals_its_numpy_statement(device_solver, pairs, name, ic):
    train, ev, tp, vp, host = pairs[name]
    if not ic:
        tp = device_solver.pack(train, has_intercept=False)
        vp = device_solver.pack(ev, has_intercept=False)
    if name == "zipf":
        d = np.diff(host["efp"])
        assert d.max() >= 20_000 and (d == 1).sum() >= 1000 and np.diff(host["tfp"]).max() >= 20_000
    te = host["te"].copy()
    assert (te >= 0).sum() > 0 and (name == "chain" or (te < 0).sum() > 0)      # (every user of the chain's validation data has training data)
    pos, has = device_solver.join_features(vp, tp, te)
    want_pos, want_has = sweep.join_features_host(host["efp"], host["eu"], host["tfp"], host["tu"], te, ic)
    assert np.array_equal(has.cpu().numpy(), want_has)
    assert np.array_equal(pos.cpu().numpy(), want_pos)
    assert (want_pos >= 0).sum() > 0 and (want_pos[want_pos >= 0] < tp.P).all()
    # a row number outside the training batch counts as no model
    te2 = te.copy()
    te2[:3] = [tp.E, -7, 2_000_000_000]
    pos2, has2 = device_solver.join_features(vp, tp, te2)
    w2 = sweep.join_features_host(host["efp"], host["eu"], host["tfp"], host["tu"], te2, ic)
    assert np.array_equal(pos2.cpu().numpy(), w2[0]) and np.array_equal(has2.cpu().numpy(), w2[1]) and not w2[1][:3].any()


def test_an_empty_evaluation_batch(device_solver, pairs):
    t = device_solver.torch
    _, _, tp, _, _ = pairs["c2"]
    empty = PackedBatch(_Packed(), {"workspace": t.empty(0, dtype=t.uint8, device=device_solver.device)}, None, True)
    pos, has = device_solver.join_features(empty, tp, np.zeros(0, np.int32))
    assert pos.numel() == 0 and has.numel() == 0
    theta = t.zeros(tp.P, dtype=t.float64, device=device_solver.device)
    logit, per = device_solver.score_models(empty, [theta, theta], pos, has)
    assert tuple(logit.shape) == (2, 0) and tuple(per.shape) == (2, 0)
    device_solver.torch.cuda.synchronize()


# ---- gdmix_re_score_models -------------------------------------------------------------------------------------------------------------
def _thetas(device_solver, tp, count, seed):
    """`count` coefficient arrays of the training batch: real solves at different l2 (thresholded: exact zeros), then made-up ones with
    exact zeros, negative zeros and negative values."""
    t = device_solver.torch
    out = []
    for l2 in (10.0, 1.0, 0.1)[:min(3, count)]:
        res = device_solver.solve(tp, SolverOptions(l2=l2, regularize_bias=False, has_intercept=True))
        assert int((res.status < 0).sum()) == 0
        out.append(res.theta_thr)
    rng = np.random.default_rng(seed)
    while len(out) < count:
        th = rng.standard_normal(tp.P) * (0.1 + len(out))
        th[rng.random(tp.P) < 0.2] = 0.0
        th[rng.random(tp.P) < 0.05] = -0.0
        th[rng.random(tp.P) < 0.1] *= -1e-3
        out.append(t.from_numpy(th).to(device_solver.device))
    return out


@pytest.mark.parametrize("name", ["chain", "c2", "zipf"])
def test_score_models_is_bit_identical_to_k_calls_of_score(device_solver, pairs, name):
    """K in {1, 3, 8} and 11 (more than one pass carries), gathered from the K arrays and from the slot-major copy: every row of logit
    and per-coordinate output has the bits gdmix_re_score writes for the host-mapped coefficients."""
    train, ev, tp, vp, host = pairs[name]
    assert device_solver.SWEEP_MODELS_PER_PASS == 8
    pos, has = device_solver.join_features(vp, tp, host["te"])
    pos_h, has_h = sweep.join_features_host(host["efp"], host["eu"], host["tfp"], host["tu"], host["te"], True)
    thetas = _thetas(device_solver, tp, 11, seed=5)
    want = []
    for th in thetas:
        th_h = th.cpu().numpy()
        mapped = np.where(pos_h >= 0, th_h[np.maximum(pos_h, 0)], 0.0)
        lo, pc = device_solver.score(vp, mapped, has_h)
        want.append((lo.cpu().numpy().view(np.uint32), pc.cpu().numpy().view(np.uint32)))
    assert len({w[0].tobytes() for w in want}) == 11          # the models differ
    for K in (1, 3, 8, 11):
        for slot_major in (False, True):
            lo, pc = device_solver.score_models(vp, thetas[:K], pos, has, slot_major=slot_major)
            lo, pc = lo.cpu().numpy().view(np.uint32), pc.cpu().numpy().view(np.uint32)
            for k in range(K):
                assert np.array_equal(lo[k], want[k][0]), (name, K, slot_major, k)
                assert np.array_equal(pc[k], want[k][1]), (name, K, slot_major, k)
    lo, pc = device_solver.score_models(vp, thetas[:3], pos, has, per_coord=False)
    assert pc is None and np.array_equal(lo.cpu().numpy().view(np.uint32)[2], want[2][0])


def test_score_models_refuses_a_small_workspace(device_solver, pairs):
    import ctypes as C
    t = device_solver.torch
    _, _, tp, vp, host = pairs["c2"]
    pos, has = device_solver.join_features(vp, tp, host["te"])
    theta = t.zeros(tp.P, dtype=t.float64, device=device_solver.device)
    ptrs = (C.c_void_p * 2)(theta.data_ptr(), theta.data_ptr())
    logit = t.empty((2, vp.N), dtype=t.float32, device=device_solver.device)
    ws = t.empty(1024, dtype=t.uint8, device=device_solver.device)
    lib = device_solver.lib
    assert lib.gdmix_re_score_models_workspace_bytes(tp.P, 2) == tp.P * 16 and lib.gdmix_re_score_models_workspace_bytes(tp.P, 11) == tp.P * 64
    rc = lib.gdmix_re_score_models(device_solver._h, C.byref(vp.c), 1, ptrs, 2, tp.P, pos.data_ptr(), has.data_ptr(), logit.data_ptr(), None,
                                   ws.data_ptr(), 1024, device_solver._stream())
    assert rc == -3 and b"workspace" in lib.gdmix_re_last_error()
    device_solver.torch.cuda.synchronize()


# ---- the stage ---------------------------------------------------------------------------------------------------------------------------
def _fresh_root(tmp_path_factory, base, name):
    root = str(tmp_path_factory.mktemp(name))
    shutil.copytree(os.path.join(base, "per_user", "partition"), os.path.join(root, "per_user", "partition"))
    return root


def _run(root, model_type, extra, child=False, env=None):
    argv = chain.stage_argv(root, "per_user", model_type, device_metrics=True) + list(extra)
    keep = {k: os.environ.get(k) for k in (env or {})}
    os.environ.update(env or {})
    try:
        chain.run_stage(argv, child_process=child)
    finally:
        for k, v in keep.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def _json(*path):
    with open(os.path.join(*path)) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def stages(tmp_path_factory, chain_base):
    """Per model type: the sweep's root, a plain run per weight (child processes, every partition a batch of its own), and a plain run at
    l2 = 3 in this process."""
    made = {}

    def get(model_type):
        if model_type in made:
            return made[model_type]
        base = chain_base(model_type)
        tag = "lin" if model_type == chain.LINEAR else "log"
        swept = _fresh_root(tmp_path_factory, base, f"sweep_{tag}")
        _run(swept, model_type, [GRID_FLAG])
        plain = []
        for k, w in enumerate(GRID):
            r = _fresh_root(tmp_path_factory, base, f"plain_{tag}_{k}")
            _run(r, model_type, [f"--l2_reg_weight={w!r}"], child=True, env={"GDMIX_PARTITIONS_PER_BATCH": "1"})
            plain.append(r)
        made[model_type] = dict(swept=swept, plain=plain, base=base)
        return made[model_type]
    return get


@pytest.mark.parametrize("model_type", [chain.LOGISTIC, chain.LINEAR])
def test_stage_sweep_metrics_winner_and_outputs(stages, tmp_path_factory, model_type):
    from test_gpu_metrics import _files
    st = stages(model_type)
    metric = "mse" if model_type == chain.LINEAR else "auc"
    mdir = os.path.join(st["swept"], "per_user", "metrics")
    values = []
    for k, w in enumerate(GRID):
        got = _json(mdir, "sweep", f"model-{k}", "evalSummary.json")
        want = _json(st["plain"][k], "per_user", "metrics", "evalSummary.json")["validation"]
        print(f"{model_type} l2 {w}: sweep {metric} {got[metric]!r}, plain run {want[metric]!r}, two_u {got['two_u']} / {want['two_u']}, "
              f"sse {got['sse']!r} / {want['sse']!r}")
        assert got["l2_reg_weight"] == w
        assert set(got) == {metric, "n", "n_pos", "n_neg", "n_nan", "two_u", "sse", "l2_reg_weight"}
        for key in ("two_u", "n_pos", "n_neg", "n", "n_nan"):
            assert got[key] == want[key], (k, key)
        assert abs(got["sse"] - want["sse"]) <= 1e-12 * abs(want["sse"])
        values.append(want[metric])
    evals = _json(mdir, "sweep", "evals.json")
    best = sweep.select_best(metric, values)
    assert evals["best model index"] == best and evals["model params"] == {"l2_reg_weight": GRID[best]} and evals["metric"] == metric
    assert [m["l2_reg_weight"] for m in evals["models"]] == list(GRID) and [m["index"] for m in evals["models"]] == list(range(len(GRID)))
    if model_type == chain.LOGISTIC:
        assert best == 2 and 0 < best < len(GRID) - 1
    # everything outside metrics/sweep/ is what a plain run at the winner writes, under the same environment (both in this process)
    plain = _fresh_root(tmp_path_factory, st["base"], "plain_best")
    _run(plain, model_type, [f"--l2_reg_weight={GRID[best]!r}"])
    a = _files(os.path.join(st["swept"], "per_user"))
    b = _files(os.path.join(plain, "per_user"))
    sweep_prefix = os.path.join("metrics", "sweep") + os.sep
    assert any(k.startswith(sweep_prefix) for k in a) and not any(k.startswith(sweep_prefix) for k in b)      # no flag, no sweep/ directory
    rest = {k: v for k, v in a.items() if not k.startswith(sweep_prefix)}
    assert sorted(rest) == sorted(b)
    for k in b:
        assert rest[k] == b[k], k
    assert any(k.startswith("models") for k in b) and any(k.startswith("validationScores") for k in b) and os.path.join("metrics", "evalSummary.json") in b


def test_a_chunked_sweep_writes_the_same_numbers(stages, tmp_path_factory):
    """The grid solved and scored two models at a time (as when K x P x 8 bytes do not fit): the same files under sweep/."""
    from test_gpu_metrics import _files
    st = stages(chain.LOGISTIC)
    root = _fresh_root(tmp_path_factory, st["base"], "sweep_chunked")
    _run(root, chain.LOGISTIC, [GRID_FLAG], env={"GDMIX_SWEEP_CHUNK": "2"})
    assert _files(os.path.join(root, "per_user", "metrics", "sweep")) == _files(os.path.join(st["swept"], "per_user", "metrics", "sweep"))
