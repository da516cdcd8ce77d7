"""--feature_normalization through the command line, both stages (gdmix_amd/feature_stats.py, model.py, fe_model.py), on the MI355X box.

Random effect: about 600 entities in 3 Java-hashed partitions, 24 features, one column times 1000 and one nearly constant (a year / 2000).
The models are held to the CPU oracle solving prior_helpers.transform_raw(mean = 0, scale) and restored, by the rule and bar of
test_gpu_prior.test_two_days_of_incremental_training: 1e-5 on the well-posed entities (the intercept is not regularised: an entity whose
labels are all equal has no finite optimum, SURVEY 8(d) class D), which must be at least nine tenths of them. Scores are x . theta + offset
with the written theta to 1 ulp of the Avro float; the statistics file equals the stand-in's exactly.

Fixed effect: n = 4 000, D = 60, held to fe_prior_helpers' Newton minimiser for mean 0 and v = s^2 at test_gpu_fe_prior's BAR; the variances
at that file's rtol; then two gloo ranks on the one GPU."""
import contextlib
import json
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

import fe_prior_helpers as fh
import prior_helpers as ph
from gdmix_amd import chain, feature_stats as fs, synthetic
from helpers import well_posed_mask
from oracle import oracle

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
L2 = 2.0
DIM = 24
PARTS = 3
BAR = 1e-5
KINDS = [fs.SCALE_WITH_STANDARD_DEVIATION, fs.SCALE_WITH_MAX_MAGNITUDE]


@contextlib.contextmanager
def pinned_avro():
    """The Avro sync marker is os.urandom(16): pinned inside the writer's module, so that equal files are equal bytes."""
    from gdmix_amd.io import avro as avro_mod

    class PinnedOs:
        urandom = staticmethod(lambda n: b"\x07" * n)

        def __getattr__(self, k):
            return getattr(os, k)
    mp = pytest.MonkeyPatch()
    mp.setattr(avro_mod, "os", PinnedOs())
    try:
        yield
    finally:
        mp.undo()


# ---- random effect ------------------------------------------------------------------------------------------------------------------------
def _rescaled(b, seed):
    """Column 3 times 1000; column 7 a year / 2000 (nearly constant)."""
    rng = np.random.default_rng(seed)
    v = b.val.copy()
    v[b.col_global == 3] *= np.float32(1000)
    at = b.col_global == 7
    v[at] = ((1940 + rng.integers(0, 60, int(at.sum()))) / 2000.0).astype(np.float32)
    b.val = v
    return b


def _write(root, name, batch, parts, sub):
    from gdmix_amd.io.grouped_reader import write_grouped_partition
    for p, ents in enumerate(parts):
        d = os.path.join(root, name, *sub, f"partitionId={p}")
        os.makedirs(d, exist_ok=True)
        write_grouped_partition(os.path.join(d, "part-00000.tfrecord"), batch.select(ents), "ent", "bag")


def _re_argv(root, tag, kind, stats_file, models=None):
    out = os.path.join(root, "out_" + tag)
    models = models or os.path.join(out, "models")
    for d in (models, os.path.join(out, "ts"), os.path.join(out, "vs")):
        os.makedirs(d, exist_ok=True)
    return out, ["gdmix", "--stage=random_effect", "--action=train", "--model_type=logistic_regression", "--uid_column_name=uid",
                 "--label_column_name=response", "--weight_column_name=weight", "--prediction_score_column_name=predictionScore",
                 f"--partition_list_file={root}/partitionList.txt", f"--training_data_dir={root}/train", f"--validation_data_dir={root}/valid",
                 f"--metadata_file={root}/meta.json", f"--feature_file={root}/features.csv", "--feature_bag=bag", "--partition_entity=ent",
                 f"--output_model_dir={models}", f"--training_score_dir={out}/ts", f"--validation_score_dir={out}/vs", "--regularize_bias=False",
                 f"--l2_reg_weight={L2}", "--random_effect_variance_mode=simple", f"--feature_normalization={kind}",
                 f"--feature_statistics_file={stats_file}"]


def _models(path):
    from gdmix_amd.io import avro
    out = {}
    for r in avro.read_file(path):
        out[r["modelId"]] = ({(m["name"], m["term"]): m["value"] for m in r["means"]},
                             {(m["name"], m["term"]): m["value"] for m in (r.get("variances") or [])})
    return out


@pytest.fixture(scope="module")
def re_stage(tmp_path_factory, device_solver):
    """The data on disk, the reference statistics, and one cold run per normalisation type."""
    from gdmix_amd.solver import java_partition_id
    root = str(tmp_path_factory.mktemp("feature_normalization_re"))
    E = 600
    train = _rescaled(synthetic.make_batch(E, 12, 4, DIM, seed=51, random_weights=True), 1)
    valid = _rescaled(synthetic.make_batch(E, 5, 4, DIM, seed=52, random_weights=True), 2)
    ids = [f"e{i}" for i in range(E)]
    train.entity_ids, valid.entity_ids = list(ids), list(ids)
    valid.uid = valid.uid + 1000000
    assert int(train.ent_n().max()) < 32          # no tall class: an entity's kernel does not depend on the batch it is solved in
    parts = [[e for e in range(E) if java_partition_id(ids[e], PARTS) == p] for p in range(PARTS)]
    assert all(len(p) > 100 for p in parts)
    _write(root, "train", train, parts, ("active",))
    _write(root, "valid", valid, parts, ())
    md = {"features": [{"name": "bag", "dtype": "float", "shape": [DIM], "isSparse": True},
                       {"name": "offset", "dtype": "float", "shape": [], "isSparse": False},
                       {"name": "weight", "dtype": "float", "shape": [], "isSparse": False},
                       {"name": "uid", "dtype": "long", "shape": [], "isSparse": False},
                       {"name": "ent", "dtype": "string", "shape": [], "isSparse": False}],
          "labels": [{"name": "response", "dtype": "int", "shape": [], "isSparse": False}]}
    json.dump(md, open(os.path.join(root, "meta.json"), "w"))
    with open(os.path.join(root, "features.csv"), "w") as f:
        f.write("".join(f"f{i},\n" for i in range(DIM)))
    with open(os.path.join(root, "partitionList.txt"), "w") as f:
        f.write(",".join(str(p) for p in range(PARTS)))
    acc = fs.NumpyAccumulator(DIM)
    stats = fs.collect(acc, lambda a: a.add(train.col_global, train.val), train.N, fs.SCALE_WITH_STANDARD_DEVIATION)
    runs = {}
    with pinned_avro():
        for kind in KINDS:
            stats_file = os.path.join(root, f"stats_{kind}.npz")
            out, argv = _re_argv(root, kind, kind, stats_file)
            chain.run_stage(argv)
            runs[kind] = dict(out=out, stats_file=stats_file)
    return dict(root=root, train=train, valid=valid, parts=parts, ids=ids, stats=stats, runs=runs)


def _expected(st, kind, p, theta0=None):
    """The oracle's model of partition p in normalised units, restored: (batch, pack, coefficient pointer, thresholded theta, variances)."""
    b = st["train"].select(st["parts"][p])
    pk = oracle.pack(b.ent_row_ptr, b.row_nnz_ptr, b.col_global)
    cp = ph.coef_ptr(pk, True)
    s = fs.factors(kind, st["stats"])
    scale = np.ones(int(cp[-1]))
    fp = pk["ent_feat_ptr"]
    scale[np.arange(int(fp[-1])) + np.repeat(np.arange(b.E), np.diff(fp)) + 1] = s[pk["unique_global"]]
    mean = np.zeros_like(scale)
    val2, off2 = ph.transform_raw(b, pk, mean, scale, True)
    kw = dict(l2=L2, regularize_bias=False, has_intercept=True)
    opts = oracle.make_opts(variance_mode=1, **kw)
    ref = oracle.solve(pk, val2, b.y, off2, b.weight, opts) if theta0 is None else oracle.solve(pk, val2, b.y, off2, b.weight, opts, theta0 / scale)
    theta, thr, variance = ph.restore(mean, scale, ref["theta"], ref["variance"], 1e-4)
    return b, pk, cp, thr, variance, well_posed_mask(b, kw)


def _compare_models(st, kind, model_dir, theta0_of=None):
    worst, worst_var, compared, total = 0.0, 0.0, 0, 0
    for p in range(PARTS):
        got = _models(os.path.join(model_dir, f"part-{p:05d}.avro"))
        b, pk, cp, want, want_var, well_posed = _expected(st, kind, p, None if theta0_of is None else theta0_of(p))
        fp = pk["ent_feat_ptr"]
        total += b.E
        for e, eid in enumerate(b.entity_ids):
            if not well_posed[e]:
                continue
            names = [("(INTERCEPT)", "")] + [(f"f{int(g)}", "") for g in pk["unique_global"][fp[e]:fp[e + 1]]]
            have = np.array([got[eid][0].get(n, 0.0) for n in names])
            w = want[cp[e]:cp[e + 1]]
            assert np.array_equal(have == 0.0, w == 0.0), eid
            worst = max(worst, float(np.abs(have - w).max() / max(1.0, np.abs(w).max())))
            kept = have != 0.0
            hv = np.array([got[eid][1].get(n, 0.0) for n in names])
            worst_var = max(worst_var, float(np.max(np.abs(hv[kept] / want_var[cp[e]:cp[e + 1]][kept] - 1.0), initial=0.0)))
            compared += 1
    return worst, worst_var, compared, total


def _written_theta(got, b, pk, cp):
    fp = pk["ent_feat_ptr"]
    written = np.zeros(int(cp[-1]))
    for e, eid in enumerate(b.entity_ids):
        names = [("(INTERCEPT)", "")] + [(f"f{int(g)}", "") for g in pk["unique_global"][fp[e]:fp[e + 1]]]
        written[cp[e]:cp[e + 1]] = [got[eid][0].get(n, 0.0) for n in names]
    return written


def test_the_reference_alone_compares_nine_tenths_of_the_entities():
    """(CPU arithmetic only.) The labels leave at most a tenth of the entities without a finite optimum."""
    train = synthetic.make_batch(600, 12, 4, DIM, seed=51, random_weights=True)
    share = float(well_posed_mask(train, dict(l2=L2, regularize_bias=False, has_intercept=True)).mean())
    print(f"well-posed entities: {share:.3f}")
    assert share >= 0.9


@pytest.mark.parametrize("kind", KINDS)
def test_random_effect_models_scores_and_statistics(re_stage, kind):
    st, run = re_stage, re_stage["runs"][kind]
    # the statistics file: the reference, exactly (a one-pass run writes no moments: count and maximum are compared)
    got = fs.load(run["stats_file"], DIM)
    if kind == fs.SCALE_WITH_STANDARD_DEVIATION:
        assert got.equal_bits(st["stats"])
    else:
        assert got.num_samples == st["train"].N and np.array_equal(got.count, st["stats"].count)
        assert np.array_equal(got.max_abs.view(np.uint32), st["stats"].max_abs.view(np.uint32)) and np.all(np.isnan(got.variance))
    s = fs.factors(kind, st["stats"])
    assert s[3] < 1e-2 and np.all(s > 0) and np.all(np.delete(s, 3) > 0.2)      # the column times 1000 gets the small factor
    # the models
    model_dir = os.path.join(run["out"], "models")
    worst, worst_var, compared, total = _compare_models(st, kind, model_dir)
    print(f"{kind}: worst coefficient distance to the oracle {worst:.3e}, worst relative variance distance {worst_var:.3e}, "
          f"over {compared} well-posed entities of {total}")
    assert compared >= 0.9 * total
    assert worst <= BAR, worst
    # Var(theta_j) = s_j^2 Var'(phi_j), SIMPLE: 1 / (H_jj + l2) at phi. phi agrees to 1e-5, the curvature weights rho (1 - rho) move by at
    # most that much times |x'| |phi| = O(10): 1e-3 bounds the relative distance with an order of magnitude to spare
    assert worst_var <= 1e-3, worst_var
    # the scores of the training and of the validation data: x . theta + offset with the written theta, 1 ulp of the Avro float
    for name, data, sdir in (("training", st["train"], "ts"), ("validation", st["valid"], "vs")):
        scores = chain.read_scores(os.path.join(run["out"], sdir))
        by_uid = dict(zip(scores[0].tolist(), scores[1].tolist()))
        assert len(by_uid) == data.N
        for p in range(PARTS):
            models = _models(os.path.join(model_dir, f"part-{p:05d}.avro"))
            b = data.select(st["parts"][p])
            pk = oracle.pack(b.ent_row_ptr, b.row_nnz_ptr, b.col_global)
            cp = ph.coef_ptr(pk, True)
            lo, _ = oracle.score(pk, b.val, b.offset, _written_theta(models, b, pk, cp), True)
            have = np.array([by_uid[int(u)] for u in b.uid], np.float32)
            u = np.abs(have.astype(np.float64) - lo.astype(np.float64)) / np.spacing(np.maximum(np.abs(have), np.abs(lo)).astype(np.float32)).astype(np.float64)
            print(f"{kind}, {name} partition {p}: scores within {u.max():.3f} ulp of x . theta + offset")
            assert u.max() <= 1.0, float(u.max())


def _model_bytes(model_dir):
    return [open(os.path.join(model_dir, f"part-{p:05d}.avro"), "rb").read() for p in range(PARTS)]


def test_a_second_run_reads_the_file_and_grouping_changes_nothing(re_stage, monkeypatch):
    from gdmix_amd import model as model_mod
    st = re_stage
    kind = fs.SCALE_WITH_STANDARD_DEVIATION
    first = _model_bytes(os.path.join(st["runs"][kind]["out"], "models"))

    def no_pass(self, col, val):
        raise AssertionError("a statistics pass ran although the file exists")
    with pinned_avro():
        with monkeypatch.context() as m:
            m.setattr(fs.DeviceAccumulator, "add", no_pass)
            out, argv = _re_argv(st["root"], "again", kind, st["runs"][kind]["stats_file"])
            chain.run_stage(argv)
        assert _model_bytes(os.path.join(out, "models")) == first
        assert model_mod.GROUP_MAX >= 3                     # the runs so far solved the three cold partitions in one device batch
        for group in (1, 4):
            monkeypatch.setattr(model_mod, "GROUP_MAX", group)
            out, argv = _re_argv(st["root"], f"group{group}", kind, os.path.join(st["root"], f"stats_group{group}.npz"))
            chain.run_stage(argv)
            assert _model_bytes(os.path.join(out, "models")) == first
            assert fs.load(os.path.join(st["root"], f"stats_group{group}.npz"), DIM).equal_bits(st["stats"])


def test_a_warm_run_from_the_first_models_stays_within_the_bar(re_stage):
    st = re_stage
    kind = fs.SCALE_WITH_STANDARD_DEVIATION
    models = os.path.join(st["root"], "models_warm")
    shutil.copytree(os.path.join(st["runs"][kind]["out"], "models"), models)
    before = _model_bytes(models)

    first = os.path.join(st["runs"][kind]["out"], "models")

    def theta0_of(p):       # the start point of partition p: the first run's written model in the batch's coefficient order
        b = st["train"].select(st["parts"][p])
        pk = oracle.pack(b.ent_row_ptr, b.row_nnz_ptr, b.col_global)
        return _written_theta(_models(os.path.join(first, f"part-{p:05d}.avro")), b, pk, ph.coef_ptr(pk, True))
    out, argv = _re_argv(st["root"], "warm", kind, st["runs"][kind]["stats_file"], models=models)
    chain.run_stage(argv)
    assert len(before) == PARTS
    worst, _, compared, total = _compare_models(st, kind, models, theta0_of)
    print(f"warm run: worst coefficient distance to the oracle started at phi0 = theta0 / s: {worst:.3e} over {compared} of {total}")
    assert compared >= 0.9 * total and worst <= BAR


# ---- fixed effect -------------------------------------------------------------------------------------------------------------------------
FE_SHAPE = (4000, 5, 60, 4)
FE_SEED = 17


def fe_case():
    """fe_prior_helpers' seeded shard with column 0 times 1000 and column 1 a year / 2000; its prior replaced by mean 0, v = s^2."""
    c = fh.case(FE_SEED, *FE_SHAPE, False)
    rng = np.random.default_rng(FE_SEED)
    val = c.val.copy()
    val[c.col == 0] *= np.float32(1000)
    at = c.col == 1
    val[at] = ((1940 + rng.integers(0, 60, int(at.sum()))) / 2000.0).astype(np.float32)
    c.val = val
    X = np.zeros((c.n, c.D + 1))
    np.add.at(X, (np.repeat(np.arange(c.n), c.k), c.col), val.astype(np.float64))
    X[:, c.D] = 1.0
    c.X = X
    acc = fs.NumpyAccumulator(c.D)
    stats = fs.collect(acc, lambda a: a.add(c.col, c.val), c.n, fs.SCALE_WITH_STANDARD_DEVIATION)
    return c, stats


def fe_minimiser(c, stats, kind):
    s = fs.factors(kind, stats)
    prior = fh.with_prior(c, np.zeros(c.D + 1), np.concatenate([s * s, [1.0]]))
    return prior, fh.newton(prior, fh.L2, True)


@pytest.mark.parametrize("kind", KINDS)
def test_fixed_effect_stage_through_the_command_line(tmp_path, kind):
    from gdmix_amd import gdmix
    from test_gpu_fe_prior import BAR as FE_BAR, _argv, _model, _write_day
    root = str(tmp_path)
    c, stats = fe_case()
    D = c.D
    md = {"features": [{"name": "global", "dtype": "float", "shape": [D], "isSparse": True},
                       {"name": "offset", "dtype": "float", "shape": [], "isSparse": False},
                       {"name": "weight", "dtype": "float", "shape": [], "isSparse": False},
                       {"name": "uid", "dtype": "long", "shape": [], "isSparse": False}],
          "labels": [{"name": "response", "dtype": "int", "shape": [], "isSparse": False}]}
    json.dump(md, open(os.path.join(root, "meta.json"), "w"))
    with open(os.path.join(root, "features.csv"), "w") as f:
        f.write("".join(f"f{i},\n" for i in range(D)))
    _write_day(root, "day1", c)
    models = os.path.join(root, "models")
    stats_file = os.path.join(root, "stats.npz")
    gdmix.run(_argv(root, "day1", models, "n", [f"--feature_normalization={kind}", f"--feature_statistics_file={stats_file}"]))
    got_stats = fs.load(stats_file, D)
    if kind == fs.SCALE_WITH_STANDARD_DEVIATION:
        assert got_stats.equal_bits(stats)
    else:
        assert np.array_equal(got_stats.count, stats.count) and np.array_equal(got_stats.max_abs.view(np.uint32), stats.max_abs.view(np.uint32))
    prior, star = fe_minimiser(c, stats, kind)
    s = fh.scale(prior, True)
    assert s[0] < 1e-2 and np.all(s[1:] > 0.2) and np.all(s[D - c.absent:D] == 1.0)      # the column times 1000; the dead features
    got, got_var = _model(os.path.join(models, "part-00000.avro"), D)
    kept = got != 0.0
    worst = float(np.max(np.abs(got - star)[kept] / s[kept]))
    print(f"{kind}: {int(kept.sum())} of {D + 1} coefficients written, max |theta - theta*| / s = {worst:.3g}")
    assert worst <= FE_BAR
    assert np.all(np.abs(star[~kept]) <= 1e-4 + FE_BAR * s[~kept])           # what the threshold dropped
    np.testing.assert_allclose(got_var[kept], fh.variances(prior, got, fh.L2, True, full=False)[kept], rtol=1e-8)
    # without the flag it is another model
    plain = os.path.join(root, "models_plain")
    gdmix.run(_argv(root, "day1", plain, "p", []))
    plain_theta, _ = _model(os.path.join(plain, "part-00000.avro"), D)
    assert np.max(np.abs(plain_theta - star) / s) > 1e3 * FE_BAR


def test_two_fixed_effect_workers_have_the_bits_of_one(tmp_path):
    from test_gpu_fe_prior import BAR as FE_BAR
    root = os.path.dirname(HERE)
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    env.pop("TF_CONFIG", None)
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2", "--master-addr", "127.0.0.1",
           "--master-port", "29643", os.path.join(root, "tests", "_fe_norm_dist_worker.py"), str(tmp_path)]
    subprocess.run(cmd, check=True, env=env, timeout=300, cwd=root)
    res = json.load(open(tmp_path / "result.json"))
    assert len(res) == 2
    a, b = res
    assert a["theta"] == b["theta"] and a["variances"] == b["variances"] and (a["status"], a["nit"], a["nfev"]) == (b["status"], b["nit"], b["nfev"])
    c, stats = fe_case()
    for rank in (0, 1):
        assert fs.load(str(tmp_path / f"stats{rank}.npz"), c.D).equal_bits(stats)          # the one-worker statistics, bit for bit
    assert os.path.exists(tmp_path / "written.npz") and fs.load(str(tmp_path / "written.npz"), c.D).equal_bits(stats)
    prior, star = fe_minimiser(c, stats, fs.SCALE_WITH_STANDARD_DEVIATION)
    theta = np.array(a["theta"])
    assert a["status"] in (0, 1)
    worst = float(np.max(np.abs(theta - star) / fh.scale(prior, True)))
    print(f"two workers ({a['_backend']}): max |theta - theta*| / s = {worst:.3g}")
    assert worst <= FE_BAR
    np.testing.assert_allclose(a["variances"], fh.variances(prior, theta, fh.L2, True, full=False), rtol=1e-8)
