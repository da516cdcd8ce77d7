"""GPU: the random effect's Poisson loss (SolverOptions(loss="poisson"); include/gdmix_re.h, "poisson") on every solve kernel family
against scipy's fmin_l_bfgs_b run live on the numpy statement of the objective (re_poisson_helpers: the reference, the sample of entities
it runs on, the adjudication rule and its bars). Batches and forced routings are those of tests/test_gpu_re_linear.py: the smallest shapes
that reach every family. Variances against the numpy restatement at the device's theta: rtol 1e-7 (SIMPLE), 1e-4 (FULL)."""
import dataclasses
import json
import os

import numpy as np
import pytest

from gdmix_amd import synthetic
from gdmix_amd.solver import SolverOptions
from oracle import oracle
import re_linear_helpers as H
import re_poisson_helpers as P
from test_gpu_re_linear import BATCHES, FAMILIES, OPTION_SETS, _families_used

pytestmark = pytest.mark.gpu

_BATCH_CACHE = {}


def _batch(name, seed):
    """The count-labelled batch and its oracle pack, made once per (batch, label seed)."""
    if (name, seed) not in _BATCH_CACHE:
        b = synthetic.with_count_labels(BATCHES[name](), seed=seed)
        _BATCH_CACHE[(name, seed)] = (b, oracle.pack(b.ent_row_ptr, b.row_nnz_ptr, b.col_global))
    return _BATCH_CACHE[(name, seed)]


def _solve_and_compare(solver, b, pk, kw, routing, warm=False, want_families=None, key=None, entities=None):
    packed = solver.pack(b, has_intercept=kw["has_intercept"])
    th0 = 0.1 * np.random.default_rng(5).standard_normal(int(packed.P)) if warm else None
    H.set_routing(solver, **routing)
    try:
        res = solver.solve(packed, SolverOptions(loss="poisson", **kw), theta0=th0).to_host()
        used = _families_used(solver, packed)
    finally:
        H.reset_routing(solver)
    if want_families is not None:
        assert want_families <= used, (want_families, used)
    assert np.all(res["status"] >= 0) and np.all(res["status"] <= 4), np.unique(res["status"])
    assert np.all(np.isfinite(res["theta"])) and np.all(np.isfinite(res["fval"]))
    coef_ptr = packed.coef_ptr_host()
    ref = P.reference(b, pk, {k: v for k, v in kw.items() if k != "variance_mode"}, th0, coef_ptr, key=key, seed=0, entities=entities)
    P.compare(res, ref, coef_ptr)
    if kw.get("variance_mode") == 1:      # the in-kernel SIMPLE variance, D_i = w_i exp(z_i) at the returned theta
        want = P.variance_numpy(b, pk, kw, 1, res["theta"], coef_ptr, entities=ref["entities"])
        for e in ref["entities"]:
            s = slice(int(coef_ptr[e]), int(coef_ptr[e + 1]))
            np.testing.assert_allclose(res["variance"][s], want[s], rtol=1e-7)
    return used, res, packed, coef_ptr, ref


@pytest.mark.parametrize("name,batch,routing,families", FAMILIES, ids=[f[0] for f in FAMILIES])
@pytest.mark.parametrize("oi", range(len(OPTION_SETS)))
def test_poisson_matches_scipy(device_solver, name, batch, routing, families, oi):
    """Every solver family (default routing; LDS-wavefront; workgroup; team tiers; device-wide; tall, tall-mid, tall-team) with the
    Poisson loss on count labels, weights and offsets; option sets: unregularised intercept, regularised intercept, no intercept,
    m in {1, 3, 10}, max_iter = 2; SIMPLE variance in two of them; a warm start on the odd option sets."""
    kw = dict(OPTION_SETS[oi])
    b, pk = _batch(batch, oi)
    _solve_and_compare(device_solver, b, pk, kw, routing, warm=bool(oi & 1), want_families=families, key=(batch, oi))


@pytest.mark.parametrize("m", [10, 12])
def test_poisson_two_loop_kernels_and_full_variance(device_solver, m):
    """m = 12 is above the compact form's history: the LDS-wavefront kernel and the two-loop workgroup kernel take everything (both with
    their own Poisson instantiation); FULL variance against the numpy restatement at the device's theta, from the solve and from
    gdmix_re_variance_full."""
    kw = dict(l2=1.0, regularize_bias=False, has_intercept=True, m=m, max_iter=100, ftol=1e-12, variance_mode=2)
    for name in ("ragged", "ml_user"):
        b, pk = _batch(name, m)
        used, res, packed, cp, ref = _solve_and_compare(device_solver, b, pk, kw, dict(lds_limit=16384, tall_min_n=0) if m == 12 else {}, key=(name, "m", m))
        if m == 12:
            assert used <= {"re_solve_wave_kernel", "re_solve_team_kernel"}, used
        want = P.variance_numpy(b, pk, kw, 2, res["theta"], cp)
        np.testing.assert_allclose(res["variance"], want, rtol=1e-4)
        v = device_solver.variance_full(device_solver.pack(b), SolverOptions(loss="poisson", **kw), res["theta"])
        np.testing.assert_allclose(v.cpu().numpy(), want, rtol=1e-4)


def test_poisson_simple_variance_on_team_classes(device_solver):
    """The team kernels hold the losses in one instantiation and get no variance pointer for Poisson: re_variance_simple_kernel<LOSS_POISSON> follows
    them with D_i = w_i exp(z_i) at the returned theta. Workgroup class, the three team tiers and the device-wide class, with and without
    an intercept."""
    for routing, name in ((dict(lds_limit=0, tall_min_n=0), "ragged"), (dict(team_nnz=64, tall_min_n=0), "zipf"), (dict(giant_nnz=1, tall_min_n=0), "tall")):
        for ic in (True, False):
            kw = dict(l2=0.5, regularize_bias=False, has_intercept=ic, m=10, max_iter=5, ftol=1e-12, variance_mode=1)
            b, pk = _batch(name, 3)
            packed = device_solver.pack(b, has_intercept=ic)
            H.set_routing(device_solver, **routing)
            try:
                res = device_solver.solve(packed, SolverOptions(loss="poisson", **kw)).to_host()
                assert _families_used(device_solver, packed) == {"re_solve_team_kernel"}
            finally:
                H.reset_routing(device_solver)
            np.testing.assert_allclose(res["variance"], P.variance_numpy(b, pk, kw, 1, res["theta"], packed.coef_ptr_host()), rtol=1e-7)


def test_poisson_range_of_exp(device_solver):
    """64 entities of 16 samples whose offsets place z over [-30, 25] at the solution: the label of a sample is the rounded rate exp(offset)
    (up to 7e10; the solver sees the float) and its weight exp(-offset), so the fitted margins stay near the offsets and the curvature
    w exp(z) near 1 on every entity: exp is evaluated over the whole range on a well-conditioned problem (with a regularised intercept, so
    that the entities whose labels are all 0 have a minimum). Everything is finite; the comparison is test 1's."""
    b0 = synthetic.make_batch(64, 16, 4, 64, seed=51, size_dist="const", with_uid=False)
    rng = np.random.default_rng(52)
    off = np.repeat(np.linspace(-30.0, 25.0, b0.E), 16) + 0.2 * rng.standard_normal(b0.N)
    y = np.round(np.exp(off + 0.1 * rng.standard_normal(b0.N))).astype(np.float32)
    b = dataclasses.replace(b0, offset=off.astype(np.float32), y=y, binary_labels=False, weight=np.exp(-off).astype(np.float32))
    pk = oracle.pack(b.ent_row_ptr, b.row_nnz_ptr, b.col_global)
    kw = dict(l2=1.0, regularize_bias=True, has_intercept=True, m=10, max_iter=100, ftol=1e-12, variance_mode=1)
    used, res, packed, cp, ref = _solve_and_compare(device_solver, b, pk, kw, {}, entities=np.arange(b.E))
    z_lo, z_hi = np.inf, -np.inf
    for e in range(b.E):
        X, _, o, _ = P.entity_sparse(b, pk, e, True)
        z = X @ res["theta"][cp[e]:cp[e + 1]] + o
        z_lo, z_hi = min(z_lo, float(z.min())), max(z_hi, float(z.max()))
    print(f"margins at the solution span [{z_lo:.2f}, {z_hi:.2f}]")
    assert z_lo <= -29.0 and z_hi >= 24.0
    assert np.all(np.isfinite(res["variance"])) and np.all(np.isfinite(res["gnorm"]))
    logit, _ = device_solver.score(packed, res["theta"])
    assert np.all(np.isfinite(logit.cpu().numpy()))


def test_poisson_c2_batch_lands_in_the_logistic_classes(device_solver):
    """Routing unchanged: the c2 batch's class_counts under Poisson equal those under logistic (classification goes by LDS footprint)."""
    b0 = BATCHES["c2"]()
    kw = dict(l2=1.0, regularize_bias=False, has_intercept=True, m=10, max_iter=3)
    packed = device_solver.pack(b0)
    device_solver.solve(packed, SolverOptions(**kw))
    logistic = device_solver.class_counts(packed)
    packed_p = device_solver.pack(synthetic.with_count_labels(b0, seed=1))
    device_solver.solve(packed_p, SolverOptions(loss="poisson", **kw))
    assert device_solver.class_counts(packed_p) == logistic
    assert sum(c for name, c in logistic if name.startswith("re_solve_grp_kernel")) == b0.E


def test_a_loss_code_outside_the_three_is_refused(device_solver):
    """gdmix_re_opts.loss is a loss code since ABI 19: 0, 1, 2 and nothing else (it used to be a flag: every non-zero value meant squared).
    The three codes reach their kernels through the launchers' one dispatch; 3 and -1 are refused at the entry point."""
    import ctypes as C
    b, _ = _batch("tall", 0)
    packed = device_solver.pack(b)
    o = SolverOptions().to_c()
    t = device_solver.torch
    theta = t.zeros(int(packed.P), dtype=t.float64, device=device_solver.device)
    var = t.zeros_like(theta)
    for code in (0, 1, 2, 3, -1):
        o.loss = code
        rc = device_solver.lib.gdmix_re_variance_full(device_solver._h, C.byref(packed.c), C.byref(o), theta.data_ptr(), var.data_ptr(), None)
        if code in (0, 1, 2):
            assert rc == 0, (code, device_solver.lib.gdmix_re_last_error())
        else:
            assert rc != 0 and b"no loss code" in device_solver.lib.gdmix_re_last_error(), code
    t.cuda.synchronize(device_solver.device)


# ---- the product path --------------------------------------------------------------------------------------------------------------
def _read_models(path, with_variance=False):
    from gdmix_amd.io import avro
    out = {}
    for r in avro.read_file(path):
        means = {(m["name"], m["term"]): m["value"] for m in r["means"]}
        out[r["modelId"]] = (means, {(m["name"], m["term"]): m["value"] for m in (r.get("variances") or [])}, r["modelClass"]) if with_variance else means
    return out


def _scipy_models(b, pk, l2=1.0):
    """scipy per entity at the CLI job's options (re_linear_helpers.job_argv): theta [P] and coef_ptr."""
    cp = np.asarray(pk["ent_feat_ptr"]) + np.arange(b.E + 1)
    kw = dict(l2=l2, regularize_bias=False, has_intercept=True, m=10, max_iter=100, ftol=1e-12)
    ref = P.reference(b, pk, kw, None, cp, entities=np.arange(b.E))
    return np.concatenate([ref["theta"][e] for e in range(b.E)]), cp


def _names(pk, e):
    fp = pk["ent_feat_ptr"]
    return [("(INTERCEPT)", "")] + [(f"f{int(g)}", "") for g in pk["unique_global"][fp[e]:fp[e + 1]]]


def test_cli_child_process_trains_and_scores_a_poisson_partition(tmp_path):
    """One partition directory (60 entities) through `python -m gdmix_amd.gdmix` as a child process: train with --metric_output_dir, then
    inference. Model Avro coefficients <= 1e-5 from scipy's on every entity, the PoissonRegressionModel class name; scores within 1 ulp of
    x . theta + offset of the Avro float (the margin, never exp); evalSummary.json's poisson_loss against numpy on the written scores.
    Then a second day with --incremental_training=True against scipy on the centred objective."""
    from gdmix_amd import chain
    from test_gpu_chain import _scores_by_uid, _ulps
    import prior_helpers as ph
    b = synthetic.with_count_labels(H.small_job_batch(E=60, seed=21, real=False), 21)
    root = str(tmp_path)
    H.write_job(root, b)
    extra = [f"--metric_output_dir={root}/metrics", "--random_effect_variance_mode=simple"]
    chain.run_stage(H.job_argv(root, "train", model_type="poisson_regression", extra=extra), child_process=True)
    chain.run_stage(H.job_argv(root, "inference", model_type="poisson_regression"), child_process=True)
    pk = oracle.pack(b.ent_row_ptr, b.row_nnz_ptr, b.col_global)
    theta, cp = _scipy_models(b, pk)
    got = _read_models(os.path.join(root, "models", "part-00000.avro"), with_variance=True)
    assert set(got) == set(b.entity_ids)
    worst, written = 0.0, np.zeros(int(cp[-1]))
    for e, eid in enumerate(b.entity_ids):
        means, _, cls = got[eid]
        assert cls == "com.linkedin.photon.ml.supervised.regression.PoissonRegressionModel"
        want = theta[cp[e]:cp[e + 1]]
        have = np.array([means.get(nm, 0.0) for nm in _names(pk, e)])
        written[cp[e]:cp[e + 1]] = have
        worst = max(worst, float(np.abs(have - np.where(np.abs(want) <= 1e-4, 0.0, want)).max() / max(1.0, np.abs(want).max())))
    print(f"model Avro against scipy: worst {worst:.3e}")
    assert worst <= 1e-5, worst
    lo, _ = oracle.score(pk, b.val, b.offset, written, True)
    order = np.argsort(b.uid, kind="stable")
    for d in ("trainingScores", "validationScores", "inferenceScores"):
        s = _scores_by_uid(os.path.join(root, d))
        assert np.array_equal(s["uid"], b.uid[order])
        assert _ulps(s["score"], lo.astype(np.float32)[order]).max() <= 1.0, d
        assert np.array_equal(s["label"], b.y[order])
    summary = json.load(open(os.path.join(root, "metrics", "evalSummary.json")))
    s = _scores_by_uid(os.path.join(root, "validationScores"))
    from gdmix_amd import metrics
    import math
    t = metrics.poisson_loss_terms(s["score"], s["label"])
    want_pl = math.fsum(t)
    assert summary["data"] == "validation" and summary["n"] == b.N and summary["n_nan"] == 0
    assert abs(summary["pl"] - want_pl) <= 3e-13 * math.fsum(np.abs(np.exp(s["score"].astype(np.float64))) + np.abs(s["label"].astype(np.float64) * s["score"].astype(np.float64)))
    assert abs(summary["poisson_loss"] - want_pl / b.N) <= 1e-12 * abs(want_pl / b.N)
    assert "auc" not in summary and "mse" not in summary and summary["training"]["n"] == b.N
    # ---- day 2: the L2 term centred on day 1's model and weighted by its precisions; scipy in the transformed space (prior_helpers)
    b2 = synthetic.with_count_labels(H.small_job_batch(E=60, seed=22, real=False), 22)
    b2 = dataclasses.replace(b2, entity_ids=list(b.entity_ids), uid=b2.uid + 100000)
    root2 = os.path.join(root, "day2")
    H.write_job(root2, b2)
    import shutil
    shutil.copytree(os.path.join(root, "models"), os.path.join(root2, "models"))
    chain.run_stage(H.job_argv(root2, "train", model_type="poisson_regression", extra=["--random_effect_variance_mode=simple", "--incremental_training=True"]),
                    child_process=True)
    pk2 = oracle.pack(b2.ent_row_ptr, b2.row_nnz_ptr, b2.col_global)
    cp2 = ph.coef_ptr(pk2, True)
    plain = {}
    for eid, (mu, va, _) in got.items():
        feats = sorted(int(n[1:]) for (n, _) in mu if n != "(INTERCEPT)")
        names = [("(INTERCEPT)", "")] + [(f"f{g}", "") for g in feats]
        plain[eid] = (np.array([mu[n] for n in names]), np.array([va[n] for n in names]), np.array(feats, np.int64))
    mean, var = ph.map_prior_plain(plain, b2.entity_ids, pk2["unique_global"], pk2["ent_feat_ptr"], True)
    var[cp2[:-1]] = 1.0      # the intercept is not regularised: no penalty, scale 1
    scale = np.sqrt(var)
    val2, off2 = ph.transform_raw(b2, pk2, mean, scale, True)
    bt = dataclasses.replace(b2, val=val2, offset=off2)
    kw = dict(l2=1.0, regularize_bias=False, has_intercept=True, m=10, max_iter=100, ftol=1e-12)
    ref = P.reference(bt, pk2, kw, None, cp2, entities=np.arange(b2.E))
    phi = np.concatenate([ref["theta"][e] for e in range(b2.E)])
    want2 = mean + scale * phi
    post = _read_models(os.path.join(root2, "models", "part-00000.avro"))
    worst2 = 0.0
    for e, eid in enumerate(b2.entity_ids):
        have = np.array([post[eid].get(nm, 0.0) for nm in _names(pk2, e)])
        w = want2[cp2[e]:cp2[e + 1]]
        worst2 = max(worst2, float(np.abs(have - np.where(np.abs(w) <= 1e-4, 0.0, w)).max() / max(1.0, np.abs(w).max())))
    print(f"day 2 (incremental) against scipy on the centred objective: worst {worst2:.3e}")
    assert worst2 <= 1e-5, worst2


def test_three_coordinate_chain_poisson_regression(tmp_path):
    """run_chain(model_type="poisson_regression") on the 100 k MovieLens-shaped ratings (1 .. 5 stars as counts), no upper bound: every
    stage's files exist and it reports poisson_loss; the training poisson_loss sum does not increase from stage to stage — each stage starts
    at theta = 0, which reproduces the previous stage's loss, and minimises per entity, so it holds per entity; 32 sampled per-user models
    agree with scipy (fed the product's previous score files as offsets) to 1e-5."""
    from gdmix_amd import chain, metrics
    from test_gpu_chain import _models, _scores_by_uid
    data = chain.make_dataset()
    assert data["n"] == 100_000
    root = str(tmp_path / "chain")
    res = chain.run_chain(root, data, num_partitions=4, model_type="poisson_regression")
    for s in chain.STAGES:
        for d in ("models", "trainingScores", "validationScores"):
            assert os.listdir(os.path.join(root, s, d)), (s, d)
        assert np.isfinite(res[s]["train_poisson_loss"]) and np.isfinite(res[s]["validation_poisson_loss"]) and "train_auc" not in res[s] and "train_mse" not in res[s]
    got = {s: _scores_by_uid(os.path.join(root, s, "trainingScores")) for s in chain.STAGES}
    for s in ("per_user", "per_movie"):      # the device's mean against numpy's on the written scores: the header's 3e-13 of the mean magnitude, plus 1e-13 for numpy's own (pairwise) mean
        s64, y64 = got[s]["score"].astype(np.float64), got[s]["label"].astype(np.float64)
        assert abs(res[s]["train_poisson_loss_device"] - res[s]["train_poisson_loss"]) <= 4e-13 * float(np.mean(np.exp(s64) + np.abs(y64 * s64)))
    uid0 = int(data["uid"].min())
    ent_of = {"per_user": np.zeros(int(data["uid"].max()) - uid0 + 1, np.int64), "per_movie": np.zeros(int(data["uid"].max()) - uid0 + 1, np.int64)}
    ent_of["per_user"][data["uid"] - uid0] = data["user"]
    ent_of["per_movie"][data["uid"] - uid0] = data["movie"]
    prev = "global"
    for s in ("per_user", "per_movie"):
        a, c = got[prev], got[s]
        assert np.array_equal(a["uid"], c["uid"])
        ent = ent_of[s][c["uid"] - uid0]
        before = np.bincount(ent, weights=metrics.poisson_loss_terms(a["score"], a["label"]))
        after = np.bincount(ent, weights=metrics.poisson_loss_terms(c["score"], c["label"]))
        # per entity: the fit minimises loss + (l2/2)|theta|^2 from theta = 0, so the loss alone does not increase. The score file holds the
        # margin rounded to fp32 (relative 2^-24): that moves a sample's loss by at most |exp(s) - y| 2^-24 |s| <= (exp(s) + y) 2^-24 |s|
        s64, y64 = c["score"].astype(np.float64), c["label"].astype(np.float64)
        slack = 2.0 ** -24 * np.bincount(ent, weights=(np.exp(s64) + y64) * np.abs(s64))
        assert np.all(after <= before + slack), (s, float((after - before - slack).max()))
        assert res[s]["train_poisson_loss"] <= res[prev]["train_poisson_loss"]
        prev = s
    # ---- 32 sampled per-user models against scipy
    stage = "per_user"
    tr = np.flatnonzero(data["train"])
    g = got["global"]
    pos = np.searchsorted(g["uid"], data["uid"][tr])
    off_tr = g["score"][pos].astype(np.float32)
    users = np.unique(data["user"][tr])
    pick = np.random.default_rng(7).choice(users, 32, replace=False)
    models = _models(root, stage, chain.D_MOVIE_FEATS, "m")
    worst = 0.0
    for u in pick:
        rows = tr[data["user"][tr] == u]
        ptr, cols, vals, dim = chain.bag_rows(data, stage, rows)
        from gdmix_amd.batch import RawBatch
        be = RawBatch(ent_row_ptr=np.array([0, rows.size]), row_nnz_ptr=ptr, col_global=cols, val=vals, y=data["rating"][rows].astype(np.float32),
                      offset=off_tr[np.searchsorted(tr, rows)], binary_labels=False)
        pke = oracle.pack(be.ent_row_ptr, be.row_nnz_ptr, be.col_global)
        X, y, off, w = P.entity_sparse(be, pke, 0, True)
        x = P.scipy_fit(P.objective(X, y, off, w, P.reg_vector(X.shape[1], 1.0, True, False)), np.zeros(X.shape[1]), 10, 100, 1e-12)[0]
        x = np.where(np.abs(x) <= 1e-4, 0.0, x)
        icpt, coef = models[str(int(u))]
        have = np.concatenate([[icpt], coef[np.asarray(pke["unique_global"])]])
        worst = max(worst, float(np.abs(have - x).max() / max(1.0, np.abs(x).max())))
    print(f"32 per-user models against scipy: worst {worst:.3e}")
    assert worst <= 1e-5, worst
