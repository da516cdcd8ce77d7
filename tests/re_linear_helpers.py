"""Shared by tests/test_re_linear.py (CPU) and tests/test_gpu_re_linear.py (GPU): the random effect's squared loss
(--model_type=linear_regression; include/gdmix_re.h, `linear` with sum_loss == 0). Test infrastructure: uses oracle/.

    f(theta) = (1/n) (sum_i w_i (y_i - z_i)^2 + (l2/2) |theta_reg|^2),   z = X~ theta + offset

  * ridge_closed_form: the minimiser from numpy in fp64 (normal equations), what the CPU test pins the oracle to;
  * variance_numpy: _compute_variance (binary_logistic_regression.py:144-189) restated with the curvature weight D_i = 2 w_i — the
    oracle's variance is logistic-only and is not used for linear;
  * run_linear_case: the adjudication rule of tests/fuzz_case.py (run_case) restated for linear=True on the same seeded draws with
    real-valued labels; it also reports which entities are strict by the oracle alone;
  * the CPU restatement of the coordinate chain for linear_regression, on functions of tests/chain_oracle.py where they fit.
"""
import numpy as np

from gdmix_amd import synthetic
from gdmix_amd.solver import SolverOptions
from helpers import per_entity_rel_err
from oracle import oracle

ROUTING_DEFAULTS = dict(lds_limit=65536, kernel_mask=7, giant_nnz=16777216, team_nnz=16384, tall_min_n=None, tall_split_n=0, tall_team_n=None, tall_mid_n=0)


def set_routing(solver, **kw):
    """The routing knobs of the C ABI in one call; reset_routing() puts the library's defaults back."""
    r = dict(ROUTING_DEFAULTS, **kw)
    solver.set_wave_lds_limit(r["lds_limit"])
    solver.set_kernel_mask(r["kernel_mask"])
    solver.set_giant_nnz(r["giant_nnz"])
    solver.set_team_nnz(r["team_nnz"])
    solver.set_tall_min_n(solver.TALL_MIN_N_DEFAULT if r["tall_min_n"] is None else r["tall_min_n"])
    solver.set_tall_split_n(r["tall_split_n"])
    solver.set_tall_team_n(solver.TALL_TEAM_N_DEFAULT if r["tall_team_n"] is None else r["tall_team_n"])
    solver.set_tall_mid_n(r["tall_mid_n"])


def reset_routing(solver):
    set_routing(solver)


def entity_dense(batch, pk, e, has_intercept):
    """Entity e as dense fp64 arrays in local index space, intercept first: (X~ [n, p], y, offset, w). Duplicates of a cell are summed,
    as the reference's toarray() does."""
    r0, r1 = int(batch.ent_row_ptr[e]), int(batch.ent_row_ptr[e + 1])
    f0, f1 = int(pk["ent_feat_ptr"][e]), int(pk["ent_feat_ptr"][e + 1])
    uniq = pk["unique_global"][f0:f1]
    ic = 1 if has_intercept else 0
    n, d = r1 - r0, f1 - f0
    X = np.zeros((n, d + ic))
    if ic:
        X[:, 0] = 1.0
    for i in range(n):
        z0, z1 = int(batch.row_nnz_ptr[r0 + i]), int(batch.row_nnz_ptr[r0 + i + 1])
        cols = np.searchsorted(uniq, batch.col_global[z0:z1])
        np.add.at(X[i], ic + cols, batch.val[z0:z1].astype(np.float64))
    w = np.ones(n) if batch.weight is None else batch.weight[r0:r1].astype(np.float64)
    return X, batch.y[r0:r1].astype(np.float64), batch.offset[r0:r1].astype(np.float64), w


def reg_vector(p, l2, has_intercept, regularize_bias):
    r = np.full(p, float(l2))
    if has_intercept and not regularize_bias:
        r[0] = 0.0
    return r


def ridge_closed_form(X, y, off, w, l2, has_intercept, regularize_bias):
    """argmin of f: (2 X~' W X~ + l2 R) theta = 2 X~' W (y - offset), R = diag(regularised)."""
    R = np.diag(reg_vector(X.shape[1], l2, has_intercept, regularize_bias))
    A = 2.0 * (X.T * w) @ X + R
    return np.linalg.solve(A, 2.0 * X.T @ (w * (y - off)))


def variance_numpy(batch, pk, kw, mode):
    """_compute_variance with D_i = 2 w_i for every entity -> [P]. mode 1 SIMPLE: 1 / (sum_i D_i X~_ij^2 + l2 [- l2 for an unregularised
    intercept] + 1e-12); mode 2 FULL: diag((X~' D X~ + (l2 + 1e-12) I [- l2 e0 e0'])^-1). Not divided by n, as in the reference."""
    ic = 1 if kw["has_intercept"] else 0
    cp = pk["ent_feat_ptr"] + np.arange(batch.E + 1) * ic
    out = np.zeros(int(cp[-1]))
    for e in range(batch.E):
        X, _, _, w = entity_dense(batch, pk, e, kw["has_intercept"])
        D = 2.0 * w
        reg = reg_vector(X.shape[1], kw["l2"], kw["has_intercept"], kw["regularize_bias"])
        if mode == 1:
            out[cp[e]:cp[e + 1]] = 1.0 / ((X * X * D[:, None]).sum(0) + reg + 1e-12)
        else:
            H = (X.T * D) @ X + np.diag(reg + 1e-12)
            out[cp[e]:cp[e + 1]] = np.diag(np.linalg.inv(H))
    return out


def make_linear_case(seed):
    """fuzz_case.make_case's draws with real-valued labels (synthetic.with_real_labels: 2 y + N(0, 1))."""
    from fuzz_case import make_case
    shape, b, kw, rng = make_case(seed)
    return shape, synthetic.with_real_labels(b, seed), kw, rng


def oracle_strict(b, pk, o, th0, P):
    """Strict by the oracle alone (fuzz_case.run_case's rule; every entity is well posed: l2 > 0 and a squared loss): reproduced under
    the three start perturbations (same status, same nit, theta to 1e-9), and not a FACTR stop. -> (ref, strict mask, stable mask, sens)."""
    ic = o.has_intercept
    cp = pk["ent_feat_ptr"] + np.arange(b.E + 1) * (1 if ic else 0)
    ref = oracle.solve(pk, b.val, b.y, b.offset, b.weight, o, theta0=th0)
    sens = np.zeros(b.E)
    stable = np.ones(b.E, bool)
    for j, mag in enumerate((1e-15, 1e-14, 1e-13)):
        jig = mag * np.random.default_rng(j + 1).standard_normal(int(P))
        pert = oracle.solve(pk, b.val, b.y, b.offset, b.weight, o, theta0=jig if th0 is None else th0 * (1.0 + jig))
        sj = per_entity_rel_err(pert["theta"], ref["theta"], cp)
        sens = np.maximum(sens, sj)
        stable &= (pert["status"] == ref["status"]) & (pert["nit"] == ref["nit"]) & (sj < 1e-9)
    return ref, stable & (ref["status"] != 1), stable, sens


def judge(b, pk, kw, th0, res, coef_ptr, theta_tol=1e-6):
    """fuzz_case.run_case's comparison and adjudication for linear=True. res: the device's result (host dict).
    -> dict(problems, adjudicated, strict [by the oracle alone], strict_ok [strict and not flagged], err)."""
    okw = dict(kw, variance_mode=0, linear=True, sum_loss=False)
    o = oracle.make_opts(**okw)
    P = int(coef_ptr[-1])
    ref, strict_o, stable, sens = oracle_strict(b, pk, o, th0, P)
    err = per_entity_rel_err(res["theta"], ref["theta"], coef_ptr)
    wp_all = np.ones(b.E, bool)
    wp = wp_all & stable
    same = (res["status"] == ref["status"]) & (res["nit"] == ref["nit"])
    strict = wp & (ref["status"] != 1) & (res["status"] != 1)
    tol = np.where((res["status"] == 1) | (ref["status"] == 1), 1e-6 if kw["ftol"] <= 1e-12 else 1e-3, theta_tol)
    problems, adjudicated = [], []
    if np.any(res["status"] < 0) or np.any(res["status"] > 4):
        problems.append(f"status out of range: {np.unique(res['status'])}")
    flagged = np.zeros(b.E, bool)
    flagged |= strict & ~same
    flagged |= strict & same & (res["nfev"] != ref["nfev"])
    flagged |= wp & (err > tol)
    flagged |= wp_all & ~stable & (err > 1e-6) & (err > 1000.0 * np.maximum(sens, 1e-12))
    tight = []

    def jiggled(j, mag):
        jig = mag * np.random.default_rng(j + 1).standard_normal(P)
        return oracle.solve(pk, b.val, b.y, b.offset, b.weight, o, theta0=jig if th0 is None else th0 * (1.0 + jig))

    def minimum():
        if not tight:
            kt = dict(okw, m=10, max_iter=5000, ftol=1e-15)
            tight.append(oracle.solve(pk, b.val, b.y, b.offset, b.weight, oracle.make_opts(**kt), theta0=th0)["fval"])
        return tight[0]
    if flagged.any():
        wide = [jiggled(10 + j, mag) for j, mag in enumerate((1e-15, 3e-15, 1e-14, 3e-14, 1e-13, 3e-13, 1e-15, 1e-14, 1e-13, 1e-12))]
        for e in np.flatnonzero(flagged):
            ok_status = res["status"][e] in (0, 1, 2) and ref["status"][e] in (0, 1, 2)
            ok_grad = res["status"][e] != 0 or res["gnorm"][e] <= 1e-5
            scale = max(abs(ref["fval"][e]), 1.0)
            ok_f = abs(res["fval"][e] - ref["fval"][e]) <= max(1e-5, 200.0 * kw["ftol"]) * scale
            if not ok_f and res["fval"][e] < ref["fval"][e]:
                ok_f = res["fval"][e] >= minimum()[e] - 1e-6 * scale
            moved = any((w["status"][e] != ref["status"][e]) or (w["nit"][e] != ref["nit"][e]) or (w["nfev"][e] != ref["nfev"][e]) for w in wide)
            spread = max([sens[e]] + [float(per_entity_rel_err(w["theta"], ref["theta"], coef_ptr)[e]) for w in wide])
            margin = min(abs(ref["gnorm"][e] - 1e-5) / 1e-5, abs(res["gnorm"][e] - 1e-5) / 1e-5) if 0 in (res["status"][e], ref["status"][e]) else 1.0
            rounding = moved or margin <= 0.05 or err[e] <= 1000.0 * max(spread, 1e-12) or 1 in (res["status"][e], ref["status"][e])
            what = (f"entity {int(e)} (n={int(b.ent_n()[e])}, p={int(coef_ptr[e + 1] - coef_ptr[e])}): device status {res['status'][e]} nit {res['nit'][e]} nfev "
                    f"{res['nfev'][e]} f {res['fval'][e]:.10g} |g| {res['gnorm'][e]:.3e}; oracle status {ref['status'][e]} nit {ref['nit'][e]} nfev {ref['nfev'][e]} "
                    f"f {ref['fval'][e]:.10g} |g| {ref['gnorm'][e]:.3e}; theta rel err {err[e]:.2e}, oracle's own spread {spread:.2e}, "
                    f"oracle changes under noise: {moved}, stop margin {margin:.3f}")
            if ok_status and ok_grad and ok_f and rounding:
                adjudicated.append(what)
            else:
                problems.append(f"UNEXPLAINED ({'status ' if not ok_status else ''}{'gradient ' if not ok_grad else ''}{'f ' if not ok_f else ''}"
                                f"{'not rounding-level ' if not rounding else ''}): " + what)
    if kw["variance_mode"] in (1, 2):     # theta-independent for the squared loss: every entity is compared
        vr = variance_numpy(b, pk, kw, kw["variance_mode"])
        rtol = 1e-7 if kw["variance_mode"] == 1 else 1e-4
        if not np.allclose(res["variance"], vr, rtol=rtol, atol=0.0):
            k = int(np.argmax(np.abs(res["variance"] - vr) / np.maximum(np.abs(vr), 1e-300)))
            problems.append(f"variance differs (mode {kw['variance_mode']}): {res['variance'][k]:.9e} vs {vr[k]:.9e}")
    return dict(problems=problems, adjudicated=adjudicated, strict=strict_o, strict_ok=strict & ~flagged, ref=ref, err=err, same=same)


def run_linear_case(solver, seed):
    """fuzz_case.run_case for linear=True: the same draws (shape, options, FULL variance, warm start, routing) in the same order, labels
    real-valued. -> dict(seed, shape, E, kw, problems, adjudicated, strict, entities)."""
    shape, b, kw, rng = make_linear_case(seed)
    has_intercept = kw["has_intercept"]
    pk = oracle.pack(b.ent_row_ptr, b.row_nnz_ptr, b.col_global)
    if shape in ("c2", "ragged", "ml", "tiny") and np.diff(pk["ent_feat_ptr"]).max() < 300 and rng.random() < 0.3:
        kw["variance_mode"] = 2
    packed = solver.pack(b, has_intercept=has_intercept)
    th0 = None
    if rng.random() < 0.3:
        th0 = 0.1 * rng.standard_normal(int(packed.P))
    routing = dict(giant=int(rng.choice([16777216, 16777216, 200000, 1])), team=int(rng.choice([16384, 16384, 2048, 256])),
                   mask=int(rng.choice([7, 7, 1])), tall=int(rng.choice([32, 32, 1, 0])))
    routing["tall_team"] = int(np.random.default_rng(seed ^ 0x7A11).choice([8192, 8192, -64, 0]))
    routing["tall_mid"] = int(np.random.default_rng(seed ^ 0x3D1D).choice([0, 0, 16]))
    set_routing(solver, giant_nnz=routing["giant"], team_nnz=routing["team"], kernel_mask=2 if routing["mask"] == 1 else routing["mask"],
                tall_min_n=routing["tall"], tall_team_n=routing["tall_team"], tall_split_n=64 if routing["tall_team"] < 0 else 0,
                tall_mid_n=routing["tall_mid"])
    try:
        res = solver.solve(packed, SolverOptions(linear=True, **kw), theta0=th0).to_host()
    finally:
        reset_routing(solver)
    problems = []
    if not np.array_equal(packed.unique_global().cpu().numpy(), pk["unique_global"]):
        problems.append("pack: unique_global differs")
    j = judge(b, pk, kw, th0, res, packed.coef_ptr_host())
    return dict(seed=seed, shape=shape, E=b.E, kw=kw, routing=routing, warm=th0 is not None, problems=problems + j["problems"],
                adjudicated=j["adjudicated"], strict=int(j["strict"].sum()), entities=int(b.E))




# ---- one random-effect job on disk, as gdmix-workflow would hand it to `python -m gdmix_amd.gdmix` -----------------------------------
def write_job(root, train, valid=None, bag="per_user", entity="user_id", dim=None, partition=0):
    """train / valid: RawBatch with integer entity ids and uids -> the partition directories, metadata, feature list and partition list of
    one random-effect stage under `root`. Labels are written as they are: a float list when the batch has binary_labels=False."""
    import json
    import os
    from gdmix_amd import partitioner
    dim = int(train.col_global.max()) + 1 if dim is None else dim
    p = os.path.join(root, "partition")
    partitioner.write_partitions(os.path.join(p, "trainingData"), {("active", partition): train}, entity, bag, int_entity_ids=True, weight_column_name=None)
    partitioner.write_partitions(os.path.join(p, "validationData"), {("", partition): train if valid is None else valid}, entity, bag, int_entity_ids=True,
                                 weight_column_name=None)
    md = {"features": [{"name": bag, "dtype": "float", "shape": [dim], "isSparse": True},
                       {"name": "offset", "dtype": "float", "shape": [], "isSparse": False},
                       {"name": "uid", "dtype": "long", "shape": [], "isSparse": False},
                       {"name": entity, "dtype": "long", "shape": [], "isSparse": False}],
          "labels": [{"name": "response", "dtype": "float", "shape": [], "isSparse": False}]}
    os.makedirs(os.path.join(p, "metadata"), exist_ok=True)
    with open(os.path.join(p, "metadata", "tensor_metadata.json"), "w") as f:
        json.dump(md, f)
    with open(os.path.join(p, "partitionList.txt"), "w") as f:
        f.write(str(partition))
    with open(os.path.join(p, "featureList"), "w") as f:
        f.write("".join(f"f{i},\n" for i in range(dim)))
    return p


def job_argv(root, action="train", model_type="linear_regression", bag="per_user", entity="user_id", extra=()):
    import os
    p = os.path.join(root, "partition")
    argv = ["gdmix", "--stage=random_effect", f"--action={action}", f"--model_type={model_type}", f"--partition_list_file={p}/partitionList.txt",
            f"--metadata_file={p}/metadata/tensor_metadata.json", f"--feature_file={p}/featureList", f"--feature_bag={bag}", f"--partition_entity={entity}",
            f"--output_model_dir={root}/models", "--uid_column_name=uid", "--label_column_name=response", "--prediction_score_column_name=predictionScore",
            "--l2_reg_weight=1.0", "--regularize_bias=False", "--lbfgs_tolerance=1.0e-12", "--num_of_lbfgs_iterations=100", "--num_of_lbfgs_curvature_pairs=10",
            "--enable_local_indexing=False", "--num_of_consumers=1", "--max_training_queue_size=10"]
    if action == "train":
        argv += [f"--training_data_dir={p}/trainingData", f"--validation_data_dir={p}/validationData", f"--training_score_dir={root}/trainingScores",
                 f"--validation_score_dir={root}/validationScores"]
    else:
        argv += [f"--validation_data_dir={p}/validationData", f"--validation_score_dir={root}/inferenceScores"]
    return argv + list(extra)


def small_job_batch(E=60, seed=11, real=True):
    """A small per-user partition: integer entity ids, uids, offsets, no weights; real-valued labels unless real=False."""
    import dataclasses
    b = synthetic.make_batch(E, 12, 4, 64, seed=seed, with_uid=True)
    b = dataclasses.replace(b, entity_ids=[str(100 + i) for i in range(E)], uid=np.arange(b.N, dtype=np.int64) + 5000)
    return synthetic.with_real_labels(b, seed) if real else b


# ---- the coordinate chain on the CPU, linear_regression ------------------------------------------------------------------------------
def chain_global_linear(data):
    """chain_oracle.global_stage with the squared loss on the ratings (the fixed effect's objective: sum_loss, not divided by n)."""
    import chain_oracle
    from gdmix_amd import chain
    from gdmix_amd import fixed_effect as fe
    tr = np.flatnonzero(data["train"])
    ptr, cols, vals, dim = chain.bag_rows(data, "global", tr)
    batch, dummy = fe.shard_as_batch(ptr, cols, vals, data["rating"][tr].astype(np.float32), None, None, True, binary_labels=False)
    pk = oracle.pack(batch.ent_row_ptr, batch.row_nnz_ptr, batch.col_global)
    o = oracle.make_opts(l2=1.0, regularize_bias=False, has_intercept=True, m=10, max_iter=100, threshold=0.0, sum_loss=True, linear=True)
    res = oracle.solve(pk, batch.val, batch.y, batch.offset, batch.weight, o)
    return chain_oracle._threshold(fe.to_global(res["theta"], pk["unique_global"], dim, True, dummy))


def chain_re_stage_linear(data, stage, prev):
    """chain_oracle.random_effect_stage restated for linear_regression (no upper bound): labels are the ratings, the oracle runs with
    linear=True, every entity is well posed. prev: the previous stage's {"train": {uid, score}, "validation": {...}}."""
    import chain_oracle
    from gdmix_amd import chain
    ent_all = data["user"] if stage == "per_user" else data["movie"]
    dim = data["bags"][stage][3]

    def offsets(rows, prev_s):
        order = np.argsort(prev_s["uid"], kind="stable")
        pos = np.searchsorted(prev_s["uid"][order], data["uid"][rows])
        return prev_s["score"][order][pos].astype(np.float32)
    tr = np.flatnonzero(data["train"])
    off_tr = offsets(tr, prev["train"])
    grp = np.argsort(ent_all[tr], kind="stable")
    rows = tr[grp]
    ents, counts = np.unique(ent_all[rows], return_counts=True)
    ent_row_ptr = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    ptr, cols, vals, _ = chain.bag_rows(data, stage, rows)
    y = data["rating"][rows].astype(np.float32)
    pk = oracle.pack(ent_row_ptr, ptr, cols)
    o = oracle.make_opts(l2=1.0, regularize_bias=False, has_intercept=True, m=10, max_iter=100, threshold=chain_oracle.THRESHOLD, linear=True)
    res = oracle.solve(pk, vals, y, off_tr[grp], None, o)
    E = ents.size
    icpt, coef, fp = np.zeros(E), np.zeros((E, dim)), pk["ent_feat_ptr"]
    for e in range(E):
        base = fp[e] + e
        icpt[e] = res["theta_thr"][base]
        coef[e, pk["unique_global"][fp[e]:fp[e + 1]]] = res["theta_thr"][base + 1:base + 1 + fp[e + 1] - fp[e]]
    out = {"entities": ents, "intercept": icpt, "coef": coef, "well_posed": np.ones(E, bool), "status": res["status"]}
    for name, mask, prev_s in (("train", data["train"], prev["train"]), ("validation", ~data["train"], prev["validation"])):
        r = np.flatnonzero(mask)
        offs = offsets(r, prev_s)
        p, c, v, _ = chain.bag_rows(data, stage, r)
        e_idx = np.searchsorted(ents, ent_all[r])
        has = (e_idx < E) & (ents[np.minimum(e_idx, E - 1)] == ent_all[r])
        e_idx = np.where(has, e_idx, 0)
        e_rows, h_rows = np.repeat(e_idx, np.diff(p)), np.repeat(has, np.diff(p))
        score, per = chain_oracle._dense_scores(p, c, v, np.where(h_rows, coef[e_rows, c], 0.0), np.where(has, icpt[e_idx], 0.0), offs)
        out[name] = {"uid": data["uid"][r], "score": score, "per_coord": per, "offset": offs}
    return out
