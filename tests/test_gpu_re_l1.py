"""GPU: the random effect's elastic net (REDeviceSolver.solve(l1=...), gdmix_re_solve_l1; include/gdmix_re.h, "elastic net") — both kernels
against the algorithm-independent reference of tests/re_l1_helpers.py (scipy's bounded L-BFGS-B on the split problem, per entity), held to
that module's bars with its tight tolerances; the routing and its edge; the ring, the all-zero solution, one iteration against the numpy
restatement, l1 = 0, determinism, the variances, and the stage through chain.run_stage. The shapes are the smallest at which each kernel
can still go wrong; tests/test_re_l1_host.py asserts that the restatement alone keeps every committed case within the bars."""
import ctypes as C
import dataclasses
import os

import numpy as np
import pytest

from gdmix_amd import solver as S
from gdmix_amd.batch import RawBatch
from gdmix_amd.solver import SolverOptions
import re_l1_helpers as R
import re_linear_helpers as H

pytestmark = pytest.mark.gpu


def _opts(loss, v, m=10, variance_mode=0, **kw):
    t = dict(R.TIGHT, **kw)
    return SolverOptions(l2=R.L2, regularize_bias=v["regularize_bias"], has_intercept=v["has_intercept"], m=m, max_iter=t["max_iter"], maxfun=t["maxfun"],
                         maxls=t["maxls"], ftol=t["ftol"], pgtol=t["pgtol"], variance_mode=variance_mode, loss=loss)


def _solve(solver, b, opts, l1=R.L1, theta0=None, lds_limit=None):
    """-> (host results, packed, (wavefront kernel's entities, workgroup kernel's))."""
    packed = solver.pack(b, has_intercept=bool(opts.has_intercept))
    if lds_limit is not None:
        solver.set_wave_lds_limit(lds_limit)
    try:
        res = solver.solve(packed, opts, theta0=theta0, l1=l1).to_host()
        counts = solver.l1_counts(packed) if l1 else None
    finally:
        H.reset_routing(solver)
    assert np.array_equal(packed.coef_ptr_host(), R.coef_ptr(b, bool(opts.has_intercept)))      # the tests' local order is the pack's
    return res, packed, counts


def _check(res, pbs, refs, cp, v, what):
    # 0 or 1; at these tolerances a search may also end at the rounding of F (status 4: the numpy restatement ends so on 12 of the block
    # batches' 6 375 entities, tests/test_re_l1_host.py has none among the compared ones). The bars below decide whatever the status is.
    assert np.all((res["status"] == 0) | (res["status"] == 1) | (res["status"] == 4)), np.unique(res["status"])
    assert (res["status"] == 4).sum() <= int(np.ceil(0.01 * res["status"].size)), int((res["status"] == 4).sum())
    assert np.all(np.isfinite(res["theta"]))
    for e, pb in pbs.items():      # gnorm is |pg|_inf at the returned point
        assert abs(res["gnorm"][e] - np.max(np.abs(pb.pseudo_gradient(res["theta"][int(cp[e]):int(cp[e + 1])])), initial=0.0)) <= 1e-12, e
    return R.check_batch(pbs, refs, res["theta"], res["fval"], cp, distance=v["distance"], what=what)


# 1 ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", list(R.VARIANTS))
@pytest.mark.parametrize("loss", R.LOSSES)
def test_three_losses_against_the_reference_default_routing(device_solver, loss, variant):
    """The mixed batch (n from 1, p from 1 to more than 64 coefficients) under default routing: every entity fits the wavefront kernel.
    Without and with weights, without an intercept, with an unregularised one (there the distance bound is no theorem and is skipped)."""
    pbs, refs, b, v = R.case(loss, variant, "mixed")
    res, packed, counts = _solve(device_solver, b, _opts(loss, v))
    assert counts == (b.E, 0)
    _check(res, pbs, refs, packed.coef_ptr_host(), v, f"device {loss} {variant}")
    thr = np.where(np.abs(res["theta"]) <= 1e-4, 0.0, res["theta"])
    assert np.array_equal(res["theta_thr"], thr)


# 2 ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("loss", R.LOSSES)
def test_every_entity_on_the_workgroup_kernel(device_solver, loss):
    """wave_lds_limit = 0 sends every entity to re_owlqn_block_kernel: the mixed entities, one with more samples and more coefficients than
    the workgroup has threads, and 2 100 tiny ones, more than the grid has workgroups, so that scratch slots are reused. The sample of
    re_l1_helpers.block_sample is held to the reference; every entity's fval is F at its theta, and its optimality gap is certified."""
    pbs, refs, b, v = R.case(loss, "plain", "block")
    big = int(np.argmax(b.ent_n()))
    assert b.ent_n()[big] > 256 and big in pbs and refs[big][0].size > 256 and b.E > 2048
    res, packed, counts = _solve(device_solver, b, _opts(loss, v), lds_limit=0)
    assert counts == (0, b.E)
    cp = packed.coef_ptr_host()
    _check(res, pbs, refs, cp, v, f"device {loss} workgroup kernel")
    # every entity, the reference apart: fval is F at theta, and theta is certified: F is strongly convex with modulus mu = l2 / n, so
    # F(theta) - min F <= |pg(theta)|^2 / (2 mu) for any theta; that gap is held to the bar of the reference comparison, 1e-9 |F|
    worst = gap = 0.0
    for e in range(b.E):
        pb = pbs[e] if e in pbs else R.entity_problem(b, e, loss, R.L1, R.L2)
        th = res["theta"][int(cp[e]):int(cp[e + 1])]
        F_np, pg = pb.F(th), pb.pseudo_gradient(th)
        worst = max(worst, abs(res["fval"][e] - F_np) / abs(F_np))
        gap = max(gap, (pg @ pg) / (2.0 * pb.l2) / abs(F_np))
    print(f"{loss}: over all {b.E} entities: worst |fval - F_numpy| / |F| {worst:.3e}, worst certified gap / |F| {gap:.3e}")
    assert worst <= 1e-9 and gap <= 1e-9


# 3 ---------------------------------------------------------------------------------------------------------------------------------------
def _edge_batch():
    """Two entities that differ by one non-zero (a cell of a column the entity already has): 16 bytes of LDS."""
    rng = np.random.default_rng(77)
    rows = [[3, 9, 20], [9, 41], [3, 20, 41, 57], [57]]
    cols_a = np.concatenate(rows)
    cols_b = np.concatenate(rows[:-1] + [[57, 3]])
    k_a, k_b = [len(r) for r in rows], [len(r) for r in rows[:-1]] + [2]
    val = (0.7 * rng.standard_normal(cols_a.size + cols_b.size)).astype(np.float32)
    y = np.array([1, 0, 1, 0, 0, 1, 1, 0], np.float32)
    return RawBatch(ent_row_ptr=np.array([0, 4, 8]), row_nnz_ptr=np.concatenate([[0], np.cumsum(k_a + k_b)]), col_global=np.concatenate([cols_a, cols_b]),
                    val=val, y=y, offset=(0.2 * rng.standard_normal(8)).astype(np.float32))


def test_the_footprint_edge(device_solver):
    """wave_lds_limit = the OWL-QN footprint of the first entity; the second is 16 bytes above it. Both are solved within the bars, and
    the counts say that each kernel took one."""
    b = _edge_batch()
    v = R.VARIANTS["plain"]
    fp = [R.lds_bytes(p=6, n=4, nnz=z, d=5, m=10, has_w=False) for z in (10, 11)]
    assert fp[1] == fp[0] + 16
    pbs = R.problems("edge", b, "logistic", R.L1, R.L2)
    refs = R.references("edge", pbs)
    for limit, want in ((fp[0], (1, 1)), (fp[0] - 16, (0, 2)), (fp[1], (2, 0))):
        res, packed, counts = _solve(device_solver, b, _opts("logistic", v), lds_limit=limit)
        assert counts == want, (limit, counts)
        _check(res, pbs, refs, packed.coef_ptr_host(), v, f"footprint edge, limit {limit}")


# 4 ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lds_limit", [None, 0])
def test_the_history_ring_wraps(device_solver, lds_limit):
    pbs, refs, b, v = R.case("poisson", "plain", "mixed")
    res, packed, _ = _solve(device_solver, b, _opts("poisson", v, m=3), lds_limit=lds_limit)
    print(f"m = 3: nit up to {int(res['nit'].max())}, {int((res['nit'] > 3).sum())} entities past the ring's length")
    assert res["nit"].max() > 3
    _check(res, pbs, refs, packed.coef_ptr_host(), v, "device poisson m = 3")


# 5 ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lds_limit", [None, 0])
@pytest.mark.parametrize("loss", R.LOSSES)
def test_the_all_zero_solution(device_solver, loss, lds_limit):
    """l1 above n |g(0)|_inf of every entity (every coefficient regularised): the start point is the solution."""
    pbs, _, b, v = R.case(loss, "weights", "mixed")
    l1 = 1.01 * max(pb.n * np.max(np.abs(pb.data(np.zeros(pb.X.shape[1]))[1])) for pb in pbs.values())
    res, packed, _ = _solve(device_solver, b, _opts(loss, v), l1=l1, lds_limit=lds_limit)
    assert np.all(res["status"] == 0) and np.all(res["nit"] == 0) and np.all(res["nfev"] == 1)
    assert np.all(res["theta"] == 0.0) and np.all(res["gnorm"] == 0.0)
    cp = packed.coef_ptr_host()
    for e, pb in pbs.items():
        F0 = pb.data(np.zeros(pb.X.shape[1]))[0]
        assert abs(res["fval"][e] - F0) <= 1e-12 * abs(F0), (e, res["fval"][e], F0)


# 6 ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("warm", [False, True])
@pytest.mark.parametrize("loss", R.LOSSES)
def test_one_iteration_counts_as_the_restatement_counts(device_solver, loss, warm):
    """max_iter = 1 from a cold start and from half the reference: (status, nit, nfev) are the restatement's for every entity whose
    restatement kept every Armijo test further than 1e-10 max(|F|, 1) from its edge (at most 1 % are excused: tests/test_re_l1_host.py),
    and fval agrees to 1e-9: the start point was honoured."""
    pbs, refs, b, v = R.case(loss, "plain", "mixed")
    one = R.one_iteration(loss, warm)
    cp = R.coef_ptr(b, True)
    theta0 = np.concatenate([0.5 * refs[e][0] for e in range(b.E)]) if warm else None
    res, packed, _ = _solve(device_solver, b, _opts(loss, v, max_iter=1), theta0=theta0)
    excused = [e for e, r in one.items() if not r[4] > R.ARMIJO_MARGIN]
    assert len(excused) <= R.MAX_EXCUSED_SHARE * len(one)
    bad = []
    for e, (status, nit, nfev, Fv, _) in one.items():
        if e in excused:
            continue
        got = (int(res["status"][e]), int(res["nit"][e]), int(res["nfev"][e]))
        if got != (status, nit, nfev) or not abs(res["fval"][e] - Fv) <= 1e-9 * abs(Fv):
            bad.append((e, got, (status, nit, nfev), float(res["fval"][e]), Fv))
    print(f"{loss} warm={warm}: {len(one) - len(excused)} entities compared, {len(excused)} excused, {len(bad)} differ")
    assert not bad, bad[:5]


# 7 ---------------------------------------------------------------------------------------------------------------------------------------
KEYS = ("theta", "theta_thr", "fval", "nit", "nfev", "status")


def test_l1_zero_is_the_plain_solve_bit_for_bit(device_solver):
    s, t = device_solver, device_solver.torch
    _, _, b, v = R.case("logistic", "weights", "mixed")
    opts = SolverOptions(l2=R.L2, loss="logistic")
    packed = s.pack(b)
    plain = s.solve(packed, opts).to_host()
    through_python = s.solve(packed, opts, l1=0.0).to_host()
    out = s.alloc_result(packed)
    c_res = S._Result(*[None if out[k] is None else out[k].data_ptr() for k in ("theta", "theta_thr", "variance", "fval", "gnorm", "nit", "nfev", "status")])
    c_opts = opts.to_c()
    assert s.lib.gdmix_re_solve_l1(s._h, C.byref(packed.c), C.byref(c_opts), 0.0, None, C.byref(c_res), s._stream()) == 0
    t.cuda.synchronize()
    for k in KEYS:
        assert np.array_equal(plain[k].view(np.uint8), through_python[k].view(np.uint8)), k
        assert np.array_equal(plain[k].view(np.uint8), out[k].cpu().numpy().view(np.uint8)), k
    with pytest.raises(S.GdmixReError, match="l1 must be finite"):
        s.solve(packed, opts, l1=-1.0)


# 8 ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lds_limit", [None, 0])
def test_the_same_bits_from_run_to_run_and_wherever_the_entity_sits(device_solver, lds_limit):
    _, _, b, v = R.case("logistic", "weights", "mixed")
    opts = _opts("logistic", v)
    first, packed, _ = _solve(device_solver, b, opts, lds_limit=lds_limit)
    again, _, _ = _solve(device_solver, b, opts, lds_limit=lds_limit)
    for k in KEYS + ("gnorm",):
        assert np.array_equal(first[k].view(np.uint8), again[k].view(np.uint8)), k
    perm = np.random.default_rng(3).permutation(b.E)
    moved, packed_m, _ = _solve(device_solver, b.select(perm), opts, lds_limit=lds_limit)
    cp, cpm = packed.coef_ptr_host(), packed_m.coef_ptr_host()
    for k in ("fval", "gnorm", "nit", "nfev", "status"):
        assert np.array_equal(moved[k].view(np.uint8), first[k][perm].view(np.uint8)), k
    for at, e in enumerate(perm):
        for k in ("theta", "theta_thr"):
            assert np.array_equal(moved[k][cpm[at]:cpm[at + 1]].view(np.uint8), first[k][cp[e]:cp[e + 1]].view(np.uint8)), (k, e)


# 9 ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lds_limit", [None, 0])
@pytest.mark.parametrize("mode", [1, 2])
@pytest.mark.parametrize("loss", R.LOSSES)
def test_variances_of_the_smooth_part_at_the_returned_theta(device_solver, loss, mode, lds_limit):
    """SIMPLE (inside the kernels) and FULL (gdmix_re_variance_full with the same l2) against numpy at the device's theta, rtol 1e-7, a
    coefficient at exactly 0 included."""
    pbs, _, b, v = R.case(loss, "free_intercept", "mixed")
    res, packed, _ = _solve(device_solver, b, _opts(loss, v, variance_mode=mode), lds_limit=lds_limit)
    cp = packed.coef_ptr_host()
    zeros = 0
    for e, pb in pbs.items():
        s = slice(int(cp[e]), int(cp[e + 1]))
        want = pb.variance(res["theta"][s], mode)
        np.testing.assert_allclose(res["variance"][s], want, rtol=1e-7, err_msg=f"entity {e}")
        zeros += int((res["theta"][s] == 0.0).sum())
    assert zeros > 0


# 10 --------------------------------------------------------------------------------------------------------------------------------------
def _read_models(path):
    from gdmix_amd.io import avro
    return {r["modelId"]: {(m["name"], m["term"]): m["value"] for m in r["means"]} for r in avro.read_file(path)}


def _argv(root, action, extra):
    argv = H.job_argv(root, action, model_type="logistic_regression", extra=extra)
    return [a.replace("--regularize_bias=False", "--regularize_bias=True") for a in argv]


def _theta_of(models, b, e):
    """The written model of entity e in the tests' local order (intercept first); a coefficient that is not in the file is 0."""
    r0, r1 = int(b.ent_row_ptr[e]), int(b.ent_row_ptr[e + 1])
    uniq = np.unique(b.col_global[int(b.row_nnz_ptr[r0]):int(b.row_nnz_ptr[r1])])
    got = models[b.entity_ids[e]]
    assert set(got) <= {("(INTERCEPT)", "")} | {(f"f{int(g)}", "") for g in uniq}
    return np.array([got.get(("(INTERCEPT)", ""), 0.0)] + [got.get((f"f{int(g)}", ""), 0.0) for g in uniq])


STAGE_BAR = 1e-7      # at the stage's pgtol 1e-5 the numpy restatement itself ends up to 1e-7 |F_ref| above the reference (the tight bars are 1e-9)


def test_the_stage(tmp_path):
    """`gdmix --stage=random_effect --elastic_net_alpha=0.5` on one partition of 60 entities, next to the plain run of the same data: the
    model file holds no feature at zero and fewer coefficients than the plain run's; the scores are x . theta + offset of the written
    model to 1 ulp of the Avro float; a second run starts from the written model and, like the first, has the reference's support outside
    the left-out set (a coefficient below the stage's sparsity threshold is one of them), lies within the distance bound, and F at the
    written model is within STAGE_BAR of the reference; inference with the flag scores as without it."""
    from gdmix_amd import chain
    from test_gpu_chain import _scores_by_uid, _ulps
    b = H.small_job_batch(E=60, seed=42, real=False)
    roots = {k: str(tmp_path / k) for k in ("plain", "net")}
    for k, extra in (("plain", []), ("net", ["--elastic_net_alpha=0.5"])):
        H.write_job(roots[k], b)
        chain.run_stage(_argv(roots[k], "train", extra))
    path = os.path.join(roots["net"], "models", "part-00000.avro")
    plain, net = _read_models(os.path.join(roots["plain"], "models", "part-00000.avro")), _read_models(path)
    assert set(net) == set(plain) == set(b.entity_ids)
    count = lambda models: sum(len(m) for m in models.values())
    icpt = ("(INTERCEPT)", "")

    def no_zero_feature(models):
        """No feature at 0 is in the file. The intercept is the first entry of every record, whatever its value: the format's rule (a
        reader takes the first entry for it), so a regularised intercept that the L1 term set to 0 is written as 0."""
        assert all(icpt in m for m in models.values())
        assert all(v != 0.0 for m in models.values() for k, v in m.items() if k != icpt)

    print(f"coefficients in the model file: plain {count(plain)}, elastic net {count(net)}")
    assert count(net) < count(plain)
    no_zero_feature(net)
    l1, l2 = 0.5, 0.5      # alpha 0.5 of --l2_reg_weight=1.0
    pbs = R.problems("stage", b, "logistic", l1, l2)
    refs = R.references("stage", pbs)
    R.check_left_out_cap(pbs, refs)
    order = np.argsort(b.uid, kind="stable")

    def check_model(models, what):
        worst = -np.inf
        for e, pb in pbs.items():
            th, (th_ref, f_ref) = _theta_of(models, b, e), refs[e]
            lo = R.left_out(pb, th_ref)
            mism = np.flatnonzero(((th != 0) != (th_ref != 0)) & ~lo)
            assert mism.size == 0, (what, e, th[mism], th_ref[mism])
            dist = np.linalg.norm(th - th_ref)
            assert dist <= R.distance_bound(pb, th, th_ref), (what, e)
            worst = max(worst, (pb.F(th) - f_ref) / abs(f_ref))
        print(f"{what}: F at the written model at most {worst:.3e} |F_ref| above the reference")
        assert worst <= STAGE_BAR

    def check_scores(models, d, what):
        z = np.concatenate([pbs[e].X @ _theta_of(models, b, e) + pbs[e].off for e in range(b.E)]).astype(np.float32)
        s = _scores_by_uid(d)
        assert np.array_equal(s["uid"], b.uid[order]) and _ulps(s["score"], z[order]).max() <= 1.0, what

    check_model(net, "first run")
    for d in ("trainingScores", "validationScores"):
        check_scores(net, os.path.join(roots["net"], d), d)
    chain.run_stage(_argv(roots["net"], "train", ["--elastic_net_alpha=0.5"]))      # the model of the first run is in output_model_dir: a warm start
    again = _read_models(path)
    no_zero_feature(again)
    check_model(again, "second run, warm")
    chain.run_stage(_argv(roots["net"], "inference", ["--elastic_net_alpha=0.5"]))
    with_flag = _scores_by_uid(os.path.join(roots["net"], "inferenceScores"))
    check_scores(again, os.path.join(roots["net"], "inferenceScores"), "inference")
    chain.run_stage(_argv(roots["net"], "inference", []))
    without = _scores_by_uid(os.path.join(roots["net"], "inferenceScores"))
    assert np.array_equal(with_flag["uid"], without["uid"]) and np.array_equal(with_flag["score"].view(np.uint32), without["score"].view(np.uint32))
