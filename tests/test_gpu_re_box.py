"""GPU: the random effect's box constraints (REDeviceSolver.solve(bounds=...), gdmix_re_solve_box; include/gdmix_re.h, "box constraints") —
both kernels against the algorithm-independent reference of tests/re_box_helpers.py (scipy's L-BFGS-B with bounds, per entity), held to that
module's bars with its tight tolerances; the routing and its edge; pinned boxes, infinite tables, NULL tables, the clamped start, a
restart, the memory-clear path and status 4, the counts against the numpy restatement, the variances, the refusals, and the stage through
chain.run_stage. The shapes are the smallest at which each kernel can still go wrong; tests/test_re_box_host.py asserts that the
restatement alone keeps every committed case within the bars."""
import ctypes as C
import json
import logging
import os

import numpy as np
import pytest

from gdmix_amd import solver as S
from gdmix_amd.solver import SolverOptions
import fe_box_helpers as FB
import re_box_helpers as B
import re_l1_helpers as R
import re_linear_helpers as H
from test_gpu_re_l1 import _edge_batch, _read_models, _theta_of

pytestmark = pytest.mark.gpu


def _opts(loss, v, m=10, variance_mode=0, **kw):
    t = dict(B.TIGHT, **kw)
    return SolverOptions(l2=B.L2, regularize_bias=v["regularize_bias"], has_intercept=v["has_intercept"], m=m, max_iter=t["max_iter"], maxfun=t["maxfun"],
                         maxls=t["maxls"], ftol=t["ftol"], pgtol=t["pgtol"], variance_mode=variance_mode, loss=loss)


def _solve(solver, b, opts, tables=None, theta0=None, lds_limit=None, out=None):
    """-> (host results, packed, (wavefront kernel's entities, workgroup kernel's))."""
    lower, upper = B.bounds() if tables is None else tables
    packed = solver.pack(b, has_intercept=bool(opts.has_intercept))
    if lds_limit is not None:
        solver.set_wave_lds_limit(lds_limit)
    try:
        res = solver.solve(packed, opts, theta0=theta0, bounds=solver.upload_bounds(lower, upper), out=out).to_host()
        counts = solver.box_counts(packed)
    finally:
        H.reset_routing(solver)
    assert np.array_equal(packed.coef_ptr_host(), R.coef_ptr(b, bool(opts.has_intercept)))      # the tests' local order is the pack's
    return res, packed, counts


def _check(res, pbs, boxes, refs, cp, v, what):
    # 0 or 1; at these tolerances a search may also end at the rounding of F (status 4: the restatement ends so on 1 of the compared
    # entities, tests/test_re_box_host.py). The bars below decide whatever the status is.
    assert np.all((res["status"] == 0) | (res["status"] == 1) | (res["status"] == 4)), np.unique(res["status"])
    assert (res["status"] == 4).sum() <= int(np.ceil(0.01 * res["status"].size)), int((res["status"] == 4).sum())
    assert np.all(np.isfinite(res["theta"]))
    for e, pb in pbs.items():      # gnorm is the projected-gradient norm at the returned point
        th = res["theta"][int(cp[e]):int(cp[e + 1])]
        assert abs(res["gnorm"][e] - FB.projected_gradient_norm(th, pb.smooth(th)[1], *boxes[e])) <= 1e-12, e
    return B.check_batch(pbs, boxes, refs, res["theta"], res["fval"], cp, convexity=v["distance"], what=what)


def _check_theta_thr(res, b, v, tables=None):
    """theta_thr is theta thresholded at 1e-4, except where the box does not contain 0."""
    lo, hi = B.batch_bounds(b, *(B.bounds() if tables is None else tables), v["has_intercept"])
    keeps = (lo > 0.0) | (hi < 0.0)
    want = np.where((np.abs(res["theta"]) <= 1e-4) & ~keeps, 0.0, res["theta"])
    assert np.array_equal(res["theta_thr"], want)
    assert np.all((lo <= res["theta"]) & (res["theta"] <= hi)) and np.all((lo <= res["theta_thr"]) | ~keeps)
    assert keeps.any() and np.array_equal(res["theta"][lo == hi], lo[lo == hi])


# 1 ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", list(B.VARIANTS))
@pytest.mark.parametrize("loss", B.LOSSES)
def test_three_losses_against_the_reference_default_routing(device_solver, loss, variant):
    """The mixed batch (n from 1, an entity without features, p from 1 to more than 64 coefficients) under default routing: every entity
    fits the wavefront kernel. Without and with weights, without an intercept, with an unregularised one (there the convexity bounds are
    no theorems and are skipped)."""
    pbs, boxes, refs, b, v = B.case(loss, variant, "mixed")
    res, packed, counts = _solve(device_solver, b, _opts(loss, v))
    assert counts == (b.E, 0)
    _check(res, pbs, boxes, refs, packed.coef_ptr_host(), v, f"device {loss} {variant}")
    _check_theta_thr(res, b, v)


# 2 ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("loss", B.LOSSES)
def test_every_entity_on_the_workgroup_kernel(device_solver, loss):
    """wave_lds_limit = 0 sends every entity to re_owlqn_block_kernel: the mixed entities, one with more samples and more coefficients than
    the workgroup has threads, and 2 100 tiny ones on 1 024 scratch slots, so that the grid takes a second trip. The sample of
    re_l1_helpers.block_sample is held to the reference; every entity is in its box and its fval is F at its theta."""
    pbs, boxes, refs, b, v = B.case(loss, "plain", "block")
    big = int(np.argmax(b.ent_n()))
    assert b.ent_n()[big] > 256 and big in pbs and refs[big][0].size > 256 and b.E > 2048
    res, packed, counts = _solve(device_solver, b, _opts(loss, v), lds_limit=0)
    assert counts == (0, b.E)
    cp = packed.coef_ptr_host()
    _check(res, pbs, boxes, refs, cp, v, f"device {loss} workgroup kernel")
    _check_theta_thr(res, b, v)
    worst = 0.0
    for e in range(b.E):
        pb = pbs[e] if e in pbs else R.entity_problem(b, e, loss, 0.0, B.L2)
        th = res["theta"][int(cp[e]):int(cp[e + 1])]
        F_np = pb.smooth(th)[0]
        worst = max(worst, abs(res["fval"][e] - F_np) / abs(F_np))
    print(f"{loss}: over all {b.E} entities: worst |fval - F_numpy| / |F| {worst:.3e}")
    assert worst <= 1e-9


def test_a_limit_that_splits_the_batch(device_solver):
    """A wave_lds_limit between the footprints: both kernels run in one call, and every entity meets the bars."""
    pbs, boxes, refs, b, v = B.case("logistic", "weights", "mixed")
    res, packed, counts = _solve(device_solver, b, _opts("logistic", v), lds_limit=8 * 1024)
    print(f"limit 8 KB: {counts[0]} entities on the wavefront kernel, {counts[1]} on the workgroup kernel")
    assert counts[0] > 0 and counts[1] > 0 and sum(counts) == b.E
    _check(res, pbs, boxes, refs, packed.coef_ptr_host(), v, "device logistic, split routing")


# 3 ---------------------------------------------------------------------------------------------------------------------------------------
def test_the_footprint_edge(device_solver):
    """wave_lds_limit = the bounded step's footprint of the first entity; the second is 16 bytes above it. Both are solved within the bars,
    and the counts say which kernel took which."""
    b = _edge_batch()
    v = B.VARIANTS["plain"]
    fp = [B.lds_bytes(p=6, n=4, nnz=z, d=5, m=10, has_w=False) for z in (10, 11)]
    assert fp[1] == fp[0] + 16
    u = np.arange(64) % 5      # ids 3, 9, 20, 41, 57: every kind but pinned
    tables = (np.where(u == 3, 0.0, np.where(u == 4, -0.05, -np.inf)), np.where(u == 4, 0.05, np.where(u == 0, -0.02, np.inf)))
    pbs = R.problems("box edge", b, "logistic", 0.0, B.L2)
    boxes = {e: B.entity_bounds(b, e, *tables) for e in pbs}
    refs = B.references("box edge", pbs, boxes)
    for limit, want in ((fp[0], (1, 1)), (fp[0] - 16, (0, 2)), (fp[1], (2, 0))):
        res, packed, counts = _solve(device_solver, b, _opts("logistic", v), tables=tables, lds_limit=limit)
        assert counts == want, (limit, counts)
        _check(res, pbs, boxes, refs, packed.coef_ptr_host(), v, f"footprint edge, limit {limit}")


# 4 ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lds_limit", [None, 0])
@pytest.mark.parametrize("pin", [0.1, 0.0])
def test_every_feature_pinned_only_the_intercept_moves(device_solver, pin, lds_limit):
    pbs, _, _, b, v = B.case("logistic", "plain", "mixed")
    tables = (np.full(B.D, pin), np.full(B.D, pin))
    boxes = {e: B.entity_bounds(b, e, *tables) for e in pbs}
    refs = B.references(("pinned", pin), pbs, boxes)
    res, packed, _ = _solve(device_solver, b, _opts("logistic", v), tables=tables, lds_limit=lds_limit)
    cp = packed.coef_ptr_host()
    feature = np.ones(int(cp[-1]), bool)
    feature[cp[:-1]] = False
    assert np.all(res["theta"][feature] == pin) and np.all(res["theta"][~feature] != 0.0)
    assert np.all(res["theta_thr"][feature] == pin)
    _check(res, pbs, boxes, refs, cp, v, f"every feature pinned at {pin}")


def test_infinite_tables_reach_the_plain_minimiser(device_solver):
    pbs, _, _, b, v = B.case("poisson", "weights", "mixed")
    tables = (np.full(B.D, -np.inf), np.full(B.D, np.inf))
    boxes = {e: B.entity_bounds(b, e, *tables) for e in pbs}
    refs = B.references("infinite", pbs, boxes)
    for which in (tables, (None, tables[1]), (tables[0], None)):
        res, packed, _ = _solve(device_solver, b, _opts("poisson", v), tables=which)
        _check(res, pbs, boxes, refs, packed.coef_ptr_host(), v, "infinite tables")
    plain = device_solver.solve(packed, _opts("poisson", v)).to_host()
    print(f"bounded solve with infinite tables against the plain solve: max |theta - theta_plain| {np.abs(res['theta'] - plain['theta']).max():.3e}")
    B.check_batch(pbs, boxes, refs, plain["theta"], plain["fval"], packed.coef_ptr_host(), what="the plain solve, same bars")


KEYS = ("theta", "theta_thr", "fval", "nit", "nfev", "status")


def test_no_tables_is_the_plain_solve_bit_for_bit(device_solver):
    s, t = device_solver, device_solver.torch
    _, _, _, b, v = B.case("logistic", "weights", "mixed")
    opts = SolverOptions(l2=B.L2, loss="logistic")
    packed = s.pack(b)
    plain = s.solve(packed, opts).to_host()
    through_python = s.solve(packed, opts, bounds=(None, None)).to_host()
    out = s.alloc_result(packed)
    c_res = S._Result(*[None if out[k] is None else out[k].data_ptr() for k in ("theta", "theta_thr", "variance", "fval", "gnorm", "nit", "nfev", "status")])
    c_opts = opts.to_c()
    assert s.lib.gdmix_re_solve_box(s._h, C.byref(packed.c), C.byref(c_opts), None, None, 0, None, C.byref(c_res), s._stream()) == 0
    t.cuda.synchronize()
    for k in KEYS:
        assert np.array_equal(plain[k].view(np.uint8), through_python[k].view(np.uint8)), k
        assert np.array_equal(plain[k].view(np.uint8), out[k].cpu().numpy().view(np.uint8)), k
    with pytest.raises(S.GdmixReError, match="l1 != 0"):
        s.solve(packed, opts, l1=0.5, bounds=s.upload_bounds(*B.bounds()))


# 5 ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lds_limit", [None, 0])
def test_a_restart_from_the_answer_stops_at_once(device_solver, lds_limit):
    """The answer of a tight solve, handed back as the start point with pgtol 1e-6: nit 0, nfev 1, status 0, the same point."""
    pbs, boxes, refs, b, v = B.case("squared", "plain", "mixed")
    first, packed, _ = _solve(device_solver, b, _opts("squared", v), lds_limit=lds_limit)
    assert first["gnorm"].max() <= 1e-6
    again, _, _ = _solve(device_solver, b, _opts("squared", v, pgtol=1e-6), theta0=first["theta"], lds_limit=lds_limit)
    assert np.all(again["nit"] == 0) and np.all(again["nfev"] == 1) and np.all(again["status"] == 0)
    assert np.array_equal(again["theta"].view(np.uint8), first["theta"].view(np.uint8))
    assert np.array_equal(again["gnorm"].view(np.uint8), first["gnorm"].view(np.uint8))


# 6 ---------------------------------------------------------------------------------------------------------------------------------------
def _compare_counts(res, runs, what):
    excused = [e for e, r in runs.items() if not r[-1] > R.ARMIJO_MARGIN]
    assert len(excused) <= R.MAX_EXCUSED_SHARE * len(runs)
    bad = []
    for e, r in runs.items():
        if e in excused:
            continue
        (status, nit, nfev, Fv) = r[:4]
        got = (int(res["status"][e]), int(res["nit"][e]), int(res["nfev"][e]))
        if got != (status, nit, nfev) or not abs(res["fval"][e] - Fv) <= 1e-9 * abs(Fv):
            bad.append((e, got, (status, nit, nfev), float(res["fval"][e]), Fv))
    print(f"{what}: {len(runs) - len(excused)} entities compared, {len(excused)} excused, {len(bad)} differ")
    assert not bad, bad[:5]


@pytest.mark.parametrize("warm", [False, True])
@pytest.mark.parametrize("loss", B.LOSSES)
def test_one_iteration_counts_as_the_restatement_counts(device_solver, loss, warm):
    """max_iter = 1 from a cold start and from a start point outside the box: (status, nit, nfev) are the restatement's for every entity
    whose restatement kept every Armijo test further than ARMIJO_MARGIN max(|F|, 1) from its edge, and fval agrees to 1e-9: the start
    point was clamped as the statement says."""
    pbs, boxes, refs, b, v = B.case(loss, "plain", "mixed")
    theta0 = np.concatenate([B.warm_start(refs[e][0]) for e in range(b.E)]) if warm else None
    res, _, _ = _solve(device_solver, b, _opts(loss, v, max_iter=1), theta0=theta0)
    _compare_counts(res, B.one_iteration(loss, warm), f"{loss} warm={warm}")


STARTS = {"cold": None, "outside": B.warm_start, "below": lambda th_ref: th_ref - 3.0}


@pytest.mark.parametrize("lds_limit", [None, 0])
@pytest.mark.parametrize("loss,start,takes", [("poisson", "cold", "stopped"), ("squared", "outside", "stopped"), ("poisson", "below", "cleared")])
def test_the_memory_clear_path_and_status_4(device_solver, loss, start, takes, lds_limit):
    """m = 3, maxls = 1, four iterations: a rejected trial with a pair stored clears the memory and searches again along -q (from three
    below the reference, where a count target's first full steps overshoot); one with no pair stored ends the solve with status 4 at the
    clamped start point (the zeros, and a start point outside the box). The restatement of these inputs takes the path that is asked for,
    and the device's counts are the restatement's."""
    pbs, boxes, refs, b, v = B.case(loss, "plain", "mixed")
    kw = dict(m=3, maxls=1, max_iter=4)
    starts = {e: None if STARTS[start] is None else STARTS[start](refs[e][0]) for e in pbs}
    runs = {e: B.counted_run(pb, *boxes[e], starts[e], **kw) for e, pb in pbs.items()}
    stopped = [e for e, r in runs.items() if r[0] == 4 and r[1] == 0]
    cleared = [e for e, r in runs.items() if r[2] - r[1] - 1 > (1 if r[0] == 4 else 0)]      # more rejected trials than a stop at maxls = 1 leaves
    print(f"{loss} from {start}: {len(stopped)} entities end with status 4 at the start point, {len(cleared)} clear the memory")
    assert stopped if takes == "stopped" else cleared
    theta0 = None if STARTS[start] is None else np.concatenate([starts[e] for e in range(b.E)])
    res, packed, _ = _solve(device_solver, b, _opts(loss, v, **kw), theta0=theta0, lds_limit=lds_limit)
    _compare_counts(res, {e: r[:4] + r[5:] for e, r in runs.items()}, f"{loss} from {start}, m = 3, maxls = 1")
    cp = packed.coef_ptr_host()
    for e in stopped:
        if runs[e][-1] > R.ARMIJO_MARGIN:
            first = np.clip(np.zeros(refs[e][0].size) if starts[e] is None else starts[e], *boxes[e])
            assert np.array_equal(res["theta"][int(cp[e]):int(cp[e + 1])], first), e


# 7 ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lds_limit", [None, 0])
@pytest.mark.parametrize("mode", [1, 2])
@pytest.mark.parametrize("loss", B.LOSSES)
def test_variances_of_the_smooth_objective_at_the_returned_theta(device_solver, loss, mode, lds_limit):
    """SIMPLE (inside the kernels) and FULL (gdmix_re_variance_full) against numpy at the device's theta, rtol 1e-7, a coefficient at a
    bound included."""
    pbs, boxes, _, b, v = B.case(loss, "free_intercept", "mixed")
    res, packed, _ = _solve(device_solver, b, _opts(loss, v, variance_mode=mode), lds_limit=lds_limit)
    cp = packed.coef_ptr_host()
    at = 0
    for e, pb in pbs.items():
        s = slice(int(cp[e]), int(cp[e + 1]))
        np.testing.assert_allclose(res["variance"][s], pb.variance(res["theta"][s], mode), rtol=1e-7, err_msg=f"entity {e}")
        at += int(FB.at_bound(res["theta"][s], *boxes[e]).sum())
    assert at > 0


# 8 ---------------------------------------------------------------------------------------------------------------------------------------
def test_refusals_on_the_device_leave_the_results_untouched(device_solver):
    s, t = device_solver, device_solver.torch
    _, _, _, b, v = B.case("logistic", "plain", "mixed")
    opts = _opts("logistic", v)
    lo, hi = (a.copy() for a in B.bounds())
    top = int(b.col_global.max())
    nan_lo, crossed = lo.copy(), lo.copy()
    nan_lo[B.D - 1] = np.nan
    crossed[7], hi[7] = 1.0, 0.5
    for tables, message in (((nan_lo, B.bounds()[1]), "NaN"), ((crossed, hi), "above its upper bound"), ((lo[:top], B.bounds()[1][:top]), "num_features")):
        packed = s.pack(b)
        out = s.alloc_result(packed)
        for k, x in out.items():
            if x is not None:
                x.fill_(-7)
        with pytest.raises(S.GdmixReError, match=message):
            s.solve(packed, opts, bounds=s.upload_bounds(*tables), out=out)
        t.cuda.synchronize()
        assert all(bool((x == -7).all()) for x in out.values() if x is not None), message
    res, _, _ = _solve(s, b, opts, tables=(lo[:top + 1], B.bounds()[1][:top + 1]))      # a table that just covers the largest id is fine
    assert np.all(res["status"] >= 0)


# 9 ---------------------------------------------------------------------------------------------------------------------------------------
STAGE_BAR = 1e-7      # test_gpu_re_l1.STAGE_BAR: at the stage's pgtol 1e-5 a restatement ends up to 1e-7 |F_ref| above the reference


def test_the_stage(tmp_path, caplog):
    """`gdmix --stage=random_effect --entity_coefficient_constraints=FILE` on one partition of 60 entities: every written coefficient lies
    in its box, a coefficient the file leaves out is 0 and its box contains 0, the log line counts the written feature coefficients that equal a bound, F at
    the written model is within STAGE_BAR of the reference, and a run without the flag differs (the parent would have dropped the flag and
    written that model; what the stage writes without the flag is the next test's)."""
    from gdmix_amd import chain
    b = H.small_job_batch(E=60, seed=42, real=False)
    dim = int(b.col_global.max()) + 1
    lower, upper = B.bounds(dim, seed=5)
    records = [dict(name=f"f{j}", term="", **({} if lower[j] == -np.inf else {"lowerBound": float(lower[j])}),
                    **({} if upper[j] == np.inf else {"upperBound": float(upper[j])})) for j in range(dim) if np.isfinite(lower[j]) or np.isfinite(upper[j])]
    roots = {k: str(tmp_path / k) for k in ("plain", "box")}
    for k in roots:
        H.write_job(roots[k], b)
    path = os.path.join(roots["box"], "constraints.json")
    with open(path, "w") as f:
        json.dump(records, f)
    argv = lambda k, extra: [a.replace("--regularize_bias=False", "--regularize_bias=True") for a in H.job_argv(roots[k], "train", model_type="logistic_regression", extra=extra)]
    chain.run_stage(argv("plain", []))
    with caplog.at_level(logging.INFO):
        chain.run_stage(argv("box", [f"--entity_coefficient_constraints={path}"]))
    plain = _read_models(os.path.join(roots["plain"], "models", "part-00000.avro"))
    box = _read_models(os.path.join(roots["box"], "models", "part-00000.avro"))
    assert set(box) == set(plain) == set(b.entity_ids) and box != plain
    pbs = R.problems("box stage", b, "logistic", 0.0, 1.0)
    boxes = {e: B.entity_bounds(b, e, lower, upper) for e in pbs}
    refs = B.references("box stage", pbs, boxes)
    worst, at_bound = -np.inf, 0
    for e, pb in pbs.items():
        th, (lo, hi), (th_ref, f_ref) = _theta_of(box, b, e), boxes[e], refs[e]
        assert np.all((lo <= th) & (th <= hi)), e
        assert np.array_equal(th[lo == hi], lo[lo == hi])
        at_bound += int(FB.at_bound(th, lo, hi)[1:].sum())
        worst = max(worst, (pb.smooth(th)[0] - f_ref) / abs(f_ref))
    print(f"F at the written model at most {worst:.3e} |F_ref| above the reference; {at_bound} coefficients at a bound")
    assert worst <= STAGE_BAR
    lines = [r.getMessage() for r in caplog.records if "equal a bound" in r.getMessage()]
    n_feat = sum(refs[e][0].size - 1 for e in pbs)
    assert len(lines) == 1 and f" {at_bound} of {n_feat} written feature coefficients" in lines[0], lines


GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "re_box_stage_parent")


def _without_sync_marker(path):
    """The bytes of an Avro container file with its sync marker zeroed: a writer draws the 16 bytes at random per file; they stand in the
    header and behind every block, and a file ends with them."""
    with open(path, "rb") as f:
        blob = f.read()
    marker = blob[-16:]
    assert blob.count(marker) >= 2
    return blob.replace(marker, bytes(16))


def test_without_the_flag_the_stage_writes_the_parents_bytes(tmp_path):
    """The stage without the flag on the same partition of 60 entities: the model file and the two score files are byte for byte what the
    commit before the flag wrote for this directory (tests/golden/re_box_stage_parent, recorded from that commit's build on an MI355X),
    the files' random sync markers apart."""
    from gdmix_amd import chain
    root = str(tmp_path / "plain")
    H.write_job(root, H.small_job_batch(E=60, seed=42, real=False))
    chain.run_stage(H.job_argv(root, "train", model_type="logistic_regression"))
    for written, recorded in ((("models", "part-00000.avro"), "model.avro"), (("trainingScores", "partitionId=0", "part-00000-active.avro"), "training_scores.avro"),
                              (("validationScores", "partitionId=0", "part-00000.avro"), "validation_scores.avro")):
        assert _without_sync_marker(os.path.join(root, *written)) == _without_sync_marker(os.path.join(GOLDEN, recorded)), recorded
