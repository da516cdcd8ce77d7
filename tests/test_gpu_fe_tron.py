"""GPU: the fixed effect's trust-region Newton optimiser on the device (fit_stepping(optimizer="TRON"); include/gdmix_fe.h, "(ABI 24) TRON";
csrc/fe_tron.hip and the HV variant of the row kernels in csrc/fe_solve.hip). The product alone against numpy through every form of the
copies; fits against a reference that does not share the algorithm (scipy's L-BFGS-B at tight tolerances; tests/fe_tron_helpers.py, which
also states the bars) and, where the trajectory is short enough to be the same to the count, against the numpy restatement of the header;
a rejected trial, the stops, the default left bit for bit, the refusals, two workers, variances, the sweep and the command line."""
import json
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

from gdmix_amd import chain
from gdmix_amd import fixed_effect as fe
import fe_l1_helpers as L1
import fe_tron_helpers as H

HERE = os.path.dirname(os.path.abspath(__file__))


def fit(s, loss, size, **kw):
    rp, col, val, y, off, D, l2 = H.case(loss, size)
    args = dict(H.FIT, offset=off, model_type=H.MODEL_TYPE[loss], l2=l2, optimizer="TRON")
    args.update(kw)
    return s.fit_stepping(rp, col, val, y, D, **args)


def options(loss, l2, **kw):
    f = dict(H.FIT, **kw)
    return fe.fit_options(f["has_intercept"], l2, f["regularize_bias"], H.MODEL_TYPE[loss], f["max_iter"], f["m"], f["tolerance"])


def bits(theta, info):
    return np.asarray(theta, np.float64).tobytes(), float(info["fval"]).hex(), int(info["nit"]), int(info["nfev"]), int(info["status"])


def solve_bits(prob, lookahead=None):
    status, _ = prob.solve() if lookahead is None else prob.solve(lookahead=lookahead)
    theta, info = prob.result()
    return bits(theta, dict(info, status=status)) + (prob.products(),)


def counts(info):
    return int(info["status"]), int(info["nit"]), int(info["nfev"]), int(info["nhv"])


# ---- 1: the product alone ---------------------------------------------------------------------------------------------------------------
FORMS = {"default": {}, "three arrays": {"GDMIX_FE_PACK": "0"}, "6-byte form": {"GDMIX_FE_COMPRESS": "3"}, "several units": {"GDMIX_FE_CHUNK": "64"},
         "frequent columns": {"GDMIX_FE_HOT_MIN": "64"}}


def product_case(device_solver, monkeypatch, loss, env, weighted=False, has_intercept=True):
    """hessian_vec at a non-zero theta against hv(), on an L-BFGS-B problem and on a TRON problem; then each solves to the bits of a problem
    that never saw the call."""
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    t = device_solver.torch
    rp, col, val, y, off, D, l2 = H.case(loss, "wide")
    rng = np.random.default_rng(5)
    P = D + (1 if has_intercept else 0)
    weight = (0.5 + rng.random(y.size)).astype(np.float32) if weighted else None
    theta, v = 0.3 * rng.standard_normal(P), rng.standard_normal(P)
    assert not has_intercept or v[-1] != 0.0
    pb = L1.Problem(loss, L1.design(rp, col, val, D, has_intercept=has_intercept), y, off, 0.0, l2)
    want = H.hv(pb, theta, v, weight)
    opts = options(loss, l2, has_intercept=has_intercept, regularize_bias=has_intercept, max_iter=12)
    up = lambda a: t.from_numpy(np.ascontiguousarray(a, np.float64)).to(device_solver.device)

    def new_problem(optimizer):
        f = fe._SteppingFit(device_solver, opts, rp, col, val, y, D, off, weight, None, None, None, None)
        if optimizer == "TRON":
            f.prob.set_optimizer("TRON")
        return f
    for optimizer in ("LBFGS", "TRON"):
        a, b = new_problem(optimizer), new_problem(optimizer)
        try:
            a.prob.hessian_vec(up(theta), up(v))
            got = a.prob.reduce_tensor().cpu().numpy().copy()
            err, scale = np.max(np.abs(got[:P] - want)), np.max(np.abs(want))
            print(f"{loss} {env} weighted {weighted} intercept {has_intercept} on a {optimizer} problem: max |Hv - numpy| {err:.3e}, |Hv|_inf {scale:.3e}")
            assert err <= 1e-12 * scale      # a fixed-order fp64 sum of <= 20 000 terms
            assert got[P] == 0.0             # the value slot of a product
            assert solve_bits(a.prob) == solve_bits(b.prob)
        finally:
            a.prob.close()
            b.prob.close()


@pytest.mark.gpu
@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("loss", H.LOSSES)
def test_the_product_through_every_form_of_the_copies(device_solver, monkeypatch, loss, form):
    product_case(device_solver, monkeypatch, loss, FORMS[form])


@pytest.mark.gpu
def test_the_product_with_sample_weights(device_solver, monkeypatch):
    product_case(device_solver, monkeypatch, "logistic", {}, weighted=True)


@pytest.mark.gpu
def test_the_product_without_an_intercept(device_solver, monkeypatch):
    product_case(device_solver, monkeypatch, "poisson", {}, has_intercept=False)


# ---- 2: against the reference -------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("size", H.SIZES)
@pytest.mark.parametrize("loss", H.LOSSES)
def test_three_losses_against_the_reference(device_solver, loss, size):
    pb = H.problem(loss, size)
    theta_ref, f_ref = H.reference(loss, size)
    theta, info = fit(fe.FixedEffectDeviceSolver(solver=device_solver), loss, size)
    r = H.tron(pb, max_iter=H.FIT["max_iter"], ftol=H.FIT["tolerance"])
    print(f"{loss} {size}: (status, nit, nfev, nhv) device {counts(info)} restatement {r[2:6]}")
    assert int(info["status"]) in (0, 1) and info["optimizer"] == "TRON"
    H.check_against_reference(pb, theta, float(info["fval"]), theta_ref, f_ref, f"{loss} {size}")


# ---- 3: one iteration from a warm start -----------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_a_warm_start_is_the_start_point(device_solver):
    s = fe.FixedEffectDeviceSolver(solver=device_solver)
    pb = H.problem("poisson", "small")
    theta_ref, f_ref = H.reference("poisson", "small")
    start = 0.5 * theta_ref
    r1 = H.tron(pb, theta0=start, max_iter=1, ftol=H.FIT["tolerance"])
    one, info1 = fit(s, "poisson", "small", theta0=start, max_iter=1)
    print(f"one iteration from the start point: device f {float(info1['fval'])!r} {counts(info1)}; restatement {r1[1]!r} {r1[2:6]}")
    assert counts(info1) == r1[2:6] and r1[2:4] == (2, 1)
    assert abs(float(info1["fval"]) - r1[1]) <= 1e-9 * abs(r1[1]) and float(info1["fval"]) < pb.smooth(start)[0]
    warm, info = fit(s, "poisson", "small", theta0=start)
    print(f"warm start: {counts(info)}")
    assert int(info["status"]) in (0, 1)
    H.check_against_reference(pb, warm, float(info["fval"]), theta_ref, f_ref, "warm start")


# ---- 4: a rejected trial ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_a_rejected_trial_leaves_the_accepted_points_curvature_in_force(device_solver):
    """From a start point of large norm the restatement rejects trials (the helper states how many). The CG after a rejected trial runs on
    the curvature weights of the accepted point, not on those the rejected evaluation wrote: with the wrong ones the fit would not meet
    the bars below."""
    loss, size = H.REJECTING["loss"], H.REJECTING["size"]
    theta0, rejected_np = H.rejecting_case()
    pb = H.problem(loss, size)
    theta_ref, f_ref = H.reference(loss, size)
    theta, info = fit(fe.FixedEffectDeviceSolver(solver=device_solver), loss, size, theta0=theta0)
    rejected = int(info["nfev"]) - int(info["nit"]) - 1
    print(f"rejecting case: device {counts(info)} rejected {rejected}; the restatement rejects {rejected_np}")
    assert int(info["status"]) in (0, 1) and rejected >= 1
    H.check_against_reference(pb, theta, float(info["fval"]), theta_ref, f_ref, "rejecting case")


# ---- 5: stops ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_the_stops(device_solver):
    s = fe.FixedEffectDeviceSolver(solver=device_solver)
    theta_ref, f_ref = H.reference("logistic", "small")
    _, info = fit(s, "logistic", "small", max_iter=2)
    assert counts(info)[:2] == (2, 2)
    theta, info = fit(s, "logistic", "small", theta0=theta_ref)
    assert counts(info) == (0, 0, 1, 0) and np.array_equal(theta, theta_ref)
    rp, col, val, y, off, D, l2 = H.case("logistic", "small")
    f = fe._SteppingFit(device_solver, options("logistic", l2), rp, col, val, y, D, off, None, None, None, None, None)
    try:
        import dataclasses
        f.prob.set_optimizer("TRON")
        f.prob.restart(dataclasses.replace(options("logistic", l2), maxfun=3), None)
        status, _ = f.prob.solve()
        _, res = f.prob.result()
        print(f"maxfun = 3: status {status} nit {res['nit']} nfev {res['nfev']}")
        assert status == 3 and res["nfev"] == 4
    finally:
        f.prob.close()


# ---- 6: the default is untouched ------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_the_default_is_the_plain_fit_bit_for_bit(device_solver):
    rp, col, val, y, off, D, l2 = H.case("logistic", "small")
    s = fe.FixedEffectDeviceSolver(solver=device_solver)
    kw = dict(H.FIT, offset=off, model_type=fe.LOGISTIC_REGRESSION, l2=l2)
    plain = bits(*s.fit_stepping(rp, col, val, y, D, **kw))
    theta, info = s.fit_stepping(rp, col, val, y, D, optimizer="LBFGS", **kw)
    assert bits(theta, info) == plain and info["nhv"] == 0
    theta, info, prob = s.fit_stepping(rp, col, val, y, D, optimizer="TRON", return_problem=True, **kw)
    try:
        assert bits(theta, info) != plain and info["nhv"] > 0
        prob.set_optimizer("LBFGS")
        assert solve_bits(prob)[:5] == plain
    finally:
        prob.close()


@pytest.mark.gpu
def test_same_bits_across_runs_lookaheads_step_forms_and_restarts(device_solver, monkeypatch):
    s = fe.FixedEffectDeviceSolver(solver=device_solver)
    rp, col, val, y, off, D, l2 = H.case("logistic", "small")
    opts = options("logistic", l2)
    theta, info, prob = fit(s, "logistic", "small", return_problem=True)
    try:
        first = bits(theta, info) + (int(info["nhv"]),)
        theta2, info2 = fit(s, "logistic", "small")
        assert bits(theta2, info2) + (int(info2["nhv"]),) == first
        prob.restart(opts, None)      # keeps the problem's optimiser
        assert solve_bits(prob) == first
        prob.restart(opts, None)
        assert solve_bits(prob, lookahead=0) == first
    finally:
        prob.close()
    for fused in ("0", "1"):      # the switch does not concern this step; it must not break it
        monkeypatch.setenv("GDMIX_FE_FUSED_TAIL", fused)
        theta2, info2 = fit(s, "logistic", "small")
        assert bits(theta2, info2) + (int(info2["nhv"]),) == first, fused


# ---- 7: refusals ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_what_the_entry_points_refuse(device_solver):
    from gdmix_amd.solver import GdmixReError
    t = device_solver.torch
    s = fe.FixedEffectDeviceSolver(solver=device_solver)
    theta, info, prob = fit(s, "logistic", "small", return_problem=True)
    try:
        P = theta.size
        mean, scale = t.zeros(P, dtype=t.float64, device=device_solver.device), t.ones(P, dtype=t.float64, device=device_solver.device)
        with pytest.raises(GdmixReError, match="TRON"):      # an L1 term on a TRON problem
            prob.set_l1(3.0)
        with pytest.raises(GdmixReError, match="TRON"):      # a prior on a TRON problem
            prob.set_prior(mean, scale)
        th, res = prob.result()      # the refused calls left the solved problem as it was
        assert np.array_equal(th, theta) and res["nfev"] == int(info["nfev"]) and prob.products() == int(info["nhv"])
        prob.set_optimizer("LBFGS")
        prob.set_l1(3.0)
        with pytest.raises(GdmixReError, match="L1 term"):   # TRON while l1 > 0
            prob.set_optimizer("TRON")
        prob.set_l1(0.0)
        prob.set_prior(mean, scale)
        with pytest.raises(GdmixReError, match="prior"):     # TRON while a prior is installed
            prob.set_optimizer("TRON")
        prob.set_prior(None, None)
        prob.set_optimizer("TRON")
        assert solve_bits(prob) == bits(theta, info) + (int(info["nhv"]),)
    finally:
        prob.close()


# ---- 8: two workers against one -----------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_two_workers_against_one(device_solver, tmp_path):
    root = os.path.dirname(HERE)
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    env.pop("TF_CONFIG", None)
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2", "--master-addr", "127.0.0.1", "--master-port", "29659",
           os.path.join(root, "tests", "_fe_tron_dist_worker.py"), str(tmp_path)]
    subprocess.run(cmd, check=True, env=env, timeout=600, cwd=root)
    with open(tmp_path / "result.json") as fh:
        a, b = json.load(fh)
    assert a["theta"] == b["theta"] and all(a[k] == b[k] for k in ("fval", "status", "nit", "nfev", "nhv"))      # replicated step
    theta_ref, f_ref = H.reference("logistic", "small")
    theta, info = fit(fe.FixedEffectDeviceSolver(solver=device_solver), "logistic", "small")
    print(f"two workers ({a['backend']}): {(a['status'], a['nit'], a['nfev'], a['nhv'])}; one worker {counts(info)}")
    assert a["status"] in (0, 1)
    H.check_against_reference(H.problem("logistic", "small"), np.array(a["theta"]), a["fval"], theta_ref, f_ref, "two workers")
    assert abs(a["fval"] - float(info["fval"])) <= 1e-9 * abs(float(info["fval"]))


# ---- 9: variances -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["SIMPLE", "FULL"])
def test_variances_after_a_tron_fit(device_solver, mode):
    """The numpy expressions of test_gpu_fe_l1.py::test_variances_are_those_of_the_smooth_part at the returned theta, with its rtols."""
    rp, col, val, y, off, D, l2 = H.case("logistic", "small")
    s = fe.FixedEffectDeviceSolver(solver=device_solver)
    theta, info = fit(s, "logistic", "small", variance_mode=mode)
    assert np.array_equal(theta, fit(s, "logistic", "small")[0])
    X = H.problem("logistic", "small").X
    rho = 1.0 / (1.0 + np.exp(-(X @ theta + off.astype(np.float64))))
    d = rho * (1.0 - rho)
    if mode == "SIMPLE":      # val^2 d per ENTRY: a column repeated inside a row counts once per entry (tests/test_gpu_fe_poisson.py)
        rows = np.repeat(np.arange(rp.size - 1), np.diff(rp))
        want = 1.0 / (np.concatenate([np.bincount(col, weights=val.astype(np.float64) ** 2 * d[rows], minlength=D), [d.sum()]]) + l2 + 1e-12)
    else:
        want = np.diagonal(np.linalg.inv(np.asarray((X.T @ X.multiply(d[:, None])).todense()) + (l2 + 1e-12) * np.eye(D + 1)))
    np.testing.assert_allclose(info["variances"], want, rtol=1e-7 if mode == "SIMPLE" else 1e-4)


# ---- 10: the sweep ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_the_sweep_keeps_the_optimizer(device_solver):
    rp, col, val, y, off, D, _ = H.case("logistic", "small")
    s = fe.FixedEffectDeviceSolver(solver=device_solver)
    grid = (10.0, 1.0, 0.1)
    kw = dict(H.FIT, offset=off, model_type=fe.LOGISTIC_REGRESSION)
    seen = []

    def select(thetas):
        seen.extend(np.array(th) for th in thetas)
        return 1
    theta, info, best = s.fit_sweep(rp, col, val, y, D, l2_grid=grid, select=select, optimizer="TRON", **kw)
    alone = [s.fit_stepping(rp, col, val, y, D, l2=w, optimizer="TRON", **kw) for w in grid]
    assert best == 1 and len(seen) == 3 and info["optimizer"] == "TRON"
    for w, th, (th1, info1) in zip(grid, seen, alone):
        assert np.array_equal(th, th1), w
        assert info1["nhv"] > 0
    assert bits(theta, info) == bits(*alone[1]) and info["nhv"] == alone[1][1]["nhv"]
    assert len({th.tobytes() for th in seen}) == 3


# ---- 11: the stage, through the command line, in process ------------------------------------------------------------------------------------
def _read_model(path):
    from gdmix_amd.io import avro
    (rec,) = list(avro.read_file(path))
    return {m["name"]: m["value"] for m in rec["means"]}


@pytest.mark.gpu
def test_the_stage_trains_by_tron_and_inference_ignores_the_flag(device_solver, tmp_path):
    data = chain.make_dataset(200, 300, 6000, train_fraction=0.5)
    base, root = str(tmp_path / "inputs"), str(tmp_path / "tron")
    chain.write_global_inputs(base, data)
    shutil.copytree(os.path.join(base, "global"), os.path.join(root, "global"))
    argv = chain.stage_argv(root, "global", chain.LOGISTIC, False)
    chain.run_stage(argv + ["--optimizer=TRON"])
    train = np.flatnonzero(data["train"])
    ptr, cols, vals, D = chain.bag_rows(data, "global", train)
    s = fe.FixedEffectDeviceSolver(solver=device_solver)
    kw = dict(has_intercept=True, l2=1.0, regularize_bias=False, model_type=fe.LOGISTIC_REGRESSION, max_iter=100, m=10, tolerance=1e-12, dummy=False)
    theta, info = s.fit_stepping(ptr, cols, vals, data["response"][train].astype(np.float32), D, optimizer="TRON", **kw)
    plain, _ = s.fit_stepping(ptr, cols, vals, data["response"][train].astype(np.float32), D, **kw)
    want = {f"g{j}": float(theta[j]) for j in range(D) if abs(theta[j]) > 1e-4}
    want["(INTERCEPT)"] = float(theta[D])
    model = _read_model(os.path.join(root, "global", "models", "part-00000.avro"))
    print(f"stage with --optimizer=TRON: {len(model)} coefficients in the file; fit {counts(info)}")
    assert model == want and info["nhv"] > 0 and not np.array_equal(theta, plain)      # the values are doubles: bit for bit, and TRON's
    scores = os.path.join(root, "global", "validationScores", "part-00000.avro")
    trained = chain.read_scores(os.path.dirname(scores))
    os.remove(scores)
    chain.run_stage([a.replace("--action=train", "--action=inference") for a in argv] + ["--optimizer=TRON"])
    again = chain.read_scores(os.path.dirname(scores))
    assert again[0].size == int((~data["train"]).sum()) and all(np.array_equal(x, y) for x, y in zip(trained, again))
