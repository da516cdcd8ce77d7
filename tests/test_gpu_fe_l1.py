"""GPU: the fixed effect's L1 / elastic-net fit by OWL-QN on the device (fit_stepping(l1=...); include/gdmix_fe.h, "(ABI 23) L1 / elastic net";
csrc/fe_qn.hip) against a reference that does not share its algorithm: scipy's bounded L-BFGS-B on the split problem (tests/fe_l1_helpers.py,
which also states the bars). Three losses at two sizes, a wrapping history ring, the all-zero solution, the plain fit bit for bit at l1 = 0, the
same bits across runs, step forms and restarts, variances, two workers against one, and the stage through the command line."""
import json
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

from gdmix_amd import chain
from gdmix_amd import fixed_effect as fe
import fe_l1_helpers as H

HERE = os.path.dirname(os.path.abspath(__file__))


def fit(s, loss, size, **kw):
    rp, col, val, y, off, D, l1, l2 = H.case(loss, size)
    args = dict(H.FIT, offset=off, model_type=H.MODEL_TYPE[loss], l1=l1, l2=l2)
    args.update(kw)
    return s.fit_stepping(rp, col, val, y, D, **args)


def bits(theta, info):
    return np.asarray(theta, np.float64).tobytes(), float(info["fval"]).hex(), int(info["nit"]), int(info["nfev"]), int(info["status"])


def solve_bits(prob, lookahead=None):
    status, _ = prob.solve() if lookahead is None else prob.solve(lookahead=lookahead)
    theta, info = prob.result()
    return bits(theta, dict(info, status=status))


# ---- 1, 2: against the reference ------------------------------------------------------------------------------------------------------
def against_reference(s, loss, size, m):
    pb = H.problem(loss, size)
    theta_ref, f_ref = H.reference(loss, size)
    theta, info = fit(s, loss, size, m=m)
    _, _, st_np, nit_np, nfev_np = H.owlqn(pb, m=m, max_iter=H.FIT["max_iter"], ftol=H.FIT["tolerance"])
    print(f"{loss} {size} m = {m}: device status {int(info['status'])} nit {int(info['nit'])} nfev {int(info['nfev'])}; restatement {st_np} {nit_np} {nfev_np}")
    assert int(info["status"]) in (0, 1)
    assert info["l1"] == pb.l1 and info["nnz"] == np.count_nonzero(theta)
    H.check_against_reference(pb, theta, float(info["fval"]), theta_ref, f_ref, f"{loss} {size} m = {m}")
    return theta, info


@pytest.mark.gpu
@pytest.mark.parametrize("size", ["small", "wide"])
@pytest.mark.parametrize("loss", H.LOSSES)
def test_three_losses_against_the_reference(device_solver, loss, size):
    against_reference(fe.FixedEffectDeviceSolver(solver=device_solver), loss, size, H.FIT["m"])


@pytest.mark.gpu
def test_the_history_ring_wraps(device_solver):
    _, info = against_reference(fe.FixedEffectDeviceSolver(solver=device_solver), "logistic", "small", 3)
    assert int(info["nit"]) > 3


# ---- 3: the all-zero solution -----------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_a_weight_above_the_gradient_at_zero_stops_at_zero(device_solver):
    rp, col, val, y, off, D, _, l2 = H.case("logistic", "small")
    pb = H.Problem("logistic", H.design(rp, col, val, D, has_intercept=False), y, off, 0.0, l2)
    l1 = 1.5 * float(np.max(np.abs(pb.smooth(np.zeros(D))[1])))
    s = fe.FixedEffectDeviceSolver(solver=device_solver)
    theta, info = s.fit_stepping(rp, col, val, y, D, offset=off, model_type=fe.LOGISTIC_REGRESSION, l1=l1, l2=l2,
                                 **dict(H.FIT, has_intercept=False, regularize_bias=False))
    assert (int(info["status"]), int(info["nit"]), int(info["nfev"]), info["nnz"]) == (0, 0, 1, 0)
    assert theta.shape == (D,) and not np.any(theta) and float(info["gnorm"]) == 0.0
    assert abs(float(info["fval"]) - pb.F(np.zeros(D))) <= 1e-12 * pb.F(np.zeros(D))


@pytest.mark.gpu
def test_a_warm_start_is_the_start_point(device_solver):
    """From theta0 = half the reference's minimiser (its support, a real distance away). One iteration from there is the restatement's one
    iteration — the start point was honoured, not zeros — and the whole fit meets the bars of the cold one."""
    s = fe.FixedEffectDeviceSolver(solver=device_solver)
    pb = H.problem("poisson", "small")
    theta_ref, f_ref = H.reference("poisson", "small")
    start = 0.5 * theta_ref
    _, F1, st1, nit1, nfev1 = H.owlqn(pb, theta0=start, m=H.FIT["m"], max_iter=1, ftol=H.FIT["tolerance"])
    one, info1 = fit(s, "poisson", "small", theta0=start, max_iter=1)
    print(f"one iteration from the start point: device F {float(info1['fval'])!r} status {int(info1['status'])} nit {int(info1['nit'])} nfev {int(info1['nfev'])}; "
          f"restatement {F1!r} {st1} {nit1} {nfev1}")
    assert (int(info1["status"]), int(info1["nit"]), int(info1["nfev"])) == (st1, nit1, nfev1) == (2, 1, nfev1)
    assert abs(float(info1["fval"]) - F1) <= 1e-9 * abs(F1) and F1 < pb.F(start)
    warm, info = fit(s, "poisson", "small", theta0=start)
    print(f"warm start: status {int(info['status'])} nit {int(info['nit'])} nfev {int(info['nfev'])}")
    assert int(info["status"]) in (0, 1)
    H.check_against_reference(pb, warm, float(info["fval"]), theta_ref, f_ref, "warm start")


@pytest.mark.gpu
def test_what_the_entry_point_refuses(device_solver):
    from gdmix_amd.solver import GdmixReError
    t = device_solver.torch
    s = fe.FixedEffectDeviceSolver(solver=device_solver)
    theta, info, prob = fit(s, "logistic", "small", return_problem=True)
    try:
        P = theta.size
        for bad in (-1.0, float("nan"), float("inf")):
            with pytest.raises(GdmixReError, match="finite and >= 0"):
                prob.set_l1(bad)
        mean, scale = t.zeros(P, dtype=t.float64, device=device_solver.device), t.ones(P, dtype=t.float64, device=device_solver.device)
        with pytest.raises(GdmixReError, match="L1 term"):      # a prior while l1 > 0
            prob.set_prior(mean, scale)
        th, res = prob.result()      # the refused calls left the solved problem as it was
        assert np.array_equal(th, theta) and res["nfev"] == int(info["nfev"])
        prob.set_l1(0.0)
        prob.set_prior(mean, scale)
        with pytest.raises(GdmixReError, match="prior"):        # an L1 term while a prior is installed
            prob.set_l1(3.0)
        prob.set_prior(None, None)
        prob.set_l1(H.case("logistic", "small")[6])
        assert solve_bits(prob) == bits(theta, info)
    finally:
        prob.close()


# ---- 4: l1 = 0 is the plain fit -----------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_l1_zero_is_the_plain_fit_bit_for_bit(device_solver):
    rp, col, val, y, off, D, _, l2 = H.case("logistic", "small")
    s = fe.FixedEffectDeviceSolver(solver=device_solver)
    kw = dict(H.FIT, offset=off, model_type=fe.LOGISTIC_REGRESSION, l2=l2)
    plain = bits(*s.fit_stepping(rp, col, val, y, D, **kw))
    assert bits(*s.fit_stepping(rp, col, val, y, D, l1=0.0, **kw)) == plain
    theta, info, prob = s.fit_stepping(rp, col, val, y, D, l1=3.0, return_problem=True, **kw)
    try:
        assert bits(theta, info) != plain and info["nnz"] < D
        prob.set_l1(0.0)
        assert solve_bits(prob) == plain
    finally:
        prob.close()


# ---- 5: the same bits across runs, lookaheads, step forms and restarts ------------------------------------------------------------------
@pytest.mark.gpu
def test_same_bits_across_runs_step_forms_and_restarts(device_solver, monkeypatch):
    s = fe.FixedEffectDeviceSolver(solver=device_solver)
    rp, col, val, y, off, D, l1, l2 = H.case("logistic", "small")
    opts = fe.fit_options(H.FIT["has_intercept"], l2, H.FIT["regularize_bias"], fe.LOGISTIC_REGRESSION, H.FIT["max_iter"], H.FIT["m"], H.FIT["tolerance"])
    theta, info, prob = fit(s, "logistic", "small", return_problem=True)
    try:
        first = bits(theta, info)
        assert bits(*fit(s, "logistic", "small")) == first
        prob.restart(opts, None)      # keeps the problem's l1
        assert solve_bits(prob) == first
        prob.restart(opts, None)
        assert solve_bits(prob, lookahead=0) == first
    finally:
        prob.close()
    for fused in ("0", "1"):      # the switch does not concern this step; it must not break it
        monkeypatch.setenv("GDMIX_FE_FUSED_TAIL", fused)
        assert bits(*fit(s, "logistic", "small")) == first, fused


# ---- 6: variances -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["SIMPLE", "FULL"])
def test_variances_are_those_of_the_smooth_part(device_solver, mode):
    """At the returned theta, gdmix_fe_hessian_diag plus l2; a coefficient at exactly 0 gets one too (the header states the choice)."""
    rp, col, val, y, off, D, l1, l2 = H.case("logistic", "small")
    s = fe.FixedEffectDeviceSolver(solver=device_solver)
    theta, info = fit(s, "logistic", "small", variance_mode=mode)
    assert np.array_equal(theta, fit(s, "logistic", "small")[0]) and 0 < info["nnz"] < D + 1
    X = H.problem("logistic", "small").X
    rho = 1.0 / (1.0 + np.exp(-(X @ theta + off.astype(np.float64))))
    d = rho * (1.0 - rho)
    if mode == "SIMPLE":      # val^2 d per ENTRY: a column repeated inside a row counts once per entry (tests/test_gpu_fe_poisson.py)
        rows = np.repeat(np.arange(rp.size - 1), np.diff(rp))
        want = 1.0 / (np.concatenate([np.bincount(col, weights=val.astype(np.float64) ** 2 * d[rows], minlength=D), [d.sum()]]) + l2 + 1e-12)
    else:
        want = np.diagonal(np.linalg.inv(np.asarray((X.T @ X.multiply(d[:, None])).todense()) + (l2 + 1e-12) * np.eye(D + 1)))
    np.testing.assert_allclose(info["variances"], want, rtol=1e-7 if mode == "SIMPLE" else 1e-4)
    assert np.all(np.asarray(info["variances"])[theta == 0] > 0)


# ---- 7: two workers against one -----------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_two_workers_against_one(device_solver, tmp_path):
    root = os.path.dirname(HERE)
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    env.pop("TF_CONFIG", None)
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2", "--master-addr", "127.0.0.1", "--master-port", "29653",
           os.path.join(root, "tests", "_fe_l1_dist_worker.py"), str(tmp_path)]
    subprocess.run(cmd, check=True, env=env, timeout=600, cwd=root)
    with open(tmp_path / "result.json") as fh:
        a, b = json.load(fh)
    assert a["theta"] == b["theta"] and (a["fval"], a["status"], a["nit"], a["nfev"]) == (b["fval"], b["status"], b["nit"], b["nfev"])      # replicated step
    theta_ref, f_ref = H.reference("logistic", "small")
    print(f"two workers ({a['backend']}): status {a['status']} nit {a['nit']} nfev {a['nfev']} non-zeros {a['nnz']}")
    assert a["status"] in (0, 1)
    H.check_against_reference(H.problem("logistic", "small"), np.array(a["theta"]), a["fval"], theta_ref, f_ref, "two workers")
    theta, info = fit(fe.FixedEffectDeviceSolver(solver=device_solver), "logistic", "small")
    assert np.array_equal(np.array(a["theta"]) != 0, theta != 0)


# ---- 8: the stage, through the command line, in process -----------------------------------------------------------------------------------
def _read_model(path):
    from gdmix_amd.io import avro
    (rec,) = list(avro.read_file(path))
    return {m["name"]: m["value"] for m in rec["means"]}


@pytest.mark.gpu
def test_the_stage_writes_the_support_and_inference_scores_with_it(device_solver, tmp_path):
    data = chain.make_dataset(200, 300, 6000, train_fraction=0.5)
    base, root = str(tmp_path / "inputs"), str(tmp_path / "l1")
    chain.write_global_inputs(base, data)
    shutil.copytree(os.path.join(base, "global"), os.path.join(root, "global"))
    argv = chain.stage_argv(root, "global", chain.LOGISTIC, False)
    chain.run_stage(argv + ["--l1_reg_weight=3"])
    train = np.flatnonzero(data["train"])
    ptr, cols, vals, D = chain.bag_rows(data, "global", train)
    s = fe.FixedEffectDeviceSolver(solver=device_solver)
    theta, info = s.fit_stepping(ptr, cols, vals, data["response"][train].astype(np.float32), D, has_intercept=True, l1=3.0, l2=1.0, regularize_bias=False,
                                 model_type=fe.LOGISTIC_REGRESSION, max_iter=100, m=10, tolerance=1e-12, dummy=False)
    want = {f"g{j}": float(theta[j]) for j in range(D) if abs(theta[j]) > 1e-4}
    want["(INTERCEPT)"] = float(theta[D])
    model = _read_model(os.path.join(root, "global", "models", "part-00000.avro"))
    print(f"stage with --l1_reg_weight=3: {len(model)} coefficients in the file, {info['nnz']} non-zeros of {D + 1}")
    assert model == want and 1 < len(model) <= info["nnz"] < D + 1      # only the support's coefficients; the values are doubles: bit for bit
    scores = os.path.join(root, "global", "validationScores", "part-00000.avro")
    trained = chain.read_scores(os.path.dirname(scores))
    os.remove(scores)
    chain.run_stage([a.replace("--action=train", "--action=inference") for a in argv] + ["--l1_reg_weight=3"])
    again = chain.read_scores(os.path.dirname(scores))
    assert again[0].size == int((~data["train"]).sum()) and all(np.array_equal(x, y) for x, y in zip(trained, again))
