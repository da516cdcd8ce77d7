"""GPU: box constraints on the fixed effect's coefficients by projected L-BFGS on the device (fit_stepping(bounds=...); include/gdmix_fe.h,
"(ABI 26) box constraints"; csrc/fe_qn.hip) against a reference that does not share its algorithm: scipy's fmin_l_bfgs_b with the same bounds
(tests/fe_box_helpers.py, which also states the bars). Three losses at two sizes, a wrapping history ring, start points, a problem solved at its
start point, the plain fit bit for bit without bounds, the same bits across runs, lookaheads and restarts, every refusal, variances, two workers
against one, and the stage through the command line."""
import json
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

from gdmix_amd import chain
from gdmix_amd import fixed_effect as fe
import fe_box_helpers as H

HERE = os.path.dirname(os.path.abspath(__file__))


def fit(s, loss, size, **kw):
    rp, col, val, y, off, D, _, l2 = H.case(loss, size)
    args = dict(H.FIT, offset=off, model_type=H.MODEL_TYPE[loss], l2=l2, bounds=H.bounds(size))
    args.update(kw)
    return s.fit_stepping(rp, col, val, y, D, **args)


def bits(theta, info):
    return np.asarray(theta, np.float64).tobytes(), float(info["fval"]).hex(), int(info["nit"]), int(info["nfev"]), int(info["status"])


def solve_bits(prob, lookahead=None):
    status, _ = prob.solve() if lookahead is None else prob.solve(lookahead=lookahead)
    theta, info = prob.result()
    return bits(theta, dict(info, status=status))


def on_device(s, a):
    t = s.solver.torch
    return t.from_numpy(np.ascontiguousarray(a, np.float64)).to(s.solver.device)


# ---- against the reference -------------------------------------------------------------------------------------------------------------
def against_reference(s, loss, size, m):
    pb = H.problem(loss, size)
    lo, hi = H.bounds(size)
    theta_ref, f_ref = H.reference(loss, size)
    theta, info = fit(s, loss, size, m=m)
    _, _, st_np, nit_np, nfev_np = H.box(pb, lo, hi, m=m, max_iter=H.FIT["max_iter"], ftol=H.FIT["tolerance"])
    print(f"{loss} {size} m = {m}: device status {int(info['status'])} nit {int(info['nit'])} nfev {int(info['nfev'])}; restatement {st_np} {nit_np} {nfev_np}")
    assert int(info["status"]) in (0, 1)
    assert info["at_bound"] == int(H.at_bound(theta, lo, hi).sum())
    H.check_against_reference(pb, lo, hi, theta, float(info["fval"]), theta_ref, f_ref, f"{loss} {size} m = {m}")
    gnorm = H.projected_gradient_norm(theta, pb.smooth(theta)[1], lo, hi)
    print(f"gnorm {float(info['gnorm'])!r} numpy projected gradient {gnorm!r}")
    assert abs(float(info["gnorm"]) - gnorm) <= 1e-9 * max(1.0, np.max(np.abs(pb.smooth(theta)[1])))      # a difference of gradients, each good to ~1e-12 relative
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


# ---- start points ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_a_cold_start_is_the_clamped_zeros(device_solver):
    """The pinned and the hi = -0.02 coefficients start at their bounds: a problem with bounds that has not taken a step returns clamp(0)."""
    s = fe.FixedEffectDeviceSolver(solver=device_solver)
    lo, hi = H.bounds("small")
    start = np.clip(np.zeros(lo.size), lo, hi)
    assert np.count_nonzero(start) > 0
    pb = H.problem("logistic", "small")
    theta, info, prob = fit(s, "logistic", "small", return_problem=True)
    try:
        opts = fe.fit_options(H.FIT["has_intercept"], pb.l2, H.FIT["regularize_bias"], fe.LOGISTIC_REGRESSION, H.FIT["max_iter"], H.FIT["m"], H.FIT["tolerance"])
        prob.restart(opts, None)
        th0, _ = prob.result()
        assert np.array_equal(th0, start)
        prob.eval()
        assert prob.step() < 0
        _, r = prob.result()      # after the first evaluation: F and the projected gradient at the clamped zeros
        F0, g0 = pb.smooth(start)
        print(f"at the clamped zeros: device F {r['fval']!r} numpy {F0!r}; gnorm {r['gnorm']!r} numpy {H.projected_gradient_norm(start, g0, lo, hi)!r}")
        assert abs(r["fval"] - F0) <= 1e-9 * abs(F0) and (r["nit"], r["nfev"]) == (0, 1)
    finally:
        prob.close()


@pytest.mark.gpu
def test_a_warm_start_is_the_clamped_start_point(device_solver):
    """From theta0 = half the reference's minimiser (outside the box where a pinned or negative-capped coefficient is halved): one iteration from
    there is the restatement's one iteration, and the whole fit meets the bars of the cold one."""
    s = fe.FixedEffectDeviceSolver(solver=device_solver)
    pb = H.problem("poisson", "small")
    lo, hi = H.bounds("small")
    theta_ref, f_ref = H.reference("poisson", "small")
    start = 0.5 * theta_ref
    assert not np.all((lo <= start) & (start <= hi))
    _, F1, st1, nit1, nfev1 = H.box(pb, lo, hi, theta0=start, m=H.FIT["m"], max_iter=1, ftol=H.FIT["tolerance"])
    one, info1 = fit(s, "poisson", "small", theta0=start, max_iter=1)
    print(f"one iteration from the start point: device F {float(info1['fval'])!r} status {int(info1['status'])} nit {int(info1['nit'])} nfev {int(info1['nfev'])}; "
          f"restatement {F1!r} {st1} {nit1} {nfev1}")
    assert (int(info1["status"]), int(info1["nit"]), int(info1["nfev"])) == (st1, nit1, nfev1) == (2, 1, nfev1)
    assert abs(float(info1["fval"]) - F1) <= 1e-9 * abs(F1) and F1 < pb.smooth(np.clip(start, lo, hi))[0]
    assert np.all((lo <= one) & (one <= hi))
    warm, info = fit(s, "poisson", "small", theta0=start)
    print(f"warm start: status {int(info['status'])} nit {int(info['nit'])} nfev {int(info['nfev'])}")
    assert int(info["status"]) in (0, 1)
    H.check_against_reference(pb, lo, hi, warm, float(info["fval"]), theta_ref, f_ref, "warm start")


@pytest.mark.gpu
def test_a_problem_whose_minimiser_is_the_start_point(device_solver):
    rp, col, val, y, off, D, _, l2 = H.case("logistic", "small")
    pb = H.L1.Problem("logistic", H.design(rp, col, val, D, has_intercept=False), y, off, 0.0, l2)
    s = fe.FixedEffectDeviceSolver(solver=device_solver)
    theta, info = s.fit_stepping(rp, col, val, y, D, offset=off, model_type=fe.LOGISTIC_REGRESSION, l2=l2, bounds=(np.zeros(D), np.zeros(D)),
                                 **dict(H.FIT, has_intercept=False, regularize_bias=False))
    assert (int(info["status"]), int(info["nit"]), int(info["nfev"]), info["at_bound"]) == (0, 0, 1, D)
    assert theta.shape == (D,) and not np.any(theta) and float(info["gnorm"]) == 0.0
    assert abs(float(info["fval"]) - pb.smooth(np.zeros(D))[0]) <= 1e-12 * pb.smooth(np.zeros(D))[0]


# ---- without bounds: the plain fit ---------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_without_bounds_the_plain_fit_bit_for_bit(device_solver):
    rp, col, val, y, off, D, _, l2 = H.case("logistic", "small")
    s = fe.FixedEffectDeviceSolver(solver=device_solver)
    kw = dict(H.FIT, offset=off, model_type=fe.LOGISTIC_REGRESSION, l2=l2)
    plain = bits(*s.fit_stepping(rp, col, val, y, D, **kw))
    assert bits(*s.fit_stepping(rp, col, val, y, D, bounds=None, **kw)) == plain
    theta, info, prob = s.fit_stepping(rp, col, val, y, D, bounds=H.bounds("small"), return_problem=True, **kw)
    try:
        assert bits(theta, info) != plain and info["at_bound"] > 0
        prob.set_bounds(None, None)
        assert solve_bits(prob) == plain
    finally:
        prob.close()


@pytest.mark.gpu
def test_all_infinite_bounds_find_the_unconstrained_minimiser(device_solver):
    """The bounded step with nothing to bind, held to the reference bars against scipy's unconstrained minimiser."""
    s = fe.FixedEffectDeviceSolver(solver=device_solver)
    pb = H.problem("logistic", "small")
    P = pb.X.shape[1]
    lo, hi = np.full(P, -np.inf), np.full(P, np.inf)
    theta_ref, f_ref = H.reference_fit(pb, lo, hi)
    theta, info = fit(s, "logistic", "small", bounds=(lo, hi))
    print(f"all-infinite bounds: status {int(info['status'])} nit {int(info['nit'])} nfev {int(info['nfev'])}")
    assert int(info["status"]) in (0, 1) and info["at_bound"] == 0
    H.check_against_reference(pb, lo, hi, theta, float(info["fval"]), theta_ref, f_ref, "all-infinite bounds")


# ---- the same bits across runs, lookaheads and restarts --------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_same_bits_across_runs_lookaheads_and_restarts(device_solver):
    s = fe.FixedEffectDeviceSolver(solver=device_solver)
    l2 = H.case("logistic", "small")[7]
    opts = fe.fit_options(H.FIT["has_intercept"], l2, H.FIT["regularize_bias"], fe.LOGISTIC_REGRESSION, H.FIT["max_iter"], H.FIT["m"], H.FIT["tolerance"])
    theta, info, prob = fit(s, "logistic", "small", return_problem=True)
    try:
        first = bits(theta, info)
        assert bits(*fit(s, "logistic", "small")) == first
        prob.restart(opts, None)      # keeps the problem's bounds
        assert solve_bits(prob) == first
        prob.restart(opts, None)
        assert solve_bits(prob, lookahead=0) == first
        prob.restart(opts, None)
        assert solve_bits(prob, lookahead=5) == first
    finally:
        prob.close()


# ---- refusals --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_what_the_entry_points_refuse(device_solver):
    from gdmix_amd.solver import GdmixReError
    s = fe.FixedEffectDeviceSolver(solver=device_solver)
    lo, hi = (np.array(b) for b in H.bounds("small"))
    theta, info, prob = fit(s, "logistic", "small", return_problem=True)
    try:
        P = theta.size
        same = lambda: (np.array_equal(prob.result()[0], theta) and prob.result()[1]["nfev"] == int(info["nfev"]))      # a refused call left the solved problem as it was

        def refused(match, lower, upper):
            with pytest.raises(GdmixReError, match=match):
                prob.set_bounds(on_device(s, lower), on_device(s, upper))
            assert same()
        bad = lo.copy(); bad[3] = np.nan
        refused("not a number", bad, hi)
        bad = hi.copy(); bad[5] = np.nan
        refused("not a number", lo, bad)
        bad = lo.copy(); bad[7] = 1.0; up = hi.copy(); up[7] = 0.5
        refused("exceeds", bad, up)
        bad = hi.copy(); bad[P - 1] = 10.0
        refused("intercept", lo, bad)
        bad = lo.copy(); bad[P - 1] = -10.0
        refused("intercept", bad, hi)
        with pytest.raises(GdmixReError, match="together"):
            prob.set_bounds(on_device(s, lo), None)
        # the mirror calls on a problem that has bounds
        with pytest.raises(GdmixReError, match="gdmix_fe_set_l1.*bounds"):
            prob.set_l1(3.0)
        with pytest.raises(GdmixReError, match="gdmix_fe_set_optimizer.*bounds"):
            prob.set_optimizer("TRON")
        mean, scale = on_device(s, np.zeros(P)), on_device(s, np.ones(P))
        with pytest.raises(GdmixReError, match="gdmix_fe_set_prior.*bounds"):
            prob.set_prior(mean, scale)
        assert same()
        # bounds on a problem with an L1 term, TRON's, or one with a prior
        prob.set_bounds(None, None)
        prob.set_l1(3.0)
        with pytest.raises(GdmixReError, match="gdmix_fe_set_bounds.*L1"):
            prob.set_bounds(on_device(s, lo), on_device(s, hi))
        prob.set_l1(0.0)
        prob.set_optimizer("TRON")
        with pytest.raises(GdmixReError, match="gdmix_fe_set_bounds.*TRON"):
            prob.set_bounds(on_device(s, lo), on_device(s, hi))
        prob.set_optimizer("LBFGS")
        prob.set_prior(mean, scale)
        with pytest.raises(GdmixReError, match="gdmix_fe_set_bounds.*prior"):
            prob.set_bounds(on_device(s, lo), on_device(s, hi))
        prob.set_prior(None, None)
        prob.set_bounds(on_device(s, lo), on_device(s, hi))
        assert solve_bits(prob) == bits(theta, info)
    finally:
        prob.close()
    with pytest.raises(ValueError, match="bounds"):
        fit(s, "logistic", "small", l1=1.0)
    with pytest.raises(ValueError, match="bounds"):
        fit(s, "logistic", "small", optimizer="TRON")
    with pytest.raises(ValueError, match="intercept"):
        fit(s, "logistic", "small", bounds=(lo, np.where(np.arange(P) == P - 1, 1.0, hi)))


# ---- variances -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_variances_are_those_of_the_smooth_objective(device_solver):
    """SIMPLE at the returned theta: gdmix_fe_hessian_diag plus l2; a coefficient at a bound gets one too (the header states the choice)."""
    rp, col, val, y, off, D, _, l2 = H.case("logistic", "small")
    lo, hi = H.bounds("small")
    s = fe.FixedEffectDeviceSolver(solver=device_solver)
    theta, info = fit(s, "logistic", "small", variance_mode="SIMPLE")
    assert np.array_equal(theta, fit(s, "logistic", "small")[0]) and 0 < info["at_bound"] < D + 1
    X = H.problem("logistic", "small").X
    rho = 1.0 / (1.0 + np.exp(-(X @ theta + off.astype(np.float64))))
    d = rho * (1.0 - rho)
    rows = np.repeat(np.arange(rp.size - 1), np.diff(rp))      # val^2 d per ENTRY: a column repeated inside a row counts once per entry
    want = 1.0 / (np.concatenate([np.bincount(col, weights=val.astype(np.float64) ** 2 * d[rows], minlength=D), [d.sum()]]) + l2 + 1e-12)
    np.testing.assert_allclose(info["variances"], want, rtol=1e-7)
    assert np.all(np.asarray(info["variances"])[H.at_bound(theta, lo, hi)] > 0)


# ---- two workers against one -------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_two_workers_against_one(device_solver, tmp_path):
    root = os.path.dirname(HERE)
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    env.pop("TF_CONFIG", None)
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2", "--master-addr", "127.0.0.1", "--master-port", "29657",
           os.path.join(root, "tests", "_fe_box_dist_worker.py"), str(tmp_path)]
    subprocess.run(cmd, check=True, env=env, timeout=600, cwd=root)
    with open(tmp_path / "result.json") as fh:
        a, b = json.load(fh)
    assert a["theta"] == b["theta"] and (a["fval"], a["status"], a["nit"], a["nfev"]) == (b["fval"], b["status"], b["nit"], b["nfev"])      # replicated step
    theta_ref, f_ref = H.reference("logistic", "small")
    print(f"two workers ({a['backend']}): status {a['status']} nit {a['nit']} nfev {a['nfev']} at a bound {a['at_bound']}")
    assert a["status"] in (0, 1)
    H.check_against_reference(H.problem("logistic", "small"), *H.bounds("small"), np.array(a["theta"]), a["fval"], theta_ref, f_ref, "two workers")


# ---- the stage, through the command line, in process ---------------------------------------------------------------------------------------------
def _read_model(path):
    from gdmix_amd.io import avro
    (rec,) = list(avro.read_file(path))
    return {(m["name"], m["term"]): m["value"] for m in rec["means"]}


CONSTRAINTS = [{"name": "g3", "term": "t1", "lowerBound": 0.05, "upperBound": 0.05},      # exact: pinned
               {"name": "g3", "term": "*", "upperBound": -0.01},                            # every other term of g3
               {"name": "g5", "term": "*", "lowerBound": 0.0},
               {"name": "*", "term": "*", "lowerBound": -0.2, "upperBound": 0.2}]


def _stage_inputs(tmp_path):
    """A small directory whose feature file has two terms per name (g0,t0 g0,t1 g1,t0 ...) and a constraints file with an exact record, a
    term wildcard and the all-wildcard -> (data, root, constraints path, features, lower, upper)."""
    data = chain.make_dataset(200, 300, 6000, train_fraction=0.5)
    base, root = str(tmp_path / "inputs"), str(tmp_path / "box")
    chain.write_global_inputs(base, data)
    shutil.copytree(os.path.join(base, "global"), os.path.join(root, "global"))
    D = data["bags"]["global"][3]
    features = [(f"g{j // 2}", f"t{j % 2}") for j in range(D)]
    with open(os.path.join(root, "global", "featureList"), "w") as f:
        f.write("".join(f"{n},{t}\n" for n, t in features))
    path = os.path.join(root, "constraints.json")
    with open(path, "w") as f:
        json.dump(CONSTRAINTS, f)
    lo, hi = np.full(D + 1, -np.inf), np.full(D + 1, np.inf)
    lo[:D], hi[:D] = -0.2, 0.2
    lo[10:12], hi[10:12] = 0.0, np.inf
    lo[6], hi[6] = -np.inf, -0.01
    lo[7], hi[7] = 0.05, 0.05
    return data, root, path, features, lo, hi


@pytest.mark.gpu
def test_the_stage_keeps_the_model_in_the_box(device_solver, tmp_path):
    data, root, path, features, lo, hi = _stage_inputs(tmp_path)
    argv = chain.stage_argv(root, "global", chain.LOGISTIC, False)
    chain.run_stage(argv + [f"--coefficient_constraints={path}"])
    train = np.flatnonzero(data["train"])
    ptr, cols, vals, D = chain.bag_rows(data, "global", train)
    s = fe.FixedEffectDeviceSolver(solver=device_solver)
    theta, info = s.fit_stepping(ptr, cols, vals, data["response"][train].astype(np.float32), D, has_intercept=True, l2=1.0, regularize_bias=False,
                                 model_type=fe.LOGISTIC_REGRESSION, max_iter=100, m=10, tolerance=1e-12, dummy=False, bounds=(lo, hi))
    model = _read_model(os.path.join(root, "global", "models", "part-00000.avro"))
    print(f"stage with --coefficient_constraints: {len(model)} coefficients in the file, {info['at_bound']} of {D + 1} at a bound, status {int(info['status'])}")
    assert info["at_bound"] > 3
    for j, key in enumerate(features):
        v = model.get(key, 0.0)      # (a coefficient thresholded to 0 stays out of the file)
        assert lo[j] <= v <= hi[j], (key, v)
        assert v == (float(theta[j]) if abs(theta[j]) > 1e-4 or not lo[j] <= 0.0 <= hi[j] else 0.0), (key, v, theta[j])
    assert model[("g3", "t1")] == 0.05 and model[("(INTERCEPT)", "")] == float(theta[D])


@pytest.mark.gpu
def test_a_sweep_keeps_the_bounds_in_every_model(device_solver, tmp_path, monkeypatch):
    data, root, path, features, lo, hi = _stage_inputs(tmp_path)
    seen = []
    inner = fe.FixedEffectDeviceSolver.fit_sweep

    def fit_sweep(self, *a, select, **k):
        def watched(thetas):
            seen.extend(np.array(th) for th in thetas)
            return select(thetas)
        return inner(self, *a, select=watched, **k)
    monkeypatch.setattr(fe.FixedEffectDeviceSolver, "fit_sweep", fit_sweep)
    argv = chain.stage_argv(root, "global", chain.LOGISTIC, False, l2_grids={"global": "10,1"})
    chain.run_stage(argv + [f"--coefficient_constraints={path}"])
    assert len(seen) == 2 and not np.array_equal(seen[0], seen[1])
    for th in seen:
        assert np.all((lo <= th) & (th <= hi)) and th[7] == 0.05 and int(H.at_bound(th, lo, hi).sum()) > 3
    model = _read_model(os.path.join(root, "global", "models", "part-00000.avro"))
    assert model[("g3", "t1")] == 0.05 and all(lo[j] <= model.get(key, 0.0) <= hi[j] for j, key in enumerate(features))
