"""Fixed effect, incremental training on the device (include/gdmix_fe.h, "incremental training"; csrc/fe_solve.hip) against the numpy
restatement of tests/fe_prior_helpers.py: theta* is Newton's minimiser of the prior-centred objective in fp64.

The bar on the coefficients is max_j |theta_j - theta*_j| / s_j <= 1e-5: the fit stops on |grad_phi|_inf <= pgtol = 1e-5, the Hessian in
phi is at least l2 = 10 on every regularised coefficient, so the distance to the minimiser is of the order of 1e-6 prior standard
deviations (scipy's L-BFGS-B leaves 4.4e-7 on these cases: tests/test_fe_prior_host.py)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import fe_prior_helpers as fh
from gdmix_amd import fixed_effect as fe
from gdmix_amd.solver import GdmixReError

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
BAR = 1e-5
FIT = dict(l2=fh.L2, tolerance=1e-15, max_iter=1000)


def shard(c):
    return c.row_nnz_ptr, c.col, c.val, c.y


def kw(c, rb, **more):
    return dict(offset=c.offset, weight=c.weight, has_intercept=bool(c.ic), regularize_bias=rb,
                model_type=fe.LINEAR_REGRESSION if c.linear else fe.LOGISTIC_REGRESSION, **FIT, **more)


def s_units(c, theta, star, rb):
    return float(np.max(np.abs(theta - star) / fh.scale(c, rb)))


def bits(x):
    return np.ascontiguousarray(x, np.float64).view(np.int64)


# ---- 1. the fit -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rb", [True, False])
@pytest.mark.parametrize("linear", [False, True])
@pytest.mark.parametrize("shape", fh.SHAPES)
def test_fit_reaches_the_minimiser_of_the_prior_centred_objective(device_solver, shape, linear, rb):
    c, star = fh.case_and_minimiser(7, shape, linear, rb)
    s = fe.FixedEffectDeviceSolver(solver=device_solver)
    theta, info = s.fit_stepping(*shard(c), c.D, prior=(c.mu, c.v), **kw(c, rb))
    err = s_units(c, theta, star, rb)
    print(f"n={c.n} linear={linear} regularize_bias={rb}: status={info['status']} nit={info['nit']} nfev={info['nfev']} "
          f"gnorm={info['gnorm']:.3g} max |theta - theta*| / s = {err:.3g}")
    assert info["status"] in (0, 1)                                   # a convergence stop
    assert err <= BAR
    j = np.arange(c.D - c.absent, c.D)                                # columns no sample touches: the prior mean, exactly
    assert np.array_equal(theta[j], c.mu[j])
    f_star = fh.objective(c, star, fh.L2, rb, hessian=False)[0]
    assert abs(info["fval"] - f_star) <= 1e-9 * abs(f_star)           # fval is F
    g_phi = fh.scale(c, rb) * fh.objective(c, theta, fh.L2, rb, hessian=False)[1]
    np.testing.assert_allclose(info["gnorm"], np.max(np.abs(g_phi)), rtol=1e-3, atol=1e-9)       # gnorm is |grad_phi|_inf


# ---- 2. a neutral prior is no prior --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fused", ["1", "0"])
@pytest.mark.parametrize("linear", [False, True])
def test_a_neutral_prior_gives_the_bits_of_no_prior(device_solver, monkeypatch, linear, fused):
    monkeypatch.setenv("GDMIX_FE_FUSED_TAIL", fused)                   # the one-launch step, the three-launch step
    c = fh.case(8, *fh.SHAPES[1], linear)
    s = fe.FixedEffectDeviceSolver(solver=device_solver)
    for rb in (True, False):
        plain, pi = s.fit_stepping(*shard(c), c.D, **kw(c, rb))
        neutral, ni = s.fit_stepping(*shard(c), c.D, prior=(np.zeros(c.D + 1), np.ones(c.D + 1)), **kw(c, rb))
        assert np.array_equal(bits(plain), bits(neutral))
        assert (pi["nit"], pi["nfev"], pi["status"]) == (ni["nit"], ni["nfev"], ni["status"])
        assert pi["fval"] == ni["fval"] and pi["gnorm"] == ni["gnorm"]
        assert pi["nit"] > 5


# ---- 3. set_prior, restart, and back -----------------------------------------------------------------------------------------------
def test_set_prior_restart_and_removal(device_solver):
    c, star = fh.case_and_minimiser(7, fh.SHAPES[0], False, True)
    s = fe.FixedEffectDeviceSolver(solver=device_solver)
    t = device_solver.torch
    k = kw(c, True)
    opts = fe.fit_options(True, k["l2"], True, k["model_type"], k["max_iter"], 10, k["tolerance"])
    first, fi = s.fit_stepping(*shard(c), c.D, prior=(c.mu, c.v), **k)                       # create + set_prior + solve
    plain, pi = s.fit_stepping(*shard(c), c.D, **k)
    fit = fe._SteppingFit(device_solver, opts, *shard(c), c.D, c.offset, c.weight, None, None, False, None, prior=(c.mu, c.v))
    try:
        a, ai = fit.run()
        assert np.array_equal(bits(a), bits(first))
        for theta0 in (None, t.from_numpy(c.mu.copy()).to(device_solver.device)):          # theta0 is in theta units: mu is phi = 0
            fit.prob.restart(opts, theta0)
            b, bi = fit.run()
            assert np.array_equal(bits(b), bits(first))
            assert (bi["nit"], bi["nfev"], bi["status"], bi["fval"]) == (fi["nit"], fi["nfev"], fi["status"], fi["fval"])
        # a start point away from the prior mean: another path to the same minimiser
        fit.prob.restart(opts, t.zeros(c.D + 1, dtype=t.float64, device=device_solver.device))
        z, zi = fit.run()
        assert zi["status"] in (0, 1) and s_units(c, z, star, True) <= BAR
        # a scale that is not finite and > 0 is refused, and the problem keeps the prior it has
        mean_dev = t.from_numpy(c.mu.copy()).to(device_solver.device)
        for bad in (0.0, -1.0, float("nan"), float("inf")):
            sc = np.sqrt(c.v)
            sc[c.D - 3] = bad
            with pytest.raises(GdmixReError, match="finite and > 0"):
                fit.prob.set_prior(mean_dev, t.from_numpy(sc).to(device_solver.device))
        with pytest.raises(GdmixReError):
            fit.prob.set_prior(mean_dev, None)
        fit.prob.restart(opts, None)
        assert np.array_equal(bits(fit.run()[0]), bits(first))
        # NULL, NULL: the plain problem again
        fit.prob.set_prior(None, None)
        p, ppi = fit.run()
        assert np.array_equal(bits(p), bits(plain))
        assert (ppi["nit"], ppi["nfev"], ppi["status"], ppi["fval"]) == (pi["nit"], pi["nfev"], pi["status"], pi["fval"])
        # ... and a prior installed on a problem that has already solved without one
        mu, sc = fe.prior_vectors(c.mu, c.v, c.D, 1, False, True)
        fit.prob.set_prior(t.from_numpy(mu).to(device_solver.device), t.from_numpy(sc).to(device_solver.device))
        assert np.array_equal(bits(fit.run()[0]), bits(first))
    finally:
        fit.prob.close()


# ---- 4. no intercept; no feature bag -----------------------------------------------------------------------------------------------
def test_model_without_an_intercept(device_solver):
    c, star = fh.case_and_minimiser(9, fh.SHAPES[0], False, False, has_intercept=False)
    s = fe.FixedEffectDeviceSolver(solver=device_solver)
    theta, info = s.fit_stepping(*shard(c), c.D, prior=(c.mu, c.v), **kw(c, False))
    assert theta.shape == (c.D,) and info["status"] in (0, 1)
    assert s_units(c, theta, star, False) <= BAR
    j = np.arange(c.D - c.absent, c.D)
    assert np.array_equal(theta[j], c.mu[j])


@pytest.mark.parametrize("rb", [True, False])
def test_intercept_only_model(device_solver, rb):
    c = fh.intercept_only(fh.case(9, *fh.SHAPES[0], False))
    star = fh.newton(c, fh.L2, rb)
    s = fe.FixedEffectDeviceSolver(solver=device_solver)
    theta, info = s.fit_stepping(np.zeros(c.n + 1, np.int64), [], [], c.y, 1, dummy=True, prior=(c.mu, c.v), variance_mode="SIMPLE", **kw(c, rb))
    assert theta.shape == (1,) and info["status"] in (0, 1)
    assert s_units(c, theta, star, rb) <= BAR
    want = fh.variances(c, theta, fh.L2, rb, full=False)
    np.testing.assert_allclose(info["variances"], want, rtol=1e-8)


# ---- 5. variances ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rb", [True, False])
@pytest.mark.parametrize("mode,host_max", [("SIMPLE", None), ("FULL", None), ("FULL", 0)])
def test_variances_are_the_posteriors(device_solver, monkeypatch, mode, host_max, rb):
    """SIMPLE, FULL on the host, and FULL by the dense device route (the host limit set to 0), at P = 301."""
    if host_max is not None:
        monkeypatch.setattr(fe, "FULL_VARIANCE_HOST_MAX", host_max)
        monkeypatch.setattr(device_solver, "variance_full", None)      # the one-worker shortcut knows no prior: it must not be taken
    c, star = fh.case_and_minimiser(7, fh.SHAPES[0], False, rb)
    s = fe.FixedEffectDeviceSolver(solver=device_solver)
    theta, info = s.fit_stepping(*shard(c), c.D, prior=(c.mu, c.v), variance_mode=mode, **kw(c, rb))
    assert s_units(c, theta, star, rb) <= BAR
    want = fh.variances(c, theta, fh.L2, rb, full=(mode == "FULL"))
    got = info["variances"]
    print(f"{mode} host_max={host_max} regularize_bias={rb}: max relative error {np.max(np.abs(got / want - 1.0)):.3g}")
    np.testing.assert_allclose(got, want, rtol=1e-8)


# ---- 6. two workers -------------------------------------------------------------------------------------------------------------------
def test_two_workers_install_the_same_prior(tmp_path):
    root = os.path.dirname(HERE)
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    env.pop("TF_CONFIG", None)
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2", "--master-addr", "127.0.0.1",
           "--master-port", "29627", os.path.join(root, "tests", "_fe_prior_dist_worker.py"), str(tmp_path)]
    subprocess.run(cmd, check=True, env=env, timeout=300, cwd=root)
    res = json.load(open(tmp_path / "result.json"))
    assert len(res) == 2
    a, b = res
    assert a["theta"] == b["theta"] and a["variances"] == b["variances"] and (a["status"], a["nit"], a["nfev"]) == (b["status"], b["nit"], b["nfev"])
    from _fe_prior_dist_worker import SEED, SHAPE
    c, star = fh.case_and_minimiser(SEED, SHAPE, False, True)
    theta = np.array(a["theta"])
    assert a["status"] in (0, 1)
    assert s_units(c, theta, star, True) <= BAR                        # theta* of the WHOLE data set
    j = np.arange(c.D - c.absent, c.D)
    assert np.array_equal(theta[j], c.mu[j])
    np.testing.assert_allclose(a["variances"], fh.variances(c, theta, fh.L2, True, full=False), rtol=1e-8)


# ---- 7. two days through the command line -------------------------------------------------------------------------------------------
def _write_day(root, name, c):
    from gdmix_amd.io import tfrecord
    recs = []
    for i in range(c.n):
        a, b = i * c.k, (i + 1) * c.k
        recs.append(tfrecord.encode_example({
            "uid": ("int64", [i]), "offset": ("float", [float(c.offset[i])]), "weight": ("float", [float(c.weight[i])]),
            "response": ("int64", [int(c.y[i])]), "global_indices": ("int64", c.col[a:b]), "global_values": ("float", c.val[a:b])}))
    os.makedirs(os.path.join(root, name), exist_ok=True)
    tfrecord.write_records(os.path.join(root, name, "part-00000.tfrecord"), recs)


def _argv(root, day, model_dir, tag, extra):
    for d in (model_dir, os.path.join(root, "ts_" + tag), os.path.join(root, "vs_" + tag)):
        os.makedirs(d, exist_ok=True)
    return ["gdmix", "--stage=fixed_effect", "--action=train", "--model_type=logistic_regression", "--uid_column_name=uid",
            "--label_column_name=response", "--weight_column_name=weight", "--prediction_score_column_name=predictionScore",
            f"--training_data_dir={os.path.join(root, day)}", f"--metadata_file={os.path.join(root, 'meta.json')}",
            f"--output_model_dir={model_dir}", f"--training_score_dir={os.path.join(root, 'ts_' + tag)}",
            f"--validation_score_dir={os.path.join(root, 'vs_' + tag)}", "--feature_bag=global", f"--feature_file={os.path.join(root, 'features.csv')}",
            f"--l2_reg_weight={fh.L2}", "--has_intercept=True", "--regularize_bias=True", "--num_of_lbfgs_iterations=1000",
            "--lbfgs_tolerance=1e-15", "--fixed_effect_variance_mode=simple"] + list(extra)


def _model(path, D):
    from gdmix_amd.io import avro
    recs = list(avro.read_file(path))
    assert len(recs) == 1

    def vec(triples):
        out = np.zeros(D + 1)
        for m in triples:
            out[D if m["name"] == "(INTERCEPT)" else int(m["name"][1:])] = m["value"]
        return out
    return vec(recs[0]["means"]), vec(recs[0]["variances"])


# Day 2's model file WITHOUT the flag as the commit before this feature wrote it: its code ran this test's day 1 (cold) and day 2 (warm start)
# on the same seeded data and flags, with the Avro sync marker pinned as below, on an MI355X; the file is that run's part-00000.avro.
GOLDEN_DAY2_PLAIN = os.path.join(HERE, "golden", "fe_prior_day2_without_the_flag.avro")


def test_two_days_through_the_command_line(tmp_path, monkeypatch):
    import shutil
    from gdmix_amd import gdmix
    from gdmix_amd.io import avro as avro_mod
    from prior_helpers import usable

    class PinnedOs:             # the Avro sync marker is os.urandom(16): pinned inside the writer's module, so that equal files are equal bytes
        urandom = staticmethod(lambda n: b"\x07" * n)

        def __getattr__(self, k):
            return getattr(os, k)
    monkeypatch.setattr(avro_mod, "os", PinnedOs())
    root = str(tmp_path)
    n, k, D, absent = fh.SHAPES[0]
    day1, day2 = fh.case(7, n, k, D, absent, False), fh.case(8, n, k, D, absent, False)
    md = {"features": [{"name": "global", "dtype": "float", "shape": [D], "isSparse": True},
                       {"name": "offset", "dtype": "float", "shape": [], "isSparse": False},
                       {"name": "weight", "dtype": "float", "shape": [], "isSparse": False},
                       {"name": "uid", "dtype": "long", "shape": [], "isSparse": False}],
          "labels": [{"name": "response", "dtype": "int", "shape": [], "isSparse": False}]}
    json.dump(md, open(os.path.join(root, "meta.json"), "w"))
    with open(os.path.join(root, "features.csv"), "w") as f:
        f.write("".join(f"f{i},\n" for i in range(D)))
    _write_day(root, "day1", day1)
    _write_day(root, "day2", day2)
    models1 = os.path.join(root, "models_day1")
    gdmix.run(_argv(root, "day1", models1, "d1", []))                  # day 1: cold, SIMPLE variances
    inc, warm, warm_false = (os.path.join(root, x) for x in ("models_inc", "models_warm", "models_warm_false"))
    for d in (inc, warm, warm_false):
        shutil.copytree(models1, d)
    gdmix.run(_argv(root, "day2", inc, "inc", ["--incremental_training=True"]))
    gdmix.run(_argv(root, "day2", warm, "warm", []))
    gdmix.run(_argv(root, "day2", warm_false, "warmf", ["--incremental_training=False"]))
    read = lambda d: open(os.path.join(d, "part-00000.avro"), "rb").read()
    # without the flag: byte for byte the file the code before this feature wrote for these two days (recorded from it), and the flag
    # set to False is no flag
    assert read(warm) == open(GOLDEN_DAY2_PLAIN, "rb").read()
    assert read(warm) == read(warm_false) and read(warm) != read(inc)
    # with it: theta* of day 2's data under day 1's written (thresholded) means and variances
    mu, var = _model(os.path.join(models1, "part-00000.avro"), D)
    assert np.count_nonzero(mu) > D // 2 and np.count_nonzero(var) == np.count_nonzero(mu)
    c = fh.with_prior(day2, mu, [usable(x) for x in var])
    star = fh.newton(c, fh.L2, True)
    got, got_var = _model(os.path.join(inc, "part-00000.avro"), D)
    kept = got != 0.0
    s = fh.scale(c, True)
    worst = float(np.max(np.abs(got - star)[kept] / s[kept]))
    print(f"two days: {int(kept.sum())} of {D + 1} coefficients written, max |theta - theta*| / s = {worst:.3g}")
    assert worst <= BAR
    assert np.all(np.abs(star[~kept]) <= 1e-4 + BAR * s[~kept])          # what the threshold dropped
    j = np.arange(D - absent, D)                                       # no sample of either day: day 1 left them at 0, below the threshold
    assert not kept[j].any()
    want_var = fh.variances(c, got, fh.L2, True, full=False)
    np.testing.assert_allclose(got_var[kept], want_var[kept], rtol=1e-8)
    # the forgetting this replaces: the warm start's model is another model — four orders of magnitude above the bar away from the posterior
    warm_theta, _ = _model(os.path.join(warm, "part-00000.avro"), D)
    assert np.max(np.abs(warm_theta - star) / s) > 1e4 * BAR
