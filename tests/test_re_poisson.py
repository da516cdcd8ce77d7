"""CPU: --model_type=poisson_regression — the host path up to the solver (with a solver stand-in, as tests/test_re_linear.py uses one), the
label check, the options' loss code, the refusals, and the reference the GPU tests compare against: scipy's fmin_l_bfgs_b on the numpy
statement of the objective (re_poisson_helpers) held to a Newton minimiser, the variance restatement to a dense Hessian, the numpy
statement of poisson_loss to math.fsum, and the device's exp restated in C to long double."""
import dataclasses
import math
import os
import subprocess

import numpy as np
import pytest

from gdmix_amd import batch as batch_mod
from gdmix_amd import constants
from gdmix_amd import gdmix as cli
from gdmix_amd import metrics
from gdmix_amd import model as model_mod
from gdmix_amd import synthetic
from gdmix_amd.io import avro
from gdmix_amd.params import Params
from gdmix_amd.solver import LOSS_CODES, SolverOptions
from helpers import OracleSolverDouble, _Res
from oracle import oracle
import re_linear_helpers as H
import re_poisson_helpers as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def count_job_batch(E=60, seed=11):
    return synthetic.with_count_labels(H.small_job_batch(E=E, seed=seed, real=False), seed)


class ScipySolver(OracleSolverDouble):
    """Stands in for REDeviceSolver: packs with the oracle, solves every entity with scipy on the Poisson objective, records what reaches it."""
    seen = []

    def __init__(self, device=0):
        pass

    def solve(self, packed, opts, theta0=None, out=None):
        b = packed.batch
        type(self).seen.append(("solve", opts.to_c().loss, bool(opts.sum_loss), bool(b.binary_labels), b.to_wire()["y_width"], np.array(b.y, copy=True)))
        assert opts.loss_name() == "poisson"
        cp = packed.coef_ptr_host()
        kw = dict(l2=opts.l2, regularize_bias=opts.regularize_bias, has_intercept=opts.has_intercept, m=opts.m, max_iter=opts.max_iter, ftol=opts.ftol)
        ref = P.reference(b, packed.pk, kw, theta0, cp, entities=np.arange(b.E))
        theta = np.concatenate([ref["theta"][e] for e in range(b.E)])
        return _Res(dict(theta=theta, theta_thr=np.where(np.abs(theta) <= opts.threshold, 0.0, theta), variance=None, fval=ref["fval"],
                         gnorm=np.zeros(b.E), nit=ref["nit"].astype(np.int32), nfev=ref["nfev"].astype(np.int32), status=ref["status"].astype(np.int32)))

    def close(self):
        pass


@pytest.fixture
def stand_in(monkeypatch):
    ScipySolver.seen = []
    monkeypatch.setattr(model_mod, "REDeviceSolver", ScipySolver)
    monkeypatch.delenv("TF_CONFIG", raising=False)
    return ScipySolver


def test_params_and_constants_accept_poisson_regression():
    assert constants.POISSON_REGRESSION == "poisson_regression"
    p = Params.__from_argv__(H.job_argv("/tmp/x", model_type="poisson_regression"), error_on_unknown=False)
    assert p.model_type == "poisson_regression"
    with pytest.raises(AssertionError, match="must be in"):
        Params.__from_argv__(H.job_argv("/tmp/x", model_type="hinge"), error_on_unknown=False)


def test_solver_options_loss_code():
    assert LOSS_CODES == {"logistic": 0, "squared": 1, "poisson": 2}
    assert SolverOptions().to_c().loss == 0
    assert SolverOptions(linear=True).to_c().loss == 1 and SolverOptions(linear=True).loss_name() == "squared"      # linear=True still means squared
    assert SolverOptions(loss="squared").to_c().loss == 1 and SolverOptions(loss="logistic").to_c().loss == 0
    assert SolverOptions(loss="poisson").to_c().loss == 2
    with pytest.raises(ValueError, match="not both"):
        SolverOptions(linear=True, loss="poisson").to_c()
    with pytest.raises(ValueError, match="must be one of"):
        SolverOptions(loss="hinge").to_c()


def test_label_check_of_a_count_target():
    for good in ([0.0, 3.0, 2.5], [0.0], []):
        batch_mod.check_count_labels(np.array(good, np.float32))
    for bad in ([1.0, -1.0], [float("nan"), 2.0], [float("inf")], [-0.5]):
        with pytest.raises(ValueError, match="finite and >= 0"):
            batch_mod.check_count_labels(np.array(bad, np.float32))


def test_with_count_labels_is_seeded_and_real_valued():
    b = synthetic.make_batch(50, 12, 4, 64, seed=3, with_uid=False)
    c, c2, c3 = synthetic.with_count_labels(b, 7), synthetic.with_count_labels(b, 7), synthetic.with_count_labels(b, 8)
    assert c.binary_labels is False and c.y.dtype == np.float32 and np.array_equal(c.y, c2.y) and not np.array_equal(c.y, c3.y)
    assert np.all(c.y >= 0) and np.all(c.y == np.round(c.y)) and c.y.max() > 1 and c.val is b.val
    rng = np.random.default_rng([7, 0xC0])
    want = rng.poisson(np.exp(0.7 * b.y.astype(np.float64) + 0.3 * rng.standard_normal(b.N))).astype(np.float32)
    assert np.array_equal(c.y, want)


def test_cli_trains_poisson_regression_and_the_loss_code_reaches_the_solver(tmp_path, stand_in):
    """`gdmix.run` with --model_type=poisson_regression: the partition is read with its count labels (binary_labels False, y_width 4), the
    solver is asked for loss code 2 and sum_loss = 0, the model file carries scipy's coefficients and Photon-ML's PoissonRegressionModel
    class name, and the scores are written."""
    b = count_job_batch()
    root = str(tmp_path)
    H.write_job(root, b)
    cli.run(H.job_argv(root, model_type="poisson_regression"))
    solves = [s for s in stand_in.seen if s[0] == "solve"]
    assert solves and all(s[1:5] == (2, False, False, 4) for s in solves)
    assert np.array_equal(solves[0][5], b.y) and np.count_nonzero(b.y > 1) > 0
    recs = {r["modelId"]: r for r in avro.read_file(os.path.join(root, "models", "part-00000.avro"))}
    assert set(recs) == set(b.entity_ids)
    assert all(r["modelClass"] == "com.linkedin.photon.ml.supervised.regression.PoissonRegressionModel" for r in recs.values())
    pk = oracle.pack(b.ent_row_ptr, b.row_nnz_ptr, b.col_global)
    for e in (0, 7, b.E - 1):
        X, y, off, w = P.entity_sparse(b, pk, e, True)
        x = P.scipy_fit(P.objective(X, y, off, w, P.reg_vector(X.shape[1], 1.0, True, False)), np.zeros(X.shape[1]), 10, 100, 1e-12)[0]
        means = recs[b.entity_ids[e]]["means"]
        got = np.array([m["value"] for m in means])
        assert means[0]["name"] == "(INTERCEPT)" and np.allclose(got, x[np.abs(x) > 1e-4], rtol=1e-6, atol=1e-6)
    for d in ("trainingScores", "validationScores"):
        files = [os.path.join(r, f) for r, _, fs in os.walk(os.path.join(root, d)) for f in fs if f.endswith(".avro")]
        assert files and sum(len(list(avro.read_file(f))) for f in files) == b.N


def test_cli_refuses_a_negative_label(tmp_path, stand_in):
    b = count_job_batch(E=9)
    y = b.y.copy()
    y[4] = -1.0
    H.write_job(str(tmp_path), dataclasses.replace(b, y=y))
    with pytest.raises(ValueError, match="finite and >= 0"):
        cli.run(H.job_argv(str(tmp_path), model_type="poisson_regression"))
    assert not stand_in.seen


def test_l2_reg_weights_is_refused_in_both_stages(tmp_path, stand_in):
    from gdmix_amd import sweep
    b = count_job_batch(E=9)
    H.write_job(str(tmp_path), b)
    extra = ["--l2_reg_weights=0.1,1.0", f"--metric_output_dir={tmp_path}/metrics"]
    with pytest.raises(sweep.SweepError, match="poisson_regression"):
        cli.run(H.job_argv(str(tmp_path), model_type="poisson_regression", extra=extra))
    assert not stand_in.seen
    from gdmix_amd.fe_model import FixedEffectLRModelLBFGS
    md = tmp_path / "md.json"
    md.write_text('{"features": [{"name": "global", "dtype": "float", "shape": [8], "isSparse": true}], "labels": []}')
    argv = ["gdmix", "--stage=fixed_effect", "--action=train", "--model_type=poisson_regression", f"--metadata_file={md}", "--feature_bag=global",
            f"--output_model_dir={tmp_path}/fe", f"--training_data_dir={tmp_path}", f"--validation_data_dir={tmp_path}", "--l2_reg_weights=0.1,1.0",
            f"--metric_output_dir={tmp_path}/metrics", "--uid_column_name=uid", "--label_column_name=response", "--prediction_score_column_name=predictionScore",
            f"--training_score_dir={tmp_path}/ts", f"--validation_score_dir={tmp_path}/vs"]
    params = Params.__from_argv__(argv, error_on_unknown=False)
    fe = FixedEffectLRModelLBFGS(raw_model_params=argv, base_training_params=params)
    with pytest.raises(sweep.SweepError, match="poisson_regression"):
        fe.check_request({constants.NUM_WORKERS: 1}, constants.ACTION_TRAIN)


def test_an_unknown_model_type_is_still_refused(tmp_path, stand_in):
    H.write_job(str(tmp_path), count_job_batch(E=5))
    with pytest.raises(ValueError, match="detext"):
        cli.run(H.job_argv(str(tmp_path), model_type="detext"))
    from gdmix_amd import chain, fixed_effect
    with pytest.raises(ValueError, match="unknown model type"):
        fixed_effect.fit_options(True, 1.0, True, "detext", 10, 10, 1e-12)
    assert fixed_effect.fit_options(True, 1.0, True, "poisson_regression", 10, 10, 1e-12).to_c().loss == 2
    assert fixed_effect.fit_options(True, 1.0, True, "linear_regression", 10, 10, 1e-12).linear is True
    with pytest.raises(ValueError, match="the chain runs"):
        chain.run_chain(str(tmp_path / "c"), {}, model_type="detext")


def test_scipy_reference_against_a_newton_minimiser():
    """The reference itself: scipy's theta on 20 small entities against the Newton minimiser of the same objective, <= 1e-6 of the scale.
    scipy runs to the minimum here (pgtol 1e-10, ftol 1e-15): at the product's pgtol = 1e-5 it stops where the gradient allows 6e-5 of the
    scale, which says where L-BFGS-B stops, not whether (f, g) is the objective's."""
    b = synthetic.with_count_labels(synthetic.make_batch(20, 10, 4, 32, seed=2, random_weights=True, with_uid=False), 2)
    pk = oracle.pack(b.ent_row_ptr, b.row_nnz_ptr, b.col_global)
    worst = 0.0
    for e in range(b.E):
        X, y, off, w = P.entity_sparse(b, pk, e, True)
        Xd, yd, od, wd = H.entity_dense(b, pk, e, True)
        assert np.array_equal(np.asarray(X.todense()), Xd) and np.array_equal(y, yd) and np.array_equal(off, od) and np.array_equal(w, wd)
        reg = P.reg_vector(X.shape[1], 0.5, True, False)
        x, f, st, nit, nfev = P.scipy_fit(P.objective(X, y, off, w, reg), np.zeros(X.shape[1]), 10, 500, 1e-15, pgtol=1e-10)
        star = P.newton_minimiser(X, y, off, w, reg)
        worst = max(worst, float(np.max(np.abs(x - star)) / np.max(np.abs(star))))
        z = Xd @ x + off
        assert abs(f - (np.sum(w * (np.exp(z) - y * z)) + 0.5 * np.sum(reg * x * x)) / X.shape[0]) <= 1e-12 * max(1.0, abs(f))
    print(f"scipy against Newton on 20 entities: worst {worst:.3e}")
    assert worst <= 1e-6, worst


def test_variance_restatement_against_a_dense_hessian():
    b = synthetic.with_count_labels(synthetic.make_ragged_batch(12, seed=5, D=30, max_n=20, max_k=5), 5)
    pk = oracle.pack(b.ent_row_ptr, b.row_nnz_ptr, b.col_global)
    cp = np.asarray(pk["ent_feat_ptr"]) + np.arange(b.E + 1)
    theta = 0.1 * np.random.default_rng(1).standard_normal(int(cp[-1]))
    for rb in (True, False):
        kw = dict(l2=0.7, regularize_bias=rb, has_intercept=True)
        vs, vf = P.variance_numpy(b, pk, kw, 1, theta, cp), P.variance_numpy(b, pk, kw, 2, theta, cp)
        for e in range(b.E):
            X, _, off, w = H.entity_dense(b, pk, e, True)
            s = slice(cp[e], cp[e + 1])
            Hm = (X.T * (w * np.exp(X @ theta[s] + off))) @ X + np.diag(P.reg_vector(X.shape[1], 0.7, True, rb)) + 1e-12 * np.eye(X.shape[1])
            np.testing.assert_allclose(vs[s], 1.0 / np.diag(Hm), rtol=1e-12)
            np.testing.assert_allclose(vf[s], np.diag(np.linalg.inv(Hm)), rtol=1e-9)
            assert np.all(vf[s] >= vs[s] * (1 - 1e-9))


def test_poisson_loss_statement_against_fsum():
    rng = np.random.default_rng(9)
    s = (2.0 * rng.standard_normal(5000)).astype(np.float32)
    y = rng.poisson(2.0, 5000).astype(np.float32)
    t = metrics.poisson_loss_terms(s, y)
    want = math.fsum(math.exp(float(a)) - float(b) * float(a) for a, b in zip(s, y))
    assert abs(math.fsum(t) - want) <= 1e-15 * math.fsum(math.exp(float(a)) + abs(float(b) * float(a)) for a, b in zip(s, y))
    from gdmix_amd import chain
    assert abs(chain.poisson_loss(y, s) - want / 5000) <= 1e-12 * abs(want / 5000)
    assert metrics.metric_of_loss("poisson") == "poisson_loss" and metrics.metric_of_loss("squared") == "mse" and metrics.metric_of_loss("logistic") == "auc"


def test_evaluate_cli_takes_poisson_loss():
    from gdmix_amd import evaluate
    good = ["--metricsInputDir", "d", "--outputMetricFile", "f", "--labelColumnName", "response", "--predictionColumnName", "predictionScore", "--metricName"]
    assert evaluate.parse(good + ["poisson_loss"])["metricName"] == "poisson_loss"
    with pytest.raises(ValueError, match="Do not support metric rmse"):
        evaluate.parse(good + ["rmse"])


def test_device_exp_restated_in_c_against_long_double(tmp_path):
    """tools/exp_any_check.c restates csrc/re_device.hpp's exp_any and checks it against long double on the 4e6-point grid over
    [-745, 709.78]: <= 0.98 ulp on normal results (exp_neg's bar), the ends IEEE. Measured: 0.847 ulp."""
    exe = str(tmp_path / "exp_any_check")
    src = os.path.join(ROOT, "tools", "exp_any_check.c")
    subprocess.run([os.environ.get("CC", "cc"), "-O2", "-ffp-contract=off", "-o", exe, src, "-lm"], check=True)
    cp = subprocess.run([exe], capture_output=True, text=True)
    print(cp.stdout)
    assert cp.returncode == 0, cp.stdout
    # the restatement is the header's: same constants, same steps
    hdr = open(os.path.join(ROOT, "gdmix_amd", "csrc", "re_device.hpp")).read()
    body = hdr[hdr.index("double exp_any(double z)"):hdr.index("poisson_terms")]
    for piece in ("1.4426950408889634074", "6.93147180369123816490e-01", "1.90821492927058770002e-10", "1.0 / 6227020800.0", "r0 - r", "(int)kf"):
        assert piece in body and piece in open(src).read(), piece
