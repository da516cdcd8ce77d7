"""GPU: the fixed effect's Poisson loss (fit_stepping(model_type="poisson_regression"); include/gdmix_fe.h, "poisson") against scipy's
fmin_l_bfgs_b on the numpy statement of the SUM objective (re_poisson_helpers.objective, sum_loss=True), at tests/test_fixed_effect.py's
tolerances: REL_TOL after a projected-gradient stop, REL_TOL_FACTR after a FACTR stop. Both step forms, SIMPLE and FULL variances against
numpy at the returned coefficients, two workers against one, a neutral prior bit for bit against no prior."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import scipy.sparse as sp

from gdmix_amd import fixed_effect as fe
import re_poisson_helpers as P
from test_fixed_effect import rel_err, tol

# scipy alone, on the CPU: the small case stops on the projected gradient after 22 iterations at l2 = 20 (the REL_TOL bar, identical counts);
# the wide case stops on FACTR after 79 at l2 = 5 (the REL_TOL_FACTR bar: such a stop is decided at the objective's rounding level, and the
# counts may then differ by an iteration, as tests/test_oracle_scipy.py explains)
FIT = dict(has_intercept=True, l2=20.0, regularize_bias=False, max_iter=100, m=10, tolerance=1e-12)
FIT_WIDE = dict(FIT, l2=5.0)


def small_case():
    """600 samples x 8 non-zeros over 50 features, weights, offsets, count labels."""
    rng = np.random.default_rng(61)
    n, k, D = 600, 8, 50
    col = rng.integers(0, D, (n, k)).astype(np.int64).ravel()
    val = (0.4 * rng.standard_normal(n * k)).astype(np.float32)
    off = (0.3 * rng.standard_normal(n)).astype(np.float32)
    wt = (0.5 + rng.random(n)).astype(np.float32)
    w_star = 0.3 * rng.standard_normal(D)
    z = (val.astype(np.float64) * w_star[col]).reshape(n, k).sum(1) + off + 0.4
    y = rng.poisson(np.exp(z)).astype(np.float32)
    return np.arange(n + 1, dtype=np.int64) * k, col, val, y, off, wt, D


def wide_case():
    """20 000 samples x 6 non-zeros over 5 000 features: both passes span several blocks."""
    rng = np.random.default_rng(62)
    n, k, D = 20000, 6, 5000
    col = rng.integers(0, D, (n, k)).astype(np.int64).ravel()
    val = (0.4 * rng.standard_normal(n * k)).astype(np.float32)
    off = (0.3 * rng.standard_normal(n)).astype(np.float32)
    w_star = 0.3 * rng.standard_normal(D)
    z = (val.astype(np.float64) * w_star[col]).reshape(n, k).sum(1) + off
    y = rng.poisson(np.exp(z)).astype(np.float32)
    return np.arange(n + 1, dtype=np.int64) * k, col, val, y, off, None, D


def design(rp, col, val, D):
    X = sp.csr_matrix((val.astype(np.float64), col, rp), shape=(rp.size - 1, D))      # (duplicates of a cell are summed)
    return sp.hstack([X, sp.csr_matrix(np.ones((rp.size - 1, 1)))], format="csr")      # intercept last


def scipy_fixed_effect(case, fit=FIT):
    rp, col, val, y, off, wt, D = case
    X = design(rp, col, val, D)
    reg = np.full(D + 1, float(fit["l2"]))
    if not fit["regularize_bias"]:
        reg[-1] = 0.0
    w = np.ones(rp.size - 1) if wt is None else wt.astype(np.float64)
    fg = P.objective(X, y.astype(np.float64), off.astype(np.float64), w, reg, sum_loss=True)
    return P.scipy_fit(fg, np.zeros(D + 1), fit["m"], fit["max_iter"], fit["tolerance"]), X, w


def dense_variances(X, w, off, theta, fit, mode, case):
    """SIMPLE: the fixed effect's diagonal adds val^2 d PER ENTRY (gdmix_fe_hessian_diag; tests/test_fixed_effect.py states it the same way): a column
    repeated inside a row — the cases draw columns with replacement — counts once per entry, not as the summed cell. FULL: the dense X~' D X~ of the
    matrix with a row's repeated cells summed, as the reference's toarray() gives it."""
    d = w * np.exp(X @ theta + off)
    reg = np.full(theta.size, float(fit["l2"]) + 1e-12)
    if not fit["regularize_bias"]:
        reg[-1] -= fit["l2"]
    if mode == "SIMPLE":
        rp, col, val = case[0], case[1], case[2]
        rows = np.repeat(np.arange(rp.size - 1), np.diff(rp))
        H = np.concatenate([np.bincount(col, weights=val.astype(np.float64) ** 2 * d[rows], minlength=theta.size - 1), [d.sum()]])
        return 1.0 / (H + reg)
    H = np.asarray((X.T @ X.multiply(d[:, None])).todense()) + np.diag(reg)
    return np.diagonal(np.linalg.inv(H))


@pytest.mark.gpu
@pytest.mark.parametrize("fused", ["0", "1"])
@pytest.mark.parametrize("name", ["small", "wide"])
def test_fixed_effect_poisson_matches_scipy(device_solver, monkeypatch, name, fused):
    case, fit = (small_case(), FIT) if name == "small" else (wide_case(), FIT_WIDE)
    rp, col, val, y, off, wt, D = case
    monkeypatch.setenv("GDMIX_FE_FUSED_TAIL", fused)      # the three-launch step / the one-launch step
    s = fe.FixedEffectDeviceSolver(solver=device_solver)
    (x, f, st, nit, nfev), X, w = scipy_fixed_effect(case, fit)
    theta, info = s.fit_stepping(rp, col, val, y, D, offset=off, weight=wt, model_type=fe.POISSON_REGRESSION, **fit)
    err = rel_err(theta, x)
    print(f"{name} (fused tail {fused}): device status {int(info['status'])} nit {int(info['nit'])} nfev {int(info['nfev'])}; scipy {st} {nit} {nfev}; theta {err:.3e}, "
          f"fval {float(info['fval'])!r} vs {f!r}")
    assert int(info["status"]) == st
    if st != 1:
        assert (int(info["nit"]), int(info["nfev"])) == (nit, nfev)
    assert err <= tol(st), err
    assert abs(float(info["fval"]) - f) <= 1e-9 * abs(f)
    for mode in ("SIMPLE", "FULL"):
        th_v, info_v = s.fit_stepping(rp, col, val, y, D, offset=off, weight=wt, model_type=fe.POISSON_REGRESSION, variance_mode=mode, **fit)
        assert np.array_equal(th_v, theta)
        want = dense_variances(X, w, off.astype(np.float64), th_v, fit, mode, case)
        np.testing.assert_allclose(info_v["variances"], want, rtol=1e-7 if mode == "SIMPLE" else 1e-4)


@pytest.mark.gpu
def test_fixed_effect_poisson_neutral_prior_and_label_check(device_solver):
    rp, col, val, y, off, wt, D = small_case()
    s = fe.FixedEffectDeviceSolver(solver=device_solver)
    kw = dict(offset=off, weight=wt, model_type=fe.POISSON_REGRESSION, **FIT)
    theta, info = s.fit_stepping(rp, col, val, y, D, **kw)
    th_p, info_p = s.fit_stepping(rp, col, val, y, D, prior=(np.zeros(D + 1), np.ones(D + 1)), **kw)
    assert np.array_equal(th_p, theta) and (info_p["nit"], info_p["nfev"], info_p["status"]) == (info["nit"], info["nfev"], info["status"])
    assert float(info_p["fval"]) == float(info["fval"])
    bad = y.copy()
    bad[5] = -1.0
    with pytest.raises(ValueError, match="finite and >= 0"):
        s.fit_stepping(rp, col, val, bad, D, **kw)


@pytest.mark.gpu
def test_fixed_effect_poisson_two_workers_against_one(device_solver, tmp_path):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    env.pop("TF_CONFIG", None)
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2", "--master-addr", "127.0.0.1", "--master-port", "29633",
           os.path.join(root, "tests", "_fe_poisson_dist_worker.py"), str(tmp_path)]
    subprocess.run(cmd, check=True, env=env, timeout=600, cwd=root)
    a, b = json.load(open(tmp_path / "result.json"))
    assert a["theta"] == b["theta"] and a["variances"] == b["variances"] and a["status"] == b["status"] and a["nit"] == b["nit"]      # replicated step
    rp, col, val, y, off, wt, D = small_case()
    s = fe.FixedEffectDeviceSolver(solver=device_solver)
    theta, info = s.fit_stepping(rp, col, val, y, D, offset=off, weight=wt, model_type=fe.POISSON_REGRESSION, variance_mode="SIMPLE", **FIT)
    err = rel_err(np.array(a["theta"]), theta)
    print(f"two workers ({a['backend']}) against one: theta {err:.3e}, status {a['status']} / {int(info['status'])}, nit {a['nit']} / {int(info['nit'])}")
    assert err <= tol(a["status"]) * 10, err      # (the bar of test_fixed_effect.py's two-worker test: the shards' sums are added in another order)
    np.testing.assert_allclose(a["variances"], info["variances"], rtol=1e-7)
