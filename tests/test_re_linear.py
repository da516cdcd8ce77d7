"""CPU: --model_type=linear_regression for the random effect — the host path up to the solver (with a solver stand-in, as tests/test_host.py
uses one) and the definition of the per-entity objective, pinned to the closed-form ridge solution."""
import dataclasses
import os

import numpy as np
import pytest

from gdmix_amd import gdmix as cli
from gdmix_amd import model as model_mod
from gdmix_amd import synthetic
from gdmix_amd.io import avro
from helpers import OracleSolverDouble, _Res
from oracle import oracle
import re_linear_helpers as H


class RecordingSolver(OracleSolverDouble):
    """The oracle stand-in of tests/test_host.py that also hands `linear` on and records what reaches it."""
    seen = []

    def __init__(self, device=0):
        pass

    def pack(self, batch, has_intercept=True):
        type(self).seen.append(("pack", bool(batch.binary_labels), batch.to_wire()["y_width"], np.array(batch.y, copy=True)))
        return super().pack(batch, has_intercept)

    def solve(self, packed, opts, theta0=None, out=None):
        type(self).seen.append(("solve", bool(opts.linear), bool(opts.sum_loss)))
        b = packed.batch
        o = oracle.make_opts(l2=opts.l2, regularize_bias=opts.regularize_bias, has_intercept=opts.has_intercept, m=opts.m, max_iter=opts.max_iter,
                             ftol=opts.ftol, variance_mode=0, threshold=opts.threshold, linear=opts.linear, sum_loss=opts.sum_loss)
        return _Res(oracle.solve(packed.pk, b.val, b.y, b.offset, b.weight, o, theta0=theta0))

    def close(self):
        pass


@pytest.fixture
def stand_in(monkeypatch):
    RecordingSolver.seen = []
    monkeypatch.setattr(model_mod, "REDeviceSolver", RecordingSolver)
    monkeypatch.delenv("TF_CONFIG", raising=False)
    return RecordingSolver


def test_cli_trains_linear_regression_and_float_labels_reach_the_solver(tmp_path, stand_in):
    """`gdmix.run` with --stage=random_effect --model_type=linear_regression no longer stops at the model-type check: the partition is read
    with its real-valued labels (binary_labels False, wire form y_width 4), the solver is asked for linear=True and sum_loss=False, the
    model file holds the oracle's coefficients, and scoring after training stays on (the scores are the next coordinate's offsets)."""
    b = H.small_job_batch()
    root = str(tmp_path)
    H.write_job(root, b)
    cli.run(H.job_argv(root))
    packs = [s for s in stand_in.seen if s[0] == "pack"]
    solves = [s for s in stand_in.seen if s[0] == "solve"]
    assert solves and all(s[1:] == (True, False) for s in solves)
    assert packs and packs[0][1] is False and packs[0][2] == 4
    assert np.array_equal(packs[0][3], b.y) and np.count_nonzero((b.y != 0) & (b.y != 1)) > b.N // 2
    # the model: the oracle's thresholded coefficients per entity
    pk = oracle.pack(b.ent_row_ptr, b.row_nnz_ptr, b.col_global)
    ref = oracle.solve(pk, b.val, b.y, b.offset, None, oracle.make_opts(l2=1.0, regularize_bias=False, linear=True))
    recs = {r["modelId"]: r for r in avro.read_file(os.path.join(root, "models", "part-00000.avro"))}
    assert set(recs) == set(b.entity_ids)
    fp = pk["ent_feat_ptr"]
    for e in (0, 7, b.E - 1):
        means = recs[b.entity_ids[e]]["means"]
        want = ref["theta_thr"][fp[e] + e:fp[e + 1] + e + 1]
        got = np.array([m["value"] for m in means])
        assert means[0]["name"] == "(INTERCEPT)" and np.allclose(got, want[want != 0.0], rtol=1e-6, atol=1e-6)
    # scores: x . theta + offset, for the training and the validation data
    for d in ("trainingScores", "validationScores"):
        files = [os.path.join(r, f) for r, _, fs in os.walk(os.path.join(root, d)) for f in fs if f.endswith(".avro")]
        assert files and sum(len(list(avro.read_file(f))) for f in files) == b.N


def test_logistic_regression_still_refuses_a_label_of_one_half(tmp_path, stand_in):
    b = H.small_job_batch()
    y = (b.y > 1.0).astype(np.float32)
    y[3] = 0.5
    H.write_job(str(tmp_path), dataclasses.replace(b, y=y))      # (binary_labels False: the float label list keeps the 0.5)
    with pytest.raises(AssertionError, match="labels must be 0 or 1"):
        cli.run(H.job_argv(str(tmp_path), model_type="logistic_regression"))
    assert not [s for s in stand_in.seen if s[0] == "solve"]


@pytest.mark.parametrize("native", [True, False])
def test_readers_take_the_label_check_as_an_argument(tmp_path, native):
    """grouped reads refuse a non-binary label unless told that labels are real-valued; the default is the refusal."""
    from gdmix_amd.io import native_reader
    from gdmix_amd.io.grouped_reader import read_grouped_partition
    from gdmix_amd.io.metadata import DatasetMetadata
    import json
    if native and not native_reader.available():
        pytest.skip("libgdmix_io.so is not built")
    b = H.small_job_batch(E=9)
    p = H.write_job(str(tmp_path), b)
    md = DatasetMetadata(json.load(open(os.path.join(p, "metadata", "tensor_metadata.json"))))
    d = os.path.join(p, "trainingData", "active", "partitionId=0")
    args = (d, md, "user_id", "per_user", "offset", "uid", "response")
    with pytest.raises(AssertionError, match="labels must be 0 or 1"):
        read_grouped_partition(*args, native=native)
    for wire in (False, True):
        got = read_grouped_partition(*args, native=native, wire=wire, binary_labels=False)
        assert got.binary_labels is False and np.array_equal(got.y, b.y) and got.to_wire()["y_width"] == 4


def test_an_unknown_model_type_is_still_refused(tmp_path, stand_in):
    H.write_job(str(tmp_path), H.small_job_batch(E=5))
    with pytest.raises(ValueError, match="logistic_regression and linear_regression"):
        cli.run(H.job_argv(str(tmp_path), model_type="detext"))      # (the one other model type Params accepts)
    with pytest.raises(ValueError, match="logistic_regression and linear_regression"):
        model_mod.RandomEffectLRLBFGSModel(H.job_argv(str(tmp_path)), base_training_params=type("P", (), {"model_type": "detext"})())


def test_oracle_minimiser_is_the_closed_form_ridge_solution():
    """Pins the definition: f = (1/n) (sum_i w_i (y_i - z_i)^2 + (l2/2) |theta|^2) with regularize_bias=True. The oracle with linear=True,
    sum_loss=False, threshold 0 and ftol 1e-15 on seeded small entities; for those that stop on the projected gradient (status 0), theta is
    within (n / l2) sqrt(p) gnorm of numpy's fp64 normal-equation solution: the Hessian (1/n)(2 X~'WX~ + l2 I) is at least (l2/n) I, so
    |theta - theta*|_2 <= (n / l2) |g|_2 <= (n / l2) sqrt(p) |g|_inf. No tolerance is chosen."""
    checked = 0
    for seed, l2, weights in ((1, 1.0, False), (2, 0.1, True), (3, 10.0, True), (4, 0.5, False)):
        b = synthetic.with_real_labels(synthetic.make_batch(40, 10, 4, 32, seed=seed, random_weights=weights, with_uid=False), seed)
        pk = oracle.pack(b.ent_row_ptr, b.row_nnz_ptr, b.col_global)
        kw = dict(l2=l2, regularize_bias=True, has_intercept=True, m=10, max_iter=500, ftol=1e-15, threshold=0.0)
        res = oracle.solve(pk, b.val, b.y, b.offset, b.weight, oracle.make_opts(linear=True, sum_loss=False, **kw))
        fp = pk["ent_feat_ptr"]
        for e in np.flatnonzero(res["status"] == 0):
            X, y, off, w = H.entity_dense(b, pk, e, True)
            n, p = X.shape
            star = H.ridge_closed_form(X, y, off, w, l2, True, True)
            theta = res["theta"][fp[e] + e:fp[e + 1] + e + 1]
            assert np.linalg.norm(theta - star) <= (n / l2) * np.sqrt(p) * res["gnorm"][e], (seed, int(e))
            # and the objective value is the definition's
            z = X @ theta + off
            f = (np.sum(w * (y - z) ** 2) + 0.5 * l2 * np.sum(theta ** 2)) / n
            assert abs(f - res["fval"][e]) <= 1e-12 * max(1.0, abs(f))
            checked += 1
    assert checked >= 100, checked


def test_variance_restatement_against_a_dense_hessian():
    """The numpy restatement of the two variance modes with D = 2 w: SIMPLE is the reciprocal diagonal, FULL the diagonal of the inverse,
    of the Hessian of n f — an unregularised intercept carries no l2 — and neither is divided by n."""
    b = synthetic.with_real_labels(synthetic.make_ragged_batch(12, seed=5, D=30, max_n=20, max_k=5), 5)
    pk = oracle.pack(b.ent_row_ptr, b.row_nnz_ptr, b.col_global)
    for rb in (True, False):
        kw = dict(l2=0.7, regularize_bias=rb, has_intercept=True)
        vs, vf = H.variance_numpy(b, pk, kw, 1), H.variance_numpy(b, pk, kw, 2)
        fp = pk["ent_feat_ptr"]
        for e in range(b.E):
            X, _, _, w = H.entity_dense(b, pk, e, True)
            Hm = 2.0 * (X.T * w) @ X + np.diag(H.reg_vector(X.shape[1], 0.7, True, rb)) + 1e-12 * np.eye(X.shape[1])
            s = slice(fp[e] + e, fp[e + 1] + e + 1)
            np.testing.assert_allclose(vs[s], 1.0 / np.diag(Hm), rtol=1e-12)
            np.testing.assert_allclose(vf[s], np.diag(np.linalg.inv(Hm)), rtol=1e-9)
            assert np.all(vf[s] >= vs[s] * (1 - 1e-9))      # diag(H^-1) >= 1 / diag(H) for an SPD matrix
