"""GPU: down-sampling of the fixed effect's training shard (csrc/re_downsample.hip; include/gdmix_re.h, "down-sampling").

The compaction bit for bit against the numpy statement (gdmix_amd/downsample.py: apply_host), every output array and kept_rows; a fit on
the sample against the fit of apply_host's arrays, bit for bit; one logistic fit against scipy on the filtered, re-weighted data at
tests/test_fixed_effect.py's tolerance; the sweep; the empty outcome; the stage through the command line; two workers against one."""
import ctypes as C
import functools
import json
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest
import scipy.sparse as sp

from gdmix_amd import chain
from gdmix_amd import downsample as ds
from gdmix_amd import fixed_effect as fe
from gdmix_amd import solver as S
from gdmix_amd.batch import RawBatch
import re_poisson_helpers as P
from test_fe_sweep_host import avro_bytes
from test_fixed_effect import rel_err, tol

HERE = os.path.dirname(os.path.abspath(__file__))
N_ROWS = 70_001      # 35 chunks of 2 048 rows: the scans span more than one workgroup, the last chunk holds a single row
LONG_ROWS = ((0, 65), (N_ROWS // 2, 5000), (N_ROWS - 1, 1025))      # first, mid-batch, last
SEED = 20240603


# ---- the compaction -------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _rows(empty_rows=False):
    """70 001 rows of 0 .. 8 non-zeros and three long ones; uids of either sign, one of them twice; labels 10 % positive."""
    rng = np.random.default_rng(71)
    n = N_ROWS
    k = rng.integers(0, 9, n)
    for i, z in LONG_ROWS:
        k[i] = z
    if empty_rows:
        k[:] = 0
    rp = np.concatenate([[0], np.cumsum(k)]).astype(np.int64)
    col = rng.integers(0, 1 << 40, rp[-1]).astype(np.int64)      # (beyond int32: the copy moves all 64 bits)
    val = rng.standard_normal(rp[-1]).astype(np.float32)
    uid = rng.integers(-2 ** 63, 2 ** 63 - 1, n, dtype=np.int64)
    uid[5], uid[6], uid[7] = -1, -2 ** 63, 0
    uid[40_000] = uid[123]                                        # a duplicated uid: one fate
    y = (rng.random(n) < 0.1).astype(np.float32)
    y[[0, N_ROWS - 1]] = 1.0                                      # (the first and the last row, both long, survive every negatives_only case)
    off = rng.standard_normal(n).astype(np.float32)
    w = (0.25 + rng.random(n)).astype(np.float32)
    return rp, col, val, uid, y, off, w


def _entities(E, kept):
    """ent_row_ptr [E + 1]: for E = 37 with a one-row entity that loses its row (when the mask drops any), an entity without rows, and
    cuts that are no multiple of anything."""
    if E == 1:
        return np.array([0, N_ROWS], np.int64)
    rng = np.random.default_rng(72)
    dropped = np.flatnonzero(~kept[1000:-1000]) + 1000
    lone = int(dropped[dropped.size // 2]) if dropped.size else 33_333
    cuts = set([lone, lone + 1])
    while len(cuts) < E - 2:
        cuts.add(int(rng.integers(1, N_ROWS)))
    erp = np.array([0] + sorted(cuts) + [sorted(cuts)[-1], N_ROWS], np.int64)      # (the repeated cut: an entity without rows)
    assert erp.size == E + 1 and np.all(np.diff(erp) >= 0)
    return erp


def _run(device_solver, erp, rp, col, val, y, off, w, uid, rate, seed, neg_only):
    b = RawBatch(ent_row_ptr=erp, row_nnz_ptr=rp, col_global=col, val=val, y=y, offset=off, weight=w, uid=np.arange(rp.size - 1, dtype=np.int64),
                 entity_ids=[str(e) for e in range(erp.size - 1)], has_label=True, binary_labels=True)
    out, counts = device_solver.downsample(device_solver.upload(b), uid, rate, seed, negatives_only=neg_only)
    device_solver.torch.cuda.synchronize()
    return out, counts


def _compare(out, counts, want, y, kept):
    assert (out["N"], out["Z"]) == (want["y"].size, want["val"].size) == (counts["kept"], counts["kept_nnz"])
    assert counts["rows"] == y.size and counts["positives"] == int((y > 0.5).sum()) and counts["negatives_kept"] == int((kept & (y <= 0.5)).sum())
    for key in ("ent_row_ptr", "row_nnz_ptr", "col_global"):
        assert np.array_equal(out[key].cpu().numpy(), want[key]), key
    for key in ("val", "y", "offset", "weight"):
        assert np.array_equal(out[key].cpu().numpy().view(np.uint32), want[key].view(np.uint32)), key
    assert np.array_equal(out["kept_rows"].cpu().numpy(), want["kept_rows"])


CASES = [(rate, neg) for rate in (0.1, 0.5, 1.0) for neg in (True, False)] + [(2.0 ** -33, False)]


@pytest.mark.gpu
@pytest.mark.parametrize("with_weight", [True, False])
@pytest.mark.parametrize("E", [1, 37])
@pytest.mark.parametrize("rate,neg_only", CASES)
def test_compaction_is_the_numpy_statement_bit_for_bit(device_solver, rate, neg_only, E, with_weight):
    rp, col, val, uid, y, off, w = _rows()
    wt = w if with_weight else None
    kept = ds.keep_mask(uid, y, rate, SEED, neg_only)
    erp = _entities(E, kept)
    want = ds.apply_host(erp, rp, col, val, y, off, wt, uid, rate, SEED, neg_only)
    out, counts = _run(device_solver, erp, rp, col, val, y, off, wt, uid, rate, SEED, neg_only)
    _compare(out, counts, want, y, kept)
    assert kept[40_000] == kept[123]
    if rate == 1.0:      # the output is the input, the weights as given or ones
        assert out["N"] == N_ROWS and np.array_equal(out["row_nnz_ptr"].cpu().numpy(), rp) and np.array_equal(out["col_global"].cpu().numpy(), col)
        assert np.array_equal(out["weight"].cpu().numpy(), w if with_weight else np.ones(N_ROWS, np.float32))
    elif rate < 1e-9:    # nothing is kept, and the run ends clean
        assert (out["N"], out["Z"]) == (0, 0) and out["ent_row_ptr"].cpu().numpy().tolist() == [0] * (E + 1)
        assert out["row_nnz_ptr"].cpu().numpy().tolist() == [0]
    else:
        assert 0 < out["N"] < N_ROWS
        if E == 37:      # an entity lost every row
            e = np.diff(want["ent_row_ptr"])
            assert ((e == 0) & (np.diff(erp) > 0)).any()
        if neg_only:
            assert kept[y > 0.5].all() and counts["negatives_kept"] == counts["kept"] - counts["positives"]


@pytest.mark.gpu
@pytest.mark.parametrize("rate", [0.5, 1.0])
def test_compaction_of_rows_without_non_zeros(device_solver, rate):
    rp, col, val, uid, y, off, w = _rows(empty_rows=True)
    assert rp[-1] == 0
    kept = ds.keep_mask(uid, y, rate, 4, True)
    erp = np.array([0, N_ROWS], np.int64)
    want = ds.apply_host(erp, rp, col, val, y, off, w, uid, rate, 4, True)
    out, counts = _run(device_solver, erp, rp, col, val, y, off, w, uid, rate, 4, True)
    _compare(out, counts, want, y, kept)
    assert out["Z"] == 0 and out["N"] == int(kept.sum()) > 0


@pytest.mark.gpu
def test_bad_requests_are_error_codes(device_solver):
    rp, col, val, uid, y, off, w = _rows()
    erp = np.array([0, N_ROWS], np.int64)
    for bad in (0.0, -0.25, 1.5, float("nan"), float("inf")):
        with pytest.raises(S.GdmixReError, match=r"\(-1\)"):      # GDMIX_RE_EINVAL
            _run(device_solver, erp, rp, col, val, y, off, w, uid, bad, 0, True)
    with pytest.raises(S.GdmixReError, match="uid"):
        _run(device_solver, erp, rp, col, val, y, off, w, uid[:-1], 0.5, 0, True)
    # 2^31 rows: refused from the counts alone, before anything is read (the pointers only need to be there)
    lib, t = device_solver.lib, device_solver.torch
    some = t.zeros(64, dtype=t.int64, device=device_solver.device)
    p = some.data_ptr()
    raw = S._RawBatch(1, 1 << 31, 8, p, p, p, p, p, p, None)
    opts = S._DownsampleOpts(0.5, 0, 1, 0)
    counts = S._DownsampleCounts()
    assert lib.gdmix_re_downsample_workspace_bytes(1, 1 << 31) == 0
    rc = lib.gdmix_re_downsample_plan(device_solver._h, C.byref(raw), p, C.byref(opts), p, 512, C.byref(counts), device_solver._stream())
    assert rc == -4 and b"2^31" in lib.gdmix_re_last_error()      # GDMIX_RE_ERANGE
    # an apply whose counts are not its plan's, or whose workspace holds no plan of this context: an error, nothing written
    b = RawBatch(ent_row_ptr=erp, row_nnz_ptr=rp, col_global=col, val=val, y=y, offset=off, weight=w, uid=np.arange(N_ROWS, dtype=np.int64),
                 entity_ids=["0"], has_label=True, binary_labels=True)
    rd = device_solver.upload(b)
    good, good_counts = device_solver.downsample(rd, uid, 0.5, 0, True)      # (the context's last plan from here on)
    c_raw = S._RawBatch(1, N_ROWS, int(rp[-1]), *(rd[k].data_ptr() for k in ("ent_row_ptr", "row_nnz_ptr", "col_global", "val", "y", "offset", "weight")))
    nbytes = int(lib.gdmix_re_downsample_workspace_bytes(1, N_ROWS))
    ws, other = (t.empty(nbytes, dtype=t.uint8, device=device_solver.device) for _ in range(2))      # (both held: two different workspaces)
    names = ("ent_row_ptr", "row_nnz_ptr", "col_global", "val", "y", "offset", "weight")
    outs = {k: good[k].clone() for k in names}
    c_out = S._DownsampleOut(good["N"], good["Z"], *(outs[k].data_ptr() for k in names))
    stale = S._DownsampleOut(good["N"] - 1, good["Z"], *(outs[k].data_ptr() for k in names))
    args = (device_solver._h, C.byref(c_raw), C.byref(opts))
    st = device_solver._stream()
    assert lib.gdmix_re_downsample_plan(*args[:2], t.from_numpy(uid).to(device_solver.device).data_ptr(), args[2], ws.data_ptr(), nbytes, C.byref(counts), st) == 0
    assert (counts.kept, counts.kept_nnz) == (good_counts["kept"], good_counts["kept_nnz"])
    assert lib.gdmix_re_downsample_apply(*args, other.data_ptr(), nbytes, C.byref(c_out), None, st) == -1 and b"last gdmix_re_downsample_plan" in lib.gdmix_re_last_error()
    assert lib.gdmix_re_downsample_apply(*args, ws.data_ptr(), nbytes, C.byref(stale), None, st) == -1 and b"plan kept" in lib.gdmix_re_last_error()
    assert lib.gdmix_re_downsample_apply(*args, ws.data_ptr(), nbytes, C.byref(c_out), None, st) == 0
    t.cuda.synchronize()
    assert all(bool(t.equal(outs[k], good[k])) for k in outs)
    raw = S._RawBatch(1, 100, 8, p, p, p, p, p, p, None)
    rc = lib.gdmix_re_downsample_plan(device_solver._h, C.byref(raw), p, C.byref(opts), p, 16, C.byref(counts), device_solver._stream())
    assert rc == -3                                                # GDMIX_RE_ENOMEM


# ---- a fit on the sample is the fit of the sample -----------------------------------------------------------------------------------------
FIT = dict(has_intercept=True, l2=2.0, regularize_bias=False, max_iter=100, m=10, tolerance=1e-12)
RATE, FIT_SEED = 0.25, 8


@functools.lru_cache(maxsize=None)
def small_case(model_type):
    """tests/test_gpu_fe_poisson.py's small_case shape (600 x 8 over 50 features, weights, offsets); labels by model type, the binary
    ones 10 % positive."""
    rng = np.random.default_rng(61)
    n, k, D = 600, 8, 50
    col = rng.integers(0, D, (n, k)).astype(np.int64).ravel()
    val = (0.4 * rng.standard_normal(n * k)).astype(np.float32)
    off = (0.3 * rng.standard_normal(n)).astype(np.float32)
    wt = (0.5 + rng.random(n)).astype(np.float32)
    w_star = 0.3 * rng.standard_normal(D)
    z = (val.astype(np.float64) * w_star[col]).reshape(n, k).sum(1) + off
    if model_type == fe.LOGISTIC_REGRESSION:
        y = (rng.random(n) < 1.0 / (1.0 + np.exp(-(z - 2.4)))).astype(np.float32)
        assert 0.06 <= y.mean() <= 0.14
    elif model_type == fe.LINEAR_REGRESSION:
        y = (z + 0.3 * rng.standard_normal(n)).astype(np.float32)
    else:
        y = rng.poisson(np.exp(z + 0.4)).astype(np.float32)
    uid = rng.integers(-2 ** 62, 2 ** 62, n, dtype=np.int64)
    return np.arange(n + 1, dtype=np.int64) * k, col, val, y, off, wt, D, uid


def _sample_of(case, model_type, rate=RATE, seed=FIT_SEED):
    rp, col, val, y, off, wt, D, uid = case
    return ds.apply_host(np.array([0, rp.size - 1]), rp, col, val, y, off, wt, uid, rate, seed, model_type == fe.LOGISTIC_REGRESSION)


def _same_fit(a, b, variances):
    (ta, ia), (tb, ib) = a, b
    assert np.array_equal(ta, tb)
    assert float(ia["fval"]) == float(ib["fval"]) and (int(ia["nit"]), int(ia["nfev"]), int(ia["status"])) == (int(ib["nit"]), int(ib["nfev"]), int(ib["status"]))
    if variances:
        assert np.array_equal(ia["variances"], ib["variances"]) and np.all(ia["variances"] > 0)


@pytest.mark.gpu
@pytest.mark.parametrize("fused", ["0", "1"])
@pytest.mark.parametrize("mode", ["SIMPLE", "FULL"])
@pytest.mark.parametrize("model_type", [fe.LOGISTIC_REGRESSION, fe.LINEAR_REGRESSION, fe.POISSON_REGRESSION])
def test_fit_on_the_sample_is_the_fit_of_the_sample(device_solver, monkeypatch, model_type, mode, fused):
    monkeypatch.setenv("GDMIX_FE_FUSED_TAIL", fused)
    case = small_case(model_type)
    rp, col, val, y, off, wt, D, uid = case
    s = fe.FixedEffectDeviceSolver(solver=device_solver)
    kw = dict(model_type=model_type, variance_mode=mode, **FIT)
    got = s.fit_stepping(rp, col, val, y, D, offset=off, weight=wt, down_sampling=(RATE, FIT_SEED, uid), **kw)
    f = _sample_of(case, model_type)
    assert 100 < f["y"].size < 300
    want = s.fit_stepping(f["row_nnz_ptr"], f["col_global"], f["val"], f["y"], D, offset=f["offset"], weight=f["weight"], **kw)
    _same_fit(got, want, True)
    assert int(got[1]["nit"]) >= 2
    c = got[1]["down_sampling"]
    assert (c["rows"], c["kept"], c["kept_nnz"], c["rate"], c["seed"]) == (600, f["y"].size, f["val"].size, RATE, FIT_SEED)
    full = s.fit_stepping(rp, col, val, y, D, offset=off, weight=wt, **kw)
    assert not np.array_equal(full[0], got[0]) and "down_sampling" not in full[1]      # (the sample is another problem than the shard)
    one = s.fit_stepping(rp, col, val, y, D, offset=off, weight=wt, down_sampling=(1.0, FIT_SEED, uid), **kw)
    _same_fit(one, full, True)                                                          # rate 1.0 is the plain fit
    assert "down_sampling" not in one[1]


@pytest.mark.gpu
@pytest.mark.parametrize("extra", ["prior", "feature_scale", "no_weight"])
def test_fit_on_the_sample_with_a_prior_a_feature_scale_and_without_weights(device_solver, extra):
    model_type = fe.LOGISTIC_REGRESSION
    case = small_case(model_type)
    rp, col, val, y, off, wt, D, uid = case
    rng = np.random.default_rng(3)
    more = {"prior": dict(prior=(0.1 * rng.standard_normal(D + 1), 0.5 + rng.random(D + 1))), "feature_scale": dict(feature_scale=0.5 + rng.random(D)),
            "no_weight": {}}[extra]
    if extra == "no_weight":
        wt = None
        case = (rp, col, val, y, off, None, D, uid)
    s = fe.FixedEffectDeviceSolver(solver=device_solver)
    kw = dict(model_type=model_type, variance_mode="SIMPLE", **FIT, **more)
    got = s.fit_stepping(rp, col, val, y, D, offset=off, weight=wt, down_sampling=(RATE, FIT_SEED, uid), **kw)
    f = _sample_of(case, model_type)
    want = s.fit_stepping(f["row_nnz_ptr"], f["col_global"], f["val"], f["y"], D, offset=f["offset"], weight=f["weight"], **kw)
    _same_fit(got, want, True)


@pytest.mark.gpu
def test_fit_on_the_sample_against_scipy(device_solver):
    """scipy's fmin_l_bfgs_b on the numpy objective of the filtered, re-weighted data: sum_i w_i (log(1 + exp(z_i)) - y_i z_i) + (l2/2)|w|^2."""
    model_type = fe.LOGISTIC_REGRESSION
    case = small_case(model_type)
    rp, col, val, y, off, wt, D, uid = case
    f = _sample_of(case, model_type)
    n = f["y"].size
    X = sp.hstack([sp.csr_matrix((f["val"].astype(np.float64), f["col_global"], f["row_nnz_ptr"]), shape=(n, D)), sp.csr_matrix(np.ones((n, 1)))], format="csr")
    XT = X.T.tocsr()
    yy, oo, ww = f["y"].astype(np.float64), f["offset"].astype(np.float64), f["weight"].astype(np.float64)
    reg = np.full(D + 1, FIT["l2"])
    reg[-1] = 0.0

    def fg(th):
        z = X @ th + oo
        return np.sum(ww * (np.logaddexp(0.0, z) - yy * z)) + 0.5 * np.sum(reg * th * th), XT @ (ww * (1.0 / (1.0 + np.exp(-z)) - yy)) + reg * th
    x, fval, st, nit, nfev = P.scipy_fit(fg, np.zeros(D + 1), FIT["m"], FIT["max_iter"], FIT["tolerance"])
    s = fe.FixedEffectDeviceSolver(solver=device_solver)
    theta, info = s.fit_stepping(rp, col, val, y, D, offset=off, weight=wt, model_type=model_type, down_sampling=(RATE, FIT_SEED, uid), **FIT)
    err = rel_err(theta, x)
    print(f"device status {int(info['status'])} nit {int(info['nit'])} nfev {int(info['nfev'])}; scipy {st} {nit} {nfev}; theta {err:.3e}; fval {float(info['fval'])!r} vs {fval!r}")
    assert int(info["status"]) == st
    assert err <= tol(st), err


# ---- the sweep --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_sweep_rows_are_plain_down_sampled_fits_and_the_shard_is_sampled_once(device_solver, monkeypatch):
    model_type = fe.LOGISTIC_REGRESSION
    rp, col, val, y, off, wt, D, uid = small_case(model_type)
    s = fe.FixedEffectDeviceSolver(solver=device_solver)
    grid = (10.0, 1.0, 0.1)
    kw = dict(FIT, model_type=model_type)
    kw.pop("l2")
    plain = [s.fit_stepping(rp, col, val, y, D, offset=off, weight=wt, l2=w, variance_mode="SIMPLE", down_sampling=(RATE, FIT_SEED, uid), **kw) for w in grid]
    calls, real, seen = [], device_solver.downsample, []
    monkeypatch.setattr(device_solver, "downsample", lambda *a, **k: calls.append(1) or real(*a, **k))

    def select(thetas):
        seen.extend(thetas)
        return 1
    theta, info, best = s.fit_sweep(rp, col, val, y, D, l2_grid=grid, select=select, offset=off, weight=wt, variance_mode="SIMPLE",
                                    down_sampling=(RATE, FIT_SEED, uid), **kw)
    assert len(calls) == 1 and best == 1 and len(seen) == len(grid)
    for k in range(len(grid)):
        assert np.array_equal(seen[k], plain[k][0]), k
    assert len({th.tobytes() for th in seen}) == len(grid)
    _same_fit((theta, info), plain[1], True)
    assert info["down_sampling"] == plain[1][1]["down_sampling"]


# ---- the empty outcome --------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("mode", [None, "SIMPLE", "FULL"])
def test_a_sample_without_rows_trains_on_the_weight_zero_sample(device_solver, mode):
    """40 negatives at rate 0.05: seed 1 keeps none of them (found with the numpy statement), seed 0 keeps three."""
    rng = np.random.default_rng(5)
    n, k, D = 40, 4, 12
    uid = np.arange(n, dtype=np.int64) * 7 + 100
    y = np.zeros(n, np.float32)
    assert not ds.keep_mask(uid, y, 0.05, 1, True).any() and ds.keep_mask(uid, y, 0.05, 0, True).sum() == 3
    rp = np.arange(n + 1, dtype=np.int64) * k
    col = rng.integers(0, D, n * k).astype(np.int64)
    val = rng.standard_normal(n * k).astype(np.float32)
    s = fe.FixedEffectDeviceSolver(solver=device_solver)
    theta, info = s.fit_stepping(rp, col, val, y, D, model_type=fe.LOGISTIC_REGRESSION, variance_mode=mode, down_sampling=(0.05, 1, uid), **FIT)
    assert theta.shape == (D + 1,) and not theta.any() and int(info["status"]) in (0, 1, 2, 3, 4)
    assert (info["down_sampling"]["kept"], info["down_sampling"]["kept_nnz"], info["down_sampling"]["rows"]) == (0, 0, n)
    if mode is not None:      # the curvature of a weight-0 sample is zero: 1 / (l2 + 1e-12), and 1e12 for the unregularised intercept
        np.testing.assert_allclose(info["variances"][:D], 1.0 / (FIT["l2"] + 1e-12), rtol=1e-12)
    # rows without non-zeros kept (a dummy-free shard of empty rows): the same fall-back
    theta2, info2 = s.fit_stepping(np.zeros(n + 1, np.int64), [], [], y, D, model_type=fe.LOGISTIC_REGRESSION, down_sampling=(0.5, 0, uid), dummy=False, **FIT)
    kept = ds.keep_mask(uid, y, 0.5, 0, True)
    f = ds.apply_host([0, n], np.zeros(n + 1, np.int64), [], [], y, None, None, uid, 0.5, 0, True)
    want = s.fit_stepping(f["row_nnz_ptr"], [], [], f["y"], D, offset=f["offset"], weight=f["weight"], model_type=fe.LOGISTIC_REGRESSION, dummy=False, **FIT)
    assert 0 < kept.sum() < n and np.array_equal(theta2, want[0]) and int(info2["nit"]) == int(want[1]["nit"])
    c = info2["down_sampling"]      # the counts are those of the shard's own rows, not of the weight-0 sample appended to them
    assert (c["rows"], c["kept"], c["kept_nnz"], c["positives"], c["negatives_kept"]) == (n, int(kept.sum()), 0, 0, int(kept.sum()))


@pytest.mark.gpu
def test_a_model_without_a_feature_bag_is_sampled_like_any_other(device_solver):
    rp, col, val, y, off, wt, D, uid = small_case(fe.LOGISTIC_REGRESSION)
    n = y.size
    s = fe.FixedEffectDeviceSolver(solver=device_solver)
    kw = dict(FIT, model_type=fe.LOGISTIC_REGRESSION, dummy=True)
    got = s.fit_stepping(np.zeros(n + 1, np.int64), [], [], y, 1, offset=off, weight=wt, down_sampling=(RATE, FIT_SEED, uid), **kw)
    f = ds.apply_host([0, n], np.zeros(n + 1, np.int64), [], [], y, off, wt, uid, RATE, FIT_SEED, True)
    want = s.fit_stepping(f["row_nnz_ptr"], [], [], f["y"], 1, offset=f["offset"], weight=f["weight"], **kw)
    _same_fit(got, want, False)
    assert got[0].shape == (1,) and got[1]["down_sampling"]["kept"] == f["y"].size


# ---- the stage, through the command line, in process ------------------------------------------------------------------------------------
def _read_model(path):
    from gdmix_amd.io import avro
    (rec,) = list(avro.read_file(path))
    return {m["name"]: m["value"] for m in rec["means"]}


def _stage(base, root, extra):
    shutil.copytree(os.path.join(base, "global"), os.path.join(root, "global"))
    chain.run_stage(chain.stage_argv(root, "global", chain.LOGISTIC, False) + [f"--metric_output_dir={chain.metric_dir(root, 'global')}"] + list(extra))
    return os.path.join(root, "global")


@pytest.mark.gpu
def test_stage_trains_on_the_sample_and_scores_every_row(device_solver, tmp_path):
    data = chain.make_dataset(200, 300, 6000, train_fraction=0.5)
    base = str(tmp_path / "inputs")
    chain.write_global_inputs(base, data)
    out = _stage(base, str(tmp_path / "sampled"), ["--down_sampling_rate=0.25", "--down_sampling_seed=3"])
    train = np.flatnonzero(data["train"])
    ptr, cols, vals, D = chain.bag_rows(data, "global", train)
    y = data["response"][train].astype(np.float32)
    uid = data["uid"][train]
    f = ds.apply_host([0, train.size], ptr, cols, vals, y, None, None, uid, 0.25, 3, True)
    assert 0 < f["y"].size < train.size
    s = fe.FixedEffectDeviceSolver(solver=device_solver)
    theta, _ = s.fit_stepping(f["row_nnz_ptr"], f["col_global"], f["val"], f["y"], D, offset=f["offset"], weight=f["weight"], has_intercept=True, l2=1.0,
                              regularize_bias=False, model_type=fe.LOGISTIC_REGRESSION, max_iter=100, m=10, tolerance=1e-12, dummy=False)
    model = _read_model(os.path.join(out, "models", "part-00000.avro"))
    want = {f"g{j}": float(theta[j]) for j in range(D) if abs(theta[j]) > 1e-4}
    want["(INTERCEPT)"] = float(theta[D])
    assert model == want and len(want) > 10                                              # bit for bit: the values are doubles
    # the score files and the metric hold every row
    for which, rows in (("trainingScores", train), ("validationScores", np.flatnonzero(~data["train"]))):
        got_uid = chain.read_scores(os.path.join(out, which))[0]
        assert np.array_equal(np.sort(got_uid), np.sort(data["uid"][rows])), which
    with open(os.path.join(out, "metrics", "evalSummary.json")) as fh:
        summary = json.load(fh)
    assert summary["validation"]["n"] == int((~data["train"]).sum()) and summary["training"]["n"] == train.size
    # rate 1.0 is a run without the flag, byte for byte
    a = _stage(base, str(tmp_path / "one"), ["--down_sampling_rate=1.0"])
    b = _stage(base, str(tmp_path / "plain"), [])
    for d in ("models", "trainingScores", "validationScores"):
        assert avro_bytes(os.path.join(a, d, "part-00000.avro")) == avro_bytes(os.path.join(b, d, "part-00000.avro")), d
    with open(os.path.join(a, "metrics", "evalSummary.json"), "rb") as fa, open(os.path.join(b, "metrics", "evalSummary.json"), "rb") as fb:
        assert fa.read() == fb.read()
    assert _read_model(os.path.join(b, "models", "part-00000.avro")) != model


# ---- two workers against one --------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_two_workers_keep_the_rows_one_worker_keeps(device_solver, tmp_path):
    root = os.path.dirname(HERE)
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    env.pop("TF_CONFIG", None)
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2", "--master-addr", "127.0.0.1", "--master-port", "29647",
           os.path.join(root, "tests", "_fe_downsample_dist_worker.py"), str(tmp_path)]
    subprocess.run(cmd, check=True, env=env, timeout=600, cwd=root)
    with open(tmp_path / "result.json") as fh:
        a, b = json.load(fh)
    assert a["theta"] == b["theta"] and a["status"] == b["status"] and a["nit"] == b["nit"]      # replicated step
    model_type = fe.LOGISTIC_REGRESSION
    rp, col, val, y, off, wt, D, uid = small_case(model_type)
    batch, _ = fe.shard_as_batch(rp, col, val, y, off, wt, True, dummy=False)
    one, counts = device_solver.downsample(device_solver.upload(batch), uid, RATE, FIT_SEED, negatives_only=True)
    one_set = uid[one["kept_rows"].cpu().numpy()].tolist()
    assert sorted(a["kept_uid"] + b["kept_uid"]) == sorted(one_set) and not set(a["kept_uid"]) & set(b["kept_uid"])
    assert a["kept_uid"] and b["kept_uid"] and counts["kept"] == len(one_set)
    s = fe.FixedEffectDeviceSolver(solver=device_solver)
    theta, info = s.fit_stepping(rp, col, val, y, D, offset=off, weight=wt, model_type=model_type, down_sampling=(RATE, FIT_SEED, uid), **FIT)
    err = rel_err(np.array(a["theta"]), theta)
    print(f"two workers ({a['backend']}) against one: theta {err:.3e}, status {a['status']} / {int(info['status'])}, nit {a['nit']} / {int(info['nit'])}")
    assert err <= tol(a["status"]) * 10, err      # (the bar of test_fixed_effect.py's two-worker test: the shards' sums are added in another order)
