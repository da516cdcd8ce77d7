"""GPU: --features_to_samples_ratio on the device (include/gdmix_re.h, "feature selection"; csrc/re_select.hip) — the keys against exact
rational arithmetic within the bound the header derives, the selection exactly given the device's own keys, the filtered raw batch and
its pack against the host, the solves on it at the existing parity bars, and the flag through the command line.
tests/feature_selection_helpers.py holds the reference and the hand-made edge batch."""
import dataclasses
import os

import numpy as np
import pytest

from gdmix_amd import feature_selection as fs
from gdmix_amd import synthetic
from gdmix_amd.solver import GdmixReError, SolverOptions
from oracle import oracle
import feature_selection_helpers as F
import re_linear_helpers as H
import re_poisson_helpers as P

pytestmark = pytest.mark.gpu

_RUNS = {}


def _run(solver, name, ratio, small_max=None):
    """Upload, pack, select on the device -> dict of host arrays; cached per (batch, ratio, small_max)."""
    key = (name, ratio, small_max)
    if key in _RUNS:
        return _RUNS[key]
    out = _RUNS[key] = _select(solver, F.batch(name), ratio, small_max)
    return out


def _select(solver, b, ratio, small_max=None, keep_device=False):
    raw = solver.upload(b)
    packed = solver.pack(raw, has_intercept=True)
    if small_max is not None:
        solver.set_select_small_max(small_max)
    try:
        filtered, keep, counts = solver.select_features(raw, packed, ratio, want_keys=True)
    finally:
        solver.set_select_small_max(solver.SELECT_SMALL_MAX_DEFAULT)
    keys = counts.pop("keys")
    out = dict(keys=keys.cpu().numpy(), keep=keep.cpu().numpy().astype(bool), counts=counts, fp=packed.ent_feat_ptr().cpu().numpy(),
               uniq=packed.unique_global().cpu().numpy().astype(np.int64), row_nnz_ptr=filtered["row_nnz_ptr"].cpu().numpy(),
               col_global=filtered["col_global"].cpu().numpy(), val=filtered["val"].cpu().numpy(), Z=filtered["Z"])
    if keep_device:
        out["filtered"], out["raw"] = filtered, raw
    return out


@pytest.mark.parametrize("name", F.NAMES)
def test_keys_against_the_exact_reference(device_solver, name):
    ref = F.reference(name)
    F.check_conditions(ref)
    got = _run(device_solver, name, 0.5)
    fp, uniq = ref["slots"][0], ref["slots"][1]
    assert np.array_equal(got["fp"], fp) and np.array_equal(got["uniq"], uniq)
    assert got["keys"].dtype == np.float32 and got["keys"].size == uniq.size and np.all(got["keys"] >= 0)
    F.check_keys(ref, got["keys"])


@pytest.mark.parametrize("ratio", F.RATIOS)
@pytest.mark.parametrize("name", F.NAMES)
def test_the_selection_is_exact_given_the_device_keys(device_solver, name, ratio):
    b, sl = F.batch(name), F.reference(name)["slots"]
    got = _run(device_solver, name, ratio)
    keep, counts = F.host_selection(b, sl, got["keys"], ratio)
    assert np.array_equal(got["keep"], keep), int((got["keep"] != keep).sum())
    assert got["counts"] == counts, (got["counts"], counts)
    assert counts["affected"] > 0 and 0 < counts["kept"] < counts["features"]
    want = fs.filter_batch(b, sl[2], keep)
    assert got["Z"] == want.Z == counts["kept_nnz"]
    assert np.array_equal(got["row_nnz_ptr"], want.row_nnz_ptr) and np.array_equal(got["col_global"], want.col_global)
    assert np.array_equal(got["val"].view(np.uint32), want.val.view(np.uint32))


@pytest.mark.parametrize("name", F.NAMES)
def test_nothing_to_drop(device_solver, name):
    b = F.batch(name)
    got = _run(device_solver, name, 1e9)
    assert got["counts"]["kept_nnz"] == b.Z == got["Z"] and got["counts"]["affected"] == 0 and got["counts"]["dropped"] == 0
    assert got["keep"].all()
    assert np.array_equal(got["row_nnz_ptr"], b.row_nnz_ptr) and np.array_equal(got["col_global"], b.col_global)
    assert np.array_equal(got["val"].view(np.uint32), b.val.view(np.uint32))


@pytest.mark.parametrize("name", F.NAMES)
def test_one_answer_whichever_path_ranks(device_solver, name):
    """small_max forced to 0 (every entity through the segmented sort) and at its default (1024: counting across the lanes up to 64
    features, against the keys in LDS above; only zipf's head entities are sorted)."""
    for ratio in F.RATIOS:
        a, c = _run(device_solver, name, ratio), _run(device_solver, name, ratio, small_max=0)
        assert np.array_equal(a["keys"].view(np.uint32), c["keys"].view(np.uint32))
        assert np.array_equal(a["keep"], c["keep"]), int((a["keep"] != c["keep"]).sum())
        assert a["counts"] == c["counts"]
    for limit in (63, 64):      # ... and limits in between, which split d_e = 63 / 64 / 65 (and c2's widest entities) differently
        c = _run(device_solver, name, 0.5, small_max=limit)
        assert np.array_equal(a["keep"], c["keep"]) and np.array_equal(a["keys"].view(np.uint32), c["keys"].view(np.uint32))


@pytest.mark.parametrize("name", F.NAMES)
def test_one_answer_wherever_the_entity_sits_and_from_run_to_run(device_solver, name):
    b = F.batch(name)
    a = _run(device_solver, name, 0.5)
    again = _select(device_solver, b, 0.5)
    for k in ("keys", "val"):
        assert np.array_equal(a[k].view(np.uint32), again[k].view(np.uint32)), k
    for k in ("keep", "row_nnz_ptr", "col_global"):
        assert np.array_equal(a[k], again[k]), k
    perm = np.random.default_rng(3).permutation(b.E)
    c = _select(device_solver, F.permuted(b, perm), 0.5)
    src = F.permute_slots(a["fp"], perm)
    assert np.array_equal(c["uniq"], a["uniq"][src])
    assert np.array_equal(c["keys"].view(np.uint32), a["keys"][src].view(np.uint32))
    assert np.array_equal(c["keep"], a["keep"][src])


def test_bad_arguments_are_refused_and_a_stale_plan_writes_nothing(device_solver):
    import ctypes as C
    from gdmix_amd import solver as S
    s, t = device_solver, device_solver.torch
    b = F.batch("edge")
    raw = s.upload(b)
    packed = s.pack(raw, has_intercept=True)
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(GdmixReError, match="finite and above 0"):
            s.select_features(raw, packed, bad)
    assert s.lib.gdmix_re_select_workspace_bytes(1 << 31, 1, 1) == 0 and s.lib.gdmix_re_select_workspace_bytes(1, 1, 1 << 31) == 0
    nbytes = int(s.lib.gdmix_re_select_workspace_bytes(b.E, b.N, b.Z))
    ws = t.empty(nbytes, dtype=t.uint8, device=s.device)
    keep = t.empty(packed.D, dtype=t.uint8, device=s.device)
    counts = S._SelectCounts()
    assert s.lib.gdmix_re_select_plan(s._h, C.byref(packed.c), 0.5, ws.data_ptr(), nbytes - 1, None, keep.data_ptr(), C.byref(counts), s._stream()) == -3
    assert s.lib.gdmix_re_select_plan(s._h, C.byref(packed.c), 0.5, ws.data_ptr(), nbytes, None, keep.data_ptr(), C.byref(counts), s._stream()) == 0
    c_raw = S._RawBatch(b.E, b.N, b.Z, raw["ent_row_ptr"].data_ptr(), raw["row_nnz_ptr"].data_ptr(), raw["col_global"].data_ptr(), raw["val"].data_ptr(),
                        raw["y"].data_ptr(), raw["offset"].data_ptr(), None)
    z = int(counts.kept_nnz)
    rp = t.full((b.N + 1,), -7, dtype=t.int64, device=s.device)
    col, val = t.full((z + 1,), -7, dtype=t.int64, device=s.device), t.full((z + 1,), -7.0, dtype=t.float32, device=s.device)
    wrong = S._SelectOut(z + 1, rp.data_ptr(), col.data_ptr(), val.data_ptr())
    assert s.lib.gdmix_re_select_apply(s._h, C.byref(c_raw), C.byref(packed.c), ws.data_ptr(), C.byref(wrong), s._stream()) == -1
    other = t.empty(nbytes, dtype=t.uint8, device=s.device)
    right = S._SelectOut(z, rp.data_ptr(), col.data_ptr(), val.data_ptr())
    assert s.lib.gdmix_re_select_apply(s._h, C.byref(c_raw), C.byref(packed.c), other.data_ptr(), C.byref(right), s._stream()) == -1
    t.cuda.synchronize(s.device)
    assert bool((rp == -7).all()) and bool((col == -7).all()) and bool((val == -7.0).all())      # nothing was written
    assert s.lib.gdmix_re_select_apply(s._h, C.byref(c_raw), C.byref(packed.c), ws.data_ptr(), C.byref(right), s._stream()) == 0
    t.cuda.synchronize(s.device)
    assert int(rp[-1]) == z and int(col[z]) == -7


# ---- downstream: unchanged kernels on new input -------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def downstream(device_solver):
    """c2 at ratio 0.5: the device's filtered batch packed again, and the host-filtered batch (the device's own mask) with oracle.pack."""
    b = F.batch("c2")
    got = _select(device_solver, b, 0.5, keep_device=True)
    sl = F.reference("c2")["slots"]
    fb = fs.filter_batch(b, sl[2], got["keep"])
    return dict(b=b, got=got, fb=fb, pk=oracle.pack(fb.ent_row_ptr, fb.row_nnz_ptr, fb.col_global))


def test_the_repacked_batch_is_the_pack_of_the_host_filtered_batch(device_solver, downstream):
    fb, pk = downstream["fb"], downstream["pk"]
    packed = device_solver.pack(downstream["got"]["filtered"], has_intercept=True)
    assert (packed.E, packed.N, packed.Z, packed.D) == (fb.E, fb.N, fb.Z, pk["D"])
    assert np.array_equal(packed.ent_feat_ptr().cpu().numpy(), pk["ent_feat_ptr"])
    assert np.array_equal(packed.ent_nnz_ptr().cpu().numpy(), pk["ent_nnz_ptr"])
    assert np.array_equal(packed.row_ptr().cpu().numpy(), pk["row_ptr"])
    assert np.array_equal(packed.csr_col().cpu().numpy(), pk["csr_col"])
    assert np.array_equal(packed.unique_global().cpu().numpy().astype(np.int64), pk["unique_global"])
    assert packed.c.csr_val == downstream["got"]["filtered"]["val"].data_ptr()      # (the CSR values are the raw batch's, in place)
    k = fs.k_all(0.5, np.diff(fb.ent_row_ptr), np.diff(downstream["got"]["fp"]))
    assert np.array_equal(np.diff(pk["ent_feat_ptr"]), k)


KW = dict(l2=1.0, regularize_bias=True, has_intercept=True, m=10, max_iter=100, ftol=1e-12, variance_mode=0)


def test_a_linear_solve_on_the_filtered_batch(device_solver, downstream):
    fb, pk = downstream["fb"], downstream["pk"]
    packed = device_solver.pack(downstream["got"]["filtered"], has_intercept=True)
    res = device_solver.solve(packed, SolverOptions(linear=True, **KW)).to_host()
    j = H.judge(fb, pk, KW, None, res, packed.coef_ptr_host(), theta_tol=1e-7)
    assert not j["problems"], j["problems"][:3]
    ok, ref = j["strict_ok"], j["ref"]
    print(f"linear on the filtered batch: {ok.mean():.1%} strict, worst strict error {j['err'][ok].max():.3e}")
    assert ok.mean() >= 0.5
    assert np.array_equal(res["status"][ok], ref["status"][ok]) and np.array_equal(res["nit"][ok], ref["nit"][ok])
    assert j["err"][ok].max() <= 1e-7


def test_a_logistic_solve_on_the_filtered_batch(device_solver, downstream):
    """(c2's labels are 0 / 1; a regularised intercept, so that every entity has a minimiser.)"""
    fb, pk = downstream["fb"], downstream["pk"]
    assert set(np.unique(fb.y)) <= {0.0, 1.0}
    packed = device_solver.pack(downstream["got"]["filtered"], has_intercept=True)
    res = device_solver.solve(packed, SolverOptions(**KW)).to_host()
    cp = packed.coef_ptr_host()
    o = oracle.make_opts(**dict(KW, linear=False, sum_loss=False))
    ref, strict, _, _ = H.oracle_strict(fb, pk, o, None, int(cp[-1]))
    err = H.per_entity_rel_err(res["theta"], ref["theta"], cp)
    print(f"logistic on the filtered batch: {strict.mean():.1%} strict, worst strict error {err[strict].max():.3e}, worst other {err[~strict].max() if (~strict).any() else 0.0:.3e}")
    assert strict.mean() >= 0.5
    assert np.array_equal(res["status"][strict], ref["status"][strict]) and np.array_equal(res["nit"][strict], ref["nit"][strict])
    assert err[strict].max() <= 1e-7
    tight = oracle.solve(pk, fb.val, fb.y, fb.offset, fb.weight, oracle.make_opts(**dict(KW, max_iter=5000, ftol=1e-15)))
    assert H.per_entity_rel_err(res["theta"], tight["theta"], cp)[~strict].max(initial=0.0) <= 1e-5


def test_a_poisson_solve_on_the_filtered_batch(device_solver, downstream):
    fb, pk = downstream["fb"], downstream["pk"]
    fbp = synthetic.with_count_labels(fb, seed=9)
    raw = dict(downstream["got"]["filtered"])
    raw["y"] = device_solver.torch.from_numpy(fbp.y).to(device_solver.device)
    packed = device_solver.pack(raw, has_intercept=True)
    res = device_solver.solve(packed, SolverOptions(loss="poisson", **KW)).to_host()
    cp = packed.coef_ptr_host()
    ref = P.reference(fbp, pk, KW, None, cp, seed=5)
    P.compare(res, ref, cp)


# ---- the product path -------------------------------------------------------------------------------------------------------------------
def _read_models(path):
    from gdmix_amd.io import avro
    return {r["modelId"]: {(m["name"], m["term"]): m["value"] for m in r["means"]} for r in avro.read_file(path)}


def _job_batch(model_type):
    if model_type == "linear_regression":
        return H.small_job_batch(E=60, seed=41, real=True)
    b = H.small_job_batch(E=60, seed=42, real=False)
    return synthetic.with_count_labels(b, 42) if model_type == "poisson_regression" else b


def _reference_fit(model_type, fb, pk):
    """The fit of the job's options (re_linear_helpers.job_argv: l2 1, unregularised intercept, m 10, 100 iterations, ftol 1e-12) on the
    filtered batch -> theta [P] in pk's index space."""
    cp = np.asarray(pk["ent_feat_ptr"]) + np.arange(fb.E + 1)
    kw = dict(l2=1.0, regularize_bias=model_type == "logistic_regression", has_intercept=True, m=10, max_iter=100, ftol=1e-12)
    if model_type == "poisson_regression":
        ref = P.reference(fb, pk, kw, None, cp, entities=np.arange(fb.E))
        return np.concatenate([ref["theta"][e] for e in range(fb.E)]), cp
    return oracle.solve(pk, fb.val, fb.y, fb.offset, None, oracle.make_opts(linear=model_type == "linear_regression", **kw))["theta"], cp


@pytest.mark.parametrize("model_type", ["logistic_regression", "linear_regression", "poisson_regression"])
def test_cli_child_process_trains_on_selected_features(tmp_path, model_type):
    """One partition (60 entities, 12 samples each on average) through `python -m gdmix_amd.gdmix --features_to_samples_ratio=0.5` as a child
    process. Every model record holds at most k_e bag features and the intercept; coefficients within 1e-5 of the reference fit on the
    filtered data; the written scores are x . theta + offset of the written model on the UNFILTERED rows, to 1 ulp of the Avro float.
    (The logistic job regularises its intercept, so that entities whose labels are all equal have a minimiser to be compared with.)"""
    from gdmix_amd import chain
    from test_gpu_chain import _scores_by_uid, _ulps
    ratio = 0.5
    b = _job_batch(model_type)
    root = str(tmp_path)
    H.write_job(root, b)
    argv = H.job_argv(root, "train", model_type=model_type, extra=[f"--features_to_samples_ratio={ratio}"])
    if model_type == "logistic_regression":
        argv = [a.replace("--regularize_bias=False", "--regularize_bias=True") for a in argv]
    chain.run_stage(argv, child_process=True)
    fb, keep, _, counts = fs.select_batch(b, ratio)
    assert counts["affected"] > 0
    pk, pkf = oracle.pack(b.ent_row_ptr, b.row_nnz_ptr, b.col_global), oracle.pack(fb.ent_row_ptr, fb.row_nnz_ptr, fb.col_global)
    theta, cpf = _reference_fit(model_type, fb, pkf)
    got = _read_models(os.path.join(root, "models", "part-00000.avro"))
    assert set(got) == set(b.entity_ids)
    fp, fpf = pk["ent_feat_ptr"], pkf["ent_feat_ptr"]
    k = fs.k_all(ratio, np.diff(b.ent_row_ptr), np.diff(fp))
    written = np.zeros(int(fp[-1]) + b.E)
    worst = 0.0
    for e, eid in enumerate(b.entity_ids):
        names = [nm for nm in got[eid] if nm != ("(INTERCEPT)", "")]
        assert len(names) <= k[e], (eid, len(names), int(k[e]))
        kept = {(f"f{int(g)}", "") for g in pkf["unique_global"][fpf[e]:fpf[e + 1]]}
        assert set(names) <= kept, eid
        want = theta[cpf[e]:cpf[e + 1]]
        want = np.where(np.abs(want) <= 1e-4, 0.0, want)
        have = np.array([got[eid].get(nm, 0.0) for nm in [("(INTERCEPT)", "")] + [(f"f{int(g)}", "") for g in pkf["unique_global"][fpf[e]:fpf[e + 1]]]])
        worst = max(worst, float(np.abs(have - want).max() / max(1.0, np.abs(want).max())))
        written[fp[e] + e:fp[e + 1] + e + 1] = [got[eid].get(nm, 0.0) for nm in [("(INTERCEPT)", "")] + [(f"f{int(g)}", "") for g in pk["unique_global"][fp[e]:fp[e + 1]]]]
    print(f"{model_type}: model Avro against the reference fit on the filtered data: worst {worst:.3e}")
    assert worst <= 1e-5, worst
    lo, _ = oracle.score(pk, b.val, b.offset, written, True)      # the written model on the unfiltered rows
    order = np.argsort(b.uid, kind="stable")
    for d in ("trainingScores", "validationScores"):
        s = _scores_by_uid(os.path.join(root, d))
        assert np.array_equal(s["uid"], b.uid[order])
        assert _ulps(s["score"], lo.astype(np.float32)[order]).max() <= 1.0, d
    chain.run_stage(H.job_argv(root, "inference", model_type=model_type, extra=[f"--features_to_samples_ratio={ratio}"]), child_process=True)
    s = _scores_by_uid(os.path.join(root, "inferenceScores"))      # inference accepts and ignores the flag
    assert _ulps(s["score"], lo.astype(np.float32)[order]).max() <= 1.0


@pytest.mark.parametrize("flag,message", [
    ("--incremental_training=True", "--features_to_samples_ratio does not run with --incremental_training"),
    ("--l2_reg_weights=1,0.1", "--features_to_samples_ratio does not run with --l2_reg_weights"),
    ("--feature_normalization=scale_with_max_magnitude", "--features_to_samples_ratio does not run with --feature_normalization"),
    ("--rebalance_entities=True", "--features_to_samples_ratio does not run with --rebalance_entities"),
])
def test_cli_refuses_what_the_selection_does_not_run_with(tmp_path, flag, message):
    from gdmix_amd import chain
    root = str(tmp_path)
    H.write_job(root, H.small_job_batch(E=4, seed=43))
    with pytest.raises(RuntimeError) as err:
        chain.run_stage(H.job_argv(root, "train", extra=["--features_to_samples_ratio=0.5", flag]), child_process=True)
    assert "stage exited with" in str(err.value) and message in str(err.value)
    assert not os.path.exists(os.path.join(root, "models"))
