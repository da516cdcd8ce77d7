"""GPU: --active_data_upper_bound on the device (include/gdmix_re.h, "active-data cap"; csrc/re_cap.hip) — the capped raw batch bit for bit
against the numpy statement (gdmix_amd/active_data.py: apply_host) whichever path ranks an entity and wherever it sits, the pack and the
solves of the capped batch against the references on the host-capped batch at the existing parity bars, and the flag through the command
line: models of the capped data, scores and metrics of every row. tests/active_data_helpers.py holds the batches."""
import ctypes as C
import json
import os

import numpy as np
import pytest

from gdmix_amd import feature_selection as fs
from gdmix_amd import solver as S
from gdmix_amd.solver import GdmixReError, SolverOptions
from oracle import oracle
import active_data_helpers as A
import fuzz_case
import re_linear_helpers as H
import re_poisson_helpers as P

pytestmark = pytest.mark.gpu

ARRAYS_INT = ("ent_row_ptr", "row_nnz_ptr", "col_global")
ARRAYS_F32 = ("val", "y", "offset", "weight")
_RUNS = {}


def _cap(solver, b, K, seed=A.SEED, small_max=None, keep_device=False):
    """Upload and cap on the device -> dict of host arrays and counts."""
    if small_max is not None:
        solver.set_cap_small_max(small_max)
    try:
        dev, counts = solver.cap_samples(solver.upload(b), b.uid, K, seed=seed)
    finally:
        solver.set_cap_small_max(solver.CAP_SMALL_MAX_DEFAULT)
    solver.torch.cuda.synchronize()
    out = {k: dev[k].cpu().numpy() for k in ARRAYS_INT + ARRAYS_F32 + ("kept_rows",)}
    out.update(N=dev["N"], Z=dev["Z"], E=dev["E"], counts=counts)
    if keep_device:
        out["device"] = dev
    return out


def _run(solver, K, with_weight, small_max=None):
    key = (K, with_weight, small_max)
    if key not in _RUNS:
        _RUNS[key] = _cap(solver, A.edge_batch(K, with_weight), K, small_max=small_max)
    return _RUNS[key]


def _same(got, want, what=""):
    assert (got["N"], got["Z"]) == (want["y"].size, want["val"].size), what
    for k in ARRAYS_INT:
        assert np.array_equal(got[k], want[k]), (what, k)
    for k in ARRAYS_F32:
        assert got[k].dtype == np.float32 and np.array_equal(got[k].view(np.uint32), want[k].view(np.uint32)), (what, k)
    assert np.array_equal(got["kept_rows"], want["kept_rows"]), what


@pytest.mark.parametrize("with_weight", [True, False])
@pytest.mark.parametrize("K", A.KS)
def test_the_capped_batch_is_the_numpy_statement_bit_for_bit(device_solver, K, with_weight):
    b = A.edge_batch(K, with_weight)
    want = A.host_cap(b, K)
    got = _run(device_solver, K, with_weight)
    _same(got, want)
    assert got["counts"] == A.counts_of(b, K, want)
    assert 0 < got["counts"]["capped"] < b.E and got["counts"]["largest"] == 5000 and got["N"] < b.N
    assert np.array_equal(np.diff(got["ent_row_ptr"]), np.minimum(b.ent_n(), K))          # no entity is emptied, none exceeds the bound


@pytest.mark.parametrize("with_weight", [True, False])
@pytest.mark.parametrize("K", A.KS)
def test_one_answer_whichever_path_ranks(device_solver, K, with_weight):
    """small_max 0: every capped entity through the radix select; 64: the split at a wavefront; 1024: the most the counting path takes;
    the default parts them at 128 rows."""
    assert device_solver.CAP_SMALL_MAX_DEFAULT == 128 and device_solver.CAP_SMALL_MAX_LIMIT == 1024
    a = _run(device_solver, K, with_weight)
    for limit in (0, 64, 1024):
        c = _run(device_solver, K, with_weight, small_max=limit)
        _same(c, a, f"small_max {limit}")
        assert c["counts"] == a["counts"]


@pytest.mark.parametrize("K", A.KS)
def test_one_answer_wherever_the_entity_sits_and_from_run_to_run(device_solver, K):
    b = A.edge_batch(K)
    a = _run(device_solver, K, True)
    again = _cap(device_solver, b, K)
    _same(again, a, "second run")
    r = _cap(device_solver, A.reversed_entities(b), K)
    assert r["counts"] == a["counts"]
    for e in range(b.E):
        f = b.E - 1 - e
        sa, sr = slice(a["ent_row_ptr"][e], a["ent_row_ptr"][e + 1]), slice(r["ent_row_ptr"][f], r["ent_row_ptr"][f + 1])
        assert np.array_equal(a["kept_rows"][sa] - b.ent_row_ptr[e], r["kept_rows"][sr] - (b.N - b.ent_row_ptr[e + 1])), e
        for k in ("y", "offset", "weight"):
            assert np.array_equal(a[k][sa].view(np.uint32), r[k][sr].view(np.uint32)), (e, k)
        za, zr = slice(a["row_nnz_ptr"][sa.start], a["row_nnz_ptr"][sa.stop]), slice(r["row_nnz_ptr"][sr.start], r["row_nnz_ptr"][sr.stop])
        assert np.array_equal(a["col_global"][za], r["col_global"][zr]) and np.array_equal(a["val"][za].view(np.uint32), r["val"][zr].view(np.uint32)), e


@pytest.mark.parametrize("with_weight", [True, False])
def test_nothing_to_drop(device_solver, with_weight):
    b = A.edge_batch(2, with_weight)
    got = _cap(device_solver, b, 5000)
    assert got["counts"] == dict(entities=b.E, capped=0, rows=b.N, kept=b.N, kept_nnz=b.Z, largest=5000)
    for k in ARRAYS_INT:
        assert np.array_equal(got[k], getattr(b, k)), k
    for k in ("val", "y", "offset"):
        assert np.array_equal(got[k].view(np.uint32), getattr(b, k).view(np.uint32)), k
    assert np.array_equal(got["weight"], b.weight if with_weight else np.ones(b.N, np.float32))
    assert np.array_equal(got["kept_rows"], np.arange(b.N))


def test_an_empty_batch(device_solver):
    got = _cap(device_solver, A.empty_batch(), 3)
    assert got["counts"] == dict(entities=0, capped=0, rows=0, kept=0, kept_nnz=0, largest=0)
    assert got["ent_row_ptr"].tolist() == [0] and got["row_nnz_ptr"].tolist() == [0] and got["N"] == 0 and got["Z"] == 0


def test_bad_arguments_are_refused_and_a_stale_plan_writes_nothing(device_solver):
    s, t, lib = device_solver, device_solver.torch, device_solver.lib
    b = A.edge_batch(64)
    raw = s.upload(b)
    for bad in (0, -1):
        with pytest.raises(GdmixReError, match=r"\(-1\)"):                                # GDMIX_RE_EINVAL
            s.cap_samples(raw, b.uid, bad)
    with pytest.raises(GdmixReError, match="uid"):
        s.cap_samples(raw, b.uid[:-1], 64)
    with pytest.raises(GdmixReError):
        s.set_cap_small_max(1025)
    # 2^31 rows: refused from the counts alone, before anything is read
    some = t.zeros(64, dtype=t.int64, device=s.device)
    p = some.data_ptr()
    opts = S._CapOpts(64, A.SEED)
    counts = S._CapCounts()
    assert lib.gdmix_re_cap_workspace_bytes(1, 1 << 31) == 0 and lib.gdmix_re_cap_workspace_bytes(1 << 31, 1) == 0
    huge = S._RawBatch(1, 1 << 31, 8, p, p, p, p, p, p, None)
    assert lib.gdmix_re_cap_plan(s._h, C.byref(huge), p, C.byref(opts), p, 512, C.byref(counts), s._stream()) == -4      # GDMIX_RE_ERANGE
    assert b"2^31" in lib.gdmix_re_last_error()
    names = ("ent_row_ptr", "row_nnz_ptr", "col_global", "val", "y", "offset", "weight")
    c_raw = S._RawBatch(b.E, b.N, b.Z, *(raw[k].data_ptr() for k in names))
    nbytes = int(lib.gdmix_re_cap_workspace_bytes(b.E, b.N))
    ws, other = (t.empty(nbytes, dtype=t.uint8, device=s.device) for _ in range(2))
    uid = t.from_numpy(b.uid).to(s.device)
    st = s._stream()
    assert lib.gdmix_re_cap_plan(s._h, C.byref(c_raw), uid.data_ptr(), C.byref(opts), ws.data_ptr(), nbytes - 1, C.byref(counts), st) == -3      # GDMIX_RE_ENOMEM
    assert lib.gdmix_re_cap_plan(s._h, C.byref(c_raw), uid.data_ptr(), C.byref(opts), ws.data_ptr(), nbytes, C.byref(counts), st) == 0
    want = A.host_cap(b, 64)
    n_out, z_out = int(counts.kept), int(counts.kept_nnz)
    assert (n_out, z_out) == (want["y"].size, want["val"].size)
    sizes = dict(ent_row_ptr=b.E + 1, row_nnz_ptr=n_out + 1, col_global=z_out, val=z_out, y=n_out, offset=n_out, weight=n_out)
    outs = {k: t.full((sizes[k] + 1,), -7, dtype=raw[k].dtype if raw[k] is not None else t.float32, device=s.device) for k in names}
    kept_rows = t.full((n_out + 1,), -7, dtype=t.int32, device=s.device)
    c_out = S._DownsampleOut(n_out, z_out, *(outs[k].data_ptr() for k in names))
    # a second plan, on another workspace, makes the first one stale
    assert lib.gdmix_re_cap_plan(s._h, C.byref(c_raw), uid.data_ptr(), C.byref(opts), other.data_ptr(), nbytes, C.byref(counts), st) == 0
    assert lib.gdmix_re_cap_apply(s._h, C.byref(c_raw), C.byref(opts), ws.data_ptr(), nbytes, C.byref(c_out), kept_rows.data_ptr(), st) == -1
    assert b"last gdmix_re_cap_plan" in lib.gdmix_re_last_error()
    wrong = S._DownsampleOut(n_out - 1, z_out, *(outs[k].data_ptr() for k in names))
    assert lib.gdmix_re_cap_apply(s._h, C.byref(c_raw), C.byref(opts), other.data_ptr(), nbytes, C.byref(wrong), kept_rows.data_ptr(), st) == -1
    assert b"plan kept" in lib.gdmix_re_last_error()
    other_bound = S._CapOpts(65, A.SEED)
    assert lib.gdmix_re_cap_apply(s._h, C.byref(c_raw), C.byref(other_bound), other.data_ptr(), nbytes, C.byref(c_out), kept_rows.data_ptr(), st) == -1
    t.cuda.synchronize(s.device)
    assert all(bool((outs[k] == -7).all()) for k in names) and bool((kept_rows == -7).all())      # nothing was written
    assert lib.gdmix_re_cap_apply(s._h, C.byref(c_raw), C.byref(opts), other.data_ptr(), nbytes, C.byref(c_out), kept_rows.data_ptr(), st) == 0
    t.cuda.synchronize(s.device)
    for k in names:
        got = outs[k].cpu().numpy()
        assert np.array_equal(got[:-1], want[k]) and got[-1] == -7, k                     # ... and then everything, and nothing past the end
    assert np.array_equal(kept_rows.cpu().numpy()[:-1], want["kept_rows"]) and int(kept_rows[-1]) == -7


# ---- downstream: unchanged kernels on new input -------------------------------------------------------------------------------------------
K_SOLVE = A.K_SOLVE
KW = dict(l2=1.0, regularize_bias=True, has_intercept=True, m=10, max_iter=100, ftol=1e-12, variance_mode=0)


@pytest.fixture(scope="module")
def downstream(device_solver):
    """helpers.solve_batch at K = 16: the device's capped batch, the host-capped batch and its oracle.pack."""
    b = A.solve_batch()
    got = _cap(device_solver, b, K_SOLVE, keep_device=True)
    hb = A.capped_batch(b, K_SOLVE)
    return dict(b=b, got=got, hb=hb, pk=oracle.pack(hb.ent_row_ptr, hb.row_nnz_ptr, hb.col_global))


def test_the_pack_of_the_capped_batch_is_the_pack_of_the_host_capped_batch(device_solver, downstream):
    hb, pk = downstream["hb"], downstream["pk"]
    packed = device_solver.pack(downstream["got"]["device"], has_intercept=True)
    assert (packed.E, packed.N, packed.Z, packed.D) == (hb.E, hb.N, hb.Z, pk["D"])
    assert np.array_equal(packed.ent_feat_ptr().cpu().numpy(), pk["ent_feat_ptr"])
    assert np.array_equal(packed.ent_nnz_ptr().cpu().numpy(), pk["ent_nnz_ptr"])
    assert np.array_equal(packed.row_ptr().cpu().numpy(), pk["row_ptr"])
    assert np.array_equal(packed.csr_col().cpu().numpy(), pk["csr_col"])
    assert np.array_equal(packed.unique_global().cpu().numpy().astype(np.int64), pk["unique_global"])


def _device_batch(solver, downstream, kind):
    """(the device's capped batch with the labels of `kind`, the host-capped batch with the same labels): labels are drawn for the
    uncapped batch and cut by the cap, as a stage's would be."""
    lb = A.with_labels(downstream["b"], kind)
    hb = A.capped_batch(lb, K_SOLVE)
    raw = dict(downstream["got"]["device"])
    raw["y"] = solver.torch.from_numpy(hb.y).to(solver.device)
    return raw, hb


def test_a_linear_solve_of_the_capped_batch(device_solver, downstream):
    """fuzz_case.run_case's comparison and adjudication as re_linear_helpers.judge restates it for the squared loss, coefficients to 1e-5."""
    raw, hb = _device_batch(device_solver, downstream, "squared")
    packed = device_solver.pack(raw, has_intercept=True)
    res = device_solver.solve(packed, SolverOptions(linear=True, **KW)).to_host()
    j = H.judge(hb, downstream["pk"], KW, None, res, packed.coef_ptr_host(), theta_tol=1e-5)
    ok = j["strict_ok"]
    print(f"linear on the capped batch: {ok.mean():.1%} strict, worst error {j['err'].max():.3e}; adjudicated {len(j['adjudicated'])}")
    assert not j["problems"], j["problems"][:3]
    assert ok.mean() >= 0.5
    assert np.array_equal(res["status"][ok], j["ref"]["status"][ok]) and np.array_equal(res["nit"][ok], j["ref"]["nit"][ok])
    assert j["err"].max() <= 1e-5


def test_a_logistic_solve_of_the_capped_batch(device_solver, downstream):
    """Entities the oracle reproduces under rounding-sized noise (fuzz_case's STRICT): the same status and iteration count; every entity's
    coefficients within 1e-5, the others' against the oracle run to the minimum. (A regularised intercept: every entity has a minimiser.)"""
    raw, hb = _device_batch(device_solver, downstream, "logistic")
    pk = downstream["pk"]
    packed = device_solver.pack(raw, has_intercept=True)
    res = device_solver.solve(packed, SolverOptions(**KW)).to_host()
    cp = packed.coef_ptr_host()
    o = oracle.make_opts(**dict(KW, linear=False, sum_loss=False))
    ref, strict, _, _ = H.oracle_strict(hb, pk, o, None, int(cp[-1]))
    err = fuzz_case.per_entity_rel_err(res["theta"], ref["theta"], cp)
    print(f"logistic on the capped batch: {strict.mean():.1%} strict, worst strict error {err[strict].max():.3e}")
    assert strict.mean() >= 0.5
    assert np.array_equal(res["status"][strict], ref["status"][strict]) and np.array_equal(res["nit"][strict], ref["nit"][strict])
    assert err[strict].max() <= 1e-5
    tight = oracle.solve(pk, hb.val, hb.y, hb.offset, hb.weight, oracle.make_opts(**dict(KW, max_iter=5000, ftol=1e-15)))
    assert fuzz_case.per_entity_rel_err(res["theta"], tight["theta"], cp)[~strict].max(initial=0.0) <= 1e-5


def test_a_poisson_solve_of_the_capped_batch(device_solver, downstream):
    """(The C oracle has no Poisson loss: scipy on the host-capped batch, by re_poisson_helpers' rule, as every Poisson test here.)"""
    raw, hb = _device_batch(device_solver, downstream, "poisson")
    packed = device_solver.pack(raw, has_intercept=True)
    res = device_solver.solve(packed, SolverOptions(loss="poisson", **KW)).to_host()
    cp = packed.coef_ptr_host()
    P.compare(res, P.reference(hb, downstream["pk"], KW, None, cp, entities=np.arange(hb.E)), cp)


# ---- the product path -------------------------------------------------------------------------------------------------------------------
BOUND, JOB_SEED = 10, 3


def _read_models(path):
    from gdmix_amd.io import avro
    return {r["modelId"]: {(m["name"], m["term"]): m["value"] for m in r["means"]} for r in avro.read_file(path)}


def _job_batch(model_type):
    from gdmix_amd import synthetic
    if model_type == "linear_regression":
        return H.small_job_batch(E=60, seed=41, real=True)
    b = H.small_job_batch(E=60, seed=42, real=False)
    return synthetic.with_count_labels(b, 42) if model_type == "poisson_regression" else b


def _reference_fit(model_type, fb, pk):
    """The fit of the job's options (re_linear_helpers.job_argv) on the capped batch, weights included -> theta [P] in pk's index space."""
    cp = np.asarray(pk["ent_feat_ptr"]) + np.arange(fb.E + 1)
    kw = dict(l2=1.0, regularize_bias=model_type == "logistic_regression", has_intercept=True, m=10, max_iter=100, ftol=1e-12)
    if model_type == "poisson_regression":
        ref = P.reference(fb, pk, kw, None, cp, entities=np.arange(fb.E))
        return np.concatenate([ref["theta"][e] for e in range(fb.E)]), cp
    return oracle.solve(pk, fb.val, fb.y, fb.offset, fb.weight, oracle.make_opts(linear=model_type == "linear_regression", **kw))["theta"], cp


def _argv(root, action, model_type, extra):
    argv = H.job_argv(root, action, model_type=model_type, extra=extra)
    if model_type == "logistic_regression":
        argv = [a.replace("--regularize_bias=False", "--regularize_bias=True") for a in argv]
    return argv


def _cli_case(tmp_path, model_type, ratio=None, inference_without=False):
    from gdmix_amd import chain
    from test_gpu_chain import _scores_by_uid, _ulps
    b = _job_batch(model_type)
    assert b.weight is None and 0 < (b.ent_n() > BOUND).sum() < b.E
    root = str(tmp_path)
    H.write_job(root, b)
    flags = [f"--active_data_upper_bound={BOUND}", f"--active_data_seed={JOB_SEED}"]
    more = [] if ratio is None else [f"--features_to_samples_ratio={ratio}"]
    chain.run_stage(_argv(root, "train", model_type, flags + more + [f"--metric_output_dir={root}/metrics"]), child_process=True)
    fb = A.capped_batch(b, BOUND, JOB_SEED)
    assert np.array_equal(fb.ent_n(), np.minimum(b.ent_n(), BOUND))
    if ratio is not None:      # the cap runs first: the selection sees the capped batch, and its n_e is the kept count
        fb, _, _, counts = fs.select_batch(fb, ratio)
        assert counts["affected"] > 0
    pk, pkf = oracle.pack(b.ent_row_ptr, b.row_nnz_ptr, b.col_global), oracle.pack(fb.ent_row_ptr, fb.row_nnz_ptr, fb.col_global)
    theta, cpf = _reference_fit(model_type, fb, pkf)
    got = _read_models(os.path.join(root, "models", "part-00000.avro"))
    assert set(got) == set(b.entity_ids)
    fp, fpf = pk["ent_feat_ptr"], pkf["ent_feat_ptr"]
    written = np.zeros(int(fp[-1]) + b.E)
    worst = 0.0
    icpt = ("(INTERCEPT)", "")
    for e, eid in enumerate(b.entity_ids):
        in_model = [(f"f{int(g)}", "") for g in pkf["unique_global"][fpf[e]:fpf[e + 1]]]
        assert set(got[eid]) <= set(in_model) | {icpt}, eid                               # a feature of passive rows alone is not in the model
        want = theta[cpf[e]:cpf[e + 1]]
        want = np.where(np.abs(want) <= 1e-4, 0.0, want)
        have = np.array([got[eid].get(nm, 0.0) for nm in [icpt] + in_model])
        worst = max(worst, float(np.abs(have - want).max() / max(1.0, np.abs(want).max())))
        written[fp[e] + e:fp[e + 1] + e + 1] = [got[eid].get(nm, 0.0) for nm in [icpt] + [(f"f{int(g)}", "") for g in pk["unique_global"][fp[e]:fp[e + 1]]]]
    print(f"{model_type}: model Avro against the reference fit on the host-capped data: worst {worst:.3e}")
    assert worst <= 1e-5, worst
    lo, _ = oracle.score(pk, b.val, b.offset, written, True)      # the written model on EVERY row, passive ones included
    order = np.argsort(b.uid, kind="stable")
    for d in ("trainingScores", "validationScores"):
        s = _scores_by_uid(os.path.join(root, d))
        assert np.array_equal(s["uid"], b.uid[order]), d
        assert _ulps(s["score"], lo.astype(np.float32)[order]).max() <= 1.0, d
    with open(os.path.join(root, "metrics", "evalSummary.json")) as fh:
        summary = json.load(fh)
    assert summary["training"]["n"] == b.N and summary["validation"]["n"] == b.N
    chain.run_stage(_argv(root, "inference", model_type, flags + more), child_process=True)
    s = _scores_by_uid(os.path.join(root, "inferenceScores"))     # inference accepts and ignores the flags
    assert np.array_equal(s["uid"], b.uid[order]) and _ulps(s["score"], lo.astype(np.float32)[order]).max() <= 1.0
    if inference_without:
        chain.run_stage(_argv(root, "inference", model_type, []))      # (in this process: the comparison needs no third child)
        plain = _scores_by_uid(os.path.join(root, "inferenceScores"))
        assert np.array_equal(plain["uid"], s["uid"]) and np.array_equal(plain["score"].view(np.uint32), s["score"].view(np.uint32))


@pytest.mark.parametrize("model_type", ["logistic_regression", "linear_regression", "poisson_regression"])
def test_cli_child_process_trains_on_the_capped_data_and_scores_every_row(tmp_path, model_type):
    """One partition (60 entities, 12 samples each on average, bound 10) through `python -m gdmix_amd.gdmix --active_data_upper_bound=10` as a
    child process: models within 1e-5 of the reference fit on the host-capped data; the score files hold every row, each score x . theta +
    offset of the written model to 1 ulp of the Avro float; evalSummary.json counts every row; inference ignores the flags."""
    _cli_case(tmp_path, model_type, inference_without=model_type == "logistic_regression")


def test_cli_the_selection_sees_the_capped_batch(tmp_path):
    _cli_case(tmp_path, "linear_regression", ratio=0.5)


def test_cli_a_bound_above_every_entity_is_a_run_without_the_flag(tmp_path):
    from gdmix_amd import chain
    b = _job_batch("logistic_regression")
    models = []
    for name, extra in (("plain", []), ("bound", [f"--active_data_upper_bound={int(b.ent_n().max())}"])):
        root = str(tmp_path / name)
        os.makedirs(root)
        H.write_job(root, b)
        chain.run_stage(_argv(root, "train", "logistic_regression", extra), child_process=True)
        models.append(_read_models(os.path.join(root, "models", "part-00000.avro")))
    plain, bound = models
    assert set(plain) == set(bound) == set(b.entity_ids)
    worst = 0.0
    for eid in plain:
        assert set(plain[eid]) == set(bound[eid]), eid
        for nm, v in plain[eid].items():
            worst = max(worst, abs(bound[eid][nm] - v) / max(abs(v), 1e-300))
    print(f"bound above every entity against no flag: worst relative difference {worst:.3e}")
    assert worst <= 1e-12, worst


@pytest.mark.parametrize("flag,message", [
    ("--incremental_training=True", "--active_data_upper_bound does not run with --incremental_training"),
    ("--l2_reg_weights=1,0.1", "--active_data_upper_bound does not run with --l2_reg_weights"),
])
def test_cli_refuses_what_the_cap_does_not_run_with(tmp_path, flag, message):
    from gdmix_amd import chain
    root = str(tmp_path)
    H.write_job(root, H.small_job_batch(E=4, seed=43))
    with pytest.raises(RuntimeError) as err:
        chain.run_stage(H.job_argv(root, "train", extra=["--active_data_upper_bound=5", flag]), child_process=True)
    assert "stage exited with" in str(err.value) and message in str(err.value)
    assert not os.path.exists(os.path.join(root, "models"))
