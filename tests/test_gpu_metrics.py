"""The device evaluator (include/gdmix_re.h "evaluation", csrc/re_evaluate.hip, gdmix_amd/metrics.py) against the numpy reference of
tests/metrics_reference.py: exact integers per entity and over a stage, both mechanisms, the SSE trees, NaN handling and limits, and
the product path (a stage that writes its metric while it scores; python -m gdmix_amd.evaluate on its score files)."""
import json
import math
import os
from fractions import Fraction

import numpy as np
import pytest

from gdmix_amd import metrics
from gdmix_amd.solver import GdmixReError

from metrics_reference import per_entity_reference, sse_reference, two_u_reference

pytestmark = pytest.mark.gpu

BOUNDARY_SIZES = [16, 17, 32, 33, 64, 65, 1, 0, 15, 31, 63, 2, 66, 128, 5]


def _samples(rng, n, ties=False):
    s = rng.standard_normal(n)
    if ties:
        s = np.round(s, 1)
    s = s.astype(np.float32)
    y = (rng.random(n) < 1.0 / (1.0 + np.exp(-s.astype(np.float64)))).astype(np.float32)
    return s, y


def _sprinkle(rng, s):
    """-0.0, +-inf and a few exact zeros at random places."""
    for v in (-0.0, 0.0, np.inf, -np.inf, -0.0, np.inf, 0.0, -np.inf):
        s[rng.integers(0, s.size, max(1, s.size // 5000))] = v
    return s


def _case(name):
    rng = np.random.default_rng({"c2": 1, "ragged": 2, "one": 3, "ml": 4, "ties": 5}[name])
    if name == "c2":
        sizes = np.full(20_000, 16, np.int64)
    elif name == "ragged":
        sizes = np.concatenate([BOUNDARY_SIZES, rng.integers(1, 301, 3000)]).astype(np.int64)
    elif name == "one":
        sizes = np.array([200_000], np.int64)
    elif name == "ml":
        from gdmix_amd import synthetic
        b = synthetic.make_movielens_20m(kind="per_movie", seed=200, entities=4000)
        rp = np.asarray(b.ent_row_ptr, np.int64)
        keep = int(np.searchsorted(rp, 2_000_000, side="right")) - 1
        sizes = np.diff(rp[:keep + 1])
    else:
        sizes = np.concatenate([BOUNDARY_SIZES, rng.integers(1, 200, 2000), [5000]]).astype(np.int64)
    rp = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    s, y = _samples(rng, int(rp[-1]), ties=(name == "ties"))
    s = _sprinkle(rng, s)
    if name in ("ragged", "ties"):      # single-class entities: the NaN pattern
        for e in (3, 20, 40, 41):
            y[rp[e]:rp[e + 1]] = float(e % 2)
    return rp, s, y


def _check_entities(got, ref, what):
    h = metrics.entities_to_host(got)
    assert [int(x) for x in h["two_u"]] == [int(x) for x in ref["two_u"]], what
    for k in ("n_pos", "n_neg", "n_nan"):
        assert np.array_equal(h[k].astype(np.int64), ref[k]), (what, k)
    raw = got["auc"].cpu().numpy()
    assert np.array_equal(np.isnan(raw), np.isnan(ref["auc"])), what
    assert np.array_equal(raw.view(np.uint64)[~np.isnan(raw)], ref["auc"].view(np.uint64)[~np.isnan(raw)]), what     # bit-equal
    return h


@pytest.fixture(scope="module")
def evaluator(device_solver):
    ev = metrics.DeviceEvaluator(device_solver)
    yield ev
    ev.set_small_max(64)


@pytest.mark.parametrize("name", ["c2", "ragged", "one", "ml", "ties"])
def test_per_entity_integers_are_exact_and_both_mechanisms_agree(evaluator, name):
    """Per entity: twoU, n_pos, n_neg equal the reference's integers, auc[e] is bit-equal to two_u / (2.0 * n_pos * n_neg) in numpy, the
    NaN pattern (single-class entities) is the same. Then every entity forced through the sort path (and with the limit at 20: both
    paths in one batch): identical integers. SSE and MSE per entity against math.fsum to 1e-12, the same bits in two runs."""
    rp, s, y = _case(name)
    if name == "ragged":
        assert all(n in np.diff(rp) for n in (16, 17, 32, 33, 64, 65))
    ref = per_entity_reference(rp, s, y)
    evaluator.set_small_max(64)
    got = evaluator.entities(rp, s, y)
    _check_entities(got, ref, name)
    for limit in (0, 20):
        evaluator.set_small_max(limit)
        _check_entities(evaluator.entities(rp, s, y), ref, (name, limit))
    # SSE / MSE on the same batch with its infinite scores (an infinite error) set to zero
    s2 = np.where(np.isinf(s), np.float32(0.0), s).astype(np.float32)
    want = per_entity_reference(rp, s2, y)["sse"]
    n = np.diff(rp)
    for limit in (64, 0):
        evaluator.set_small_max(limit)
        got = evaluator.entities(rp, s2, y)
        h = metrics.entities_to_host(got)
        rel = np.abs(h["sse"] - want) / np.maximum(want, 1e-300)
        print(f"{name}, small limit {limit}: per-entity SSE worst relative error {rel.max():.3e}")
        assert rel.max() <= 1e-12
        assert np.all(np.abs(h["mse"][n > 0] - want[n > 0] / n[n > 0]) <= 1e-12 * want[n > 0] / n[n > 0]) and np.isnan(h["mse"][n == 0]).all()
        again = evaluator.entities(rp, s2, y)
        assert np.array_equal(again["sse"].cpu().numpy().view(np.uint64), got["sse"].cpu().numpy().view(np.uint64))
    evaluator.set_small_max(64)


def test_entities_of_a_packed_batch(device_solver, evaluator):
    """The form the pipeline uses: a PackedBatch (its labels) and the scores gdmix_re_score wrote for it."""
    from gdmix_amd import synthetic
    raw = synthetic.make_batch(E=300, seed=3)
    packed = device_solver.pack(raw, has_intercept=True)
    theta = np.random.default_rng(0).standard_normal(packed.P) * 0.3
    logit, _ = device_solver.score(packed, theta)
    got = evaluator.entities(packed, logit)
    ref = per_entity_reference(np.asarray(raw.ent_row_ptr), logit.cpu().numpy(), np.asarray(raw.y, np.float32))
    _check_entities(got, ref, "packed")


def _global_reference(s, y):
    two_u, n_pos, n_neg, n_nan = two_u_reference(s, y)
    return dict(two_u=two_u, n_pos=n_pos, n_neg=n_neg, n_nan=n_nan)


def test_global_metric_is_that_of_the_concatenation(evaluator):
    """One batch, seven uneven batches, the batches in reverse order: the same integers, those of the reference; auc is the correctly
    rounded quotient; MSE against math.fsum to 1e-12 and the same bits in two runs."""
    rng = np.random.default_rng(17)
    s, y = _samples(rng, 300_001, ties=True)
    s = _sprinkle(rng, s)
    ref = _global_reference(s, y)
    cuts = [0, 1, 70, 5000, 5001, 120_000, 250_000, s.size]
    runs = []
    for order in ([(0, s.size)], list(zip(cuts[:-1], cuts[1:])), list(zip(cuts[:-1], cuts[1:]))[::-1], [(0, s.size)]):
        evaluator.reset()
        for a, b in order:
            evaluator.add(s[a:b], y[a:b])
        runs.append(evaluator.finish())
    for r in runs:
        assert {k: r[k] for k in ref} == ref
        assert r["n"] == s.size
        assert r["auc"] == float(Fraction(ref["two_u"], 2 * ref["n_pos"] * ref["n_neg"]))
    finite = np.isfinite(s)
    evaluator.reset()
    evaluator.add(s[finite], y[finite])
    a = evaluator.finish()
    evaluator.reset()
    evaluator.add(s[finite], y[finite])
    b = evaluator.finish()
    want = sse_reference(s[finite], y[finite])
    print(f"global SSE relative error {abs(a['sse'] - want) / want:.3e}")
    assert abs(a["sse"] - want) <= 1e-12 * want and a["sse"] == b["sse"]
    assert abs(a["mse"] - want / int(finite.sum())) <= 1e-12 * want / int(finite.sum())
    assert math.isinf(runs[0]["sse"])      # an infinite score has an infinite error


def test_global_metric_at_c2_size(evaluator):
    """16 M samples (the C2 stage) against the numpy reference, added as sixteen partitions."""
    rng = np.random.default_rng(23)
    n = 16_000_000
    s = rng.standard_normal(n).astype(np.float32)
    y = (rng.random(n, dtype=np.float32) < 1.0 / (1.0 + np.exp(-s))).astype(np.float32)
    ref = _global_reference(s, y)
    evaluator.reset()
    evaluator.reserve(n)
    for a in range(0, n, 1_000_000):
        evaluator.add(s[a:a + 1_000_000], y[a:a + 1_000_000])
    r = evaluator.finish()
    assert {k: r[k] for k in ref} == ref
    assert r["auc"] == float(Fraction(ref["two_u"], 2 * ref["n_pos"] * ref["n_neg"]))
    d = y.astype(np.float64) - s.astype(np.float64)
    want = math.fsum((d * d).tolist())
    print(f"16 M samples: AUC {r['auc']:.6f}, SSE relative error {abs(r['sse'] - want) / want:.3e}")
    assert abs(r["sse"] - want) <= 1e-12 * want


def test_nan_scores_are_counted_and_left_out(evaluator):
    rng = np.random.default_rng(29)
    s, y = _samples(rng, 5000)
    rp = np.concatenate([[0], np.cumsum(np.concatenate([[10, 40, 700], np.full(425, 10)]))]).astype(np.int64)
    assert rp[-1] == s.size
    where = [3, 30, 500]      # one in a row-sized entity, one in a wavefront-sized one, one in a sorted one
    clean = np.delete(s, where), np.delete(y, where)
    s[where] = np.nan
    ref = _global_reference(clean[0], clean[1])
    evaluator.reset()
    evaluator.add(s, y)
    r = evaluator.finish()
    assert r["n_nan"] == 3 and r["n"] == s.size
    assert (r["two_u"], r["n_pos"], r["n_neg"]) == (ref["two_u"], ref["n_pos"], ref["n_neg"])
    want = sse_reference(clean[0], clean[1])
    assert abs(r["sse"] - want) <= 1e-12 * want
    assert math.isnan(r["auc"]) and math.isnan(r["mse"])
    pe = per_entity_reference(rp, s, y)
    assert pe["n_nan"][:3].tolist() == [1, 1, 1]
    got = evaluator.entities(rp, s, y)
    h = _check_entities(got, pe, "nan")
    assert np.all(np.abs(h["sse"] - pe["sse"]) <= 1e-12 * pe["sse"])
    assert np.isnan(h["auc"][:3]).all() and np.isnan(h["mse"][:3]).all() and not np.isnan(h["mse"][3:]).any()


def test_small_buffers_and_limits_are_errors_not_faults(device_solver, evaluator):
    import ctypes as C
    from gdmix_amd import solver as S
    t = device_solver.torch
    rng = np.random.default_rng(31)
    s, y = _samples(rng, 4096)
    rp = np.arange(0, 4097, 128, dtype=np.int64)
    with pytest.raises(GdmixReError, match=r"\(-3\).*workspace"):
        evaluator.entities(rp, s, y, workspace_bytes=1024)
    sd, yd = t.from_numpy(s).to(device_solver.device), t.from_numpy(y).to(device_solver.device)
    keys = t.empty(4000, dtype=t.int64, device=device_solver.device)
    state = t.empty(S.EVAL_ACC_STATE_BYTES, dtype=t.uint8, device=device_solver.device)
    acc = S._EvalAcc(keys.data_ptr(), 4000, 0, state.data_ptr())
    lib, h, st = device_solver.lib, device_solver._h, device_solver._stream()
    assert lib.gdmix_re_eval_acc_reset(h, C.byref(acc), st) == 0
    assert lib.gdmix_re_eval_acc_add(h, C.byref(acc), sd.data_ptr(), yd.data_ptr(), 4096, st) == -3
    assert b"key buffer" in lib.gdmix_re_last_error() and acc.count == 0
    assert lib.gdmix_re_eval_acc_add(h, C.byref(acc), sd.data_ptr(), yd.data_ptr(), 4000, st) == 0 and acc.count == 4000
    tot = S._EvalTotals()
    ws = t.empty(256, dtype=t.uint8, device=device_solver.device)
    assert lib.gdmix_re_eval_acc_finish(h, C.byref(acc), ws.data_ptr(), 256, C.byref(tot), st) == -3
    assert b"workspace" in lib.gdmix_re_last_error()
    # the limits are refused on the host, before anything is launched
    assert lib.gdmix_re_eval_workspace_bytes(10, 1 << 31) == 0
    out = S._EvalOut()
    assert lib.gdmix_re_eval_entities(h, sd.data_ptr(), 1, 1 << 31, sd.data_ptr(), yd.data_ptr(), C.byref(out), ws.data_ptr(), 256, st) == -4
    assert lib.gdmix_re_eval_acc_add(h, C.byref(acc), sd.data_ptr(), yd.data_ptr(), (1 << 31) - 4000, st) == -4 and acc.count == 4000
    device_solver.torch.cuda.synchronize()


# ---- through the product path --------------------------------------------------------------------------------------------------------
def _files(d):
    """relative path -> content: the bytes of a file, the schema and records of an Avro file (its sync marker is random)."""
    from gdmix_amd.io import avro
    out = {}
    for r, _, fs in os.walk(d):
        for fn in fs:
            p = os.path.join(r, fn)
            if fn.endswith(".avro"):
                out[os.path.relpath(p, d)] = (json.dumps(avro.read_schema(p), sort_keys=True), repr(list(avro.read_file(p))))
            else:
                with open(p, "rb") as f:
                    out[os.path.relpath(p, d)] = f.read()
    return out


def _stage_scores(root, stage, which):
    from gdmix_amd import chain
    _, sc, _, lab = chain.read_scores(os.path.join(root, stage, "trainingScores" if which == "training" else "validationScores"))
    return sc, lab


def _per_entity_records(root, stage):
    from gdmix_amd.io import avro
    d = os.path.join(root, stage, "metrics", "perEntity")
    out = {}
    for fn in sorted(os.listdir(d)):
        assert fn.startswith("part-") and fn.endswith(".avro")
        out[fn] = list(avro.read_file(os.path.join(d, fn)))
    return out


@pytest.fixture(scope="module")
def chains(tmp_path_factory):
    """The 100 k-rating chain of tests/test_gpu_chain.py, in process: logistic and linear with the device metric, logistic without."""
    from gdmix_amd import chain
    data = chain.make_dataset()
    roots = {}
    for name, kw in (("auc", dict()), ("mse", dict(model_type="linear_regression")), ("off", dict(device_metrics=False))):
        roots[name] = str(tmp_path_factory.mktemp(name))
        roots[name + "_result"] = chain.run_chain(roots[name], data, upper_bounds={"per_user": 200, "per_movie": 300}, **kw)
    return data, roots


@pytest.mark.parametrize("metric", ["auc", "mse"])
def test_stage_summary_is_the_exact_metric_of_its_score_files(chains, metric):
    from gdmix_amd import chain
    data, roots = chains
    root, result = roots[metric], roots[metric + "_result"]
    ent_of = {"per_user": data["user"], "per_movie": data["movie"]}
    for stage in ("per_user", "per_movie"):
        with open(os.path.join(root, stage, "metrics", "evalSummary.json")) as f:
            summary = json.load(f)
        for which in ("training", "validation"):
            sc, lab = _stage_scores(root, stage, which)
            two_u, n_pos, n_neg, n_nan = two_u_reference(sc, lab)
            blk = summary[which]
            assert (blk["n"], blk["n_nan"]) == (sc.size, 0) and n_nan == 0
            if metric == "auc":
                assert (blk["two_u"], blk["n_pos"], blk["n_neg"]) == (two_u, n_pos, n_neg)
                assert blk["auc"] == float(Fraction(two_u, 2 * n_pos * n_neg))
            else:
                want = sse_reference(sc, lab) / sc.size
                print(f"{stage} {which}: MSE {blk['mse']!r}, reference {want!r}")
                assert abs(blk["mse"] - want) <= 1e-12 * want
            assert result[stage][("train" if which == "training" else "validation") + f"_{metric}_device"] == blk[metric]
        assert summary["data"] == "validation" and summary[metric] == summary["validation"][metric]
        # one record per scored entity and file, with the reference's integers
        uid_tr, sc_tr, _, lab_tr = chain.read_scores(os.path.join(root, stage, "trainingScores"))
        uid_va, sc_va, _, lab_va = chain.read_scores(os.path.join(root, stage, "validationScores"))
        ent_by_uid = dict(zip(data["uid"].tolist(), ent_of[stage].tolist()))
        recs = _per_entity_records(root, stage)
        for which, uid, sc, lab in (("training", uid_tr, sc_tr, lab_tr), ("validation", uid_va, sc_va, lab_va)):
            mine = [r for fn, rs in recs.items() if fn.startswith(f"part-{which}-") for r in rs]
            assert sum(r["n"] for r in mine) == uid.size
            ent = np.array([ent_by_uid[u] for u in uid.tolist()])
            want_n, want_pos = {}, {}
            for e, y in zip(ent.tolist(), (lab > 0.5).tolist()):
                want_n[e] = want_n.get(e, 0) + 1
                want_pos[e] = want_pos.get(e, 0) + int(y)
            got_n, got_pos = {}, {}
            for r in mine:      # (an entity above the upper bound is scored twice: its active and its passive samples)
                e = int(r["entityId"])
                got_n[e] = got_n.get(e, 0) + r["n"]
                got_pos[e] = got_pos.get(e, 0) + r["n_pos"]
            assert got_n == want_n and got_pos == want_pos
        # the AUC / MSE of single records: every validation entity against the reference on its samples
        ent = np.array([ent_by_uid[u] for u in uid_va.tolist()])
        checked = 0
        for r in (r for fn, rs in recs.items() if fn.startswith("part-validation-") for r in rs):
            m = ent == int(r["entityId"])
            tu, p, n, _ = two_u_reference(sc_va[m], lab_va[m])
            assert (r["n"], r["n_pos"]) == (int(m.sum()), p)
            assert r["auc"] == (None if p == 0 or n == 0 else tu / (2.0 * p * n))
            want = sse_reference(sc_va[m], lab_va[m]) / int(m.sum())
            assert abs(r["mse"] - want) <= 1e-12 * want
            checked += 1
        assert checked > 500


def test_without_metric_output_dir_the_stage_writes_what_it_wrote(chains):
    """metric_output_dir unset: no metrics directory, and every file of the stage's output holds what the same stage writes with the
    metric on (the metric adds files and changes none): the same files, the same bytes, for Avro files the same schema and records."""
    _, roots = chains
    for stage in ("per_user", "per_movie"):
        off = _files(os.path.join(roots["off"], stage))
        on = _files(os.path.join(roots["auc"], stage))
        assert not any(k.startswith("metrics") for k in off) and any(k.startswith("metrics") for k in on)
        assert off == {k: v for k, v in on.items() if not k.startswith("metrics")}
    assert "train_auc_device" not in roots["off_result"]["per_user"]


@pytest.mark.parametrize("metric", ["auc", "mse"])
def test_evaluate_command_line_writes_the_same_number(chains, metric, device_solver, tmp_path):
    from gdmix_amd import evaluate
    _, roots = chains
    root = roots[metric]
    for stage in ("per_user", "per_movie"):
        out = str(tmp_path / stage)
        v = evaluate.run(["--metricsInputDir", os.path.join(root, stage, "validationScores"), "--outputMetricFile", out, "--labelColumnName", "response",
                          "--predictionColumnName", "predictionScore", "--metricName", metric], solver=device_solver)
        with open(os.path.join(out, "evalSummary.json")) as f:
            assert json.load(f) == {metric: v}
        with open(os.path.join(root, stage, "metrics", "evalSummary.json")) as f:
            stage_v = json.load(f)["validation"][metric]
        # the AUC is a quotient of exact integers; the SSE was added up partition by partition in the stage and in one batch here
        assert stage_v == v if metric == "auc" else abs(stage_v - v) <= 1e-12 * v
