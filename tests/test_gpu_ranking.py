"""The ranking evaluation on the device (include/gdmix_re.h, "(ABI 27) ranking evaluation"; csrc/re_evaluate.hip, csrc/re_evaluate_poisson.hip;
gdmix_amd/metrics.py) against the exact reference of tests/ranking_reference.py: the four integers of precision@k per entity on both
paths, the AUC outputs of the same call bit for bit, the log loss within its stated bound, the error codes, and a stage that writes the
requested evaluators while it scores."""
import ctypes as C
import functools
import json
import math
import os
import shutil

import numpy as np
import pytest

from gdmix_amd import metrics
from gdmix_amd import solver as S
from gdmix_amd.solver import GdmixReError

import ranking_reference as ref

pytestmark = pytest.mark.gpu

# the lane-width edges of the small path, an empty entity, entities across the 4 096-key tile of the rank pass
SIZES = [16, 17, 32, 33, 64, 65, 1, 0, 15, 31, 63, 2, 66, 128, 5, 2049, 5000]
KS = ([1, 5, 16, 64], [65, 4096, 5000, 2**31 - 1])
COUNTS = ("hits_sure", "slots", "tie_pos", "tie_size")


@functools.lru_cache(maxsize=None)
def _case(name):
    """-> (ent_row_ptr, score, label, {ks tuple: reference counts}); built once per name and never changed."""
    rng = np.random.default_rng({"continuous": 101, "halves": 102, "special": 103, "one_small": 104, "one_large": 105}[name])
    sizes = {"one_small": [37], "one_large": [4100]}.get(name, SIZES)
    rp = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    n = int(rp[-1])
    s = rng.standard_normal(n)
    if name in ("halves", "special", "one_large"):
        s = np.round(s * 2.0) / 2.0
    s = s.astype(np.float32)
    y = (rng.random(n) < 1.0 / (1.0 + np.exp(-s.astype(np.float64)))).astype(np.float32)
    if name == "special":
        ent = lambda e: slice(int(rp[e]), int(rp[e + 1]))
        for v in (np.nan, -0.0, 0.0, np.inf, -np.inf, np.nan, -0.0, np.inf, 0.0, -np.inf):
            s[rng.integers(0, n, 12)] = v
        s[ent(0)] = 0.25                    # 16: all scores equal
        s[ent(13)] = -1.5                   # 128 (sort path): all scores equal
        y[ent(2)] = 1.0                     # 32: all positive
        y[ent(3)] = 0.0                     # 33: all negative
        y[ent(15)] = 1.0                    # 2 049 (sort path): all positive
        s[rp[5]:rp[5] + 3] = [np.inf, np.inf, np.nan]       # 65: ties at +inf next to a NaN on the sort path
        s[rp[1]:rp[1] + 4] = [0.0, -0.0, 0.0, -0.0]         # 17: the two zeros are one score
    return rp, s, y, {tuple(ks): ref.per_entity_counts(rp, s, y, ks) for ks in KS}


@pytest.fixture(scope="module")
def rankers(device_solver):
    made = {tuple(ks): metrics.RankingEvaluator(device_solver, ks) for ks in KS}
    yield made
    made[tuple(KS[0])].set_small_max(64)


def _assert_counts(got, want, what):
    for name in COUNTS:
        g = got[name].cpu().numpy().astype(np.int64)
        assert g.shape == want[name].shape, (what, name)
        assert np.array_equal(g, want[name]), (what, name, np.argwhere(g != want[name])[:5].tolist())


@pytest.mark.parametrize("name", ["continuous", "halves", "special", "one_small", "one_large"])
def test_topk_integers_are_exact_on_both_paths(rankers, name):
    """hits_sure, slots, tie_pos, tie_size per entity and k equal the reference's integers, with the small path (limit 64), with every
    entity through the sort path (limit 0) and with both in one batch (limit 20), for both lists of k; and without auc_out."""
    rp, s, y, want = _case(name)
    if name == "halves":      # the tie case is not vacuous: the cut of a quarter of the pairs with n > k goes through a mixed tie group
        pairs = cut = 0
        for ks in KS:
            w = want[tuple(ks)]
            for j, k in enumerate(ks):
                big = w["n"] > k
                pairs += int(big.sum())
                cut += int((big & (w["slots"][j] < w["tie_size"][j]) & (0 < w["tie_pos"][j]) & (w["tie_pos"][j] < w["tie_size"][j])).sum())
        print(f"halves: {cut} of {pairs} (entity, k) pairs with n > k cut a tie group of both classes")
        assert pairs == 49 and 4 * cut >= pairs
    if name == "special":
        w = want[tuple(KS[0])]
        assert w["tie_size"][0, 0] == 16 and w["tie_size"][3, 13] == 128 and w["hits_sure"][3, 2] == w["n"][2] > 0 and w["hits_sure"][:, 3].sum() == 0
        assert w["n"][5] < 65 and np.isnan(s).any() and np.isinf(s).any()
    for ks in KS:
        ev = rankers[tuple(ks)]
        for limit in (64, 0, 20):
            ev.set_small_max(limit)
            _assert_counts(ev.entities(rp, s, y), want[tuple(ks)], (name, ks, limit))
        ev.set_small_max(64)
        _assert_counts(ev.entities(rp, s, y, with_auc=False), want[tuple(ks)], (name, ks, "no auc_out"))
        ev.set_small_max(0)
        _assert_counts(ev.entities(rp, s, y, with_auc=False), want[tuple(ks)], (name, ks, "no auc_out, sorted"))
        ev.set_small_max(64)


def test_host_division_of_the_device_counts(rankers):
    """ranking_entities_to_host on the device's tensors: precision_at_k is the correctly rounded H / k, NaN where a score is NaN."""
    rp, s, y, _ = _case("special")
    ks = KS[0]
    ev = rankers[tuple(ks)]
    h = ev.to_host(ev.entities(rp, s, y))
    for k in ks:
        got = h[metrics.precision_key(k)]
        for e in range(rp.size - 1):
            se, ye = s[rp[e]:rp[e + 1]], y[rp[e]:rp[e + 1]]
            if np.isnan(se).any():
                assert math.isnan(got[e]), (k, e)
            else:
                assert got[e] == float(ref.precision(se, ye, k)), (k, e)
    assert np.isnan(s).any()


@pytest.mark.parametrize("name", ["halves", "special", "one_large"])
def test_auc_out_of_the_ranking_call_is_that_of_eval_entities_bit_for_bit(device_solver, rankers, name):
    rp, s, y, _ = _case(name)
    plain = metrics.DeviceEvaluator(device_solver)
    ev = rankers[tuple(KS[0])]
    for limit in (64, 0, 20):
        ev.set_small_max(limit)
        a, b = plain.entities(rp, s, y), ev.entities(rp, s, y)
        for key, _ in metrics.DeviceEvaluator.OUTPUTS:
            x, z = a[key].cpu().numpy(), b[key].cpu().numpy()
            assert x.dtype == z.dtype and np.array_equal(x.view(np.uint8), z.view(np.uint8)), (name, limit, key)
    ev.set_small_max(64)


def _ll_bound(sum_terms, n):
    """include/gdmix_re.h, the log loss: |LL - exact| <= 2.5e-13 * sum of the terms + n * eps, eps the measured absolute error of a term."""
    return 2.5e-13 * sum_terms + n * S.EVAL_LL_TERM_EPS


def test_log_loss_per_entity_and_accumulated(device_solver):
    """Per entity on both paths, and a stage's accumulator fed in two batch orders: within the header's bound of math.fsum over
    log(1 + exp(s)) - [y > 0.5] s; identical bits in the two orders; a NaN score counted and left out; reset empties."""
    rng = np.random.default_rng(211)
    rp = np.concatenate([[0], np.cumsum(SIZES + [40_000])]).astype(np.int64)
    n = int(rp[-1])
    s = (rng.standard_normal(n) * 3.0).astype(np.float32)
    s[[7, 100, 3000, 9000]] = [0.0, -0.0, 30.5, -41.25]
    y = (rng.random(n) < 1.0 / (1.0 + np.exp(-s.astype(np.float64)))).astype(np.float32)
    where = [3, int(rp[5]) + 2, int(rp[16]) + 77]      # a NaN in a row-sized entity, in a sorted one and in a large one
    s[where] = np.nan
    ev = metrics.LogLossEvaluator(device_solver)
    worst = 0.0
    for limit in (64, 0):
        ev.set_small_max(limit)
        h = ev.to_host(ev.entities(rp, s, y))
        for e in range(rp.size - 1):
            want, mag, cnt = ref.log_loss_reference(s[rp[e]:rp[e + 1]], y[rp[e]:rp[e + 1]])
            nans = int(np.isnan(s[rp[e]:rp[e + 1]]).sum())
            assert h["n"][e] == cnt + nans and h["n_nan"][e] == nans
            err = abs(h["ll"][e] - want)
            if cnt:
                worst = max(worst, err / _ll_bound(mag, cnt))
            assert err <= _ll_bound(mag, cnt), (limit, e, err)
            assert math.isnan(h["logistic_loss"][e]) if (nans or cnt == 0) else h["logistic_loss"][e] == h["ll"][e] / cnt
    ev.set_small_max(64)
    print(f"log loss per entity: worst error / bound {worst:.3e}")
    want, mag, cnt = ref.log_loss_reference(s, y)
    cuts = [0, 1, 5000, 5001, 30_000, n]
    bits = []
    for order in (range(5), (3, 0, 4, 2, 1)):
        ev.reset()
        assert ev.count == 0
        for i in order:
            ev.add(s[cuts[i]:cuts[i + 1]], y[cuts[i]:cuts[i + 1]])
        r = ev.finish()
        assert (r["n"], r["n_nan"]) == (n, 3) and cnt == n - 3 and math.isnan(r["logistic_loss"])
        print(f"log loss accumulated: error / bound {abs(r['ll'] - want) / _ll_bound(mag, cnt):.3e}")
        assert abs(r["ll"] - want) <= _ll_bound(mag, cnt)
        bits.append(np.float64(r["ll"]).view(np.uint64))
    assert bits[0] == bits[1]
    clean = ~np.isnan(s)
    ev.reset()
    ev.add(s[clean], y[clean])
    r = ev.finish()
    assert r["n_nan"] == 0 and r["logistic_loss"] == r["ll"] / cnt and abs(r["ll"] - want) <= _ll_bound(mag, cnt)
    ev.reset()
    assert ev.finish()["n"] == 0 and ev.finish()["ll"] == 0.0


def test_small_workspace_and_bad_k_are_errors_not_faults(device_solver, rankers):
    """Return codes only: too small a workspace is GDMIX_RE_ENOMEM, nk or a k out of range GDMIX_RE_EINVAL, 2^31 samples GDMIX_RE_ERANGE —
    each refused on the host before anything is launched."""
    t = device_solver.torch
    rng = np.random.default_rng(31)
    s = rng.standard_normal(4096).astype(np.float32)
    y = (rng.random(4096) < 0.5).astype(np.float32)
    rp = np.arange(0, 4097, 128, dtype=np.int64)
    ev = rankers[tuple(KS[0])]
    with pytest.raises(GdmixReError, match=r"\(-3\).*workspace"):
        ev.entities(rp, s, y, workspace_bytes=1024)
    with pytest.raises(GdmixReError):
        metrics.RankingEvaluator(device_solver, [1, 2, 3, 4, 5])
    with pytest.raises(GdmixReError):
        metrics.RankingEvaluator(device_solver, [0])
    with pytest.raises(GdmixReError):
        metrics.RankingEvaluator(device_solver, [3, 3])
    lib, h, st = device_solver.lib, device_solver._h, device_solver._stream()
    sd, yd, rpd = (t.from_numpy(x).to(device_solver.device) for x in (s, y, rp))
    nbytes = int(lib.gdmix_re_eval_topk_workspace_bytes(32, 4096))
    ws = t.empty(nbytes, dtype=t.uint8, device=device_solver.device)
    counts = t.zeros((4, 32), dtype=t.int32, device=device_solver.device)
    out = S._EvalTopkOut(counts.data_ptr(), None, None, None)

    def call(ks, nk, N=4096, bytes_=nbytes):
        return lib.gdmix_re_eval_topk_entities(h, rpd.data_ptr(), 32, N, sd.data_ptr(), yd.data_ptr(), (C.c_int32 * len(ks))(*ks), nk, C.byref(out), None,
                                               ws.data_ptr(), bytes_, st)
    assert call([1, 2, 3, 4, 5], 5) == -1 and call([1], 0) == -1 and call([0, 1], 2) == -1 and call([2, 2], 2) == -1 and call([-5], 1) == -1
    assert call([1], 1, bytes_=nbytes - 1) == -3 and b"workspace" in lib.gdmix_re_last_error()
    assert call([1], 1, N=1 << 31) == -4
    assert call([128, 1], 2) == 0      # (only hits_sure is asked for: the other three pointers are NULL)
    t.cuda.synchronize()
    got = counts.cpu().numpy()
    want = ref.per_entity_counts(rp, s, y, [128, 1])
    assert np.array_equal(got[:2], want["hits_sure"])


# ---- through the product path --------------------------------------------------------------------------------------------------------
LIST = "LOGISTIC_LOSS,AUC:user_id,PRECISION@1:user_id,PRECISION@5:user_id"
OUTPUTS = ("models", "trainingScores", "validationScores", "metrics")


@pytest.fixture(scope="module")
def stages(tmp_path_factory):
    """The 100 k-rating data set of tests/test_gpu_metrics.py: the global stage once (with --evaluators=LOGISTIC_LOSS), the per-user partition
    job once, then the per-user stage four times from the same inputs — with the list (its default grouping of partitions; one and four
    partitions per device batch) and without the flag. Each run's outputs are moved aside, so every run is a cold start."""
    from gdmix_amd import chain, model
    data = chain.make_dataset()
    root = str(tmp_path_factory.mktemp("ranking"))
    chain.write_global_inputs(root, data)
    chain.run_stage(chain.stage_argv(root, "global", evaluators={"global": "LOGISTIC_LOSS"}))
    chain.partition_stage(root, data, "per_user", os.path.join(root, "global", "trainingScores"), os.path.join(root, "global", "validationScores"), 4,
                          upper_bound=200)
    runs = {}
    saved = model.GROUP_MAX      # (what GDMIX_PARTITIONS_PER_BATCH sets when the module is imported)
    try:
        for tag, group, kw in (("list", saved, dict(evaluators={"per_user": LIST})), ("one", 1, dict(evaluators={"per_user": LIST})),
                               ("four", 4, dict(evaluators={"per_user": LIST})), ("plain", saved, dict(device_metrics=True))):
            model.GROUP_MAX = group
            chain.run_stage(chain.stage_argv(root, "per_user", **kw))
            runs[tag] = os.path.join(root, "runs", tag)
            os.makedirs(runs[tag])
            for d in OUTPUTS:
                shutil.move(os.path.join(root, "per_user", d), os.path.join(runs[tag], d))
    finally:
        model.GROUP_MAX = saved
    return data, root, runs


def _summary(run):
    with open(os.path.join(run, "metrics", "evalSummary.json")) as f:
        return json.load(f)


def _records_and_samples(run, data):
    """-> {which: [(record, scores, labels)]}: every per-entity record of a run next to its samples in the score file the record was
    written for. A score file holds its batch's samples in the batch's order and the record file that batch's entities in theirs, so
    record i covers the next record["n"] rows — all of its entity, which is checked. (Passive data may hold an entity in several
    groups: several records of one entityId in one file.)"""
    from gdmix_amd.io import avro
    ent_by_uid = dict(zip(data["uid"].tolist(), data["user"].tolist()))
    out = {"training": [], "validation": []}
    for which, d in (("training", "trainingScores"), ("validation", "validationScores")):
        for r, _, fs in sorted(os.walk(os.path.join(run, d))):
            for fn in sorted(f for f in fs if f.endswith(".avro")):
                rows = list(avro.read_file(os.path.join(r, fn)))
                name = f"part-{which}-{os.path.basename(r)}-{fn[len('part-'):]}"
                recs = list(avro.read_file(os.path.join(run, "metrics", "perEntity", name)))
                assert sum(x["n"] for x in recs) == len(rows)
                at = 0
                for x in recs:
                    mine = rows[at:at + x["n"]]
                    at += x["n"]
                    assert all(ent_by_uid[m["uid"]] == int(x["entityId"]) for m in mine)
                    out[which].append((x, np.array([m["predictionScore"] for m in mine], np.float32), np.array([m["response"] for m in mine], np.float32)))
    return out


def test_stage_writes_the_requested_evaluators(stages):
    """--evaluators=LOGISTIC_LOSS,AUC:user_id,PRECISION@1:user_id,PRECISION@5:user_id on the per-user stage: every precision_at_K field and
    the summary's aggregates equal the reference computed from the stage's own score files joined to its entities; ll is within its bound."""
    from gdmix_amd import chain
    data, root, runs = stages
    summary = _summary(runs["list"])
    joined = _records_and_samples(runs["list"], data)
    twice = 0
    for which in ("training", "validation"):
        blk = summary[which]
        aucs, p1, p5, seen = [], [], [], set()
        for rec, s, y in joined[which]:
            assert rec["n"] == s.size >= 1 and rec["n_pos"] == int((y > 0.5).sum())
            twice += which == "training" and rec["entityId"] in seen
            seen.add(rec["entityId"])
            for k, acc in ((1, p1), (5, p5)):
                want = float(ref.precision(s, y, k))
                assert rec[f"precision_at_{k}"] == want, (which, rec, k)
                acc.append(want)
            a = ref.auc_exact(s, y)
            assert rec["auc"] == (None if a is None else float(a))
            if a is not None:
                aucs.append(float(a))
        assert blk["auc:user_id"] == ref.mean_of_records(aucs) and blk["auc:user_id_records"] == len(aucs) > 100
        assert blk["precision@1:user_id"] == ref.mean_of_records(p1) and blk["precision@1:user_id_records"] == len(p1) == len(joined[which])
        assert blk["precision@5:user_id"] == ref.mean_of_records(p5) and blk["precision@5:user_id_records"] == len(p5)
        _, sc, _, lab = chain.read_scores(os.path.join(runs["list"], "trainingScores" if which == "training" else "validationScores"))
        want, mag, cnt = ref.log_loss_reference(sc, lab)
        print(f"per_user {which}: ll {blk['ll']!r}, reference {want!r}, error / bound {abs(blk['ll'] - want) / _ll_bound(mag, cnt):.3e}")
        assert abs(blk["ll"] - want) <= _ll_bound(mag, cnt) and blk["logistic_loss"] == blk["ll"] / cnt and blk["n"] == cnt
    assert twice > 0      # an entity above the active-data bound has two training records, and both are averaged
    for key in ("logistic_loss", "ll", "auc:user_id", "auc:user_id_records", "precision@1:user_id", "precision@5:user_id_records"):
        assert summary[key] == summary["validation"][key]


def test_aggregates_do_not_depend_on_the_grouping_of_partitions(stages):
    """One partition per device batch and four (GDMIX_PARTITIONS_PER_BATCH = 1 and 4): the same aggregates. (The log loss is a sum in trees
    whose batches differ: its value agrees within the bound, not to the bit.)"""
    _, _, runs = stages
    one, four = _summary(runs["one"]), _summary(runs["four"])
    for which in ("training", "validation"):
        for key in one[which]:
            if key.startswith("auc:") or key.startswith("precision@"):
                assert one[which][key] == four[which][key], (which, key)
        assert one[which]["logistic_loss"] is not None
    assert any(key.startswith("precision@") for key in one["validation"])


def test_without_the_flag_the_stage_writes_what_it_wrote(stages):
    """The run without --evaluators: no new key in the summary, the parent's per-entity schema; every file outside metrics/ holds what the
    run with the flag wrote, and the summary's own keys hold the same values."""
    from gdmix_amd.io import avro
    from test_gpu_metrics import _files
    _, _, runs = stages
    plain, listed = _summary(runs["plain"]), _summary(runs["list"])
    assert set(plain) == {"auc", "n", "n_pos", "n_neg", "n_nan", "two_u", "sse", "data", "training", "validation"}
    # the file itself, byte for byte: the summary of the run with the flag, cut down to the keys a stage wrote before the flag existed
    cut = {k: ({kk: vv for kk, vv in v.items() if kk in plain[k]} if isinstance(v, dict) else v) for k, v in listed.items() if k in plain}
    with open(os.path.join(runs["plain"], "metrics", "evalSummary.json"), "rb") as f:
        assert f.read() == json.dumps(cut).encode()
    for which in ("training", "validation"):
        assert list(plain[which]) == ["auc", "n", "n_pos", "n_neg", "n_nan", "two_u", "sse"]
        assert {k: listed[which][k] for k in plain[which]} == plain[which]
    d = os.path.join(runs["plain"], "metrics", "perEntity")
    for fn in os.listdir(d):
        assert avro.read_schema(os.path.join(d, fn)) == metrics.PER_ENTITY_SCHEMA
    a, b = _files(runs["plain"]), _files(runs["list"])
    assert {k: v for k, v in a.items() if not k.startswith("metrics")} == {k: v for k, v in b.items() if not k.startswith("metrics")}
    assert set(a) == set(b)
    # the records of the run with the flag are the plain run's with the new fields behind them
    for fn in os.listdir(d):
        with_flag = list(avro.read_file(os.path.join(runs["list"], "metrics", "perEntity", fn)))
        assert [{k: v for k, v in r.items() if not k.startswith("precision_at_")} for r in with_flag] == list(avro.read_file(os.path.join(d, fn)))


def test_fixed_effect_stage_reports_the_log_loss_of_its_score_files(stages):
    from gdmix_amd import chain
    _, root, _ = stages
    with open(os.path.join(root, "global", "metrics", "evalSummary.json")) as f:
        summary = json.load(f)
    for which, d in (("training", "trainingScores"), ("validation", "validationScores")):
        _, sc, _, lab = chain.read_scores(os.path.join(root, "global", d))
        want, mag, cnt = ref.log_loss_reference(sc, lab)
        blk = summary[which]
        print(f"global {which}: ll {blk['ll']!r}, reference {want!r}, error / bound {abs(blk['ll'] - want) / _ll_bound(mag, cnt):.3e}")
        assert abs(blk["ll"] - want) <= _ll_bound(mag, cnt) and blk["logistic_loss"] == blk["ll"] / cnt and blk["n"] == cnt
        assert not any(k.startswith("auc:") or k.startswith("precision@") for k in blk)
    assert summary["logistic_loss"] == summary["validation"]["logistic_loss"]
    assert not os.path.exists(os.path.join(root, "global", "metrics", "perEntity"))
