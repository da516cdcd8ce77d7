"""NDCG@K on the device (include/gdmix_re.h, "NDCG"; csrc/re_evaluate_ndcg.hip; gdmix_amd/metrics.py) against the 50-digit reference of
tests/ndcg_reference.py: the two discounted sums within the header's relative bound and the counts, on the register path and on the sort
path; the argument checks; and a linear-regression stage that writes ndcg@3 while it scores."""
import ctypes as C
import functools
import json
import os
import shutil

import numpy as np
import pytest

from gdmix_amd import chain, metrics, solver
from gdmix_amd.io import avro

import ndcg_reference as ref

pytestmark = pytest.mark.gpu

BOUND = solver.EVAL_NDCG_BOUND      # the header's: |dcg - exact| <= 7.5e-13 * exact, and the same for idcg
W = 256                             # the sort path's workgroup width
# the lane-width edges of the register path (n = 0, 1, 2 are n < K, n = K and n = K + 1 for K = 1), the workgroup's, a lane's second term
SIZES = [0, 1, 2, 15, 16, 17, 31, 32, 33, 63, 64, 65, W, W + 1, 2 * W + 1, 2049]
KS = (1, 3, 10, 2**31 - 1)
STRADDLE, ALL_EQUAL, ZEROS, NO_GAIN, NEG_LABEL, HALVES, NAN_SCORE, NAN_LABEL, INF_LABEL, NAN_BIG, ALL_EQUAL_BIG, BIG_LABEL, CONTINUOUS = 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15
RP = np.concatenate([[0], np.cumsum(SIZES)]).astype(np.int64)
ENT = lambda e: slice(int(RP[e]), int(RP[e + 1]))
assert ref.mpmath.mp.dps == 50 and BOUND <= 1e-12


@functools.lru_cache(maxsize=None)
def _case():
    """-> (score, label, [[(dcg, idcg, n, n_nan, n_bad_label) per entity] per K]); built once and never changed. Scores from eight values,
    so ties are the rule and tie groups straddle every K; labels are whole stars 0 .. 5 unless said otherwise."""
    rng = np.random.default_rng(511)
    s = rng.choice(np.array([-2.5, -1.0, -0.25, 0.0, 0.5, 0.75, 1.5, 3.0], np.float32), int(RP[-1]))
    y = rng.integers(0, 6, s.size).astype(np.float32)
    s[ENT(STRADDLE)][:6] = [5.0, 5.0, 4.0, 4.0, 4.0, 4.0]      # ranks 2 .. 5 are one group across K = 3
    s[ENT(ALL_EQUAL)], s[ENT(ALL_EQUAL_BIG)] = 0.25, -1.5
    s[ENT(ZEROS)][:4], y[ENT(ZEROS)][:4] = [0.0, -0.0, 0.0, -0.0], [5.0, 0.0, 1.0, 3.0]      # one score
    y[ENT(NO_GAIN)] = 0.0
    y[ENT(1)], y[ENT(2)] = 4.0, [1.0, 3.0]
    for e in (HALVES, INF_LABEL, CONTINUOUS):
        y[ENT(e)] = rng.integers(0, 11, SIZES[e]).astype(np.float32) / 2.0      # half stars
    s[ENT(CONTINUOUS)] = rng.standard_normal(SIZES[CONTINUOUS]).astype(np.float32)
    s[RP[NAN_SCORE] + 7], s[RP[NAN_BIG] + 100] = np.nan, np.nan
    y[RP[NEG_LABEL] + 3], y[RP[NAN_LABEL] + 63], y[RP[INF_LABEL] + 1], y[RP[BIG_LABEL] + 400] = -1.0, np.nan, np.inf, 65.0
    return s, y, [[ref.dcg_idcg(s[ENT(e)], y[ENT(e)], k) for e in range(len(SIZES))] for k in KS]


@functools.lru_cache(maxsize=None)
def _device(device_solver, small_max):
    s, y, _ = _case()
    ev = metrics.NdcgEvaluator(device_solver, KS)
    ev.set_small_max(small_max)
    try:
        return ev.to_host(ev.entities(RP, s, y))
    finally:
        ev.set_small_max(64)


@pytest.mark.parametrize("small_max", [64, 0])
def test_sums_are_within_the_bound_and_counts_equal_on_both_paths(device_solver, small_max):
    _, _, exact = _case()
    got, first = _device(device_solver, small_max), _device(device_solver, 64)
    worst = 0.0
    for j, k in enumerate(KS):
        for e, (dcg, idcg, n, n_nan, n_bad) in enumerate(exact[j]):
            assert (got["n"][e], got["n_nan"][e], got["n_bad_label"][e]) == (n, n_nan, n_bad), (k, e)
            for key, want in (("dcg", dcg), ("idcg", idcg)):
                err = abs(ref.mpmath.mpf(float(got[key][j, e])) - want)
                worst = max(worst, float(err / (BOUND * want)) if want else 0.0)
                assert err <= BOUND * want, (small_max, k, e, key, float(got[key][j, e]), float(want))
                assert abs(got[key][j, e] - first[key][j, e]) <= BOUND * first[key][j, e], (k, e, key)      # the two paths
            null = idcg == 0 or n_nan or n_bad
            v = got[metrics.ndcg_key(k)][e]
            assert np.isnan(v) if null else v == got["dcg"][j, e] / got["idcg"][j, e], (k, e)
    print(f"small_max {small_max}: worst error / bound {worst:.3e}")
    nulls = np.flatnonzero(np.isnan(got[metrics.ndcg_key(10)])).tolist()
    assert nulls == [0, NO_GAIN, NEG_LABEL, NAN_SCORE, NAN_LABEL, INF_LABEL, NAN_BIG, BIG_LABEL]
    assert got["n_bad_label"].tolist() == [int(e in (NEG_LABEL, NAN_LABEL, INF_LABEL, BIG_LABEL)) for e in range(len(SIZES))]
    assert got["idcg"][0, 1] == got["dcg"][0, 1] == 15.0      # one sample of four stars at K = 1: its gain, exactly (d(0) is 1)


def test_bad_ks_are_refused_before_anything_is_launched_and_null_outputs_accepted(device_solver):
    t, lib = device_solver.torch, device_solver.lib
    s, y, _ = _case()
    sd, yd, rpd = (t.from_numpy(x).to(device_solver.device) for x in (s, y, RP))
    E, N = len(SIZES), int(RP[-1])
    nbytes = int(lib.gdmix_re_eval_ndcg_workspace_bytes(E, N))
    ws = t.empty(nbytes, dtype=t.uint8, device=device_solver.device)
    out = solver._EvalNdcgOut()      # every pointer NULL

    def call(ks, nk, E=E, N=N):
        return lib.gdmix_re_eval_ndcg_entities(device_solver._h, rpd.data_ptr(), E, N, sd.data_ptr(), yd.data_ptr(), (C.c_int32 * len(ks))(*ks), nk, C.byref(out),
                                               ws.data_ptr(), nbytes, device_solver._stream())
    for empty in (dict(), dict(E=0, N=0)):
        assert call([1], 0, **empty) == -1 and call([1, 2, 3, 4, 5], 5, **empty) == -1 and call([3, 7, 3], 3, **empty) == -1 and call([2, 0], 2, **empty) == -1
        assert b"gdmix_re_eval_ndcg_entities" in lib.gdmix_re_last_error()
    assert call([1, 3], 2, E=0, N=0) == 0 and call(list(KS), 4) == 0
    t.cuda.synchronize()
    with pytest.raises(solver.GdmixReError, match=r"\(-3\).*workspace"):
        metrics.NdcgEvaluator(device_solver, (5,)).entities(RP, s, y, workspace_bytes=1024)
    for ks in ((), (1, 2, 3, 4, 5), (2, 2), (0,), (2**31,)):
        with pytest.raises(solver.GdmixReError):
            metrics.NdcgEvaluator(device_solver, ks)


def test_linear_stage_writes_ndcg_at_3_next_to_its_mse(tmp_path):
    """A small per-user stage on 1 .. 5-star ratings under --model_type=linear_regression --evaluators=NDCG@3:user_id: the record field, the
    mean and the record count agree with the reference on the stage's own score files; mse is still there; without the flag the stage
    writes what it wrote before."""
    from test_gpu_metrics import _files
    from test_gpu_ranking import _summary
    data, root, runs = chain.make_dataset(users=40, movies=100, ratings=3000), str(tmp_path), {}
    user_of = dict(zip(data["uid"].tolist(), data["user"].tolist()))
    chain.write_global_inputs(root, data, model_type=chain.LINEAR)
    chain.run_stage(chain.stage_argv(root, "global", chain.LINEAR))
    chain.run_stage(chain.global_training_scores_argv(root, chain.LINEAR))
    chain.partition_stage(root, data, "per_user", os.path.join(root, "global", "trainingScores"), os.path.join(root, "global", "validationScores"), 2,
                          model_type=chain.LINEAR)
    for tag, kw in (("new", dict(evaluators={"per_user": "ndcg@3:user_id"})), ("old", dict(device_metrics=True))):
        chain.run_stage(chain.stage_argv(root, "per_user", chain.LINEAR, **kw))
        runs[tag] = os.path.join(root, "runs", tag)
        os.makedirs(runs[tag])
        for d in ("models", "trainingScores", "validationScores", "metrics"):
            shutil.move(os.path.join(root, "per_user", d), os.path.join(runs[tag], d))
    new, old = _summary(runs["new"]), _summary(runs["old"])
    for which, d in (("training", "trainingScores"), ("validation", "validationScores")):
        values = []
        for r, _, fs in sorted(os.walk(os.path.join(runs["new"], d))):
            for fn in sorted(f for f in fs if f.endswith(".avro")):
                rows, at = list(avro.read_file(os.path.join(r, fn))), 0
                for rec in avro.read_file(os.path.join(runs["new"], "metrics", "perEntity", f"part-{which}-{os.path.basename(r)}-{fn[len('part-'):]}")):
                    mine, at = rows[at:at + rec["n"]], at + rec["n"]
                    assert all(user_of[m["uid"]] == int(rec["entityId"]) for m in mine)
                    want = ref.ndcg([m["predictionScore"] for m in mine], [m["response"] for m in mine], 3)
                    assert rec["ndcg_at_3"] is None if want is None else abs(rec["ndcg_at_3"] - want) <= (2 * BOUND + 2.0 ** -52) * want, (which, rec)
                    values += [] if want is None else [rec["ndcg_at_3"]]
        blk = new[which]
        assert blk["ndcg@3:user_id"] == ref.mean_of_records(values) and blk["ndcg@3:user_id_records"] == len(values) > 20
        assert blk["mse"] == old[which]["mse"] > 0.0 and not any(k.startswith("ndcg") for k in old[which])
    assert new["ndcg@3:user_id"] == new["validation"]["ndcg@3:user_id"]
    cut = {k: ({kk: vv for kk, vv in v.items() if kk in old[k]} if isinstance(v, dict) else v) for k, v in new.items() if k in old}
    with open(os.path.join(runs["old"], "metrics", "evalSummary.json"), "rb") as f:
        assert f.read() == json.dumps(cut).encode()
    for fn in os.listdir(os.path.join(runs["old"], "metrics", "perEntity")):
        assert avro.read_schema(os.path.join(runs["old"], "metrics", "perEntity", fn)) == metrics.PER_ENTITY_SCHEMA
        assert avro.read_schema(os.path.join(runs["new"], "metrics", "perEntity", fn)) == metrics.ranking_entity_schema((), ndcg_ks=(3,))
        assert [{k: v for k, v in r.items() if k != "ndcg_at_3"} for r in avro.read_file(os.path.join(runs["new"], "metrics", "perEntity", fn))] == \
            list(avro.read_file(os.path.join(runs["old"], "metrics", "perEntity", fn)))
    a, b = _files(runs["old"]), _files(runs["new"])
    assert set(a) == set(b) and {k: v for k, v in a.items() if not k.startswith("metrics")} == {k: v for k, v in b.items() if not k.startswith("metrics")}
