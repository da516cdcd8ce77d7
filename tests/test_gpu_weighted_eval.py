"""The weighted evaluation on the device (include/gdmix_re.h, "weighted evaluation"; csrc/re_evaluate_weighted.hip, csrc/re_evaluate_poisson.hip)
against the exact rationals of tests/weighted_eval_reference.py: per entity on the register path and on the sort path, the accumulators under
three batchings, and a stage with a weight column that writes the three --evaluators items."""
import functools
import json
import math
import os
import shutil

import numpy as np
import pytest

from gdmix_amd import chain, metrics, solver
from gdmix_amd.io import avro

import weighted_eval_reference as ref

pytestmark = pytest.mark.gpu

BOUND = solver.EVAL_W_BOUND       # the header's: |twoU_w - exact| <= 7.5e-13 * exact (6 413 roundings), W_pos, W_neg and W inside it
LL_BOUND, LL_EPS = 3e-13, solver.EVAL_LL_TERM_EPS      # |LL_w - exact| <= 3e-13 * LL_w + eps * W
T = solver.EVAL_W_SCAN_TILE       # sorted keys per workgroup of the scan
SIZES = [0, 1, 2, 3, 16, 17, 63, 64, 65, 130, T - 1, T, T + 1, 2 * T + 1]
ALL_POS, SPECIAL, NAN_W, ZERO_POS, NEG_W = 4, 5, 6, 7, 9      # entities (16, 17, 63, 64, 130 samples) with something to show
RP = np.concatenate([[0], np.cumsum(SIZES)]).astype(np.int64)
ENT = lambda e: slice(int(RP[e]), int(RP[e + 1]))


@functools.lru_cache(maxsize=None)
def _case(kind):
    """-> (score, label, weight or None); built once per kind of weight and never changed. Scores from eight values: ties are the rule."""
    rng = np.random.default_rng(411)
    s = rng.choice(np.array([-2.5, -1.0, -0.25, 0.0, 0.5, 0.75, 1.5, 3.0], np.float32), int(RP[-1]))
    y = (rng.random(s.size) < 1.0 / (1.0 + np.exp(-s.astype(np.float64)))).astype(np.float32)
    s[ENT(SPECIAL)][:7] = [0.0, -0.0, np.inf, -np.inf, np.nan, np.inf, -0.0]
    y[ENT(SPECIAL)][:7] = [1.0, 0.0, 1.0, 0.0, 1.0, 0.0, 1.0]      # (the second +inf under a negative label: its log loss is +inf)
    y[ENT(ALL_POS)] = 1.0
    if kind in ("ones", "absent"):
        return s, y, (np.ones(s.size, np.float32) if kind == "ones" else None)
    w = rng.integers(0, 4, s.size).astype(np.float32) if kind == "integer" else np.exp(rng.uniform(np.log(0.01), np.log(100.0), s.size)).astype(np.float32)
    w[ENT(ZERO_POS)][y[ENT(ZERO_POS)] > 0.5] = 0.0
    w[ENT(ZERO_POS)][:1] = -0.0
    w[RP[NAN_W] + 5], w[RP[NEG_W] + 77], w[RP[SPECIAL] + 5] = np.nan, -1.0, 2.0
    return s, y, w


@functools.lru_cache(maxsize=None)
def _exact(kind):
    s, y, w = _case(kind)
    per = lambda f: [f(s[ENT(e)], y[ENT(e)], None if w is None else w[ENT(e)]) for e in range(len(SIZES))]
    return per(ref.rank_sums_exact), per(ref.logloss_sums_exact), ref.rank_sums_exact(s, y, w), ref.logloss_sums_exact(s, y, w)


def _entities(device_solver, cls, small_max, *args, **kw):
    ev = cls(device_solver)
    ev.set_small_max(small_max)
    try:
        return {k: v.cpu().numpy() for k, v in ev.entities(*args, **kw).items()}
    finally:
        ev.set_small_max(64)


def _within(got, exact, bound, what, slack=0.0):
    print(f"{what}: {got!r}, exact {float(exact)!r}, error / bound {abs(got - exact) / (bound * exact + slack) if exact else 0.0:.3e}")
    assert abs(got - exact) <= bound * exact + slack, what


@pytest.mark.parametrize("small_max", [64, 0])
def test_integer_weights_equal_the_unweighted_call_on_the_replicated_batch(device_solver, small_max):
    s, y, w = _case("integer")
    times = np.where(w >= 0, w, 0).astype(np.int64)      # a bad weight: the sample is left out
    rp_rep = np.concatenate([[0], np.cumsum([times[ENT(e)].sum() for e in range(len(SIZES))])]).astype(np.int64)
    got = _entities(device_solver, metrics.WeightedEvaluator, small_max, RP, s, y, w)
    want = _entities(device_solver, metrics.DeviceEvaluator, small_max, rp_rep, np.repeat(s, times), np.repeat(y, times))
    for a, b in (("two_u_w", "two_u"), ("w_pos", "n_pos"), ("w_neg", "n_neg")):
        assert np.array_equal(got[a], want[b].astype(np.float64)), a
    assert np.array_equal(got["auc"].view(np.uint64), want["auc"].view(np.uint64))
    assert got["n_bad_weight"].tolist() == [int(e in (NAN_W, NEG_W)) for e in range(len(SIZES))] and got["n_nan"].sum() == got["n_nan"][SPECIAL] == 1
    assert math.isnan(got["auc"][ALL_POS]) and math.isnan(got["auc"][ZERO_POS]) and got["w_pos"][ZERO_POS] == 0.0 < got["w_neg"][ZERO_POS]


@pytest.mark.parametrize("small_max", [64, 0])
@pytest.mark.parametrize("kind", ["ones", "absent"])
def test_unit_and_absent_weights_give_the_unweighted_result(device_solver, kind, small_max):
    s, y, w = _case(kind)
    got = _entities(device_solver, metrics.WeightedEvaluator, small_max, RP, s, y, w)
    want = _entities(device_solver, metrics.DeviceEvaluator, small_max, RP, s, y)
    assert all(np.array_equal(got[a], want[b].astype(np.float64)) for a, b in (("two_u_w", "two_u"), ("w_pos", "n_pos"), ("w_neg", "n_neg")))
    assert np.array_equal(got["auc"].view(np.uint64), want["auc"].view(np.uint64)) and np.array_equal(got["n_nan"], want["n_nan"]) and not got["n_bad_weight"].any()
    ll = _entities(device_solver, metrics.WeightedLogLossEvaluator, small_max, RP, s, y, w)
    plain = _entities(device_solver, metrics.LogLossEvaluator, small_max, RP, s, y)
    assert np.array_equal(ll["ll_w"], plain["pl"]) and np.array_equal(ll["w"], plain["n"].astype(np.float64))      # (a weight of one: the same terms, the same trees)


def test_real_weights_are_within_the_bound_on_both_paths(device_solver):
    s, y, w = _case("real")
    rank, ll, _, _ = _exact("real")
    paths = {m: (_entities(device_solver, metrics.WeightedEvaluator, m, RP, s, y, w), _entities(device_solver, metrics.WeightedLogLossEvaluator, m, RP, s, y, w)) for m in (64, 0)}
    for m, (got, gl) in paths.items():
        for e, ((two_u, w_pos, w_neg, n_nan, n_bad), (ll_w, w_all, _, _)) in enumerate(zip(rank, ll)):
            for key, exact in (("two_u_w", two_u), ("w_pos", w_pos), ("w_neg", w_neg)):
                _within(float(got[key][e]), exact, BOUND, (m, e, key))
            assert (got["n_nan"][e], got["n_bad_weight"][e], gl["n_nan"][e], gl["n_bad_weight"][e]) == (n_nan, n_bad, n_nan, n_bad)
            assert math.isnan(got["auc"][e]) if not (w_pos and w_neg) else got["auc"][e] == got["two_u_w"][e] / (2.0 * got["w_pos"][e] * got["w_neg"][e])
            _within(float(gl["w"][e]), w_all, BOUND, (m, e, "w"))
            if ll_w == math.inf:
                assert gl["ll_w"][e] == math.inf and e == SPECIAL
            else:
                _within(float(gl["ll_w"][e]), ll_w, LL_BOUND, (m, e, "ll_w"), slack=LL_EPS * float(w_all))
    for key in ("two_u_w", "w_pos", "w_neg"):      # the two paths: different trees over the same terms
        a, b = paths[64][0][key], paths[0][0][key]
        assert np.all(np.abs(a - b) <= 2 * BOUND * np.maximum(a, b)), key
    assert rank[NAN_W][4] == rank[NEG_W][4] == 1 and rank[SPECIAL][3] == 1 and rank[ZERO_POS][1] == 0 < rank[ZERO_POS][2]


@pytest.mark.parametrize("kind", ["real", "integer"])
def test_stage_sums_do_not_depend_on_the_batches(device_solver, kind):      # one batch, five uneven ones, the five reversed
    s, y, w = _case(kind)
    _, _, (two_u, w_pos, w_neg, n_nan, n_bad), (ll_w, w_all, _, _) = _exact(kind)
    cuts = [0, 15, T + 1, T + 2, 3 * T - 7, s.size]
    five = list(zip(cuts, cuts[1:]))
    fin = np.isfinite(s) | np.isnan(s)      # the log loss without the infinite scores: the TwoSum pair holds finite totals
    ll_exact, w_fin, _, _ = ref.logloss_sums_exact(s[fin], y[fin], w[fin])
    bits, ll_bits = set(), {}
    for name, order in (("one", [(0, s.size)]), ("five", five), ("reversed", five[::-1]), ("five again", five)):
        ev, ll = metrics.WeightedEvaluator(device_solver), metrics.WeightedLogLossEvaluator(device_solver)
        for a, b in order:
            ev.add(s[a:b], y[a:b], w[a:b])
            ll.add(s[a:b][fin[a:b]], y[a:b][fin[a:b]], w[a:b][fin[a:b]])
        r, rl = ev.finish(), ll.finish()
        assert (r["n"], r["n_nan"], r["n_bad_weight"], rl["n"], rl["n_nan"], rl["n_bad_weight"]) == (s.size, n_nan, n_bad, int(fin.sum()), n_nan, n_bad) and n_bad == 2
        for key, exact in (("two_u_w", two_u), ("w_pos", w_pos), ("w_neg", w_neg)):
            _within(r[key], exact, BOUND, (kind, name, key))
            assert kind != "integer" or r[key] == exact
        bits.add(tuple(np.float64(r[k]).view(np.uint64).item() for k in ("two_u_w", "w_pos", "w_neg")))
        assert math.isnan(r["weighted_auc"]) and metrics.weighted_auc_from_sums(r["two_u_w"], r["w_pos"], r["w_neg"]) == r["two_u_w"] / (2.0 * r["w_pos"] * r["w_neg"])
        _within(rl["w"], w_fin, BOUND, (kind, name, "w"))
        _within(rl["ll_w"], ll_exact, LL_BOUND, (kind, name, "ll_w"), slack=LL_EPS * float(w_fin))
        ll_bits[name] = tuple(np.float64(rl[k]).view(np.uint64).item() for k in ("ll_w", "w"))
    assert len(bits) == 1 and ll_bits["five"] == ll_bits["five again"] and ll_w == math.inf


def test_stage_with_a_weight_column_writes_the_three_items(tmp_path):
    """A small job (the AUPR stage test's size). The values equal the reference on the written scores joined to the weights; without the items
    every file is the other run's less the new keys."""
    from test_gpu_metrics import _files
    from test_gpu_ranking import _summary
    data, root, runs = chain.make_dataset(users=60, movies=100, ratings=4000), str(tmp_path), {}
    weights = np.exp(np.random.default_rng(412).uniform(np.log(0.05), np.log(20.0), data["uid"].size)).astype(np.float32)
    w_of, user_of = dict(zip(data["uid"].tolist(), weights.tolist())), dict(zip(data["uid"].tolist(), data["user"].tolist()))
    chain.write_global_inputs(root, data)
    chain.run_stage(chain.stage_argv(root, "global"))
    chain.partition_stage(root, data, "per_user", os.path.join(root, "global", "trainingScores"), os.path.join(root, "global", "validationScores"), 2,
                          upper_bound=60, weights=weights)
    for tag, listed in (("new", "LOGISTIC_LOSS,AUC:user_id,WEIGHTED_AUC,WEIGHTED_AUC:user_id,WEIGHTED_LOGISTIC_LOSS"), ("old", "LOGISTIC_LOSS,AUC:user_id")):
        chain.run_stage(chain.stage_argv(root, "per_user", evaluators={"per_user": listed}, weighted=True))
        runs[tag] = os.path.join(root, "runs", tag)
        os.makedirs(runs[tag])
        for d in ("models", "trainingScores", "validationScores", "metrics"):
            shutil.move(os.path.join(root, "per_user", d), os.path.join(runs[tag], d))
    new, old = _summary(runs["new"]), _summary(runs["old"])
    for which, d in (("training", "trainingScores"), ("validation", "validationScores")):
        uid, sc, _, lab = chain.read_scores(os.path.join(runs["new"], d))
        w = np.array([w_of[u] for u in uid.tolist()], np.float32)
        two_u, w_pos, w_neg, _, _ = ref.rank_sums_exact(sc, lab, w)
        ll_w, w_all, _, _ = ref.logloss_sums_exact(sc, lab, w)
        blk = new[which]
        for key, exact in (("two_u_w", two_u), ("w_pos", w_pos), ("w_neg", w_neg), ("w", w_all)):
            _within(blk[key], exact, BOUND, (which, key))
        _within(blk["ll_w"], ll_w, LL_BOUND, (which, "ll_w"), slack=LL_EPS * float(w_all))
        assert blk["weighted_auc"] == blk["two_u_w"] / (2.0 * blk["w_pos"] * blk["w_neg"]) and blk["weighted_logistic_loss"] == blk["ll_w"] / blk["w"]
        # per entity: a score file holds its batch's samples in the batch's order, the record file that batch's entities in theirs
        values = []
        for r, _, fs in sorted(os.walk(os.path.join(runs["new"], d))):
            for fn in sorted(f for f in fs if f.endswith(".avro")):
                rows, at = list(avro.read_file(os.path.join(r, fn))), 0
                for rec in avro.read_file(os.path.join(runs["new"], "metrics", "perEntity", f"part-{which}-{os.path.basename(r)}-{fn[len('part-'):]}")):
                    mine, at = rows[at:at + rec["n"]], at + rec["n"]
                    assert all(user_of[m["uid"]] == int(rec["entityId"]) for m in mine)
                    two_u, w_pos, w_neg, _, _ = ref.rank_sums_exact([m["predictionScore"] for m in mine], [m["response"] for m in mine], [w_of[m["uid"]] for m in mine])
                    want = float(two_u / (2 * w_pos * w_neg)) if w_pos and w_neg else None      # (the record holds the quotient of three sums inside the bound)
                    assert rec["weighted_auc"] is None if want is None else abs(rec["weighted_auc"] - want) <= (3 * BOUND + 2.0 ** -51) * want, (which, rec)
                    values += [] if want is None else [rec["weighted_auc"]]
        assert blk["weighted_auc:user_id"] == math.fsum(values) / len(values) and blk["weighted_auc:user_id_records"] == len(values) > 20
        assert not any(k.startswith("weighted") or k in ("two_u_w", "w_pos", "w_neg", "ll_w", "w") for k in old[which])
    cut = {k: ({kk: vv for kk, vv in v.items() if kk in old[k]} if isinstance(v, dict) else v) for k, v in new.items() if k in old}
    with open(os.path.join(runs["old"], "metrics", "evalSummary.json"), "rb") as f:
        assert f.read() == json.dumps(cut).encode()
    for fn in os.listdir(os.path.join(runs["old"], "metrics", "perEntity")):
        assert avro.read_schema(os.path.join(runs["old"], "metrics", "perEntity", fn)) == metrics.ranking_entity_schema(())
        assert [{k: v for k, v in r.items() if k != "weighted_auc"} for r in avro.read_file(os.path.join(runs["new"], "metrics", "perEntity", fn))] == \
            list(avro.read_file(os.path.join(runs["old"], "metrics", "perEntity", fn)))
    a, b = _files(runs["old"]), _files(runs["new"])
    assert set(a) == set(b) and {k: v for k, v in a.items() if not k.startswith("metrics")} == {k: v for k, v in b.items() if not k.startswith("metrics")}
