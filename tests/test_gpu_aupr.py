"""AUPR on the device (include/gdmix_re.h, "AUPR"; csrc/re_evaluate.hip) against the exact rationals of tests/aupr_reference.py: per entity
on the register path and on the sort path, the accumulator under three batchings, and a stage that writes the two --evaluators items."""
import functools
import json
import math
import os
import shutil

import numpy as np
import pytest

from gdmix_amd import chain, metrics
from gdmix_amd.io import avro

import aupr_reference as ref

pytestmark = pytest.mark.gpu

BOUND = 3e-13      # the header's: |pr_sum - exact| <= 3e-13 * exact (fewer than 2 211 roundings in a chain of additions, four in a term)
# the lane-width edges, an empty entity, entities across the 4 096-key tile; four of 3 000 with boundaries inside tiles and a thread's 16 keys
SIZES = [16, 17, 32, 33, 64, 65, 1, 0, 15, 31, 63, 2, 66, 128, 2049, 5000] + [3000] * 4


@functools.lru_cache(maxsize=None)
def _case(name):
    """-> (ent_row_ptr, score, label, the reference per entity, the reference over all samples); built once per name and never changed."""
    rng = np.random.default_rng({"continuous": 301, "halves": 302, "special": 303}[name])
    rp = np.concatenate([[0], np.cumsum(SIZES)]).astype(np.int64)
    s = rng.standard_normal(int(rp[-1]))
    if name != "continuous":
        s = np.round(s * 2.0) / 2.0      # frequent ties: tie groups straddle thread and tile boundaries of the sorted array
    s = s.astype(np.float32)
    y = (rng.random(s.size) < 1.0 / (1.0 + np.exp(-s.astype(np.float64)))).astype(np.float32)
    if name == "special":
        ent = lambda e: slice(int(rp[e]), int(rp[e + 1]))
        for v in (np.nan, -0.0, 0.0, np.inf, -np.inf, np.nan, -0.0, np.inf, 0.0, -np.inf):
            s[rng.integers(0, s.size, 12)] = v
        s[ent(0)], s[ent(13)] = 0.25, -1.5                  # 16, and 128 on the sort path: all scores equal
        y[ent(2)], y[ent(14)] = 1.0, 1.0                    # 32, and 2 049 on the sort path: all positive
        y[ent(3)], y[ent(16)] = 0.0, 0.0                    # 33, and 3 000 on the sort path: all negative
        s[rp[5]:rp[5] + 3] = [np.inf, np.inf, np.nan]       # 65: ties at +inf next to a NaN on the sort path
        s[rp[1]:rp[1] + 4] = [0.0, -0.0, 0.0, -0.0]         # 17: the two zeros are one score
    return rp, s, y, [ref.pr_sum_exact(s[rp[e]:rp[e + 1]], y[rp[e]:rp[e + 1]]) for e in range(rp.size - 1)], ref.pr_sum_exact(s, y)


def _within(got, exact, what):
    print(f"{what}: pr_sum {got!r}, exact {float(exact)!r}, error / bound {abs(got - exact) / (BOUND * exact) if exact else 0.0:.3e}")
    assert abs(got - exact) <= BOUND * exact, what


@pytest.mark.parametrize("small_max", [64, 0])
@pytest.mark.parametrize("name", ["continuous", "halves", "special"])
def test_per_entity_counts_are_exact_and_sums_within_the_bound(device_solver, name, small_max):
    rp, s, y, want, _ = _case(name)
    aupr = metrics.AuprEvaluator(device_solver)
    aupr.set_small_max(small_max)
    try:
        res = aupr.entities(rp, s, y)
    finally:
        aupr.set_small_max(64)
    got = {k: v.cpu().numpy() for k, v in res.items()}
    assert all(got[key].tolist() == [w[col] for w in want] for key, col in (("n_pos", 1), ("n_neg", 2), ("n_nan", 3)))
    for e, (exact, n_pos, _, _) in enumerate(want):
        _within(float(got["pr_sum"][e]), exact, (name, small_max, e))
        assert math.isnan(got["aupr"][e]) if n_pos == 0 else got["aupr"][e] == float(got["pr_sum"][e]) / n_pos
    if name == "special":
        assert np.isnan(s).any() and np.isinf(s).any() and got["aupr"][14] == 1.0 and want[14][2] == 0      # (no negative: AUPR is 1)
        host = aupr.to_host(res)
        assert all(math.isnan(host["aupr"][e]) == (w[3] > 0 or w[1] == 0) for e, w in enumerate(want)) and host["n"].tolist() == SIZES


@pytest.mark.parametrize("name", ["halves", "special"])
def test_accumulator_does_not_depend_on_the_batches_and_leaves_the_keys(device_solver, name):      # one batch, three, the three reversed
    aupr = metrics.AuprEvaluator(device_solver)
    _, s, y, _, (exact, n_pos, n_neg, n_nan) = _case(name)
    cuts, bits = [0, 4097, 9000, s.size], set()
    for order in ([(0, s.size)], list(zip(cuts, cuts[1:])), list(zip(cuts, cuts[1:]))[::-1]):
        ev = metrics.DeviceEvaluator(device_solver)
        for a, b in order:
            ev.add(s[a:b], y[a:b])
        before = ev.finish()
        r = aupr.finish(ev)
        assert repr(ev.finish()) == repr(before)      # (by their text: a NaN metric compares unequal to itself)
        assert (r["n"], r["n_pos"], r["n_neg"], r["n_nan"]) == (s.size, n_pos, n_neg, n_nan) == (before["n"], before["n_pos"], before["n_neg"], before["n_nan"])
        _within(r["pr_sum"], exact, (name, len(order)))
        assert math.isnan(r["aupr"]) if n_nan else r["aupr"] == r["pr_sum"] / n_pos
        bits.add(np.float64(r["pr_sum"]).view(np.uint64).item())
    assert len(bits) == 1


def test_stage_writes_aupr_and_without_the_items_what_it_wrote(tmp_path):
    """A small job. The values equal the reference on the written scores; without the items every file is the other run's less the new keys."""
    from test_gpu_metrics import _files
    from test_gpu_ranking import _records_and_samples, _summary
    data, root, runs = chain.make_dataset(users=60, movies=100, ratings=4000), str(tmp_path), {}
    chain.write_global_inputs(root, data)
    chain.run_stage(chain.stage_argv(root, "global", evaluators={"global": "AUPR"}))
    chain.partition_stage(root, data, "per_user", os.path.join(root, "global", "trainingScores"), os.path.join(root, "global", "validationScores"), 2,
                          upper_bound=60)
    for tag, listed in (("new", "LOGISTIC_LOSS,AUC:user_id,AUPR,AUPR:user_id"), ("old", "LOGISTIC_LOSS,AUC:user_id")):
        chain.run_stage(chain.stage_argv(root, "per_user", evaluators={"per_user": listed}))
        runs[tag] = os.path.join(root, "runs", tag, "metrics")
        os.makedirs(os.path.dirname(runs[tag]))
        for d in ("models", "trainingScores", "validationScores", "metrics"):
            shutil.move(os.path.join(root, "per_user", d), os.path.join(root, "runs", tag, d))
    new, old, glob = (_summary(os.path.dirname(d)) for d in (runs["new"], runs["old"], os.path.join(root, "global", "metrics")))
    joined = _records_and_samples(os.path.dirname(runs["new"]), data)
    for which, d in (("training", "trainingScores"), ("validation", "validationScores")):
        for blk, scores in ((new[which], os.path.join(root, "runs", "new", d)), (glob[which], os.path.join(root, "global", d))):
            _, sc, _, lab = chain.read_scores(scores)
            exact, n_pos, _, _ = ref.pr_sum_exact(sc, lab)
            _within(blk["pr_sum"], exact, (scores, which))
            assert blk["aupr"] == blk["pr_sum"] / n_pos
        for rec, s, y in joined[which]:
            exact, n_pos, _, _ = ref.pr_sum_exact(s, y)
            want = float(exact / n_pos) if n_pos else None      # (the record holds the quotient: one more rounding, and one of this conversion)
            assert rec["aupr"] is None if want is None else abs(rec["aupr"] - want) <= (BOUND + 2.0 ** -52) * want, (which, rec)
        values = [rec["aupr"] for rec, _, _ in joined[which] if rec["aupr"] is not None]
        assert new[which]["aupr:user_id"] == math.fsum(values) / len(values) and new[which]["aupr:user_id_records"] == len(values) > 20
        assert not any(k.startswith("aupr:") for k in glob[which]) and not any("aupr" in k or k == "pr_sum" for k in old[which])
    cut = {k: ({kk: vv for kk, vv in v.items() if kk in old[k]} if isinstance(v, dict) else v) for k, v in new.items() if k in old}
    with open(os.path.join(runs["old"], "evalSummary.json"), "rb") as f:
        assert f.read() == json.dumps(cut).encode()
    for fn in os.listdir(os.path.join(runs["old"], "perEntity")):
        assert avro.read_schema(os.path.join(runs["old"], "perEntity", fn)) == metrics.ranking_entity_schema(())
        assert [{k: v for k, v in r.items() if k != "aupr"} for r in avro.read_file(os.path.join(runs["new"], "perEntity", fn))] == list(avro.read_file(os.path.join(runs["old"], "perEntity", fn)))
    a, b = _files(os.path.dirname(runs["old"])), _files(os.path.dirname(runs["new"]))
    assert set(a) == set(b) and {k: v for k, v in a.items() if not k.startswith("metrics")} == {k: v for k, v in b.items() if not k.startswith("metrics")}
