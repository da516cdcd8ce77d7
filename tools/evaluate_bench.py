"""Time of the device evaluator (gdmix_amd/metrics.py, csrc/re_evaluate.hip) on the C2 scored batch (1 M entities, 16 M samples), next to
gdmix_re_score on the same batch and next to the numpy reference on the host.

    PYTHONPATH=. python tools/evaluate_bench.py [entities] [reps] > profiles/evaluate_bench.txt

Every figure is the median (and the range) of `reps` calls after three warm-up calls, a host clock around a call that ends in a device
synchronise: (a) gdmix_re_eval_entities by default routing and with every entity forced through the sort path, (b) accumulate + finish of
the same samples (as one batch, and as sixteen). Bytes are the algorithm's: 8 B per sample read, 40 B per entity written.

    PYTHONPATH=. python tools/evaluate_bench.py ranking [reps] > profiles/eval_ranking.txt

times what the ranking evaluation adds (include/gdmix_re.h, "ranking evaluation"): on a C2-shaped batch (1 M entities x 16 samples) and on a
MovieLens-20M per-movie-shaped batch, gdmix_re_eval_entities alone (the baseline) next to gdmix_re_eval_topk_entities with auc_out and four
values of k, the same way: one process, one session, median and range.
"""
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))      # metrics_reference

from gdmix_amd import metrics, synthetic  # noqa: E402
from gdmix_amd.solver import REDeviceSolver  # noqa: E402

RANKING = sys.argv[1:2] == ["ranking"]
E = int(sys.argv[1]) if len(sys.argv) > 1 and not RANKING else 1_000_000
REPS = int(sys.argv[2]) if len(sys.argv) > 2 else 12


def timed(fn, reps=REPS, warm=3):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        t = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t) * 1e3)
    return statistics.median(ms), min(ms), max(ms)


def line(what, t, nbytes=None):
    med, lo, hi = t
    extra = f", {nbytes / med / 1e6:.0f} GB/s of algorithmic bytes" if nbytes else ""
    print(f"{what:<58s} {med:9.3f} ms  (min {lo:.3f}, max {hi:.3f}, {REPS} calls){extra}", flush=True)


def ranking_bench():
    """Both calls on both shapes; the scores are standard normal, rounded to 1/64 so that ties occur, the labels drawn from their sigmoid."""
    s = REDeviceSolver(0)
    plain, ks = metrics.DeviceEvaluator(s), (1, 5, 10, 100)
    ranker = metrics.RankingEvaluator(s, ks)
    shapes = (("C2-shaped: 1 M entities x 16 samples", np.arange(0, 16 * 1_000_000 + 1, 16, dtype=np.int64)),
              ("MovieLens-20M per movie", np.asarray(synthetic.make_movielens_20m(kind="per_movie", seed=200).ent_row_ptr, np.int64)))
    gen = torch.Generator(device=s.device).manual_seed(5)
    for what, rp in shapes:
        n = np.diff(rp)
        N = int(rp[-1])
        score = (torch.randn(N, device=s.device, generator=gen) * 64.0).round() / 64.0
        label = (torch.rand(N, device=s.device, generator=gen) < torch.sigmoid(score)).to(torch.float32)
        rp_dev = torch.from_numpy(rp).to(s.device)
        print(f"{what}: {n.size} entities, {N} samples (largest entity {int(n.max())}, {int((n > 64).sum())} entities / {int(n[n > 64].sum())} samples on the sort path)")
        base = timed(lambda: plain.entities(rp_dev, score, label))
        both = timed(lambda: ranker.entities(rp_dev, score, label))
        only = timed(lambda: ranker.entities(rp_dev, score, label, with_auc=False))
        line("  gdmix_re_eval_entities (baseline)", base)
        line(f"  gdmix_re_eval_topk_entities, auc_out and k = {list(ks)}", both)
        line("  gdmix_re_eval_topk_entities without auc_out", only)
        print(f"  combined / baseline = {both[0] / base[0]:.3f} (the baseline run twice: 2.000)", flush=True)
        a, r = plain.entities(rp_dev, score, label), ranker.entities(rp_dev, score, label)
        assert all(torch.equal(a[k].view(torch.uint8), r[k].view(torch.uint8)) for k in a), "auc_out differs from gdmix_re_eval_entities"
        h = ranker.to_host(r)
        some = h["n"] >= 1
        print("  auc_out: the baseline's bits; mean precision@k over the entities with a sample: " +
              ", ".join(f"@{k} {float(np.mean(h[metrics.precision_key(k)][some])):.4f}" for k in ks))
    s.close()


if RANKING:
    ranking_bench()
    sys.exit(0)

b = synthetic.make_batch(E, 16, 4, 1024, seed=synthetic.C2_SEED, with_uid=False)
s = REDeviceSolver(0)
pk = s.pack(s.upload(b))
theta = 0.3 * torch.randn(int(pk.P), dtype=torch.float64, device=s.device, generator=torch.Generator(device=s.device).manual_seed(1))
logit, _ = s.score(pk, theta)
label = pk._raw_dev["y"]
n = np.diff(b.ent_row_ptr)
print(f"C2 scored batch: {b.E} entities, {b.N} samples (largest entity {int(n.max())}, {int((n > 16).sum())} above 16, {int((n > 32).sum())} above 32 samples)")
ev = metrics.DeviceEvaluator(s)
io_bytes = 8.0 * b.N + 8.0 * (b.E + 1) + 40.0 * b.E

line("gdmix_re_score", timed(lambda: s.score(pk, theta)))
ev.set_small_max(64)
line("gdmix_re_eval_entities, default routing", timed(lambda: ev.entities(pk, logit)), io_bytes)
default = metrics.entities_to_host(ev.entities(pk, logit))
ev.set_small_max(0)
line("gdmix_re_eval_entities, every entity by the sort path", timed(lambda: ev.entities(pk, logit)))
forced = metrics.entities_to_host(ev.entities(pk, logit))
ev.set_small_max(64)
for k in ("two_u", "n_pos", "n_neg", "n_nan"):
    assert np.array_equal(default[k], forced[k]), k
print("both routings: identical integers")
ev.reserve(b.N)


def accumulate(parts):
    ev.reset()
    step = (b.N + parts - 1) // parts
    for a in range(0, b.N, step):
        ev.add(logit[a:a + step], label[a:a + step])
    return ev.finish()


line("accumulate (one batch) + finish", timed(lambda: accumulate(1)))
line("accumulate (sixteen batches) + finish", timed(lambda: accumulate(16)))
ev.reset()
line("  of which: accumulate (one batch)", timed(lambda: (ev.reset(), ev.add(logit, label))))
r = accumulate(16)
print(f"stage metric: AUC {r['auc']:.6f}, MSE {r['mse']:.6f}, n_pos {r['n_pos']}, n_neg {r['n_neg']}")

# the numpy reference on the host (tests/metrics_reference.py): the global integers, and the per-entity loop on a slice
from metrics_reference import per_entity_reference, two_u_reference  # noqa: E402
sc, lab = logit.cpu().numpy(), label.cpu().numpy()
t = time.perf_counter()
ref = two_u_reference(sc, lab)
t_global = time.perf_counter() - t
assert ref == (r["two_u"], r["n_pos"], r["n_neg"], r["n_nan"])
print(f"numpy reference, global (np.unique + bincount + cumsum){'':<4s} {t_global * 1e3:9.0f} ms  (one call; same integers as the device)")
cut = min(b.E, 20_000)
t = time.perf_counter()
pe = per_entity_reference(b.ent_row_ptr[:cut + 1], sc, lab)
t_slice = time.perf_counter() - t
assert [int(x) for x in pe["two_u"]] == [int(x) for x in default["two_u"][:cut]]
print(f"numpy reference, per entity, {cut} entities{'':<19s} {t_slice * 1e3:9.0f} ms  (one call; x {b.E / cut:.0f} for the batch: {t_slice * b.E / cut:.0f} s)")
