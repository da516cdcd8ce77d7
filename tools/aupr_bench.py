"""Time of AUPR on the device (include/gdmix_re.h, "AUPR"; csrc/re_evaluate.hip) next to the calls of the same library that pay the same sort.

    PYTHONPATH=. python tools/aupr_bench.py [reps] > profiles/aupr.txt

Per entity: gdmix_re_eval_aupr_entities next to gdmix_re_eval_topk_entities (without auc_out, four values of k) on a C2-shaped batch (1 M
entities x 16 samples: the register path alone) and on a MovieLens-20M per-movie-shaped batch (most samples on the sort path). Over a stage:
gdmix_re_eval_aupr_acc_finish next to gdmix_re_eval_acc_finish on one accumulator of 16 M keys. Every figure is the median (and the range)
of `reps` calls after three warm-up calls, a host clock around a call that ends in a device synchronise; one process, the two calls of a
pair alternating shape by shape. The scores are standard normal, rounded to 1/64 so that ties occur, the labels drawn from their sigmoid.
"""
import statistics
import sys
import time

import numpy as np
import torch

from gdmix_amd import metrics, synthetic
from gdmix_amd.solver import REDeviceSolver

REPS = int(sys.argv[1]) if len(sys.argv) > 1 else 12


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


def line(what, t):
    med, lo, hi = t
    print(f"{what:<58s} {med:9.3f} ms  (min {lo:.3f}, max {hi:.3f}, {REPS} calls)", flush=True)


s = REDeviceSolver(0)
ks = (1, 5, 10, 100)
ranker, pr = metrics.RankingEvaluator(s, ks), metrics.AuprEvaluator(s)
gen = torch.Generator(device=s.device).manual_seed(5)
shapes = (("C2-shaped: 1 M entities x 16 samples", np.arange(0, 16 * 1_000_000 + 1, 16, dtype=np.int64)),
          ("MovieLens-20M per movie", np.asarray(synthetic.make_movielens_20m(kind="per_movie", seed=200).ent_row_ptr, np.int64)))
for what, rp in shapes:
    n = np.diff(rp)
    N = int(rp[-1])
    score = (torch.randn(N, device=s.device, generator=gen) * 64.0).round() / 64.0
    label = (torch.rand(N, device=s.device, generator=gen) < torch.sigmoid(score)).to(torch.float32)
    rp_dev = torch.from_numpy(rp).to(s.device)
    print(f"{what}: {n.size} entities, {N} samples (largest entity {int(n.max())}, {int((n > 64).sum())} entities / {int(n[n > 64].sum())} samples on the sort path)")
    topk = timed(lambda: ranker.entities(rp_dev, score, label, with_auc=False))
    aupr = timed(lambda: pr.entities(rp_dev, score, label))
    line(f"  gdmix_re_eval_topk_entities, k = {list(ks)}, no auc_out", topk)
    line("  gdmix_re_eval_aupr_entities", aupr)
    h = pr.to_host(pr.entities(rp_dev, score, label))
    print(f"  aupr / topk = {aupr[0] / topk[0]:.3f}; mean AUPR over the entities with a positive: {float(np.nanmean(h['aupr'])):.4f}", flush=True)

N = 16_000_000
score = (torch.randn(N, device=s.device, generator=gen) * 64.0).round() / 64.0
label = (torch.rand(N, device=s.device, generator=gen) < torch.sigmoid(score)).to(torch.float32)
ev = metrics.DeviceEvaluator(s)
ev.reserve(N)
ev.add(score, label)
print(f"one accumulator of {N} keys")
auc = timed(ev.finish)
aupr = timed(lambda: pr.finish(ev))
line("  gdmix_re_eval_acc_finish", auc)
line("  gdmix_re_eval_aupr_acc_finish", aupr)
a, b = pr.finish(ev), pr.finish(ev)
assert np.float64(a["pr_sum"]).view(np.uint64) == np.float64(b["pr_sum"]).view(np.uint64)
print(f"  aupr / auc = {aupr[0] / auc[0]:.3f}; AUC {ev.finish()['auc']:.6f}, AUPR {a['aupr']:.6f} (two runs: the same bits)")
s.close()
