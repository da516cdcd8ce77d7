"""Time of the weighted evaluation on the device (include/gdmix_re.h, "weighted evaluation"; csrc/re_evaluate_weighted.hip) next to its
unweighted siblings, in the same run.

    PYTHONPATH=. python tools/weighted_eval_bench.py [reps] > profiles/weighted_eval.txt

Per entity: gdmix_re_eval_w_entities next to gdmix_re_eval_entities on a C2-shaped batch (1 M entities x 16 samples: the register path alone)
and on a MovieLens-20M per-movie-shaped batch (most samples on the sort path). Over a stage: gdmix_re_eval_w_acc_finish next to
gdmix_re_eval_acc_finish on accumulators of 16 M keys. Every figure is the median (and the range) of `reps` calls after three warm-up calls,
a host clock around a call that ends in a device synchronise; one process, the two calls of a pair alternating shape by shape. The scores
are standard normal, rounded to 1/64 so that ties occur, the labels drawn from their sigmoid, the weights log-uniform in [0.01, 100].
"""
import statistics
import sys
import time

import numpy as np
import torch

from gdmix_amd import metrics, synthetic
from gdmix_amd.solver import REDeviceSolver

REPS = int(sys.argv[1]) if len(sys.argv) > 1 else 7


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


def draw(N, gen, device):
    score = (torch.randn(N, device=device, generator=gen) * 64.0).round() / 64.0
    label = (torch.rand(N, device=device, generator=gen) < torch.sigmoid(score)).to(torch.float32)
    weight = torch.exp((torch.rand(N, device=device, generator=gen) * 2.0 - 1.0) * float(np.log(100.0)))
    return score, label, weight


s = REDeviceSolver(0)
plain, weighted = metrics.DeviceEvaluator(s), metrics.WeightedEvaluator(s)
gen = torch.Generator(device=s.device).manual_seed(5)
shapes = (("C2-shaped: 1 M entities x 16 samples", np.arange(0, 16 * 1_000_000 + 1, 16, dtype=np.int64)),
          ("MovieLens-20M per movie", np.asarray(synthetic.make_movielens_20m(kind="per_movie", seed=200).ent_row_ptr, np.int64)))
for what, rp in shapes:
    n = np.diff(rp)
    N = int(rp[-1])
    score, label, weight = draw(N, gen, s.device)
    rp_dev = torch.from_numpy(rp).to(s.device)
    print(f"{what}: {n.size} entities, {N} samples (largest entity {int(n.max())}, {int((n > 64).sum())} entities / {int(n[n > 64].sum())} samples on the sort path)")
    a = timed(lambda: plain.entities(rp_dev, score, label))
    b = timed(lambda: weighted.entities(rp_dev, score, label, weight))
    line("  gdmix_re_eval_entities", a)
    line("  gdmix_re_eval_w_entities", b)
    h = weighted.to_host(weighted.entities(rp_dev, score, label, weight))
    print(f"  weighted / unweighted = {b[0] / a[0]:.3f}; mean weighted AUC over the entities with weight in both classes: {float(np.nanmean(h['weighted_auc'])):.4f}",
          flush=True)

N = 16_000_000
score, label, weight = draw(N, gen, s.device)
plain.reserve(N)
plain.add(score, label)
weighted.reserve(N)
weighted.add(score, label, weight)
print(f"accumulators of {N} keys")
a = timed(plain.finish)
b = timed(weighted.finish)
line("  gdmix_re_eval_acc_finish", a)
line("  gdmix_re_eval_w_acc_finish", b)
x, y = weighted.finish(), weighted.finish()
assert all(np.float64(x[k]).view(np.uint64) == np.float64(y[k]).view(np.uint64) for k in ("two_u_w", "w_pos", "w_neg"))
print(f"  weighted / unweighted = {b[0] / a[0]:.3f}; AUC {plain.finish()['auc']:.6f}, weighted AUC {x['weighted_auc']:.6f} (two runs: the same bits)")
s.close()
