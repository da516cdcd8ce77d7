"""Time of NDCG@K on the device (include/gdmix_re.h, "NDCG"; csrc/re_evaluate_ndcg.hip) next to its yardstick, the precision@k call.

    PYTHONPATH=. python tools/ndcg_bench.py [reps] > profiles/ndcg.txt

gdmix_re_eval_ndcg_entities next to gdmix_re_eval_topk_entities (without auc_out), four values of K each, on the same batch in the same run:
a C2-shaped batch (1 M entities x 16 samples: the register path alone), a MovieLens-20M per-movie-shaped batch with ratings as labels (most
samples on the sort path), and that batch with the small limit at 0 (every entity on the sort path). Every figure is the median (and the
range) of `reps` calls after three warm-up calls, a host clock around a call that ends in a device synchronise; one process, the two calls
of a pair alternating shape by shape. The scores are standard normal, rounded to 1/64 so that ties occur; the labels are half stars in
[0.5, 5] that follow the score (the top-k call reads them as its binary labels: a label above 0.5 is positive).
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
ranker, nd = metrics.RankingEvaluator(s, ks), metrics.NdcgEvaluator(s, ks)
gen = torch.Generator(device=s.device).manual_seed(7)
movies = np.asarray(synthetic.make_movielens_20m(kind="per_movie", seed=200).ent_row_ptr, np.int64)
shapes = (("C2-shaped: 1 M entities x 16 samples", np.arange(0, 16 * 1_000_000 + 1, 16, dtype=np.int64), 64),
          ("MovieLens-20M per movie", movies, 64), ("MovieLens-20M per movie, every entity on the sort path", movies, 0))
for what, rp, small_max in shapes:
    n = np.diff(rp)
    N = int(rp[-1])
    score = (torch.randn(N, device=s.device, generator=gen) * 64.0).round() / 64.0
    label = ((torch.sigmoid(score + torch.randn(N, device=s.device, generator=gen)) * 10.0).ceil().clamp(1.0, 10.0) / 2.0).to(torch.float32)
    rp_dev = torch.from_numpy(rp).to(s.device)
    nd.set_small_max(small_max)
    print(f"{what}: {n.size} entities, {N} samples (largest entity {int(n.max())}, {int((n > small_max).sum())} entities / {int(n[n > small_max].sum())} samples on the sort path)")
    topk = timed(lambda: ranker.entities(rp_dev, score, label, with_auc=False))
    ndcg = timed(lambda: nd.entities(rp_dev, score, label))
    line(f"  gdmix_re_eval_topk_entities, k = {list(ks)}, no auc_out", topk)
    line(f"  gdmix_re_eval_ndcg_entities, K = {list(ks)}", ndcg)
    h = nd.to_host(nd.entities(rp_dev, score, label))
    print(f"  ndcg / topk = {ndcg[0] / topk[0]:.3f}; mean NDCG@10 over the entities where it is defined: {float(np.nanmean(h[metrics.ndcg_key(10)])):.4f}", flush=True)
nd.set_small_max(64)
s.close()
