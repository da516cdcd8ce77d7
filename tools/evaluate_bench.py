"""Time of the device evaluator (gdmix_amd/metrics.py, csrc/re_evaluate.hip) on the C2 scored batch (1 M entities, 16 M samples), next to
gdmix_re_score on the same batch and next to the numpy reference on the host.

    PYTHONPATH=. python tools/evaluate_bench.py [entities] [reps] > profiles/evaluate_bench.txt

Every figure is the median (and the range) of `reps` calls after three warm-up calls, a host clock around a call that ends in a device
synchronise: (a) gdmix_re_eval_entities by default routing and with every entity forced through the sort path, (b) accumulate + finish of
the same samples (as one batch, and as sixteen). Bytes are the algorithm's: 8 B per sample read, 40 B per entity written.
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

E = int(sys.argv[1]) if len(sys.argv) > 1 else 1_000_000
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
