"""The random effect's squared loss (--model_type=linear_regression) against the logistic loss on the same draws, in one process:
C2 shape and the two MovieLens-20M entity-size shapes. Steps (pack + solve) run under HIP events after a warm-up; per-class kernel times
come from a second set of steps with the library's own per-class events switched on (gdmix_re_set_timing serialises the side streams, so
they are kept out of the step time).

    python tools/re_linear_bench.py [--entities 1000000] [--steps 5] [--warmup 2] [--out profiles/re_linear_bench.txt]

Reports per shape and loss: ms per step, entities/s, mean nfev, the kernel time of every class above 2 % of the solve, and for the
dominant class ms / entities / mean nfev of its entities for both losses: a trip (evaluation and step) of one entity with and without the
transcendental part (exp, log, reciprocal) — to be read next to the two mean nfev, since the squared loss runs more iterations and a
later iteration's direction step works with more history pairs. Also the size of libgdmix_re.so and its build id.
"""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gdmix_amd import build, synthetic      # noqa: E402
from gdmix_amd.solver import REDeviceSolver, SolverOptions


def measure(s, dev_raw, kw, steps, warmup):
    def step():
        return s.solve(s.pack(dev_raw), SolverOptions(**kw))
    for _ in range(warmup):
        res = step()
    torch.cuda.synchronize()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    ev[0].record()
    for _ in range(steps):
        res = step()
    ev[1].record()
    torch.cuda.synchronize()
    ms = ev[0].elapsed_time(ev[1]) / steps
    s.set_timing(True)
    cls_ms = np.zeros(len(s.last_solve_ms()))
    try:
        for _ in range(steps):
            packed = s.pack(dev_raw)
            res = s.solve(packed, SolverOptions(**kw))
            torch.cuda.synchronize()
            cls_ms += np.array(s.last_solve_ms())
    finally:
        s.set_timing(False)
    cls_ms /= steps
    host = res.to_host(keys=("nfev", "status"))
    counts = s.class_counts(packed)
    order = packed._view(packed.c.order, packed.E, torch.int32).cpu().numpy() if hasattr(packed.c, "order") else None
    return ms, cls_ms, counts, host, order


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--entities", type=int, default=1_000_000)
    ap.add_argument("--ml-entities", type=int, default=0, help="entities of the MovieLens-20M shapes (0: the data set's own counts)")
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    lines = []

    def say(x):
        print(x, flush=True)
        lines.append(x)
    s = REDeviceSolver(0)
    say(f"build id {s.lib.gdmix_re_build_id().decode()}  libgdmix_re.so {os.path.getsize(build.LIB)} bytes  device {torch.cuda.get_device_name(0)}")
    say(f"steps {a.steps} after {a.warmup} warm-up; step = pack + solve (l2 1, m 10, max_iter 100, ftol 1e-12, unregularised intercept), HIP events")
    shapes = [("c2", lambda: synthetic.make_batch(a.entities, 16, 4, 1024, seed=synthetic.C2_SEED, with_uid=False)),
              ("ml20m_per_user", lambda: synthetic.make_movielens_20m("per_user", entities=a.ml_entities or None)),
              ("ml20m_per_movie", lambda: synthetic.make_movielens_20m("per_movie", entities=a.ml_entities or None))]
    kw0 = dict(l2=1.0, regularize_bias=False, has_intercept=True, m=10, max_iter=100, ftol=1e-12)
    for name, make in shapes:
        b = make()
        per = {}
        for loss, raw in (("logistic", b), ("linear", synthetic.with_real_labels(b, seed=1))):
            dev_raw = s.upload(raw)
            ms, cls_ms, counts, host, order = measure(s, dev_raw, dict(kw0, linear=(loss == "linear")), a.steps, a.warmup)
            nfev = host["nfev"].astype(np.float64)
            say(f"{name} {loss}: {raw.E} entities, {raw.N} samples: {ms:.3f} ms per step, {raw.E / ms / 1e3:.2f} M entities/s, mean nfev {nfev.mean():.2f}, "
                f"status counts {np.bincount(host['status'], minlength=3).tolist()}")
            total = cls_ms.sum()
            begin = 0
            for c, ((kname, cnt), t) in enumerate(zip(counts, cls_ms)):
                if cnt and order is not None:
                    ents = order[begin:begin + cnt]
                    mean_nfev = float(nfev[ents].mean())
                else:
                    mean_nfev = float(nfev.mean())
                if cnt and t >= 0.02 * total:
                    say(f"    class {c:2d} {kname}: {cnt} entities, {t:.3f} ms, mean nfev {mean_nfev:.2f}, {t * 1e6 / cnt / mean_nfev:.2f} ns per entity and evaluation")
                    per.setdefault(c, {})[loss] = (kname, cnt, t, mean_nfev)
                begin += cnt
            del dev_raw
        both = {c: v for c, v in per.items() if len(v) == 2}
        if both:
            c = max(both, key=lambda c: both[c]["logistic"][2])
            lo, li = both[c]["logistic"], both[c]["linear"]
            a_lo, a_li = lo[2] * 1e6 / lo[1] / lo[3], li[2] * 1e6 / li[1] / li[3]
            say(f"  dominant class {c} {lo[0]}: ms / entities / mean nfev: logistic {a_lo:.2f} ns, linear {a_li:.2f} ns, linear / logistic {a_li / a_lo:.2f} "
                f"(mean nfev {lo[3]:.2f} / {li[3]:.2f}: a run of more iterations works with a fuller history, so its average trip costs more)")
    s.close()
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    sys.exit(main())
