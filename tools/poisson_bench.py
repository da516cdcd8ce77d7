"""The random effect's Poisson loss (--model_type=poisson_regression) against the logistic loss on the C2 batch, in one process, per class:
ms / entities / mean nfev. Steps (pack + solve) run under HIP events after a warm-up; per-class kernel times come from a second set of
steps with the library's own per-class events switched on (tools/re_linear_bench.py does the same for the squared loss and explains why
the two sets are kept apart).

    python tools/poisson_bench.py [--entities 1000000] [--steps 5] [--warmup 2] [--out profiles/poisson_bench.txt]

The expectation it is there to check: one exp replaces exp + log + two refined reciprocals, so an evaluation of a Poisson entity should
cost no more than one of a logistic entity. The two losses run different numbers of evaluations, and a later iteration's direction step
works with more history pairs: read the ratio next to the two mean nfev.
"""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from gdmix_amd import build, synthetic      # noqa: E402
from gdmix_amd.solver import REDeviceSolver      # noqa: E402
from re_linear_bench import measure      # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--entities", type=int, default=1_000_000)
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
    kw0 = dict(l2=1.0, regularize_bias=False, has_intercept=True, m=10, max_iter=100, ftol=1e-12)
    b = synthetic.make_batch(a.entities, 16, 4, 1024, seed=synthetic.C2_SEED, with_uid=False)
    per = {}
    for loss, raw in (("logistic", b), ("poisson", synthetic.with_count_labels(b, seed=1))):
        dev_raw = s.upload(raw)
        ms, cls_ms, counts, host, order = measure(s, dev_raw, dict(kw0, loss=loss), a.steps, a.warmup)
        nfev = host["nfev"].astype(np.float64)
        say(f"c2 {loss}: {raw.E} entities, {raw.N} samples: {ms:.3f} ms per step, {raw.E / ms / 1e3:.2f} M entities/s, mean nfev {nfev.mean():.2f}, "
            f"status counts {np.bincount(host['status'], minlength=5).tolist()}")
        begin = 0
        for c, ((kname, cnt), t) in enumerate(zip(counts, cls_ms)):
            if cnt:
                mean_nfev = float(nfev[order[begin:begin + cnt]].mean()) if order is not None else float(nfev.mean())
                say(f"    class {c:2d} {kname}: {cnt} entities, {t:.3f} ms, mean nfev {mean_nfev:.2f}, {t * 1e6 / cnt / mean_nfev:.2f} ns per entity and evaluation")
                per.setdefault(c, {})[loss] = (kname, cnt, t, mean_nfev)
            begin += cnt
        del dev_raw
    for c, v in sorted(per.items()):
        if len(v) == 2:
            lo, po = v["logistic"], v["poisson"]
            a_lo, a_po = lo[2] * 1e6 / lo[1] / lo[3], po[2] * 1e6 / po[1] / po[3]
            say(f"  class {c:2d} {lo[0]}: ms / entities / mean nfev: logistic {a_lo:.2f} ns, poisson {a_po:.2f} ns, poisson / logistic {a_po / a_lo:.3f} "
                f"(mean nfev {lo[3]:.2f} / {po[3]:.2f})")
    s.close()
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    sys.exit(main())
