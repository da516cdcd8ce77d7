"""--features_to_samples_ratio on the C2 batch against the stage without the flag, in one process on one device: what the selection
costs (the pass itself and the second pack) and what it saves (the solve of entities that moved into narrower size classes).

    python tools/feature_selection_bench.py [--entities 1000000] [--ratio 0.5] [--steps 5] [--warmup 2] [--out profiles/feature_selection.txt]

A step without the flag is pack + solve: the yardstick. A step with it is pack + select (gdmix_re_select_plan + _apply) + pack + solve.
Parts are timed with HIP events on the solver's stream after a warm-up; the selection synchronises once (its counts), which the events
include. The expectation to record, not a bar: the flagged step is not slower.
"""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gdmix_amd import build, synthetic      # noqa: E402
from gdmix_amd.solver import REDeviceSolver, SolverOptions      # noqa: E402


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    b.synchronize()
    return out, a.elapsed_time(b)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--entities", type=int, default=1_000_000)
    ap.add_argument("--ratio", type=float, default=0.5)
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
    say(f"steps {a.steps} after {a.warmup} warm-up; logistic loss, l2 1, m 10, max_iter 100, ftol 1e-12, unregularised intercept; HIP events, ms")
    opts = SolverOptions(l2=1.0, regularize_bias=False, has_intercept=True, m=10, max_iter=100, ftol=1e-12)
    b = synthetic.make_batch(a.entities, 16, 4, 1024, seed=synthetic.C2_SEED, with_uid=False)
    raw = s.upload(b)
    plain, flagged, counts, classes = [], [], None, {}
    for step in range(a.warmup + a.steps):
        packed, t_pack = timed(lambda: s.pack(raw, has_intercept=True))
        res, t_solve = timed(lambda: s.solve(packed, opts))
        if step >= a.warmup:
            plain.append((t_pack, t_solve))
        classes["without"] = [(n, c) for n, c in s.class_counts(packed) if c]
        nfev0 = float(res.nfev.double().mean())
        del res
        packed, t_pack = timed(lambda: s.pack(raw, has_intercept=True))
        (filtered, keep, counts), t_select = timed(lambda: s.select_features(raw, packed, a.ratio))
        packed2, t_pack2 = timed(lambda: s.pack(filtered, has_intercept=True))
        res, t_solve = timed(lambda: s.solve(packed2, opts))
        if step >= a.warmup:
            flagged.append((t_pack, t_select, t_pack2, t_solve))
        classes["with"] = [(n, c) for n, c in s.class_counts(packed2) if c]
        nfev1 = float(res.nfev.double().mean())
        del res, packed, packed2, filtered, keep
    p, f = np.median(np.array(plain), axis=0), np.median(np.array(flagged), axis=0)
    say(f"c2: {b.E} entities, {b.N} samples, {b.Z} non-zeros; ratio {a.ratio:g}: {counts}")
    say(f"without the flag (the yardstick): pack {p[0]:.3f} + solve {p[1]:.3f} = {p.sum():.3f} ms per step (medians), {b.E / p.sum() / 1e3:.2f} M entities/s, mean nfev {nfev0:.2f}")
    say(f"with the flag: pack {f[0]:.3f} + select {f[1]:.3f} + second pack {f[2]:.3f} + solve {f[3]:.3f} = {f.sum():.3f} ms per step (medians), "
        f"{b.E / f.sum() / 1e3:.2f} M entities/s, mean nfev {nfev1:.2f}")
    say(f"flagged / plain: {f.sum() / p.sum():.3f} (solve alone {f[3] / p[1]:.3f})")
    for k in ("without", "with"):
        say(f"  classes {k} the flag: " + "; ".join(f"{n}: {c}" for n, c in classes[k]))
    s.close()
    if a.out:
        with open(a.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    sys.exit(main())
