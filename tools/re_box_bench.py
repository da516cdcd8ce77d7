"""What the random effect's bounded solve costs next to its elastic-net solve (include/gdmix_re.h, "box constraints" and "elastic net";
csrc/re_owlqn.hip under ReBoxRule and ReOwlRule: the same two kernels, the same routing).

    python tools/re_box_bench.py [--entities 1000000] [--steps 5] [--warmup 2] [--out profiles/re_box.txt]

The C2-shaped batch of profiles/re_l1.txt, packed once. In one process and in alternation: the bounded solve under a sign constraint
(lower bound 0) on every third feature of the bag, and the elastic-net solve at alpha = 0.5 of lambda = 1, both with the stage's
tolerances; torch events around REDeviceSolver.solve, results left on the device. Reported for both: ms per solve, evaluations per entity,
ms per evaluation; for the bounded solve the share of coefficients at a bound. The yardstick is the elastic-net solve's ms per evaluation
in this same run, existing code on the same kernels: the bounded solve's may be at most BAR times it — two more vectors are read per
elementwise pass, an entity needs 8 p bytes more LDS, and the run-to-run spread is about +-20 % (the margin the fixed effect set for its
bounded step, tools/fe_box_bench.py). Without a device the output says "not measured". What the output file holds from its first line of
dashes on (profiles/re_box.txt: the elastic net on the parent's library and on this one, bench.py in alternation) is kept as it is."""
import argparse
import os
import sys

import numpy as np

BAR = 1.25


def sign_tables(D):
    """Lower bound 0 on every third feature of the bag, by global feature id."""
    lo = np.full(D, -np.inf)
    lo[0:D:3] = 0.0
    return lo, np.full(D, np.inf)


def measure(E, steps, warmup):
    import torch
    from gdmix_amd import synthetic
    from gdmix_amd.solver import REDeviceSolver, SolverOptions
    D = 1024
    b = synthetic.make_survey_batch(E, 16, 4, D, seed=synthetic.C2_SEED)
    solver = REDeviceSolver(0)
    packed = solver.pack(b, has_intercept=True)
    lines = [f"C2-shaped synthetic batch (make_survey_batch({E}, 16, 4, {D}, seed=C2_SEED)): {packed.E} entities, {b.N} samples, {b.Z} non-zeros, {packed.P} coefficients",
             f"stage tolerances (pgtol 1e-5, ftol 1e-12, max_iter 100, m 10), intercept regularised; median of {steps} timed solves after {warmup} warm-up solves, "
             "the two solves in alternation"]
    lo, hi = sign_tables(D)
    bounds = solver.upload_bounds(lo, hi)
    kinds = {"bounded": (SolverOptions(l2=1.0, ftol=1e-12), dict(bounds=bounds)),
             "elastic net": (SolverOptions(l2=0.5, ftol=1e-12), dict(l1=0.5))}
    ms, last, counts = {k: [] for k in kinds}, {}, {}
    for step in range(warmup + steps):
        for k, (opts, kw) in kinds.items():
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            res = solver.solve(packed, opts, **kw)
            t1.record()
            torch.cuda.synchronize()
            if step >= warmup:
                ms[k].append(t0.elapsed_time(t1))
            last[k], counts[k] = res, solver.box_counts(packed)
    per_eval = {}
    for k in kinds:
        r = last[k].to_host()
        med, nfev = float(np.median(ms[k])), float(r["nfev"].mean())
        per_eval[k] = med / nfev
        what = "sign constraint on every third feature, l2 = 1" if k == "bounded" else "alpha = 0.5 of lambda = 1 (l1 = 0.5, l2 = 0.5)"
        lines.append(f"{k}, {what}: {med:.3f} ms per solve (runs {', '.join(f'{x:.3f}' for x in ms[k])}); nit mean {r['nit'].mean():.2f}, "
                     f"evaluations per entity {nfev:.2f}; {per_eval[k]:.3f} ms per evaluation; status counts {np.bincount(r['status'], minlength=5).tolist()}; "
                     f"{counts[k][0]} entities on re_owlqn_wave_kernel, {counts[k][1]} on re_owlqn_block_kernel")
        if k == "bounded":
            uniq = packed.unique_global().cpu().numpy()
            cp = packed.coef_ptr_host()
            feature = np.ones(int(cp[-1]), bool)
            feature[cp[:-1]] = False
            th = r["theta"][feature]
            at = int(np.count_nonzero((th == lo[uniq]) | (th == hi[uniq])))
            lines.append(f"bounded: {at} of {r['theta'].size} coefficients at a bound ({100.0 * at / r['theta'].size:.1f} %), "
                         f"{int(np.isfinite(lo[uniq]).sum())} of them bounded at all")
    ratio = per_eval["bounded"] / per_eval["elastic net"]
    lines.append(f"bounded / elastic net, ms per evaluation: {ratio:.2f} x (bar: at most {BAR}) -> {'held' if ratio <= BAR else 'MISSED'}")
    solver.close()
    return lines


def main():
    here = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, here)
    ap = argparse.ArgumentParser()
    ap.add_argument("--entities", type=int, default=1_000_000)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(here, "profiles", "re_box.txt"))
    a = ap.parse_args()
    head = ["Random effect, the bounded solve (gdmix_re_solve_box) next to the elastic-net solve (gdmix_re_solve_l1): 1 x MI355X, torch events around "
            "REDeviceSolver.solve, results left on the device."]
    try:
        import torch
        have = torch.cuda.is_available()
    except Exception:
        have = False
    lines = head + (measure(a.entities, a.steps, a.warmup) if have else ["not measured: no device"])
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    if os.path.exists(a.out):
        kept = open(a.out).read()
        at = kept.find("\n----")
        if at >= 0:
            text += kept[at:]
    with open(a.out, "w") as f:
        f.write(text)
    print(text, end="")


if __name__ == "__main__":
    main()
