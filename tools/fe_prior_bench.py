"""What the prior variants of the fixed-effect kernels cost (include/gdmix_fe.h, "incremental training").

    python tools/fe_prior_bench.py [--rows 4000000] [--evals 12] [--runs 5] [--parent-tree DIR] [--out profiles/fe_prior_step.txt]

The shard of bench.py's fixed-effect leg (rows x 32 uniform columns of 100 000 features, logistic, m = 10), packed once, ONE problem. A run
is a gdmix_fe_restart (or gdmix_fe_set_prior) followed by `evals` evaluations, each timed with events on the stream: the passes
(gdmix_fe_eval) and the step (gdmix_fe_step_async) separately; a run's figure is the median over its evaluations. Runs without a prior and
with a NEUTRAL prior (mu = 0, s = 1: the same trajectory bit for bit, so both do the same work) alternate in one process, `runs` each
after a warm-up; reported: median of the runs with min and max. --parent-tree names a checkout of the parent commit with its library
built: the no-prior runs are repeated on it in a child process of the same call, and the requirement — the no-prior path is no slower
than before — is read off the two spreads. Without a device the output says "not measured"."""
import argparse
import json
import os
import subprocess
import sys

import numpy as np


def measure(tree, rows, evals, runs, with_prior):
    sys.path.insert(0, tree)
    import torch
    from gdmix_amd import fixed_effect as fe
    from gdmix_amd.solver import REDeviceSolver, SolverOptions
    solver = REDeviceSolver(0)
    rng = np.random.default_rng(0)
    n, k, D = rows, 32, 100_000
    cols = rng.integers(0, D, n * k, dtype=np.int64)
    vals = (rng.random(n * k, dtype=np.float32) - 0.5) * 2.0
    y = (rng.random(n, dtype=np.float32) < 0.5).astype(np.float32)
    batch, _ = fe.shard_as_batch(np.arange(n + 1, dtype=np.int64) * k, cols, vals, y, np.zeros(n, np.float32), None, True)
    packed = solver.pack(batch)
    opts = SolverOptions(l2=1.0, regularize_bias=True, has_intercept=True, m=10, max_iter=10 * evals, threshold=0.0, sum_loss=True, ftol=0.0,
                         pgtol=0.0)      # no convergence stop inside a run: a stopped problem's evaluations are no-ops
    prob = fe._SteppingProblem(solver, packed, D, opts, None)
    with_prior = with_prior and hasattr(prob, "set_prior")
    zeros = torch.zeros(D + 1, dtype=torch.float64, device=solver.device)
    ones = torch.ones(D + 1, dtype=torch.float64, device=solver.device)

    def one_run(prior):
        if prior:
            prob.set_prior(zeros, ones)
        elif with_prior:
            prob.set_prior(None, None)
        else:
            prob.restart(opts, None)
        ev = [[torch.cuda.Event(enable_timing=True) for _ in range(3)] for _ in range(evals)]
        for e in ev:
            e[0].record()
            prob.eval()
            e[1].record()
            prob.step_async()
            e[2].record()
        torch.cuda.synchronize()
        _, info = prob.result()
        assert info["nfev"] == evals, "the fit stopped inside the measured evaluations"
        return float(np.median([e[0].elapsed_time(e[1]) for e in ev])), float(np.median([e[1].elapsed_time(e[2]) for e in ev])), info["fval"]

    one_run(False)
    if with_prior:
        one_run(True)
    res = {"plain": [], "prior": []}
    for _ in range(runs):
        res["plain"].append(one_run(False))
        if with_prior:
            res["prior"].append(one_run(True))
    prob.close()
    if with_prior:
        assert {r[2] for r in res["plain"]} == {r[2] for r in res["prior"]}, "a neutral prior must walk the trajectory of no prior"
    return {k: {"passes_ms": [r[0] for r in v], "step_ms": [r[1] for r in v]} for k, v in res.items() if v}


def line(name, d):
    f = lambda x: f"{np.median(x):.4f} (min {min(x):.4f}, max {max(x):.4f})"
    tot = [a + b for a, b in zip(d["passes_ms"], d["step_ms"])]
    return f"{name:<28} passes {f(d['passes_ms'])}   step {f(d['step_ms'])}   evaluation {f(tot)}"


def main():
    here = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=4_000_000)
    ap.add_argument("--evals", type=int, default=12)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--tree", default=here)
    ap.add_argument("--parent-tree", default=None)
    ap.add_argument("--child", action="store_true", help="print the no-prior figures of --tree as JSON (what --parent-tree starts)")
    ap.add_argument("--out", default=os.path.join(here, "profiles", "fe_prior_step.txt"))
    a = ap.parse_args()
    # the one-launch step on both sides: left to itself the library takes the three-launch step on a device another process is present on,
    # and the parent's child process runs next to this one
    os.environ.setdefault("GDMIX_FE_FUSED_TAIL", "1")
    if a.child:
        print("RESULT " + json.dumps(measure(a.tree, a.rows, a.evals, a.runs, False)))
        return
    head = [f"fixed effect, the step with and without a prior: {a.rows} samples x 32 uniform columns of 100000 features, logistic, m = 10",
            f"ms per evaluation, median over {a.runs} runs of {a.evals} evaluations each (a run: median over its evaluations); events on the stream"]
    try:
        import torch
        have = torch.cuda.is_available()
    except Exception:
        have = False
    if not have:
        lines = head + ["not measured: no device"]
    else:
        mine = measure(a.tree, a.rows, a.evals, a.runs, True)
        lines = head + [line("this tree, no prior", mine["plain"]), line("this tree, neutral prior", mine["prior"])]
        if a.parent_tree:
            out = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--tree", a.parent_tree, "--rows", str(a.rows), "--evals", str(a.evals),
                                  "--runs", str(a.runs)], check=True, capture_output=True, text=True, timeout=900).stdout
            parent = json.loads([x for x in out.splitlines() if x.startswith("RESULT ")][-1][7:])
            lines.append(line("parent commit, no prior", parent["plain"]))
            p_tot = [x + y for x, y in zip(parent["plain"]["passes_ms"], parent["plain"]["step_ms"])]
            m_tot = float(np.median([x + y for x, y in zip(mine["plain"]["passes_ms"], mine["plain"]["step_ms"])]))
            verdict = "within" if m_tot <= max(p_tot) else "ABOVE"
            lines.append(f"no prior, this tree: median {m_tot:.4f} ms per evaluation is {verdict} the parent's spread [{min(p_tot):.4f}, {max(p_tot):.4f}]")
        else:
            lines.append("parent commit: not measured (no --parent-tree)")
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)
    print(text, end="")


if __name__ == "__main__":
    main()
