"""What the OWL-QN step of the fixed effect costs next to the L-BFGS-B step (include/gdmix_fe.h, "(ABI 23) L1 / elastic net"; csrc/fe_qn.hip under OwlRule).

    python tools/fe_l1_bench.py [--rows 4000000] [--evals 40] [--out profiles/fe_l1_step.txt]

The shard of tools/fe_bench.py and bench.py's fixed-effect leg (rows x 32 uniform columns of 100 000 features, logistic, m = 10), packed once.
Steps are timed one by one with events on the stream around gdmix_fe_step_async; the passes around gdmix_fe_eval. After each OWL-QN step the
host reads nit: a step behind which it rose was an ACCEPTED step (pair stored, new direction over the history, first trial), any other a
BACKTRACKING step (a new trial from x, d and the orthant: no history read). The L-BFGS-B step is timed in both forms (GDMIX_FE_FUSED_TAIL=1 / 0,
a problem each: the hook is read at creation). Then the fit itself at l1 in {0.1, 1, 10} with the stage's stop tests: evaluations, iterations,
status and the model's non-zeros. Without a device the output says "not measured"."""
import argparse
import os
import sys

import numpy as np

L1_TIMED = 1.0
L1_GRID = (0.1, 1.0, 10.0)


def shard(solver, fe, rows):
    rng = np.random.default_rng(0)
    n, k, D = rows, 32, 100_000
    cols = rng.integers(0, D, n * k, dtype=np.int64)
    vals = (rng.random(n * k, dtype=np.float32) - 0.5) * 2.0
    y = (rng.random(n, dtype=np.float32) < 0.5).astype(np.float32)
    batch, _ = fe.shard_as_batch(np.arange(n + 1, dtype=np.int64) * k, cols, vals, y, np.zeros(n, np.float32), None, True)
    return solver.pack(batch), D


def timed_steps(torch, prob, evals, classify):
    """-> [(passes ms, step ms, accepted?)] of up to `evals` evaluations; stops at the problem's stop."""
    out, nit = [], 0
    for _ in range(evals):
        e = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
        e[0].record()
        prob.eval()
        e[1].record()
        seq = prob.step_async()
        e[2].record()
        status = prob.step_status(seq)
        torch.cuda.synchronize()
        accepted = None
        if classify:
            _, info = prob.result()
            accepted, nit = info["nit"] > nit, info["nit"]
        out.append((e[0].elapsed_time(e[1]), e[1].elapsed_time(e[2]), accepted))
        if status >= 0:
            break
    return out


def fmt(x):
    return f"{1e3 * np.median(x):.1f} us (min {1e3 * min(x):.1f}, max {1e3 * max(x):.1f}, {len(x)} steps)" if len(x) else "not observed"


def measure(rows, evals):
    import torch
    from gdmix_amd import fixed_effect as fe
    from gdmix_amd.solver import REDeviceSolver, SolverOptions
    solver = REDeviceSolver(0)
    packed, D = shard(solver, fe, rows)
    endless = SolverOptions(l2=1.0, regularize_bias=True, has_intercept=True, m=10, max_iter=10 * evals, threshold=0.0, sum_loss=True, ftol=0.0, pgtol=0.0)
    lines = []
    for fused in ("1", "0"):
        os.environ["GDMIX_FE_FUSED_TAIL"] = fused
        prob = fe._SteppingProblem(solver, packed, D, endless, None)
        timed_steps(torch, prob, 4, False)      # warm-up
        prob.restart(endless, None)
        t = timed_steps(torch, prob, evals, False)[2:]      # (the first steps run over a short history)
        lines.append(f"L-BFGS-B step, {'one launch' if fused == '1' else 'three launches'}: {fmt([s for _, s, _ in t])}; passes {fmt([p for p, _, _ in t])}")
        if fused == "0":
            prob.set_l1(L1_TIMED)
            timed_steps(torch, prob, 4, True)
            prob.restart(endless, None)
            t = timed_steps(torch, prob, evals, True)
            lines.append(f"OWL-QN step at l1 = {L1_TIMED}, accepted (three launches): {fmt([s for _, s, a in t[2:] if a])}")
            lines.append(f"OWL-QN step at l1 = {L1_TIMED}, backtracking (three launches): {fmt([s for _, s, a in t[2:] if not a])}; passes {fmt([p for p, _, _ in t])}")
            stage = fe.fit_options(True, 1.0, True, fe.LOGISTIC_REGRESSION, 100, 10, 1e-12)
            for l1 in (0.0,) + L1_GRID:
                prob.set_l1(l1)
                prob.restart(stage, None)
                status, _ = prob.solve()
                theta, info = prob.result()
                lines.append(f"fit at l1 = {l1} (l2 = 1, max_iter 100, tolerance 1e-12): status {status}, {info['nit']} iterations, {info['nfev']} evaluations, "
                             f"F {info['fval']!r}, {int(np.count_nonzero(theta))} of {theta.size} coefficients non-zero")
        prob.close()
    return lines


def main():
    here = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, here)
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=4_000_000)
    ap.add_argument("--evals", type=int, default=40)
    ap.add_argument("--out", default=os.path.join(here, "profiles", "fe_l1_step.txt"))
    a = ap.parse_args()
    head = [f"fixed effect, the OWL-QN step next to the L-BFGS-B step: {a.rows} samples x 32 uniform columns of 100000 features, logistic, m = 10",
            "one figure per step, events on the stream around the step's launches; median (min, max)"]
    try:
        import torch
        have = torch.cuda.is_available()
    except Exception:
        have = False
    lines = head + (measure(a.rows, a.evals) if have else ["not measured: no device"])
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)
    print(text, end="")


if __name__ == "__main__":
    main()
