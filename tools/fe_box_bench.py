"""What the projected L-BFGS step of the fixed effect costs next to the L-BFGS-B and OWL-QN steps (include/gdmix_fe.h, "(ABI 26) box
constraints"; csrc/fe_qn.hip under BoxRule).

    python tools/fe_box_bench.py [--rows 4000000] [--evals 40] [--out profiles/fe_box.txt]

The shard of tools/fe_l1_bench.py (rows x 32 uniform columns of 100 000 features, logistic, m = 10), packed once; every step is timed in this
one run, one by one, with events on the stream around gdmix_fe_step_async, the passes around gdmix_fe_eval. After each OWL-QN or bounded step
the host reads nit: a step behind which it rose was an ACCEPTED step (pair stored, new direction over the history, first trial), any other a
BACKTRACKING step (a new trial from x, d and the bounds: no history read). The bounds are a sign constraint (lower bound 0) on every third
feature. The bounded step is held against the OWL-QN step of the same run, existing code with the same three launches: its median may be at
most BAR times OWL-QN's — it reads two more vectors of P doubles, and the run-to-run spread recorded in profiles/fe_l1_step.txt is about
+-20 %. Then the fit itself under the sign constraint with the stage's stop tests. Without a device the output says "not measured"."""
import argparse
import os
import sys

import numpy as np

from fe_l1_bench import L1_TIMED, fmt, shard, timed_steps

BAR = 1.25


def sign_bounds(P):
    """Lower bound 0 on every third feature; the intercept (last) free."""
    lo, hi = np.full(P, -np.inf), np.full(P, np.inf)
    lo[0:P - 1:3] = 0.0
    return lo, hi


def measure(rows, evals):
    import torch
    from gdmix_amd import fixed_effect as fe
    from gdmix_amd.solver import REDeviceSolver, SolverOptions
    solver = REDeviceSolver(0)
    packed, D = shard(solver, fe, rows)
    endless = SolverOptions(l2=1.0, regularize_bias=True, has_intercept=True, m=10, max_iter=10 * evals, threshold=0.0, sum_loss=True, ftol=0.0, pgtol=0.0)
    lo, hi = sign_bounds(D + 1)
    up = lambda a: torch.from_numpy(a).to(solver.device)
    lo_dev, hi_dev = up(lo), up(hi)
    lines, med = [], {}
    for fused in ("1", "0"):
        os.environ["GDMIX_FE_FUSED_TAIL"] = fused
        prob = fe._SteppingProblem(solver, packed, D, endless, None)
        timed_steps(torch, prob, 4, False)      # warm-up
        prob.restart(endless, None)
        t = timed_steps(torch, prob, evals, False)[2:]      # (the first steps run over a short history)
        lines.append(f"L-BFGS-B step, {'one launch' if fused == '1' else 'three launches'}: {fmt([s for _, s, _ in t])}; passes {fmt([p for p, _, _ in t])}")
        if fused == "0":
            for name, select in (("OWL-QN", lambda: prob.set_l1(L1_TIMED)), ("bounded", lambda: (prob.set_l1(0.0), prob.set_bounds(lo_dev, hi_dev)))):
                select()
                timed_steps(torch, prob, 4, True)
                prob.restart(endless, None)
                t = timed_steps(torch, prob, evals, True)
                acc, back = [s for _, s, a in t[2:] if a], [s for _, s, a in t[2:] if not a]
                med[name] = (np.median(acc) if acc else None, np.median(back) if back else None)
                what = f"at l1 = {L1_TIMED}" if name == "OWL-QN" else "under a sign constraint on every third feature"
                lines.append(f"{name} step {what}, accepted (three launches): {fmt(acc)}")
                lines.append(f"{name} step {what}, backtracking (three launches): {fmt(back)}; passes {fmt([p for p, _, _ in t])}")
            for kind, (b, o) in (("accepted", (med["bounded"][0], med["OWL-QN"][0])), ("backtracking", (med["bounded"][1], med["OWL-QN"][1]))):
                if b is None or o is None:
                    lines.append(f"bounded / OWL-QN, {kind}: not observed in both")
                else:
                    lines.append(f"bounded / OWL-QN, {kind}: {b / o:.2f} x the median (bar: at most {BAR}) -> {'held' if b <= BAR * o else 'MISSED'}")
            stage = fe.fit_options(True, 1.0, True, fe.LOGISTIC_REGRESSION, 100, 10, 1e-12)
            for name, select in (("without bounds (the L-BFGS-B step)", lambda: prob.set_bounds(None, None)),
                                 ("under the sign constraint", lambda: prob.set_bounds(lo_dev, hi_dev))):
                select()
                prob.restart(stage, None)
                status, _ = prob.solve()
                theta, info = prob.result()
                lines.append(f"fit {name} (l2 = 1, max_iter 100, tolerance 1e-12): status {status}, {info['nit']} iterations, {info['nfev']} evaluations, "
                             f"F {info['fval']!r}, {fe.count_at_bound(theta, (lo, hi))} of {theta.size} coefficients at a bound")
        prob.close()
    return lines


def main():
    here = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, here)
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=4_000_000)
    ap.add_argument("--evals", type=int, default=40)
    ap.add_argument("--out", default=os.path.join(here, "profiles", "fe_box.txt"))
    a = ap.parse_args()
    head = [f"fixed effect, the bounded (projected L-BFGS) step next to the L-BFGS-B and OWL-QN steps: {a.rows} samples x 32 uniform columns of 100000 features, "
            "logistic, m = 10", "one figure per step, events on the stream around the step's launches; median (min, max)"]
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
