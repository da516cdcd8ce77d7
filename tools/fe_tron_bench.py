"""What the TRON optimiser of the fixed effect costs and buys next to L-BFGS-B (include/gdmix_fe.h, "(ABI 24) TRON"; csrc/fe_tron.hip with the share sums of
csrc/fe_step_shares.hpp, and the HV variant of the row kernels in csrc/fe_solve.hip).

    python tools/fe_tron_bench.py [--rows 4000000] [--pairs 60] [--out profiles/fe_tron_bench.txt]

The shard of tools/fe_bench.py (rows x 32 columns of 100 000 features, standard-normal values, m = 10), uniform and Zipf columns, packed once each.
1. Cost of a product: pass pairs are timed one by one with events on the stream around gdmix_fe_eval. On a TRON problem the host reads the
   product count behind each step: a pair behind which it rose was a PRODUCT, any other an EVALUATION of the HV variant (which also writes the
   curvature weights). The yardstick is the evaluation of an L-BFGS-B problem on the same copies in the same run: the parent's kernels. Medians.
   The library's own events split the second pass pair of each problem into row and column pass (gdmix_fe_last_eval_ms): an evaluation on the
   L-BFGS-B problem, the first product on the TRON problem. The bar: product <= 1.05 x evaluation on both shards.
2. Cost of the step: events around gdmix_fe_step_async, TRON's three launches next to the L-BFGS-B step's three (GDMIX_FE_FUSED_TAIL=0) and one.
3. What it buys: logistic and Poisson labels on the uniform shard at l2 = 1 and 0.01, the stage's tolerances (pgtol 1e-5, ftol 1e-12, m = 10):
   pass pairs and wall time of gdmix_fe_solve to the stop and |g|_inf there, TRON against L-BFGS-B. A report, not a bar.
Without a device the output says "not measured"."""
import argparse
import os
import sys
import time

import numpy as np

MAX_ITER = 1000      # so that the tolerances stop the fits, not the iteration cap


def shard(rows, zipf, label):
    """The arrays of tools/fe_bench.py's shard; label: "logistic" | "poisson"."""
    rng = np.random.default_rng(0)
    n, k, D = rows, 32, 100_000
    if zipf:
        cols = np.minimum((float(D + 1) ** rng.random((n, k))).astype(np.int64) - 1, D - 1)
    else:
        cols = rng.integers(0, D, (n, k), dtype=np.int64)
    vals = rng.standard_normal((n, k), dtype=np.float32)
    w_true = rng.standard_normal(D) * 0.1
    z = (vals * w_true[cols]).sum(1)
    y = (rng.random(n) < 1 / (1 + np.exp(-z))).astype(np.float32) if label == "logistic" else rng.poisson(np.exp(np.minimum(z, 3.0))).astype(np.float32)
    return np.arange(n + 1, dtype=np.int64) * k, cols.ravel(), vals.ravel(), y, D


def timed_pairs(torch, prob, pairs):
    """-> [(pass pair ms, step ms, was a product?)] of up to `pairs` pass pairs; stops at the problem's stop."""
    out, nhv = [], prob.products()
    for _ in range(pairs):
        e = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
        e[0].record()
        prob.eval()
        e[1].record()
        seq = prob.step_async()
        e[2].record()
        status = prob.step_status(seq)
        torch.cuda.synchronize()
        now = prob.products()
        out.append((e[0].elapsed_time(e[1]), e[1].elapsed_time(e[2]), now > nhv))
        nhv = now
        if status >= 0:
            break
    return out


def fmt(x, unit="us"):
    k, nd = (1e3, 1) if unit == "us" else (1.0, 4)
    return f"{k * np.median(x):.{nd}f} {unit} (min {k * min(x):.{nd}f}, max {k * max(x):.{nd}f}, {len(x)})" if len(x) else "not observed"


def product_cost(torch, fe, solver, packed, D, pairs, name):
    from gdmix_amd.solver import SolverOptions
    endless = SolverOptions(l2=1.0, regularize_bias=True, has_intercept=True, m=10, max_iter=100 * pairs, threshold=0.0, sum_loss=True, ftol=0.0, pgtol=0.0)
    lines, med = [], {}
    os.environ["GDMIX_FE_FUSED_TAIL"] = "0"
    prob = fe._SteppingProblem(solver, packed, D, endless, None)
    try:
        for optimizer in ("LBFGS", "TRON"):
            prob.set_optimizer(optimizer)
            timed_pairs(torch, prob, 4)      # warm-up
            prob.restart(endless, None)
            t = timed_pairs(torch, prob, pairs)
            rows_ms, cols_ms = prob.last_eval_ms()
            t = t[2:]
            if optimizer == "LBFGS":
                med["eval"] = np.median([p for p, _, _ in t])
                lines.append(f"{name}: L-BFGS-B problem, evaluation pass pair {fmt([p for p, _, _ in t], 'ms')}; its second pair: rows {rows_ms:.4f} ms, columns {cols_ms:.4f} ms; "
                             f"step (three launches) {fmt([s for _, s, _ in t])}")
            else:
                prod, ev = [p for p, _, h in t if h], [p for p, _, h in t if not h]
                med["product"] = np.median(prod)
                lines.append(f"{name}: TRON problem, product pass pair {fmt(prod, 'ms')}; its first product: rows {rows_ms:.4f} ms, columns {cols_ms:.4f} ms")
                lines.append(f"{name}: TRON problem, evaluation pass pair (HV variant: also writes the curvature weights) {fmt(ev, 'ms')}; "
                             f"step (three launches) behind a product {fmt([s for _, s, h in t if h])}, behind an evaluation {fmt([s for _, s, h in t if not h])}")
        ratio = med["product"] / med["eval"]
        lines.append(f"{name}: product / evaluation = {ratio:.3f} (bar: <= 1.05): {'met' if ratio <= 1.05 else 'MISSED'}")
    finally:
        prob.close()
    os.environ["GDMIX_FE_FUSED_TAIL"] = "1"
    prob = fe._SteppingProblem(solver, packed, D, endless, None)
    try:
        timed_pairs(torch, prob, 4)
        prob.restart(endless, None)
        t = timed_pairs(torch, prob, pairs)[2:]
        lines.append(f"{name}: L-BFGS-B step, one launch {fmt([s for _, s, _ in t])}")
    finally:
        prob.close()
    os.environ.pop("GDMIX_FE_FUSED_TAIL")
    return lines


def what_it_buys(torch, fe, solver, packed, D, label):
    model_type = fe.LOGISTIC_REGRESSION if label == "logistic" else fe.POISSON_REGRESSION
    lines = []
    prob = fe._SteppingProblem(solver, packed, D, fe.fit_options(True, 1.0, True, model_type, MAX_ITER, 10, 1e-12), None)
    try:
        for l2 in (1.0, 0.01):
            opts = fe.fit_options(True, l2, True, model_type, MAX_ITER, 10, 1e-12)
            for optimizer in ("LBFGS", "TRON"):
                prob.set_optimizer(optimizer)
                for _ in range(2):      # the second run is the measured one
                    prob.restart(opts, None)
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    status, _ = prob.solve()
                    torch.cuda.synchronize()
                    dt = time.perf_counter() - t0
                _, info = prob.result()
                nhv = prob.products()
                lines.append(f"{label}, l2 = {l2}, {optimizer}: status {status}, {info['nit']} iterations, {info['nfev']} evaluations + {nhv} products = "
                             f"{info['nfev'] + nhv} pass pairs, {1e3 * dt:.1f} ms to the stop, f {info['fval']!r}, |g|_inf {info['gnorm']:.3e}")
    finally:
        prob.close()
    return lines


def measure(rows, pairs):
    import torch
    from gdmix_amd import fixed_effect as fe
    from gdmix_amd.solver import REDeviceSolver
    solver = REDeviceSolver(0)
    lines = []
    for name, zipf, label in (("uniform", False, "logistic"), ("zipf", True, "logistic"), ("uniform", False, "poisson")):
        rp, cols, vals, y, D = shard(rows, zipf, label)
        batch, _ = fe.shard_as_batch(rp, cols, vals, y, np.zeros(rows, np.float32), None, True, binary_labels=label == "logistic")
        del rp, cols, vals
        packed = solver.pack(batch)
        del batch
        if label == "logistic":
            lines += product_cost(torch, fe, solver, packed, D, pairs, name)
        if not zipf:
            lines += what_it_buys(torch, fe, solver, packed, D, label)
        del packed
        torch.cuda.empty_cache()
    return lines


def main():
    here = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, here)
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=4_000_000)
    ap.add_argument("--pairs", type=int, default=60)
    ap.add_argument("--out", default=os.path.join(here, "profiles", "fe_tron_bench.txt"))
    a = ap.parse_args()
    head = [f"fixed effect, TRON next to L-BFGS-B: {a.rows} samples x 32 columns of 100000 features (tools/fe_bench.py's shard), m = 10",
            "pass pairs and steps timed one by one with events on the stream; median (min, max, count)"]
    try:
        import torch
        have = torch.cuda.is_available()
    except Exception:
        have = False
    lines = head + (measure(a.rows, a.pairs) if have else ["not measured: no device"])
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)
    print(text, end="")


if __name__ == "__main__":
    main()
