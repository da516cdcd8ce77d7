"""What the column statistics of --feature_normalization cost (csrc/feature_stats.hip, gdmix_amd/feature_stats.py), next to the work of the
stage they precede, on the same arrays in the same process.

    PYTHONPATH=. python tools/feature_stats_bench.py [--entities 1000000] [--rows 4000000] [--features 1048576] [--out profiles/feature_stats.txt]

  1. both passes on the C2 raw batch (entities x 16 samples x 4 non-zeros, D = 1 024: the LDS path), on the int64 ids of the raw form and on
     the uint16 ids of the wire form — next to gdmix_re_pack + gdmix_re_solve of that batch;
  2. both passes on the fixed-effect benchmark shard (rows x 32 columns of 100 000 features: global atomics), uniform and Zipf columns —
     next to one fixed-effect evaluation (passes + step) of the uniform shard;
  3. feature_stats.finish on the host at D = 2^20 (every feature live and dense, a fifth of them constant: the exact-integer branch).

Device events on the stream around each call; one warm-up, then the median of three with [min, max]. A report, not a bar: a statistics pass
that takes longer than the step it precedes is a defect to be explained. Bytes are the algorithm's: 4 B of value and the id per entry and
pass. Without a device the output says "not measured"."""
import argparse
import os
import statistics
import sys
import time

import numpy as np

HBM_PEAK = 8.0e12       # bytes/s, MI355X
RUNS = 3


def timed(torch, fn, runs=RUNS):
    out = fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(runs):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        out = fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return (statistics.median(ms), min(ms), max(ms)), out


def fmt(t):
    return f"{t[0]:9.3f} ms [{t[1]:.3f}, {t[2]:.3f}]"


def passes(torch, solver, fs, D, col, val, lines, what):
    """Time pass 1 and pass 2 over (col, val) device tensors; the accumulators of the last timed call are checked against a fresh one."""
    Z = int(val.numel())
    width = col.element_size()

    def pass1():
        acc = fs.DeviceAccumulator(solver, D)
        acc.add(col, val)
        return acc
    t1, acc = timed(torch, pass1)
    acc.shifts()

    def pass2():
        acc.limbs.zero_()
        acc.add(col, val)
        return acc
    t2, _ = timed(torch, pass2)
    first = acc.host_limbs()
    acc.limbs.zero_()
    acc.add(col, val)
    assert np.array_equal(first, acc.host_limbs()), "two runs of pass 2 must give the same bits"
    assert all(n == 0 for n, _ in acc.take_bad())
    nbytes = (4.0 + width) * Z
    for name, t in (("pass 1 (count, max)", t1), ("pass 2 (moments)", t2)):
        lines.append(f"  {what:<34s} {name:<22s} {fmt(t)}   {nbytes / t[0] / 1e6:8.0f} GB/s, {100.0 * nbytes / (t[0] * 1e-3) / HBM_PEAK:5.1f} % of the HBM peak")
    return t1[0] + t2[0]


def zipf_columns(rng, n, D, power=8):
    return np.minimum((D * rng.random(n) ** power).astype(np.int64), D - 1)


def measure(a):
    import torch
    from gdmix_amd import feature_stats as fs
    from gdmix_amd import fixed_effect as fe
    from gdmix_amd import synthetic
    from gdmix_amd.solver import REDeviceSolver, SolverOptions
    s = REDeviceSolver(0)
    lines = []
    # 1. the C2 raw batch
    b = synthetic.make_batch(a.entities, 16, 4, 1024, seed=synthetic.C2_SEED, with_uid=False)
    raw = s.upload(b)
    t_pack, packed = timed(torch, lambda: s.pack(raw))
    t_solve, _ = timed(torch, lambda: s.solve(packed, SolverOptions()))
    step = t_pack[0] + t_solve[0]
    lines.append(f"1. C2 raw batch: {b.E} entities, {b.N} samples, {b.Z} non-zeros, D = 1024 (LDS path)")
    lines.append(f"  gdmix_re_pack                      {fmt(t_pack)}")
    lines.append(f"  gdmix_re_solve                     {fmt(t_solve)}")
    both = passes(torch, s, fs, 1024, raw["col_global"], raw["val"], lines, "int64 ids (raw form)")
    lines.append(f"  both passes = {both:.3f} ms = {100.0 * both / step:.1f} % of pack + solve ({step:.3f} ms)")
    col16 = torch.from_numpy(b.col_global.astype(np.uint16)).to(s.device)
    both = passes(torch, s, fs, 1024, col16, raw["val"], lines, "uint16 ids (wire form)")
    lines.append(f"  both passes = {both:.3f} ms = {100.0 * both / step:.1f} % of pack + solve ({step:.3f} ms)")
    del packed, raw, col16, b
    torch.cuda.empty_cache()
    # 2. the fixed-effect benchmark shard
    rng = np.random.default_rng(0)
    n, k, D = a.rows, 32, 100_000
    cols = rng.integers(0, D, n * k, dtype=np.int64)
    vals = (rng.random(n * k, dtype=np.float32) - 0.5) * 2.0
    y = (rng.random(n, dtype=np.float32) < 0.5).astype(np.float32)
    batch, _ = fe.shard_as_batch(np.arange(n + 1, dtype=np.int64) * k, cols, vals, y, np.zeros(n, np.float32), None, True)
    packed = s.pack(batch)
    opts = SolverOptions(l2=1.0, regularize_bias=True, has_intercept=True, m=10, max_iter=1000, threshold=0.0, sum_loss=True, ftol=0.0, pgtol=0.0)
    prob = fe._SteppingProblem(s, packed, D, opts, None)

    def evaluation():
        prob.eval()
        prob.step_async()
    t_eval, _ = timed(torch, evaluation)
    prob.close()
    del prob, packed, batch
    torch.cuda.empty_cache()
    lines.append(f"2. fixed-effect shard: {n} samples x {k} columns of {D} features = {n * k} non-zeros (global atomics)")
    lines.append(f"  one evaluation (passes + step)     {fmt(t_eval)}")
    cd, vd = torch.from_numpy(cols).to(s.device), torch.from_numpy(vals).to(s.device)
    both = passes(torch, s, fs, D, cd, vd, lines, "uniform columns")
    lines.append(f"  both passes = {both:.3f} ms = {both / t_eval[0]:.2f} evaluations")
    zc = zipf_columns(rng, n * k, D)
    hottest = int(np.bincount(zc, minlength=D).max())
    cd.copy_(torch.from_numpy(zc))
    both = passes(torch, s, fs, D, cd, vd, lines, f"Zipf columns (hottest {100.0 * hottest / (n * k):.0f} %)")
    lines.append(f"  both passes = {both:.3f} ms = {both / t_eval[0]:.2f} evaluations of the uniform shard")
    s.close()
    return lines


def finish_on_the_host(D, lines):
    from gdmix_amd import feature_stats as fs
    rng = np.random.default_rng(1)
    Z = 4 * D
    col = np.tile(np.arange(D, dtype=np.int64), 4)          # four samples, every feature stored in each
    val = (rng.standard_normal(Z) * np.exp(rng.uniform(-20, 20, D))[col]).astype(np.float32)
    const = col % 5 == 0
    val[const] = np.float32(0.97)
    acc = fs.NumpyAccumulator(D)
    acc.add(col, val)
    L, s1, s2 = acc.shifts()
    acc.add(col, val)
    count, bits = acc.host_extent()
    N = 4
    ms = []
    for _ in range(RUNS + 1):
        t0 = time.perf_counter()
        mean, var = fs.finish(count, bits.view(np.float32), L, s1, s2, acc.limbs, N)
        ms.append(1e3 * (time.perf_counter() - t0))
    ms = ms[1:]
    assert np.all(np.isfinite(var)) and np.all(var >= 0)
    lines.append(f"3. feature_stats.finish on the host, D = {D} (all live, {int((var == 0).sum())} with variance exactly 0)")
    lines.append(f"  finish                             {statistics.median(ms):9.1f} ms [{min(ms):.1f}, {max(ms):.1f}]   (host clock)")


def main():
    here = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    ap = argparse.ArgumentParser()
    ap.add_argument("--entities", type=int, default=1_000_000)
    ap.add_argument("--rows", type=int, default=4_000_000)
    ap.add_argument("--features", type=int, default=1 << 20)
    ap.add_argument("--out", default=os.path.join(here, "profiles", "feature_stats.txt"))
    a = ap.parse_args()
    lines = ["column statistics of --feature_normalization; median of three after a warm-up, [min, max]; events on the stream"]
    try:
        import torch
        have = torch.cuda.is_available()
    except Exception:
        have = False
    lines += measure(a) if have else ["1. and 2.: not measured: no device"]
    finish_on_the_host(a.features, lines)
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)
    print(text, end="")


if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    main()
