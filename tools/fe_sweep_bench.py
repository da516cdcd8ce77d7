"""What the fixed-effect stage's sweep over l2_reg_weight costs (gdmix_amd/fe_model.py, csrc/fe_sweep.hip, gdmix_fe_restart), measured.

    PYTHONPATH=. python tools/fe_sweep_bench.py [rows] [K] [reps] > profiles/fe_sweep_bench.txt      (plus tools/kernel_resources.py --match fe_sweep)

On the shard bench.py's fixed-effect leg uses (rows x 32 uniform columns of 100 k features, logistic, m = 10, 20 iterations; 4 M rows =
128 M non-zeros) with a validation shard a quarter of its size:

  sweep     (a) one gdmix_fe_create, K x (gdmix_fe_restart + solve), one gdmix_fe_score_models — the stage with --l2_reg_weights;
  K plain   (b) K x (gdmix_fe_create + solve + gdmix_fe_score) — K plain runs of the stage, as before the flag existed.
Both on shards already in HBM ("device work"), and once more from the host arrays ("with upload and pack": fit_sweep against
K x (fit_stepping + device_score), which upload and pack the training shard and upload the validation shard K times).
The same card, alternating, medians of `reps` runs with [min, max]; a host clock around work that ends in a device synchronise.

  scoring   gdmix_fe_score_models at K = 1, 3, 5, 8 — from the slot-major copy and from the K arrays — against K calls of gdmix_fe_score.
            Bytes are the algorithm's: 12 B per non-zero (column + value) and 8 B per sample (row pointer) read once, 8 K B per sample written.
"""
import statistics
import sys
import time

import numpy as np

ROWS = int(sys.argv[1]) if len(sys.argv) > 1 else 4_000_000
K = int(sys.argv[2]) if len(sys.argv) > 2 else 5
REPS = int(sys.argv[3]) if len(sys.argv) > 3 else 3
NNZ, D, ITERS = 32, 100_000, 20
GRID = (100.0, 30.0, 10.0, 3.0, 1.0, 0.3, 0.1, 0.01)[:K]
HBM_PEAK = 8.0e12       # bytes/s, MI355X


def shard(rng, n):
    cols = rng.integers(0, D, n * NNZ, dtype=np.int64)
    vals = (rng.random(n * NNZ, dtype=np.float32) - 0.5) * 2.0
    y = (rng.random(n, dtype=np.float32) < 0.5).astype(np.float32)
    return np.arange(n + 1, dtype=np.int64) * NNZ, cols, vals, y, np.zeros(n, np.float32)


def alternating(fns, reps, warm=1):
    """{name: fn} -> {name: (median, min, max) ms}: every round calls each fn once, in order."""
    import torch
    for _ in range(warm):
        for fn in fns.values():
            fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in fns}
    for _ in range(reps):
        for k, fn in fns.items():
            t = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            ms[k].append((time.perf_counter() - t) * 1e3)
    return {k: (statistics.median(v), min(v), max(v)) for k, v in ms.items()}


def fmt(t):
    return f"{t[0]:10.2f} ms [{t[1]:.2f}, {t[2]:.2f}]"


def main():
    import dataclasses
    import torch
    from gdmix_amd import fixed_effect as fe
    from gdmix_amd.solver import REDeviceSolver, SolverOptions
    s = REDeviceSolver(0)
    f = fe.FixedEffectDeviceSolver(solver=s)
    rng = np.random.default_rng(0)
    rp, cols, vals, y, off = shard(rng, ROWS)
    vrp, vcols, vvals, vy, voff = shard(rng, ROWS // 4)
    print(f"training shard {ROWS} samples x {NNZ} uniform columns of {D} features ({ROWS * NNZ / 1e6:.0f} M non-zeros), validation shard {ROWS // 4} samples "
          f"({ROWS // 4 * NNZ / 1e6:.0f} M non-zeros); logistic, m = 10, {ITERS} iterations, K = {K} weights {list(GRID)}", flush=True)
    batch, _ = fe.shard_as_batch(rp, cols, vals, y, off, None, True)
    packed = s.pack(batch)
    vshard = f.upload(vrp, vcols, vvals, voff, D)
    opts = SolverOptions(l2=1.0, regularize_bias=True, has_intercept=True, m=10, max_iter=ITERS, threshold=0.0, sum_loss=True)
    kept = {}

    def solved(prob):
        fe.run_stepping_loop(prob)
        th = torch.empty(D + 1, dtype=torch.float64, device=s.device)
        prob._check(prob.lib.gdmix_fe_result(prob._h, th.data_ptr(), None, None, None, None, s._stream()), "gdmix_fe_result")
        return th

    def sweep_device():
        prob = fe._SteppingProblem(s, packed, D, dataclasses.replace(opts, l2=GRID[0]), None)
        thetas = []
        for w in GRID:
            prob.restart(dataclasses.replace(opts, l2=w), None)
            thetas.append(solved(prob))
        prob.close()
        kept["sweep"] = f.score_models(vshard, thetas, True, per_coord=True)

    def plain_device():
        rows = []
        for w in GRID:
            prob = fe._SteppingProblem(s, packed, D, dataclasses.replace(opts, l2=w), None)
            th = solved(prob)
            prob.close()
            rows.append(f.score_device(vshard, th, True))
        kept["plain"] = rows

    r = alternating({"sweep": sweep_device, "plain": plain_device}, REPS)
    sc, pc = kept["sweep"]
    for k in range(K):      # the thing measured is the thing specified
        a, b = kept["plain"][k]
        assert torch.equal(sc[k].view(torch.int32), a.view(torch.int32)) and torch.equal(pc[k].view(torch.int32), b.view(torch.int32))
    print("\ndevice work (shards in HBM, the training shard packed)")
    print(f"  (a) 1 create, {K} x (restart + solve), 1 score_models        {fmt(r['sweep'])}")
    print(f"  (b) {K} x (create + solve + gdmix_fe_score)                    {fmt(r['plain'])}   (a) is {r['sweep'][0] / r['plain'][0]:.2f} x (b)", flush=True)
    # the pieces
    prob = fe._SteppingProblem(s, packed, D, opts, None)
    pieces = alternating({"create": lambda: fe._SteppingProblem(s, packed, D, opts, None).close(),
                          "restart + solve": lambda: (prob.restart(opts, None), solved(prob))}, REPS)
    prob.close()
    for name, t in pieces.items():
        print(f"      {name:<22s} {fmt(t)}")
    del kept["sweep"], kept["plain"], sc, pc
    torch.cuda.empty_cache()

    def sweep_host():
        pick = lambda thetas: 0
        f.fit_sweep(rp, cols, vals, y, D, l2_grid=GRID, select=pick, offset=off, max_iter=ITERS, dummy=False)
        sh = f.upload(vrp, vcols, vvals, voff, D)
        f.score_models(sh, [np.zeros(D + 1)] * K, True, per_coord=True)

    def plain_host():
        for w in GRID:
            th, _ = f.fit_stepping(rp, cols, vals, y, D, offset=off, l2=w, max_iter=ITERS, dummy=False)
            fe.device_score(s, vrp, vcols, vvals, voff, th, D, True)

    r = alternating({"sweep": sweep_host, "plain": plain_host}, REPS, warm=0)
    print("\nwith upload and pack (from the host arrays, scores of (b) copied back as the stage does)")
    print(f"  (a) fit_sweep + upload + score_models                          {fmt(r['sweep'])}")
    print(f"  (b) {K} x (fit_stepping + device_score)                        {fmt(r['plain'])}   (a) is {r['sweep'][0] / r['plain'][0]:.2f} x (b)", flush=True)

    print("\nscoring the validation shard under K models")
    g = torch.Generator(device=s.device).manual_seed(1)
    thetas = [0.3 * torch.randn(D + 1, dtype=torch.float64, device=s.device, generator=g) for _ in range(8)]
    n, z = vshard.n, vshard.n * NNZ
    for kk in (1, 3, 5, 8):
        def base():
            for k in range(kk):
                f.score_device(vshard, thetas[k], True)
        r = alternating({"slot": lambda: f.score_models(vshard, thetas[:kk], True, per_coord=True, slot_major=True), "base": base,
                         "gather": lambda: f.score_models(vshard, thetas[:kk], True, per_coord=True, slot_major=False)}, max(REPS, 7), warm=2)
        nbytes = 12.0 * z + 12.0 * n + 8.0 * kk * n
        print(f"  K = {kk}: {kk} x gdmix_fe_score              {fmt(r['base'])}")
        for key, what in (("slot", "score_models, slot-major copy"), ("gather", "score_models, K arrays       ")):
            print(f"         {what}   {fmt(r[key])}   {r['base'][0] / r[key][0]:.2f} x the K calls; {nbytes / 1e6:.0f} MB needed, "
                  f"{100.0 * nbytes / (r[key][0] * 1e-3) / HBM_PEAK:.1f} % of the HBM peak", flush=True)
    s.close()


if __name__ == "__main__":
    main()
