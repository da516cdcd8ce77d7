"""What down-sampling the fixed effect's training shard costs and buys, on the shard shape of bench.py's fixed-effect leg.

    python tools/fe_downsample_bench.py [--rows 4000000] [--rate 0.1] [--positives 0.02] [--repeats 7]

The shard: rows x 32 uniform columns of 100 k features (bench.py: fixed_effect_leg), labels 2 % positive, logistic loss (every positive is
kept). One process, one JSON line:
  * milliseconds of gdmix_re_downsample_plan + gdmix_re_downsample_apply (REDeviceSolver.downsample: the output arrays' allocation and the
    plan's one synchronisation included) next to the milliseconds of gdmix_re_pack of the FULL shard, alternating, after two warm-up rounds;
    median and minimum over the repeats;
  * the two calls on buffers allocated beforehand, each after two warm-up calls, median and minimum over the repeats: the plan under a
    host clock (it ends in its own synchronisation), the apply pass under device events; their sum next to the pack is the comparison
    that does not depend on the state of torch's caching allocator (the pack's own figure includes its workspace allocation);
  * the bytes the apply pass has to move over its time as a share of the HBM peak: per kept non-zero 12 B read + 12 B written; per kept
    row 20 B of pointers read by the copy, 20 B read and 28 B written by the row pass; per input row 5 B (keep flag, row scan);
  * gdmix_fe_last_eval_ms (rows pass + columns pass) and the wall time per evaluation of a 20-iteration fit of the down-sampled problem
    against the full problem, next to the ratio of their non-zeros.
Not a gate: the figures go into DESIGN.md by hand."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

HBM_PEAK_GBS = 8000.0   # MI355X HBM3E spec peak (bench.py)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=4_000_000)
    ap.add_argument("--nnz-per-row", type=int, default=32)
    ap.add_argument("--features", type=int, default=100_000)
    ap.add_argument("--rate", type=float, default=0.1)
    ap.add_argument("--positives", type=float, default=0.02)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--iters", type=int, default=20)
    a = ap.parse_args()
    import torch
    from gdmix_amd import fixed_effect as fe
    from gdmix_amd import solver as S
    solver = S.REDeviceSolver(0)
    rng = np.random.default_rng(0)
    n, k, D = a.rows, a.nnz_per_row, a.features
    cols = rng.integers(0, D, n * k, dtype=np.int64)
    vals = (rng.random(n * k, dtype=np.float32) - 0.5) * 2.0
    y = (rng.random(n, dtype=np.float32) < a.positives).astype(np.float32)
    uid = np.arange(n, dtype=np.int64) + 1000
    batch, _ = fe.shard_as_batch(np.arange(n + 1, dtype=np.int64) * k, cols, vals, y, np.zeros(n, np.float32), None, True)
    rd = solver.upload(batch)
    uid_dev = torch.from_numpy(uid).to(solver.device)
    sync = torch.cuda.synchronize

    def timed(fn):
        sync()
        t0 = time.perf_counter()
        out = fn()
        sync()
        return (time.perf_counter() - t0) * 1e3, out

    ds_ms, pack_ms, sample, counts = [], [], None, None
    for r in range(2 + a.repeats):      # alternating; the first two rounds warm both up
        ms, (sample, counts) = timed(lambda: solver.downsample(rd, uid_dev, a.rate, a.seed, negatives_only=True))
        ms_p, packed_full = timed(lambda: solver.pack(rd))
        if r >= 2:
            ds_ms.append(ms)
            pack_ms.append(ms_p)
        if r < 1 + a.repeats:
            del packed_full
    # the apply pass alone: the same workspace planned once, device events around the call
    E, N, Z = 1, n, n * k
    ptr = lambda x: None if x is None or x.numel() == 0 else x.data_ptr()
    c_raw = S._RawBatch(E, N, Z, rd["ent_row_ptr"].data_ptr(), rd["row_nnz_ptr"].data_ptr(), ptr(rd["col_global"]), ptr(rd["val"]), ptr(rd["y"]),
                        ptr(rd["offset"]), ptr(rd["weight"]))
    c_opts = S._DownsampleOpts(a.rate, a.seed, 1, 0)
    nbytes = int(solver.lib.gdmix_re_downsample_workspace_bytes(E, N))
    ws = torch.empty(nbytes, dtype=torch.uint8, device=solver.device)
    c_counts = S._DownsampleCounts()
    st = solver._stream()
    plan_ms = []      # (the plan ends in its own synchronisation: a host clock around it, buffers allocated beforehand)
    for r in range(2 + a.repeats):
        ms, _ = timed(lambda: S._check(solver.lib.gdmix_re_downsample_plan(solver._h, C.byref(c_raw), uid_dev.data_ptr(), C.byref(c_opts), ws.data_ptr(), nbytes,
                                                                            C.byref(c_counts), st), "plan"))
        if r >= 2:
            plan_ms.append(ms)
    n_out, z_out = int(c_counts.kept), int(c_counts.kept_nnz)
    c_out = S._DownsampleOut(n_out, z_out, sample["ent_row_ptr"].data_ptr(), sample["row_nnz_ptr"].data_ptr(), ptr(sample["col_global"]), ptr(sample["val"]),
                             ptr(sample["y"]), ptr(sample["offset"]), ptr(sample["weight"]))
    apply_ms = []
    for r in range(2 + a.repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        S._check(solver.lib.gdmix_re_downsample_apply(solver._h, C.byref(c_raw), C.byref(c_opts), ws.data_ptr(), nbytes, C.byref(c_out),
                                                      ptr(sample["kept_rows"]), st), "apply")
        e1.record()
        sync()
        if r >= 2:
            apply_ms.append(e0.elapsed_time(e1))
    apply_bytes = 24.0 * z_out + 68.0 * n_out + 5.0 * N
    # an evaluation of the down-sampled problem against the full one
    opts = S.SolverOptions(l2=1.0, regularize_bias=True, has_intercept=True, m=10, max_iter=a.iters, threshold=0.0, sum_loss=True)
    evals = {}
    for name, packed in (("full", packed_full), ("sampled", solver.pack(sample))):
        for _ in range(2):      # the second fit is the measured one
            prob = fe._SteppingProblem(solver, packed, D, opts, None)
            sync()
            t0 = time.perf_counter()
            fe.run_stepping_loop(prob)
            sync()
            dt = time.perf_counter() - t0
            _, info = prob.result()
            rows_ms, cols_ms = prob.last_eval_ms()
            prob.close()
        evals[name] = {"non_zeros": int(packed.Z), "rows": int(packed.N), "evaluations": int(info["nfev"]), "last_eval_ms": rows_ms + cols_ms,
                       "rows_pass_ms": rows_ms, "cols_pass_ms": cols_ms, "wall_ms_per_evaluation": dt * 1e3 / int(info["nfev"])}
    med, lo = statistics.median, min
    out = {"shard": f"{n} rows x {k} uniform columns of {D} features, {a.positives:.0%} positives, rate {a.rate}, logistic", "counts": counts,
           "device": torch.cuda.get_device_name(0), "repeats": a.repeats,
           "downsample_ms": {"median": med(ds_ms), "min": lo(ds_ms)}, "pack_full_ms": {"median": med(pack_ms), "min": lo(pack_ms)},
           "downsample_over_pack": med(ds_ms) / med(pack_ms), "plan_ms": {"median": med(plan_ms), "min": lo(plan_ms)},
           "plan_plus_apply_ms": med(plan_ms) + med(apply_ms), "plan_plus_apply_over_pack": (med(plan_ms) + med(apply_ms)) / med(pack_ms),
           "apply_ms": {"median": med(apply_ms), "min": lo(apply_ms)}, "apply_bytes": apply_bytes,
           "apply_GBps": apply_bytes / (med(apply_ms) * 1e-3) / 1e9, "apply_frac_of_hbm_peak": apply_bytes / (med(apply_ms) * 1e-3) / 1e9 / HBM_PEAK_GBS,
           "evaluation": evals, "non_zeros_ratio": evals["sampled"]["non_zeros"] / evals["full"]["non_zeros"],
           "last_eval_ms_ratio": evals["sampled"]["last_eval_ms"] / evals["full"]["last_eval_ms"],
           "wall_ms_per_evaluation_ratio": evals["sampled"]["wall_ms_per_evaluation"] / evals["full"]["wall_ms_per_evaluation"]}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
