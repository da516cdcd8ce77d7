#!/usr/bin/env python3
"""What the resident coordinate descent costs on one MI355X (gdmix_amd/descent.py), next to the file chain on the same data.

    PYTHONPATH=. python tools/descent_bench.py [--passes 4] [--repeat 3] [--group-scale 64] [--no-chain] [--group-only]

Data: chain.make_dataset() at its default 100 k ratings. Reported, each from a host clock around work that ends in a device synchronise:
  * set-up per coordinate (upload + group + pack; a fixed effect: pack + gdmix_fe_create), per pass and per update, for `--passes`
    passes; run `--repeat` times after one warm-up run, every run listed;
  * the grouping alone (gdmix_re_group_rows) on the per-user bag tiled `--group-scale` times, so that the copy of the non-zeros moves
    enough bytes to be timed: the whole call by HIP events, and the bytes its copy kernel moves (24 B read + 24 B written per non-zero:
    int64 column + float value, and the row pointers). The copy kernel's own time comes from a kernel trace of `--group-only`
    (ds_nnz_kernel), taken in a run of its own;
  * chain.run_chain in process on the same data (unless --no-chain): the stages' files and the host partition steps.
No ratio is promised: the tool prints what it measured.
"""
import json
import sys
import tempfile
import time

import numpy as np

from gdmix_amd import chain

HBM_PEAK = 8.0e12      # bytes / s, MI355X


def arg(name, default):
    return type(default)(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


def group_alone(solver, data, scale, repeat):
    t = solver.torch
    tr = np.flatnonzero(data["train"])
    ptr, col, val, _ = chain.bag_rows(data, "per_user", tr)
    k = np.tile(np.diff(ptr), scale)
    ptr_s = np.concatenate([[0], np.cumsum(k)]).astype(np.int64)
    ids, inv = np.unique(data["user"][tr], return_inverse=True)
    idx = np.tile(inv, scale).astype(np.int32)
    up = lambda a: t.from_numpy(np.ascontiguousarray(a)).to(solver.device)
    d = (up(ptr_s), up(np.tile(col, scale)), up(np.tile(val, scale)), up(idx))
    times = []
    for _ in range(repeat + 1):
        a, b = t.cuda.Event(enable_timing=True), t.cuda.Event(enable_timing=True)
        a.record()
        g, counts = solver.group_rows(*d, ids.size)
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b) * 1e-3)
    z, n = counts["grouped_nnz"], counts["grouped"]
    moved = 2 * z * 12 + 2 * (n + 1) * 8 + n * 4      # non-zeros in and out, both row-pointer arrays, the row map
    return dict(rows=n, nnz=z, entities=counts["entities"], copy_bytes=moved, call_s=times[1:], first_call_s=times[0],
                copy_s_at_hbm_peak=moved / HBM_PEAK)


def main():
    passes, repeat, scale = arg("--passes", 4), arg("--repeat", 3), arg("--group-scale", 64)
    from gdmix_amd.solver import REDeviceSolver
    solver = REDeviceSolver(0)
    t = solver.torch
    data = chain.make_dataset()
    print(f"device: {t.cuda.get_device_name(0)}; data: chain.make_dataset() = {data['n']} ratings, {int(data['train'].sum())} training samples, "
          f"{chain.USERS} users x {chain.MOVIES} movies", flush=True)
    g = group_alone(solver, data, scale, repeat)
    print(f"grouping alone, per-user bag x {scale}: {g['rows']} rows, {g['nnz']} non-zeros, {g['entities']} entities; the copy moves {g['copy_bytes']} B "
          f"(= {g['copy_s_at_hbm_peak'] * 1e6:.1f} us at the 8 TB/s peak); gdmix_re_group_rows, whole call (sort, scans, one synchronise, copy): "
          f"{' '.join(f'{s * 1e3:.3f}' for s in g['call_s'])} ms (first call {g['first_call_s'] * 1e3:.3f} ms)", flush=True)
    if "--group-only" in sys.argv:
        return
    runs = []
    for rep in range(repeat + 1):
        t0 = time.perf_counter()
        res = chain.run_resident(data, passes=passes, solver=solver)
        total = time.perf_counter() - t0
        C = len(chain.STAGES)
        line = dict(total_s=total, setup_s=res.setup_s, pass_s=res.pass_s, update_s=[res.update_s[p * C:(p + 1) * C] for p in range(passes)],
                    validation=[e[f"validation_{res.metric}"] for e in res.history][C - 1::C])
        runs.append(line)
        print(("warm-up run " if rep == 0 else f"run {rep} ") + json.dumps(line), flush=True)
    if "--no-chain" not in sys.argv:
        for rep in range(2):
            with tempfile.TemporaryDirectory() as d:
                r = chain.run_chain(d, data)
            stages = " ".join("%.3f" % r[s]["s"] for s in chain.STAGES)
            parts = " ".join("%.3f" % r[s]["partition_s"] for s in chain.STAGES)
            print(("warm-up " if rep == 0 else "") + f"chain.run_chain in process: {r['total_s']:.3f} s; stages {stages} s, partition steps {parts} s; "
                  f"validation AUC {r['per_movie']['validation_auc']:.4f}", flush=True)
    solver.close()


if __name__ == "__main__":
    main()
