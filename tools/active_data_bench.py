"""--active_data_upper_bound on a C5-shaped Zipf batch against the stage without the flag, in one process on one device: what the cap pass
costs, by path, what the solver's batch shrinks to, and what the single-workgroup radix select takes on the largest entity alone.

    python tools/active_data_bench.py [--entities 1000000] [--max-nnz 4194304] [--steps 5] [--warmup 2] [--out profiles/active_data.txt]

The batch is synthetic.make_c5_share_device's (nnz per entity Zipf-like, P(nnz >= x) ~ x^-1.2, mean 256, eight non-zeros a row)
with the truncation raised to --max-nnz, so that the head entity has a few hundred thousand rows. A step without the flag is pack + solve
of the whole batch. With it, for K in {100, 1000, 10000}: the cap pass (gdmix_re_cap_plan + _apply; with the counting path at its default
limit, and with every capped entity on the radix select), then pack + solve of the capped batch. The pass is reported as a multiple of
gdmix_re_pack of the uncapped batch. Last, the pass at K = 10 and 100 for every limit of the counting path: why the default is what it is. The head entity alone (a batch of one entity): gdmix_re_cap_plan at K, and at K = n_e, where
no entity kernel runs; the difference is the one workgroup's radix select. HIP events on the solver's stream after a warm-up, medians, ms;
the plan synchronises once (its counts), which the events include. No threshold is asserted here.
"""
import argparse
import ctypes as C
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gdmix_amd import build, synthetic      # noqa: E402
from gdmix_amd import solver as S           # noqa: E402
from gdmix_amd.solver import REDeviceSolver, SolverOptions      # noqa: E402

BOUNDS = (100, 1000, 10000)
SEED = 20240603


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    b.synchronize()
    return out, a.elapsed_time(b)


def lone_entity(raw, n):
    """The largest entity as a batch of its own (views of the batch's arrays; the row pointers rebased)."""
    e = int(np.argmax(n))
    r0 = int(np.concatenate([[0], np.cumsum(n)])[e])
    rows = int(n[e])
    rp = raw["row_nnz_ptr"][r0:r0 + rows + 1]
    z0, z1 = int(rp[0]), int(rp[-1])
    dev = raw["y"].device
    return dict(E=1, N=rows, Z=z1 - z0, ent_row_ptr=torch.tensor([0, rows], dtype=torch.int64, device=dev), row_nnz_ptr=(rp - z0).contiguous(),
                col_global=raw["col_global"][z0:z1], val=raw["val"][z0:z1], y=raw["y"][r0:r0 + rows], offset=raw["offset"][r0:r0 + rows], weight=None), r0


def plan_only(s, raw, uid, K):
    """gdmix_re_cap_plan alone on a raw device batch -> its counts."""
    ptr = lambda x: None if x is None or x.numel() == 0 else x.data_ptr()
    c_raw = S._RawBatch(raw["E"], raw["N"], raw["Z"], raw["ent_row_ptr"].data_ptr(), raw["row_nnz_ptr"].data_ptr(), ptr(raw["col_global"]), ptr(raw["val"]),
                        ptr(raw["y"]), ptr(raw["offset"]), ptr(raw["weight"]))
    nbytes = int(s.lib.gdmix_re_cap_workspace_bytes(raw["E"], raw["N"]))
    ws = torch.empty(nbytes, dtype=torch.uint8, device=s.device)
    counts = S._CapCounts()
    S._check(s.lib.gdmix_re_cap_plan(s._h, C.byref(c_raw), uid.data_ptr(), C.byref(S._CapOpts(int(K), SEED)), ws.data_ptr(), nbytes, C.byref(counts), s._stream()),
             "gdmix_re_cap_plan")
    return counts


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--entities", type=int, default=1_000_000)
    ap.add_argument("--max-nnz", type=int, default=1 << 22)
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
    say(f"steps {a.steps} after {a.warmup} warm-up; logistic loss, l2 1, m 10, max_iter 100, ftol 1e-12, unregularised intercept; HIP events, medians, ms")
    opts = SolverOptions(l2=1.0, regularize_bias=False, has_intercept=True, m=10, max_iter=100, ftol=1e-12)
    raw, n = synthetic.make_c5_share_device(s.device, a.entities, max_nnz=a.max_nnz)
    N = raw["N"]
    uid = torch.arange(N, dtype=torch.int64, device=s.device) * 0x9E3779B1 - 7_000_000_000
    say(f"c5 share: {raw['E']} entities, {N} rows, {raw['Z']} non-zeros; largest entity {int(n.max())} rows, {int((n > 1024).sum())} entities above 1024 rows")
    med = lambda rows: np.median(np.array(rows), axis=0)
    plain = []
    for step in range(a.warmup + a.steps):
        packed, t_pack = timed(lambda: s.pack(raw, has_intercept=True))
        res, t_solve = timed(lambda: s.solve(packed, opts))
        if step >= a.warmup:
            plain.append((t_pack, t_solve))
        del res, packed
    p = med(plain)
    say(f"without the flag (same process): pack {p[0]:.3f} + solve {p[1]:.3f} = {p.sum():.3f} ms per step")
    one, _ = lone_entity(raw, n)
    r0 = int(np.concatenate([[0], np.cumsum(n)])[int(np.argmax(n))])
    one_uid = uid[r0:r0 + one["N"]].contiguous()
    for K in BOUNDS:
        rows = []
        counts = None
        for step in range(a.warmup + a.steps):
            (capped, counts), t_cap = timed(lambda: s.cap_samples(raw, uid, K, seed=SEED))
            s.set_cap_small_max(0)
            try:
                (other, _), t_radix = timed(lambda: s.cap_samples(raw, uid, K, seed=SEED))
            finally:
                s.set_cap_small_max(s.CAP_SMALL_MAX_DEFAULT)
            del other
            packed, t_pack = timed(lambda: s.pack(capped, has_intercept=True))
            res, t_solve = timed(lambda: s.solve(packed, opts))
            _, t_one = timed(lambda: plan_only(s, one, one_uid, K))
            _, t_base = timed(lambda: plan_only(s, one, one_uid, one["N"]))
            if step >= a.warmup:
                rows.append((t_cap, t_radix, t_pack, t_solve, t_one, t_base))
            del res, packed, capped
        f = med(rows)
        say(f"K = {K}: {counts['capped']} of {counts['entities']} entities capped, {counts['kept']} of {counts['rows']} rows kept ({counts['kept_nnz']} non-zeros)")
        say(f"  cap pass (plan + apply): {f[0]:.3f} ms with the counting path up to {s.CAP_SMALL_MAX_DEFAULT} rows (the default), {f[1]:.3f} ms with every capped "
            "entity on the radix select" + ("" if K < s.CAP_SMALL_MAX_DEFAULT else f" (at this K every capped entity is above {s.CAP_SMALL_MAX_DEFAULT} rows: one path)"))
        say(f"  cap pass / gdmix_re_pack of the uncapped batch: {f[0] / p[0]:.3f}")
        say(f"  capped batch: pack {f[2]:.3f} + solve {f[3]:.3f} = {f[2] + f[3]:.3f} ms; cap + pack + solve {f[0] + f[2] + f[3]:.3f} ms against {p.sum():.3f} ms without the flag "
            f"({(f[0] + f[2] + f[3]) / p.sum():.3f})")
        say(f"  head entity alone ({one['N']} rows, one workgroup): plan {f[4]:.3f} ms, plan without an entity kernel (K = n_e) {f[5]:.3f} ms, "
            f"radix select {f[4] - f[5]:.3f} ms = {(f[4] - f[5]) / f[0]:.2f} of the whole batch's cap pass")
    # where the two paths part (gdmix_re_set_cap_small_max): the evidence for the default
    for K in (10, 100):
        parts = []
        for limit in (0, 32, 64, 128, 256, 512, 1024):
            s.set_cap_small_max(limit)
            try:
                ts = []
                for step in range(a.warmup + a.steps):
                    (out, _), t = timed(lambda: s.cap_samples(raw, uid, K, seed=SEED))
                    del out
                    if step >= a.warmup:
                        ts.append(t)
            finally:
                s.set_cap_small_max(s.CAP_SMALL_MAX_DEFAULT)
            parts.append(f"{limit}: {np.median(ts):.3f}")
        say(f"cap pass at K = {K} by the limit of the counting path (rows: ms): " + "; ".join(parts))
    s.close()
    if a.out:
        with open(a.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    sys.exit(main())
