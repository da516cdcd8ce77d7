"""What the random effect's trust-region Newton solve costs next to the plain solve (include/gdmix_re.h, "TRON"; csrc/re_tron.hip).

    python tools/re_tron_bench.py [--entities 1000000] [--steps 5] [--warmup 2] [--out profiles/re_tron.txt]

The C2-shaped batch of profiles/re_l1.txt, packed once, logistic loss, the stage's tolerances. In one process and in alternation: TRON
(solve_tron), the plain solve on the like-for-like LDS wavefront kernel (kernel mask 2: one wavefront per entity, block and state in LDS)
and the plain solve under default routing (the group kernels); torch events around the call, results left on the device. Reported for
each: ms per solve, evaluations and products per entity, ms per pass (solve ms / (nfev + nhv)). The yardstick is the plain wavefront
kernel's ms per evaluation in this same run, the parent's kernel: TRON's ms per pass may be at most BAR times it — a product does a
strict subset of an evaluation's work on the same staged block, and 1.05 is the margin the fixed effect's product was given against its
evaluation. Total time against the group kernels is reported, not barred. Also reported: the LDS per workgroup of the TRON wavefront
launches and of the plain wavefront kernel on this batch, and the wavefronts a CU of 160 KB holds of each. Without a device the output says
"not measured". What the output file holds from its first line of dashes on is kept as it is.

    python tools/re_tron_bench.py --rows [--parent DIR] [--out profiles/re_tron_rows.txt]

The row kernel (re_tron_rows_kernel: four entities per wavefront) on the same batch: in one process and in alternation, the TRON solve under
a row limit of 0 (the routing without that kernel), 6, 8 and 10 KB, and the plain solve under default routing for information. For each:
the median of the timed solves with [min, max], the share of entities on the row kernel, evaluations and products per entity, ms per pass.
--parent DIR names a tree that holds another build of the package (DIR/gdmix_amd with its library, e.g. the parent commit's): its TRON
solve, as that build routes it by default, is timed on the same batch by a child process right behind the others, on the same device in the
same session. --parent-label says in the output what that build is (the directory's name otherwise); both options may be given several times.

    python tools/re_tron_bench.py --pcg [--steps 7] [--out profiles/re_tron_pcg.txt]

The preconditioned solve (set_tron_preconditioner(0.01): "TRON_PCG") next to TRON on two batches in one process, the legs in alternation: the
C2-shaped batch, and the same batch with every global column's values multiplied by 10^u, u uniform in [-3, 3]. Legs: TRON as shipped
(default row limit), TRON under a row limit of 0 (the routing TRON_PCG has: it has no row kernel), TRON_PCG. For each: median [min, max] ms
per solve, evaluations, products (= CG steps: a step takes one product) per entity, CG steps per trust-region subproblem, ms per pass."""
import argparse
import os
import sys

import numpy as np

BAR = 1.05
CU_LDS = 160 * 1024
SMALL_LDS = 20 * 1024      # csrc/re_entity_scaffold.hpp, WAVE_SMALL_LDS


def footprints(batch, packed, m):
    """(TRON, plain wavefront kernel) LDS bytes per entity: csrc/re_entity_scaffold.hpp solver_lds_bytes, csrc/re_internal.hpp wave_lds_bytes."""
    n = np.diff(np.asarray(batch.ent_row_ptr))
    z = np.diff(packed.ent_nnz_ptr().cpu().numpy())
    d = np.diff(packed.ent_feat_ptr().cpu().numpy())
    p = d + 1
    w32 = 4 * z + (n + 1) + (d + 1) + 2 * n
    plain = (((5 + 2 * m) * p + n + 2 * m) * 8 + w32 * 4 + 15) & ~15
    tron = ((((5 * p + n) * 8 + w32 * 4 + 15) & ~15) + 8 * (2 * p + 2 * n) + 15) & ~15
    return tron, plain


def measure(E, steps, warmup):
    import torch
    from gdmix_amd import synthetic
    from gdmix_amd.solver import REDeviceSolver, SolverOptions
    D = 1024
    b = synthetic.make_survey_batch(E, 16, 4, D, seed=synthetic.C2_SEED)
    solver = REDeviceSolver(0)
    packed = solver.pack(b, has_intercept=True)
    opts = SolverOptions(l2=1.0, ftol=1e-12)
    lines = [f"C2-shaped synthetic batch (make_survey_batch({E}, 16, 4, {D}, seed=C2_SEED)): {packed.E} entities, {b.N} samples, {b.Z} non-zeros, {packed.P} coefficients",
             f"logistic, l2 = 1, stage tolerances (pgtol 1e-5, ftol 1e-12, max_iter 100, m 10), intercept regularised; median of {steps} timed solves after "
             f"{warmup} warm-up solves, the three solves in alternation", ""]
    kinds = {"TRON": None, "plain, LDS wavefront kernel (kernel mask 2)": 2, "plain, default routing (group kernels)": 7}
    ms, last = {k: [] for k in kinds}, {}
    counts = launches = None
    for step in range(warmup + steps):
        for k, mask in kinds.items():
            if mask is not None:
                solver.set_kernel_mask(mask)
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            res = solver.solve_tron(packed, opts) if mask is None else solver.solve(packed, opts)
            t1.record()
            torch.cuda.synchronize()
            solver.set_kernel_mask(7)
            if step >= warmup:
                ms[k].append(t0.elapsed_time(t1))
            last[k] = res
            if mask is None:
                cc = packed._view(packed.c.class_count, 5, torch.int32).cpu().numpy()
                counts, launches = (int(cc[0]), int(cc[1])), (int(cc[4]), int(cc[2]), int(cc[3]))
    per_pass = {}
    for k in kinds:
        r = last[k].to_host()
        med, nfev = float(np.median(ms[k])), float(r["nfev"].mean())
        nhv = float(r["nhv"].mean()) if r.get("nhv") is not None and k == "TRON" else 0.0
        per_pass[k] = med / (nfev + nhv)
        lines.append(f"{k}: {med:.3f} ms per solve (runs {', '.join(f'{x:.3f}' for x in ms[k])}); nit mean {r['nit'].mean():.2f}, evaluations per entity {nfev:.2f}, "
                     f"products per entity {nhv:.2f}; {per_pass[k]:.3f} ms per pass; status counts {np.bincount(r['status'], minlength=5).tolist()}")
    lines.append(f"TRON routing: {counts[0]} entities on re_tron_wave_kernel ({launches[0]} in the launch with {SMALL_LDS} B of LDS, {launches[1]} in the launch "
                 f"with {launches[2]} B), {counts[1]} on re_tron_block_kernel")
    names = list(kinds)
    ratio = per_pass[names[0]] / per_pass[names[1]]
    lines.append(f"TRON ms per pass / plain wavefront kernel ms per evaluation: {ratio:.3f} (bar: at most {BAR}) -> {'held' if ratio <= BAR else 'MISSED'}")
    lines.append(f"TRON ms per solve / plain default routing ms per solve: {np.median(ms[names[0]]) / np.median(ms[names[2]]):.2f} x (reported, not barred)")
    tron, plain = footprints(b, packed, opts.m)
    lines += ["", f"LDS footprint per entity, bytes: TRON mean {tron.mean():.0f}, median {np.median(tron):.0f}, max {tron.max()}; plain wavefront kernel (m = {opts.m}) mean "
              f"{plain.mean():.0f}, median {np.median(plain):.0f}, max {plain.max()}",
              f"LDS per one-wavefront workgroup as launched: TRON {SMALL_LDS} B for {launches[0]} entities ({CU_LDS // SMALL_LDS} resident wavefronts per CU of 160 KB)"
              + (f", {launches[2]} B for {launches[1]} ({CU_LDS // max(launches[2], 1)} per CU)" if launches[1] else "")
              + f"; the plain wavefront kernel launches its class with the batch's largest footprint, {plain.max()} B ({CU_LDS // int(plain.max())} per CU)",
              f"by footprint alone a CU of 160 KB would hold {CU_LDS // int(np.median(tron))} median TRON entities and {CU_LDS // int(np.median(plain))} median plain ones"]
    solver.close()
    return lines


ROW_LIMITS = (0, 6144, 8192, 10240)


def _c2(E):
    import torch      # noqa: F401
    from gdmix_amd import synthetic
    from gdmix_amd.solver import REDeviceSolver, SolverOptions
    b = synthetic.make_survey_batch(E, 16, 4, 1024, seed=synthetic.C2_SEED)
    solver = REDeviceSolver(0)
    return b, solver, solver.pack(b, has_intercept=True), SolverOptions(l2=1.0, ftol=1e-12)


def _timed(call):
    import torch
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    res = call()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1), res


def _spread(ms):
    return f"{np.median(ms):.3f} ms [{min(ms):.3f}, {max(ms):.3f}]"


def time_package_tron(E, steps, warmup):
    """The TRON solve of whichever package is first on sys.path, as that package routes it by default -> the timed runs in ms."""
    b, solver, packed, opts = _c2(E)
    ms = [_timed(lambda: solver.solve_tron(packed, opts))[0] for _ in range(warmup + steps)][warmup:]
    solver.close()
    return ms


def measure_rows(E, steps, warmup, parents):
    import json
    import subprocess
    b, solver, packed, opts = _c2(E)
    lines = [f"C2-shaped synthetic batch (make_survey_batch({E}, 16, 4, 1024, seed=C2_SEED)): {packed.E} entities, {b.N} samples, {b.Z} non-zeros, {packed.P} coefficients",
             f"logistic, l2 = 1, stage tolerances (pgtol 1e-5, ftol 1e-12, max_iter 100); median [min, max] of {steps} timed solves after {warmup} warm-up "
             f"solves, the settings in alternation in one process", ""]
    ms = {k: [] for k in ROW_LIMITS + ("plain",)}
    last, rows = {}, {}
    for step in range(warmup + steps):
        for k in ms:
            if k == "plain":
                t, res = _timed(lambda: solver.solve(packed, opts))
            else:
                solver.set_tron_row_lds_limit(k)
                t, res = _timed(lambda: solver.solve_tron(packed, opts))
                rows[k] = solver.tron_row_count(packed)
            if step >= warmup:
                ms[k].append(t)
            last[k] = res
    solver.set_tron_row_lds_limit(solver.TRON_ROW_LDS_DEFAULT)
    host = {k: last[k].to_host() for k in ROW_LIMITS}
    tron, _ = footprints(b, packed, opts.m)
    for k in ROW_LIMITS:
        r = host[k]
        nfev, nhv = float(r["nfev"].mean()), float(r["nhv"].mean())
        same = all(np.array_equal(r[f], host[0][f]) for f in ("nfev", "nhv", "nit", "status")) and r["theta"].tobytes() == host[0]["theta"].tobytes()
        fits = tron[tron <= k]
        lds = f"LDS per workgroup 4 x {int(fits.max())} = {4 * int(fits.max())} B: {CU_LDS // (4 * int(fits.max()))} wavefronts, {4 * (CU_LDS // (4 * int(fits.max())))} entities per CU by arithmetic" if k and fits.size else "no row launch"
        lines.append(f"TRON, row limit {k:5d} B: {_spread(ms[k])}; {rows[k]} of {packed.E} entities on the row kernel ({rows[k] / packed.E:.1%}); evaluations per entity "
                     f"{nfev:.2f}, products per entity {nhv:.2f}, {np.median(ms[k]) / (nfev + nhv):.3f} ms per pass; counts and theta "
                     f"{'equal to' if same else 'DIFFERENT from'} row limit 0's; {lds}")
    lines.append(f"plain solve, default routing (for information): {_spread(ms['plain'])}")
    d = solver.TRON_ROW_LDS_DEFAULT
    faster = max(ms[d]) < min(ms[0])
    lines.append(f"default row limit {d} B against row limit 0: {np.median(ms[0]) / np.median(ms[d]):.2f} x, [min, max] {'do not overlap: faster' if faster else 'OVERLAP or slower: bar missed'}; "
                 f"against the plain solve under default routing: {np.median(ms[d]) / np.median(ms['plain']):.2f} x its time (reported only)")
    solver.close()
    here = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    for parent, label in parents:
        cp = subprocess.run([sys.executable, os.path.abspath(__file__), "--rows-child", "--package-root", parent, "--entities", str(E), "--steps", str(steps),
                             "--warmup", str(warmup)], capture_output=True, text=True, cwd=here)
        if cp.returncode == 0:
            pm = json.loads(cp.stdout.strip().splitlines()[-1])
            def near(mine):      # do the two runs' [min, max] overlap?
                return "[min, max] overlap" if min(pm) <= max(mine) and min(mine) <= max(pm) else "[min, max] APART"
            lines.append(f"another build, {label}: its TRON solve under its default routing, a child process right behind: {_spread(pm)}; against row limit 0 "
                         f"here ({_spread(ms[0])}): {near(ms[0])}; against row limit {d} here ({_spread(ms[d])}): {near(ms[d])}")
        else:
            lines.append(f"another build, {label}: not measured, the child process failed: {cp.stderr[-300:]}")
    return lines


def measure_pcg(E, steps, warmup):
    import dataclasses
    b, solver, packed, opts = _c2(E)
    scale = (10.0 ** np.random.default_rng(5).uniform(-3.0, 3.0, 1024)).astype(np.float32)
    b2 = dataclasses.replace(b, val=(b.val * scale[b.col_global]).astype(np.float32))
    lines = [f"C2-shaped synthetic batch (make_survey_batch({E}, 16, 4, 1024, seed=C2_SEED)): {packed.E} entities, {b.N} samples, {b.Z} non-zeros, {packed.P} coefficients",
             f"logistic, l2 = 1, stage tolerances (pgtol 1e-5, ftol 1e-12, max_iter 100); median [min, max] of {steps} timed solves after {warmup} warm-up "
             f"solves, the legs in alternation in one process; a = {solver.TRON_PCG_A}", ""]
    legs = {"TRON, default row limit": (solver.TRON_ROW_LDS_DEFAULT, 0.0), "TRON, row limit 0": (0, 0.0), "TRON_PCG": (solver.TRON_ROW_LDS_DEFAULT, solver.TRON_PCG_A)}
    for what, batch in (("plain C2", b), ("C2 with its columns rescaled over 1e-3 .. 1e3 (10^u per global column, u uniform, seed 5)", b2)):
        pk = packed if batch is b else solver.pack(batch, has_intercept=True)
        ms, last = {k: [] for k in legs}, {}
        for step in range(warmup + steps):
            for k, (limit, a) in legs.items():
                solver.set_tron_row_lds_limit(limit)
                solver.set_tron_preconditioner(a)
                t, last[k] = _timed(lambda: solver.solve_tron(pk, opts))
                if step >= warmup:
                    ms[k].append(t)
        solver.set_tron_preconditioner(0.0)
        solver.set_tron_row_lds_limit(solver.TRON_ROW_LDS_DEFAULT)
        lines.append(f"{what}:")
        for k in legs:
            r = last[k].to_host()
            nfev, nhv = float(r["nfev"].mean()), float(r["nhv"].mean())
            lines.append(f"  {k}: {_spread(ms[k])}; evaluations per entity {nfev:.2f}, products (CG steps) per entity {nhv:.2f}, CG steps per subproblem "
                         f"{r['nhv'].sum() / max(r['nfev'].sum() - packed.E, 1):.2f}, {np.median(ms[k]) / (nfev + nhv):.3f} ms per pass; status counts "
                         f"{np.bincount(r['status'], minlength=5).tolist()}")
        m = {k: float(np.median(v)) for k, v in ms.items()}
        pp = lambda k: m[k] / float(last[k].to_host()["nfev"].mean() + last[k].to_host()["nhv"].mean())
        lines.append(f"  TRON_PCG ms per solve / TRON's: {m['TRON_PCG'] / m['TRON, default row limit']:.3f} (default row limit), {m['TRON_PCG'] / m['TRON, row limit 0']:.3f} (row limit 0); "
                     f"ms per pass / TRON's under row limit 0: {pp('TRON_PCG') / pp('TRON, row limit 0'):.3f}")
        if batch is b:
            tron, _ = footprints(b, packed, opts.m)
            n9 = tron + 16 * (np.diff(packed.ent_feat_ptr().cpu().numpy()) + 1)
            lines.append(f"  LDS footprint per entity at nine vectors, bytes: mean {n9.mean():.0f}, median {np.median(n9):.0f}, max {n9.max()} (seven: mean {tron.mean():.0f}, max "
                         f"{tron.max()}); {int((n9 <= SMALL_LDS).sum())} of {packed.E} within the {SMALL_LDS} B launch: {CU_LDS // SMALL_LDS} resident wavefronts per CU of "
                         f"160 KB there — arithmetic on the launch's LDS size, not a measurement")
        lines.append("")
    solver.close()
    return lines


def main():
    here = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    if "--package-root" in sys.argv:      # (before the package is imported: another build's tree in this one's place)
        here = os.path.abspath(sys.argv[sys.argv.index("--package-root") + 1])
    sys.path.insert(0, here)
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", action="store_true", help="the row kernel's measurements (profiles/re_tron_rows.txt)")
    ap.add_argument("--parent", action="append", default=[], help="with --rows: a tree with another build of the package, timed by a child process")
    ap.add_argument("--parent-label", action="append", default=[], help="what the output calls that build (default: the directory's name)")
    ap.add_argument("--pcg", action="store_true", help="TRON_PCG next to TRON on C2 and on C2 with rescaled columns (profiles/re_tron_pcg.txt)")
    ap.add_argument("--rows-child", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--package-root", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--entities", type=int, default=1_000_000)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(here, "profiles", "re_tron.txt"))
    a = ap.parse_args()
    if a.rows_child:
        import json
        print(json.dumps(time_package_tron(a.entities, a.steps, a.warmup)))
        return
    if a.rows and a.out.endswith("re_tron.txt"):
        a.out = os.path.join(os.path.dirname(a.out), "re_tron_rows.txt")
    head = ["Random effect, trust-region Newton per entity (gdmix_re_solve_tron) next to the plain solve (gdmix_re_solve): 1 x MI355X, torch events around "
            "REDeviceSolver.solve_tron / solve, results left on the device."]
    try:
        import torch
        have = torch.cuda.is_available()
    except Exception:
        have = False
    if a.pcg:
        if a.out.endswith("re_tron.txt"):
            a.out = os.path.join(os.path.dirname(a.out), "re_tron_pcg.txt")
        head = ["Random effect, TRON with diagonally preconditioned CG (TRON_PCG: gdmix_re_set_tron_preconditioner) next to TRON: 1 x MI355X, torch events around "
                "REDeviceSolver.solve_tron, results left on the device."]
        lines = head + (measure_pcg(a.entities, a.steps, a.warmup) if have else ["not measured: no device"])
    elif a.rows:
        labels = a.parent_label + [os.path.basename(os.path.normpath(d)) for d in a.parent[len(a.parent_label):]]
        parents = list(zip(a.parent, labels))
        head = ["Random effect, TRON with four entities per wavefront (re_tron_rows_kernel) next to the one-entity wavefront kernel: 1 x MI355X, torch events "
                "around REDeviceSolver.solve_tron, results left on the device."]
        lines = head + (measure_rows(a.entities, a.steps, a.warmup, parents) if have else ["not measured: no device"])
    else:
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
