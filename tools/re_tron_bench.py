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
"not measured". What the output file holds from its first line of dashes on is kept as it is."""
import argparse
import os
import sys

import numpy as np

BAR = 1.05
CU_LDS = 160 * 1024
SMALL_LDS = 20 * 1024      # csrc/re_tron.hip, TRON_SMALL_LDS (and csrc/re_owlqn.hip, OWL_SMALL_LDS)


def footprints(batch, packed, m):
    """(TRON, plain wavefront kernel) LDS bytes per entity: csrc/re_tron.hip tron_lds_bytes, csrc/re_internal.hpp wave_lds_bytes."""
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


def main():
    here = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, here)
    ap = argparse.ArgumentParser()
    ap.add_argument("--entities", type=int, default=1_000_000)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(here, "profiles", "re_tron.txt"))
    a = ap.parse_args()
    head = ["Random effect, trust-region Newton per entity (gdmix_re_solve_tron) next to the plain solve (gdmix_re_solve): 1 x MI355X, torch events around "
            "REDeviceSolver.solve_tron / solve, results left on the device."]
    try:
        import torch
        have = torch.cuda.is_available()
    except Exception:
        have = False
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
