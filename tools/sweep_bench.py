"""What the sweep over l2_reg_weight costs (gdmix_amd/sweep.py, csrc/re_sweep.hip), measured three ways.

    PYTHONPATH=. python tools/sweep_bench.py [kernels|cli|all] [entities] [reps] > profiles/sweep_bench.txt

kernels   gdmix_re_score_models at K = 1, 4, 8 (gathered from the K arrays, and from the slot-major copy) against K calls of
          gdmix_re_score with pre-mapped coefficients — the kernel every stage scores with — and gdmix_re_join_features, on a C2-shaped
          pair (`entities` training entities, 16 samples each, the evaluation batch a re-draw with 10 % new entities) and on a Zipf pair of
          200 k entities. Warm; medians of `reps` calls with [min, max]; both sides alternate in one process; a host clock around calls
          that end in a device synchronise. Bytes are the algorithm's: 8 B per non-zero and 8 B per sample read once, 8 B of coef_pos
          per slot, 8 K B per coefficient the models have, 8 K B per sample written (logit and per-coordinate, fp32 each).
cli       `entities` C2 entities in 8 partitions with validation data through the CLI: the sweep at K = 8 against one plain run and against
          eight plain runs (the only way to sweep without the flag), wall time each, every run into a fresh output directory.
"""
import json
import os
import shutil
import statistics
import sys
import tempfile
import time

import numpy as np

from gdmix_amd import synthetic

WHAT = sys.argv[1] if len(sys.argv) > 1 else "all"
E = int(sys.argv[2]) if len(sys.argv) > 2 else 1_000_000
REPS = int(sys.argv[3]) if len(sys.argv) > 3 else 12
HBM_PEAK = 8.0e12       # bytes/s, MI355X
GRID8 = (100.0, 30.0, 10.0, 3.0, 1.0, 0.3, 0.1, 0.01)


def alternating(fns, reps=REPS, warm=2):
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
    return f"{t[0]:9.3f} ms [{t[1]:.3f}, {t[2]:.3f}]"


def zipf_batch(seed, E, id_base):
    b = synthetic.make_batch(E, 32, 8, 65536, seed=seed, size_dist="zipf", with_uid=False, entity_id_base=id_base)
    return b


def kernels():
    import torch
    from gdmix_amd import sweep
    from gdmix_amd.solver import REDeviceSolver
    s = REDeviceSolver(0)
    pairs = (("C2", synthetic.make_batch(E, 16, 4, 1024, seed=synthetic.C2_SEED, with_uid=False),
              synthetic.make_batch(E, 16, 4, 1024, seed=synthetic.C2_SEED + 1, with_uid=False, entity_id_base=E // 10)),
             ("Zipf-200k", zipf_batch(synthetic.C5_SEED, 200_000, 0), zipf_batch(synthetic.C5_SEED + 1, 200_000, 20_000)))
    for name, train, ev in pairs:
        tp = s.pack(s.upload(train))
        vp = s.pack(s.upload(ev))
        te = sweep.train_entity_map(ev.entity_ids, train.entity_ids)
        te_dev = torch.from_numpy(te).to(s.device)
        pos, has = s.join_features(vp, tp, te_dev)
        mapped_slots = int((pos >= 0).sum())
        print(f"\n{name}: training batch {tp.E} entities / {tp.P} coefficients, evaluation batch {vp.E} entities, {vp.N} samples, {vp.Z} non-zeros, "
              f"{vp.P} slots of which {mapped_slots} have a coefficient ({int(has.sum())} entities with a model)", flush=True)
        g = torch.Generator(device=s.device).manual_seed(1)
        thetas = [0.3 * torch.randn(tp.P, dtype=torch.float64, device=s.device, generator=g) for _ in range(8)]
        mapped = [torch.where(pos >= 0, th[pos.clamp(min=0)], torch.zeros((), dtype=torch.float64, device=s.device)) for th in thetas]
        join_bytes = 4.0 * vp.D + 8.0 * vp.P + 9.0 * vp.E
        t = alternating({"join": lambda: s.join_features(vp, tp, te_dev)})["join"]
        print(f"  gdmix_re_join_features                       {fmt(t)}   {join_bytes / 1e6:.0f} MB read + written besides the probes, {join_bytes / t[0] / 1e6:.0f} GB/s")
        for K in (1, 4, 8):
            def base():
                for k in range(K):
                    s.score(vp, mapped[k], has)
            r = alternating({"gather": lambda: s.score_models(vp, thetas[:K], pos, has), "base": base,
                             "slot": lambda: s.score_models(vp, thetas[:K], pos, has, slot_major=True)})
            nbytes = 8.0 * vp.Z + 8.0 * vp.N + 8.0 * vp.P + 8.0 * K * mapped_slots + 8.0 * K * vp.N
            for key, what in (("base", f"{K} x gdmix_re_score, pre-mapped coefficients"), ("gather", f"gdmix_re_score_models K = {K}, K arrays"),
                              ("slot", f"gdmix_re_score_models K = {K}, slot-major copy")):
                extra = "" if key == "base" else (f"   {r['base'][0] / r[key][0]:.2f} x the K calls; {nbytes / 1e6:.0f} MB needed, "
                                                  f"{100.0 * nbytes / (r[key][0] * 1e-3) / HBM_PEAK:.1f} % of the HBM peak")
                print(f"  {what:<46s} {fmt(r[key])}{extra}", flush=True)
            lo, pc = s.score_models(vp, thetas[:K], pos, has)
            for k in range(K):      # the thing measured is the thing specified
                a, b = s.score(vp, mapped[k], has)
                assert torch.equal(lo[k].view(torch.int32), a.view(torch.int32)) and torch.equal(pc[k].view(torch.int32), b.view(torch.int32))
        del tp, vp, thetas, mapped
    s.close()


def cli():
    from gdmix_amd import gdmix as cli_mod
    from gdmix_amd.io.grouped_reader import write_grouped_partition
    parts = 8
    md = {"features": [{"name": "bag", "dtype": "float", "shape": [1024], "isSparse": True}, {"name": "offset", "dtype": "float", "shape": [], "isSparse": False},
                       {"name": "uid", "dtype": "long", "shape": [], "isSparse": False}, {"name": "ent", "dtype": "string", "shape": [], "isSparse": False}],
          "labels": [{"name": "response", "dtype": "int", "shape": [], "isSparse": False}]}
    with tempfile.TemporaryDirectory() as d:
        train = synthetic.make_batch(E, 16, 4, 1024, seed=1)
        valid = synthetic.make_batch(E, 4, 4, 1024, seed=2)        # the same entity ids, a quarter of the samples
        per = (E + parts - 1) // parts
        for k in range(parts):
            rows = np.arange(k * per, min(E, (k + 1) * per))
            write_grouped_partition(os.path.join(d, "train", "active", f"partitionId={k}", "part-0.tfrecord"), train.select(rows), "ent", "bag", weight_column_name=None)
            write_grouped_partition(os.path.join(d, "valid", f"partitionId={k}", "part-0.tfrecord"), valid.select(rows), "ent", "bag", weight_column_name=None)
        json.dump(md, open(os.path.join(d, "meta.json"), "w"))
        with open(os.path.join(d, "features.csv"), "w") as f:
            f.write("".join(f"f{i},\n" for i in range(1024)))
        open(os.path.join(d, "plist.txt"), "w").write(",".join(str(k) for k in range(parts)))
        print(f"\nCLI: {E} C2 entities, {train.N} training and {valid.N} validation samples in {parts} partitions", flush=True)

        def run(out, extra):
            argv = ["gdmix", "--stage=random_effect", "--model_type=logistic_regression", "--uid_column_name=uid", "--label_column_name=response",
                    "--prediction_score_column_name=predictionScore", f"--partition_list_file={d}/plist.txt", f"--training_data_dir={d}/train",
                    f"--validation_data_dir={d}/valid", f"--metadata_file={d}/meta.json", f"--output_model_dir={out}/models", "--feature_bag=bag",
                    f"--feature_file={d}/features.csv", "--partition_entity=ent", "--regularize_bias=False", f"--training_score_dir={out}/ts",
                    f"--validation_score_dir={out}/vs", f"--metric_output_dir={out}/metrics", "--action=train"] + extra
            t = time.perf_counter()
            cli_mod.run(argv)
            dt = time.perf_counter() - t
            shutil.rmtree(out)
            return dt
        os.environ.pop("TF_CONFIG", None)
        run(os.path.join(d, "warm"), ["--l2_reg_weight=1.0"])       # pays for the HIP context and the library load
        flag = "--l2_reg_weights=" + ",".join(repr(w) for w in GRID8)
        plain, eight, swept = [], [], []
        for rep in range(3):
            plain.append(run(os.path.join(d, "plain"), ["--l2_reg_weight=1.0"]))
            swept.append(run(os.path.join(d, "swept"), [flag]))
            eight.append(sum(run(os.path.join(d, f"plain{k}"), [f"--l2_reg_weight={w!r}"]) for k, w in enumerate(GRID8)))
        med = statistics.median
        for what, v in (("one plain run", plain), ("eight plain runs, one per weight", eight), ("one run with --l2_reg_weights (K = 8)", swept)):
            print(f"  {what:<42s} {med(v):7.2f} s [{min(v):.2f}, {max(v):.2f}] (3 runs, alternating)")
        print(f"  the sweep is {med(swept) / med(plain):.2f} x one plain run and {med(swept) / med(eight):.2f} x eight plain runs")


if WHAT in ("kernels", "all"):
    kernels()
if WHAT in ("cli", "all"):
    cli()
