"""Worker of the two-process test of the fixed effect's feature normalisation: each rank holds every other sample of the seeded case of
tests/test_gpu_feature_normalization.py (fe_case) as its shard, computes the stage's factors as fe_model does (two passes on its device
shard, the integers all-reduced; the chief writes the file) and runs the product path fit_stepping(feature_scale=...). With at least two
GPUs every rank takes its own device and the collectives are RCCL; on a 1-GPU box the ranks share GPU 0 and they go through gloo."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np
import torch
import torch.distributed as dist

import fe_prior_helpers as fh
from gdmix_amd import feature_stats as fs
from gdmix_amd import fixed_effect as fe


def main():
    from test_gpu_feature_normalization import fe_case
    base = sys.argv[1]
    world = int(os.environ["WORLD_SIZE"])
    rccl = torch.cuda.device_count() >= world
    dev = int(os.environ.get("LOCAL_RANK", "0")) if rccl else 0
    torch.cuda.set_device(dev)
    if rccl:
        dist.init_process_group("nccl", device_id=torch.device("cuda", dev))
    else:
        dist.init_process_group("gloo")
    rank, world = dist.get_rank(), dist.get_world_size()
    c, _ = fe_case()
    rp, col, val, y, off, wt = fh.rows_of(c, np.arange(rank, c.n, world))
    s = fe.FixedEffectDeviceSolver(dev)
    shard = s.upload(rp, col, val, off, c.D)
    factor, stats = fs.fixed_effect_factors(fs.SCALE_WITH_STANDARD_DEVIATION, os.path.join(base, "written.npz"), s.solver, c.D, shard.cg, shard.vl,
                                            len(y), is_chief=rank == 0)
    fs.save(os.path.join(base, f"stats{rank}.npz"), stats)
    theta, info = s.fit_stepping(rp, col, val, y, c.D, offset=off, weight=wt, has_intercept=True, l2=fh.L2, regularize_bias=True,
                                 max_iter=1000, tolerance=1e-15, feature_scale=factor, variance_mode="SIMPLE")
    out = {"_backend": dist.get_backend(), "theta": theta.tolist(), "variances": np.asarray(info["variances"]).tolist(),
           "status": int(info["status"]), "nit": int(info["nit"]), "nfev": int(info["nfev"])}
    gathered = [None] * world
    dist.all_gather_object(gathered, out)
    if rank == 0:
        json.dump(gathered, open(os.path.join(base, "result.json"), "w"))
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
