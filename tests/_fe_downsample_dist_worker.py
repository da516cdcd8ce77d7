"""Worker of the two-process down-sampling test: each rank holds every other sample of test_gpu_downsample.small_case (logistic labels) as
its shard, down-samples it with the common rate and seed, and runs the product path fit_stepping(down_sampling=...). It reports the uids its
own down-sampling pass kept next to the coefficients. With two GPUs every rank takes its own device and the all-reduce is RCCL; on a 1-GPU
box the ranks share GPU 0 and the all-reduce goes through gloo."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np
import torch
import torch.distributed as dist

from gdmix_amd import fixed_effect as fe
from test_gpu_downsample import FIT, FIT_SEED, RATE, small_case


def main():
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
    model_type = fe.LOGISTIC_REGRESSION
    rp, col, val, y, off, wt, D, uid = small_case(model_type)
    rows = np.arange(rank, rp.size - 1, world)
    k = np.diff(rp)[rows]
    nz = np.concatenate([np.arange(rp[i], rp[i + 1]) for i in rows])
    shard = (np.concatenate([[0], np.cumsum(k)]).astype(np.int64), col[nz], val[nz], y[rows])
    s = fe.FixedEffectDeviceSolver(dev)
    batch, _ = fe.shard_as_batch(*shard, off[rows], wt[rows], True, dummy=False)
    sample, _ = s.solver.downsample(s.solver.upload(batch), uid[rows], RATE, FIT_SEED, negatives_only=True)
    kept_uid = uid[rows][sample["kept_rows"].cpu().numpy()]
    theta, info = s.fit_stepping(*shard, D, offset=off[rows], weight=wt[rows], model_type=model_type, down_sampling=(RATE, FIT_SEED, uid[rows]), **FIT)
    out = {"theta": theta.tolist(), "status": int(info["status"]), "nit": int(info["nit"]), "nfev": int(info["nfev"]), "kept_uid": kept_uid.tolist(),
           "kept": int(info["down_sampling"]["kept"]), "backend": dist.get_backend()}
    assert out["kept"] == kept_uid.size
    gathered = [None] * world
    dist.all_gather_object(gathered, out)
    if rank == 0:
        json.dump(gathered, open(os.path.join(base, "result.json"), "w"))
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
