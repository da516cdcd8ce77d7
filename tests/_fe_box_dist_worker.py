"""Worker of the two-process fixed-effect box-constraint test: each rank holds every other sample of fe_box_helpers.case("logistic", "small") as
its shard and runs the product path fit_stepping(bounds=...); every rank passes the same bounds. With two GPUs every rank takes its own device
and the all-reduce is RCCL; on a 1-GPU box the ranks share GPU 0 and the all-reduce goes through gloo."""
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
import fe_box_helpers as H


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
    rp, col, val, y, off, D, _, l2 = H.case("logistic", "small")
    rows = np.arange(rank, rp.size - 1, world)
    k = np.diff(rp)[rows]
    nz = np.concatenate([np.arange(rp[i], rp[i + 1]) for i in rows])
    s = fe.FixedEffectDeviceSolver(dev)
    theta, info = s.fit_stepping(np.concatenate([[0], np.cumsum(k)]), col[nz], val[nz], y[rows], D, offset=off[rows], model_type=fe.LOGISTIC_REGRESSION,
                                 l2=l2, bounds=H.bounds("small"), **H.FIT)
    out = {"theta": theta.tolist(), "fval": float(info["fval"]), "status": int(info["status"]), "nit": int(info["nit"]), "nfev": int(info["nfev"]),
           "at_bound": int(info["at_bound"]), "backend": dist.get_backend()}
    gathered = [None] * world
    dist.all_gather_object(gathered, out)
    if rank == 0:
        json.dump(gathered, open(os.path.join(base, "result.json"), "w"))
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
