"""Worker of the two-process host test of the feature statistics: each gloo rank holds every other stored entry of a seeded case
(tests/test_feature_stats_host.py: small_case) and half of the samples, runs the numpy stand-in of the two kernels through
feature_stats.collect with the group's all-reduce, and writes what it ends with. No GPU."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np
import torch.distributed as dist

from gdmix_amd import feature_stats as fs

CASE = dict(seed=11, D=40, N=501)


def main():
    from test_feature_stats_host import small_case
    base = sys.argv[1]
    dist.init_process_group("gloo")
    rank, world = dist.get_rank(), dist.get_world_size()
    col, val, D, N = small_case(**CASE)
    mine = np.arange(rank, col.size, world)
    n_mine = len(range(rank, N, world))
    acc = fs.NumpyAccumulator(D)
    stats = fs.collect(acc, lambda a: a.add(col[mine], val[mine]), n_mine, fs.SCALE_WITH_STANDARD_DEVIATION, fs.group_all_reduce())
    fs.save(os.path.join(base, f"rank{rank}.npz"), stats)
    np.save(os.path.join(base, f"limbs{rank}.npy"), stats.limbs)
    if rank == 0:
        json.dump({"world": world, "backend": dist.get_backend()}, open(os.path.join(base, "result.json"), "w"))
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
