"""GPU: the host path the elastic net, the box solve and TRON share (csrc/re_entity_scaffold.hpp, solve_three_lists): one mixed batch per
loss on which a solve fills all three lists — the wavefront kernel's small entities, its large ones and the workgroup kernel's — so that
the three launches and the side-stream fork and join run in one call, for solve(l1=0.5), solve(bounds=...) and solve_tron. Every result
array is compared byte for byte with what the commit before the shared driver returned for the same seeded batch
(tests/golden/re_three_lists_parent/{l1,box,tron}.npz, results only). The solves are deterministic wherever an entity sits
(test_the_same_bits_from_run_to_run_and_wherever_the_entity_sits), so equality needs no tolerance.

The fixture was recorded on an MI355X from the library of commit 2d23fbd ("Random effect: trust-region Newton (TRON) per entity on the
device": `python -m gdmix_amd.build --out lib_parent.so` in a checkout of it), copied over gdmix_amd/libgdmix_re.so of this tree
(solver.py and the helpers are the same in both):

    GDMIX_ALLOW_STALE_LIB=1 PYTHONPATH=.:tests python tests/test_gpu_re_three_lists.py --record
"""
import functools
import os
import sys

import numpy as np
import pytest

import re_box_helpers as B
import re_l1_helpers as R
import re_linear_helpers as H
import re_tron_helpers as T

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "re_three_lists_parent")
ENTRIES = ("l1", "box", "tron")
FIELDS = ("theta", "theta_thr", "fval", "gnorm", "nit", "nfev", "status")
WIDE = [(90, 10, 300), (110, 10, 340), (130, 12, 380)]      # (n, k_max, d_max) of re_l1_helpers.make_batch: up to a few hundred coefficients
SMALL_LDS = 20 * 1024      # csrc/re_entity_scaffold.hpp, WAVE_SMALL_LDS
M = 10


@functools.lru_cache(maxsize=None)
def _batch(loss):
    """The `mixed` case's 40 shapes (n from 1 to 64, p from 1 to more than 64) and three wider entities."""
    return R.make_batch(loss, R.mixed_shapes(40, R.LOSSES.index(loss)) + WIDE, seed=900 + R.LOSSES.index(loss))


def _footprints(entry, b, packed):
    """LDS bytes of every entity under the entry point's solver, by the tests' restatements of the footprint."""
    f, z, n = packed.ent_feat_ptr().cpu().numpy(), packed.ent_nnz_ptr().cpu().numpy(), b.ent_n()
    d, nnz = np.diff(f), np.diff(z)
    if entry == "tron":
        return np.array([T.lds_bytes(int(d[e]) + 1, int(n[e]), int(nnz[e]), int(d[e]), False) for e in range(b.E)])
    lds = R.lds_bytes if entry == "l1" else B.lds_bytes
    return np.array([lds(int(d[e]) + 1, int(n[e]), int(nnz[e]), int(d[e]), M, False) for e in range(b.E)])


def _solve(solver, entry, loss):
    """-> (host results, count words 0-4). wave_lds_limit is the largest footprint below the batch's largest: the largest entity goes to
    the workgroup kernel, the others above SMALL_LDS to the wavefront kernel's large launch, the rest to its small one."""
    from gdmix_amd.solver import SolverOptions
    b = _batch(loss)
    opts = SolverOptions(l2=R.L2, m=M, loss=loss)
    packed = solver.pack(b, has_intercept=True)
    fp = _footprints(entry, b, packed)
    limit = int(fp[(fp < fp.max()) & (fp <= 65536)].max())
    assert limit > SMALL_LDS and (fp <= SMALL_LDS).any(), (entry, loss, sorted(fp)[-4:])
    solver.set_wave_lds_limit(limit)
    try:
        if entry == "l1":
            res = solver.solve(packed, opts, l1=R.L1)
        elif entry == "box":
            res = solver.solve(packed, opts, bounds=solver.upload_bounds(*B.bounds()))
        else:
            res = solver.solve_tron(packed, opts)
        res = res.to_host()
        cc = packed._view(packed.c.class_count, 5, solver.torch.int32).cpu().numpy()
    finally:
        H.reset_routing(solver)
    return res, cc


def _fields(entry):
    return FIELDS + (("nhv",) if entry == "tron" else ())


@pytest.mark.parametrize("loss", R.LOSSES)
@pytest.mark.parametrize("entry", ENTRIES)
def test_three_lists_in_one_solve_return_the_parents_bytes(device_solver, entry, loss):
    res, cc = _solve(device_solver, entry, loss)
    b = _batch(loss)
    print(f"{entry} {loss}: small {cc[4]}, large {cc[2]} (LDS {cc[3]}), workgroup {cc[1]} of {b.E} entities")
    assert cc[4] > 0 and cc[2] > 0 and cc[1] > 0 and cc[2] + cc[4] == cc[0] and cc[0] + cc[1] == b.E, cc
    with np.load(os.path.join(GOLDEN, entry + ".npz")) as gold:
        for k in _fields(entry):
            want, have = gold[f"{loss}_{k}"], np.asarray(res[k])
            assert have.dtype == want.dtype and have.shape == want.shape, (k, have.dtype, have.shape)
            assert have.tobytes() == want.tobytes(), (k, int(np.sum(have != want)))


def _record():
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from gdmix_amd.solver import REDeviceSolver
    solver = REDeviceSolver(0)
    os.makedirs(GOLDEN, exist_ok=True)
    for entry in ENTRIES:
        out = {}
        for loss in R.LOSSES:
            res, cc = _solve(solver, entry, loss)
            assert cc[4] > 0 and cc[2] > 0 and cc[1] > 0, (entry, loss, cc)
            print(entry, loss, "counts", cc.tolist())
            out.update({f"{loss}_{k}": np.asarray(res[k]) for k in _fields(entry)})
        np.savez_compressed(os.path.join(GOLDEN, entry + ".npz"), **out)
    solver.close()


if __name__ == "__main__":
    if "--record" in sys.argv:
        _record()
