"""Child process of tests/test_gpu_fe_sweep.py: gdmix_fe_restart through the host loop `do { eval; } while (step() < 0)` with the step as
three launches (GDMIX_FE_FUSED_TAIL=0 is read when a problem is created, so it is set by the parent for this process alone).
argv: <golden fixture name> <result.json>. Writes, per weight, whether restart + loop gave the bits of create + loop."""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

from gdmix_amd import fixed_effect as fe      # noqa: E402
from gdmix_amd.solver import REDeviceSolver, SolverOptions      # noqa: E402


def loop(prob, max_evals=2000):
    for _ in range(max_evals):
        prob.eval()
        st = prob.step()
        if st >= 0:
            theta, info = prob.result()
            return theta, dict(info, status=st)
    raise RuntimeError("the loop did not stop")


def main(name, out):
    assert os.environ.get("GDMIX_FE_FUSED_TAIL") == "0"
    z = np.load(os.path.join(HERE, "golden", f"fe_{name}.npz"))
    c = {k: z[k] for k in z.files}
    ic, D, linear = bool(c["has_intercept"]), int(c["num_features"]), bool(c["linear"])
    s = REDeviceSolver(0)
    batch, _ = fe.shard_as_batch(c["row_nnz_ptr"], c["col_global"], c["val"], c["y"], c["offset"], None, ic, binary_labels=not linear, dummy=False)
    packed = s.pack(batch, has_intercept=ic)
    opts = lambda w: SolverOptions(l2=w, regularize_bias=ic, has_intercept=ic, m=10, max_iter=100, threshold=0.0, sum_loss=True, linear=linear)
    weights = (10.0, 1.0, 0.1)
    fresh = []
    for w in weights:
        prob = fe._SteppingProblem(s, packed, D, opts(w), None)
        fresh.append(loop(prob))
        prob.close()
    prob = fe._SteppingProblem(s, packed, D, opts(weights[-1]), None)
    loop(prob)
    res = []
    for w, (th, info) in zip(weights, fresh):
        prob.restart(opts(w), None)
        th2, info2 = loop(prob)
        res.append({"l2": w, "theta_equal": bool(np.array_equal(th, th2)), "info_equal": info == info2, "nit": int(info["nit"]), "status": int(info["status"])})
    prob.close()
    s.close()
    with open(out, "w") as f:
        json.dump(res, f)


if __name__ == "__main__":
    main(sys.argv[1], sys.argv[2])
