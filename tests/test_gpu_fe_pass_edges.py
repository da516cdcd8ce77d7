"""The fixed-effect passes at their unit, block, form and hot edges, on the device: one gdmix_fe_eval (and one Hessian diagonal, one product)
of every shard of tests/fe_pass_edges_helpers.py under every hook set, held element by element to the longdouble reference under the
tolerance law stated there. stream_bytes() of every problem must equal the restated plan's two byte counts: the packed, three-array and
6-byte forms, the cuts and the frequent columns are then what the helper says they are (tests/test_fe_pass_edges.py asserts, without a
GPU, that those plans show every edge). Different forms are not compared bit for bit: the packed form adds a lane's pair in another order.

The many-units case (1.1 M entries at chunk 64, nred = 23 460) is the one test that takes more than about a second."""
import time

import numpy as np
import pytest

from gdmix_amd import fixed_effect as fe
import fe_pass_edges_helpers as H

L2 = 0.5      # (the buffer holds the data term alone: the regulariser must not show)


def set_hooks(monkeypatch, hooks):
    for var, value in H.env_of(hooks).items():
        if value is None:
            monkeypatch.delenv(var, raising=False)
        else:
            monkeypatch.setenv(var, value)


def num_cus(device_solver):
    return int(device_solver.torch.cuda.get_device_properties(device_solver.device).multi_processor_count)


class Case:
    """A shard packed for (loss, weighted, ic); new() creates a problem at theta0 under the hooks in force."""

    def __init__(self, device_solver, key, loss, weighted, ic):
        self.s, self.t = device_solver, device_solver.torch
        self.key, self.loss, self.weighted, self.ic = key, loss, weighted, ic
        self.sh = sh = H.shard(key)
        self.P = sh.D + ic
        batch, dummy = fe.shard_as_batch(sh.rp, sh.col, sh.val, sh.labels(loss), sh.off, sh.wt if weighted else None, bool(ic),
                                         binary_labels=loss == "logistic", dummy=False)
        assert not dummy
        self.packed = device_solver.pack(batch, has_intercept=bool(ic))
        self.opts = fe.fit_options(bool(ic), L2, False, H.MODEL_TYPE[loss], 10, 5, 1e-7)
        self.theta0, self.theta1, self.vec = (self.up(sh.point(w, ic)) for w in ("theta0", "theta1", "vec"))

    def up(self, a):
        return self.t.from_numpy(np.ascontiguousarray(a, np.float64)).to(self.s.device)

    def new(self):
        return fe._SteppingProblem(self.s, self.packed, self.sh.D, self.opts, self.theta0)

    def ref(self):
        return H.reference(self.key, self.loss, self.weighted, self.ic)


def read(prob):
    return prob.reduce_tensor().cpu().numpy().copy()


def held(got, ref, E, what, n=None):
    """got under the law against ref with the bounds E (the first n slots); prints the figure before it asserts."""
    n = ref.size if n is None else n
    ratio = H.law_ratio(got[:n], ref[:n], E[:n])
    print(f"{what}: max err / E = {ratio:.3f} (K = {H.K:.1f})")
    assert ratio <= H.K, (what, ratio)


def exact_zeros(case, got, what):
    """Point 9: the slot of a feature absent from the shard, and of a column whose terms cancel exactly, is +0.0."""
    sh = case.sh
    for j in list(sh.absent) + [int(sh.uniq[c]) for c in sh.cancel_cols]:
        assert got[j] == 0.0 and not np.signbit(got[j]), (what, j, got[j])


def check_problem(case, hooks, plan_cus):
    sh, P = case.sh, case.P
    ref = case.ref()
    plan = H.pass_plans(sh, hooks, plan_cus)
    prob, twin = case.new(), case.new()
    try:
        what = f"{case.key} [{H.hook_id(hooks)}] {case.loss} weighted={case.weighted} ic={case.ic}"
        assert prob.stream_bytes() == (plan.rows.stream_bytes, plan.cols.stream_bytes), (what, prob.stream_bytes(), plan.rows.stream_bytes, plan.cols.stream_bytes)
        assert prob.count == P + 1
        prob.eval()
        g0 = read(prob)
        held(g0, ref["grad"], ref["E_grad"], what + " eval")
        exact_zeros(case, g0, what + " eval")
        prob.eval()
        assert read(prob).tobytes() == g0.tobytes(), what + ": a second eval"
        twin.eval()
        assert read(twin).tobytes() == g0.tobytes(), what + ": a second creation"
        prob.restart(case.opts, case.theta0)
        prob.eval()
        assert read(prob).tobytes() == g0.tobytes(), what + ": eval behind a restart"
        prob.hessian_diag(case.theta1)
        h = read(prob)
        held(h, ref["diag"], ref["E_diag"], what + " hessian_diag", P)
        for j in sh.absent:
            assert h[j] == 0.0 and not np.signbit(h[j]), (what, "hessian_diag", j)
        prob.eval()       # the solver's point is back in xl and the buffer cleared: the cancelling columns' slots held 2 v^2 D a moment ago
        g1 = read(prob)
        assert g1.tobytes() == g0.tobytes(), what + ": eval behind hessian_diag"
        exact_zeros(case, g1, what + " eval behind hessian_diag")
        return prob, twin
    except BaseException:
        prob.close()
        twin.close()
        raise


_CASES = {}


def case_of(device_solver, key, loss, weighted, ic):
    k = (key, loss, weighted, ic)
    if k not in _CASES:
        _CASES.clear()      # one packed shard alive at a time
        _CASES[k] = Case(device_solver, key, loss, weighted, ic)
    return _CASES[k]


SMALL = H.problems(H.SMALL_KEYS)


@pytest.mark.gpu
@pytest.mark.parametrize("key,hooks", SMALL, ids=[f"{k}-{H.hook_id(h)}" for k, h in SMALL])
def test_one_evaluation_of_every_edge_shard_in_every_form(device_solver, monkeypatch, key, hooks):
    set_hooks(monkeypatch, hooks)
    case = case_of(device_solver, key, *H.DEFAULT_CASE)
    prob, twin = check_problem(case, hooks, num_cus(device_solver))
    prob.close()
    twin.close()


@pytest.mark.gpu
@pytest.mark.parametrize("pack", [None, 0], ids=["packed", "three-array"])
def test_the_many_units_case(device_solver, monkeypatch, pack):
    """nred = 23 460 > 64 * 256: a range of fe_finish_kernel's value sums takes two trips of its 256 threads; 17 000 units a pass."""
    hooks = dict(H._HOOK_TABLE["many_units"][0][0], pack=pack)
    set_hooks(monkeypatch, hooks)
    case = case_of(device_solver, "many_units", *H.DEFAULT_CASE)
    t0 = time.perf_counter()
    prob, twin = check_problem(case, hooks, num_cus(device_solver))
    print(f"many_units [{H.hook_id(hooks)}]: two creations, five evaluations and a Hessian diagonal in {time.perf_counter() - t0:.2f} s")
    prob.close()
    twin.close()


VARIANT_IDS = [f"{k}-{loss}-{'weighted' if w else 'unweighted'}-{'intercept' if ic else 'no_intercept'}" for k in H.VARIANT_SHARDS for loss, w, ic in H.VARIANTS]


@pytest.mark.gpu
@pytest.mark.parametrize("key,loss,weighted,ic", [(k,) + v for k in H.VARIANT_SHARDS for v in H.VARIANTS], ids=VARIANT_IDS)
def test_losses_weights_intercept_the_product_and_tron(device_solver, monkeypatch, key, loss, weighted, ic):
    """The two variant shards under every (loss, weights, intercept): the evaluation, the diagonal, the product on an L-BFGS problem; then the
    same problem as TRON's: its evaluation (the HV row variant) and its product, under the same law."""
    hooks = H.VARIANT_SHARDS[key]
    set_hooks(monkeypatch, hooks)
    case = case_of(device_solver, key, loss, weighted, ic)
    ref, P = case.ref(), case.P
    what = f"{key} [{H.hook_id(hooks)}] {loss} weighted={weighted} ic={ic}"
    prob, twin = check_problem(case, hooks, num_cus(device_solver))
    try:
        prob.hessian_vec(case.theta1, case.vec)
        hv = read(prob)
        held(hv, ref["hv"], ref["E_hv"], what + " hessian_vec (L-BFGS problem)")
        prob.eval()
        g0 = read(prob)
        held(g0, ref["grad"], ref["E_grad"], what + " eval behind hessian_vec")
        twin.set_optimizer("TRON")
        twin.restart(case.opts, case.theta0)
        twin.eval()
        gt = read(twin)
        held(gt, ref["grad"], ref["E_grad"], what + " eval (TRON problem)")
        exact_zeros(case, gt, what + " eval (TRON problem)")
        twin.hessian_vec(case.theta1, case.vec)
        held(read(twin), ref["hv"], ref["E_hv"], what + " hessian_vec (TRON problem)")
        twin.eval()
        assert read(twin).tobytes() == gt.tobytes(), what + ": a TRON problem's eval behind hessian_vec"
    finally:
        prob.close()
        twin.close()


@pytest.mark.gpu
@pytest.mark.parametrize("key", list(H.VARIANT_SHARDS))
def test_a_prior_moves_the_point_and_a_neutral_one_moves_nothing(device_solver, monkeypatch, key):
    """set_prior, then restart with theta0 in theta units: the reference is evaluated at the point result() reports before any step, because the
    change of variables rounds; the buffer carries the theta-space gradient. mu = 0, s = 1 gives the bits of no prior."""
    hooks = H.VARIANT_SHARDS[key]
    set_hooks(monkeypatch, hooks)
    case = case_of(device_solver, key, *H.DEFAULT_CASE)
    sh, P = case.sh, case.P
    rng = np.random.default_rng(3)
    prob = case.new()
    try:
        prob.eval()
        plain = read(prob)
        prob.set_prior(case.up(np.zeros(P)), case.up(np.ones(P)))
        prob.restart(case.opts, case.theta0)
        prob.eval()
        assert read(prob).tobytes() == plain.tobytes(), f"{key}: a neutral prior"
        mu, sc = 0.1 * rng.standard_normal(P), rng.uniform(0.5, 2.0, P)
        prob.set_prior(case.up(mu), case.up(sc))
        prob.restart(case.opts, case.theta0)
        at, _ = prob.result()
        assert np.max(np.abs(at - sh.point("theta0", 1))) <= 1e-15
        prob.eval()
        got = read(prob)
        ref = H.evaluate(sh, *H.DEFAULT_CASE, theta0=at)
        held(got, ref["grad"], ref["E_grad"], f"{key} [{H.hook_id(hooks)}] eval with a prior")
        exact_zeros(case, got, f"{key} eval with a prior")
    finally:
        prob.close()
