"""GPU: the random effect's trust-region Newton solve (REDeviceSolver.solve_tron, gdmix_re_solve_tron; include/gdmix_re.h, "TRON") — both
kernels against the numpy restatement and the algorithm-independent reference of tests/re_tron_helpers.py, held to that module's rule at
its tight tolerances; lane, thread, slot and footprint edges; the CG cap, the boundary branch, rejected trials, one iteration, a start at
the solution, determinism, the variances, the other solves left alone, the refusals, the stage and the chain. The shapes are the smallest
at which each kernel can still go wrong; tests/test_re_tron_host.py asserts that the restatement alone keeps the committed cases within
the bars."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from gdmix_amd import solver as S
from gdmix_amd.batch import RawBatch
from gdmix_amd.solver import SolverOptions
import re_l1_helpers as R
import re_linear_helpers as H
import re_tron_helpers as T

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _opts(loss, v, variance_mode=0, l2=T.L2, **kw):
    t = dict(T.TIGHT, **kw)
    return SolverOptions(l2=l2, regularize_bias=v["regularize_bias"], has_intercept=v["has_intercept"], m=10, max_iter=t["max_iter"], maxfun=t["maxfun"],
                         maxls=t["maxls"], ftol=t["ftol"], pgtol=t["pgtol"], variance_mode=variance_mode, loss=loss)


def _solve(solver, b, opts, theta0=None, lds_limit=None):
    """-> (host results, packed, (wavefront kernel's entities, workgroup kernel's), (its large-LDS launch, its small-LDS launch))."""
    packed = solver.pack(b, has_intercept=bool(opts.has_intercept))
    if lds_limit is not None:
        solver.set_wave_lds_limit(lds_limit)
    try:
        res = solver.solve_tron(packed, opts, theta0=theta0).to_host()
        cc = packed._view(packed.c.class_count, 5, solver.torch.int32).cpu().numpy()
    finally:
        H.reset_routing(solver)
    assert np.array_equal(packed.coef_ptr_host(), R.coef_ptr(b, bool(opts.has_intercept)))      # the tests' local order is the pack's
    assert (int(cc[0]), int(cc[1])) == solver.tron_counts(packed) and cc[2] + cc[4] == cc[0]
    return res, packed, (int(cc[0]), int(cc[1])), (int(cc[2]), int(cc[4]))


def _gnorm_is_the_gradients(res, pbs, cp):
    for e, pb in pbs.items():
        g = pb.smooth(res["theta"][int(cp[e]):int(cp[e + 1])])[1]
        assert abs(res["gnorm"][e] - np.max(np.abs(g), initial=0.0)) <= 1e-12, e


# 1 ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lds_limit", [None, 0], ids=["wavefront", "workgroup"])
@pytest.mark.parametrize("variant", list(T.VARIANTS))
@pytest.mark.parametrize("loss", T.LOSSES)
def test_three_losses_against_the_restatement_and_the_reference(device_solver, loss, variant, lds_limit):
    """The mixed batch (n from 1, p from 1 to more than 64 coefficients) under default routing — every entity fits the wavefront kernel —
    and with wave_lds_limit = 0, every entity on the workgroup kernel. Without and with weights, without an intercept, with an
    unregularised one (there the distance bound is no theorem and is skipped)."""
    pbs, refs, rest, b, v = T.case(loss, variant, "mixed")
    res, packed, counts, _ = _solve(device_solver, b, _opts(loss, v), lds_limit=lds_limit)
    assert counts == ((b.E, 0) if lds_limit is None else (0, b.E))
    cp = packed.coef_ptr_host()
    T.compare(res, pbs, rest, refs, cp, distance=v["distance"], what=f"device {loss} {variant} {'wavefront' if lds_limit is None else 'workgroup'}")
    _gnorm_is_the_gradients(res, pbs, cp)
    assert np.array_equal(res["theta_thr"], np.where(np.abs(res["theta"]) <= T.THRESHOLD, 0.0, res["theta"]))


# 2 ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("loss", T.LOSSES)
def test_more_samples_and_coefficients_than_threads_and_more_entities_than_slots(device_solver, loss):
    """wave_lds_limit = 0: the mixed entities, one with more samples and more coefficients than the workgroup has threads (n, p > 256), and
    2 100 tiny ones, more than the grid has workgroups (1 024 slots), so that scratch slots are reused. The sample of
    re_l1_helpers.block_sample is held to the rule; every entity's fval is F at its theta."""
    pbs, refs, rest, b, v = T.case(loss, "plain", "block")
    big = int(np.argmax(b.ent_n()))
    assert b.ent_n()[big] > 256 and big in pbs and refs[big][0].size > 256 and b.E > 2048
    res, packed, counts, _ = _solve(device_solver, b, _opts(loss, v), lds_limit=0)
    assert counts == (0, b.E)
    cp = packed.coef_ptr_host()
    T.compare(res, pbs, rest, refs, cp, what=f"device {loss} workgroup kernel, block batch")
    assert np.all((res["status"] >= 0) & (res["status"] <= 4)) and np.all(res["nhv"] >= res["nit"])
    worst = 0.0
    for e in range(b.E):
        pb = pbs[e] if e in pbs else R.entity_problem(b, e, loss, 0.0, T.L2)
        F_np = pb.smooth(res["theta"][int(cp[e]):int(cp[e + 1])])[0]
        worst = max(worst, abs(res["fval"][e] - F_np) / abs(F_np))
    print(f"{loss}: over all {b.E} entities: worst |fval - F_numpy| / |F| {worst:.3e}")
    assert worst <= 1e-9


# 3 ---------------------------------------------------------------------------------------------------------------------------------------
EDGE_P = (1, 2, 63, 64, 65, 127, 128, 129)
EDGE_N = (1, 2, 63, 64, 65)


def _exact_batch(loss, shapes, seed, D=600, spread=0.0):
    """Entities of exactly (p, n): p - 1 features, each in at least one row (feature j in row j mod n), two more cells per row where the
    entity has features; p = 1 is an entity whose samples are all empty rows (d = 0: the intercept alone). spread: feature j's values are
    scaled by 10^u_j, u_j uniform in [-spread, spread] (an ill-conditioned Hessian)."""
    rng = np.random.default_rng(seed)
    col_scale = 10.0 ** rng.uniform(-spread, spread, D) if spread else np.ones(D)
    erp, rnp, cols, vals = [0], [0], [], []
    for (p, n) in shapes:
        d = p - 1
        own = rng.choice(D, size=d, replace=False)
        for i in range(n):
            c = list(own[i::n]) + (list(rng.choice(own, size=2)) if d else [])
            cols.append(np.array(c, np.int64))
            vals.append((0.6 * rng.standard_normal(len(c)) * col_scale[cols[-1]]).astype(np.float32))
            rnp.append(rnp[-1] + len(c))
        erp.append(erp[-1] + n)
    N = erp[-1]
    z = 0.7 * rng.standard_normal(N)
    return RawBatch(ent_row_ptr=np.array(erp), row_nnz_ptr=np.array(rnp), col_global=np.concatenate(cols), val=np.concatenate(vals),
                    y=R._labels(rng, loss, z), offset=(0.3 * rng.standard_normal(N)).astype(np.float32), weight=None, binary_labels=loss == "logistic")


_EDGE = {}


def _edge_case(loss):
    if loss not in _EDGE:
        b = _exact_batch(loss, [(p, n) for p in EDGE_P for n in EDGE_N], seed=500 + T.LOSSES.index(loss))
        v = T.VARIANTS["plain"]
        pbs = T.problems(("edges", loss), b, loss, v)
        assert sorted({pb.X.shape[1] for pb in pbs.values()}) == list(EDGE_P) and sorted({pb.n for pb in pbs.values()}) == list(EDGE_N)
        _EDGE[loss] = (pbs, T.references(("edges", loss), pbs), T.restatements(("edges", loss), pbs), b, v)
    return _EDGE[loss]


@pytest.mark.parametrize("lds_limit", [None, 0], ids=["wavefront", "workgroup"])
@pytest.mark.parametrize("loss", T.LOSSES)
def test_lane_and_thread_edges(device_solver, loss, lds_limit):
    """Every p of 1, 2, 63, 64, 65, 127, 128, 129 coefficients with every n of 1, 2, 63, 64, 65 samples; p = 1 is d = 0 under an intercept,
    every sample an empty row."""
    pbs, refs, rest, b, v = _edge_case(loss)
    res, packed, counts, _ = _solve(device_solver, b, _opts(loss, v), lds_limit=lds_limit)
    assert counts == ((b.E, 0) if lds_limit is None else (0, b.E))
    T.compare(res, pbs, rest, refs, packed.coef_ptr_host(), what=f"device {loss} edges")
    empty = [e for e, pb in pbs.items() if pb.X.shape[1] == 1]
    assert len(empty) == len(EDGE_N) and all(res["nhv"][e] >= 1 or res["status"][e] == 0 for e in empty)


# 4 ---------------------------------------------------------------------------------------------------------------------------------------
def test_the_footprint_edge_between_the_two_kernels(device_solver):
    """wave_lds_limit = the TRON footprint of the first entity; the second has one cell more: 16 bytes. Both are solved within the bars,
    and the counts say that each kernel took one."""
    from test_gpu_re_l1 import _edge_batch
    b = _edge_batch()
    v = T.VARIANTS["plain"]
    fp = [T.lds_bytes(p=6, n=4, nnz=z, d=5, has_w=False) for z in (10, 11)]
    assert fp[1] == fp[0] + 16
    pbs = T.problems(("kernel edge",), b, "logistic", v)
    refs, rest = T.references(("kernel edge",), pbs), T.restatements(("kernel edge",), pbs)
    for limit, want in ((fp[0], (1, 1)), (fp[0] - 16, (0, 2)), (fp[1], (2, 0))):
        res, packed, counts, _ = _solve(device_solver, b, _opts("logistic", v), lds_limit=limit)
        assert counts == want, (limit, counts)
        T.compare(res, pbs, rest, refs, packed.coef_ptr_host(), what=f"footprint edge, limit {limit}")


def test_the_edge_between_the_small_and_the_large_launch(device_solver):
    """Two entities either side of the 20 KB at which the wavefront kernel's entities are launched apart, next to small ones: the counts
    say which launch took which, and all are solved within the bars."""
    n, shapes = 64, []
    for p in range(150, 260):      # the first p whose footprint passes 20 KB, and the one before it
        nnz = n * 2 + (p - 1)
        if T.lds_bytes(p, n, nnz, p - 1, False) > T.SMALL_LDS:
            shapes = [(p - 1, n), (p, n), (5, 3), (64, 2)]
            break
    b = _exact_batch("logistic", shapes, seed=77)
    fps = [T.lds_bytes(p, m, int(b.row_nnz_ptr[b.ent_row_ptr[e + 1]] - b.row_nnz_ptr[b.ent_row_ptr[e]]), p - 1, False) for e, (p, m) in enumerate(shapes)]
    print(f"footprints {fps} around {T.SMALL_LDS}")
    assert fps[0] <= T.SMALL_LDS < fps[1] and fps[1] - fps[0] <= 64
    v = T.VARIANTS["plain"]
    pbs = T.problems(("launch edge",), b, "logistic", v)
    refs, rest = T.references(("launch edge",), pbs), T.restatements(("launch edge",), pbs)
    res, packed, counts, launches = _solve(device_solver, b, _opts("logistic", v))
    assert counts == (4, 0) and launches == (1, 3)
    T.compare(res, pbs, rest, refs, packed.coef_ptr_host(), what="launch edge")


# 5 ---------------------------------------------------------------------------------------------------------------------------------------
CG_CAP = dict(loss="squared", shapes=[(120, 100), (90, 80), (70, 64)], seed=91, spread=1.0, scale=100.0)
_CG = {}


def _cg_cap_case():
    """Squared loss, features that differ in scale by two decades (condition numbers of 1e6 and more), and a start theta_ref + sum_i q_i /
    lambda_i over the Hessian's eigenpairs: the gradient there has the same weight on every eigenvector, so CG has the whole spectrum to
    work through, and the Newton step is shorter than |g|, so the trust region does not end it early."""
    if not _CG:
        import dataclasses
        b = _exact_batch(CG_CAP["loss"], CG_CAP["shapes"], seed=CG_CAP["seed"], spread=CG_CAP["spread"])
        b = dataclasses.replace(b, val=(b.val * CG_CAP["scale"]).astype(np.float32))
        v = T.VARIANTS["plain"]
        pbs = T.problems(("cg cap",), b, CG_CAP["loss"], v)
        theta0 = []
        for e in range(b.E):
            pb, p = pbs[e], pbs[e].X.shape[1]
            lam, Q = np.linalg.eigh(np.column_stack([T.product(pb, np.zeros(p), np.eye(p)[j]) for j in range(p)]))
            theta0.append(T.reference_fit(pb)[0] + Q @ (1.0 / lam))
        theta0 = np.concatenate(theta0)
        _CG["case"] = (b, v, pbs, theta0, T.restatements(("cg cap",), pbs, theta0=theta0, cp=R.coef_ptr(b, True), max_iter=1))
    return _CG["case"]


@pytest.mark.parametrize("lds_limit", [None, 0], ids=["wavefront", "workgroup"])
def test_the_cg_cap(device_solver, lds_limit):
    """Entities of more than 50 coefficients on which the restatement's one outer iteration runs into 50 products (chosen on the CPU, and
    asserted here: nit 1, nfev 2, nhv 50 on strict entities). On those the device's four counts are the restatement's, fval is the numpy
    objective at the device's theta to 1e-9, and the step went downhill. theta itself is not held to the restatement's here: fifty CG steps
    on a Hessian of condition 1e6 carry the order of the sums into the result — the restatement run on the same entities with their
    samples in another order (the same problem, other rounding) moves its own theta by 1e-5 .. 1e-3 of the coefficient scale, and an
    MI355X differed from it by 4e-6 .. 1.4e-3 — so the 1e-7 of the strict rule has no footing on this case; every other test holds it."""
    b, v, pbs, theta0, rest = _cg_cap_case()
    print(f"restatement, one iteration: {[(T.counts(r['fit']), r['strict']) for r in rest.values()]}")
    capped = [e for e, r in rest.items() if T.counts(r["fit"]) == (2, 1, 2, T.MAX_CG) and r["strict"]]
    assert len(capped) >= 2
    res, packed, _, _ = _solve(device_solver, b, _opts(CG_CAP["loss"], v, max_iter=1), theta0=theta0, lds_limit=lds_limit)
    cp = packed.coef_ptr_host()
    for e in capped:
        s = slice(int(cp[e]), int(cp[e + 1]))
        got = (int(res["status"][e]), int(res["nit"][e]), int(res["nfev"][e]), int(res["nhv"][e]))
        F_np, F0 = pbs[e].smooth(res["theta"][s])[0], pbs[e].smooth(theta0[s])[0]
        print(f"entity {e}: device {got}, fval {res['fval'][e]!r}, numpy at theta {F_np!r}, at the start {F0!r}, restatement {rest[e]['fit'][1]!r}")
        assert got == (2, 1, 2, T.MAX_CG)
        assert abs(res["fval"][e] - F_np) <= 1e-9 * abs(F_np) and res["fval"][e] < F0


# 6, 8 ------------------------------------------------------------------------------------------------------------------------------------
_ONE = {}


@pytest.mark.parametrize("lds_limit", [None, 0], ids=["wavefront", "workgroup"])
@pytest.mark.parametrize("warm", [False, True], ids=["cold", "warm"])
@pytest.mark.parametrize("loss", T.LOSSES)
def test_one_iteration_counts_as_the_restatement_counts(device_solver, loss, warm, lds_limit):
    """max_iter = 1 from a cold start and from half the reference: (status, nit, nfev, nhv), theta and fval are the restatement's. From the
    cold start Delta = |g| and the first iteration's CG ends on the trust-region boundary for most entities — at its first product
    (s'd = 0) and, for the squared and the Poisson loss, at a later one (s'd > 0; in exact arithmetic Steihaug's s'd is never negative) — so
    the root formula is what the compared step came from."""
    pbs, refs, _, b, v = T.case(loss, "plain", "mixed")
    cp = R.coef_ptr(b, True)
    theta0 = np.concatenate([0.5 * refs[e][0] for e in range(b.E)]) if warm else None
    if (loss, warm) not in _ONE:
        _ONE[(loss, warm)] = T.restatements(("one", loss, warm), pbs, theta0=theta0, cp=cp, max_iter=1)
    rest = _ONE[(loss, warm)]
    if not warm:
        branches = {T.first_branch(pb) for e, pb in pbs.items() if rest[e]["strict"]}
        print(f"{loss}: first-iteration CG exits of the strict entities {sorted(branches)}")
        assert ("boundary", 0) in branches and (loss == "logistic" or ("boundary", 1) in branches)
    res, packed, _, _ = _solve(device_solver, b, _opts(loss, v, max_iter=1), theta0=theta0, lds_limit=lds_limit)
    T.compare(res, pbs, rest, None, cp, what=f"one iteration {loss} warm={warm}")
    assert np.all(res["nit"] <= 1) and np.all(res["status"][res["nit"] == 1] <= 2)


# 7 ---------------------------------------------------------------------------------------------------------------------------------------
REJECTING = dict(loss="poisson", seed=9, scale=4.0, at_least=8)      # 13 such entities at this scale, 7 at scale 3, 16 at 5


@pytest.mark.parametrize("lds_limit", [None, 0], ids=["wavefront", "workgroup"])
def test_rejected_trials(device_solver, lds_limit):
    """Poisson entities from a start point of large norm (the recipe of fe_tron_helpers.rejecting_case): the restatement rejects at least
    one trial on at least 8 strict entities (chosen on the CPU), and the device's counts are the restatement's."""
    loss = REJECTING["loss"]
    pbs, refs, _, b, v = T.case(loss, "plain", "mixed")
    cp = R.coef_ptr(b, True)
    theta0 = REJECTING["scale"] * np.random.default_rng(REJECTING["seed"]).standard_normal(int(cp[-1]))
    rest = T.restatements(("rejecting",), pbs, theta0=theta0, cp=cp)
    rejecting = [e for e, r in rest.items() if r["strict"] and r["fit"][6] >= 1]
    print(f"{len(rejecting)} strict entities whose restatement rejects a trial (up to {max(r['fit'][6] for r in rest.values())})")
    assert len(rejecting) >= REJECTING["at_least"]
    res, packed, _, _ = _solve(device_solver, b, _opts(loss, v), theta0=theta0, lds_limit=lds_limit)
    T.compare(res, pbs, rest, refs, cp, what="rejected trials")


# 9 ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lds_limit", [None, 0], ids=["wavefront", "workgroup"])
@pytest.mark.parametrize("loss", T.LOSSES)
def test_a_start_at_the_solution(device_solver, loss, lds_limit):
    """From the tight solve's own theta, at pgtol 1e-5: status 0 with nit 0, nfev 1, nhv 0, and theta is the start point's bits."""
    _, _, _, b, v = T.case(loss, "weights", "mixed")
    first, packed, _, _ = _solve(device_solver, b, _opts(loss, v), lds_limit=lds_limit)
    at = first["gnorm"] <= T.TIGHT["pgtol"]
    assert at.sum() >= 0.9 * b.E
    res, _, _, _ = _solve(device_solver, b, _opts(loss, v, pgtol=1e-5), theta0=first["theta"], lds_limit=lds_limit)
    assert np.all(res["status"][at] == 0) and np.all(res["nit"][at] == 0) and np.all(res["nfev"][at] == 1) and np.all(res["nhv"][at] == 0)
    cp = packed.coef_ptr_host()
    for e in np.flatnonzero(at):
        s = slice(int(cp[e]), int(cp[e + 1]))
        assert np.array_equal(res["theta"][s].view(np.uint8), first["theta"][s].view(np.uint8))
    assert np.array_equal(res["fval"][at].view(np.uint8), first["fval"][at].view(np.uint8))


# 10 --------------------------------------------------------------------------------------------------------------------------------------
KEYS = ("theta", "theta_thr", "fval", "nit", "nfev", "status")
STATS = ("fval", "gnorm", "nit", "nfev", "nhv", "status")


@pytest.mark.parametrize("lds_limit", [None, 0], ids=["wavefront", "workgroup"])
def test_the_same_bits_from_run_to_run_and_wherever_the_entity_sits(device_solver, lds_limit):
    _, _, _, b, v = T.case("logistic", "weights", "mixed")
    opts = _opts("logistic", v, variance_mode=1)
    first, packed, _, _ = _solve(device_solver, b, opts, lds_limit=lds_limit)
    again, _, _, _ = _solve(device_solver, b, opts, lds_limit=lds_limit)
    for k in KEYS + ("gnorm", "nhv", "variance"):
        assert np.array_equal(first[k].view(np.uint8), again[k].view(np.uint8)), k
    perm = np.random.default_rng(3).permutation(b.E)
    moved, packed_m, _, _ = _solve(device_solver, b.select(perm), opts, lds_limit=lds_limit)
    cp, cpm = packed.coef_ptr_host(), packed_m.coef_ptr_host()
    for k in STATS:
        assert np.array_equal(moved[k].view(np.uint8), first[k][perm].view(np.uint8)), k
    for at, e in enumerate(perm):
        for k in ("theta", "theta_thr", "variance"):
            assert np.array_equal(moved[k][cpm[at]:cpm[at + 1]].view(np.uint8), first[k][cp[e]:cp[e + 1]].view(np.uint8)), (k, e)
    for e in (3, 4, 17):      # alone in a batch
        alone, _, _, _ = _solve(device_solver, b.select(np.array([e])), opts, lds_limit=lds_limit)
        for k in STATS:
            assert alone[k][0] == first[k][e], (k, e)
        for k in ("theta", "theta_thr", "variance"):
            assert np.array_equal(alone[k].view(np.uint8), first[k][cp[e]:cp[e + 1]].view(np.uint8)), (k, e)


# 11 --------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lds_limit", [None, 0], ids=["wavefront", "workgroup"])
@pytest.mark.parametrize("mode", [1, 2], ids=["simple", "full"])
@pytest.mark.parametrize("loss", T.LOSSES)
def test_variances_at_the_returned_theta(device_solver, loss, mode, lds_limit):
    """SIMPLE (inside the solve kernels, from the D the solve holds) and FULL (gdmix_re_variance_full) against numpy at the device's theta:
    rtol 1e-7 and 1e-4, as the Poisson tests hold them."""
    pbs, _, _, b, v = T.case(loss, "free_intercept", "mixed")
    res, packed, _, _ = _solve(device_solver, b, _opts(loss, v, variance_mode=mode), lds_limit=lds_limit)
    cp = packed.coef_ptr_host()
    for e, pb in pbs.items():
        s = slice(int(cp[e]), int(cp[e + 1]))
        np.testing.assert_allclose(res["variance"][s], pb.variance(res["theta"][s], mode), rtol=1e-7 if mode == 1 else 1e-4, err_msg=f"entity {e}")


# 12 --------------------------------------------------------------------------------------------------------------------------------------
UNCHANGED = r'''
import sys
import numpy as np
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[2])
from gdmix_amd.solver import REDeviceSolver, SolverOptions
import re_l1_helpers as R
s = REDeviceSolver(0)
b = R.mixed_batch("logistic", "weights")
opts = SolverOptions(l2=1.0, loss="logistic", variance_mode=1)
packed = s.pack(b)
D = int(b.col_global.max()) + 1
bounds = s.upload_bounds(np.full(D, -0.05), np.full(D, 0.07))
KEYS = ("theta", "theta_thr", "variance", "fval", "gnorm", "nit", "nfev", "status")
def three():
    out = []
    for kw in ({}, {"l1": 0.5}, {"bounds": bounds}):
        out.append(s.solve(packed, opts, **kw).to_host())
    return out
before = three()      # before any solve_tron call in this process
tron = s.solve_tron(packed, opts).to_host()
assert tron["nhv"].sum() > 0 and np.all(tron["status"] >= 0)
after = three()
for x, y in zip(before, after):
    for k in KEYS:
        assert np.array_equal(x[k].view(np.uint8), y[k].view(np.uint8)), k
s.close()
print("UNCHANGED-OK")
'''


def test_the_other_solves_are_what_they_were_bit_for_bit(tmp_path):
    """gdmix_re_solve, the elastic net and the box solve on one packed batch before any solve_tron call in the process and after one on the
    same batch (the count record and `order` are shared): the same bits, in a process of its own so that `before` is before."""
    script = tmp_path / "unchanged.py"
    script.write_text(UNCHANGED)
    cp = subprocess.run([sys.executable, str(script), ROOT, os.path.join(ROOT, "tests")], capture_output=True, text=True, cwd=ROOT)
    assert cp.returncode == 0 and "UNCHANGED-OK" in cp.stdout, cp.stderr[-3000:]


# 13 --------------------------------------------------------------------------------------------------------------------------------------
def test_refusals_at_the_entry_point(device_solver):
    s = device_solver
    _, _, _, b, v = T.case("logistic", "plain", "mixed")
    packed = s.pack(b)
    out = s.alloc_result(packed)
    c_res = S._Result(*[None if out[k] is None else out[k].data_ptr() for k in ("theta", "theta_thr", "variance", "fval", "gnorm", "nit", "nfev", "status")])
    call = lambda pk, o: s.lib.gdmix_re_solve_tron(s._h, pk, C.byref(o), None, C.byref(c_res), None, s._stream())
    summed = SolverOptions(sum_loss=True).to_c()
    assert call(C.byref(packed.c), summed) == -1 and b"sum_loss" in s.lib.gdmix_re_last_error()
    bad = SolverOptions().to_c()
    bad.loss = 7
    assert call(C.byref(packed.c), bad) == -1
    assert call(None, SolverOptions().to_c()) == -1
    s.torch.cuda.synchronize()
    assert np.all(out["status"].cpu().numpy() == -1)      # the results were not touched
    with pytest.raises(S.GdmixReError, match="sum_loss"):
        s.solve_tron(packed, SolverOptions(sum_loss=True))
    assert s.tron_scratch_bytes(packed) >= s.lib.gdmix_re_solve_scratch_bytes(C.byref(packed.c), C.byref(SolverOptions().to_c()))


# 14 --------------------------------------------------------------------------------------------------------------------------------------
def _argv(root, action, extra):
    argv = H.job_argv(root, action, model_type="logistic_regression", extra=extra)
    return [a.replace("--regularize_bias=False", "--regularize_bias=True") for a in argv]


def test_the_stage_as_a_child_process(tmp_path):
    """`gdmix --stage=random_effect --entity_optimizer=TRON` on one partition of 60 entities next to the plain run of the same data, each
    stage a child process: the scores are x . theta + offset of the written model to 1 ulp of the Avro float; every coefficient is
    regularised, so the two runs' models lie within the strong-convexity bound taken at both runs' gradients (plus what the sparsity
    threshold may have removed from either); the metric files are there; inference with the flag gives the plain inference's bytes."""
    from gdmix_amd import chain
    from test_gpu_chain import _scores_by_uid, _ulps
    from test_gpu_re_l1 import _read_models, _theta_of
    b = H.small_job_batch(E=60, seed=42, real=False)
    roots = {k: str(tmp_path / k) for k in ("plain", "tron")}
    flags = {"plain": [], "tron": ["--entity_optimizer=TRON"]}
    for k in roots:
        H.write_job(roots[k], b)
        chain.run_stage(_argv(roots[k], "train", flags[k] + [f"--metric_output_dir={roots[k]}/metrics", "--random_effect_variance_mode=simple"]), True)
        assert os.path.exists(os.path.join(roots[k], "metrics", "evalSummary.json"))
    assert sorted(os.listdir(os.path.join(roots["tron"], "metrics"))) == sorted(os.listdir(os.path.join(roots["plain"], "metrics")))
    models = {k: _read_models(os.path.join(roots[k], "models", "part-00000.avro")) for k in roots}
    assert set(models["tron"]) == set(models["plain"]) == set(b.entity_ids)
    pbs = T.problems(("stage",), b, "logistic", T.VARIANTS["plain"], l2=1.0)
    worst = 0.0
    for e, pb in pbs.items():
        th = {k: _theta_of(models[k], b, e) for k in roots}
        g = {k: pb.smooth(th[k])[1] for k in roots}
        slack = T.THRESHOLD * np.sqrt(2.0 * th["tron"].size)      # a coefficient within the threshold of 0 is written as 0 in either file
        bound = (np.linalg.norm(g["tron"]) + np.linalg.norm(g["plain"])) / pb.l2 + slack
        dist = np.linalg.norm(th["tron"] - th["plain"])
        worst = max(worst, dist / bound)
        assert dist <= bound, (e, dist, bound)
    print(f"TRON's written models against the plain run's: worst distance / bound {worst:.3e}")
    order = np.argsort(b.uid, kind="stable")
    for d in ("trainingScores", "validationScores"):
        z = np.concatenate([pbs[e].X @ _theta_of(models["tron"], b, e) + pbs[e].off for e in range(b.E)]).astype(np.float32)
        s = _scores_by_uid(os.path.join(roots["tron"], d))
        assert np.array_equal(s["uid"], b.uid[order]) and _ulps(s["score"], z[order]).max() <= 1.0, d
    chain.run_stage(_argv(roots["tron"], "inference", ["--entity_optimizer=TRON"]), True)
    with_flag = _scores_by_uid(os.path.join(roots["tron"], "inferenceScores"))
    chain.run_stage(_argv(roots["tron"], "inference", []), True)
    without = _scores_by_uid(os.path.join(roots["tron"], "inferenceScores"))
    assert np.array_equal(with_flag["uid"], without["uid"]) and np.array_equal(with_flag["score"].view(np.uint32), without["score"].view(np.uint32))


# 15 --------------------------------------------------------------------------------------------------------------------------------------
CHAIN_BAR = 1e-4      # tests/test_gpu_chain.py holds the device chain's scores to 1e-4 max(1, |score|) of the free-running CPU chain's


def test_a_three_coordinate_chain_with_tron_on_both_random_effect_stages(tmp_path):
    from gdmix_amd import chain
    data = chain.make_dataset(300, 500, 20_000)
    bounds = {"per_user": 48}
    plain = chain.run_chain(str(tmp_path / "plain"), data, num_partitions=4, upper_bounds=bounds)
    tron = chain.run_chain(str(tmp_path / "tron"), data, num_partitions=4, upper_bounds=bounds, entity_optimizer="TRON")
    for stage in chain.STAGES[1:]:
        for k in ("train_auc", "validation_auc", "train_auc_device", "validation_auc_device"):
            print(f"{stage} {k}: plain {plain[stage][k]!r} TRON {tron[stage][k]!r}")
            assert abs(tron[stage][k] - plain[stage][k]) <= CHAIN_BAR, (stage, k)
