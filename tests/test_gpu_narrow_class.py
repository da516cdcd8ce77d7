"""The narrow kernel, re_solve_grp_kernel<16,5,24,96>: the entities of the class "re_solve_grp_kernel<32,3> n<=32 nnz<=128" with at most
80 coefficients, 24 samples and 96 non-zeros, four to a wavefront, the older half of the L-BFGS history in a per-lane ring
(csrc/re_solve_quad.hpp, quad_solve's KR; include/gdmix_re.h, gdmix_re_set_narrow). Every case is checked against oracle.solve with the
rules of tests/test_gpu_parity.py's _solve_and_compare (narrow_helpers.compare_with_oracle); the oracle has no Poisson loss, so that one
case is held to scipy by the rule of tests/re_poisson_helpers.py, like every other Poisson test of the suite."""
import numpy as np
import pytest

import narrow_helpers as nh
import re_linear_helpers as lh
import re_poisson_helpers as ph
from gdmix_amd import synthetic
from gdmix_amd.solver import SolverOptions
from oracle import oracle

pytestmark = pytest.mark.gpu

KW = dict(l2=1.0, regularize_bias=True, has_intercept=True, m=10, max_iter=100, ftol=1e-12)      # every entity well posed: all are compared


@pytest.fixture()
def solver(device_solver):
    device_solver.set_narrow(True)
    yield device_solver
    device_solver.set_narrow(True)


def _shape_of(packed, b, ic):
    return np.diff(packed.coef_ptr_host()), b.ent_n(), b.ent_nnz()


def _run(solver, b, kw, theta0=None):
    """Pack and solve b -> (packed, host result, oracle result, class counts, narrow count)."""
    packed = solver.pack(b, has_intercept=kw["has_intercept"])
    res = solver.solve(packed, SolverOptions(**kw), theta0=theta0).to_host()
    pk = oracle.pack(b.ent_row_ptr, b.row_nnz_ptr, b.col_global)
    ref = oracle.solve(pk, b.val, b.y, b.offset, b.weight, oracle.make_opts(**kw), theta0=theta0)
    return packed, res, ref, dict(solver.class_counts(packed)), solver.narrow_count(packed)


def test_edges_of_the_caps(solver):
    """p in {64, 65, 80, 81} x n in {1, 17, 24, 25} x nnz in {96, 97}: 32 entities. Narrow are exactly those inside the three caps (p = 65 or
    80, n <= 24, nnz = 96: six); p = 64 stays with <16,4>, the rest of the host class runs on <32,3> as before; all agree with the oracle."""
    shapes = [(p - 1, n, z) for p in (64, 65, 80, 81) for n in (1, 17, 24, 25) for z in (96, 97)]
    b = nh.make_shaped_batch(shapes, seed=11)
    packed, res, ref, counts, narrow = _run(solver, b, KW)
    p, n, z = _shape_of(packed, b, 1)
    assert np.array_equal(p, [s[0] + 1 for s in shapes]) and np.array_equal(n, [s[1] for s in shapes]) and np.array_equal(z, [s[2] for s in shapes])
    want = nh.is_narrow(p, n, z)
    assert int(want.sum()) == 6 and narrow == 6
    assert counts[nh.HOST_CLASS] == int((p > 64).sum()) == 24
    assert counts["re_solve_grp_kernel<16,4> n<=32 nnz<=128"] == 8
    # the narrow entities are the front of the class's segment of `order`, the others its back
    base = int(packed._view(packed.c.class_count, 2 * len(counts), solver.torch.int32).cpu().numpy()[len(counts) + list(counts).index(nh.HOST_CLASS)])
    order = packed._view(packed.c.order, packed.E, solver.torch.int32).cpu().numpy()
    assert sorted(order[base:base + 6].tolist()) == np.flatnonzero(want).tolist()
    assert sorted(order[base + 6:base + 24].tolist()) == np.flatnonzero((p > 64) & ~want).tolist()
    nh.compare_with_oracle(res, ref, packed.coef_ptr_host())


@pytest.mark.parametrize("size", [1, 2, 3, 5])
def test_ragged_wavefronts(solver, size):
    """1, 2, 3 and 5 narrow entities: the last (or only) wavefront has rows without an entity."""
    b = nh.make_shaped_batch(nh.narrow_shapes(np.random.default_rng(100 + size), size), seed=20 + size)
    packed, res, ref, counts, narrow = _run(solver, b, KW)
    assert narrow == size == counts[nh.HOST_CLASS]
    nh.compare_with_oracle(res, ref, packed.coef_ptr_host())


@pytest.mark.parametrize("m,l2", sorted(nh.HISTORY_CASES))
def test_history_beyond_the_registers(solver, m, l2):
    """Fits that run past the register-resident pairs and past ten pairs, with m = 3 (the ring is never read), 7 and 10. Two batches: four
    entities (one wavefront, whatever the order) and thirteen. First the conditions on the oracle's own run: an entity with nit >= 15,
    memory wraps, and in the four-entity wavefront entities whose nit differ by at least 5 (rows that finish while others go on pushing)."""
    kw = dict(KW, m=m, l2=l2)
    for E, seed in zip((4, 13), nh.HISTORY_CASES[(m, l2)]):
        b = nh.history_batch(E, seed)
        _, mx, spread, wraps = nh.history_conditions(b, kw)
        assert mx >= 15 and wraps > 0 and (E != 4 or spread >= 5), (E, mx, spread, wraps)
        packed, res, ref, counts, narrow = _run(solver, b, kw)
        assert narrow == E == counts[nh.HOST_CLASS]
        nh.compare_with_oracle(res, ref, packed.coef_ptr_host())


def _mixed_labels(b):
    y1 = np.add.reduceat(b.y, b.ent_row_ptr[:-1])
    return (y1 > 0) & (y1 < b.ent_n())


def test_without_intercept(solver):
    kw = dict(KW, has_intercept=False)
    b = nh.make_shaped_batch(nh.narrow_shapes(np.random.default_rng(31), 9, ic=0), seed=31)
    packed, res, ref, counts, narrow = _run(solver, b, kw)
    assert narrow == 9
    nh.compare_with_oracle(res, ref, packed.coef_ptr_host())


def test_with_weights_and_an_unregularised_intercept(solver):
    kw = dict(KW, regularize_bias=False)
    b = nh.make_shaped_batch(nh.narrow_shapes(np.random.default_rng(32), 9), seed=32, random_weights=True)
    packed, res, ref, counts, narrow = _run(solver, b, kw)
    assert narrow == 9
    wp = _mixed_labels(b)      # (an entity of one label has no minimiser under an unregularised intercept: SURVEY 8(d), class D)
    assert wp.sum() >= 5
    nh.compare_with_oracle(res, ref, packed.coef_ptr_host(), wp=wp)


def test_with_a_warm_start(solver):
    b = nh.make_shaped_batch(nh.narrow_shapes(np.random.default_rng(33), 9), seed=33)
    P = int(b.E + sum(len(np.unique(b.col_global[b.row_nnz_ptr[b.ent_row_ptr[e]]:b.row_nnz_ptr[b.ent_row_ptr[e + 1]]])) for e in range(b.E)))
    th0 = 0.3 * np.random.default_rng(34).standard_normal(P)
    packed, res, ref, counts, narrow = _run(solver, b, KW, theta0=th0)
    assert narrow == 9 and packed.P == P
    nh.compare_with_oracle(res, ref, packed.coef_ptr_host())


def test_with_simple_variance(solver):
    kw = dict(KW, variance_mode=1)
    b = nh.make_shaped_batch(nh.narrow_shapes(np.random.default_rng(35), 9), seed=35, random_weights=True)
    packed, res, ref, counts, narrow = _run(solver, b, kw)
    assert narrow == 9
    nh.compare_with_oracle(res, ref, packed.coef_ptr_host(), variance=True)


def test_with_the_squared_loss(solver):
    b = synthetic.with_real_labels(nh.make_shaped_batch(nh.narrow_shapes(np.random.default_rng(36), 9), seed=36), seed=36)
    kw = dict(KW, variance_mode=1)
    packed = solver.pack(b, has_intercept=True)
    res = solver.solve(packed, SolverOptions(linear=True, **kw)).to_host()
    assert solver.narrow_count(packed) == 9
    pk = oracle.pack(b.ent_row_ptr, b.row_nnz_ptr, b.col_global)
    ref = oracle.solve(pk, b.val, b.y, b.offset, b.weight, oracle.make_opts(**dict(kw, variance_mode=0), linear=True))
    nh.compare_with_oracle(res, ref, packed.coef_ptr_host())
    np.testing.assert_allclose(res["variance"], lh.variance_numpy(b, pk, kw, 1), rtol=1e-7)      # (D_i = 2 w_i: the oracle's variance is the logistic one)


def test_with_the_poisson_loss(solver):
    """Counts as labels; the reference is scipy on the Poisson objective (the oracle has no Poisson loss), compared by re_poisson_helpers'
    rule; SIMPLE variance against numpy at the device's theta."""
    b = synthetic.with_count_labels(nh.make_shaped_batch(nh.narrow_shapes(np.random.default_rng(37), 9), seed=37), seed=37)
    kw = dict(KW, variance_mode=1)
    packed = solver.pack(b, has_intercept=True)
    res = solver.solve(packed, SolverOptions(loss="poisson", **kw)).to_host()
    assert solver.narrow_count(packed) == 9
    pk = oracle.pack(b.ent_row_ptr, b.row_nnz_ptr, b.col_global)
    cp = packed.coef_ptr_host()
    ph.compare(res, ph.reference(b, pk, kw, None, cp, entities=np.arange(b.E)), cp)
    np.testing.assert_allclose(res["variance"], ph.variance_numpy(b, pk, kw, 1, res["theta"], cp), rtol=1e-7)


def test_switch(solver):
    """Off: no narrow entity, the class as before, results within REL_TOL_DEVICE of the narrow kernel's (and equal counts). On twice:
    bitwise equal. The batch mixes narrow entities with the rest of the host class."""
    rng = np.random.default_rng(41)
    shapes = nh.narrow_shapes(rng, 21) + [(85, 20, 90), (70, 30, 100), (66, 10, 120)]
    b = nh.make_shaped_batch(shapes, seed=41)
    packed = solver.pack(b, has_intercept=True)
    on1 = solver.solve(packed, SolverOptions(**KW)).to_host()
    assert solver.narrow_count(packed) == 21 and dict(solver.class_counts(packed))[nh.HOST_CLASS] == 24
    on2 = solver.solve(packed, SolverOptions(**KW)).to_host()
    for k in ("theta", "theta_thr", "fval", "gnorm", "nit", "nfev", "status"):
        assert np.array_equal(on1[k], on2[k]), k
    solver.set_narrow(False)
    off = solver.solve(packed, SolverOptions(**KW)).to_host()
    assert solver.narrow_count(packed) == 0 and dict(solver.class_counts(packed))[nh.HOST_CLASS] == 24
    for k in ("nit", "nfev", "status"):
        assert np.array_equal(on1[k], off[k]), k
    cp = packed.coef_ptr_host()
    err = max(np.max(np.abs(on1["theta"][cp[e]:cp[e + 1]] - off["theta"][cp[e]:cp[e + 1]])) / np.max(np.abs(off["theta"][cp[e]:cp[e + 1]])) for e in range(b.E))
    print(f"switch: worst theta rel difference on / off {err:.3e}")
    assert err <= nh.REL_TOL_DEVICE
    # the three entities outside the caps ran on <32,3> both times: bit for bit
    for e in (21, 22, 23):
        assert np.array_equal(on1["theta"][cp[e]:cp[e + 1]], off["theta"][cp[e]:cp[e + 1]])
