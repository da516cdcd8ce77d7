"""The staging of re_solve_grp_kernel (csrc/re_solve.hip, docs/kernels.md "Staging"): an entity's block comes in by rounds of predicated
loads whose trip counts are the class's caps, so what can go wrong is a load or a store on the wrong side of its own bound — an entity
of one sample, one without a non-zero, one exactly on the caps, a wavefront with empty slots, the entity whose block ends on the last
element of every array of the batch.

For each class the C2 benchmark launches (<16,2,16,64>, <16,3,16,64>, <16,4,16,64>, the narrow <16,5,24,96>, <32,3,32,128>, <32,4,32,128>)
and for one class of more than a wavefront per entity (<128,3,128,1024>), for the three losses, with and without an intercept, with and
without a weight column, ONE batch of three entities (five for <16,2,16,64> with an intercept):

    the smallest member of the class: one sample, the lowest p the class takes, one non-zero per feature. For <16,2,16,64> that is the
        entity of one sample and one non-zero; no other class can hold that entity (it has p <= 2, and p decides the class), nor the next:
    (<16,2,16,64> with an intercept only: p = 1) an entity of three samples and no non-zero at all, and a second one-sample entity;
    a middle one: odd n and nnz, a last lane that is partly filled;
    the corner (p, n, nnz) = the caps, LAST: its staging ends on the last element of every input array.

Three or five entities are no multiple of the four (two) entities of a workgroup: the last workgroup has empty slots. The class every
entity ran in is read back from cls_tmp (and the narrow count for <16,5,24,96>, which shares a class with <32,3,32,128>). The batch is
solved a second time with its entities in reversed order — the corner first, the smallest last — and as a batch of the corner alone:
every per-entity result is bit for bit the first solve's.

The first solve is held to the CPU reference by the rule of tests/test_gpu_class_caps.py for the loss: oracle.solve through
narrow_helpers.compare_with_oracle (logistic) and re_linear_helpers.judge (squared) on the entities the oracle reproduces under
re_linear_helpers.oracle_strict — every entity of every batch here, asserted —, theta within 1e-7, equal status / nit / nfev, fval to
rtol 1e-9; oracle/ has no Poisson loss, so that loss is held to scipy by re_poisson_helpers, as in every Poisson test of the suite."""
import numpy as np
import pytest

import class_caps_helpers as ch
import narrow_helpers as nh
import re_linear_helpers as lh
import re_poisson_helpers as ph
from gdmix_amd import batch as gb
from gdmix_amd.solver import SolverOptions
from oracle import oracle

pytestmark = pytest.mark.gpu

BITWISE = ("fval", "gnorm", "nit", "nfev", "status")
LOSS_OPTIONS = {"logistic": {}, "squared": dict(linear=True), "poisson": dict(loss="poisson")}
KW = dict(l2=1.0, regularize_bias=True, has_intercept=True, m=10, max_iter=100, ftol=1e-12)      # every entity well posed
# name -> (class index of cls_tmp, narrow, (G, EPL, NCAP, ZCAP), lowest p, highest p)
CLASSES = {
    "16x2": (0, False, (16, 2, 16, 64), 1, 32),
    "16x3": (3, False, (16, 3, 16, 64), 33, 48),
    "16x4": (6, False, (16, 4, 16, 64), 49, 64),
    "narrow": (9, True, (16, 5, 24, 96), 65, 80),
    "32x3": (9, False, (32, 3, 32, 128), 81, 96),
    "32x4": (12, False, (32, 4, 32, 128), 97, 128),
    "128x3": (19, False, (128, 3, 128, 1024), 257, 384),
}


def shapes_of(name, ic):
    """[(p, n, nnz)] of the batch, in forward order (see the module docstring); p counts the intercept."""
    k, narrow, (g, epl, ncap, zcap), lo, cap = CLASSES[name]
    assert cap == g * epl and (narrow or ch.GROUP_CLASSES[k] == (g, epl, ncap, zcap))
    p0 = max(lo, 1 + ic)
    small = (p0, 1, p0 - ic)
    pm = (lo + cap) // 2
    nm = (ncap // 2) | 1
    mid = (pm, nm, min(((max(pm - ic, nm) + zcap) // 2) | 1, zcap))
    out = [small, mid, (cap, ncap, zcap)]
    if name == "16x2" and ic:
        out = [(1, 3, 0), small] + out
    for p, n, z in out:
        assert ch.route(p, n, z, KW["m"], False, 32, ic=ic) == k, (name, p, n, z)      # (32: the library's default tall rule)
        assert bool(nh.is_narrow(p, n, z)) == narrow, (name, p, n, z)
    return out


def make_batch(name, loss, ic, weights):
    shapes = shapes_of(name, ic)
    seed = 7 + 1000 * list(CLASSES).index(name) + 100 * ch.LOSSES.index(loss) + 10 * ic + int(weights)
    full = [s for s in shapes if s[2] > 0]
    b = nh.make_shaped_batch([(p - ic, n, z) for p, n, z in full], seed=seed, D=ch.D, random_weights=weights)
    if len(full) < len(shapes):      # the entity without a non-zero goes in front
        rng = np.random.default_rng([seed, 0x5E])
        n = shapes[0][1]
        empty = gb.RawBatch(ent_row_ptr=np.array([0, n]), row_nnz_ptr=np.zeros(n + 1, np.int64), col_global=np.zeros(0, np.int64),
                            val=np.zeros(0, np.float32), y=np.array([1, 0, 1][:n], np.float32), offset=rng.standard_normal(n).astype(np.float32),
                            weight=(0.25 + 2.0 * rng.random(n)).astype(np.float32) if weights else None, uid=np.arange(n, dtype=np.int64) + 10 ** 6,
                            entity_ids=["empty"])
        b = gb.concat([empty, b])
    assert b.E == len(shapes) and np.array_equal(b.ent_n(), [s[1] for s in shapes]) and np.array_equal(b.ent_nnz(), [s[2] for s in shapes])
    return shapes, ch._with_labels(b, loss, seed)


def reference_and_compare(b, loss, kw, res, cp):
    """The first solve against the CPU reference, by the loss's rule of tests/test_gpu_class_caps.py; every entity must be compared."""
    pk = oracle.pack(b.ent_row_ptr, b.row_nnz_ptr, b.col_global)
    assert np.array_equal(cp, pk["ent_feat_ptr"] + np.arange(b.E + 1) * int(kw["has_intercept"]))
    if loss == "poisson":
        ref = ph.reference(b, pk, kw, None, cp, entities=np.arange(b.E))
        assert (ref["strict"] & (ref["status"] != 1)).all(), (ref["strict"], ref["status"])
        ph.compare(res, ref, cp)
    elif loss == "squared":
        j = lh.judge(b, pk, dict(kw, variance_mode=0), None, res, cp, theta_tol=nh.REL_TOL_DEVICE)
        assert not j["problems"], j["problems"][:3]
        ok, ref = j["strict_ok"], j["ref"]
        print(f"squared compare: {int(ok.sum())} of {b.E} strict and not flagged, worst theta error {float(j['err'].max()):.3e}")
        assert j["strict"].all() and ok.all(), (j["strict"], j["adjudicated"][:3])
        for k in ("status", "nit", "nfev"):
            assert np.array_equal(res[k], ref[k]), k
        assert j["err"].max() <= nh.REL_TOL_DEVICE
        np.testing.assert_allclose(res["fval"], ref["fval"], rtol=1e-9, atol=1e-13)
    else:
        ref, strict, _, _ = lh.oracle_strict(b, pk, oracle.make_opts(**dict(kw, variance_mode=0)), None, int(cp[-1]))
        assert strict.all(), strict
        nh.compare_with_oracle(res, ref, cp, wp=strict)


@pytest.fixture()
def solver(device_solver):
    device_solver.set_narrow(True)
    lh.reset_routing(device_solver)
    yield device_solver
    device_solver.set_narrow(True)


def _solve(solver, b, kw, loss):
    packed = solver.pack(b, has_intercept=kw["has_intercept"])
    res = solver.solve(packed, SolverOptions(**kw, **LOSS_OPTIONS[loss])).to_host()
    cls = packed._view(packed.c.cls_tmp, packed.E, solver.torch.int32).cpu().numpy().copy()
    return packed, res, cls, solver.narrow_count(packed)


def _same_bits(a, cpa, ea, b, cpb, eb):
    """Entity ea of result a and entity eb of result b: every output bit for bit."""
    sa, sb = slice(int(cpa[ea]), int(cpa[ea + 1])), slice(int(cpb[eb]), int(cpb[eb + 1]))
    for k in ("theta", "theta_thr"):
        assert np.array_equal(a[k][sa], b[k][sb]), (k, ea, eb)
    for k in BITWISE:
        assert a[k][ea] == b[k][eb], (k, ea, eb, a[k][ea], b[k][eb])


@pytest.mark.parametrize("weights", [False, True], ids=["unit", "weights"])
@pytest.mark.parametrize("ic", [1, 0], ids=["intercept", "no_intercept"])
@pytest.mark.parametrize("loss", ch.LOSSES)
@pytest.mark.parametrize("name", list(CLASSES))
def test_staging(solver, name, loss, ic, weights):
    k, narrow, _, _, _ = CLASSES[name]
    shapes, b = make_batch(name, loss, ic, weights)
    kw = dict(KW, has_intercept=bool(ic))
    E = b.E
    packed, res, cls, nnarrow = _solve(solver, b, kw, loss)
    cp = packed.coef_ptr_host()
    assert np.array_equal(np.diff(cp), [s[0] for s in shapes])
    assert np.all(cls == k) and nnarrow == (E if narrow else 0), (cls, nnarrow)
    reference_and_compare(b, loss, kw, res, cp)
    # the entities in reversed order: the corner first, the smallest last
    _, rev, cls_r, narrow_r = _solve(solver, b.select(np.arange(E)[::-1]), kw, loss)
    assert np.all(cls_r == k) and narrow_r == nnarrow
    cpr = np.concatenate([[0], np.cumsum(np.diff(cp)[::-1])])
    for e in range(E):
        _same_bits(res, cp, e, rev, cpr, E - 1 - e)
    # the corner alone: a batch of one entity
    _, one, cls_1, narrow_1 = _solve(solver, b.select([E - 1]), kw, loss)
    assert np.all(cls_1 == k) and narrow_1 == (1 if narrow else 0)
    _same_bits(res, cp, E - 1, one, np.array([0, cp[E] - cp[E - 1]]), 0)
