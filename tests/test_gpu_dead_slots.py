"""Dead coefficient slots of re_solve_grp_kernel (csrc/re_solve_quad.hpp, docs/kernels.md "Dead slots"): a slot j = gl + G s >= p of an
entity's G * EPL holds zeros in the registers and in the row's xs / xo / go arrays, and the trip runs over every slot without the bounds
test j < p. What can go wrong is a dead slot that is no zero (a sum, the maximum or a restored point picks it up) or a live one treated
as dead: entities with one live slot, one dead slot, one live lane in the last slot, none dead.

Classes: the six re_solve_grp_kernel instantiations the C2 benchmark launches (<16,2,16,64>, <16,3,16,64>, <16,4,16,64>, the narrow
<16,5,24,96>, <32,3,32,128>, <32,4,32,128>), <64,3,64,512>, two classes of more than a wavefront per entity (<128,3,128,1024>,
<128,3,1024,3072>) and <32,3,256,1024>. Per class, ONE batch of the entities with

    p = 1 (an intercept alone), 2, G (EPL - 1), G (EPL - 1) + 1 (one live lane in the last slot), G EPL - 1 and G EPL (no dead slot)

that the first-fit rule leaves in the class (re_classify_kernel takes the first class that holds an entity, so a class sees no p that
an earlier class takes: <16,3,16,64> gets 33, 47 and 48; all six reach <16,2,16,64> and the two classes of many samples, which are here
for that). n is the class's sample cap (24 for the narrow kernel), with one non-zero per sample or feature. The class every entity ran
in is read back from cls_tmp (and the narrow count for <16,5,24,96>, which shares a class index with <32,3,32,128>).

Every batch is held to the CPU reference by the rule of tests/test_gpu_class_caps.py for its loss — oracle.solve through
narrow_helpers.compare_with_oracle (logistic) and re_linear_helpers.judge (squared) on the entities the oracle reproduces under
re_linear_helpers.oracle_strict, scipy through re_poisson_helpers (Poisson): theta within 1e-7, equal status / nit / nfev, fval to rtol
1e-9 — and every entity of every batch is one the reference reproduces (asserted). Options: an intercept regularised or not, no
intercept, the three losses, a non-zero warm start.

Besides: rows of one wavefront that mix such entities, with an empty last row, give each entity the bits it gets alone; the golden
entities that take the line-search restart and the abnormal exit (both restore x and g from xo / go) in a kernel with 27 to 30 dead
slots of 32; an entity without samples next to others (the kernels divide by n)."""
import numpy as np
import pytest

import class_caps_helpers as ch
import narrow_helpers as nh
import re_linear_helpers as lh
import re_poisson_helpers as ph
from gdmix_amd import batch as gb
from gdmix_amd.solver import SolverOptions
from helpers import load_fixture, opts_kwargs, parity_mask, per_entity_rel_err
from oracle import oracle

pytestmark = pytest.mark.gpu

BITWISE = ("fval", "gnorm", "nit", "nfev", "status")
LOSS_OPTIONS = {"logistic": {}, "squared": dict(linear=True), "poisson": dict(loss="poisson")}
KW = dict(l2=1.0, regularize_bias=True, has_intercept=True, m=10, max_iter=100, ftol=1e-12)
# name -> (class index of cls_tmp, narrow, (G, EPL, NCAP, ZCAP))
CLASSES = {
    "16x2": (0, False, (16, 2, 16, 64)),
    "16x3": (3, False, (16, 3, 16, 64)),
    "16x4": (6, False, (16, 4, 16, 64)),
    "narrow": (9, True, (16, 5, 24, 96)),
    "32x3": (9, False, (32, 3, 32, 128)),
    "32x4": (12, False, (32, 4, 32, 128)),
    "64x3": (15, False, (64, 3, 64, 512)),
    "128x3": (19, False, (128, 3, 128, 1024)),
    "32x3_long": (11, False, (32, 3, 256, 1024)),
    "128x3_long": (20, False, (128, 3, 1024, 3072)),
}
# (the squared loss at l2 = 10, as the corners of tests/class_caps_helpers.py: at l2 = 1 its long runs on the classes of many samples move under
# rounding and the oracle does not reproduce them)
L2 = {"logistic": 1.0, "squared": 10.0, "poisson": 1.0}
# name -> (loss, has_intercept, regularize_bias, warm start)
CONFIGS = {
    "logistic": ("logistic", True, True, False),
    "logistic_free_intercept": ("logistic", True, False, False),
    "logistic_no_intercept": ("logistic", False, True, False),
    "logistic_warm": ("logistic", True, False, True),
    "squared": ("squared", True, True, False),
    "squared_no_intercept": ("squared", False, True, False),
    "poisson": ("poisson", True, True, False),
    "poisson_free_intercept": ("poisson", True, False, False),
    "poisson_no_intercept": ("poisson", False, True, False),
}


def first_fit(p, n, nnz):
    """-> (class index, narrow) by the rule of re_classify_kernel for m <= 10 with the tall rule off."""
    for k, (g, epl, ncap, zcap) in enumerate(ch.GROUP_CLASSES):
        if p <= g * epl and n <= ncap and nnz <= zcap:
            return k, bool(k == 9 and nh.is_narrow(p, n, nnz))
    return ch.BLOCK_CLASS, False


def shapes_of(name, ic):
    """[(p, n, nnz)] of the class's batch: the six p of the module docstring that the first-fit rule leaves in it."""
    k, narrow, (g, epl, ncap, zcap) = CLASSES[name]
    assert narrow or ch.GROUP_CLASSES[k] == (g, epl, ncap, zcap)
    out = []
    for p in sorted({1, 2, g * (epl - 1), g * (epl - 1) + 1, g * epl - 1, g * epl}):
        d = p - ic
        if d < 0 or (d == 0 and not ic):
            continue
        n = ncap
        z = max(d, n) if d else 0
        if z <= zcap and first_fit(p, n, z) == (k, narrow):
            out.append((p, n, z))
    assert len(out) >= 3 and out[-1][0] == g * epl and any(s[0] == g * (epl - 1) + 1 for s in out), (name, out)
    return out


def empty_entity(n, seed, y=None):
    """An entity of n samples without a non-zero (d = 0: an intercept alone). Labels alternate, so both occur."""
    rng = np.random.default_rng([seed, 0x5E])
    return gb.RawBatch(ent_row_ptr=np.array([0, n]), row_nnz_ptr=np.zeros(n + 1, np.int64), col_global=np.zeros(0, np.int64),
                       val=np.zeros(0, np.float32), y=(np.arange(n) % 2 == 0).astype(np.float32) if y is None else y,
                       offset=rng.standard_normal(n).astype(np.float32), weight=None, uid=np.arange(n, dtype=np.int64) + 10 ** 6, entity_ids=["empty"])


_BATCHES = {}


def make_batch(name, loss, ic):
    key = (name, loss, ic)
    if key not in _BATCHES:
        shapes = shapes_of(name, ic)
        seed = 11 + 1000 * list(CLASSES).index(name) + 100 * ch.LOSSES.index(loss) + 10 * ic
        full = [s for s in shapes if s[2] > 0]
        b = nh.make_shaped_batch([(p - ic, n, z) for p, n, z in full], seed=seed, D=ch.D)
        if len(full) < len(shapes):      # p = 1 with an intercept: in front, as the shapes are sorted by p
            assert shapes[0][0] == 1 and len(full) == len(shapes) - 1
            b = gb.concat([empty_entity(shapes[0][1], seed), b])
        assert b.E == len(shapes) and np.array_equal(b.ent_n(), [s[1] for s in shapes]) and np.array_equal(b.ent_nnz(), [s[2] for s in shapes])
        _BATCHES[key] = (shapes, ch._with_labels(b, loss, seed))
    return _BATCHES[key]


def reference_and_compare(b, loss, kw, res, cp, th0=None):
    """The solve against the CPU reference, by the loss's rule of tests/test_gpu_class_caps.py; every entity must be one it compares."""
    pk = oracle.pack(b.ent_row_ptr, b.row_nnz_ptr, b.col_global)
    assert np.array_equal(cp, pk["ent_feat_ptr"] + np.arange(b.E + 1) * int(kw["has_intercept"]))
    if loss == "poisson":
        ref = ph.reference(b, pk, kw, th0, cp, entities=np.arange(b.E))
        assert (ref["strict"] & (ref["status"] != 1)).all(), (ref["strict"], ref["status"])
        ph.compare(res, ref, cp)
    elif loss == "squared":
        j = lh.judge(b, pk, dict(kw, variance_mode=0), th0, res, cp, theta_tol=nh.REL_TOL_DEVICE)
        assert not j["problems"], j["problems"][:3]
        ok, ref = j["strict_ok"], j["ref"]
        print(f"squared compare: {int(ok.sum())} of {b.E} strict and not flagged, worst theta error {float(j['err'].max()):.3e}")
        assert j["strict"].all() and ok.all(), (j["strict"], j["adjudicated"][:3])
        for k in ("status", "nit", "nfev"):
            assert np.array_equal(res[k], ref[k]), k
        assert j["err"].max() <= nh.REL_TOL_DEVICE
        np.testing.assert_allclose(res["fval"], ref["fval"], rtol=1e-9, atol=1e-13)
    else:
        ref, strict, _, _ = lh.oracle_strict(b, pk, oracle.make_opts(**dict(kw, variance_mode=0)), th0, int(cp[-1]))
        assert strict.all(), strict
        nh.compare_with_oracle(res, ref, cp, wp=strict)


@pytest.fixture()
def solver(device_solver):
    """The narrow kernel on, the tall rule off (entities of p <= 64 and 32 samples or more stay in their group class)."""
    device_solver.set_narrow(True)
    lh.set_routing(device_solver, tall_min_n=0)
    yield device_solver
    lh.reset_routing(device_solver)
    device_solver.set_narrow(True)


def _solve(solver, b, kw, loss="logistic", th0=None):
    packed = solver.pack(b, has_intercept=kw["has_intercept"])
    res = solver.solve(packed, SolverOptions(**kw, **LOSS_OPTIONS[loss]), theta0=th0).to_host()
    cls = packed._view(packed.c.cls_tmp, packed.E, solver.torch.int32).cpu().numpy().copy()
    return packed, res, cls, solver.narrow_count(packed)


def _same_bits(a, cpa, ea, b, cpb, eb):
    """Entity ea of result a and entity eb of result b: every output bit for bit."""
    sa, sb = slice(int(cpa[ea]), int(cpa[ea + 1])), slice(int(cpb[eb]), int(cpb[eb + 1]))
    for k in ("theta", "theta_thr"):
        assert np.array_equal(a[k][sa], b[k][sb]), (k, ea, eb)
    for k in BITWISE:
        assert a[k][ea] == b[k][eb], (k, ea, eb, a[k][ea], b[k][eb])


@pytest.mark.parametrize("config", list(CONFIGS))
@pytest.mark.parametrize("name", list(CLASSES))
def test_dead_slots(solver, name, config):
    k, narrow, _ = CLASSES[name]
    loss, has_ic, reg_bias, warm = CONFIGS[config]
    shapes, b = make_batch(name, loss, int(has_ic))
    kw = dict(KW, has_intercept=has_ic, regularize_bias=reg_bias, l2=L2[loss])
    P = int(sum(s[0] for s in shapes))
    th0 = 0.1 * np.random.default_rng([5, list(CLASSES).index(name)]).standard_normal(P) if warm else None
    packed, res, cls, nnarrow = _solve(solver, b, kw, loss, th0)
    cp = packed.coef_ptr_host()
    assert np.array_equal(np.diff(cp), [s[0] for s in shapes])
    assert np.all(cls == k) and nnarrow == (b.E if narrow else 0), (cls, nnarrow)
    reference_and_compare(b, loss, kw, res, cp, th0)


@pytest.mark.parametrize("name", ["16x2", "16x3", "narrow", "32x3"])
def test_rows_of_a_wavefront(solver, name):
    """Entities with dead slots and a full one in the rows of one wavefront, the last wavefront with an empty row: each entity gets the
    bits it gets as a batch of its own (where the other rows of its wavefront are empty)."""
    k, narrow, (g, _, _, _) = CLASSES[name]
    shapes, b = make_batch(name, "logistic", 1)
    assert b.E % (64 // g) != 0 and shapes[-1][0] == CLASSES[name][2][0] * CLASSES[name][2][1]
    packed, res, cls, nnarrow = _solve(solver, b, KW)
    cp = packed.coef_ptr_host()
    assert np.all(cls == k) and nnarrow == (b.E if narrow else 0)
    for e in range(b.E):
        _, one, cls_1, _ = _solve(solver, b.select([e]), KW)
        assert np.all(cls_1 == k)
        _same_bits(res, cp, e, one, np.array([0, cp[e + 1] - cp[e]]), 0)


@pytest.mark.parametrize("fixture,counter", [("exit_extreme_02", "maxls_aborts"), ("exit_extreme_03", "gd_restarts")])
def test_restart_and_abnormal_exit(solver, fixture, counter):
    """The golden entities of extreme inputs: p <= 5 in <16,2,16,64>, 27 and more of their 32 slots dead. Those the reference reproduces
    take the line-search restart (20 evaluations without a step: `maxls_aborts`; a direction that does not descend: `gd_restarts`) and
    the abnormal exit (status 4), which put x and g back from xo / go. Held to the reference's own recorded run as
    tests/test_gpu_parity.py holds them."""
    b, opts, exp, _ = load_fixture(fixture)
    kw = opts_kwargs(opts)
    wp = parity_mask(b, opts, exp)
    assert not np.any(exp["theta0"]) and kw["variance_mode"] == 0
    strict = b.select(np.flatnonzero(wp))
    pk = oracle.pack(strict.ent_row_ptr, strict.row_nnz_ptr, strict.col_global)
    oracle.branch_counts(reset=True)
    oracle.solve(pk, strict.val, strict.y, strict.offset, strict.weight, oracle.make_opts(**kw))
    assert oracle.branch_counts(reset=True)[counter] > 0 and np.any(exp["status"][wp] == 4)
    packed, res, cls, _ = _solve(solver, b, kw)
    cp = packed.coef_ptr_host()
    assert np.all(cls == 0) and np.diff(cp).max() <= 5
    assert np.all(res["status"] >= 0)
    err = per_entity_rel_err(res["theta"], exp["theta"], cp)
    print(f"{fixture}: {int(wp.sum())} entities compared, {int((exp['status'][wp] == 4).sum())} with status 4, worst theta error {err[wp].max():.3e}")
    for key in ("status", "nit", "nfev"):
        assert np.array_equal(res[key][wp], exp[key][wp]), key
    assert err[wp].max() <= nh.REL_TOL_DEVICE
    fv = wp & (exp["status"] != 4)      # (f after the abnormal exit: scipy's driver reports the last trial's, tests/test_oracle_golden.py)
    np.testing.assert_allclose(res["fval"][fv], exp["fval"][fv], rtol=1e-9, atol=1e-13)


@pytest.mark.parametrize("ic", [1, 0], ids=["intercept", "no_intercept"])
def test_an_entity_without_samples(solver, ic):
    """n = 0 (the pack takes such an entity): no column, p = ic, and 1 / n = inf. Its gradient is inf * 0 in the intercept's slot alone
    and 0 in every dead slot, so the largest |g| over the row comes out 0 and the solve stops at its start: status 0, no iteration, one
    evaluation, theta = 0, f = inf * 0. The entities around it (the same wavefront) are the bits they are without it."""
    shapes, full = make_batch("16x2", "logistic", ic)
    none = empty_entity(0, 3)
    b = gb.concat([full.select([0, 1]), none, full.select(np.arange(2, full.E))])
    kw = dict(KW, has_intercept=bool(ic))
    packed, res, cls, _ = _solve(solver, b, kw)
    cp = packed.coef_ptr_host()
    assert np.all(cls == 0) and cp[3] - cp[2] == ic and b.ent_n()[2] == 0
    assert (res["status"][2], res["nit"][2], res["nfev"][2], res["gnorm"][2]) == (0, 0, 1, 0.0) and np.isnan(res["fval"][2])
    assert np.all(res["theta"][cp[2]:cp[3]] == 0.0) and np.all(res["theta_thr"][cp[2]:cp[3]] == 0.0)
    _, ref, _, _ = _solve(solver, full, kw)
    cpf = ref_cp = np.concatenate([[0], np.cumsum([s[0] for s in shapes])])
    for e in range(full.E):
        _same_bits(res, cp, e if e < 2 else e + 1, ref, cpf, e)
    assert ref_cp[-1] + ic == cp[-1]
