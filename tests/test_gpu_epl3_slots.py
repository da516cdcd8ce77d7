"""The EPL = 3 group kernels at their slot edges and the narrow kernel's ring at its own (csrc/re_solve_quad.hpp; docs/kernels.md "Dead slots"
and "The narrow kernel and the split history"; profiles/grp_epl3_slots.txt).

EPL = 3, <16,3,16,64> and <32,3,32,128>: the restore of x and g at a line search's restart keeps its bounds test in these kernels (what
the register allocation of the two-loop steps hangs on), every other slot loop runs without one. Entities with no dead slot (p = 3 G),
with exactly one live lane in slot 2 (p = 2 G + 1) and one lane short of full, alone in a wavefront's first row and next to a full
entity, so that the rows of a wavefront finish at different trips. p = 2 G (slot 2 wholly dead) and p = 1 cannot be put into these two
kernels: the first-fit rule hands every p <= 2 G to a class in front of them at any sample count (`test_what_the_first_fit_rule_leaves`
holds that to the table); tests/test_gpu_dead_slots.py runs those p where they land.

Narrow kernel <16,5,24,96> (KR = 5 pairs in registers, the older five in a ring indexed by stored per-pair offsets that move only when
a pair is stored): an entity at the three caps; runs cut by max_iter at nit = KR and KR + 1 (nothing stored, the ring unread: a push
stores only when it finds KR pairs, and iteration nit pushes none), KR + 2 (one pair stored and read once) and free runs of 2 KR + 2
iterations and more (the ring wrapped); a wavefront of four entities of which exactly one has more than KR pairs (three rows idle in
every ring step); m = 3 (no pair is stored). Each of these for the three losses, with and without an intercept. The seeds below are the
first at which the REFERENCE's own run gives those iteration counts; the tests assert them on the reference before they compare.

Every solve is held to the CPU reference by the rule of tests/test_gpu_class_caps.py for its loss: theta within 1e-7, equal status / nit /
nfev, fval to rtol 1e-9, on entities the reference reproduces — all of them (asserted)."""
import numpy as np
import pytest

import class_caps_helpers as ch
import narrow_helpers as nh
import re_linear_helpers as lh
import re_poisson_helpers as ph
from gdmix_amd.solver import SolverOptions
from oracle import oracle

KR = 5                      # GDMIX_NARROW_KR (csrc/re_solve.hip)
NARROW_CLASS = 9            # the narrow kernel shares the class index of <32,3,32,128>
LOSS_OPTIONS = {"logistic": {}, "squared": dict(linear=True), "poisson": dict(loss="poisson")}
L2 = {"logistic": 1.0, "squared": 10.0, "poisson": 1.0}      # (the squared loss at 10, as the corners of class_caps_helpers)
KW = dict(l2=1.0, regularize_bias=True, has_intercept=True, m=10, max_iter=100, ftol=1e-12)
# name -> (class index, (G, EPL, NCAP, ZCAP), n of the entities: the class's cap, which for <32,3,32,128> also keeps them out of the narrow kernel)
EPL3 = {"16x3": (3, (16, 3, 16, 64), 16), "32x3": (9, (32, 3, 32, 128), 32)}
SEED_EPL3 = 21
SEED_CAPS = 3
# the ring tests: l2 at which the reference's free runs are long enough (9 iterations and more in every entity, 2 KR + 2 and more in one)
RING_L2 = {"logistic": 1e-3, "squared": 1.0, "poisson": 1.0}
SEED_RING = 4
# (loss, intercept) -> (seed, l2) of the wavefront with one long row. Poisson with an intercept at l2 = 10: at 1 the three scaled entities
# still take 6 to 10 iterations to place their intercept (seeds 1 .. 24 tried on the reference)
SEED_MIXED = {(loss, ic): (1, L2[loss]) for loss in ch.LOSSES for ic in (1, 0)}
SEED_MIXED["poisson", 1] = (1, 10.0)
SEED_M3 = 6


def first_fit(p, n, nnz):
    for k, (g, epl, ncap, zcap) in enumerate(ch.GROUP_CLASSES):
        if p <= g * epl and n <= ncap and nnz <= zcap:
            return k
    return ch.BLOCK_CLASS


def epl3_shapes(name, ic):
    """[(p, n, nnz)]: a wavefront of its own per tested p (the entity in the first row, the other rows empty or full entities), then
    wavefronts that mix them. <16,3>: four rows per wavefront; <32,3>: two."""
    k, (g, epl, ncap, zcap), n = EPL3[name]
    full, one, short = g * epl, g * (epl - 1) + 1, g * epl - 1
    rows = 64 // g
    order = []
    for p in (full, one, short):
        order += [p] + [full] * (rows - 1)      # next to full entities
    order += [one, short, full, one][:rows] + [one]      # mixed, and a last wavefront with empty rows
    out = []
    for p in order:
        d = p - ic
        z = max(d, n)
        assert z <= zcap and first_fit(p, n, z) == k and not nh.is_narrow(p, n, z), (name, p)
        out.append((p, n, z))
    return out


_PLANS = {}


def plan(key, shapes, seed, loss, kw, scale=None):
    """The batch of `shapes` [(p, n, nnz)] and the reference's own run of it, once per key. scale: per-entity power of two the feature
    values are multiplied by (exact in fp32)."""
    if key not in _PLANS:
        ic = int(kw["has_intercept"])
        b = nh.make_shaped_batch([(p - ic, n, z) for p, n, z in shapes], seed=seed, D=ch.D)
        if scale is not None:
            per_nz = np.repeat(np.asarray(scale, np.float32), b.ent_nnz())
            b.val[:] = b.val * per_nz
        b = ch._with_labels(b, loss, seed)
        pk = oracle.pack(b.ent_row_ptr, b.row_nnz_ptr, b.col_global)
        cp = pk["ent_feat_ptr"] + np.arange(b.E + 1) * ic
        assert np.array_equal(np.diff(cp), [s[0] for s in shapes])
        if loss == "poisson":
            ref = ph.reference(b, pk, kw, None, cp, key=("epl3_slots", key), entities=np.arange(b.E))
            strict = ref["strict"] & (ref["status"] != 1)
        elif loss == "squared":
            ref, strict, _, _ = lh.oracle_strict(b, pk, oracle.make_opts(**dict(kw, variance_mode=0, linear=True, sum_loss=False)), None, int(cp[-1]))
        else:
            ref, strict, _, _ = lh.oracle_strict(b, pk, oracle.make_opts(**dict(kw, variance_mode=0)), None, int(cp[-1]))
        _PLANS[key] = dict(b=b, pk=pk, cp=cp, ref=ref, strict=np.asarray(strict), nit=np.asarray(ref["nit"]))
    return _PLANS[key]


def compare(pl, loss, kw, res):
    assert pl["strict"].all(), pl["strict"]
    if loss == "poisson":
        ph.compare(res, pl["ref"], pl["cp"])
    elif loss == "squared":
        j = lh.judge(pl["b"], pl["pk"], dict(kw, variance_mode=0), None, res, pl["cp"], theta_tol=nh.REL_TOL_DEVICE)
        assert not j["problems"] and j["strict_ok"].all(), (j["problems"][:3], j["adjudicated"][:3])
        for k in ("status", "nit", "nfev"):
            assert np.array_equal(res[k], j["ref"][k]), k
        assert j["err"].max() <= nh.REL_TOL_DEVICE
        np.testing.assert_allclose(res["fval"], j["ref"]["fval"], rtol=1e-9, atol=1e-13)
    else:
        nh.compare_with_oracle(res, pl["ref"], pl["cp"], wp=pl["strict"])


@pytest.fixture()
def solver(device_solver):
    device_solver.set_narrow(True)
    lh.set_routing(device_solver, tall_min_n=0)
    yield device_solver
    lh.reset_routing(device_solver)
    device_solver.set_narrow(True)


def _solve(solver, b, kw, loss="logistic"):
    packed = solver.pack(b, has_intercept=kw["has_intercept"])
    res = solver.solve(packed, SolverOptions(**kw, **LOSS_OPTIONS[loss])).to_host()
    cls = packed._view(packed.c.cls_tmp, packed.E, solver.torch.int32).cpu().numpy().copy()
    return res, cls, solver.narrow_count(packed)


def epl3_plan(name, loss, ic):
    kw = dict(KW, has_intercept=bool(ic), l2=L2[loss])
    return kw, plan(("epl3", name, loss, ic), epl3_shapes(name, ic), SEED_EPL3 + 10 * ch.LOSSES.index(loss) + ic, loss, kw)


def narrow_shapes(seed, count, full=False):
    if full:
        return [(nh.NARROW_P, nh.NARROW_N, nh.NARROW_NNZ)] * count
    return [(d + 1, n, z) for d, n, z in nh.narrow_shapes(np.random.default_rng([seed, 0x4E]), count)]


def ring_plan(loss, ic, max_iter):
    kw = dict(KW, has_intercept=bool(ic), l2=RING_L2[loss], max_iter=max_iter)
    return kw, plan(("ring", loss, ic, max_iter), narrow_shapes(SEED_RING, 5), SEED_RING, loss, kw)


def mixed_plan(loss, ic):
    """Four entities, one wavefront: the features of the first three are scaled by 1 / 64, which leaves them little to fit."""
    seed, l2 = SEED_MIXED[loss, ic]
    kw = dict(KW, has_intercept=bool(ic), l2=l2)
    return kw, plan(("mixed", loss, ic, seed), narrow_shapes(seed, 4), seed, loss, kw, scale=[1 / 64, 1 / 64, 1 / 64, 1.0])


def short_memory_plan(loss, ic):
    kw = dict(KW, has_intercept=bool(ic), l2=RING_L2[loss], m=3)
    return kw, plan(("m3", loss, ic), narrow_shapes(SEED_M3, 5), SEED_M3, loss, kw)


def test_what_the_first_fit_rule_leaves():
    """p = 2 G and p = 1 reach neither EPL = 3 kernel of the C2 step: a class in front of it holds p <= 2 G at the same sample and non-zero
    caps, so it takes every entity of those p that the kernel could hold. Held to the class table, and to the rule over every (n, nnz)."""
    for name, (k, (g, epl, ncap, zcap), _) in EPL3.items():
        assert any(g0 * e0 >= 2 * g and n0 >= ncap and z0 >= zcap for g0, e0, n0, z0 in ch.GROUP_CLASSES[:k]), name
        for p in (1, 2 * g):
            assert all(first_fit(p, n, z) < k for n in range(1, ncap + 1) for z in range(max(p - 1, n), zcap + 1)), (name, p)


@pytest.mark.gpu
@pytest.mark.parametrize("ic", [1, 0], ids=["intercept", "no_intercept"])
@pytest.mark.parametrize("loss", list(ch.LOSSES))
@pytest.mark.parametrize("name", list(EPL3))
def test_epl3_slots(solver, name, loss, ic):
    kw, pl = epl3_plan(name, loss, ic)
    res, cls, nnarrow = _solve(solver, pl["b"], kw, loss)
    assert np.all(cls == EPL3[name][0]) and nnarrow == 0, (cls, nnarrow)
    rows = 64 // EPL3[name][1][0]
    if loss == "logistic" and rows > 1:
        assert any(len(set(pl["nit"][w:w + rows].tolist())) > 1 for w in range(0, pl["b"].E, rows)), pl["nit"]      # rows that finish at different trips
    compare(pl, loss, kw, res)


@pytest.mark.gpu
@pytest.mark.parametrize("ic", [1, 0], ids=["intercept", "no_intercept"])
@pytest.mark.parametrize("loss", list(ch.LOSSES))
def test_narrow_caps(solver, loss, ic):
    kw = dict(KW, has_intercept=bool(ic), l2=L2[loss])
    pl = plan(("caps", loss, ic), narrow_shapes(0, 5, full=True), SEED_CAPS + 10 * ch.LOSSES.index(loss) + ic, loss, kw)
    res, cls, nnarrow = _solve(solver, pl["b"], kw, loss)
    assert np.all(cls == NARROW_CLASS) and nnarrow == pl["b"].E
    compare(pl, loss, kw, res)


@pytest.mark.gpu
@pytest.mark.parametrize("max_iter", [KR, KR + 1, KR + 2, 100])
@pytest.mark.parametrize("ic", [1, 0], ids=["intercept", "no_intercept"])
@pytest.mark.parametrize("loss", list(ch.LOSSES))
def test_narrow_ring_by_iterations(solver, loss, ic, max_iter):
    """A pair is pushed at the end of iterations 1 .. nit - 1 and stored only by a push that finds KR pairs, so nit = KR and KR + 1 leave the
    ring empty (the last direction of nit = KR + 1 uses exactly the KR register pairs), nit = KR + 2 stores one pair and reads it once, and
    a run of 2 KR + 2 iterations and more has filled the five slots and written over the first."""
    kw, pl = ring_plan(loss, ic, max_iter)
    if max_iter < 100:
        assert np.all(pl["nit"] == max_iter) and np.all(pl["ref"]["status"] == 2), (pl["nit"], pl["ref"]["status"])
    else:
        assert pl["nit"].min() >= KR + 2 and pl["nit"].max() >= 2 * KR + 2, pl["nit"]      # every row reads the ring; one wraps it
    res, cls, nnarrow = _solve(solver, pl["b"], kw, loss)
    assert np.all(cls == NARROW_CLASS) and nnarrow == pl["b"].E
    compare(pl, loss, kw, res)


@pytest.mark.gpu
@pytest.mark.parametrize("ic", [1, 0], ids=["intercept", "no_intercept"])
@pytest.mark.parametrize("loss", list(ch.LOSSES))
def test_narrow_one_row_reads_the_ring(solver, loss, ic):
    kw, pl = mixed_plan(loss, ic)
    assert np.all(pl["nit"][:3] <= KR) and pl["nit"][3] >= KR + 2, pl["nit"]
    res, cls, nnarrow = _solve(solver, pl["b"], kw, loss)
    assert np.all(cls == NARROW_CLASS) and nnarrow == 4
    compare(pl, loss, kw, res)


@pytest.mark.gpu
@pytest.mark.parametrize("ic", [1, 0], ids=["intercept", "no_intercept"])
@pytest.mark.parametrize("loss", list(ch.LOSSES))
def test_narrow_short_memory(solver, loss, ic):
    kw, pl = short_memory_plan(loss, ic)
    assert pl["nit"].max() >= 2 * KR + 2, pl["nit"]
    res, cls, nnarrow = _solve(solver, pl["b"], kw, loss)
    assert np.all(cls == NARROW_CLASS) and nnarrow == pl["b"].E
    compare(pl, loss, kw, res)
