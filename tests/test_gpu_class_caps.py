"""Every group class (re_solve_grp_kernel<G, EPL, NCAP, ZCAP>, 28 rows of kClasses in csrc/re_internal.hpp) and both LDS buckets of
re_solve_wave_kernel, each with entities ON its caps and one past them: the class every entity ran in is read back and held to
class_caps_helpers.route (the tests' own statement of re_classify_kernel's first-fit rule), and the solution to the CPU reference by the
rule each loss's own tests use (narrow_helpers.compare_with_oracle, re_linear_helpers.judge, re_poisson_helpers.compare). What the
reference itself must meet for this to mean something is checked on the CPU by tests/test_class_caps.py.

A NEW OR CHANGED ROW of kClasses is added to class_caps_helpers.GROUP_CLASSES (or WAVE_BUCKETS): test_the_table_is_the_librarys fails
until it is, and the shape lists then put entities on the row's caps."""
import numpy as np
import pytest

import class_caps_helpers as ch
import narrow_helpers as nh
import re_linear_helpers as lh
import re_poisson_helpers as ph
from gdmix_amd.solver import NUM_CLASSES, SolverOptions

pytestmark = pytest.mark.gpu

BITWISE = ("theta", "theta_thr", "fval", "gnorm", "nit", "nfev", "status")
LOSS_OPTIONS = {"logistic": {}, "squared": dict(linear=True), "poisson": dict(loss="poisson")}


def _solve(solver, c, tall_min_n=0, variance=False, twice=False):
    """Pack and solve the case's batch with the tall rule at tall_min_n (None: the library's default), every other routing knob at its
    default -> (packed, host result, per-entity class, {class name: count}[, the second solve's host result])."""
    packed = solver.pack(c["b"], has_intercept=c["kw"]["has_intercept"])
    opts = SolverOptions(**dict(c["kw"], variance_mode=1 if variance else 0), **LOSS_OPTIONS[c["loss"]])
    lh.set_routing(solver, tall_min_n=tall_min_n)
    try:
        res = solver.solve(packed, opts).to_host()
        counts = dict(solver.class_counts(packed))
        cls = packed._view(packed.c.cls_tmp, packed.E, solver.torch.int32).cpu().numpy().copy()
        again = solver.solve(packed, opts).to_host() if twice else None
    finally:
        lh.reset_routing(solver)
    assert sum(counts.values()) == packed.E == len(c["shapes"])
    return (packed, res, cls, counts) + ((again,) if twice else ())


def _compare(name, packed, res, variance):
    """The result of one solve of case `name` against its reference, by the loss's own rule, on the entities the reference reproduces
    (tests/test_class_caps.py: every class has one, and they are at least 90 % — all of them at the committed seed)."""
    c, r = ch.case(name), ch.reference(name)
    b, kw, cp, strict = c["b"], dict(c["kw"], variance_mode=1 if variance else 0), packed.coef_ptr_host(), r["strict"]
    assert np.array_equal(cp, r["coef_ptr"])
    cls = np.array([s[3] for s in c["shapes"]])
    assert strict.mean() >= 0.9 and all(strict[cls == k].any() for k in np.unique(cls))
    if c["loss"] == "logistic":
        nh.compare_with_oracle(res, r["ref"], cp, wp=strict)
        if variance:      # (the oracle's variance is taken at the oracle's theta: on the entities compared above)
            coefs = np.repeat(strict, np.diff(cp))
            np.testing.assert_allclose(res["variance"][coefs], r["ref"]["variance"][coefs], rtol=1e-7)
    elif c["loss"] == "squared":
        j = lh.judge(b, r["pk"], kw, None, res, cp, theta_tol=nh.REL_TOL_DEVICE)      # (SIMPLE variance at rtol 1e-7 is one of its problems)
        assert not j["problems"], j["problems"][:3]
        ok, ref = j["strict_ok"], j["ref"]
        print(f"{name}: {int(ok.sum())} of {b.E} strict and not flagged, worst theta error {float(j['err'][ok].max()):.3e}")
        assert np.array_equal(ok, strict), (np.flatnonzero(ok != strict), j["adjudicated"][:3])
        for k in ("status", "nit", "nfev"):
            assert np.array_equal(res[k][ok], ref[k][ok]), k
        assert j["err"][ok].max() <= nh.REL_TOL_DEVICE
        np.testing.assert_allclose(res["fval"][ok], ref["fval"][ok], rtol=1e-9, atol=1e-13)
    else:
        ph.compare(res, r["ref"], cp)
        if variance:
            np.testing.assert_allclose(res["variance"], ph.variance_numpy(b, r["pk"], kw, 1, res["theta"], cp), rtol=1e-7)


def _routed(name, tall_min_n, has_w=False):
    c = ch.case(name)
    return np.array([ch.route(s[0], s[1], s[2], c["kw"]["m"], has_w, tall_min_n, ic=c["ic"]) for s in c["shapes"]])


def test_the_table_is_the_librarys(device_solver):
    c = ch.case("ragged-7-1")
    packed = device_solver.pack(c["b"], has_intercept=True)
    device_solver.solve(packed, SolverOptions(**c["kw"]))
    names = [name for name, _ in device_solver.class_counts(packed)]
    assert NUM_CLASSES == ch.NUM_CLASSES == 40 == len(names)
    assert names[:30] == ch.class_names()
    assert names[ch.BLOCK_CLASS] == ch.BLOCK_NAME
    assert names[ch.TALL_LEAN_CLASS] == "re_solve_tall_kernel<1> lean p<=64" and names[ch.TALL_ONE_CLASS] == "re_solve_tall_kernel<1> p<=64"
    assert all("tall" in names[k] for k in ch.TALL_CLASSES) and not any("tall" in n for k, n in enumerate(names) if k not in ch.TALL_CLASSES)


def test_group_classes_at_their_caps(device_solver):
    """edges(): 121 entities, every group class at its corner and along its edges, the tall rule off. Class by class as route() says,
    every entity against the oracle; SIMPLE variance; a second solve bit for bit the first."""
    c = ch.case("edges")
    packed, res, cls, counts, again = _solve(device_solver, c, twice=True)
    want = _routed("edges", 0)
    assert np.array_equal(want, [s[3] for s in c["shapes"]])
    assert np.array_equal(cls, want), np.flatnonzero(cls != want)
    names = ch.class_names()
    assert all(counts[names[k]] == int((want == k).sum()) > 0 for k in range(28)), counts
    assert ch.reference("edges")["strict"].all()
    _compare("edges", packed, res, variance=False)
    for k in BITWISE:
        assert np.array_equal(res[k], again[k]), k
    packed_v, res_v, cls_v, _ = _solve(device_solver, c, variance=True)
    assert np.array_equal(cls_v, want)
    _compare("edges", packed_v, res_v, variance=True)


@pytest.mark.parametrize("loss", ch.LOSSES)
def test_corners_with_weights_and_an_unregularised_intercept(device_solver, loss):
    name = f"corners-{loss}"
    packed, res, cls, counts = _solve(device_solver, ch.case(name), variance=True)
    assert np.array_equal(cls, np.arange(28)), cls
    _compare(name, packed, res, variance=True)


@pytest.mark.parametrize("loss", ch.LOSSES)
def test_corners_without_intercept(device_solver, loss):
    """d = G * EPL: the last coefficient slot of the last lane holds a feature."""
    name = f"corners_no_intercept-{loss}"
    packed, res, cls, counts = _solve(device_solver, ch.case(name), variance=True)
    assert np.array_equal(np.diff(packed.coef_ptr_host()), [g * epl for g, epl, _, _ in ch.GROUP_CLASSES])
    assert np.array_equal(cls, np.arange(28)), cls
    _compare(name, packed, res, variance=True)


def test_one_past_each_cap(device_solver):
    """neighbours(): p + 1, n + 1 and nnz + 1 of every corner. None stays in the class whose cap it exceeds; each is where route() says
    (a later group class, or the workgroup class) and agrees with the oracle there."""
    c = ch.case("neighbours")
    packed, res, cls, counts, again = _solve(device_solver, c, twice=True)
    want = _routed("neighbours", 0)
    assert np.array_equal(want, [s[3] for s in c["shapes"]])
    assert np.array_equal(cls, want), np.flatnonzero(cls != want)
    assert not np.any(cls == np.array([s[4] for s in c["shapes"]]))
    assert counts[ch.BLOCK_NAME] == int((want == ch.BLOCK_CLASS).sum()) > 0
    _compare("neighbours", packed, res, variance=False)
    for k in BITWISE:
        assert np.array_equal(res[k], again[k]), k
    packed_v, res_v, _, _ = _solve(device_solver, c, variance=True)
    _compare("neighbours", packed_v, res_v, variance=True)


def test_default_routing(device_solver):
    """edges() as a caller gets it: entities of p <= 64 and n >= 32 go to the tall kernels, every other one to the same class as before."""
    c = ch.case("edges")
    packed, res, cls, counts, again = _solve(device_solver, c, tall_min_n=None, twice=True)
    assert device_solver.TALL_MIN_N_DEFAULT == 32
    want, group = _routed("edges", 32), _routed("edges", 0)
    tall = np.array([s[0] <= 64 and s[1] >= 32 for s in c["shapes"]])
    assert tall.sum() >= 9 and np.all(np.isin(want[tall], list(ch.TALL_CLASSES))) and np.array_equal(want[~tall], group[~tall])
    assert np.array_equal(cls, want), (np.flatnonzero(cls != want), cls[cls != want])
    _compare("edges", packed, res, variance=False)
    for k in BITWISE:
        assert np.array_equal(res[k], again[k]), k
    packed_v, res_v, _, _ = _solve(device_solver, c, tall_min_n=None, variance=True)
    _compare("edges", packed_v, res_v, variance=True)


@pytest.mark.parametrize("size", ch.RAGGED_SIZES)
@pytest.mark.parametrize("k", ch.RAGGED_CLASSES)
def test_ragged_last_workgroup(device_solver, k, size):
    """1, 2, 3 and 5 corner entities of a four-per-wavefront and of a two-per-wavefront class: rows of the last wavefront have no entity."""
    name = f"ragged-{k}-{size}"
    c = ch.case(name)
    packed, res, cls, counts, again = _solve(device_solver, c, twice=True)
    assert np.all(cls == k) and counts[ch.class_names()[k]] == size
    _compare(name, packed, res, variance=False)
    for key in BITWISE:
        assert np.array_equal(res[key], again[key]), key
    packed_v, res_v, _, _ = _solve(device_solver, c, variance=True)
    _compare(name, packed_v, res_v, variance=True)


@pytest.mark.parametrize("weights", [False, True])
def test_wavefront_buckets(device_solver, weights):
    """m = 12 (no group class): entities of exactly 24 576 B run in the 24 KiB bucket, of 24 592 B and of 65 536 B in the 64 KiB bucket,
    of 65 552 B on a workgroup — the kernel's carve-up holds what wave_lds_bytes promises, to the last non-zero."""
    name = "wave_weights" if weights else "wave"
    c = ch.case(name)
    packed, res, cls, counts, again = _solve(device_solver, c, twice=True)
    size = np.array([s[4] for s in c["shapes"]])
    assert np.array_equal(_routed(name, 0, has_w=weights), [s[3] for s in c["shapes"]])
    assert np.all(cls[size == 24576] == ch.WAVE_24K) and np.all(cls[(size == 24592) | (size == 65536)] == ch.WAVE_64K)
    assert np.all(cls[size == 65552] == ch.BLOCK_CLASS)
    names = ch.class_names()
    assert counts[names[ch.WAVE_24K]] == 3 and counts[names[ch.WAVE_64K]] == 6 and counts[ch.BLOCK_NAME] == 3
    _compare(name, packed, res, variance=False)
    for k in BITWISE:
        assert np.array_equal(res[k], again[k]), k
    packed_v, res_v, _, _ = _solve(device_solver, c, variance=True)
    _compare(name, packed_v, res_v, variance=True)
