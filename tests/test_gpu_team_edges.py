"""The five classes of re_solve_team_kernel<NW, GRID> ("workgroup", "128 teams", "32 teams", "8 teams", "device-wide";
csrc/re_solve_team.hpp) with entities ON the constants team_fg's column pass branches on (TEAM_SHORT_COL, TEAM_CHUNK, TEAM_LONGC,
TEAM_LONG_CAP), at every team count GDMIX_RE_TEAMS can pin, and with entities on the tier thresholds of re_classify_kernel: the class
every entity ran in is read back and held to team_edges_helpers.route_large, and the solution to the CPU reference by the rule each
loss's own tests use (narrow_helpers.compare_with_oracle, re_linear_helpers.judge, re_poisson_helpers.compare). What the reference and
the shapes must meet for this to mean something is checked on the CPU by tests/test_team_edges.py.

A CHANGED CONSTANT of csrc/re_solve_team.hpp is changed in team_edges_helpers too: test_the_constants_are_the_librarys fails until it
is, and tests/test_team_edges.py then names the situations the shapes of edge_entities() no longer show.

Every solve asserts that no entity reports GDMIX_RE_ST_ABORTED (a team's barrier gives up after 4 s): that is a failure, never a
reason to run again."""
import os
import re

import numpy as np
import pytest

import class_caps_helpers as ch
import narrow_helpers as nh
import re_linear_helpers as lh
import re_poisson_helpers as ph
import team_edges_helpers as th
from gdmix_amd import solver as solver_module
from gdmix_amd.solver import NUM_CLASSES, SolverOptions

pytestmark = pytest.mark.gpu

BITWISE = ("theta", "theta_thr", "fval", "gnorm", "nit", "nfev", "status")
LOSS_OPTIONS = {"logistic": {}, "squared": dict(linear=True), "poisson": dict(loss="poisson")}
ST_ABORTED = 9      # GDMIX_RE_ST_ABORTED (include/gdmix_re.h)
PAIRS = [(loss, ic) for loss in th.LOSSES for ic in (1, 0)]


def _solve(solver, c, routing, variance=False, twice=False):
    """Pack and solve the case's batch under the routing knobs of `routing` (re_linear_helpers.set_routing; the others at their defaults)
    -> (packed, host result, per-entity class, {class name: count}[, the second solve's host result])."""
    packed = solver.pack(c["b"], has_intercept=c["kw"]["has_intercept"])
    opts = SolverOptions(**dict(c["kw"], variance_mode=1 if variance else 0), **LOSS_OPTIONS[c["loss"]])
    lh.set_routing(solver, **routing)
    try:
        res = solver.solve(packed, opts).to_host()
        counts = dict(solver.class_counts(packed))
        cls = packed._view(packed.c.cls_tmp, packed.E, solver.torch.int32).cpu().numpy().copy()
        again = solver.solve(packed, opts).to_host() if twice else None
    finally:
        lh.reset_routing(solver)
    assert sum(counts.values()) == packed.E == c["b"].E
    for r in (res, again):
        if r is not None:
            assert np.all(r["status"] >= 0) and not np.any(r["status"] == ST_ABORTED), np.unique(r["status"])
    return (packed, res, cls, counts) + ((again,) if twice else ())


def _compare(c, packed, res, variance):
    """One solve of case c against its reference, by the loss's own rule (tests/test_gpu_class_caps.py, _compare: the same counts, the
    same tolerances) on the entities the reference reproduces; every edge entity is one (tests/test_team_edges.py)."""
    r = th.reference(c)
    b, kw, cp, strict = c["b"], dict(c["kw"], variance_mode=1 if variance else 0), packed.coef_ptr_host(), r["strict"]
    assert np.array_equal(cp, r["coef_ptr"])
    assert strict[c["edge"]].all() and strict.mean() >= 0.5
    if c["loss"] == "logistic":
        nh.compare_with_oracle(res, r["ref"], cp, wp=strict)
        if variance:      # (the oracle's variance is taken at the oracle's theta: on the entities compared above)
            coefs = np.repeat(strict, np.diff(cp))
            np.testing.assert_allclose(res["variance"][coefs], r["ref"]["variance"][coefs], rtol=1e-7)
    elif c["loss"] == "squared":
        j = lh.judge(b, r["pk"], kw, None, res, cp, theta_tol=nh.REL_TOL_DEVICE)      # (SIMPLE variance at rtol 1e-7 is one of its problems)
        assert not j["problems"], j["problems"][:3]
        ok, ref = j["strict_ok"], j["ref"]
        print(f"{c['name']}: {int(ok.sum())} of {b.E} strict and not flagged, worst theta error {float(j['err'][ok].max()):.3e}")
        assert np.array_equal(ok, strict), (np.flatnonzero(ok != strict), j["adjudicated"][:3])
        for k in ("status", "nit", "nfev"):
            assert np.array_equal(res[k][ok], ref[k][ok]), k
        assert j["err"][ok].max() <= nh.REL_TOL_DEVICE
        np.testing.assert_allclose(res["fval"][ok], ref["fval"][ok], rtol=1e-9, atol=1e-13)
    else:
        ph.compare(res, r["ref"], cp)
        if variance:
            np.testing.assert_allclose(res["variance"], ph.variance_numpy(b, r["pk"], kw, 1, res["theta"], cp), rtol=1e-7)


def _solve_and_compare(solver, c, routing, check_classes):
    """Two solves without variance, bit for bit the same; one with SIMPLE variance, whose solution is the same bits again and is held
    to the reference together with the variances. check_classes(cls, counts) states where the entities must have run."""
    packed, res, cls, counts, again = _solve(solver, c, routing, twice=True)
    check_classes(cls, counts)
    for k in BITWISE:
        assert np.array_equal(res[k], again[k]), k
    _compare(c, packed, res, variance=False)
    packed_v, res_v, cls_v, _ = _solve(solver, c, routing, variance=True)
    assert np.array_equal(cls_v, cls)
    _compare(c, packed_v, res_v, variance=True)


def _names(solver):
    return [solver.lib.gdmix_re_class_kernel_name(k).decode() for k in range(NUM_CLASSES)]


def test_the_constants_are_the_librarys(device_solver):
    names = _names(device_solver)
    assert NUM_CLASSES == 40 == len(names) and names[-5:] == th.TEAM_NAMES
    assert [names[k] for k in (th.BLOCK_CLASS, th.TEAM128_CLASS, th.TEAM32_CLASS, th.TEAM8_CLASS, th.GIANT_CLASS)] == th.TEAM_NAMES
    header = os.path.join(os.path.dirname(solver_module.LIB_PATH), "csrc", "re_solve_team.hpp")
    if not os.path.exists(header):
        pytest.skip("the sources are not shipped next to the library: the constants cannot be read (the class names were compared)")
    with open(header) as fh:
        text = fh.read()
    for name, value in th.CONSTANTS.items():
        found = re.findall(rf"constexpr\s+int\s+{name}\s*=\s*(\d+)\s*;", text)
        assert found == [str(value)], (name, found, value)
    assert th.WAVE == 64 and "item >> 6" in text      # 64 slices per split column


@pytest.mark.parametrize("loss,ic", PAIRS)
def test_one_workgroup_class(device_solver, loss, ic):
    """lds_limit = 0 and no team tier: every entity of the edge batch on one workgroup (eight wavefronts, p-vectors in LDS where they fit)."""
    c = th.case(loss, ic)

    def classes(cls, counts):
        assert np.all(cls == th.BLOCK_CLASS) and counts[th.TEAM_NAMES[0]] == c["b"].E, np.unique(cls)
    _solve_and_compare(device_solver, c, dict(lds_limit=0, team_nnz=0, tall_min_n=0), classes)


TEAM_COUNTS = [("logistic", 1, t) for t in (128, 64, 32, 16, 8, 4, 2, 1)] + [(loss, ic, t) for loss, ic in PAIRS[1:] for t in (128, 8, 1)]


@pytest.mark.parametrize("loss,ic,t", TEAM_COUNTS)
def test_every_team_size(device_solver, monkeypatch, loss, ic, t):
    """team_nnz = 2: every edge entity in a team tier, GDMIX_RE_TEAMS = t teams of (CUs / t) workgroups each. The library does not report
    the team count it used: team_count() keeps the knob's value when it divides the CUs and the batch has at least that many scratch
    slots, i.e. entities (slots_for), and both are asserted here. Results for different t differ to rounding and are not compared.
    (At team_nnz = 2 every edge entity has 128 x team_nnz non-zeros and more, so they all read back in "8 teams": the knob replaces the
    tier's own choice, its maximum included, and the kernel is the same for the three tiers.)"""
    c = th.case(loss, ic)
    cus = device_solver.torch.cuda.get_device_properties(0).multi_processor_count
    assert cus % t == 0 and c["b"].E >= t and t <= 256, (cus, t, c["b"].E)
    monkeypatch.setenv("GDMIX_RE_TEAMS", str(t))

    def classes(cls, counts):
        assert np.all(np.isin(cls[c["edge"]], th.TEAM_TIERS)), cls[c["edge"]]
        assert np.all(cls[th.N_EDGE:] < len(ch.GROUP_CLASSES)), np.unique(cls[th.N_EDGE:])
        assert sum(counts[n] for n in th.TEAM_NAMES[1:4]) == th.N_EDGE
    _solve_and_compare(device_solver, c, dict(team_nnz=2, tall_min_n=0), classes)


@pytest.mark.parametrize("loss", th.LOSSES)
def test_device_wide_class(device_solver, loss):
    c = th.case(loss, 1)

    def classes(cls, counts):
        assert np.all(cls[c["edge"]] == th.GIANT_CLASS) and counts[th.TEAM_NAMES[4]] == th.N_EDGE, cls[c["edge"]]
        assert np.all(cls[th.N_EDGE:] < len(ch.GROUP_CLASSES))
    _solve_and_compare(device_solver, c, dict(giant_nnz=2, tall_min_n=0), classes)


def _routed(c, has_w, tall_min_n, team_nnz, giant_nnz):
    b = c["b"]
    p = np.diff(th.reference(c)["coef_ptr"])
    return np.array([th.route_large(int(p[e]), int(n), int(z), c["kw"]["m"], has_w, tall_min_n, team_nnz, giant_nnz, ic=c["ic"])
                     for e, (n, z) in enumerate(zip(b.ent_n(), b.ent_nnz()))])


def _classes_as_routed(want, names):
    def classes(cls, counts):
        fixed = want != th.TALL_ANY
        assert np.array_equal(cls[fixed], want[fixed]), (np.flatnonzero(fixed & (cls != want)), cls[fixed & (cls != want)])
        assert np.all(np.isin(cls[~fixed], list(ch.TALL_CLASSES)))
        for k in np.unique(want[fixed]):
            if k not in ch.TALL_CLASSES:      # (a lean tall class may be launched with the class behind it; its count stays its own)
                assert counts[names[k]] == int((want == k).sum()), (names[k], counts[names[k]])
    return classes


def test_tier_thresholds(device_solver):
    """z >= team_nnz, 8 x, 128 x, giant_nnz and the tall rule's precedence, with entities one below and on each threshold: at team_nnz = 64
    and giant_nnz = 20 000 with the tall rule off, the same again with the tall rule at 32 samples (every entity here has p <= 64: all
    become tall but the two of 20 000 non-zeros, which stay device-wide), then at the library's defaults (16 384 and 131 072; the 128 x
    boundary is checked at the scaled knob only)."""
    names = _names(device_solver)
    c = th.tier_case("scaled")
    T128, T32, T8, G = th.TEAM128_CLASS, th.TEAM32_CLASS, th.TEAM8_CLASS, th.GIANT_CLASS
    want = _routed(c, True, 0, th.TIER_TEAM_NNZ, th.TIER_GIANT_NNZ)
    assert want[0] < len(ch.GROUP_CLASSES) and want[1:].tolist() == [T128, T128, T32, T32, T8, T8, G, T128, G]
    _solve_and_compare(device_solver, c, dict(team_nnz=th.TIER_TEAM_NNZ, giant_nnz=th.TIER_GIANT_NNZ, tall_min_n=0), _classes_as_routed(want, names))
    want = _routed(c, True, th.TIER_TALL_MIN_N, th.TIER_TEAM_NNZ, th.TIER_GIANT_NNZ)
    assert np.all(np.isin(want[[0, 1, 2, 3, 4, 5, 6, 8]], list(ch.TALL_CLASSES))) and want[7] == want[9] == G
    _solve_and_compare(device_solver, c, dict(team_nnz=th.TIER_TEAM_NNZ, giant_nnz=th.TIER_GIANT_NNZ, tall_min_n=th.TIER_TALL_MIN_N),
                       _classes_as_routed(want, names))
    c = th.tier_case("defaults")
    want = _routed(c, True, device_solver.TALL_MIN_N_DEFAULT, th.TEAM_NNZ_DEFAULT, th.GIANT_NNZ_DEFAULT)
    assert want.tolist() == [th.BLOCK_CLASS, T128, T128, T32]
    _solve_and_compare(device_solver, c, dict(), _classes_as_routed(want, names))


@pytest.mark.parametrize("loss", th.LOSSES)
def test_default_routing(device_solver, monkeypatch, loss):
    """The edge batch as a caller gets it: no knob, no environment variable."""
    monkeypatch.delenv("GDMIX_RE_TEAMS", raising=False)
    c = th.case(loss, 1)
    assert device_solver.TALL_MIN_N_DEFAULT == 32 and (lh.ROUTING_DEFAULTS["team_nnz"], lh.ROUTING_DEFAULTS["giant_nnz"]) == (th.TEAM_NNZ_DEFAULT, th.GIANT_NNZ_DEFAULT)
    want = _routed(c, True, 32, th.TEAM_NNZ_DEFAULT, th.GIANT_NNZ_DEFAULT)
    by_name = dict(zip(th.EDGE_NAMES, want[:th.N_EDGE].tolist()))
    assert by_name["mixed"] == th.TEAM128_CLASS and by_name["cap256"] == by_name["cap257"] == th.TEAM32_CLASS
    assert by_name["wide1101"] == by_name["wide1025"] == by_name["wide513"] == th.BLOCK_CLASS
    assert by_name["one_col"] == by_name["four_col"] == th.TALL_ANY and by_name["rows"] < len(ch.GROUP_CLASSES) and np.all(want[th.N_EDGE:] == 0)
    _solve_and_compare(device_solver, c, dict(), _classes_as_routed(want, _names(device_solver)))
