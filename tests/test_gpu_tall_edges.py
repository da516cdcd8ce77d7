"""The five tall classes (re_solve_tall_kernel<1>, <1> lean, <4>, <8> and re_solve_tall_team_kernel<8> x4; csrc/re_solve_tall.hip) with
entities ON what their code branches on: the trip of a pass (R x NT samples, every width class), the LDS arena (an entity of exactly
its bytes and the next one up, with and without weights, at both counts of accumulator sets), p = 32 / 33 / 64 and d = 0, the padded
tail of the batch, samples without entries and repeated columns, and teams whose members live in different homes. Under pinned
routing knobs the class every entity ran in is read back and held to tall_edges_helpers.route_tall; every entity is held to the CPU
reference by the rule its loss's own tests use (narrow_helpers.compare_with_oracle, re_poisson_helpers.compare: equal status, nit and
nfev, theta to REL_TOL_DEVICE, fval to rtol 1e-9) and its SIMPLE variance to the dense statement at rtol 1e-7; a second solve gives the
same bits. What the shapes and the reference must meet for this to mean something is checked on the CPU by tests/test_tall_edges.py:
every named entity is strict there, so nothing is filtered here.

WHICH HOME AN ENTITY TOOK CANNOT BE READ BACK: tall_setup decides resident or streamed inside the kernel and reports nothing. The
tests hold both sides of every arena to the reference — a carve-up that disagreed with tall_resident_bytes would overwrite the last
array of the entity ON the arena, a wrong residency test would stage the one above it past the arena — and to each other's bits where
the code promises that. The lean routing threshold is the one arena whose side is visible, through cls_tmp.

A CHANGED CONSTANT of the tall kernels is changed in tall_edges_helpers too: test_the_constants_are_the_librarys fails until it is, and
tests/test_tall_edges.py then names the situations the batches no longer show.

Every solve asserts that no entity reports GDMIX_RE_ST_ABORTED (a team member gives up after 4 s): that is a failure, never a reason
to run again."""
import os
import re

import numpy as np
import pytest

import narrow_helpers as nh
import re_linear_helpers as lh
import re_poisson_helpers as ph
import tall_edges_helpers as th
from gdmix_amd import solver as solver_module
from gdmix_amd.solver import NUM_CLASSES, SolverOptions

pytestmark = pytest.mark.gpu

BITWISE = ("theta", "theta_thr", "variance", "fval", "gnorm", "nit", "nfev", "status")
LOSS_OPTIONS = {"logistic": {}, "squared": dict(linear=True), "poisson": dict(loss="poisson")}
ST_ABORTED = 9      # GDMIX_RE_ST_ABORTED (include/gdmix_re.h)
TALL_RANGE = list(range(th.TALL_TEAM_CLASS, th.TALL_LARGE_CLASS + 1))


def _solve(solver, c, twice=True):
    """Pack and solve the case's batch with SIMPLE variance under its pinned routing -> (packed, host result, per-entity class, the second
    solve's host result or None)."""
    packed = solver.pack(c["b"], has_intercept=c["kw"]["has_intercept"])
    opts = SolverOptions(**dict(c["kw"], variance_mode=1), **LOSS_OPTIONS[c["loss"]])
    lh.set_routing(solver, **c["routing"])
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
    if again is not None:
        for k in BITWISE:
            assert np.array_equal(res[k], again[k]), (c["name"], k)
    return packed, res, cls, again


def _check_classes(c, cls):
    want = th.routed(c)
    tall = want != th.NOT_TALL
    wrong = np.flatnonzero(tall & (cls != want))
    assert wrong.size == 0, [(c["names"][e], int(cls[e]), int(want[e])) for e in wrong]
    assert not np.isin(cls[~tall], TALL_RANGE).any(), [c["names"][e] for e in np.flatnonzero(~tall)]


def _compare(c, packed, res):
    """One solve against the case's reference on EVERY entity, and the variances against the dense statement at the device's theta."""
    r = th.reference(c)
    cp = packed.coef_ptr_host()
    assert np.array_equal(cp, r["coef_ptr"])
    assert r["strict"].all(), [n for n, s in zip(c["names"], r["strict"]) if not s]
    if c["loss"] == "poisson":
        ph.compare(res, r["ref"], cp, min_strict_share=1.0)
    else:
        assert nh.REL_TOL_DEVICE == 1e-7
        nh.compare_with_oracle(res, r["ref"], cp, wp=r["strict"])      # (fval: rtol 1e-9, the figure of test_gpu_parity's _slice_edge_compare)
    np.testing.assert_allclose(res["variance"], th.variance_dense(c["b"], r["pk"], c["kw"], c["loss"], res["theta"], cp), rtol=1e-7)


def _run(solver, c):
    packed, res, cls, _ = _solve(solver, c)
    _check_classes(c, cls)
    _compare(c, packed, res)
    return packed, res


def _per_entity(c, packed, res):
    """{name: the entity's outputs as a tuple of arrays}"""
    cp = packed.coef_ptr_host()
    return {n: tuple(res[k][cp[e]:cp[e + 1]] if k in ("theta", "theta_thr", "variance") else res[k][e:e + 1] for k in BITWISE) for e, n in enumerate(c["names"])}


def _same_bits(a, b, names):
    for n in names:
        for k, x, y in zip(BITWISE, a[n], b[n]):
            assert np.array_equal(x, y), (n, k)


def test_the_constants_are_the_librarys(device_solver):
    names = [device_solver.lib.gdmix_re_class_kernel_name(k).decode() for k in range(NUM_CLASSES)]
    assert NUM_CLASSES == 40 and names[th.TALL_TEAM_CLASS:th.TALL_LARGE_CLASS + 1] == th.TALL_NAMES
    assert (device_solver.TALL_SPLIT_N_DEFAULT, device_solver.TALL_TEAM_N_DEFAULT) == (th.TALL_SPLIT_N_DEFAULT, th.TALL_TEAM_N_DEFAULT) == (4096, 8192)
    src = os.path.join(os.path.dirname(solver_module.LIB_PATH), "csrc")
    if not os.path.exists(os.path.join(src, "re_solve_tall.hip")):
        pytest.skip("the sources are not shipped next to the library: the constants cannot be read (the class names were compared)")
    text = {}
    for f in ("re_internal.hpp", "re_solve_tall.hip", "re_solve_wreg.hpp", "re_device.hpp", "re_route.hip"):
        with open(os.path.join(src, f)) as fh:
            text[f] = fh.read()

    def const(f, name):
        found = re.findall(rf"constexpr\s+int\s+{name}\s*=\s*([^;]+);", text[f])
        assert len(found) == 1, (name, found)
        return found[0].strip()

    def define(f, name):
        found = re.findall(rf"#define\s+{name}\s+(\d+)", text[f])
        assert len(found) == 1, (name, found)
        return int(found[0])
    hpp, hip = "re_internal.hpp", "re_solve_tall.hip"
    for name in ("TALL_MAX_P", "TALL_TEAM_C", "TALL_TEAM_MIN_N", "TALL_NW", "TALL_NW_MID", "TALL_MID_WGS"):
        assert int(const(hpp, name)) == getattr(th, name), name
    assert int(const(hip, "TALL_TAIL")) == th.TALL_TAIL
    assert const(hpp, "TALL_LEAN_WGS") == "4 * TALL_LEAN_WAVES" and 4 * int(const(hpp, "TALL_LEAN_WAVES")) == th.TALL_LEAN_WGS
    assert const(hpp, "TALL_NW_SMALL") == "GDMIX_TALL_NW_SMALL" and define(hpp, "GDMIX_TALL_NW_SMALL") == th.TALL_NW_SMALL
    assert define(hip, "GDMIX_TALL_R8") == th.GDMIX_TALL_R8 and define(hip, "GDMIX_TALL_WAVES_SMALL") == th.GDMIX_TALL_WAVES_SMALL
    assert int(const("re_solve_wreg.hpp", "M_REG")) == th.M_REG and int(const("re_device.hpp", "WAVE")) == th.WAVE
    # tall_sets, tall_lds_bytes, TALL_LEAN_ARENA, tall_resident_bytes
    (a, b, c, d), = re.findall(r"tall_sets\(int nw, int p\) \{ return \(nw > (\d+) && p <= (\d+)\) \? (\d+) : (\d+); \}", text[hpp])
    for nw in (1, 2, 4, 8):
        for p in (1, 31, 32, 33, 64):
            assert th.tall_sets(nw, p) == (int(c) if (nw > int(a) and p <= int(b)) else int(d)), (nw, p)
    (k, wb, minus), = re.findall(r"tall_lds_bytes\(int wg_per_cu\) \{ return (\d+) \* (\d+) / wg_per_cu - (\d+); \}", text[hpp])
    for w in (1, 2, 8, 12):
        assert th.tall_lds_bytes(w) == int(k) * int(wb) // w - int(minus)
    (lean_minus, lean_mask), = re.findall(r"TALL_LEAN_ARENA = \(tall_lds_bytes\(TALL_LEAN_WGS\) - (\d+)\) & ~(\d+);", text[hpp])
    assert th.TALL_LEAN_ARENA == (th.tall_lds_bytes(th.TALL_LEAN_WGS) - int(lean_minus)) & ~int(lean_mask) == 11728
    assert ("return (size_t)nw * (d + 1) * (S + 1) * 8 + (size_t)8 * (nnz + 8) + (size_t)4 * (n + 2) + (size_t)(has_w ? 12 : 8) * n + 16;" in text[hpp])
    assert th.tall_resident_bytes(3, 5, 7, 11, 13, True) == 3 * 8 * 6 * 8 + 8 * 21 + 4 * 13 + 12 * 11 + 16
    assert th.tall_resident_bytes(3, 5, 7, 11, 13, False) == 3 * 8 * 6 * 8 + 8 * 21 + 4 * 13 + 8 * 11 + 16
    assert "tall_resident_bytes(1, tall_sets(1, p), d, n, z, has_w) <= (size_t)TALL_LEAN_ARENA ? TALL_L_CLASS : TALL_S_CLASS" in text["re_route.hip"]
    assert "if (tab.tall_team_n > 0 && tab.tall_team_n < TALL_TEAM_MIN_N) tab.tall_team_n = TALL_TEAM_MIN_N;" in text["re_route.hip"]
    # TallLds: its fields, hence its size
    body, = re.findall(r"struct TallLds \{(.*?)\n\};", text[hip], re.S)
    fields, size = [], 0
    for line in body.split("\n"):
        line = line.split("//")[0].strip()
        if not line:
            continue
        typ, rest = line.rstrip(";").split(" ", 1)
        for decl in rest.split(","):
            fields.append(decl.strip())
            count = 1
            for dim in re.findall(r"\[(\w+)\]", decl):
                count *= {"WAVE": th.WAVE, "M_REG": th.M_REG}.get(dim, None) or (8 if dim == "NW" else int(dim))
            size += count * {"double": 8, "int": 4}[typ]
    assert fields == th.TALL_LDS_FIELDS, fields
    assert size == th.tall_lds_sizeof(8) and th.tall_lds_sizeof(1) == 816 + 528
    mask, = re.findall(r"return \(lds_bytes - \(int\)sizeof\(TallLds<NW>\)\) & ~(\d+);", text[hip])
    assert int(mask) == 15
    # which launch gets how much LDS (the third argument of GDMIX_TALL_CASE: workgroups per CU), by wavefronts and LEAN
    wgs = {(nw, lean): w.strip() for nw, lean, w in re.findall(r"GDMIX_TALL_CASE\(\s*(\w+)\s*,\s*(true|false)\s*,\s*([^,]+),[^)]*\)\s*;", text[hip])}
    assert wgs == {("1", "true"): "TALL_LEAN_WGS", ("TALL_NW_MID", "false"): "TALL_MID_WGS", ("TALL_NW", "false"): "1",
                   ("TALL_NW_SMALL", "false"): "4 * GDMIX_TALL_WAVES_SMALL / TALL_NW_SMALL"}, wgs
    team_wgs, = re.findall(r"launch_tall_team_t\(.*?const int lds = tall_lds_bytes\((\d+)\);", text[hip], re.S)
    assert int(team_wgs) == 1
    # the numbers of the carve-up, of the two clamps (each inside its function) and of a team's split; the residency test's operator
    slack, = re.findall(r"\(ent \+ nnz \+ (\d+)\)", text[hip])
    assert int(slack) == th.TALL_TAIL == 8      # (tall_resident_bytes counts nnz + 8 entries)
    (rp_add, rp_mask), = re.findall(r"rp \+ \(\(ns \+ (\d+)\) & ~(\d+)\)", text[hip])
    assert (int(rp_add), int(rp_mask)) == (2, 1)      # (at most the n + 2 of tall_resident_bytes)
    for fn, nxt in (("tall_load_ranges", "tall_load_rows"), ("tall_load_rows", "tall_rows_fast")):
        body, = re.findall(rf"void {fn}\((.*?)void {nxt}\(", text[hip], re.S)
        clamp, = re.findall(r"i = i < n \? i : n - (\d+);", body)
        assert int(clamp) == 1, fn
    op, = re.findall(r"tall_resident_bytes\(NW,[^;]*?\)\s*(<=|<)\s*\(size_t\)arena_bytes", text[hip])
    assert op == "<="
    q_c, = re.findall(r"const int q = \(n \+ C - (\d+)\) / C;", text[hip])
    assert int(q_c) == 1 and th.team_slices(5)[0] == 2
    r8, = re.findall(r"tall_rows_fast<NW, (\w+), 8, PF, LOSS>", text[hip])
    assert r8 == "GDMIX_TALL_R8"
    (r_pf, r_plain), = re.findall(r"tall_rows_fast<NW, PF \? (\d+) : (\d+), 4, PF, LOSS>", text[hip])
    assert (int(r_pf), int(r_plain)) == (th.TALL_R4_PREFETCH, 1)
    step, = re.findall(r"for \(int h = 0; h < S; h \+= (\d+)\)", text[hip])
    assert int(step) == th.TALL_REDUCE
    assert {v: th.arena(v) for v in th.VARIANTS} == th.ARENA_FIGURES


@pytest.mark.parametrize("ic", [1, 0])
@pytest.mark.parametrize("has_w", [True, False])
@pytest.mark.parametrize("loss", th.LOSSES)
@pytest.mark.parametrize("variant", th.SOLO)
def test_trips(device_solver, variant, loss, has_w, ic):
    """n on R NT - 1, R NT, R NT + 1, 2 R NT - 1, 2 R NT, 2 R NT + 1 and 3 R NT + 1 of the variant's pass, per width class."""
    _run(device_solver, th.case(f"trips:{variant}", loss, has_w, ic))


EDGE_CASES = [(b,) + k for b in th.BATCHES if not b.startswith(("trips", "positions")) for k in th.cases_of(b)]


@pytest.mark.parametrize("batch,loss,has_w,ic", EDGE_CASES)
def test_edges(device_solver, batch, loss, has_w, ic):
    """arena, widths, structures, team_mixed: the three losses with weights and intercept, logistic also without each."""
    _run(device_solver, th.case(batch, loss, has_w, ic))


@pytest.mark.parametrize("which", ["one", "large"])
def test_an_entitys_bits_do_not_depend_on_its_place(device_solver, which):
    """A streamed entity whose last sample has one entry: first and in the middle of the batch its last windows run into the next
    entity's entries, last they read TallTail. Each batch against the reference, and the entity bit-equal in the three places."""
    for loss, has_w, ic in th.cases_of("positions"):
        out = []
        for place in th.POSITIONS:
            c = th.case(f"positions:{which},{place}", loss, has_w, ic)
            packed, res = _run(device_solver, c)
            out.append(_per_entity(c, packed, res))
        for other in out[1:]:
            _same_bits(out[0], other, [f"pos-{which}", "pos-filler0", "pos-filler1"])


@pytest.mark.parametrize("variant", th.SOLO)
def test_batch_order_does_not_change_an_entitys_bits(device_solver, variant):
    c, rev = th.case(f"trips:{variant}", "logistic", True, 1), th.case(f"trips:{variant}", "logistic", True, 1, reverse=True)
    assert rev["names"] == c["names"][::-1]
    packed, res, cls, _ = _solve(device_solver, c, twice=False)
    packed_r, res_r, cls_r, _ = _solve(device_solver, rev, twice=False)
    assert np.array_equal(cls, cls_r[::-1])
    _same_bits(_per_entity(c, packed, res), _per_entity(rev, packed_r, res_r), c["names"])


@pytest.mark.parametrize("loss", th.LOSSES)
@pytest.mark.parametrize("batch", ["trips:lean", "arena:one"])
def test_lean_proper_against_merged_lean(device_solver, monkeypatch, batch, loss):
    """A small lean class runs merged into the <1> launch (re_solve_tall_kernel<1, false> takes its entities); with
    GDMIX_RE_LEAN_MERGE_ROUNDS=0 it gets its own launch of re_solve_tall_kernel<1, true>. Identical bits, and the per-class times show
    which of the two ran: the only evidence that the lean instantiation itself ran at these shapes."""
    c = th.case(batch, loss, True, 1)
    lean = th.routed(c) == th.TALL_LEAN_CLASS
    assert lean.any()
    device_solver.set_timing(True)
    try:
        monkeypatch.delenv("GDMIX_RE_LEAN_MERGE_ROUNDS", raising=False)
        packed, merged, cls, _ = _solve(device_solver, c, twice=False)
        ms_merged = np.array(device_solver.last_solve_ms())
        monkeypatch.setenv("GDMIX_RE_LEAN_MERGE_ROUNDS", "0")
        packed_p, proper, cls_p, _ = _solve(device_solver, c, twice=False)
        ms_proper = np.array(device_solver.last_solve_ms())
    finally:
        device_solver.set_timing(False)
    assert np.array_equal(cls, cls_p) and np.array_equal(cls == th.TALL_LEAN_CLASS, lean)
    assert ms_merged[th.TALL_LEAN_CLASS] == 0.0 and ms_merged[th.TALL_ONE_CLASS] > 0.0, ms_merged[TALL_RANGE]
    assert ms_proper[th.TALL_LEAN_CLASS] > 0.0, ms_proper[TALL_RANGE]
    for k in BITWISE:
        assert np.array_equal(merged[k], proper[k]), k
    _compare(c, packed_p, proper)
