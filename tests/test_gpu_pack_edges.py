"""The pack (csrc/re_pack.hip, csrc/re_pack_big.hip) held to the CPU reference BIT FOR BIT — its output is integers and copied floats,
there is no tolerance anywhere in this file — where the fixtures and the other pack tests do not reach: entities on and around every
constant that decides a tier or a path, in every feature space that opens or closes a path, with the bitmap and the counting sort on
and off; batches large enough for a wavefront of each of the three wavefront tiers to walk several entities (the pointers handed out
from lanes 1 and up, the loads requested one entity ahead, SKIP between SMALL entities, the LDS staging reused); more big entities than
one tile of big_head_kernel; and the column range check. What the batches must show for this to mean something is checked on the CPU by
tests/test_pack_edges.py.

A CHANGED CONSTANT or grid of the pack is changed in pack_edges_helpers too: test_the_constants_are_the_librarys fails until it is,
and tests/test_pack_edges.py then names the shapes to move."""
import os
import re

import numpy as np
import pytest

import pack_edges_helpers as pe
from gdmix_amd import solver as solver_module
from gdmix_amd.solver import GdmixReError, REDeviceSolver

pytestmark = pytest.mark.gpu

ERANGE = -4      # GDMIX_RE_ERANGE (include/gdmix_re.h)


def _entity_of(x, name, i):
    """The entity that owns element i of array `name` of a packed batch."""
    E = x["E"]
    ents = np.arange(E + 1)
    starts = {"unique_global": x["ent_feat_ptr"], "row_ptr": None, "col_ptr": x["ent_nnz_ptr"] + ents}.get(name, x["ent_nnz_ptr"])
    if name in ("ent_feat_ptr", "ent_nnz_ptr"):
        return min(int(i), E - 1)
    if starts is None:
        starts = x["ent_row_ptr"] + ents
    return int(np.searchsorted(starts, i, side="right") - 1)


def _check(packed, x, b, what):
    """Every array of the packed batch and its maxima equal expected(b). A difference names the array, the first entity that differs, its
    samples and non-zeros and its (tier, path)."""
    x = dict(x, ent_row_ptr=b.ent_row_ptr)
    assert (packed.E, packed.N, packed.Z, packed.D) == (x["E"], x["N"], x["Z"], x["D"]), what
    got = dict(ent_feat_ptr=packed.ent_feat_ptr(), ent_nnz_ptr=packed.ent_nnz_ptr(), unique_global=packed.unique_global(), csr_col=packed.csr_col(),
               row_ptr=packed.row_ptr(), col_ptr=packed.col_ptr(), csc_row=packed.csc_row(), csc_val=packed.csc_val())
    for name, t in got.items():
        g, w = t.cpu().numpy(), x[name]
        assert g.shape == w.shape, (what, name, g.shape, w.shape)
        if name == "csc_val":
            g, w = g.view(np.uint32), w.view(np.uint32)
        differ = g != w
        if name == "col_ptr":
            differ &= x["col_ptr_defined"]
        if differ.any():
            i = int(np.flatnonzero(differ)[0])
            e = _entity_of(x, name, i)
            n, nnz = int(b.ent_n()[e]), int(b.ent_nnz()[e])
            z0 = int(x["ent_nnz_ptr"][e])
            routes = [pe.plan(n, nnz, b.col_global[z0:z0 + nnz], on) for on in (True, False)]
            pytest.fail(f"{what}: {name}[{i}] is {g[i]}, expected {w[i]} ({int(differ.sum())} elements differ); first in entity {e} of {x['E']}: "
                        f"{n} samples, {nnz} non-zeros, (tier, path) {routes[0]} with the bitmap, {routes[1]} without")
    assert (packed.max_p, packed.max_n, packed.max_nnz) == (x["max_p"], x["max_n"], x["max_nnz"]), what


def test_the_constants_are_the_librarys():
    src = os.path.join(os.path.dirname(solver_module.LIB_PATH), "csrc")
    if not all(os.path.exists(os.path.join(src, f)) for f in pe.CONSTANTS):
        pytest.skip("the sources are not shipped next to the library: the constants cannot be read")
    for fname, constants in pe.CONSTANTS.items():
        with open(os.path.join(src, fname)) as fh:
            text = fh.read()
        for name, value in constants.items():
            found = re.findall(rf"\b{name}\s*=\s*(\d+(?:\s*<<\s*\d+)?)\s*[;,]", text)
            assert len(found) == 1 and eval(found[0]) == value, (fname, name, found, value)
        if fname == "re_pack.hip":
            assert re.findall(r"#define\s+GDMIX_PACK_LDS_KEYS\s+(\d+)", text) == [str(pe.GDMIX_PACK_LDS_KEYS)]
            assert "PACK_CAP1 = PACK_LDS_KEYS," in text and "PACK_LDS_KEYS = GDMIX_PACK_LDS_KEYS;" in text
            squeezed = " ".join(text.split())
            for line in pe.GRID_LINES:      # the grids the helper's table of wavefronts per CU was read from
                assert squeezed.count(line) == 1, line
            assert pe.TIER_WAVES_PER_CU == (32, 4 * 4, 4 * 2) and pe.PACK_WAVES * 8 == 32      # 8 workgroups of 4: the hardware's 32 wavefronts per CU
            assert "it0 += stride * WAVE" in text and pe.WAVE == 64      # a wavefront's next 64 trips sit one per lane
    assert pe.N_LIST[-1] == pe.PACK_CAP3 + 1 and {pe.GDMIX_PACK_LDS_KEYS, pe.PACK_CAP2, pe.PACK_CAP3, pe.PACK_RANK_MAX} < set(pe.NNZ_LIST)


def _env(monkeypatch, bitmap, big_count):
    for name, on in (("GDMIX_PACK_BITMAP", bitmap), ("GDMIX_PACK_BIG_COUNT", big_count)):
        if on:
            monkeypatch.delenv(name, raising=False)
        else:
            monkeypatch.setenv(name, "0")


# (the counting sort can be switched off where it would run: the largest column of the big entities below 2^11, i.e. the spaces up to 2 048)
EDGE_CASES = [(space, bitmap, big_count, ic) for space in pe.SPACES for bitmap in (True, False)
              for big_count in ((True, False) if space <= 1 << pe.BIG_COUNT_CBITS else (True,)) for ic in (1, 0)]


@pytest.mark.parametrize("space,bitmap,big_count,ic", EDGE_CASES)
def test_edge_entities_every_path(device_solver, monkeypatch, space, bitmap, big_count, ic):
    _env(monkeypatch, bitmap, big_count)
    b = pe.edge_batch(space)["b"]
    x = pe.expected_of(("edge", space), b, bool(ic))
    for k in range(2):      # (the context keeps its temporaries between calls)
        _check(device_solver.pack(b, has_intercept=bool(ic)), x, b, f"edge batch of space {space}, pack {k}")


@pytest.mark.parametrize("defer", [True, False])
@pytest.mark.parametrize("side_streams", ["default", "0"])
def test_wavefronts_that_walk_several_entities(device_solver, monkeypatch, side_streams, defer):
    """trips_batch(CUs of this device), an edge batch, the trips batch again on one context: both packs of the large batch are exact, and
    the small one between them would show lists, counters or staging left over from the large one. On the shared context and on one
    without side streams (GDMIX_RE_SIDE_STREAM=0: every stage on the caller's stream, empty tiers launched blind), with the compaction
    of the unique ids deferred and not (a context without side streams never defers)."""
    _env(monkeypatch, True, True)
    cus = device_solver.torch.cuda.get_device_properties(0).multi_processor_count
    e1, e2, e3 = pe.trips_sizes(cus)
    assert (e1 + e2 + e3) * 110 < pe.MAX_TRIPS_NNZ, f"{cus} CUs: the trips batch would have about {(e1 + e2 + e3) * 100} non-zeros; size it anew instead of shrinking it"
    big = pe.trips_batch(cus)
    assert big.Z < pe.MAX_TRIPS_NNZ, (cus, big.Z)
    tier, _ = pe.batch_plan(big)
    counts = [int((tier == t).sum()) for t in (1, 2, 3)]
    waves = [w * cus for w in pe.TIER_WAVES_PER_CU]
    print(f"trips batch for {cus} CUs: E {big.E}, N {big.N}, Z {big.Z}; tier counts {counts} for at most {waves} wavefronts: "
          f"{[round(c / w, 2) for c, w in zip(counts, waves)]} trips each (the first tier walks all {big.E}: {big.E / waves[0]:.2f})")
    assert all(c > 2 * w for c, w in zip(counts, waves))
    small = pe.edge_batch(2049)["b"]
    xb, xs = pe.expected_of(("trips", cus), big), pe.expected_of(("edge", 2049), small)
    if side_streams == "0":
        monkeypatch.setenv("GDMIX_RE_SIDE_STREAM", "0")
        solver = REDeviceSolver(0)
    else:
        solver = device_solver
    try:
        solver.set_defer_unique(defer)
        _check(solver.pack(big), xb, big, "trips batch, first pack")
        _check(solver.pack(small), xs, small, "edge batch after the trips batch")
        _check(solver.pack(big), xb, big, "trips batch, second pack")
    finally:
        if solver is device_solver:
            solver.set_defer_unique(os.environ.get("GDMIX_RE_DEFER_UNIQUE", "1") != "0")
        else:
            solver.close()


def test_more_big_entities_than_one_tile_of_the_head(device_solver, monkeypatch):
    _env(monkeypatch, True, True)
    for space, path in ((2000, "counting"), (70000, "sort")):
        b = pe.many_big_batch(space)
        assert pe.big_path(b) == path
        x = pe.expected_of(("many_big", space), b)
        for k in range(2):
            _check(device_solver.pack(b), x, b, f"1 100 big entities on the {path} path, pack {k}")


def test_column_range(device_solver, monkeypatch):
    """Column 2^31 - 1 is legal in every tier; 2^31 and -1 are refused with GDMIX_RE_ERANGE whichever tier holds them, and the context
    packs exactly afterwards.

    No address is formed from such a column (read in csrc/re_pack.hip and csrc/re_pack_big.hip before this test was written): the
    wavefront tiers OR all columns of an entity and take the bitmap only when the OR is below 2 048 and the count only when it is below
    64 — 2^31 and -1 set bit 31 and more — so the entity goes to the rank sort or the bitonic network, which sort the low 32 bits as a
    key and copy them; big_maxcol_kernel leaves the column out of the maximum, big_hist_kernel and big_scatter_kernel index their tables
    by column & (C - 1), big_fill_kernel masks it into the key. This test exercises an error RETURN only."""
    _env(monkeypatch, True, True)
    top = pe.edge_batch(2 ** 31)
    b = top["b"]
    tier, _ = pe.batch_plan(b)
    holds = np.zeros(b.E, bool)
    holds[np.repeat(np.arange(b.E), b.ent_nnz())[b.col_global == 2 ** 31 - 1]] = True
    assert all((holds & (tier == t)).any() for t in pe.TIERS)
    x = pe.expected_of(("edge", 2 ** 31), b)
    assert x["unique_global"].max() == 2 ** 31 - 1
    _check(device_solver.pack(b), x, b, "column 2^31 - 1 in every tier")
    for big_count in (True, False):
        _env(monkeypatch, True, big_count)
        for value in (2 ** 31, -1):
            for t in pe.TIERS:
                with pytest.raises(GdmixReError, match=rf"\({ERANGE}\)"):
                    device_solver.pack(pe.with_bad_column(t, value))
        _check(device_solver.pack(b), x, b, "the edge batch after the refused ones")
