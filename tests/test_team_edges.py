"""CPU checks of what tests/test_gpu_team_edges.py stands on, so that it cannot pass by missing the edges it is about: the generators
give exactly the stated column and row lengths, team_edges_helpers.column_pass_plan shows every situation of team_fg's column pass
(csrc/re_solve_team.hpp) on the edge entities, route_large states the tier rules, and the REFERENCE's own run of every case is
reproducible (strict) on every edge entity."""
import numpy as np
import pytest

import class_caps_helpers as ch
import team_edges_helpers as th


def _plans():
    b = th.edge_batch("logistic")
    return {(name, ic): th.column_pass_plan(th.entity_col_ptr(b, e), ic) for e, name in enumerate(th.EDGE_NAMES) for ic in (1, 0)}


def test_generators_give_the_stated_lengths():
    b = th.edge_batch("logistic")
    b.validate()
    assert b.E == th.N_EDGE + th.FILLERS and b.weight is not None and 0.25 <= b.weight.min() and b.weight.max() < 2.25
    for e, (name, kind, size, lens) in enumerate(th.edge_entities()):
        r0, r1 = int(b.ent_row_ptr[e]), int(b.ent_row_ptr[e + 1])
        cols = np.diff(th.entity_col_ptr(b, e))
        rows = np.diff(b.row_nnz_ptr[r0:r1 + 1])
        if kind == "columns":
            assert r1 - r0 == size and np.array_equal(cols, lens), name
        else:
            assert cols.size == size and np.array_equal(rows, lens + [size]), name
        for i in range(r0, r1):      # distinct columns inside a row, distinct rows inside a column
            c = b.col_global[b.row_nnz_ptr[i]:b.row_nnz_ptr[i + 1]]
            assert np.unique(c).size == c.size, (name, i)
    n, nnz = b.ent_n(), b.ent_nnz()
    assert np.all(n[th.N_EDGE:] == 1) and np.all(nnz[th.N_EDGE:] == 1)
    shape = dict(zip(th.EDGE_NAMES, zip(n.tolist(), nnz.tolist())))
    assert shape["mixed"][0] == 2100 and 31000 < shape["mixed"][1] < 32000 and len(th.edge_entities()[0][3]) == 388
    assert shape["cap256"][1] == 256 * 2048 + sum(th.short(20)) and shape["one_col"] == (2049, 2049) and shape["four_col"][0] == 2048
    e = th.EDGE_NAMES.index("rows")
    assert shape["rows"][0] == 66 and int((np.diff(b.row_nnz_ptr[b.ent_row_ptr[e]:b.ent_row_ptr[e + 1] + 1]) == 0).sum()) == 10
    assert [len(e[3]) for e in th.edge_entities()[5:8]] == [1100, 1024, 512]      # p = 1101 / 1025 / 513 with an intercept, 1100 / 1024 / 512 without


def test_the_plan_of_hand_made_columns():
    """column_pass_plan on pointers small enough to follow by hand."""
    # intercept + 63 columns of 16: one tile, lane per column
    p = th.column_pass_plan(np.arange(64) * 16, 1)
    assert p["split"] == [] and len(p["tiles"]) == 1 and p["tiles"][0]["path"] == "lane"
    # the same without an intercept and one column of 17 more: still one tile, now chunked: 63 * 16 + 17 = 1025 entries, chunks of 512, 512, 1
    p = th.column_pass_plan(np.concatenate([np.arange(64) * 16, [1025]]), 0)
    assert len(p["tiles"]) == 1 and p["tiles"][0]["path"] == "chunked" and [c["owners"] for c in p["tiles"][0]["chunks"]] == [32, 32, 1]
    # a split column of 2049 in front of one of 600: chunks 0 .. 3 lie inside the split column, chunk 4 holds its last entry and 511 of the other
    p = th.column_pass_plan(np.array([0, 2049, 2649]), 1)
    assert p["split"] == [0] and p["tiles"][0]["first_is_split"] and p["tiles"][0]["n_split"] == 1
    assert [(c["owners"], c["masked"]) for c in p["tiles"][0]["chunks"]] == [(0, True)] * 4 + [(1, True), (1, False)]
    # 2047 is not split; with the cap at 0 neither is 2048
    assert th.column_pass_plan(np.array([0, 2047]), 0)["split"] == [] and th.column_pass_plan(np.array([0, 2048]), 0, n_long_cap=0)["split"] == []
    # the tile boundary moves by one lane with the intercept
    assert len(th.column_pass_plan(np.arange(65), 0)["tiles"]) == 1 and len(th.column_pass_plan(np.arange(65), 1)["tiles"]) == 2


def test_the_edge_entities_cover_the_column_pass():
    """Every situation team_fg branches on occurs in some edge entity. Each assertion names its situation: when a constant of the library
    moves (test_the_constants_are_the_librarys), the one that fails says which shape to move."""
    plans = _plans()
    tiles = [t for p in plans.values() for t in p["tiles"]]
    chunks = [c for t in tiles for c in t["chunks"]]
    assert any(t["path"] == "lane" and th.TEAM_SHORT_COL in t["lens"] for t in tiles), "a lane-per-column tile with a column of exactly TEAM_SHORT_COL"
    assert any(t["path"] == "chunked" and max(t["lens"]) == th.TEAM_SHORT_COL + 1 for t in tiles), "a chunked tile whose longest non-split column is TEAM_SHORT_COL + 1"
    assert any(len(t["chunks"]) > 1 for t in tiles), "a tile of more than one chunk"
    assert any(c["owners"] == 1 for c in chunks), "a one-owner chunk"
    assert any(c["owners"] == 1 and c["masked"] for c in chunks), "a one-owner chunk holding masked entries of a split column"
    assert any(c["owners"] >= 2 for c in chunks), "a multi-owner chunk"
    assert any(c["owners"] == 0 for c in chunks), "a skipped chunk"
    assert any(t["n_split"] >= 9 for t in tiles), "a tile owning at least 9 split columns (two rounds of the collection)"
    assert any(t["first_is_split"] and t["path"] == "chunked" for t in tiles), "a chunked tile whose first feature lane is a split column"
    split_lens = {n for t in tiles for n in t["split_lens"]}
    assert th.TEAM_LONGC in split_lens and th.TEAM_LONGC + 1 in split_lens, "split columns of TEAM_LONGC and TEAM_LONGC + 1"
    assert any(th.TEAM_LONGC - 1 in t["lens"] for t in tiles), "a non-split column of TEAM_LONGC - 1"
    assert any(len(p["split"]) == th.TEAM_LONG_CAP for p in plans.values()), "a split list of exactly TEAM_LONG_CAP"
    assert any(p["n_long"] == th.TEAM_LONG_CAP + 1 and p["split"] == [] for p in plans.values()), "TEAM_LONG_CAP + 1 long columns and none split"
    # what the table of the helper says of single entities
    for ic in (1, 0):
        last = plans[("mixed", ic)]["tiles"][-1]
        assert len(plans[("mixed", ic)]["tiles"]) == 7 and len(last["lens"]) + last["n_split"] == 5 - (1 - ic) and last["n_split"] == 1 and last["path"] == "chunked"
        assert all(t["path"] == "chunked" and t["n_split"] == 0 for t in plans[("cap257", ic)]["tiles"][:4])
        assert sum(t["n_split"] for t in plans[("cap256", ic)]["tiles"]) == 256
        assert plans[("one_col", ic)]["split"] == [0] and plans[("four_col", ic)]["split"] == [0] and plans[("four_col", ic)]["tiles"][0]["path"] == "chunked"
        assert -(-2049 // th.WAVE) == 33 and 33 * 63 > 2049      # slice size 33: the last slice of the 2 049-entry column is empty
        for name in ("wide1101", "wide1025", "wide513"):
            assert all(t["path"] == "lane" for t in plans[(name, ic)]["tiles"]) and plans[(name, ic)]["split"] == []
    assert [len(plans[(n, 1)]["tiles"]) for n in ("wide1101", "wide1025", "wide513")] == [18, 17, 9]
    assert [len(plans[(n, 0)]["tiles"]) for n in ("wide1101", "wide1025", "wide513")] == [18, 16, 8]


def test_route_large():
    """Below the thresholds route_large is class_caps_helpers.route; on and above them the tiers, the device-wide class and the tall
    rule's precedence, on boundary shapes written out by hand."""
    for p, n, z, k in ch.edges() + [s[:4] for s in ch.neighbours()]:
        for tall in (0, 32):
            assert th.route_large(p, n, z, 10, False, tall) == ch.route(p, n, z, 10, False, tall)
    for p, n, z, k, _ in ch.wave_bucket_shapes(False):
        assert th.route_large(p, n, z, 12, False, 0) == k
    B, T128, T32, T8, G = th.BLOCK_CLASS, th.TEAM128_CLASS, th.TEAM32_CLASS, th.TEAM8_CLASS, th.GIANT_CLASS
    assert (B, T128, T32, T8, G) == (35, 36, 37, 38, 39) and ch.BLOCK_CLASS == B
    small = ch.route(41, 60, 63, 10, True, 0)
    assert small < 28
    # (p, n, nnz, tall_min_n, team_nnz, giant_nnz) -> class
    for args, want in (((41, 60, 63, 0, 64, 20000), small), ((41, 60, 64, 0, 64, 20000), T128), ((41, 60, 511, 0, 64, 20000), T128),
                       ((41, 60, 512, 0, 64, 20000), T32), ((41, 60, 8191, 0, 64, 20000), T32), ((41, 60, 8192, 0, 64, 20000), T8),
                       ((41, 60, 19999, 0, 64, 20000), T8), ((41, 60, 20000, 0, 64, 20000), G),
                       ((30, 40, 100, 32, 64, 20000), ch.TALL_LEAN_CLASS), ((30, 40, 100, 0, 64, 20000), T128), ((30, 40, 20000, 32, 64, 20000), G),
                       ((30, 31, 100, 32, 64, 20000), T128), ((65, 40, 100, 32, 64, 20000), T128),
                       ((81, 60, 16383, 32, 16384, 16777216), B), ((81, 60, 16384, 32, 16384, 16777216), T128),
                       ((81, 60, 131071, 32, 16384, 16777216), T128), ((81, 60, 131072, 32, 16384, 16777216), T32),
                       ((81, 60, 2097151, 32, 16384, 16777216), T32), ((81, 60, 2097152, 32, 16384, 16777216), T8),
                       ((81, 60, 16777216, 32, 16384, 16777216), G), ((2, 2049, 2049, 32, 16384, 16777216), th.TALL_ANY),
                       ((41, 60, 20000, 0, 64, 0), T8), ((41, 60, 20000, 0, 0, 0), B), ((41, 60, 64, 0, 0, 20000), small)):
        p, n, z, tall, team, giant = args
        assert th.route_large(p, n, z, 10, True, tall, team, giant) == want, (args, want)
    # more than ten pairs: both thresholds are off
    assert th.route_large(41, 60, 20000, 12, True, 0, 64, 20000) == B and th.route_large(41, 60, 64, 12, True, 0, 64, 20000) == ch.route(41, 60, 64, 12, True, 0)
    # the shapes of the GPU test's tier cases
    for which in th.TIER_SHAPES:
        c = th.tier_case(which)
        assert np.array_equal(c["b"].ent_n(), [s[1] for s in c["shapes"]]) and np.array_equal(c["b"].ent_nnz(), [s[2] for s in c["shapes"]])


@pytest.mark.parametrize("ic", [1, 0])
@pytest.mark.parametrize("loss", th.LOSSES)
def test_the_reference_is_strict_on_every_edge_entity(loss, ic):
    """Every edge entity is reproduced by the reference from starts moved by 1e-15, 1e-14 and 1e-13 and is no FACTR stop: the GPU tests
    compare them iteration for iteration. At least one runs past m = 10 iterations, so the history is full and team_products makes
    one-tile trips as well as two-tile trips."""
    c = th.case(loss, ic)
    r = th.reference(c)
    strict, nit = r["strict"][c["edge"]], r["nit"][c["edge"]]
    print(f"{c['name']}: strict {strict.astype(int).tolist()}, nit {nit.tolist()}; fillers strict {int(r['strict'][th.N_EDGE:].sum())} of {th.FILLERS}")
    assert np.array_equal(np.diff(r["coef_ptr"])[:th.N_EDGE], [len(e[3]) + ic if e[1] == "columns" else e[2] + ic for e in th.edge_entities()])
    assert strict.all(), [n for n, s in zip(th.EDGE_NAMES, strict) if not s]
    assert nit.max() < c["kw"]["max_iter"], nit
    assert r["strict"].mean() >= 0.5      # (re_poisson_helpers.compare asks for this share over all compared entities)
    if ic == 0:      # (the references of both are cached by now)
        both = np.concatenate([nit, th.reference(th.case(loss, 1))["nit"][c["edge"]]])
        assert both.max() > c["kw"]["m"], both


@pytest.mark.parametrize("which", sorted(th.TIER_SHAPES))
def test_the_reference_is_strict_on_the_tier_entities(which):
    c = th.tier_case(which)
    r = th.reference(c)
    print(f"{c['name']}: strict {r['strict'].astype(int).tolist()}, nit {r['nit'].tolist()}")
    assert r["strict"].all()
