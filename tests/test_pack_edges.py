"""CPU checks of what tests/test_gpu_pack_edges.py stands on, so that it cannot pass by missing the edges it is about: the edge
batches of pack_edges_helpers show every (tier, path) pair of the pack (csrc/re_pack.hip, csrc/re_pack_big.hip) a feature space can
reach, every listed sample and non-zero count in every path the rules admit it to, and every row and column structure in every pair;
expected() agrees with a per-entity restatement that shares nothing with it; the trips batch has the tier sizes that make every
wavefront walk several entities, with every path and skipped entities in each of the first tier's trips.

Each assertion names what is missing: when a constant of the library moves (test_gpu_pack_edges.test_the_constants_are_the_librarys
says so), the message says which shapes of pack_edges_helpers to move."""
import numpy as np
import pytest

import pack_edges_helpers as pe

PAIRS = [(t, p) for t in (1, 2, 3) for p in pe.WAVE_PATHS]


def _reachable(space, bitmap_on):
    """The paths a wavefront tier can take with columns below `space`: the bitmap when it is on (every space has entities wholly below
    2 048); the rank sort when it is off, or a column can be 2 048 or above; the count always (every space keeps entities wholly below
    64); the bitonic network when a column can be 64 or above."""
    return [p for p, ok in (("bitmap", bitmap_on), ("rank", not bitmap_on or space > pe.PACK_BITMAP_COLS), ("count", True),
                            ("bitonic", space > pe.PACK_COUNT_COLS)) if ok]


def _planned(space, bitmap_on):
    c = pe.edge_batch(space)
    tier, path = pe.batch_plan(c["b"], bitmap_on)
    return c, tier, path


@pytest.mark.parametrize("space", pe.SPACES)
def test_the_plan_of_a_batch_is_the_plan_of_its_entities(space):
    """batch_plan (vectorised, used below and for the trips batch) against plan() entity by entity, and the generator against its specs."""
    c = pe.edge_batch(space)
    b = c["b"]
    b.validate()
    n, nnz = b.ent_n(), b.ent_nnz()
    assert b.E == len(c["specs"]) and np.array_equal(n, [s[0] for s in c["specs"]]) and np.array_equal(nnz, [s[1] for s in c["specs"]])
    assert 0 <= b.col_global.min() and b.col_global.max() == space - 1
    for on in (True, False):
        tier, path = pe.batch_plan(b, on)
        for e in range(b.E):
            z0 = int(b.row_nnz_ptr[b.ent_row_ptr[e]])
            t, p = pe.plan(n[e], nnz[e], b.col_global[z0:z0 + nnz[e]], on)
            assert (t, p or "") == (tier[e], path[e]), (e, c["specs"][e])
    assert 200 <= b.E <= 1000, b.E      # "a few hundred entities"


def test_plan_on_hand_made_entities():
    assert pe.plan(1, 0, [], True) == (1, "bitmap") and pe.plan(1, 0, [], False) == (1, "rank")
    assert pe.plan(256, 128, [2047], True) == (1, "bitmap") and pe.plan(256, 128, [2048], True) == (1, "rank")
    assert pe.plan(257, 128, [0], True) == (2, "bitmap") and pe.plan(300, 40, [5000], True) == (2, "rank")
    assert pe.plan(3, 129, [63], True) == (1, "count") and pe.plan(3, 129, [64], True) == (1, "bitonic")
    assert pe.plan(3, 256, [63], True) == (1, "count") and pe.plan(3, 257, [63], True) == (2, "count")
    assert pe.plan(3, 512, [99], True) == (2, "bitonic") and pe.plan(3, 513, [99], True) == (3, "bitonic")
    assert pe.plan(1024, 1024, [0], True) == (3, "count") and pe.plan(1025, 0, [], True) == (pe.BIG, None) and pe.plan(1, 1025, [0], True) == (pe.BIG, None)
    assert pe.trips_sizes(256) == (24576, 8792, 4396)


@pytest.mark.parametrize("space", pe.SPACES)
def test_every_reachable_tier_and_path_has_entities(space):
    for on in (True, False):
        c, tier, path = _planned(space, on)
        have = set(zip(tier.tolist(), path.tolist()))
        for t in (1, 2, 3):
            for p in _reachable(space, on):
                assert (t, p) in have, f"space {space}, bitmap {'on' if on else 'off'}: no entity of tier {t} on the {p} path"
        assert (pe.BIG, "") in have, f"space {space}: no big entity"
    want = "counting" if space <= 1 << pe.BIG_COUNT_CBITS else "sort"
    assert pe.big_path(c["b"], True) == want, f"space {space}: the big entities take {pe.big_path(c['b'], True)}, not {want}"
    assert pe.big_path(c["b"], False) == "sort"


def test_every_tier_and_path_over_the_spaces():
    have = set()
    for space in pe.SPACES:
        for on in (True, False):
            _, tier, path = _planned(space, on)
            have |= set(zip(tier.tolist(), path.tolist()))
    assert not [x for x in PAIRS if x not in have], [x for x in PAIRS if x not in have]
    assert {pe.big_path(pe.edge_batch(s)["b"], on) for s in pe.SPACES for on in (True, False)} == set(pe.BIG_PATHS)


@pytest.mark.parametrize("space", pe.SPACES)
def test_every_listed_size_in_every_path_that_admits_it(space):
    """Samples-wise: every n of N_LIST with 0, 1 and up to 128 non-zeros, on the bitmap and the rank sort of n's tier (n = 1 025: big).
    Non-zeros-wise: every nnz of NNZ_LIST with few samples, up to 128 on the bitmap and the rank sort, 129 to 1 024 on the count and the
    bitonic network, more on the big path."""
    for on in (True, False):
        c, tier, path = _planned(space, on)
        n, nnz = c["b"].ent_n(), c["b"].ent_nnz()
        for p in _reachable(space, on):
            sel = path == p
            if p in ("bitmap", "rank"):
                for v in pe.N_LIST[:-1]:
                    for k, what in ((nnz == 0, "no non-zero"), (nnz == 1, "one non-zero"), (nnz > 1, "2 to 128 non-zeros")):
                        if what == "no non-zero" and p == "rank" and on:
                            continue      # (an entity without columns has none of 2 048 or above: the bitmap takes it whenever it is on)
                        assert (sel & (n == v) & k & (tier == pe.tier_of(v, 0))).any(), f"space {space}, {p}: no entity of {v} samples and {what}"
                sizes = [v for v in pe.NNZ_LIST if v <= pe.PACK_RANK_MAX]
            else:
                sizes = [v for v in pe.NNZ_LIST if pe.PACK_RANK_MAX < v <= pe.PACK_CAP3]
            for v in sizes:
                if v == 0 and p == "rank" and on:
                    continue      # (an entity without columns has none of 2 048 or above: the bitmap takes it whenever it is on)
                assert (sel & (nnz == v) & (n <= 8) & (tier == pe.tier_of(1, v))).any(), f"space {space}, {p}: no entity of {v} non-zeros and few samples"
        big = tier == pe.BIG
        for k, what in ((nnz == 0, "no non-zero"), (nnz == 1, "one non-zero"), ((nnz > 1) & (nnz <= pe.PACK_RANK_MAX), "2 to 128 non-zeros")):
            assert (big & (n == pe.N_LIST[-1]) & k).any(), f"space {space}: no big entity of 1 025 samples and {what}"
        for v in [v for v in pe.NNZ_LIST if v > pe.PACK_CAP3]:
            assert (big & (nnz == v) & (n <= 8)).any(), f"space {space}: no big entity of {v} non-zeros and few samples"


@pytest.mark.parametrize("space", pe.SPACES)
def test_every_row_and_column_structure_in_every_tier_and_path(space):
    """Read from the ARRAYS, not from the specs. One entry per sample needs samples = non-zeros, which the bitmap and the rank sort of the
    512- and 1 024-key tiers cannot have (more than 256 samples, at most 128 non-zeros): not asked of those four pairs."""
    b = pe.edge_batch(space)["b"]
    n, nnz, E = b.ent_n(), b.ent_nnz(), b.E
    first, last, alternate, one_each, dup, single, distinct, d64, d65, border, all64, only63, only0 = (np.zeros(E, bool) for _ in range(13))
    for e in range(E):
        r0, r1 = int(b.ent_row_ptr[e]), int(b.ent_row_ptr[e + 1])
        k = np.diff(b.row_nnz_ptr[r0:r1 + 1])
        cols = b.col_global[int(b.row_nnz_ptr[r0]):int(b.row_nnz_ptr[r1])]
        if cols.size == 0:
            continue
        u = np.unique(cols)
        first[e] = k.size > 1 and k[0] == cols.size
        last[e] = k.size > 1 and k[-1] == cols.size
        alternate[e] = k.size > 2 and not k[1::2].any() and np.count_nonzero(k[0::2]) > 1
        one_each[e] = k.size > 1 and np.all(k == 1)
        start = np.cumsum(k) - k
        dup[e] = any(np.unique(cols[s:s + c]).size < c for s, c in zip(start[k > 1], k[k > 1]))
        single[e], distinct[e], d64[e], d65[e] = u.size == 1 and cols.size > 1, u.size == cols.size > 1, u.size == 64, u.size == 65
        at = np.arange(64, cols.size, 64)
        border[e] = at.size > 0 and np.all(cols[at] == cols[at - 1])
        all64[e], only63[e], only0[e] = u.size == 64 and u[-1] == 63, u.size == 1 and u[0] == 63, u.size == 1 and u[0] == 0
    for on in (True, False):
        tier, path = pe.batch_plan(b, on)
        pairs = [(t, p) for t in (1, 2, 3) for p in _reachable(space, on)] + [(pe.BIG, "")]
        for t, p in pairs:
            sel = (tier == t) & (path == p)
            where = f"space {space}, tier {t}, {p or 'big'}"
            for name, has in (("everything in the first sample", first), ("everything in the last sample", last), ("every other sample empty", alternate),
                              ("a column twice in one sample", dup), ("a single column", single), ("all columns distinct", distinct)):
                if name == "all columns distinct" and (p == "count" or p == "bitonic" and space <= pe.PACK_RANK_MAX or t == pe.BIG and space <= pe.PACK_CAP3):
                    continue      # (more non-zeros than columns: above 128 below column 64 or in a space of 65, above 1 024 in a space of fewer)
                assert (sel & has).any(), f"{where}: no entity with {name}"
            if not (t in (2, 3) and p in ("bitmap", "rank")):
                assert (sel & one_each).any(), f"{where}: no entity with one entry per sample"
            if p in ("bitmap", "rank") and space >= 64:
                assert (sel & d64 & (nnz <= pe.PACK_RANK_MAX)).any(), f"{where}: no entity of exactly 64 distinct columns"
            if p == "rank" and space >= 65 or p == "bitmap" and space > 65:      # (space 65 with the bitmap on: 65 distinct columns include column 64 ... which the bitmap holds too)
                assert (sel & d65 & (nnz <= pe.PACK_RANK_MAX)).any(), f"{where}: no entity of exactly 65 distinct columns"
            if p in ("count", "bitonic") or t == pe.BIG:
                assert (sel & border & (nnz > pe.PACK_RANK_MAX)).any(), f"{where}: no entity with equal columns on both sides of every 64-entry tile border"
            if p == "count":
                assert (sel & only0).any(), f"{where}: no entity of column 0 only"
                if space >= pe.PACK_COUNT_COLS:
                    assert (sel & all64).any() and (sel & only63).any(), f"{where}: no entity with all 64 columns / with column 63 only"
            if p in ("bitmap", "rank"):
                assert (sel & border).any(), f"{where}: no entity with equal columns on both sides of the tile border"
        # d = 1 up to 1 024 non-zeros, on the count and (a column of 64 or above) on the bitonic network
        for p in [q for q in ("count", "bitonic") if q in _reachable(space, on)]:
            assert ((path == p) & single & (nnz == pe.PACK_CAP3)).any(), f"space {space}, {p}: no single-column entity of 1 024 non-zeros"


def test_every_tier_first_and_last_and_the_top_column_in_every_tier():
    firsts, lasts = set(), set()
    for space in pe.SPACES:
        c = pe.edge_batch(space)
        b = c["b"]
        tier, _ = pe.batch_plan(b)
        n, nnz = b.ent_n(), b.ent_nnz()
        assert sorted(tier[:4]) == sorted(tier[-4:]) == [1, 2, 3, 4]
        assert sorted(nnz[:4]) == [256, 512, 1024, 2049] and sorted(n[-4:]) == [256, 512, 1024, 1025], "the entities at the ends of the batch sit at their tiers' capacities"
        firsts.add(int(tier[0]))
        lasts.add(int(tier[-1]))
        holds = np.zeros(b.E, bool)
        holds[np.repeat(np.arange(b.E), nnz)[b.col_global == space - 1]] = True
        for t in pe.TIERS:
            assert (holds & (tier == t)).any(), f"space {space}: column {space - 1} occurs in no entity of tier {t}"
    assert firsts == lasts == set(pe.TIERS), (firsts, lasts)


@pytest.mark.parametrize("space", pe.SPACES)
def test_expected_against_the_restatement(space):
    b = pe.edge_batch(space)["b"]
    x = pe.expected(b, True)
    n, nnz = b.ent_n(), b.ent_nnz()
    assert (x["max_n"], x["max_nnz"]) == (int(n.max()), int(nnz.max())) and pe.expected_of(("edge", space), b, False)["max_p"] == x["max_p"] - 1
    d_max, slots = 0, 0
    for e in range(b.E):
        r = pe.restated_entity(b, e)
        z0, f0, r0 = int(x["ent_nnz_ptr"][e]), int(x["ent_feat_ptr"][e]), int(b.ent_row_ptr[e])
        d = r["unique_global"].size
        assert x["ent_nnz_ptr"][e + 1] - z0 == nnz[e] and x["ent_feat_ptr"][e + 1] - f0 == d, e
        assert np.array_equal(x["unique_global"][f0:f0 + d], r["unique_global"]), e
        assert np.array_equal(x["row_ptr"][r0 + e:r0 + e + n[e] + 1], r["row_ptr"]), e
        assert np.array_equal(x["col_ptr"][z0 + e:z0 + e + d + 1], r["col_ptr"]) and x["col_ptr_defined"][z0 + e:z0 + e + d + 1].all(), e
        assert not x["col_ptr_defined"][z0 + e + d + 1:z0 + e + nnz[e] + 1].any(), e
        for k in ("csr_col", "csc_row", "csc_val"):
            assert np.array_equal(x[k][z0:z0 + nnz[e]], r[k]), (k, e)
        d_max, slots = max(d_max, d), slots + d + 1
    assert x["max_p"] == d_max + 1 and x["D"] == x["ent_feat_ptr"][-1] and int(x["col_ptr_defined"].sum()) == slots


def test_the_trips_batch():
    """At 256 CUs: the tier counts that give every wavefront of every tier's grid more than two entities, within 10 M non-zeros; every
    trip 0, 1, 2 of the first tier's walk (entities t x stride to (t + 1) x stride - 1 in batch order, stride = 32 wavefronts x 256 CUs)
    holds entities of all four paths and entities of the other tiers, which the walk skips; the mid tiers are two thirds large by
    their samples only."""
    cus = 256
    b = pe.trips_batch(cus)
    b.validate()
    tier, path = pe.batch_plan(b, True)
    n, nnz = b.ent_n(), b.ent_nnz()
    counts = tuple(int((tier == t).sum()) for t in (1, 2, 3))
    assert counts == pe.trips_sizes(cus) == (24576, 8792, 4396) and not (tier == pe.BIG).any() and b.E == 37764
    for t, w in zip((1, 2, 3), pe.TIER_WAVES_PER_CU):
        assert counts[t - 1] > 2 * w * cus, f"tier {t}: {counts[t - 1]} entities are no third trip for {w * cus} wavefronts"
    print(f"trips_batch({cus}): E {b.E}, N {b.N}, Z {b.Z}; tier counts {counts} for {[w * cus for w in pe.TIER_WAVES_PER_CU]} wavefronts")
    assert 3_000_000 <= b.Z <= 4_500_000 and b.Z < pe.MAX_TRIPS_NNZ and b.N < 7_000_000
    stride = pe.TIER_WAVES_PER_CU[0] * cus
    for trip in range(3):
        s = slice(trip * stride, (trip + 1) * stride)
        for p in pe.WAVE_PATHS:
            assert ((tier[s] == 1) & (path[s] == p)).any(), f"trip {trip} of the first tier: no entity on the {p} path"
        assert (tier[s] != 1).any(), f"trip {trip} of the first tier: nothing to skip"
        assert (np.diff((tier[s] == 1).astype(int)) != 0).sum() > 100, f"trip {trip}: SMALL and SKIP entities are not mixed"
    for t, lo in ((2, 256), (3, 512)):
        sel = tier == t
        share = float((sel & (n > lo) & (nnz <= 60)).sum()) / float(sel.sum())
        assert 0.6 < share < 0.72 and (sel & (nnz > lo)).sum() > 0.25 * sel.sum(), (t, share)
        for p in pe.WAVE_PATHS:
            assert (sel & (path == p)).any(), f"tier {t} of the trips batch: no entity on the {p} path"
        assert (sel & (n == 2 * lo)).any() and (sel & (nnz == 2 * lo)).any() and (sel & (n == lo + 1)).any() and (sel & (nnz == lo + 1)).any()
    assert ((tier == 1) & (n == 256)).any() and ((tier == 1) & (nnz == 256)).any()
    low = pe._ent_max_col(b) < pe.PACK_COUNT_COLS
    assert b.col_global.max() < 3000 and 0.08 < low[nnz > 0].mean() < 0.2


@pytest.mark.parametrize("space", [2000, 70000])
def test_the_many_big_batch(space):
    b = pe.many_big_batch(space)
    b.validate()
    tier, _ = pe.batch_plan(b)
    n, nnz = b.ent_n(), b.ent_nnz()
    assert b.E == 1100 > 1024 and np.all(tier == pe.BIG) and b.E < pe.BIG_HEAD_MAX
    heavy = nnz > pe.PACK_CAP3
    assert heavy.sum() == 30 and nnz.max() <= 5000 and heavy[[0, 1023, 1024, 1099]].all() and np.all(nnz[~heavy] <= 8) and np.all(n[~heavy] == 1025)
    assert (nnz[~heavy] == 0).any() and (n[heavy] < 40).any() and (n[heavy] == 1025).any()
    assert nnz[1024:].sum() > 0 and nnz[:1024].sum() > 0      # all three scans carry something over the tile border
    assert pe.big_path(b, True) == ("counting" if space <= 2048 else "sort") and b.col_global.max() == space - 1


@pytest.mark.parametrize("value", [2 ** 31, -1])
def test_the_bad_column_batches(value):
    for t in pe.TIERS:
        b = pe.with_bad_column(t, value)
        tier, _ = pe.batch_plan(b)
        assert tier.tolist() == [1, t, 1] and int(((b.col_global < 0) | (b.col_global > 2 ** 31 - 1)).sum()) == 1
        assert b.col_global[b.row_nnz_ptr[b.ent_row_ptr[1]]:b.row_nnz_ptr[b.ent_row_ptr[2]]].tolist().count(value) == 1
