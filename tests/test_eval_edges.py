"""CPU checks of what tests/test_gpu_eval_edges.py stands on, so that it cannot pass by missing the edges it is about: the restated shape
of csrc/re_eval_sum.hpp shows every situation of the run, second-level and accumulator edges on a NAMED size, the term grid holds the
named scores (the overflow and underflow neighbours computed from long double), the integer recipes keep every partial sum exact, the
builders place every size in every position of a wavefront and every segment end on its edge, and the references alone satisfy what the
GPU file assumes of them. When a constant of the library moves (test_the_constants_are_the_librarys of the GPU file) and the helper
follows, the assertion that fails here names the situation that is gone."""
import math

import numpy as np

import eval_edges_helpers as eh
import metrics_reference as mref


def test_lane_situations_by_name():
    assert (eh.EVAL_THREADS, eh.EVAL_RUN, eh.EVAL_RUNS) == (256, 2048, 64)
    assert eh.ONE_RUN == 524_288 and eh.ONE_TOP == 33_554_432
    assert eh.RUN_EDGE_SIZES == (524_287, 524_288, 524_289, 524_545) and eh.TOP_EDGE_SIZE == 33_554_689
    below, on, above, row = (eh.lane_shape(n) for n in eh.RUN_EDGE_SIZES)
    # one sample short: the last lane closes no run, every other lane closes exactly one and adds nothing after it
    assert below["runs"][255] == 0 and below["terms"][255] == eh.EVAL_RUN - 1 and np.all(below["runs"][:255] == 1) and np.all(below["after_run"][:255] == 0)
    # a lane that closes exactly one run and adds nothing after it: every lane
    assert np.all(on["runs"] == 1) and np.all(on["after_run"] == 0) and np.all(on["tops"] == 0)
    # one that closes a run and adds one term (lane 0), next to one that adds none (lane 1)
    assert (above["runs"][0], above["after_run"][0]) == (1, 1) and (above["runs"][1], above["after_run"][1]) == (1, 0)
    # a full row more and one: lane 0 adds two terms to its closed run, the others one
    assert row["after_run"][0] == 2 and np.all(row["after_run"][1:] == 1) and np.all(row["runs"] == 1)
    # the second level: exactly closed; closed with one term behind it next to a lane with none; the size the GPU runs
    exact, one, run = eh.lane_shape(eh.ONE_TOP), eh.lane_shape(eh.ONE_TOP + 1), eh.lane_shape(eh.TOP_EDGE_SIZE)
    assert np.all(exact["tops"] == 1) and np.all(exact["after_top"] == 0) and np.all(exact["after_run"] == 0)
    assert (one["tops"][0], one["runs"][0], one["after_top"][0], one["after_run"][0]) == (1, 64, 0, 1), "closes 64 runs and adds one term"
    assert (one["tops"][1], one["after_top"][1], one["after_run"][1]) == (1, 0, 0), "the lane next to it does not"
    assert np.all(run["tops"] == 1) and np.all(run["runs"] == 64) and np.all(run["after_top"] == 0)
    assert np.all(run["after_run"][1:] == 1), "255 lanes close 64 runs and add one term"
    assert run["after_run"][0] == 2, "the lane next to them adds two"
    # no smaller entity reaches the second level, and the largest of the existing tests (200 000) closes no run at all
    assert np.all(eh.lane_shape(eh.ONE_TOP - 1)["tops"][255:] == 0) and np.all(eh.lane_shape(200_000)["runs"] == 0)
    for n in eh.RUN_EDGE_SIZES + (eh.TOP_EDGE_SIZE,):
        assert int(eh.lane_shape(n)["terms"].sum()) == n
        i = eh.last_lane_last_term(n)
        assert i % 256 == 255 and i < n <= i + 256, "the NaN sits in the last lane's last term"
        assert n < 1 << 31 and eh.sse_partial_sum_bound(n) < 1 << 53, "every partial sum of the integer data is an exact double"
    assert eh.sse_partial_sum_bound(eh.ACC_EDGE_SIZES[-1]) < 1 << 53


def test_accumulator_situations_by_name():
    assert (eh.ACC_MAX_GROUPS, eh.ACC_PER_THREAD, eh.ACC_GROUP_SAMPLES) == (4096, 16, 4096)
    assert eh.ACC_EDGE_SIZES == (4096, 4097, 65_536, 65_537, 16_777_216, 16_777_473)
    g1, g2, g16, g17, full, over = (eh.acc_shape(N) for N in eh.ACC_EDGE_SIZES)
    assert g1["groups"] == 1 and np.all(g1["terms"] == 16)
    assert g2["groups"] == 2 and g2["terms"][0] == 9 and np.all(g2["terms"][1:] == 8), "4 097 samples: a second workgroup"
    # a batch of 16 groups: lane 0 of the last tree takes all sixteen sums; of 17: lane 1 takes one
    assert g16["groups"] == 16 and list(g16["tree_take"][:2]) == [16, 0]
    assert g17["groups"] == 17 and list(g17["tree_take"][:3]) == [16, 1, 0]
    # the full grid: every lane 16 terms, every lane of the last tree 16 sums; one more trip: lanes of 17 and of 16 terms
    assert full["groups"] == 4096 and np.all(full["terms"] == 16) and np.all(full["tree_take"] == 16)
    assert over["groups"] == 4096 and np.all(over["terms"][:257] == 17) and np.all(over["terms"][257:] == 16)
    for N, s in zip(eh.ACC_EDGE_SIZES, (g1, g2, g16, g17, full, over)):
        assert int(s["terms"].sum()) == N and int(s["tree_take"].sum()) == s["groups"] and np.all(s["runs"] == 0)
    # the accumulator's own run closes only in a batch beyond every test's reach on one device call (2 048 terms a lane: 2^31 samples)
    assert eh.ACC_MAX_GROUPS * eh.EVAL_THREADS * eh.EVAL_RUN == 1 << 31


def test_term_grid_holds_the_named_scores():
    eh.require_long_double()
    s = eh.term_scores()
    names = eh.named_scores()
    counts = eh.exponent_counts(s)
    assert np.all(counts[:, :255] >= 1024), "every fp32 exponent, denormals included, both signs"
    assert s.size >= 2 * 255 * 2048 and not np.isnan(s).any()
    have = set(s.view(np.uint32).tolist())
    for name, v in names.items():
        assert np.float32(v).view(np.uint32).item() in have, name
        if name not in eh.NO_WINDOW:
            w = eh._window(v)
            assert w.size == 2 * eh.WINDOW + 1 and set(w.view(np.uint32).tolist()) <= have, name
    # the neighbours of the ends are what long double says they are
    last, first_inf = names["exp_last_finite"], names["exp_first_inf"]
    assert first_inf == np.nextafter(last, np.float32(np.inf)) and np.isfinite(eh.exp64(last)) and np.isposinf(eh.exp64(first_inf))
    assert abs(float(last) - 709.78) < 1e-2 and eh.exp64(last) > 2.0 ** 1023, "kf = 1024 with p < 1"
    assert round(float(last) * 1.4426950408889634) == 1024
    nz, z = names["exp_last_nonzero"], names["exp_first_zero"]
    assert z == np.nextafter(nz, np.float32(-np.inf)) and eh.exp64(nz) == eh.TINY and eh.exp64(z) == 0.0 and abs(float(nz) + 745.13) < 1e-2
    assert 0.0 < eh.exp64(names["exp_subnormal_from"]) < eh.MIN_NORMAL and eh.exp64(np.float32(-708.39)) >= eh.MIN_NORMAL
    # the ties of the reduction's rint: odd multiples of ln 2 / 2 have fp32 neighbours on both sides of half an integer
    for k in (1, 3, 5, 7):
        w = eh._window(names[f"tie+{k}"]).astype(np.float64) * 1.4426950408889634
        assert w.min() < k / 2 < w.max()
    denormal = s[(np.abs(s) > 0) & (np.abs(s) < np.finfo(np.float32).tiny)]
    assert denormal.size >= 2048 and np.isinf(s).sum() == 2 and (s == 0).sum() >= 2
    assert np.float32(eh.LL_LABELS[2]) == np.float32(0.5) and np.float32(eh.LL_LABELS[3]) > np.float32(0.5) and eh.LL_LABELS[3] - 0.5 == 2.0 ** -24


def test_references_alone_satisfy_what_the_gpu_file_assumes():
    eh.require_long_double()
    s = eh.term_scores()
    # the header's ce: finite or +inf, never NaN, never negative, on the whole grid and every label
    for y in eh.LL_LABELS:
        ref, u = eh.ll_reference(s, np.full(s.shape, y, np.float32))
        assert not np.isnan(ref).any() and np.all(ref >= 0)
        inf = np.isinf(s)
        assert np.all(np.isfinite(ref[~inf])) and np.all((ref[inf] == 0) | np.isposinf(ref[inf]))
        assert np.all(np.isfinite(u[~inf]))
    a = eh.ll_reference(s, np.full(s.shape, eh.LL_LABELS[2], np.float32))[0]
    b = eh.ll_reference(s, np.full(s.shape, eh.LL_LABELS[3], np.float32))[0]
    big = np.isfinite(s) & (np.abs(s) > 1)
    mag = np.abs(s[big].astype(eh.LD))
    assert np.all(np.abs(np.abs(a[big] - b[big]) - mag) <= mag * 2.0 ** -60), "0.5 is a negative, the next float a positive: the terms differ by |s|"
    # the statement the library's own host function is NOT used for: it gives NaN at an infinite score
    from gdmix_amd import metrics
    with np.errstate(all="ignore"):
        assert np.isnan(metrics.logistic_loss_terms(np.array([np.inf], np.float32), np.array([1.0], np.float32))[0])
    # the Poisson term: NaN exactly at s = +inf with y >= 0 and s = -inf with y = 0; the cancellation label cancels where fp32 can hold it
    for which in eh.PL_LABELS:
        y = eh.pl_labels(s, which)
        ref, ue, ur, e = eh.pl_reference(s, y)
        want_nan = (np.isposinf(s) & (y >= 0)) | (np.isneginf(s) & (y == 0))
        assert np.array_equal(np.isnan(ref), want_nan), which
        assert np.all(np.isfinite(y))
    y = eh.cancel_labels(s)
    ref, ue, ur, e = eh.pl_reference(s, y)
    mid = np.isfinite(s) & (np.abs(s) > 2.0 ** -20) & (s > -80) & (s < 80)
    ys = y[mid].astype(eh.LD) * s[mid].astype(eh.LD)
    assert np.all((ys > e[mid] / 2) & (ys < e[mid] * 2)) and np.all(np.abs(ref[mid]) < e[mid] * 2.0 ** -20)
    # ulp: the spacing of the binade, the subnormal spacing at the bottom
    assert [float(x) for x in eh.ulp(np.array([1.0, 1.5, 2.0, 0.75, 0.0, 1e-320, 2.0 ** -1022], eh.LD))] == [2.0 ** -52, 2.0 ** -52, 2.0 ** -51, 2.0 ** -53, eh.TINY,
                                                                                                             eh.TINY, eh.TINY]
    # the bound's categories on hand-made terms
    sc = np.array([0.0, -740.0, 800.0, np.inf, -np.inf], np.float32)
    yy = np.array([0.0, 0.0, 3.0, 1.0, 0.0], np.float32)
    ref, ue, ur, e = eh.pl_reference(sc, yy)
    with np.errstate(over="ignore"):
        got = ref.astype(np.float64)
    b, ref64 = eh.pl_term_bound(got, ref, ue, ur, e)
    assert 0.98 * 2.0 ** -52 < float(b[0]) < 1.5 * 2.0 ** -52 and float(b[1]) == eh.TINY and np.isnan(b[2:]).all()
    assert np.isposinf(ref64[2]) and np.isnan(ref64[3]) and np.isnan(ref64[4])


def test_recipes_are_exact_and_sensitive():
    i = np.arange(0, 5000, dtype=np.int64)
    s, y, d = eh.sse_recipe(i)
    assert d.min() == 0 and d.max() == 1020 and np.array_equal(y - s, d) and s.min() == -3 and s.max() == 3
    assert np.all(d[1:] != d[:-1]) and np.all(d[256:] != d[:-256]), "a dropped term with its neighbour repeated changes the sum"
    assert np.array_equal(s.astype(np.float32).astype(np.int64), s) and np.array_equal(y.astype(np.float32).astype(np.int64), y)
    s, y = eh.unit_recipe(i)
    assert not s.any() and set(y.tolist()) == {0, 1, 2, 3, 4}
    s, y, code = eh.mixed_recipe(i)
    assert set(s.tolist()) == {-1, 0, 1, 2} and set(y.tolist()) == {0, 1, 2, 3} and set(code.tolist()) == set(range(16))
    assert np.array_equal(code // 4 - 1, s) and np.array_equal(code % 4, y)
    from gdmix_amd import metrics
    for which, terms in (("pl", metrics.poisson_loss_terms), ("ll", metrics.logistic_loss_terms)):
        tot, mag = eh.mixed_sums(np.bincount(code, minlength=16), which)
        want = math.fsum(terms(s.astype(np.float32), y.astype(np.float32)).tolist())
        assert abs(tot - want) <= 1e-15 * mag and mag >= abs(tot) > 0      # (the fp64 statement rounds each term, the table each entry)
    # one missing term of size ~1 among 524 288 is far outside the header's bound
    assert 1.0 / eh.mixed_sums(np.full(16, eh.ONE_RUN // 16), "pl")[1] > 1e4 * eh.PL_BOUND


def test_quad_sweep_has_every_size_in_every_position():
    rp, s, y, sizes = eh.quad_sweep()
    E = sizes.size
    assert E % 4 == 3 and np.array_equal(np.diff(rp), sizes) and rp[-1] == s.size == y.size
    full = sizes[:E - 3].reshape(-1, 4)
    seen = {(int(n), p) for row in full for p, n in enumerate(row)}
    assert {(n, p) for n in range(67) for p in range(4)} <= seen, "every n in 0 .. 66 at each of the four positions"
    assert {(n, p) for n in eh.OTHERS for p in range(4)} <= seen
    # the widths: a wavefront of width 16, 32 and 64 with 16 | 17 and 32 | 33 inside, and one that leaves an entity to the large path
    small = np.where(full <= 64, full, 0).max(axis=1)
    for lo, hi in ((16, 16), (17, 17), (32, 32), (33, 33), (64, 64)):
        assert np.any((small >= lo) & (small <= hi))
    assert np.any((full == 16).any(axis=1) & (full == 17).any(axis=1)) and np.any((full == 32).any(axis=1) & (full == 33).any(axis=1))
    assert np.any((full > 64).any(axis=1))
    for tail in (1, 2, 3):
        prp, ps, py, psz = eh.quad_prefix(tail)
        assert psz.size % 4 == tail and prp[-1] == ps.size == py.size and prp.size == psz.size + 1
    nan_sizes = sorted(int(sizes[e]) for e in range(E) if np.isnan(s[rp[e]:rp[e + 1]]).any())
    assert len(nan_sizes) == 4 and nan_sizes[0] <= 16 < nan_sizes[1] <= 32 < nan_sizes[2] <= 64 < nan_sizes[3], "one NaN score in an entity of each width"
    assert (s == 0).sum() > 100 and np.signbit(s[s == 0]).any() and not np.isinf(s).any()
    assert set(eh.LIMITS) == {64, 33, 32, 17, 16, 1, 0} and eh.KS == (1, 16, 63, 64)


def test_packed_maxima_reach_the_fields_maxima():
    import ranking_reference as rref
    rp, s, y, names = eh.packed_maxima()
    assert list(np.diff(rp)) == [64] * 4
    ref = mref.per_entity_reference(rp, s, y)
    at = {n: e for e, n in enumerate(names)}
    assert ref["two_u"][at["two_u_2048"]] == 2048 and (ref["n_pos"][at["two_u_2048"]], ref["n_neg"][at["two_u_2048"]]) == (32, 32)
    assert ref["two_u"][at["all_equal_mixed"]] == 1024
    assert ref["n_nan"][at["all_nan"]] == 64 and ref["n_pos"][at["all_nan"]] == 0
    c = rref.per_entity_counts(rp, s, y, eh.KS)
    e = at["all_equal_positive"]
    assert eh.KS[0] == 1 and c["tie_size"][0, e] == 64 and c["tie_pos"][0, e] == 64 and c["slots"][0, e] == 1
    assert c["hits_sure"][3, e] == 64 and c["tie_size"][3, e] == 0, "n = k = 64: every sample is sure"


def test_rank_edges_place_the_segment_ends():
    rp, s, y, names = eh.rank_edges()
    ends = {n: int(rp[e + 1]) for n, e in names.items()}
    T = eh.RANK_TILE
    assert (eh.RANK_THREADS, eh.RANK_ITEMS, T) == (256, 16, 4096)
    assert [ends[k] for k in ("ends_15", "ends_16", "ends_17", "ends_4095", "ends_4096", "ends_4097", "ends_8192")] == [15, 16, 17, T - 1, T, T + 1, 2 * T]
    e = names["tie_over_three_tiles"]
    a, b = int(rp[e]), int(rp[e + 1])
    assert b - a == 10_000 and (b - 1) // T - a // T == 2, "one tie group over three tiles"
    seg = slice(a, b)
    assert np.unique(s[seg]).size == 1 and 0 < (y[seg] > 0.5).sum() < 10_000
    two_u, n_pos, n_neg, _ = mref.two_u_reference(s[seg], y[seg])
    assert two_u == n_pos * n_neg
    # 70 entities of 65: a wavefront of the walk (64 threads of 16 keys) holds several segments; the entity of 5 000 holds whole wavefronts
    wave = 64 * eh.RANK_ITEMS
    a65, b65 = int(rp[names["of_65_0"]]), int(rp[names["of_65_69"] + 1])
    assert b65 - a65 == 70 * 65 and any(a65 <= w and w + wave <= b65 for w in range(0, int(rp[-1]), wave))
    a5, b5 = int(rp[names["of_5000"]]), int(rp[names["of_5000"] + 1])
    assert sum(a5 <= w and w + wave <= b5 for w in range(0, int(rp[-1]), wave)) >= 3
    # NaN keys at a segment's end exactly on a tile edge
    e = names["nan_at_tile_edge"]
    assert ends["nan_at_tile_edge"] % T == 0 and ends["nan_at_tile_edge"] == rp[-1] and np.isnan(s[rp[e]:rp[e + 1]]).sum() == 3
    assert np.isnan(s[rp[names["ends_4095"]]:rp[names["ends_4095"] + 1]]).sum() == 1
    assert rp[names["empty"] + 1] == rp[names["empty"]]
