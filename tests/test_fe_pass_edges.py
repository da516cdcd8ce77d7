"""CPU half of the fixed-effect edge suite (tests/test_gpu_fe_pass_edges.py is the GPU half): the helper's constants are the library's, r_ref
is measured anew, the restated plans of the edge shards show every situation the suite is there for — by name, with the shape to move —,
the tolerance law hides nothing (conditions (a) and (b)), and the reference agrees with a dense statement.

CHANGE A CONSTANT IN tests/fe_pass_edges_helpers.py FIRST, then run this file: it names what the shards no longer show."""
import os

import numpy as np
import pytest

import fe_pass_edges_helpers as H

B, TRIP = H.FE_B, H.TRIP


def test_the_constants_are_the_librarys():
    """The literals of tests/fe_pass_edges_helpers.py against gdmix_amd/csrc. When a constant of the passes moves: change it in the helper
    first (this test then fails on the old source line), run this file, and move the shapes the other tests name."""
    import gdmix_amd
    src = os.path.join(os.path.dirname(os.path.abspath(gdmix_amd.__file__)), "csrc")
    names = {f for f, _ in H.SOURCE_LINES}
    if not all(os.path.exists(os.path.join(src, f)) for f in names):
        pytest.skip("the sources are not shipped next to the package: the constants cannot be read")
    text = {}
    for f in names:
        with open(os.path.join(src, f)) as fh:
            text[f] = " ".join(fh.read().split())
    for fname, line in H.SOURCE_LINES:
        assert text[fname].count(line) == 1, (fname, line)
    assert (H.WAVE, H.FE_B, H.FE_U, H.TRIP, H.FE_THREADS) == (64, 2048, 8, 512, 256)
    assert (H.FE_STRANDS, H.FE_RED_OUT, H.FE_FIX_PER_BLOCK, H.FE_FIN_BLOCKS, H.FE_HOT_STRANDS) == (16, 16, 128, 64, 8)
    assert (H.FE_HOT_MAX, H.FE_HOT_REP, H.FE_HOT_MIN) == (64, 32, 65536)
    assert (H.FE_CTRIP, H.FE_CTRIP_BYTES, H.FE_CDELTA_MAX, H.FE_SPAN_BITS, H.FE_LOC_BITS) == (512, 3072, 31, 21, 11)
    assert (H.CHUNK_FLOOR, H.CHUNK_HOOK_MIN, H.CHUNK_CLIP, H.FE_COMPRESS_DEFAULT) == (8192, 64, 1 << 28, 2)
    assert 1 << H.FE_LOC_BITS == H.FE_B and H.FE_HOT_MAX * H.FE_HOT_REP <= H.FE_B


def plans(key):
    """[(hook set, PassPlans)] of a shard under its own hook sets (packed; the three-array form only changes the bytes per entry)."""
    return [(h, H.pass_plans(H.shard(key), h)) for h in H._HOOK_TABLE[key][0]]


def both(p):
    return (("row pass", p.rows), ("column pass", p.cols))


# ---- r_ref and the law -------------------------------------------------------------------------------------------------------------------
def test_r_ref_is_what_the_helper_holds():
    r, where, rows = H.measure_r_ref()
    print(f"r_ref = {r:.4f} at {where}; {len(rows)} (case, quantity) pairs")
    for q in H.QUANTITIES:
        sel = [max(x[2], x[3]) for x in rows if x[1] == q]
        print(f"  {q}: {min(sel):.3f} .. {max(sel):.3f}")
    assert r <= H.R_REF, f"measured r_ref {r} above the literal R_REF {H.R_REF}: raise it (two digits, rounded up) and the docs with it"
    assert H.R_REF <= max(1.0, np.ceil(r * 10 + 1) / 10), f"R_REF {H.R_REF} is no longer the measured {r} rounded up to two digits"
    assert H.K == 8 * max(H.R_REF, 1.0)


ALL_CASES = H.small_cases() + [("many_units",) + H.DEFAULT_CASE]


@pytest.mark.parametrize("key,loss,weighted,ic", ALL_CASES, ids=["-".join(map(str, c)) for c in ALL_CASES])
def test_the_law_hides_nothing(key, loss, weighted, ic):
    """(a) K E <= 1e-9 sum |terms| for every output of every quantity: no case is looser than the fit tests. (b) EVERY entry's term of the
    gradient (and of the Hessian diagonal) exceeds 4 K E of its column: one dropped, doubled or misrouted entry moves its column — seen from
    the row side, at least one column — by more than the test allows. The same for every sample's residual in the intercept's entry."""
    sh, ref = H.shard(key), H.reference(key, loss, weighted, ic)
    K = np.longdouble(H.K)
    for q in H.QUANTITIES:
        E, S = ref["E_" + q], ref["S_" + q]
        has = S > 0
        assert np.all(E[~has] == 0)
        worst = float(np.max(K * E[has] / S[has]))
        assert worst <= H.FIT_RTOL, f"(a) {key} {loss} {q}: K E / sum |terms| = {worst:.2e}: choose another seed for the shard"
    for q in ("grad", "diag"):
        bound = 4 * K * ref["E_" + q][sh.uniq][sh.lcol]
        ratio = float(np.min(ref["T_" + q] / bound))
        assert ratio > 1, f"(b) {key} {loss} {q}: an entry's term is {ratio:.2e} of 4 K E of its column: choose another seed for the shard"
    if ic:
        # (the residuals are not kept: |r_i| = T_grad / |v| on the rows with entries; an empty row's residual is one term of n in a sum of n)
        r_abs = ref["T_grad"] / np.abs(sh.val.astype(np.longdouble))
        assert float(np.min(r_abs)) > float(4 * K * ref["E_grad"][sh.D]), f"(b) {key} {loss}: a residual below 4 K E of the intercept's entry"
        assert ref["grad"][sh.D] != 0


SMALL_DENSE = ("square1", "strands1", "strands2", "hot1", "exact", "hotunits1", "strands16")


@pytest.mark.parametrize("key", SMALL_DENSE)
@pytest.mark.parametrize("loss,weighted,ic", [("logistic", True, 1), ("squared", False, 0), ("poisson", True, 1)])
def test_the_reference_against_a_dense_statement(key, loss, weighted, ic):
    sh = H.shard(key)
    T = np.longdouble
    X = np.zeros((sh.n, sh.D + 1), T)
    np.add.at(X, (sh.row, sh.col), sh.val.astype(T))
    X[:, sh.D] = ic
    w = sh.wt.astype(T) if weighted else np.ones(sh.n, T)
    y, o = sh.labels(loss).astype(T), sh.off.astype(T)
    ref = H.evaluate(sh, loss, weighted, ic)
    pick = lambda a: np.concatenate([a[:sh.D], a[sh.D:sh.D + ic]]).astype(T)
    z0 = X @ pick(sh.theta0) if ic else X[:, :sh.D] @ sh.theta0[:sh.D].astype(T)
    z0 = z0 + o
    ell, r, _, _ = H.loss_parts(loss, z0, y, w)
    P = sh.D + ic
    Xc = X[:, :P]
    tol = lambda E: np.maximum(E[:P] * T(2.0 ** -8), T(0))      # longdouble against longdouble: far inside the law
    assert np.all(np.abs(Xc.T @ r - ref["grad"][:P]) <= tol(ref["E_grad"]))
    assert abs(ell.sum() - ref["grad"][P]) <= ref["E_grad"][P] * T(2.0 ** -8)
    th1 = sh.theta1[:P].astype(T)
    z1 = Xc @ th1 + o
    Dd, _ = H.diag_parts(loss, z1, w)
    # per entry, not per cell: a column twice in a row adds v^2 twice, not (2 v)^2
    X2 = np.zeros((sh.n, sh.D + 1), T)
    np.add.at(X2, (sh.row, sh.col), sh.val.astype(T) ** 2)
    X2[:, sh.D] = ic
    assert np.all(np.abs(X2[:, :P].T @ Dd - ref["diag"][:P]) <= tol(ref["E_diag"]))
    _, _, D1, _ = H.loss_parts(loss, z1, y, w)
    hv = Xc.T @ (D1 * (Xc @ sh.vec[:P].astype(T)))
    assert np.all(np.abs(hv - ref["hv"][:P]) <= tol(ref["E_hv"]))
    assert np.all(ref["grad"][sh.absent] == 0) and np.all(ref["E_grad"][sh.absent] == 0)


# ---- the nine points, by name ------------------------------------------------------------------------------------------------------------
def test_point_1_blocks_of_outputs():
    sizes = {H.shard(f"square{s}").n for s in H.SQUARE_S}
    assert sizes == {1, B - 1, B, B + 1, 2 * B + 1}, "point 1: SQUARE_S must hold 1, FE_B - 1, FE_B, FE_B + 1 and 2 FE_B + 1"
    for s in H.SQUARE_S:
        sh = H.shard(f"square{s}")
        assert sh.n == sh.d == s, f"point 1: square{s} must have n = d = {s} (every column needs an entry)"
        for h, p in plans(f"square{s}"):
            assert p.rows.nblock == p.cols.nblock == -(-s // B)
    last_rows = {(H.shard(f"square{s}").n - 1) % B + 1 for s in H.SQUARE_S}
    assert {1, B} <= last_rows, "point 1: a last block of one row and one of exactly FE_B rows"
    assert any(H.shard(f"square{s}").d % H.FE_RED_OUT == 1 for s in H.SQUARE_S), "point 1: a last fe_finish_kernel workgroup with one live output"
    # fe_rows_fix_kernel's row < F.n guard is live: a cut last block that is not full
    assert any(p.nmulti and (p.multi[-1] + 1) * B > H.shard(f"square{s}").n for s in H.SQUARE_S for _, p in plans(f"square{s}")), \
        "point 1: a row block of several units that ends beyond n (chunk 64 on square2049 / square4097)"


def test_point_2_a_whole_block_next_to_a_cut_one_without_a_hook():
    (h, p), = plans("whole_and_cut")
    assert h == {}, "point 2 runs without a hook"
    for name, c in both(p):
        assert c.chunk == H.CHUNK_FLOOR and c.nblock == 2, f"point 2, {name}: two blocks at the 8 192-entry floor"
        assert [c.units_of_block(b) for b in (0, 1)] == [1, 2], f"point 2, {name}: one whole block, one of two units (move whole_and_cut's extra entry)"
        assert list(c.ulen) == [H.CHUNK_FLOOR, H.CHUNK_FLOOR, 1], f"point 2, {name}: 8 192, then 8 192 + 1"
    assert p.nmulti == 1 and list(p.multi) == [1] and p.nred == 3 + H.FE_FIX_PER_BLOCK


def test_point_3_trips():
    sh = H.shard("trips")
    seen = {}
    for h, p in plans("trips"):
        for name, c in both(p):
            for length, start in zip(c.ulen, c.ustart[:-1]):
                seen.setdefault((name, int(length)), set()).add(int(start) % 2)
    assert {h["chunk"] for h, _ in plans("trips")} == {64, TRIP, TRIP + 1}
    for name in ("row pass", "column pass"):
        for length in (TRIP, TRIP + 1, TRIP - 1, 1):
            assert (name, length) in seen, f"point 3, {name}: no unit of {length} entries (TRIPS_BLOCKS)"
        for length in (TRIP, TRIP + 1, TRIP - 1):
            assert 1 in seen[(name, length)], f"point 3, {name}: no unit of {length} entries starts at an odd entry (the first block must hold an odd count)"
    # accumulator 0 of either block is a live output with a non-zero sum, in both passes
    ref = H.reference("trips", *H.DEFAULT_CASE)
    for i in (0, B):
        assert sh.row_count[i] > 0 and ref["grad"][sh.uniq[i]] != 0, f"point 3: row / column {i} (accumulator 0) must hold entries"


def test_point_4_strand_sums():
    want = {1, 2, 16, 17, 48, 49, 64, 65, 81}
    seen = {"row pass": set(), "column pass": set()}
    for key in [f"strands{k}" for k in H.STRAND_UNITS_SMALL] + ["strands_big"]:
        for h, p in plans(key):
            assert h == {"chunk": 64}
            for name, c in both(p):
                seen[name] |= {c.units_of_block(b) for b in range(c.nblock)}
    for name in seen:
        assert want <= seen[name], f"point 4, {name}: no block of {sorted(want - seen[name])} units at chunk 64 (STRAND_UNITS_*)"
    hot = set()
    for k in H.HOT_UNITS:
        (h, p), = plans(f"hotunits{k}")
        assert p.hot.size > 0 and p.cols.nblock == p.vbase // B + 1
        hot.add(p.cols.units_of_block(p.vbase // B))
    assert hot == {1, 8, 9, 32, 33, 41}, f"point 4: the virtual block's units are {sorted(hot)} (HOT_UNITS: eight strands, unrolled by four)"


def test_point_5_empty_blocks_and_windows():
    sh = H.shard("empties")
    per_block = np.add.reduceat(sh.row_count, np.arange(0, sh.n, B))
    assert list(per_block > 0) == [True, False, True, False], "point 5: row blocks 1 and 3 (the last) of `empties` hold no non-zero"
    assert sh.row_count[0] == 0 and sh.row_count[-1] == 0, "point 5: the first and the last row are empty"
    for h, p in plans("empties"):
        r = p.rows
        assert r.nblock == 4 and r.units_of_block(1) == r.units_of_block(3) == 1, "point 5: an empty block keeps one unit"
        assert r.ulen[r.ufirst[1]] == 0 and r.ulen[r.ufirst[3]] == 0 and r.ublock[-1] == 3, "point 5: the last unit is an empty block's"
    # a column block without entries: every column of it is frequent
    p = dict((H.hook_id(h), q) for h, q in plans("hot2050"))[f"hot_min={H.HOT_H}"]
    assert H.shard("hot2050").d == B + 2 and set(p.hot) >= {B, B + 1}, "point 5: columns 2 048 and 2 049 of hot2050 are both frequent"
    assert p.cols.units_of_block(1) == 1 and p.cols.ulen[p.cols.ufirst[1]] == 0, "point 5: column block 1 of hot2050 is left without entries"
    w = H.shard("windows")
    assert (w.n, w.d) == (2 * B + 1, B + 1), "point 5: the windows shard has n = 4 097 and d = 2 049"
    bits = set()
    for h, p in plans("windows"):
        bits.add(h["window_bits"])
        for name, c in both(p):
            assert c.nwin > 1 and c.nunit < c.nblock * c.nwin, f"point 5, {name}: empty windows that are not a block's first keep no unit"
            assert np.mean(c.kbase > 0) > 0.5, f"point 5, {name}: kbase > 0 on most units"
        if h["window_bits"] == 1:
            assert p.rows.nwin == (w.d - 1) // 2 + 1 and p.cols.nwin == (w.n - 1) // 2 + 1 and p.cols.nwin > 1000
            live = np.bincount(p.cols.ublock * p.cols.nwin + p.cols.uwin, minlength=p.cols.nblock * p.cols.nwin)[p.cols.nwin:]
            assert np.mean(live == 0) > 0.9, "point 5: most windows of column block 1 are empty"
    assert bits == {1, 6}


def test_point_6_frequent_columns():
    h = H.HOT_H
    drops = 0
    for key, (d, ncand) in H.HOT_SHAPES.items():
        sh = H.shard(key)
        p = dict((H.hook_id(hk), q) for hk, q in plans(key))
        on, off = p[f"hot_min={h}"], p["hot_min=0"]
        assert sh.d == d and off.hot.size == 0 and off.vbase == 0, f"point 6, {key}: GDMIX_FE_HOT_MIN=0 on the same shard"
        cand = np.flatnonzero(sh.col_count >= h)
        assert cand.size == ncand and on.hot.size == min(ncand, H.FE_HOT_MAX), f"point 6, {key}: {ncand} candidates"
        assert {h - 1, h, h + 1} <= set(sh.col_count.tolist()), f"point 6, {key}: columns of h - 1, h and h + 1 entries"
        assert not set(np.flatnonzero(sh.col_count == h - 1)) & set(on.hot)
        if ncand > H.FE_HOT_MAX:
            dropped = np.setdiff1d(cand, on.hot)
            least = cand[sh.col_count[cand] == sh.col_count[cand].min()]
            assert least.size >= 2 and list(dropped) == [least.max()], f"point 6, {key}: the least frequent is dropped, on a tie the highest column"
            drops += 1
        assert on.vbase == -(-d // B) * B
        # twice in one row; a first entry at every residue of the position mod 32
        pos = np.arange(sh.z)
        firsts = {int(pos[sh.lcol == c][0]) % H.FE_HOT_REP for c in on.hot}
        assert firsts == set(range(H.FE_HOT_REP)), f"point 6, {key}: frequent columns start at residues {sorted(firsts)} only (row 0 of the shard)"
        rc = sh.row[sh.lcol == on.hot[1]]
        assert np.unique(rc).size < rc.size, f"point 6, {key}: a frequent column twice in one row"
    assert drops == 1 and {n for _, n in H.HOT_SHAPES.values()} == {63, 64, 65}, "point 6: 63, 64 and 65 candidates"
    p48 = dict((H.hook_id(hk), q) for hk, q in plans("hot2048"))[f"hot_min={h}"]
    p49 = dict((H.hook_id(hk), q) for hk, q in plans("hot2049"))[f"hot_min={h}"]
    assert p48.vbase == B and p49.vbase == 2 * B, "point 6: vbase 2 048 at d = 2 048, 4 096 at d = 2 049"
    assert B not in set(p49.hot) and p49.cols.ulen[p49.cols.ufirst[1]] == H.shard("hot2049").col_count[B], "point 6: block 1 of hot2049 holds one ordinary column"
    one = dict((H.hook_id(hk), q) for hk, q in plans("hot1"))[f"hot_min={h}"]
    assert H.shard("hot1").d == 1 and list(one.hot) == [0] and one.vbase == B, "point 6: d = 1 with its only column frequent"


def test_point_7_the_six_byte_form():
    sh = H.shard("compress")
    (h, p) = plans("compress")[0]
    assert h == {"window_bits": H.COMPRESS_WINDOW_BITS, "compress": 3}
    for name, c in both(p):
        rows_pass = name == "row pass"
        unit = {}
        for t, ((rb, cb), gaps) in H.COMPRESS_TILES.items():
            blk, win = (rb, cb) if rows_pass else (cb, rb)
            u, = np.flatnonzero((c.ublock == blk) & (c.uwin == win))
            unit[t] = int(u)
            g = c.gap[c.ustart[u] + 1:c.ustart[u + 1]]
            assert dict(zip(*map(list, np.unique(g, return_counts=True)))) == gaps, f"point 7, {name}: tile {t} does not show its gaps"
        A, Bu, C, D, E = (unit[t] for t in "ABCDE")
        assert (c.ulen[A], c.fillers[A], bool(c.taken[A])) == (427, 0, True), f"point 7, {name}: 427 entries without fillers are taken"
        assert (c.ulen[Bu], c.fillers[Bu], bool(c.taken[Bu])) == (426, 0, False), f"point 7, {name}: 426 entries without fillers are not"
        assert (c.cnt[C], c.trips[C], bool(c.taken[C])) == (H.FE_CTRIP, 1, True), f"point 7, {name}: a count of exactly 512 is one trip"
        assert (c.cnt[D], c.trips[D], bool(c.taken[D])) == (H.FE_CTRIP + 1, 2, False), f"point 7, {name}: a count of 513 is two trips, and stays plain"
        assert c.trips[E] == 2 and c.taken[E] and c.cnt[E] % H.FE_CTRIP, f"point 7, {name}: a taken unit of two trips with padding"
        gaps_taken = set(c.gap[c.ustart[C] + 1:c.ustart[C + 1]].tolist()) | set(c.gap[c.ustart[A] + 1:c.ustart[A + 1]].tolist())
        assert {0, 1, 31, 32, 62, 63, 1000} <= gaps_taken, f"point 7, {name}: key gaps inside taken units"
        assert [int(H.fillers(g)) for g in (0, 1, 31, 32, 62, 63, 1000)] == [0, 0, 0, 1, 1, 2, 32]
        assert c.taken.any() and (~c.taken & (c.ulen > 0)).any(), f"point 7, {name}: taken and plain units in one launch"
    assert {hk["compress"] for hk, _ in plans("compress")} == {0, 1, 2, 3}
    assert all(H._HOOK_TABLE[k][1] for k in ("trips", "empties", "windows")), "the shards of points 3 and 5 also run under GDMIX_FE_COMPRESS 0 .. 3"


def test_point_8_the_reduction_of_partial_sums():
    nred = {}
    for key in H.BUILDERS:
        for h, p in plans(key):
            nred[(key, H.hook_id(h))] = p.nred
    vals = set(nred.values())
    assert 1 in vals and nred[("square1", "plain")] == 1, "point 8: nred = 1 (the n = 1 shard)"
    m = 3 * H.FE_FIN_BLOCKS
    assert {m - 1, m, m + 1} <= vals, "point 8: nred just below, at and above a multiple of 64 (strands63 / 64 / 65: one cut block)"
    big = nred[("many_units", "chunk=64")]
    assert big > H.FE_FIN_BLOCKS * H.FE_THREADS, "point 8: nred above 64 * 256 (many_units)"
    assert -(-big // H.FE_FIN_BLOCKS) > H.FE_THREADS
    (h, p), = plans("many_units")
    assert 16000 < p.rows.nunit < 18000 and 16000 < p.cols.nunit < 18000


def test_point_9_exact_zeros():
    sh = H.shard("exact")
    assert sh.cancel_cols == [H.EXACT_D, H.EXACT_D + 1]
    for loss, weighted, ic in (H.DEFAULT_CASE, ("squared", False, 0), ("poisson", True, 1)):
        ref = H.evaluate(sh, loss, weighted, ic)
        for c in sh.cancel_cols:
            e = np.flatnonzero(sh.lcol == c)
            assert e.size == 2 and sh.row[e[0]] == sh.row[e[1]] and sh.val[e[0]] == -sh.val[e[1]] != 0, "point 9: v and -v in one row"
            assert ref["grad"][sh.uniq[c]] == 0 and ref["E_grad"][sh.uniq[c]] > 0 and ref["diag"][sh.uniq[c]] > 0
    for key in H.BUILDERS:
        s = H.shard(key)
        assert s.absent.size == 3 and not set(s.absent) & set(s.uniq) and s.absent.max() == s.D - 1, f"point 9, {key}: absent features first, middle, last"
    assert np.all(np.abs(sh.theta0[sh.absent]) >= 0.05), "theta0 is non-zero on absent coefficients too"


def test_the_ranges_of_the_shards():
    for key in H.BUILDERS:
        s = H.shard(key)
        a = np.abs(s.val)
        assert a.min() >= np.float32(0.1) - 1e-7 and a.max() <= 1.0
        for th in (s.theta0, s.theta1, s.vec):
            assert th.shape == (s.D + 1,) and np.abs(th).min() >= 0.05 and np.abs(th).max() <= 0.5
        assert s.wt.min() >= 0.25 and s.wt.max() <= 2.25
        if key != "many_units":
            assert s.z <= 40000, f"{key}: a small shard has at most a few ten thousand non-zeros"
