"""What tests/test_gpu_full_variance_edges.py relies on, checked without a GPU: that the batches and matrices of full_variance_helpers
show, BY NAME, every size, structure and option the FULL variance kernels have an edge at; that the longdouble reference and the two
float64 routes agree under the tolerance law, with r_ref measured here and the helper's literal held to it; that the law is never looser
than the older tests' rtol 1e-8 on an entity that is not ill-conditioned on purpose; and that the helper's constants are the library's.

A CHANGED CONSTANT of the FULL variance kernels is changed in full_variance_helpers first: these tests then name the shapes to move."""
import os
import re

import numpy as np
import pytest

import full_variance_helpers as fv


def _sources():
    import gdmix_amd
    return os.path.join(os.path.dirname(os.path.abspath(gdmix_amd.__file__)), "csrc")


def test_the_constants_are_the_librarys():
    src = _sources()
    names = set(fv.CONSTANTS) | {f for f, _ in fv.SOURCE_LINES}
    if not all(os.path.exists(os.path.join(src, f)) for f in names):
        pytest.skip("the sources are not shipped next to the package: the constants cannot be read")
    text = {}
    for f in names:
        with open(os.path.join(src, f)) as fh:
            text[f] = fh.read()
    for fname, constants in fv.CONSTANTS.items():
        for name, value in constants.items():
            found = re.findall(rf"\bconstexpr\s+\w+\s+{name}\s*=\s*(\d+)\s*;", text[fname])
            assert found == [str(value)], (fname, name, found, value)
    for fname, line in fv.SOURCE_LINES:
        assert " ".join(text[fname].split()).count(line) == 1, (fname, line)
    assert fv.slot_doubles(64) == 2 * 64 * 64 + 64 + 8 and fv.VAR_SLOTS_MAX == 2048 and fv.WAVE == 64
    assert fv.tiles_ld(1) == 64 and fv.tiles_ld(64) == 64 and fv.tiles_ld(65) == 128 and fv.VF_T == 64


# ---- the shapes ------------------------------------------------------------------------------------------------------------------------------
def test_factor_cases_show_one_two_and_three_tiles_and_both_conditionings():
    T = fv.VF_T
    assert set(fv.FACTOR_P) == {1, 2, T - 1, T, T + 1, 2 * T - 1, 2 * T, 2 * T + 1, 3 * T, 3 * T + 1}
    shapes = fv.factor_shapes()
    assert {ld // T for _, ld in shapes} == {1, 2, 3, 4}
    assert {(p, ld) for p, ld in shapes if ld != fv.tiles_ld(p)} == {(1, 2 * T), (T, 2 * T), (T + 1, 3 * T)}
    for p in fv.FACTOR_P:
        cases = fv.factor_cases(p)
        assert {c for c, _, _ in cases} == {"sparse", "spectrum"} and {l2 for _, l2, _ in cases} == {0.0, 0.7}
        assert {u for _, _, u in cases} == {-1, 0, p - 1}
        for cond in fv.FACTOR_CONDS:
            A = fv.factor_matrix(p, cond)
            assert A.shape == (p, p) and np.array_equal(A, A.T) and np.linalg.eigvalsh(A)[0] > 0      # SPD as uploaded
        if p > 1:
            assert fv.factor_reference(p, "spectrum", 0.0, -1)["kappa"] == pytest.approx(fv.SPECTRUM_KAPPA, rel=1e-3)
            assert fv.factor_reference(p, "spectrum", 0.7, 0)["kappa"] > 1e7
        for l2 in fv.FACTOR_L2:
            assert fv.factor_reference(p, "sparse", l2, p - 1)["kappa"] < 200


def _row_lists(b, e):
    r0, r1 = int(b.ent_row_ptr[e]), int(b.ent_row_ptr[e + 1])
    return [b.col_global[b.row_nnz_ptr[i]:b.row_nnz_ptr[i + 1]] for i in range(r0, r1)]


def _most_repeats(row):
    return int(np.unique(row, return_counts=True)[1].max()) if row.size else 0


def test_build_cases_show_every_structure():
    G, TH = fv.VAR_BIG_BUILD_GROUPS, fv.VF_THREADS
    assert {d for d, _, _ in fv.BUILD_CASES.values()} == {5, G - 1, G, G + 1, 300}
    seen = set()
    for name, (d, n, st) in fv.BUILD_CASES.items():
        for ic in fv.BUILD_IC:
            b = fv.build_batch(name, ic)
            assert (b.E, b.N) == (1, n) and n >= 64 and fv.coef_ptr_of(b, ic)[-1] == d + ic
            p = d + ic
            seen.add("no column for some workgroup" if p < G else ("one column each" if p == G else "several columns for a workgroup"))
            seen.add("weights" if b.weight is not None else "no weights")
            seen.add("intercept" if ic else "no intercept")
            rows, runs = _row_lists(b, 0), fv.column_runs(b)
            if n > TH:
                seen.add("more samples than threads")
            if max(r[0] for r in runs) > TH:
                seen.add("a column of more entries than threads")
            seen |= {f"a pair {k} times" for k in (2, 3) if any(r[1] == k for r in runs)}
            if any(r[2] for r in runs):
                seen.add("a run across a multiple of the threads")
                assert "straddle" in st
            if rows[0].size == 0 and rows[-1].size == 0 and any(r.size == 0 for r in rows[1:-1]):
                seen.add("empty samples")
            cols = np.unique(b.col_global)
            if any(all((r == c).any() for r in rows) for c in cols[:1]):
                seen.add("every sample in one column")
            assert ("dense" in st) == all((r == cols[0]).any() for r in rows)
    assert seen == {"no column for some workgroup", "one column each", "several columns for a workgroup", "weights", "no weights", "intercept",
                    "no intercept", "more samples than threads", "a column of more entries than threads", "a pair 2 times", "a pair 3 times",
                    "a run across a multiple of the threads", "empty samples", "every sample in one column"}
    assert fv.BUILD_CASES["d300"][0] + 1 > 2 * G          # a workgroup re-uses its vector twice over
    for name in fv.BUILD_CASES:                            # every d with weights and without
        assert {fv.build_weighted(name, ic) for ic in fv.BUILD_IC} == {True, False}


def test_wavefront_batch_shows_every_edge():
    w = fv.wave_batch()
    b = w["b"]
    for ic in (1, 0):
        p = np.diff(fv.coef_ptr_of(b, ic))
        assert np.array_equal(p, w["d"] + ic)
        assert set(fv.WAVE_P) <= set(p.tolist()), (ic, sorted(set(fv.WAVE_P) - set(p.tolist())))
    assert set(fv.WAVE_P) == {1, 2, 63, 64, 65, 127, 128, 129, 640}
    d = w["d"]
    assert d[0] > 10 * d[1] and d[2] > 10 * d[1] and d[2] > 10 * d[3] and d[4] > 10 * d[3]       # large, small, large, small, large
    assert b.weight is not None
    lens, repeats = set(), set()
    for e in range(b.E):
        rows = _row_lists(b, e)
        assert max(r.size for r in rows) <= fv.WAVE_ROW_MAX
        assert rows[0].size == 0 and rows[-1].size == 0                   # an empty sample first and last
        lens |= {r.size for r in rows}
        repeats |= {_most_repeats(r) for r in rows}
        if d[e] == 0:
            assert len(rows) > 0 and all(r.size == 0 for r in rows)       # samples, and not one non-zero
        assert {"twice", "thrice", "empty_first", "empty_last"} <= w["tags"][e] or d[e] == 0
    assert 0 in d and {2, 3} <= repeats
    assert set(fv.WAVE_M) <= lens
    for ic in (1, 0):      # the pattern loop `t < m * m` against the 64 lanes: below, equal, above
        sq = {(m + ic) ** 2 for m in fv.WAVE_M}
        assert fv.WAVE in sq and any(s < fv.WAVE for s in sq) and any(s > fv.WAVE for s in sq)
        assert max(s for s in sq if s < fv.WAVE) == 49                    # (63 is no square: 49 is the closest from below)
    assert set(fv.WAVE_CASES) == {(1, False), (1, True), (0, True), (0, False)}


def test_slot_batches_make_the_trips_they_are_meant_to():
    b = fv.slots_batch()
    p = np.diff(fv.coef_ptr_of(b, 1))
    S = fv.VAR_SLOTS_MAX
    assert b.E == fv.SLOTS_E > 2 * S and p.max() == fv.SLOTS_MAX_P and p.min() == 1
    assert fv.slot_doubles(int(p.max())) * 8 * S < 2 << 30               # the 2 GiB budget does not cut the slots below 2 048
    first, second, third = p[:S], p[S:2 * S], p[2 * S:]
    assert (first > second).sum() > 100 and (first < second).sum() > 100      # a wider entity before a narrower one in a slot, and the reverse
    assert third.size > 50 and (second[:third.size] > third).any() and (second[:third.size] < third).any()
    assert max(r.size for e in range(0, b.E, 97) for r in _row_lists(b, e)) <= fv.WAVE_ROW_MAX
    f = fv.four_slot_batch()
    assert f.E == fv.FOUR_E == 64 and set(np.diff(fv.coef_ptr_of(f, 1)).tolist()) == {fv.FOUR_P} and fv.FOUR_P == 64
    assert (f.Z + 1) * 8 < 4 * fv.slot_doubles(fv.FOUR_P) * 8               # the batch's own scratch is the smaller one
    assert f.E // 4 == 16                                                  # sixteen trips of four wavefronts
    assert max(r.size for e in range(f.E) for r in _row_lists(f, e)) <= fv.WAVE_ROW_MAX


def test_hand_over_batches_sit_on_the_cap_and_the_tile_edges():
    cap, T = fv.VAR_FULL_MAX_P, fv.VF_T
    assert set(fv.HAND_OVER_P) == {cap + 1, cap + T, cap + T + 1} and cap % T == 0
    assert fv.HAND_OVER_P[0] > fv.HAND_OVER_P[1]                           # a larger whole-device entity before a smaller one
    for ic in (1, 0):
        b = fv.hand_over_batch(ic)
        p = np.diff(fv.coef_ptr_of(b, ic))
        assert np.array_equal(p[0::2], fv.HAND_OVER_P) and np.array_equal(p[1::2], np.array(fv.HAND_OVER_SMALL_D) + ic)
        assert (b.weight is None) == (ic == 1)
        for e in range(0, b.E, 2):
            rows = _row_lists(b, e)
            assert len(rows) == fv.HAND_OVER_N == 128
            assert {r.size for r in rows} <= {16, 17} and all(np.unique(r).size == r.size for r in rows)
    assert fv.HAND_OVER_P[1] - 1 == cap                                     # d = 2 048 with the intercept is p = 2 049: the whole device
    a = fv.at_cap_batch()
    p = np.diff(fv.coef_ptr_of(a, 0))
    assert (p[0], p[2]) == fv.AT_CAP_P == (cap, cap + 1) and p[1] < 10      # d = 2 048 without: the wavefront kernel's last size
    assert max(r.size for r in _row_lists(a, 0)) <= fv.WAVE_ROW_MAX
    assert np.diff(fv.coef_ptr_of(fv.at_cap_batch(1024), 0))[0] == 1024
    z = fv.beyond_batch()
    assert fv.coef_ptr_of(z, 1)[-1] == fv.VAR_FULL_BIG_MAX_P + 1


# ---- the law ------------------------------------------------------------------------------------------------------------------------------------
def test_the_three_routes_agree_under_the_law_and_r_ref_is_the_helpers():
    r_ref, where, rows = fv.measure_r_ref()
    by_family = {}
    for name, kappa, c, i in rows:
        fam = " ".join(name.split()[:1] + ([name.split()[2]] if name.startswith("factor") else []))
        lo, hi = by_family.get(fam, (np.inf, 0.0))
        by_family[fam] = (min(lo, c, i), max(hi, c, i))
    print(f"r_ref = {r_ref:.3f} at {where}; {len(rows)} small cases; (least, largest) ratio per family: "
          + ", ".join(f"{k}: {lo:.3f} .. {hi:.3f}" for k, (lo, hi) in by_family.items()))
    assert len(rows) > 10000 and {"factor sparse", "factor spectrum", "wave", "slots", "four"} == set(by_family)
    assert r_ref <= fv.R_REF <= 1.25 * max(r_ref, 1.0), (r_ref, fv.R_REF)
    assert fv.K == 8.0 * max(fv.R_REF, 1.0)
    for name, kappa, c, i in rows:      # (what the law asks of the device, the float64 routes meet with the factor 8 to spare)
        assert max(c, i) <= fv.K / 8.0, (name, c, i)
        if "spectrum" not in name:
            assert fv.K * kappa * fv.U <= fv.RTOL_CAP, (name, kappa)
    assert max(k for n, k, _, _ in rows if "spectrum" in n and "l2=0.0" in n) > 0.99 * fv.SPECTRUM_KAPPA


@pytest.mark.parametrize("ic", [1, 0])
def test_the_law_is_no_looser_than_1e_8_on_the_large_entities(ic):
    b = fv.hand_over_batch(ic)
    for loss in fv.LOSSES:
        r = fv.reference("hand", b, loss, fv.L2, ic, False)
        assert np.all(np.isfinite(r["var"].astype(np.float64))) and np.all(r["var"] > 0)
        assert fv.K * r["kappa"].max() * fv.U <= fv.RTOL_CAP, (loss, r["kappa"].max())


def test_the_build_bound_is_far_below_the_entries_it_guards():
    """n 2^-53 sum|terms| against the diagonal entries, which are sums of positive terms: below 1e-12 of them, so that the build comparison
    resolves a dropped or doubled sample of a column of 600."""
    for name in fv.BUILD_CASES:
        H, bound = fv.build_reference(name, 1, "logistic", fv.draw_theta(("build", name, 1), fv.BUILD_CASES[name][0] + 1))
        assert np.all(bound >= 0) and np.all(H.diagonal() > 0)
        assert np.all(bound.diagonal() < 1e-12 * H.diagonal())
