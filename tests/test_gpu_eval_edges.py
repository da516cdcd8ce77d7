"""The evaluation units on the device at their edges (csrc/re_evaluate_poisson.hip: the Poisson and the log-loss term and their sums;
csrc/re_eval_sum.hpp: the fixed-shape fp64 sum; csrc/re_evaluate.hip: SSE, the four-per-wavefront kernels, the rank pass), on the inputs
of tests/eval_edges_helpers.py. What those inputs must be for this to mean something is checked on the CPU by tests/test_eval_edges.py.

  terms        a single-sample entity's sum IS its term (the butterfly adds zeros): every point of the grid against long double, by the
               figures of include/gdmix_re.h and csrc/re_device.hpp — exp_any <= 0.98 ulp and ONE rounding for exp(s) - y s; the log loss
               |ce - exact| <= 2^-53 ce + GDMIX_RE_EVAL_LL_TERM_EPS; +inf, 0 and NaN exactly where IEEE puts them. The measured maxima are printed.
  run edges    one entity of 524 287 .. 524 545 samples (a lane's run of 2 048 terms closes) and one of 33 554 689 (64 runs close), on integer
               data whose sums are exact, with a NaN score in the last lane's last term.
  accumulator  one `add` of 4 096 | 4 097 samples, 16 | 17 workgroups, the full grid and one more trip; stale workgroup sums; the TwoSum total
               of PL / LL as the rounded exact sum of the batches' sums in all six orders; SSE added in the order given.
  geometry     every size 0 .. 66 in every position of a wavefront under the limits 64, 33, 32, 17, 16, 1, 0 through the five kernels that
               share the geometry; the packed fields at their maxima.
  rank pass    segment ends and tie groups on the 16-key and 4 096-key edges, per entity and as one accumulated set.

A CHANGED CONSTANT of the evaluation units is changed in eval_edges_helpers too: test_the_constants_are_the_librarys fails until it is."""
import functools
import itertools
import math
import os
import re
import time
from fractions import Fraction

import numpy as np
import pytest

import eval_edges_helpers as eh
import metrics_reference as mref
import ranking_reference as rref
from gdmix_amd import metrics
from gdmix_amd import solver as solver_module

pytestmark = pytest.mark.gpu

LD = eh.LD
EPS = solver_module.EVAL_LL_TERM_EPS


def _np(x):
    return x.cpu().numpy()


def _bits(x):
    return np.ascontiguousarray(x, np.float64).view(np.uint64)


def _ll_bound(sum_terms, n):
    return eh.LL_BOUND * sum_terms + n * EPS


@pytest.fixture()
def small_max(device_solver):
    """set(limit) moves the context's small limit (one knob for every evaluator); the default comes back after the test."""
    ev = metrics.PoissonEvaluator(device_solver)
    yield ev.set_small_max
    ev.set_small_max(eh.SMALL_MAX)


def test_the_constants_are_the_librarys(device_solver):
    src = os.path.join(os.path.dirname(solver_module.LIB_PATH), "csrc")
    if not os.path.exists(os.path.join(src, "re_eval_sum.hpp")):
        pytest.skip("the sources are not shipped next to the library: the constants cannot be read")
    text = {}
    for f in ("re_eval_sum.hpp", "re_evaluate.hip", "re_evaluate_poisson.hip"):
        with open(os.path.join(src, f)) as fh:
            text[f] = fh.read()

    def const(f, name):
        found = re.findall(rf"constexpr\s+int\s+(?:\w+\s*=\s*[^,;]+,\s*)*{name}\s*=\s*([^,;]+)[,;]", text[f])
        assert len(found) == 1, (name, found)
        return found[0].strip()
    for name in ("EVAL_THREADS", "EVAL_RUN", "EVAL_RUNS", "ACC_MAX_GROUPS", "ACC_PER_THREAD"):
        assert int(const("re_eval_sum.hpp", name)) == getattr(eh, name), name
    for name in ("RANK_THREADS", "RANK_ITEMS"):
        assert int(const("re_evaluate.hip", name)) == getattr(eh, name), name
    assert const("re_evaluate.hip", "RANK_TILE") == "RANK_THREADS * RANK_ITEMS"
    assert "(N + (int64_t)EVAL_THREADS * 16 - 1) / ((int64_t)EVAL_THREADS * 16)" in text["re_eval_sum.hpp"] and eh.ACC_SAMPLES_PER_LANE == 16
    width = "const int W = nmax <= 16 ? 16 : (nmax <= 32 ? 32 : 64);"
    assert text["re_evaluate.hip"].count(width) == 2 and text["re_evaluate_poisson.hip"].count(width) == 1 and eh.SMALL_WIDTHS == (16, 32, 64)
    assert text["re_evaluate_poisson.hip"].count("const int small_max = ci->eval_small_set ? ci->eval_small_max : 64;") == 1 and eh.SMALL_MAX == 64
    assert "y > 0.5f ? -z : z" in text["re_evaluate_poisson.hip"]
    with open(os.path.join(os.path.dirname(src), os.pardir, "include", "gdmix_re.h")) as fh:
        assert f"#define GDMIX_RE_EVAL_LL_TERM_EPS {EPS!r}" in fh.read()


# ---- terms ----------------------------------------------------------------------------------------------------------------------------
def _device_terms(ev, s, y):
    """Every (score, label) as an entity of one sample -> (its sum, n, n_nan) on the host."""
    rp = np.arange(s.size + 1, dtype=np.int64)
    res = ev.entities(rp, np.array(s), np.array(y))      # (copies: the grid itself is read-only)
    return _np(res["pl"]), _np(res["n"]), _np(res["n_nan"])


@pytest.mark.parametrize("which", [str(w) for w in eh.PL_LABELS])
def test_poisson_term_on_every_grid_point(device_solver, which):
    """exp(s) - y s of the device against expl(s) - y s. s = +-inf is a score like any other (include/gdmix_re.h, "poisson evaluation",
    `infinities`): +inf for y < 0 at +inf and y > 0 at -inf, NaN where the statement is inf - inf or 0 * inf (y = 0 at either)."""
    s = eh.term_scores()
    y = eh.pl_labels(s, "cancel" if which == "cancel" else float(which))
    got, n, n_nan = _device_terms(metrics.PoissonEvaluator(device_solver), s, y)
    assert np.all(n == 1) and not n_nan.any()
    ref, ulp_e, ulp_ref, e = eh.pl_reference(s, y, eh.term_exp())
    bound, ref64 = eh.pl_term_bound(got, ref, ulp_e, ulp_ref, e)
    exact = np.isnan(bound)
    with np.errstate(invalid="ignore"):
        err = np.abs(got.astype(LD) - ref)
    # the measured maxima, printed before anything is asserted
    normal = ~exact & (eh.exp64(s) >= eh.MIN_NORMAL)
    sub = ~exact & ~normal
    # (in ulps of the TERM; with y = 0 the term is exp(s) and this is exp_any's own error)
    in_ulps = np.where(normal, err / ulp_ref, 0)
    share = np.where(normal, err / bound, 0)
    i, j = int(np.argmax(in_ulps)), int(np.argmax(share))
    print(f"PL term, y = {which}: {int(normal.sum())} normal points, worst {float(in_ulps[i]):.4f} ulp of the term = {float(err[i]):.3e} at s = {float(s[i])!r}"
          f" (y = {float(y[i])!r}); worst error / bound {float(share[j]):.4f} at s = {float(s[j])!r} (y = {float(y[j])!r}); "
          f"{int(sub.sum())} points with a subnormal exp: worst {float(err[sub].max() / eh.TINY) if sub.any() else 0.0:.2f} spacings; {int(exact.sum())} exact points")
    with np.errstate(over="ignore"):
        same = (got == ref64) | (np.isnan(got) & np.isnan(ref64))
    assert np.all(same[exact]), [(float(s[k]), float(y[k]), float(got[k]), float(ref64[k])) for k in np.flatnonzero(exact & ~same)[:5]]
    bad = ~exact & ~(err <= bound)
    assert not bad.any(), [(float(s[k]), float(y[k]), float(got[k]), float(err[k] / bound[k])) for k in np.flatnonzero(bad)[:5]]
    if which == "0.0":      # the named ends, by name
        at = {name: int(np.flatnonzero(s.view(np.uint32) == np.float32(v).view(np.uint32))[0]) for name, v in eh.named_scores().items()}
        assert np.isfinite(got[at["exp_last_finite"]]) and got[at["exp_last_finite"]] > 2.0 ** 1023 and np.isposinf(got[at["exp_first_inf"]])
        assert got[at["exp_last_nonzero"]] == eh.TINY and got[at["exp_first_zero"]] == 0.0
        assert np.isnan(got[at["+inf"]]) and np.isnan(got[at["-inf"]]), "y = 0 at an infinite score: 0 * inf, NaN by the statement"
        assert got[at["zero"]] == 1.0 and got[at["minus_zero"]] == 1.0
        assert np.isposinf(got[at["+800"]]) and got[at["-800"]] == 0.0 and np.isposinf(got[at["+3.4e+38"]]) and got[at["-1100"]] == 0.0


@pytest.mark.parametrize("label", eh.LL_LABELS)
def test_log_loss_term_on_every_grid_point(device_solver, label):
    """ce of the device against the header's formula in long double: |ce - exact| <= 2^-53 ce + GDMIX_RE_EVAL_LL_TERM_EPS on every finite
    score, exactly 0 or +inf at the infinite ones; 0.5 is a negative label and the next float a positive one."""
    s = eh.term_scores()
    y = np.full(s.shape, label, np.float32)
    got, n, n_nan = _device_terms(metrics.LogLossEvaluator(device_solver), s, y)
    assert np.all(n == 1) and not n_nan.any()
    ref, _ = eh.ll_reference(s, y)
    fin = np.isfinite(ref)
    assert np.all(fin | np.isinf(s)), "only an infinite score has an infinite term"
    err = np.abs(got[fin].astype(LD) - ref[fin])
    over = err - ref[fin] * LD(2.0 ** -53)
    i, k = int(np.argmax(over)), int(np.argmax(err))
    print(f"LL term, y = {label!r}: worst |ce - exact| - 2^-53 ce = {float(over[i]):.4e} at s = {float(s[fin][i])!r} (header: {EPS!r}); "
          f"worst |ce - exact| = {float(err[k]):.4e} at s = {float(s[fin][k])!r}")
    inf = np.isinf(s)
    assert np.all(got[inf] == ref[inf].astype(np.float64)) and set(got[inf].tolist()) == {0.0, math.inf}
    assert np.all(got[~fin] == math.inf) and np.all(np.isfinite(got[fin]))
    bad = ~(over <= LD(EPS))
    assert not bad.any(), [(float(s[fin][q]), float(got[fin][q]), float(over[q])) for q in np.flatnonzero(bad)[:5]]
    # the side of the label: a positive pays for a negative score
    positive = np.float32(label) > np.float32(0.5)
    assert positive == (label not in (0.0, 0.5, -1.0))
    far = np.isfinite(s) & (np.abs(s) > 40)
    wrong_side = (s < 0) if positive else (s > 0)
    assert np.all(got[far & wrong_side] == np.abs(s[far & wrong_side]).astype(np.float64)) and np.all(got[far & ~wrong_side] < 1e-17)


def test_terms_are_one_function_on_both_paths(device_solver, small_max):
    """A 2^16-point subset of the grid (61 440 points evenly spaced over the exponents, and the 4 096 at its end: the windows and the extremes)
    with a workgroup per entity (limit 0): the same bits."""
    s = eh.term_scores()
    pick = np.concatenate([np.linspace(0, s.size - 4097, 61_440).astype(np.int64), np.arange(s.size - 4096, s.size)])
    assert pick.size == np.unique(pick).size == 1 << 16
    s = s[pick]
    for ev, y in ((metrics.PoissonEvaluator(device_solver), eh.cancel_labels(s)), (metrics.PoissonEvaluator(device_solver), np.full(s.shape, 3.0, np.float32)),
                  (metrics.LogLossEvaluator(device_solver), (np.arange(s.size) % 2).astype(np.float32))):
        small_max(eh.SMALL_MAX)
        a = _device_terms(ev, s, y)
        small_max(0)
        b = _device_terms(ev, s, y)
        assert np.array_equal(_bits(a[0]), _bits(b[0])) and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2])


# ---- run edges --------------------------------------------------------------------------------------------------------------------------
def _one_entity(device_solver, n, recipe):
    """A recipe's samples on the device with a NaN score in the last lane's last term -> (ent_row_ptr, score, label, the recipe's integer
    tensors, the index of the NaN)."""
    t, dev = device_solver.torch, device_solver.device
    i = t.arange(n, dtype=t.int64, device=dev)
    parts = recipe(i)
    s, y = parts[0].to(t.float32), parts[1].to(t.float32)
    at = eh.last_lane_last_term(n)
    s[at] = float("nan")
    return t.tensor([0, n], dtype=t.int64, device=dev), s, y, parts, at


def _timed(device_solver, f):
    t = device_solver.torch
    t.cuda.synchronize()
    t0 = time.perf_counter()
    r = f()
    t.cuda.synchronize()
    return r, time.perf_counter() - t0


def _sse_entity(device_solver, n, with_auc):
    rp, s, y, (_, _, d), at = _one_entity(device_solver, n, eh.sse_recipe)
    want = int((d * d).sum()) - int(d[at]) ** 2
    assert want < 1 << 53
    res, sec = _timed(device_solver, lambda: metrics.DeviceEvaluator(device_solver).entities(rp, s, y))
    got = {k: _np(v)[0] for k, v in res.items()}
    assert got["n_nan"] == 1 and got["n_pos"] + got["n_neg"] == n - 1
    assert got["sse"] == float(want), (n, got["sse"], want)
    if with_auc:
        two_u, n_pos, n_neg, n_nan = mref.two_u_reference(_np(s), _np(y))
        assert (int(got["two_u"]), int(got["n_pos"]), int(got["n_neg"]), int(got["n_nan"])) == (two_u, n_pos, n_neg, n_nan) and n_neg > 100
    else:
        assert int(got["n_pos"]) == int((y[s == s] > 0.5).sum())
    return sec


def _unit_entity(device_solver, n):
    """s = 0: every Poisson term is exactly 1.0, every log-loss term the device's log 2 -> the two times."""
    rp, s, y, _, at = _one_entity(device_solver, n, eh.unit_recipe)
    res, sec_pl = _timed(device_solver, lambda: metrics.PoissonEvaluator(device_solver).entities(rp, s, y))
    assert (float(_np(res["pl"])[0]), int(_np(res["n"])[0]), int(_np(res["n_nan"])[0])) == (float(n - 1), n - 1, 1)
    res, sec_ll = _timed(device_solver, lambda: metrics.LogLossEvaluator(device_solver).entities(rp, s, y))
    want = float(Fraction(n - 1) * Fraction(float(np.log(LD(2.0)))))
    assert abs(float(_np(res["pl"])[0]) - want) <= _ll_bound(want, n - 1) and int(_np(res["n"])[0]) == n - 1 and int(_np(res["n_nan"])[0]) == 1
    return sec_pl, sec_ll


def _mixed_counts(device_solver, code, skip=None):
    t = device_solver.torch
    counts = _np(t.bincount(code, minlength=16)).astype(np.int64)
    if skip is not None:
        counts[int(code[skip])] -= 1
    return counts


@pytest.mark.parametrize("n", eh.RUN_EDGE_SIZES)
def test_a_lanes_run_closes(device_solver, n):
    """One entity whose lanes close a run of 2 048 terms — none yet, exactly, one term behind it, a row and one behind it: SSE an exact
    integer, the AUC integers the reference's, PL = n - 1 exactly on unit terms, PL and LL within the header's bounds of the exact sum on
    terms of mixed size (one lost term of size ~1 is seven orders above the bound)."""
    sec = [_sse_entity(device_solver, n, with_auc=True), *_unit_entity(device_solver, n)]
    rp, s, y, (_, _, code), at = _one_entity(device_solver, n, eh.mixed_recipe)
    counts = _mixed_counts(device_solver, code, skip=at)
    assert counts.sum() == n - 1 and counts.min() > 30_000
    for ev, which in ((metrics.PoissonEvaluator(device_solver), "pl"), (metrics.LogLossEvaluator(device_solver), "ll")):
        want, mag = eh.mixed_sums(counts, which)
        res = ev.entities(rp, s, y)
        got = float(_np(res["pl"])[0])
        bound = eh.PL_BOUND * mag if which == "pl" else _ll_bound(mag, n - 1)
        print(f"{which} of {n} mixed terms: error / bound {abs(got - want) / bound:.3e}")
        assert abs(got - want) <= bound and int(_np(res["n"])[0]) == n - 1 and int(_np(res["n_nan"])[0]) == 1
    print(f"n = {n}: SSE with the sort {sec[0] * 1e3:.1f} ms, PL {sec[1] * 1e3:.1f} ms, LL {sec[2] * 1e3:.1f} ms")


def test_a_lanes_second_level_closes(device_solver):
    """One entity of 33 554 432 + 256 + 1 samples, the smallest that closes 64 runs on every lane and adds behind them: the cheap references
    only (an exact integer, n - 1, (n - 1) log 2). One test for the three metrics; the times are printed."""
    n = eh.TOP_EDGE_SIZE
    sec_sse = _sse_entity(device_solver, n, with_auc=False)
    sec_pl, sec_ll = _unit_entity(device_solver, n)
    print(f"n = {n}: SSE with the sort {sec_sse:.3f} s, PL {sec_pl:.3f} s, LL {sec_ll:.3f} s")


# ---- accumulator ----------------------------------------------------------------------------------------------------------------------
def _recipe_batch(device_solver, N, recipe, first=0):
    t, dev = device_solver.torch, device_solver.device
    parts = recipe(t.arange(first, first + N, dtype=t.int64, device=dev))
    return parts[0].to(t.float32), parts[1].to(t.float32), parts


def _add_recipes(device_solver, sizes):
    """The three metrics over batches of the given sizes (consecutive sample indices), each batch one `add` -> the checks of the totals."""
    N = sum(sizes)
    ev = metrics.DeviceEvaluator(device_solver)
    want, n_pos, first = 0, 0, 0
    host = []
    for n in sizes:
        s, y, (_, _, d) = _recipe_batch(device_solver, n, eh.sse_recipe, first)
        ev.add(s, y)
        want += int((d * d).sum())
        n_pos += int((y > 0.5).sum())
        if N <= 1 << 17:
            host.append((_np(s), _np(y)))
        first += n
    r, sec = _timed(device_solver, ev.finish)
    assert want < 1 << 53 and r["sse"] == float(want), (sizes, r["sse"], want)
    assert (r["n"], r["n_pos"], r["n_neg"], r["n_nan"]) == (N, n_pos, N - n_pos, 0)
    if host:
        assert r["two_u"] == mref.two_u_reference(np.concatenate([h[0] for h in host]), np.concatenate([h[1] for h in host]))[0]
    for cls, which in ((metrics.PoissonEvaluator, "pl"), (metrics.LogLossEvaluator, "ll")):
        unit, mixed = cls(device_solver), cls(device_solver)
        counts, first = np.zeros(16, np.int64), 0
        for n in sizes:
            s, y, _ = _recipe_batch(device_solver, n, eh.unit_recipe, first)
            unit.add(s, y)
            s, y, (_, _, code) = _recipe_batch(device_solver, n, eh.mixed_recipe, first)
            mixed.add(s, y)
            counts += _mixed_counts(device_solver, code)
            first += n
        r = unit.finish()
        assert (r["n"], r["n_nan"]) == (N, 0)
        if which == "pl":
            assert r["pl"] == float(N), (sizes, r["pl"])
        else:
            want = float(Fraction(N) * Fraction(float(np.log(LD(2.0)))))
            assert abs(r["ll"] - want) <= _ll_bound(want, N)
        want, mag = eh.mixed_sums(counts, which)
        r = mixed.finish()
        bound = eh.PL_BOUND * mag if which == "pl" else _ll_bound(mag, N)
        assert abs(r[which] - want) <= bound and (r["n"], r["n_nan"]) == (N, 0), (sizes, which, r[which], want)
    return sec


@pytest.mark.parametrize("N", eh.ACC_EDGE_SIZES)
def test_one_add_at_the_accumulators_edges(device_solver, N):
    """A single `add` of one workgroup | two, 16 | 17 workgroups (the last tree's lane 0 full | lane 1 begun), the full grid and one more
    trip (lanes of 17 and of 16 terms): SSE an exact integer, PL = N exactly on unit terms, PL and LL within their bounds on mixed terms."""
    sec = _add_recipes(device_solver, [N])
    print(f"N = {N}: finish of the AUC / SSE accumulator (the sort) {sec * 1e3:.1f} ms")


def test_a_small_batch_after_a_large_one_reads_no_stale_sum(device_solver):
    """17 workgroups, then 1 into the same accumulator: sixteen workgroup sums of the first batch are still in the state."""
    _add_recipes(device_solver, [16 * eh.ACC_GROUP_SAMPLES + 1, 100])
    _add_recipes(device_solver, [eh.ACC_GROUP_SAMPLES + 1, eh.ACC_GROUP_SAMPLES])


def _single_sums(ev, batches, key):
    out = []
    for s, y in batches:
        ev.reset()
        ev.add(s, y)
        out.append(ev.finish()[key])
    ev.reset()
    return out


def _rounded_exact_sum_in_all_orders(ev, batches, key):
    sums = _single_sums(ev, batches, key)
    want = float(sum((Fraction(x) for x in sums), Fraction(0)))
    naive = set()
    for order in itertools.permutations(range(3)):
        ev.reset()
        for k in order:
            ev.add(*batches[k])
        got = ev.finish()[key]
        assert _bits(got) == _bits(want), (key, order, got, want)
        naive.add((sums[order[0]] + sums[order[1]]) + sums[order[2]])
    assert len(naive) > 1 and any(x != want for x in naive), "the three sums are such that a plain fp64 addition depends on the order"
    return sums, want


def test_pl_total_is_the_rounded_exact_sum_of_the_batches_sums(device_solver):
    """Three batches whose sums are about +1.1e12, -1.1e12 + 3 and 0.1 (labels of 2^20 times scores of -1 and +1): each batch's own sum from a
    fresh accumulator, their exact rational sum rounded once, and all six orders must give that double, bit for bit."""
    t, dev = device_solver.torch, device_solver.device
    n = 1 << 20
    i = t.arange(n, dtype=t.int64, device=dev)
    k = int(n * (math.e + 1.0 / math.e - 3.0)) - 3
    ya = (i % 3 + n).to(t.float32)
    yb = (i % 3 + n + 3 + (i < k).to(t.int64)).to(t.float32)
    one = t.ones(n, dtype=t.float32, device=dev)
    batches = [(-one, ya), (one, yb), (t.tensor([math.log(0.1)], dtype=t.float32, device=dev), t.zeros(1, dtype=t.float32, device=dev))]
    sums, want = _rounded_exact_sum_in_all_orders(metrics.PoissonEvaluator(device_solver), batches, "pl")
    print(f"PL batches {sums!r} -> {want!r}")
    assert 1.0e12 < sums[0] < 1.2e12 and -1.2e12 < sums[1] < -1.0e12 and 0.0 < sums[0] + sums[1] < 10.0 and 0.09 < sums[2] < 0.11


def test_ll_total_is_the_rounded_exact_sum_of_the_batches_sums(device_solver):
    """The log loss has no negative term, so its three sums are about 1.1e12 (scores of 2^20 on the wrong side), 3 and 0.1: the same six orders,
    the same rounded exact sum."""
    t, dev = device_solver.torch, device_solver.device
    n = 1 << 20
    i = t.arange(n, dtype=t.int64, device=dev)
    zero = t.zeros(n, dtype=t.float32, device=dev)
    batches = [((i % 3 + n).to(t.float32), zero), (t.tensor([1.0, -1.5, 0.25], dtype=t.float32, device=dev), t.tensor([0.0, 1.0, 0.0], dtype=t.float32, device=dev)),
               (t.tensor([-2.25], dtype=t.float32, device=dev), t.zeros(1, dtype=t.float32, device=dev))]
    sums, want = _rounded_exact_sum_in_all_orders(metrics.LogLossEvaluator(device_solver), batches, "ll")
    print(f"LL batches {sums!r} -> {want!r}")
    assert 1.0e12 < sums[0] < 1.2e12 and 3.0 < sums[1] < 4.0 and 0.09 < sums[2] < 0.11


def test_sse_batches_add_up_in_the_order_given(device_solver):
    """The SSE total after three batches is the left-to-right fp64 sum of the three single-batch sums, bit for bit, in two orders."""
    rng = np.random.default_rng(17)
    t = device_solver.torch
    batches = []
    for n in (5000, eh.ACC_GROUP_SAMPLES + 1, 70_000):
        s = rng.standard_normal(n).astype(np.float32)
        y = (rng.random(n) < 0.5).astype(np.float32)
        batches.append((t.from_numpy(s).to(device_solver.device), t.from_numpy(y).to(device_solver.device)))
    ev = metrics.DeviceEvaluator(device_solver)
    sums = _single_sums(ev, batches, "sse")
    totals = []
    for order in ((0, 1, 2), (2, 0, 1)):
        ev.reset()
        for k in order:
            ev.add(*batches[k])
        got = ev.finish()["sse"]
        want = (sums[order[0]] + sums[order[1]]) + sums[order[2]]
        assert _bits(got) == _bits(want), (order, got, want)
        totals.append(got)
    print(f"SSE batches {sums!r}: totals {totals!r}")


# ---- the four-per-wavefront geometry ----------------------------------------------------------------------------------------------------
def _term_sums(rp, s, y):
    """Per entity: fsum of the long-double terms rounded once each, and of their magnitudes, NaN scores left out -> {pl, pl_mag, ll, n, n_nan}."""
    E = rp.size - 1
    out = {k: np.zeros(E) for k in ("pl", "pl_mag", "ll")}
    out["n"], out["n_nan"] = np.zeros(E, np.int64), np.zeros(E, np.int64)
    ok = ~np.isnan(s)
    pl = eh.pl_reference(s, y)[0].astype(np.float64)
    mag = (eh.exp_ld(s) + np.abs(y.astype(LD) * s.astype(LD))).astype(np.float64)
    ll = eh.ll_reference(s, y)[0].astype(np.float64)
    for e in range(E):
        sl = slice(int(rp[e]), int(rp[e + 1]))
        m = ok[sl]
        out["pl"][e], out["pl_mag"][e], out["ll"][e] = math.fsum(pl[sl][m].tolist()), math.fsum(mag[sl][m].tolist()), math.fsum(ll[sl][m].tolist())
        out["n"][e], out["n_nan"][e] = int(m.sum()), int((~m).sum())
    return out


@functools.lru_cache(maxsize=None)
def _geometry_reference(name):
    """The references of a small-geometry batch, computed once: quad_sweep's cover its three prefixes."""
    rp, s, y = (eh.quad_sweep() if name == "quad_sweep" else eh.packed_maxima())[:3]
    return dict(ints=mref.per_entity_reference(rp, s, y), topk=rref.per_entity_counts(rp, s, y, eh.KS), terms=_term_sums(rp, s, y))


def _small_geometry(device_solver, small_max, name, rp, s, y):
    E = rp.size - 1
    sizes = np.diff(rp)
    ref = _geometry_reference(name)
    ints, topk, terms = ref["ints"], ref["topk"], ref["terms"]
    plain, ranker = metrics.DeviceEvaluator(device_solver), metrics.RankingEvaluator(device_solver, eh.KS)
    pl_ev, ll_ev = metrics.PoissonEvaluator(device_solver), metrics.LogLossEvaluator(device_solver)
    t = device_solver.torch
    rp_d, s_d, y_d = (t.from_numpy(np.array(a)).to(device_solver.device) for a in (rp, s, y))
    sums = {}
    for limit in eh.LIMITS:
        small_max(limit)
        a = {k: _np(v) for k, v in plain.entities(rp_d, s_d, y_d).items()}                      # eval_small_kernel
        b = {k: _np(v) for k, v in ranker.entities(rp_d, s_d, y_d).items()}                     # topk_small_kernel<true>
        c = {k: _np(v) for k, v in ranker.entities(rp_d, s_d, y_d, with_auc=False).items()}     # topk_small_kernel<false>
        p = {k: _np(v) for k, v in pl_ev.entities(rp_d, s_d, y_d).items()}                      # eval_pl_small_kernel<PlTerm>
        q = {k: _np(v) for k, v in ll_ev.entities(rp_d, s_d, y_d).items()}                      # eval_pl_small_kernel<LlTerm>
        for got in (a, b):
            for k in ("two_u", "n_pos", "n_neg", "n_nan"):
                want = ints[k][:E].astype(np.int64)
                assert np.array_equal(got[k].astype(np.int64), want), (name, limit, k, np.flatnonzero(got[k].astype(np.int64) != want)[:5].tolist())
            assert np.array_equal(got["auc"], ints["auc"][:E], equal_nan=True), (name, limit, "auc")
            assert np.all(np.abs(got["sse"] - ints["sse"][:E]) <= eh.SSE_BOUND * ints["sse"][:E]), (name, limit, "sse")
        for k, _ in metrics.DeviceEvaluator.OUTPUTS:
            assert np.array_equal(a[k].view(np.uint8), b[k].view(np.uint8)), (name, limit, k, "the ranking call's auc_out")
        for got in (b, c):
            for k in metrics.RankingEvaluator.COUNTS:
                assert np.array_equal(got[k].astype(np.int64), topk[k][:, :E]), (name, limit, k, np.argwhere(got[k] != topk[k][:, :E])[:5].tolist())
        for got, key in ((p, "pl"), (q, "ll")):
            assert np.array_equal(got["n"], terms["n"][:E]) and np.array_equal(got["n_nan"], terms["n_nan"][:E]), (name, limit, key)
            bound = eh.PL_BOUND * terms["pl_mag"][:E] if key == "pl" else _ll_bound(terms["ll"][:E], terms["n"][:E])
            assert np.all(np.abs(got["pl"] - terms[key][:E]) <= bound), (name, limit, key)
        sums[limit] = dict(auc=a["auc"], sse=a["sse"], pl=p["pl"], ll=q["pl"])
    for limit in eh.LIMITS:      # an entity of the small path under both limits: the same bits, whatever width its wavefront took
        stay = sizes <= limit
        for k, v in sums[limit].items():
            assert np.array_equal(_bits(v[stay]), _bits(sums[eh.SMALL_MAX][k][stay])), (name, limit, k)
    return sums


@pytest.mark.parametrize("tail", [1, 2, 3])
def test_every_size_in_every_position_of_a_wavefront(device_solver, small_max, tail):
    rp, s, y, sizes = eh.quad_prefix(tail)
    assert (sizes.size % 4) == tail
    _small_geometry(device_solver, small_max, "quad_sweep", rp, s, y)


def test_packed_fields_at_their_maxima(device_solver, small_max):
    rp, s, y, names = eh.packed_maxima()
    _small_geometry(device_solver, small_max, "packed_maxima", rp, s, y)


# ---- the rank pass ----------------------------------------------------------------------------------------------------------------------
def test_rank_pass_on_its_edges(device_solver, small_max):
    """rank_edges with the small limit 0, so that every entity with a sample is a segment of the sorted keys: the integers of
    gdmix_re_eval_entities and of gdmix_re_eval_topk_entities (with and without auc_out) are the references'; the same samples as ONE
    accumulated set give the global integers."""
    rp, s, y, names = eh.rank_edges()
    rp, s, y = np.array(rp), np.array(s), np.array(y)      # (copies: the builder's arrays are read-only)
    ints = mref.per_entity_reference(rp, s, y)
    topk = rref.per_entity_counts(rp, s, y, eh.KS)
    assert ints["two_u"][names["tie_over_three_tiles"]] == ints["n_pos"][names["tie_over_three_tiles"]] * ints["n_neg"][names["tie_over_three_tiles"]]
    plain, ranker = metrics.DeviceEvaluator(device_solver), metrics.RankingEvaluator(device_solver, eh.KS)
    small_max(0)
    a = {k: _np(v) for k, v in plain.entities(rp, s, y).items()}
    b = {k: _np(v) for k, v in ranker.entities(rp, s, y).items()}
    c = {k: _np(v) for k, v in ranker.entities(rp, s, y, with_auc=False).items()}
    small_max(eh.SMALL_MAX)
    name_of = {e: n for n, e in names.items()}
    for got in (a, b):
        for k in ("two_u", "n_pos", "n_neg", "n_nan"):
            want = ints[k].astype(np.int64)
            assert np.array_equal(got[k].astype(np.int64), want), (k, [name_of[int(e)] for e in np.flatnonzero(got[k].astype(np.int64) != want)[:5]])
        assert np.array_equal(got["auc"], ints["auc"], equal_nan=True)
        assert np.all(np.abs(got["sse"] - ints["sse"]) <= eh.SSE_BOUND * ints["sse"])
    for got in (b, c):
        for k in metrics.RankingEvaluator.COUNTS:
            assert np.array_equal(got[k].astype(np.int64), topk[k]), (k, np.argwhere(got[k] != topk[k])[:5].tolist())
    two_u, n_pos, n_neg, n_nan = mref.two_u_reference(s, y)
    for cuts in ([0, s.size], [0, 15, eh.RANK_TILE + 1, s.size]):
        plain.reset()
        for lo, hi in zip(cuts[:-1], cuts[1:]):
            plain.add(s[lo:hi], y[lo:hi])
        r = plain.finish()
        assert (r["two_u"], r["n_pos"], r["n_neg"], r["n_nan"], r["n"]) == (two_u, n_pos, n_neg, n_nan, s.size) and n_nan == 4
