"""What tests/test_eval_edges.py (CPU) and tests/test_gpu_eval_edges.py (GPU) share: the evaluation units (csrc/re_evaluate_poisson.hip,
csrc/re_eval_sum.hpp, csrc/re_evaluate.hip) restated and driven ONTO what their code branches on.

  the term grid     fp32 scores over every exponent and sign with windows round the scores at which exp_any / exp_neg change what they do,
                    the labels of the two losses, and the terms in long double (exp(s) - y s; the header's ce formula) with their ulps.
  the shape         what a lane of the fixed-shape sum does with an entity of n samples (terms, closed runs, closed second levels) and what
                    an accumulator batch of N samples is (workgroups, terms per lane, workgroup sums per lane of the last tree).
  the recipes       integer data whose every partial sum is exact, given as formulas over the sample index so that the large arrays are
                    built on the device (numpy and torch both take them).
  the builders      quad_sweep, packed_maxima, rank_edges: (ent_row_ptr, score, label) of the four-per-wavefront geometry and of the rank
                    pass at their edges.

THE CONSTANTS are literals here, each next to the file it comes from; tests/test_gpu_eval_edges.py reads them from the sources and fails
until a changed one is changed here too — tests/test_eval_edges.py then names the situation the inputs no longer reach."""
import functools
import math
from fractions import Fraction

import numpy as np

# csrc/re_eval_sum.hpp
EVAL_THREADS = 256
EVAL_RUN = 2048
EVAL_RUNS = 64
ACC_MAX_GROUPS = 4096
ACC_PER_THREAD = 16
ACC_SAMPLES_PER_LANE = 16            # acc_groups: 16 samples per lane until the grid is full
ACC_GROUP_SAMPLES = EVAL_THREADS * ACC_SAMPLES_PER_LANE      # 4 096
# csrc/re_evaluate.hip
RANK_THREADS = 256
RANK_ITEMS = 16
RANK_TILE = RANK_THREADS * RANK_ITEMS                        # 4 096
SMALL_WIDTHS = (16, 32, 64)          # lanes per entity of the four-per-wavefront kernels
SMALL_MAX = 64

LIMITS = (64, 33, 32, 17, 16, 1, 0)  # gdmix_re_set_eval_small_max values of the small-geometry tests
KS = (1, 16, 63, 64)                 # precision@k

LD = np.longdouble
F32 = np.float32
TINY = 2.0 ** -1074                  # the spacing of subnormal doubles
MIN_NORMAL = 2.0 ** -1022
FLT_MAX = float(np.finfo(np.float32).max)


def require_long_double():
    """The references are long double of at least 64 mantissa bits (x87); numpy's nmant counts the stored ones."""
    assert np.finfo(np.longdouble).nmant >= 63, "np.longdouble is not an 80-bit format here: the term references need mpmath on a thinned grid"


# ---- the term grid ---------------------------------------------------------------------------------------------------------------------
def _f32(x):
    return np.float32(x)


def _step(x, toward, times=1):
    x = np.float32(x)
    for _ in range(times):
        x = np.nextafter(x, np.float32(toward), dtype=np.float32)
    return x


def exp_ld(s32):
    """exp of fp32 scores in long double (an 80-bit exp overflows past 11 356 only: +inf there, as for an infinite score)."""
    with np.errstate(over="ignore", under="ignore"):
        return np.exp(np.asarray(s32, np.float32).astype(LD))


def exp64(s32):
    """exp(s) rounded ONCE from long double to a double: +inf past the fp64 overflow, subnormal and 0 at the other end."""
    with np.errstate(over="ignore", under="ignore"):
        return exp_ld(s32).astype(np.float64)


@functools.lru_cache(maxsize=None)
def named_scores():
    """{name: fp32 score}. The overflow and underflow neighbours are COMPUTED from long double, not typed in."""
    out = {"zero": _f32(0.0), "minus_zero": _f32(-0.0)}
    for k in range(1, 9):
        out[f"tie+{k}"] = _f32(k * math.log(2.0) / 2.0)       # k odd: z log2(e) is half an integer, the tie of the reduction's rint
        out[f"tie-{k}"] = _f32(-k * math.log(2.0) / 2.0)
    out["fp32_exp_overflow+"] = _f32(88.72)
    out["fp32_exp_overflow-"] = _f32(-88.72)
    s = _f32(709.78)
    while np.isfinite(exp64(_step(s, np.inf))):
        s = _step(s, np.inf)
    while not np.isfinite(exp64(s)):
        s = _step(s, -np.inf)
    out["exp_last_finite"] = s                                 # kf = 1024 with p < 1
    out["exp_first_inf"] = _step(s, np.inf)
    out["exp_subnormal_from"] = _f32(-708.4)
    s = _f32(-745.13)
    while exp64(_step(s, -np.inf)) > 0.0:
        s = _step(s, -np.inf)
    while exp64(s) == 0.0:
        s = _step(s, np.inf)
    out["exp_last_nonzero"] = s
    out["exp_first_zero"] = _step(s, -np.inf)
    for v in (800.0, 1100.0, 3.4e38, np.inf):
        out[f"+{v:g}"] = _f32(v)
        out[f"-{v:g}"] = _f32(-v)
    return out


WINDOW = 64                          # fp32 values on each side of a named score
NO_WINDOW = ("+800", "-800", "+1100", "-1100", "+3.4e+38", "-3.4e+38", "+inf", "-inf", "minus_zero")


def _window(center):
    up, down = [np.float32(center)], [np.float32(center)]
    for _ in range(WINDOW):
        up.append(np.nextafter(up[-1], np.float32(np.inf), dtype=np.float32))
        down.append(np.nextafter(down[-1], np.float32(-np.inf), dtype=np.float32))
    return np.array(down[:0:-1] + up, np.float32)


@functools.lru_cache(maxsize=None)
def term_scores(mantissas=2048, seed=2026):
    """The fp32 scores of the term grid: `mantissas` per exponent (0 .. 254: denormals included) and sign, one drawn in each of as many equal
    strata of the 2^23 mantissas; the +-64-ulp windows; the extremes. Never changed after it is built."""
    rng = np.random.default_rng(seed)
    width = (1 << 23) // mantissas
    mant = (np.arange(mantissas, dtype=np.uint32) * np.uint32(width))[None, :] + rng.integers(0, width, (255, mantissas)).astype(np.uint32)
    bits = ((np.arange(255, dtype=np.uint32)[:, None] << np.uint32(23)) | mant).ravel()
    parts = [bits.view(np.float32), (bits | np.uint32(0x80000000)).view(np.float32)]
    for name, v in named_scores().items():
        parts.append(np.array([v], np.float32) if name in NO_WINDOW else _window(v))
    s = np.concatenate(parts).astype(np.float32)
    assert not np.isnan(s).any()
    s.setflags(write=False)
    return s


def exponent_counts(s32):
    """How many scores of each (sign, biased exponent) the grid holds: [2, 256]."""
    b = np.asarray(s32, np.float32).view(np.uint32)
    out = np.zeros((2, 256), np.int64)
    np.add.at(out, ((b >> np.uint32(31)).astype(np.int64), ((b >> np.uint32(23)) & np.uint32(0xFF)).astype(np.int64)), 1)
    return out


LL_LABELS = (0.0, 1.0, 0.5, float(np.nextafter(np.float32(0.5), np.float32(1.0))), 2.0, -1.0)
PL_LABELS = (0.0, 1.0, 3.0, float(2 ** 24), "cancel")


def cancel_labels(s32):
    """A label per score with y s within a factor 2 of exp(s) wherever fp32 can hold one (exp(s) / s rounded to fp32, held to the finite
    range; 0 where it underflows): the subtraction of the Poisson term cancels."""
    s = np.asarray(s32, np.float32).astype(LD)
    with np.errstate(all="ignore"):
        q = exp_ld(s32) / s
    q = np.where(np.isnan(q), LD(0.0), np.clip(q, -FLT_MAX, FLT_MAX))
    return q.astype(np.float32)


def pl_labels(s32, which):
    return cancel_labels(s32) if which == "cancel" else np.full(np.asarray(s32).shape, which, np.float32)


def ulp(x):
    """The spacing of doubles in the binade of |x| (long double in, long double out): 2^(e - 52) for 2^e <= |x| < 2^(e + 1), 2^-1074 at and
    below the subnormals, NaN for what is not finite."""
    x = np.abs(np.asarray(x, LD))
    fin = np.isfinite(x)
    _, e = np.frexp(np.where(fin, x, LD(1.0)))       # |x| = m 2^e, m in [0.5, 1)
    e = np.where(x == 0, -2000, e)
    u = np.ldexp(LD(1.0), np.maximum(e.astype(np.int64) - 53, -1074).astype(np.int32))
    return np.where(fin, u, LD(np.nan))


@functools.lru_cache(maxsize=None)
def term_exp():
    """exp_ld of the term grid, computed once."""
    e = exp_ld(term_scores())
    e.setflags(write=False)
    return e


def pl_reference(s32, y32, e=None):
    """-> (reference, ulp(exp(s)), ulp(reference), exp(s)) in long double: expl(s) - y s, the product of two floats exact in 64 bits.
    (e: exp_ld(s32) where the caller has it.)"""
    require_long_double()
    s = np.asarray(s32, np.float32).astype(LD)
    y = np.asarray(y32, np.float32).astype(LD)
    e = exp_ld(s32) if e is None else e
    with np.errstate(invalid="ignore", over="ignore"):
        ref = e - y * s
    return ref, ulp(e), ulp(ref), e


def ll_reference(s32, y32):
    """-> (reference, ulp(reference)) in long double: the header's ce, max(-s, 0) for a positive and max(s, 0) for a negative, plus
    log1p(exp(-|s|)). Never NaN: an infinite score gives 0 or +inf."""
    require_long_double()
    s = np.asarray(s32, np.float32).astype(LD)
    pos = np.asarray(y32, np.float32) > np.float32(0.5)
    with np.errstate(under="ignore"):
        ref = np.maximum(np.where(pos, -s, s), LD(0.0)) + np.log1p(np.exp(-np.abs(s)))
    return ref, ulp(ref)


def pl_term_bound(got, ref, ulp_e, ulp_ref, e):
    """The issue's bound of one Poisson term on the device, long double [n]; NaN where the term is checked exactly instead (the reference
    rounds to +-inf, NaN or 0). exp(s) normal in fp64: 0.98 ulp(exp(s)) + 0.5 ulp(got) + 2^-10 ulp(ref). Below: one spacing of the subnormals."""
    with np.errstate(over="ignore", under="ignore", invalid="ignore"):
        e64, ref64 = e.astype(np.float64), ref.astype(np.float64)
    normal = np.isfinite(e64) & (e64 >= MIN_NORMAL)
    b = np.where(normal, LD(0.98) * ulp_e + LD(0.5) * ulp(got) + ulp_ref / LD(1024.0), LD(TINY))
    exact = ~np.isfinite(ref64) | (ref64 == 0.0)
    return np.where(exact, LD(np.nan), b), ref64


# ---- the shape restated (csrc/re_eval_sum.hpp) -------------------------------------------------------------------------------------------
def lane_shape(n):
    """An entity of n samples on one workgroup: per lane t of 256 -> (terms, closed runs, closed second levels, terms after the last closed
    run, closed runs after the last closed second level), int64 [256] each. Lane t takes samples t, t + 256, ..."""
    t = np.arange(EVAL_THREADS, dtype=np.int64)
    terms = np.maximum((n - t + EVAL_THREADS - 1) // EVAL_THREADS, 0)
    runs = terms // EVAL_RUN
    return dict(terms=terms, runs=runs, tops=runs // EVAL_RUNS, after_run=terms % EVAL_RUN, after_top=runs % EVAL_RUNS)


def acc_shape(N):
    """An accumulator batch of N samples -> (groups, terms per lane of the grid [groups * 256], closed runs per lane, workgroup sums per
    lane of the last tree [256])."""
    groups = min((N + ACC_GROUP_SAMPLES - 1) // ACC_GROUP_SAMPLES, ACC_MAX_GROUPS)
    g = np.arange(groups * EVAL_THREADS, dtype=np.int64)
    stride = groups * EVAL_THREADS
    terms = np.maximum((N - g + stride - 1) // stride, 0)
    take = np.clip(groups - np.arange(EVAL_THREADS, dtype=np.int64) * ACC_PER_THREAD, 0, ACC_PER_THREAD)
    return dict(groups=int(groups), terms=terms, runs=terms // EVAL_RUN, tree_take=take)


ONE_RUN = EVAL_THREADS * EVAL_RUN                    # 524 288: every lane closes exactly one run
ONE_TOP = ONE_RUN * EVAL_RUNS                        # 33 554 432: every lane closes exactly one second level
RUN_EDGE_SIZES = (ONE_RUN - 1, ONE_RUN, ONE_RUN + 1, ONE_RUN + EVAL_THREADS + 1)
TOP_EDGE_SIZE = ONE_TOP + EVAL_THREADS + 1
ACC_EDGE_SIZES = (ACC_GROUP_SAMPLES, ACC_GROUP_SAMPLES + 1, 16 * ACC_GROUP_SAMPLES, 16 * ACC_GROUP_SAMPLES + 1,
                  ACC_MAX_GROUPS * ACC_GROUP_SAMPLES, ACC_MAX_GROUPS * ACC_GROUP_SAMPLES + EVAL_THREADS + 1)


def last_lane_last_term(n):
    """The index of the last sample the last lane (255) of an entity's workgroup adds."""
    assert n >= EVAL_THREADS
    return ((n - EVAL_THREADS) // EVAL_THREADS) * EVAL_THREADS + EVAL_THREADS - 1


# ---- the recipes: integer data as formulas over the sample index i (an int64 numpy array or torch tensor) --------------------------------
SSE_D_MOD, SSE_D_MUL = 1021, 37


def sse_recipe(i):
    """-> (score, label, d = label - score) as integers: d = (37 i) mod 1021 in 0 .. 1 020 differs from that of the next sample and of the
    lane's next term (i + 256), so a dropped term with its neighbour repeated changes the sum; every (y - s)^2 and every partial sum is an
    integer below 2^53 (sse_partial_sum_bound)."""
    d = (i * SSE_D_MUL) % SSE_D_MOD
    s = i % 7 - 3
    return s, s + d, d


def sse_partial_sum_bound(n):
    return n * (SSE_D_MOD - 1) ** 2


def unit_recipe(i):
    """-> (score, label): s = 0 and any integer label. Every Poisson term is exp(0) - y 0 = 1.0 exactly; every log-loss term is log 2."""
    return i * 0, i % 5


def mixed_recipe(i):
    """-> (score, label, code): s in {-1, 0, 1, 2} by i mod 4 and y in 0 .. 3 by i mod 13, all 16 pairs (code = 4 (s + 1) + y in 0 .. 15)."""
    s = (i * 3) % 4 - 1
    y = (i % 13) % 4
    return s, y, (s + 1) * 4 + y


def mixed_sums(counts, which):
    """The exact sum of the long-double terms of mixed_recipe rounded once each to a double, and the sum of their magnitudes (what the
    header's bound is relative to), from how often each of the 16 codes occurs -> (sum, magnitudes) as doubles."""
    codes = np.arange(16)
    s = (codes // 4 - 1).astype(np.float32)
    y = (codes % 4).astype(np.float32)
    if which == "pl":
        ref = pl_reference(s, y)[0]
        mag = exp_ld(s) + np.abs(y.astype(LD) * s.astype(LD))
    else:
        ref = ll_reference(s, y)[0]
        mag = ref
    tot = sum((Fraction(int(c)) * Fraction(float(r)) for c, r in zip(counts, ref.astype(np.float64))), Fraction(0))
    m = sum((Fraction(int(c)) * Fraction(float(r)) for c, r in zip(counts, mag.astype(np.float64))), Fraction(0))
    return float(tot), float(m)


PL_BOUND = 3e-13                     # include/gdmix_re.h, "poisson evaluation": |PL - exact| <= 3e-13 * sum (exp(s) + |y s|)
SSE_BOUND = 2.5e-13                  # "evaluation": relative error of SSE
LL_BOUND = 2.5e-13                   # the log loss: 2.5e-13 * sum of the terms + n * GDMIX_RE_EVAL_LL_TERM_EPS


# ---- the four-per-wavefront geometry ---------------------------------------------------------------------------------------------------
OTHERS = (0, 1, 16, 17, 32, 33, 64, 65, 200)
SWEEP_N = tuple(range(0, 67))
QUAD_TAIL = (64, 17, 5)              # the three entities behind the last full wavefront; a prefix of E - 2, E - 1 or E entities ends in 1, 2 or 3


@functools.lru_cache(maxsize=None)
def quad_sweep(seed=77):
    """-> (ent_row_ptr, score, label, sizes [E]): every n in 0 .. 66 at each of the four positions of a wavefront, the other three sizes
    drawn from OTHERS (each of them at every position too); then QUAD_TAIL. Scores on a grid of halves (ties inside every entity), both
    zeros; one NaN score in an entity of each width (<= 16, <= 32, <= 64) and in a larger one. quad_prefix cuts the batch tails."""
    rng = np.random.default_rng(seed)
    sizes, at = [], 0
    for n in SWEEP_N:
        for pos in range(4):
            quad = [OTHERS[(at + 3 * j + pos) % len(OTHERS)] for j in range(4)]
            at += 1
            quad[pos] = n
            sizes += quad
    sizes = np.array(sizes + list(QUAD_TAIL), np.int64)
    rp = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    N = int(rp[-1])
    s = (np.round(rng.standard_normal(N) * 2.0) / 2.0).astype(np.float32)
    s[rng.integers(0, N, 200)] = -0.0
    y = (rng.random(N) < 1.0 / (1.0 + np.exp(-s.astype(np.float64)))).astype(np.float32)
    y[rng.integers(0, N, 300)] = 3.0                       # (a count label for the Poisson term; positive for the others)
    for lo, hi in ((2, 16), (17, 32), (33, 64), (65, 200)):
        e = int(np.flatnonzero((sizes >= lo) & (sizes <= hi))[3])
        s[int(rp[e]) + int(sizes[e]) // 2] = np.nan
    for a in (rp, s, y, sizes):
        a.setflags(write=False)
    return rp, s, y, sizes


def quad_prefix(tail):
    """quad_sweep cut to a batch whose last wavefront holds `tail` (1, 2 or 3) entities -> (ent_row_ptr, score, label, sizes)."""
    rp, s, y, sizes = quad_sweep()
    E = sizes.size - len(QUAD_TAIL) + tail
    assert E % 4 == tail
    return rp[:E + 1], s[:int(rp[E])], y[:int(rp[E])], sizes[:E]


@functools.lru_cache(maxsize=None)
def packed_maxima():
    """-> (ent_row_ptr, score, label, names): four entities of 64 samples, one wavefront of four passes, that drive the packed fields of
    the small kernels to their maxima."""
    names = ("two_u_2048", "all_equal_mixed", "all_equal_positive", "all_nan")
    s, y = np.zeros((4, 64), np.float32), np.zeros((4, 64), np.float32)
    s[0, :32], y[0, :32] = np.arange(32) - 40.0, 0.0       # 32 negatives all below
    s[0, 32:], y[0, 32:] = np.arange(32) + 1.0, 1.0        # 32 positives: two_u = 2 * 32 * 32
    s[1], y[1, ::2] = 0.75, 1.0                            # one tie group of 32 + 32: two_u = 32 * 32
    s[2], y[2] = -1.25, 1.0                                # tie_size = tie_pos = 64 at k = 1
    s[3], y[3, :10] = np.nan, 1.0
    order = np.random.default_rng(5).permutation(64)
    s[0], y[0] = s[0][order], y[0][order]
    rp = np.arange(0, 257, 64, dtype=np.int64)
    return rp, s.ravel(), y.ravel(), names


# ---- the rank pass at its edges (run with the small limit 0: every entity with a sample is a segment of the sorted keys) ----------------
@functools.lru_cache(maxsize=None)
def rank_edges(seed=91):
    """-> (ent_row_ptr, score, label, names {name: entity}). The sorted segments lie in the entities' order, so a segment ends at the running
    sum of the sizes: 15 | 16 | 17 (a thread's 16 keys), 4 095 | 4 096 | 4 097 (a workgroup's tile) and 8 192; then one entity of 10 000 equal
    scores with mixed labels (one tie group over three tiles), 70 entities of 65 samples (wavefronts of several segments), one of 5 000
    (wavefronts wholly inside one segment) and one that ends on a tile edge with NaN scores (they sort last in their segment)."""
    rng = np.random.default_rng(seed)
    sizes, names = [], {}

    def add(name, n):
        names[name] = len(sizes)
        sizes.append(n)
    add("ends_15", 15), add("ends_16", 1), add("ends_17", 1)
    add("ends_4095", RANK_TILE - 1 - 17), add("ends_4096", 1), add("empty", 0), add("ends_4097", 1)
    add("ends_8192", 2 * RANK_TILE - (RANK_TILE + 1))
    add("tie_over_three_tiles", 10_000)
    for j in range(70):
        add(f"of_65_{j}", 65)
    add("of_5000", 5000)
    at = sum(sizes)
    add("nan_at_tile_edge", (-at) % RANK_TILE)
    sizes = np.array(sizes, np.int64)
    rp = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    N = int(rp[-1])
    s = (np.round(rng.standard_normal(N) * 4.0) / 4.0).astype(np.float32)
    y = (rng.random(N) < 0.4).astype(np.float32)
    e = names["tie_over_three_tiles"]
    s[rp[e]:rp[e + 1]] = 0.5
    e = names["nan_at_tile_edge"]
    s[rp[e] + np.array([0, 7, int(sizes[e]) - 1])] = np.nan
    e = names["ends_4095"]
    s[rp[e] + 5] = np.nan                                  # NaN keys just in front of the tile's last key
    for a in (rp, s, y):
        a.setflags(write=False)
    return rp, s, y, names
