"""Shared by tests/test_class_caps.py (CPU) and tests/test_gpu_class_caps.py (GPU): the tests' own statement of the size classes below the
tall ones — the 28 rows of re_solve_grp_kernel<G, EPL, NCAP, ZCAP> and the two LDS buckets of re_solve_wave_kernel (kClasses,
csrc/re_internal.hpp) —, of the first-fit rule of re_classify_kernel (csrc/re_route.hip), and entities that sit on a class's caps or one
past them. The table is a literal ON PURPOSE: a row changed in the library and not here fails test_the_table_is_the_librarys, and the
changed row then gets its entities at the new caps. Nothing new is compared here: narrow_helpers.compare_with_oracle,
re_linear_helpers.judge / oracle_strict and re_poisson_helpers.reference / compare / variance_numpy are the rules."""
import numpy as np

import narrow_helpers as nh
import re_linear_helpers as lh
import re_poisson_helpers as ph
from gdmix_amd import synthetic
from oracle import oracle

D = 8192
M_REG = 10               # more history pairs than this: no group class and no tall class
NUM_CLASSES = 40

# (G lanes per entity, EPL coefficient slots per lane, NCAP samples, ZCAP non-zeros), in routing order: classes 0 .. 27
GROUP_CLASSES = [
    (16, 2, 16, 64), (16, 2, 32, 128), (16, 2, 128, 512),
    (16, 3, 16, 64), (16, 3, 32, 128), (16, 3, 128, 512),
    (16, 4, 16, 64), (16, 4, 32, 128), (16, 4, 128, 512),
    (32, 3, 32, 128), (32, 3, 64, 256), (32, 3, 256, 1024),
    (32, 4, 32, 128), (32, 4, 64, 256), (32, 4, 256, 1024),
    (64, 3, 64, 512), (64, 3, 512, 2048),
    (64, 4, 64, 512), (64, 4, 512, 2048),
    (128, 3, 128, 1024), (128, 3, 1024, 3072),
    (128, 4, 128, 1024), (128, 4, 1024, 3072),
    (256, 3, 256, 2048), (256, 3, 2048, 4096),
    (256, 4, 256, 2048), (256, 4, 2048, 4096),
    (512, 4, 512, 4096)]
WAVE_BUCKETS = [24576, 65536]                                   # classes 28, 29
WAVE_24K, WAVE_64K = len(GROUP_CLASSES), len(GROUP_CLASSES) + 1
TALL_LEAN_CLASS, TALL_ONE_CLASS = 31, 32                        # "re_solve_tall_kernel<1> lean p<=64", "re_solve_tall_kernel<1> p<=64"
TALL_CLASSES = range(30, 35)
BLOCK_CLASS = 35                                                # "re_solve_team_kernel workgroup"
BLOCK_NAME = "re_solve_team_kernel workgroup"
TALL_MAX_P = 64
TALL_LEAN_ARENA = (160 * 1024 // 12 - 512 - 1408) & ~15         # what a lean workgroup can stage (tall_lds_bytes(12) - 1408, csrc/re_internal.hpp)


def class_names():
    """The names of classes 0 .. 29 as gdmix_re_class_kernel_name spells them."""
    return ([f"re_solve_grp_kernel<{g},{epl}> n<={ncap} nnz<={zcap}" for g, epl, ncap, zcap in GROUP_CLASSES] +
            [f"re_solve_wave_kernel lds<={b // 1024}K" for b in WAVE_BUCKETS])


def wave_lds_bytes(p, n, nnz, d, m, has_w):
    """LDS bytes of an entity in re_solve_wave_kernel (csrc/re_internal.hpp, restated)."""
    dbl = (5 + 2 * m) * p + n + 2 * m
    w32 = 4 * nnz + (n + 1) + (d + 1) + (3 if has_w else 2) * n
    return (dbl * 8 + w32 * 4 + 15) & ~15


def tall_resident_bytes(nw, sets, d, n, nnz, has_w):
    return nw * (d + 1) * (sets + 1) * 8 + 8 * (nnz + 8) + 4 * (n + 2) + (12 if has_w else 8) * n + 16


def route(p, n, nnz, m, has_w, tall_min_n, ic=1, team_nnz=16384):
    """The class of an entity of p coefficients (ic of them the intercept), n samples and nnz non-zeros: the first group class whose three
    caps hold it (m <= 10 only), then the first wavefront bucket that holds its wave_lds_bytes, else the workgroup class; with
    tall_min_n > 0 an entity of p <= 64 and n >= tall_min_n (m <= 10) is tall instead: the lean one-wavefront class when it is resident
    in a lean workgroup's arena, else the one-wavefront class. The team, giant and tall-split thresholds are at their defaults
    (16 384 non-zeros and more, 512 samples and more at p <= 64), out of reach of the shapes of this file. team_nnz: the first non-zero
    count this rule does not speak for (team_edges_helpers.route_large states the tiers from there on and passes its own)."""
    assert nnz < team_nnz and not (p <= TALL_MAX_P and n >= 512)
    d = p - ic
    c = BLOCK_CLASS
    for k, (g, epl, ncap, zcap) in enumerate(GROUP_CLASSES):
        if m <= M_REG and p <= g * epl and n <= ncap and nnz <= zcap:
            c = k
            break
    else:
        for k, bucket in enumerate(WAVE_BUCKETS):
            if wave_lds_bytes(p, n, nnz, d, m, has_w) <= bucket:
                c = len(GROUP_CLASSES) + k
                break
    if tall_min_n > 0 and m <= M_REG and p <= TALL_MAX_P and n >= tall_min_n:
        c = TALL_LEAN_CLASS if tall_resident_bytes(1, 16, d, n, nnz, has_w) <= TALL_LEAN_ARENA else TALL_ONE_CLASS
    return c


def _kind_range(k):
    """(lowest, highest) p of the kind (G, EPL) of class k: the previous kind's cap + 1 .. G * EPL."""
    caps = sorted({g * epl for g, epl, _, _ in GROUP_CLASSES})
    cap = GROUP_CLASSES[k][0] * GROUP_CLASSES[k][1]
    i = caps.index(cap)
    return (caps[i - 1] + 1 if i else 1), cap


def corners():
    """[(p, n, nnz, class)]: one entity per group class at all three caps. It belongs to its class by construction: every earlier
    class has a smaller cap on the coefficients, the samples or the non-zeros."""
    return [(g * epl, ncap, zcap, k) for k, (g, epl, ncap, zcap) in enumerate(GROUP_CLASSES)]


def edges(m=10, has_w=False):
    """[(p, n, nnz, class)]: per group class k
        the corner;
        the lowest p of the kind's range at NCAP and ZCAP (not for <16,2>: its lowest p is 1, an intercept alone, and an entity of
            the generator has a feature);
        p = cap with one sample and one non-zero per column (the first class of the kind takes it: dropped for the others);
        p = cap, n = NCAP and max(d, n) non-zeros: one per row or column;
        n = min(NCAP, ZCAP) at ZCAP in the middle of the kind's range of p (a last lane that is partly filled).
    Those that route() places in another class are dropped. 121 entities with the table above."""
    out = []
    for k, (g, epl, ncap, zcap) in enumerate(GROUP_CLASSES):
        lo, cap = _kind_range(k)
        cand = [(cap, ncap, zcap)]
        if lo > 1:
            cand.append((lo, ncap, zcap))
        cand += [(cap, 1, max(cap - 1, 1)), (cap, ncap, max(cap - 1, ncap)), ((lo + cap) // 2, min(ncap, zcap), zcap)]
        out += [(p, n, z, k) for p, n, z in cand if z >= max(p - 1, n) and route(p, n, z, m, has_w, 0) == k]
    return out


def neighbours(m=10, has_w=False):
    """[(p, n, nnz, class by route(), the group class whose cap it is one past)]: per group class p + 1, n + 1 and nnz + 1 of the corner."""
    out = []
    for k, (g, epl, ncap, zcap) in enumerate(GROUP_CLASSES):
        for p, n, z in ((g * epl + 1, ncap, zcap), (g * epl, ncap + 1, zcap), (g * epl, ncap, zcap + 1)):
            out.append((p, n, z, route(p, n, z, m, has_w, 0), k))
    return out


WAVE_M = 12
WAVE_SIZES = (24576, 24592, 65536, 65552)
# (d, n) per bucket: wide, in between, tall. All twelve entities of either list are strict by the oracle alone; with (9, 300) and
# (120, 500) as the tall pair two of them ran 70 iterations and were not
WAVE_PAIRS = {24576: ((59, 8), (30, 64), (20, 100)), 65536: ((65, 40), (257, 8), (150, 100))}


def wave_bucket_shapes(has_w):
    """[(p, n, nnz, class, bytes)] for m = 12 and an intercept: entities whose wave_lds_bytes is exactly a bucket (the last that fits) and
    16 bytes, one non-zero, more (the first that does not). One more non-zero adds 16 bytes, so an exact hit always exists."""
    out = []
    for size in WAVE_SIZES:
        for d, n in WAVE_PAIRS[24576 if size < 65536 else 65536]:
            z = (size - wave_lds_bytes(d + 1, n, 0, d, WAVE_M, has_w)) // 16
            z = next(k for k in (z - 1, z, z + 1) if wave_lds_bytes(d + 1, n, k, d, WAVE_M, has_w) == size)
            assert z >= max(d, n), (d, n, z, size)
            out.append((d + 1, n, z, route(d + 1, n, z, WAVE_M, has_w, 0), size))
    return out


def shaped_batch(shapes, seed, ic=1, random_weights=False):
    """narrow_helpers.make_shaped_batch over D = 8192 for entities stated by their p (d = p - ic features)."""
    return nh.make_shaped_batch([(s[0] - ic, s[1], s[2]) for s in shapes], seed=seed, D=D, random_weights=random_weights)


# ---- the cases of tests/test_gpu_class_caps.py: (shapes, batch, solver options, loss), with the reference's own run ---------------------
KW_EDGES = dict(l2=1.0, regularize_bias=True, has_intercept=True, m=10, max_iter=100, ftol=1e-12)
# corners at l2 = 10: at l2 = 1 the squared loss with an unregularised intercept takes 100 and more iterations on the classes of many
# samples and moves under rounding (not strict)
KW_CORNERS = dict(KW_EDGES, l2=10.0, regularize_bias=False)
KW_NO_INTERCEPT = dict(KW_EDGES, has_intercept=False)
KW_WAVE = dict(KW_EDGES, m=WAVE_M, l2=0.01)
RAGGED_CLASSES = (7, 13)            # <16,4> n<=32 nnz<=128 and <32,4> n<=64 nnz<=256
RAGGED_SIZES = (1, 2, 3, 5)
LOSSES = ("logistic", "squared", "poisson")
SEED = 5      # the first seed at which the oracle's own runs meet the conditions of tests/test_class_caps.py


def _with_labels(b, loss, seed):
    if loss == "squared":
        return synthetic.with_real_labels(b, seed=seed)
    if loss == "poisson":
        return synthetic.with_count_labels(b, seed=seed)
    return b


def case_names():
    names = ["edges", "neighbours"]
    names += [f"corners-{loss}" for loss in LOSSES] + [f"corners_no_intercept-{loss}" for loss in LOSSES]
    names += [f"ragged-{c}-{size}" for c in RAGGED_CLASSES for size in RAGGED_SIZES]
    return names + ["wave", "wave_weights"]


_CASES = {}


def case(name):
    """-> dict(shapes [(p, n, nnz, class, ...)], b, kw, loss, ic). Built once per name."""
    if name in _CASES:
        return _CASES[name]
    kind, _, arg = name.partition("-")
    loss = "logistic"
    if kind == "edges":
        shapes, kw, b = edges(), KW_EDGES, None
    elif kind == "neighbours":
        shapes, kw, b = neighbours(), KW_EDGES, None
    elif kind == "corners":
        loss, shapes, kw = arg, corners(), KW_CORNERS
        b = _with_labels(shaped_batch(shapes, SEED, random_weights=True), loss, SEED)
    elif kind == "corners_no_intercept":      # d = G * EPL: the last slot of the last lane holds a feature
        loss, shapes, kw = arg, corners(), KW_NO_INTERCEPT
        b = _with_labels(shaped_batch(shapes, SEED, ic=0, random_weights=True), loss, SEED)
    elif kind == "ragged":
        c, size = (int(x) for x in arg.split("-"))
        shapes, kw = [corners()[c]] * size, KW_EDGES
        b = shaped_batch(shapes, 100 * c + size)
    elif kind in ("wave", "wave_weights"):
        shapes, kw = wave_bucket_shapes(kind == "wave_weights"), KW_WAVE
        b = shaped_batch(shapes, SEED, random_weights=kind == "wave_weights")
    else:
        raise KeyError(name)
    if b is None:
        b = shaped_batch(shapes, SEED)
    _CASES[name] = dict(name=name, shapes=shapes, b=b, kw=kw, loss=loss, ic=1 if kw["has_intercept"] else 0)
    return _CASES[name]


_REFS = {}


def reference(name):
    """The reference's own run of a case, computed once and left unchanged -> dict(pk, coef_ptr, ref, strict [E] bool, nit [E]).
    logistic, squared: oracle.solve (SIMPLE variance on for logistic: the oracle's variance is the logistic one), strict by
    re_linear_helpers.oracle_strict; Poisson: scipy by re_poisson_helpers.reference, strict as it says."""
    if name in _REFS:
        return _REFS[name]
    c = case(name)
    b, kw = c["b"], c["kw"]
    pk = oracle.pack(b.ent_row_ptr, b.row_nnz_ptr, b.col_global)
    cp = pk["ent_feat_ptr"] + np.arange(b.E + 1) * c["ic"]
    if c["loss"] == "poisson":
        ref = ph.reference(b, pk, kw, None, cp, key=("class_caps", name), entities=np.arange(b.E))
        strict, nit = ref["strict"] & (ref["status"] != 1), ref["nit"]
    else:
        okw = dict(kw, variance_mode=0, linear=True, sum_loss=False) if c["loss"] == "squared" else dict(kw, variance_mode=1)
        ref, strict, _, _ = lh.oracle_strict(b, pk, oracle.make_opts(**okw), None, int(cp[-1]))
        nit = ref["nit"]
    _REFS[name] = dict(pk=pk, coef_ptr=cp, ref=ref, strict=strict, nit=np.asarray(nit))
    return _REFS[name]
