"""Shared by tests/test_tall_edges.py (CPU) and tests/test_gpu_tall_edges.py (GPU): entities built to sit ON what the tall kernels
branch on (csrc/re_solve_tall.hip: re_solve_tall_kernel<1>, <1> lean, <4>, <8> and re_solve_tall_team_kernel<8> x4) — the trip of a
pass, the LDS arena, the accumulator sets, the padded tail of the batch, samples without entries and repeated columns, a team whose
members live in different homes — and the tests' own statement of what tall_setup and tall_pass do with an entity (pass_plan,
team_slices, slice_plan) and of where re_classify_kernel and class_base_kernel send it under pinned knobs (route_tall).

The constants are literals ON PURPOSE: one changed in the library and not here fails test_the_constants_are_the_librarys, and
tests/test_tall_edges.py then names the situations the batches no longer show. Nothing new is compared here:
narrow_helpers.compare_with_oracle, re_linear_helpers.oracle_strict and re_poisson_helpers.reference / compare are the rules; the
per-entity SIMPLE variance is restated densely (variance_dense) because the repeated cells of `structures` are summed before squaring.

An entity is drawn from a generator of its own, seeded by (SEED, its name, its draw): a shape that needs another draw (REDRAW) moves
no other entity, and an entity has the same arrays wherever it stands in a batch."""
import zlib

import numpy as np

import class_caps_helpers as ch
import re_linear_helpers as lh
import re_poisson_helpers as ph
from class_caps_helpers import tall_resident_bytes      # (the one restatement of csrc/re_internal.hpp's formula)
from gdmix_amd.batch import RawBatch
from oracle import oracle

WAVE = 64
# csrc/re_internal.hpp
TALL_MAX_P = 64
TALL_TEAM_C = 4
TALL_TEAM_MIN_N = 64
TALL_NW = 8
TALL_NW_SMALL = 1            # GDMIX_TALL_NW_SMALL
TALL_NW_MID = 4
TALL_MID_WGS = 2
TALL_LEAN_WGS = 12           # 4 * TALL_LEAN_WAVES, TALL_LEAN_WAVES = 3
# csrc/re_solve_tall.hip
TALL_TAIL = 8
GDMIX_TALL_R8 = 1            # samples per thread and trip of the 8-wide pass
GDMIX_TALL_WAVES_SMALL = 2   # the <1> launch has 4 * GDMIX_TALL_WAVES_SMALL / TALL_NW_SMALL workgroups per CU
TALL_R4_PREFETCH = 2         # tall_rows_fast<NW, PF ? 2 : 1, 4, ...>: samples per thread and trip of the 4-wide pass with loads ahead
TALL_REDUCE = 16             # tall_pass reads a column's accumulator sets sixteen at a time
# include/gdmix_re.h
TALL_SPLIT_N_DEFAULT = 4096
TALL_TEAM_N_DEFAULT = 8192
M_REG = ch.M_REG

TALL_TEAM_CLASS, TALL_LEAN_CLASS, TALL_ONE_CLASS, TALL_MID_CLASS, TALL_LARGE_CLASS = 30, 31, 32, 33, 34
TALL_NAMES = ["re_solve_tall_team_kernel<8> x4 p<=64", "re_solve_tall_kernel<1> lean p<=64", "re_solve_tall_kernel<1> p<=64",
              "re_solve_tall_kernel<4> p<=64", "re_solve_tall_kernel<8> p<=64"]
NOT_TALL = -1                # route_tall: the entity leaves the tall classes (class_caps_helpers.route and team_edges_helpers.route_large speak there)
TALL_LDS_FIELDS = ["xs[WAVE]", "acc[NW][WAVE]", "red[NW][2]", "rho[M_REG]", "alpha[M_REG]", "ls[16]", "cur", "ctl", "kmax", "pad"]


def tall_lds_bytes(w):
    return 160 * 1024 // w - 512


def tall_lds_sizeof(nw):
    """sizeof(TallLds<NW>): xs[64], acc[NW][64], red[NW][2], rho[10], alpha[10], ls[16] doubles and four ints = 816 + 528 NW."""
    return 8 * (WAVE + nw * WAVE + nw * 2 + M_REG + M_REG + 16) + 4 * 4


def tall_sets(nw, p):
    return 32 if (nw > 1 and p <= 32) else 16


# variant -> (wavefronts, loads ahead (PF), workgroups per CU, class)
VARIANTS = {"one": (TALL_NW_SMALL, True, 4 * GDMIX_TALL_WAVES_SMALL // TALL_NW_SMALL, TALL_ONE_CLASS),
            "lean": (1, False, TALL_LEAN_WGS, TALL_LEAN_CLASS),
            "mid": (TALL_NW_MID, True, TALL_MID_WGS, TALL_MID_CLASS),
            "large": (TALL_NW, True, 1, TALL_LARGE_CLASS),
            "team": (TALL_NW, True, 1, TALL_TEAM_CLASS)}
SOLO = ("one", "lean", "mid", "large")


def arena(variant):
    """tall_arena_bytes<NW>(tall_lds_bytes(workgroups per CU)): what tall_setup may carve up."""
    nw, _, wgs, _ = VARIANTS[variant]
    return (tall_lds_bytes(wgs) - tall_lds_sizeof(nw)) & ~15


TALL_LEAN_ARENA = (tall_lds_bytes(TALL_LEAN_WGS) - 1408) & ~15      # re_classify_kernel's threshold of the lean class
ARENA_FIGURES = {"one": 18624, "lean": 11792, "mid": 78480, "large": 158288, "team": 158288}


# ---- what tall_setup and tall_pass do with an entity ----------------------------------------------------------------------------------
def pass_plan(entity, variant, has_w, ic):
    """entity: dict(lens [row lengths of the samples this workgroup takes], d, room [entries from the entity's first to the end of the
    batch's arrays, Z - z0], k_lo [the entity-relative index of the slice's first entry, 0 for a whole entity]).
    -> dict(NT threads, R samples per thread and trip, width 4 | 8 | 0 (by the longest sample: the straight-line passes, or the general
    one), trips of the pass, S accumulator sets, bytes, resident, tail: a window of the fast pass starts past safe_end - W and reads
    TallTail — only a streamed workgroup, only the fast pass (the general pass and the variance pass load entry by entry)."""
    nw, pf, _, _ = VARIANTS[variant]
    lens = np.asarray(entity["lens"], np.int64)
    n, nnz, d = int(lens.size), int(lens.sum()), int(entity["d"])
    NT = WAVE * nw
    kmax = int(lens.max()) if n else 0
    width = 4 if kmax <= 4 else (8 if kmax <= 8 else 0)
    R = (TALL_R4_PREFETCH if pf else 1) if width == 4 else (GDMIX_TALL_R8 if width == 8 else 1)
    S = tall_sets(nw, d + ic)
    nbytes = tall_resident_bytes(nw, S, d, n, nnz, has_w)
    resident = n > 0 and nbytes <= arena(variant)
    last_k0 = int(entity.get("k_lo", 0)) + (nnz - int(lens[-1]) if n else 0)
    tail = bool(n > 0 and not resident and width != 0 and last_k0 + width > int(entity["room"]))
    return dict(NT=NT, R=R, width=width, trips=-(-n // (R * NT)), S=S, bytes=nbytes, resident=bool(resident), tail=tail)


def team_slices(n):
    """-> (q = ceil(n / 4), [(i0, i1)] of the four members)."""
    q = -(-n // TALL_TEAM_C)
    return q, [(min(m * q, n), min(m * q + q, n)) for m in range(TALL_TEAM_C)]


def slice_plan(entity, has_w, ic):
    """pass_plan per member of a team on `entity` (a whole entity: lens, d, room)."""
    lens = np.asarray(entity["lens"], np.int64)
    starts = np.concatenate([[0], np.cumsum(lens)])
    return [pass_plan(dict(lens=lens[i0:i1], d=entity["d"], room=entity["room"], k_lo=int(starts[i0])), "team", has_w, ic)
            for i0, i1 in team_slices(lens.size)[1]]


def route_tall(p, n, nnz, m, has_w, knobs, ic=1):
    """The tall class of an entity under PINNED knobs (dict: tall_min_n, tall_split_n > 0, tall_mid_n >= 0, tall_team_n <= 0), or NOT_TALL.
    csrc/re_route.hip lines 90 - 91: p <= 64, n >= tall_min_n, m <= 10 -> the eight-wavefront class from tall_split_n samples on, else
    lean when tall_resident_bytes(1, 16, ...) <= TALL_LEAN_ARENA, else one wavefront. class_base_kernel / re_order_kernel with fixed
    thresholds: tall_mid_n > 0 moves the ONE-WAVEFRONT entities of at least that many samples to <4> (lean ones stay lean);
    tall_team_n < 0 moves the eight-wavefront entities of at least max(-tall_team_n, 64) samples to a team."""
    split, mid, team = knobs.get("tall_split_n", 0), knobs.get("tall_mid_n", 0), knobs.get("tall_team_n", 0)
    assert split > 0 and mid >= 0 and team <= 0, "the per-batch choices stay with tests/test_gpu_parity.py"
    tall_min_n = knobs.get("tall_min_n", 32)
    if not (tall_min_n > 0 and m <= M_REG and p <= TALL_MAX_P and n >= tall_min_n):
        return NOT_TALL
    if n >= split:
        return TALL_TEAM_CLASS if (team < 0 and n >= max(-team, TALL_TEAM_MIN_N)) else TALL_LARGE_CLASS
    if tall_resident_bytes(1, tall_sets(1, p), p - ic, n, nnz, has_w) <= TALL_LEAN_ARENA:
        return TALL_LEAN_CLASS
    return TALL_MID_CLASS if (mid > 0 and n >= mid) else TALL_ONE_CLASS


ROUTING = {"one": dict(tall_min_n=1, tall_team_n=0, tall_split_n=TALL_SPLIT_N_DEFAULT, tall_mid_n=0),      # lean or <1>, by the bytes
           "mid": dict(tall_min_n=1, tall_team_n=0, tall_split_n=TALL_SPLIT_N_DEFAULT, tall_mid_n=1),      # lean or <4>
           "large": dict(tall_min_n=1, tall_team_n=0, tall_split_n=1, tall_mid_n=0),                      # <8>
           "team": dict(tall_min_n=1, tall_team_n=-1, tall_split_n=1, tall_mid_n=0),                      # -1 is clamped to 64: a team from 64 samples on, else <8>
           "ladder": dict(tall_min_n=1, tall_team_n=-600, tall_split_n=300, tall_mid_n=1)}                # lean / <4> below 300, <8> below 600, a team from there
ROUTING["lean"] = ROUTING["one"]

# ---- entities ---------------------------------------------------------------------------------------------------------------------------
LOSSES = ch.LOSSES
KW = dict(l2=10.0, regularize_bias=False, m=10, max_iter=100, ftol=1e-12)
TINY_BATCHES = ("trips:lean", "trips:large")      # they hold entities of 1 and 2 samples, which have a minimiser only under a regularised intercept


def batch_kw(batch, ic):
    """The options of a batch: the intercept is NOT regularised (the fits and the variance's regulariser see first_reg = 1) except in the
    two batches with the entities of one and two samples."""
    return dict(KW, has_intercept=bool(ic), regularize_bias=batch in TINY_BATCHES)
SEED = 7                 # every named entity is strict by the reference alone for the three losses, with and without an intercept (tests/test_tall_edges.py)
REDRAW = {}              # name -> draw: a shape whose first draw is not strict under SEED gets one of its own
F = 24                   # the feature space of an entity unless its spec says otherwise


def build_entity(name, lens, F=F, rule="perm", want=None, tags=()):
    """An entity over a feature space of F columns whose sample i has exactly lens[i] entries. The first F entry slots, in row-major
    order, take columns 0 .. F - 1 (every feature occurs when the entity has F entries; a sample's columns stay distinct), the others by
    `rule`:
        perm      distinct random columns per sample;
        dup       perm, then in every third later sample of two and more entries the LAST entry takes the column of the FIRST;
        same      perm, then every sample of nine and more entries is its first column repeated;
        lastcol   every later entry is column F - 1 (samples of one entry).
    Values N(0, 1) / 2 fp32, offsets N(0, 1) / 2, weights in [0.25, 2.25); labels for the three losses from a hidden w* and entity bias:
    y ~ Bernoulli(sigmoid(logit)), 2 y + N(0, 1), Poisson(exp(0.7 y + 0.3 N(0, 1))) (the rules of gdmix_amd.synthetic, per entity)."""
    rng = np.random.default_rng([SEED, zlib.crc32(name.encode()), REDRAW.get(name, 0)])
    lens = np.asarray(lens, np.int64)
    n, nnz = int(lens.size), int(lens.sum())
    assert n >= 1 and lens.min() >= 0 and lens.max() <= F, name
    starts = np.concatenate([[0], np.cumsum(lens)])
    later = starts[:-1] >= F                                          # samples behind the F entry slots that cover the features
    perm = np.argsort(rng.random((n, F)), axis=1)
    col = perm[np.arange(F)[None, :] < lens[:, None]].astype(np.int64)      # row-major: the first lens[i] of sample i's permutation
    for i in np.flatnonzero(~later & (lens > 0)):
        k0, k = int(starts[i]), int(lens[i])
        fixed = np.arange(k0, min(k0 + k, F))
        col[k0:k0 + k] = np.concatenate([fixed, rng.permutation(np.setdiff1d(np.arange(F), fixed))[:k - fixed.size]])
    if rule == "lastcol":
        col[np.repeat(later, lens)] = F - 1
    elif rule == "dup":
        rows = np.flatnonzero(later & (lens >= 2) & (np.arange(n) % 3 == 0))
        col[starts[rows] + lens[rows] - 1] = col[starts[rows]]
    elif rule == "same":
        for i in np.flatnonzero(later & (lens >= 9)):
            col[starts[i]:starts[i + 1]] = col[starts[i]]
    val = (rng.standard_normal(nnz) / 2.0).astype(np.float32)
    offset = (0.5 * rng.standard_normal(n)).astype(np.float32)
    weight = (0.25 + 2.0 * rng.random(n)).astype(np.float32)
    w_star = 0.5 * rng.standard_normal(F)
    row_of = np.repeat(np.arange(n), lens)
    logit = np.bincount(row_of, weights=val.astype(np.float64) * w_star[col], minlength=n) + 0.5 * rng.standard_normal() + offset
    y01 = (rng.random(n) < 1.0 / (1.0 + np.exp(-logit))).astype(np.float32)
    y = {"logistic": y01, "squared": (2.0 * y01 + rng.standard_normal(n)).astype(np.float32),
         "poisson": rng.poisson(np.exp(0.7 * y01 + 0.3 * rng.standard_normal(n))).astype(np.float32)}
    return dict(name=name, lens=lens, col=col, val=val, offset=offset, weight=weight, y=y, F=F, d=int(np.unique(col).size), want=want, tags=tuple(tags),
                rule=rule)


def lens_between(rng_key, n, lo, hi, force=()):
    """n row lengths drawn uniformly from lo .. hi (a generator of their own: the lengths are part of the shape, not of the draw);
    force: (index, length) pairs set afterwards."""
    rng = np.random.default_rng([0x7A11, zlib.crc32(rng_key.encode())])
    lens = rng.integers(lo, hi + 1, size=n)
    for i, k in force:
        lens[i] = k
    return lens


def lens_total(rng_key, n, nnz):
    """n row lengths of exactly nnz entries in all: nnz // n everywhere and one more in randomly chosen samples."""
    rng = np.random.default_rng([0x7A12, zlib.crc32(rng_key.encode())])
    base, extra = divmod(nnz, n)
    lens = np.full(n, base, np.int64)
    lens[rng.choice(n, size=extra, replace=False)] += 1
    return lens


def assemble(entities, loss, has_w):
    """The entities in this order as one RawBatch with the loss's labels; entity_ids are their names."""
    ent_n = np.array([e["lens"].size for e in entities], np.int64)
    lens = np.concatenate([e["lens"] for e in entities])
    return RawBatch(ent_row_ptr=np.concatenate([[0], np.cumsum(ent_n)]), row_nnz_ptr=np.concatenate([[0], np.cumsum(lens)]).astype(np.int64),
                    col_global=np.concatenate([e["col"] for e in entities]).astype(np.int64), val=np.concatenate([e["val"] for e in entities]),
                    y=np.concatenate([e["y"][loss] for e in entities]), offset=np.concatenate([e["offset"] for e in entities]),
                    weight=np.concatenate([e["weight"] for e in entities]) if has_w else None, entity_ids=[e["name"] for e in entities],
                    binary_labels=loss == "logistic")


def placed(entities):
    """{name: dict(lens, d, room, index)}: what pass_plan needs of every entity, given its place in this batch."""
    nnz = np.array([int(e["lens"].sum()) for e in entities], np.int64)
    z0 = np.concatenate([[0], np.cumsum(nnz)])
    return {e["name"]: dict(lens=e["lens"], d=e["d"], room=int(z0[-1] - z0[k]), index=k) for k, e in enumerate(entities)}


# ---- the batches: {name: entity}, in batch order (a dict keeps it) -------------------------------------------------------------------------
WIDTHS_OF_TRIPS = (4, 8, 0)
TRIP_SITUATIONS = ("T-1", "T", "T+1", "2T-1", "2T", "2T+1", "3T+1")


def trip_counts(variant, width):
    """{situation: n} for the pass the variant runs on an entity of this width class: T = R NT samples per trip."""
    nw, pf, _, _ = VARIANTS[variant]
    R = (TALL_R4_PREFETCH if pf else 1) if width == 4 else (GDMIX_TALL_R8 if width == 8 else 1)
    T = R * WAVE * nw
    return dict(zip(TRIP_SITUATIONS, (T - 1, T, T + 1, 2 * T - 1, 2 * T, 2 * T + 1, 3 * T + 1)))


def _trip_lens(variant, width, name, n):
    """Row lengths of a `trips` entity: the lean ones short (they must stay within TALL_LEAN_ARENA), the others long (the <1> and <4> ones
    must exceed it: 3 - 4 entries at width 4, 5 - 8 otherwise); width 8 has samples of 8 and 5 at its first and last sample, width 0 one
    sample of 9 at its last."""
    lo, hi = (1, 2) if variant == "lean" else ((3, 4) if width == 4 else (5, 8))
    force = [] if width == 4 else ([(0, 8), (n - 1, 5)] if width == 8 else [(n - 1, 9)])
    return lens_between(name, n, lo, hi, force)


def _feature_space(variant, lens):
    """24 features where the entity then goes to the variant's class with and without weights; else the smallest of 40 and 60 at which
    it does (a <1> entity of 127 samples of at most four entries has 9 584 B at 24 features and would run lean)."""
    if variant in ("lean", "large"):
        return F
    n, nnz = int(lens.size), int(lens.sum())
    for f in (F, 40, 60):
        if all(route_tall(f + ic, n, nnz, 10, w, ROUTING[variant], ic) == VARIANTS[variant][3] for w in (True, False) for ic in (0, 1)):
            return f
    raise AssertionError((variant, n, nnz))


_BUILT = {}


def _entity(name, lens, **kw):
    key = (name, REDRAW.get(name, 0))
    if key not in _BUILT:
        _BUILT[key] = build_entity(name, lens, **kw)
    return _BUILT[key]


def trips(variant):
    """One entity per width class and trip situation of the variant, plus n = 1 and n = 2 where the routing can take them (lean, and <8>
    through tall_split_n = 1). The largest: 3 073 samples on <8> at width 4."""
    out = {}
    for width in WIDTHS_OF_TRIPS:
        for sit, n in trip_counts(variant, width).items():
            name = f"trips-{variant}-w{width}-{sit}"
            lens = _trip_lens(variant, width, name, n)
            out[name] = _entity(name, lens, F=_feature_space(variant, lens), want=variant, tags=("trip", width, sit))
    if variant in ("lean", "large"):
        for n in (1, 2):
            name = f"trips-{variant}-n{n}"
            out[name] = _entity(name, np.full(n, 3), want=variant, tags=("tiny", n))
    return out


def _exact_shape(variant, d, S_p, has_w, n, target):
    """nnz such that an entity of d features, n samples and p = S_p coefficients (for the accumulator sets) has exactly `target` bytes."""
    nw = VARIANTS[variant][0]
    z = (target - tall_resident_bytes(nw, tall_sets(nw, S_p), d, n, 0, has_w)) // 8
    assert tall_resident_bytes(nw, tall_sets(nw, S_p), d, n, z, has_w) == target and z >= max(d, n), (variant, d, n, z, target)
    return z


ARENA_N = {"one": 400, "lean": 200, "mid": 1000, "large": 3000}


def arena_batch(variant, has_w, ic, last=None):
    """Per arena the variant's routing reaches: an entity of exactly the arena's bytes (`exact`), one more entry (`entry`: 8 B more) and
    one more sample with the same entries (`sample`). "one": the lean routing threshold, the lean kernel's own arena (out of the lean
    class's reach: it runs on <1>) and the <1> arena; "mid", "large": at p <= 32 (24 features, S = 32) and at p = 33 (33 - ic features,
    S = 16); "team": entities of four slices of 3 000 samples whose members all sit exactly on the <8> arena, and the same with one more
    entry in member 0 and in member 3. The bytes depend on the weights and, through S, on the intercept: a batch per (has_w, ic).
    last: the name of the entity to move to the end of the batch."""
    out = {}
    w = "w" if has_w else "u"

    def three(tag, v, d, target, n, wants):
        z = _exact_shape(v, d, d + ic, has_w, n, target)
        for (kind, nn, zz), want in zip((("exact", n, z), ("entry", n, z + 1), ("sample", n + 1, z)), wants):
            name = f"arena-{tag}-{w}{ic}-{kind}"
            out[name] = _entity(name, lens_total(name, nn, zz), F=d, want=want, tags=("arena", tag, kind))
    if variant == "one":
        three("leanroute", "lean", F, TALL_LEAN_ARENA, ARENA_N["lean"], ("lean", "one", "one"))
        three("leanarena", "lean", F, arena("lean"), ARENA_N["lean"], ("one",) * 3)
        three("one", "one", F, arena("one"), ARENA_N["one"], ("one",) * 3)
    elif variant in ("mid", "large"):
        three(f"{variant}-S32", variant, F, arena(variant), ARENA_N[variant], (variant,) * 3)
        three(f"{variant}-S16", variant, 33 - ic, arena(variant), ARENA_N[variant], (variant,) * 3)
    else:
        for tag, d in (("team-S32", F), ("team-S16", 33 - ic)):
            z = _exact_shape("team", d, d + ic, has_w, ARENA_N["large"], arena("team"))
            for kind, bump in (("exact", None), ("entry0", 0), ("entry3", 3)):
                name = f"arena-{tag}-{w}{ic}-{kind}"
                parts = [lens_total(f"{name}-{m}", ARENA_N["large"], z + (1 if bump == m else 0)) for m in range(TALL_TEAM_C)]
                out[name] = _entity(name, np.concatenate(parts), F=d, want="team", tags=("arena", tag, kind))
    if last is not None:
        out[last] = out.pop(last)
    return out


ARENA_LAST = "arena-one-{w}{ic}-entry"      # just above the <1> arena: streamed; at the end of the batch its last windows read the tail
WIDTH_N = {"lean": 100, "mid": 280, "large": 400, "team": 700}      # under ROUTING["ladder"]


def widths(ic):
    """p = 32, 33 and 64 on <4>, <8> and a team (d = p - ic: p = 64 is d = 64 without an intercept and d = 63 with one), p = 65 (leaves the
    tall classes), an entity that but for its first six samples uses only column d - 1 (one entry per sample: on the lean class, <8> and a
    team), and with an intercept d = 0 (p = 1: no sample has an entry) on the same three."""
    out = {}
    for v in ("mid", "large", "team"):
        for p in (32, 33, 64):
            name = f"widths-{v}-p{p}-ic{ic}"
            out[name] = _entity(name, lens_between(name, WIDTH_N[v], 3, 8), F=p - ic, want=v, tags=("width", p))
    name = f"widths-p65-ic{ic}"
    out[name] = _entity(name, lens_between(name, WIDTH_N["large"], 3, 8), F=65 - ic, want=None, tags=("width", 65))
    for v in ("lean", "large", "team"):
        name = f"widths-{v}-lastcol"
        out[name] = _entity(name, np.concatenate([np.full(F // 4, 4), np.ones(WIDTH_N[v] - F // 4, np.int64)]), rule="lastcol", want=v, tags=("lastcol",))
    if ic:
        for v in ("lean", "large", "team"):
            name = f"widths-{v}-d0"
            out[name] = _entity(name, np.zeros(WIDTH_N[v], np.int64), want=v, tags=("d0",))
    return out


STRUCTURES = ("empties", "tail3", "dup-w4", "dup-w8", "dup-w0", "same9")
STRUCT_N = {("one", "resident"): 300, ("one", "streamed"): 640, ("large", "resident"): 1500, ("large", "streamed"): 5200}


def _struct_lens(kind, name, n):
    if kind == "empties":      # empty first, last and every other sample; the others long, so that the entity keeps its class
        lens = lens_between(name, n, 5, 8)
        lens[0::2] = 0
        lens[n - 1] = 0
        return lens
    if kind == "tail3":
        return lens_between(name, n, 3, 4, [(n - 4, 3), (n - 3, 0), (n - 2, 0), (n - 1, 0)])      # (three entries: the last sample WITH entries has a window past the arrays too)
    if kind == "dup-w4":
        return lens_between(name, n, 3, 4)
    if kind == "dup-w8":
        return lens_between(name, n, 5, 8)
    return lens_between(name, n, 3, 4, [(n // 2 - n // 2 % 3, 9), (n - 1 - (n - 1) % 3, 9)])      # dup-w0, same9: two samples of nine (at indices the dup rule takes)


def structures(variant):
    """Every structure once resident and once streamed on the variant ("one" or "large"): samples without entries (first, last and every
    other; the last three), a column twice in a sample (first and last entry) in each width class, a sample that is one column nine
    times. The streamed `tail3` is the batch's last entity: its last windows start at the very end of the batch's arrays."""
    out = {}
    for home in ("resident", "streamed"):
        n = STRUCT_N[(variant, home)]
        for kind in STRUCTURES:
            name = f"struct-{variant}-{home}-{kind}"
            rule = "dup" if kind.startswith("dup") else ("same" if kind == "same9" else "perm")
            nn = n // 2 if (kind == "dup-w8" and home == "resident") else n      # (samples of 5 - 8 entries: half as many fit the arena)
            out[name] = _entity(name, _struct_lens(kind, name, nn), rule=rule, want=variant, tags=("struct", kind, home))
    last = f"struct-{variant}-streamed-tail3"
    out[last] = out.pop(last)
    return out


POSITIONS = ("first", "middle", "last")
POSITION_ROUTING = dict(tall_min_n=1, tall_team_n=0, tall_split_n=2000, tall_mid_n=0)


def positions(which, place):
    """One streamed entity of <1> (which = "one", 640 samples) or <8> ("large", 5 200) whose last sample has a single entry, first, in the
    middle or last among two lean fillers: otherwise identical batches."""
    n = STRUCT_N[(which, "streamed")]
    x = _entity(f"pos-{which}", lens_between(f"pos-{which}", n, 3, 4, [(n - 1, 1)]), want=which, tags=("position",))
    a, b = (_entity(f"pos-filler{k}", lens_between(f"pos-filler{k}", 40 + k, 1, 3), want="lean") for k in (0, 1))
    order = {"first": [x, a, b], "middle": [a, x, b], "last": [a, b, x]}[place]
    return {e["name"]: e for e in order}


TEAM_MIXED = {"rrrs": (10401, "rrrs"), "sssr": (10402, "sssr"), "ssss": (10403, "ssss"), "rrrr": (10400, "rrrr")}


def team_mixed():
    """Teams whose members differ: members 0 - 2 resident and member 3 streamed, the reverse, all streamed, all resident; n mod 4 = 1, 2, 3,
    0; every slice of about 2 600 samples (three trips of 1 024). A resident slice has samples of 1 - 3 entries, a streamed one of 4 (at
    24 features a slice is resident up to 52 800 + 8 nnz + 16 n <= 158 288 with weights). And n = 64 and n = 63 under tall_team_n = -1,
    which is clamped to 64: the first is on a team, the second on <8>. `ssss` ends the batch; every entity's last sample has one entry,
    so that the last member's last window runs past the batch's arrays when it is streamed."""
    out = {}
    for n in (64, 63):
        name = f"team-n{n}"
        out[name] = _entity(name, lens_between(name, n, 3, 4), want="team" if n == 64 else "large", tags=("clamp", n))
    for key in ("rrrs", "sssr", "rrrr", "ssss"):
        n, homes = TEAM_MIXED[key]
        name = f"team-{key}"
        parts = [lens_between(f"{name}-{m}", i1 - i0, *((1, 3) if homes[m] == "r" else (4, 4))) for m, (i0, i1) in enumerate(team_slices(n)[1])]
        lens = np.concatenate(parts)
        lens[-1] = 1      # (a last sample of four entries ends exactly at the end of the arrays: its window is safe)
        out[name] = _entity(name, lens, want="team", tags=("mixed", homes))
    return out


# (batch name -> routing, builder); has_w and ic reach the builders that depend on them
def batch_entities(batch, has_w=True, ic=1):
    kind, _, arg = batch.partition(":")
    if kind == "trips":
        return trips(arg)
    if kind == "arena":
        return arena_batch(arg, has_w, ic, last=ARENA_LAST.format(w="w" if has_w else "u", ic=ic) if arg == "one" else None)
    if kind == "widths":
        return widths(ic)
    if kind == "structures":
        return structures(arg)
    if kind == "positions":
        which, place = arg.split(",")
        return positions(which, place)
    if kind == "team_mixed":
        return team_mixed()
    raise KeyError(batch)


def batch_routing(batch):
    kind, _, arg = batch.partition(":")
    if kind in ("trips", "arena", "structures"):
        return ROUTING[arg]
    return {"widths": ROUTING["ladder"], "positions": POSITION_ROUTING, "team_mixed": ROUTING["team"]}[kind]


BATCHES = ([f"trips:{v}" for v in SOLO] + [f"arena:{v}" for v in ("one", "mid", "large", "team")] + ["widths", "structures:one", "structures:large"] +
           [f"positions:{w},{p}" for w in ("one", "large") for p in POSITIONS] + ["team_mixed"])


def cases_of(batch):
    """(loss, has_w, ic) the GPU file runs a batch with: `trips` the full cross; the others the three losses with weights and intercept,
    logistic also without each."""
    if batch.startswith("trips"):
        return [(loss, w, ic) for loss in LOSSES for w in (True, False) for ic in (1, 0)]
    return [(loss, True, 1) for loss in LOSSES] + [("logistic", False, 1), ("logistic", True, 0)]


# ---- cases and references: built once, left unchanged -------------------------------------------------------------------------------------
_CASES, _REFS = {}, {}


def case(batch, loss, has_w, ic, reverse=False):
    """-> dict(name, b, kw, loss, ic, has_w, entities [in batch order], names, placed, routing)."""
    key = (batch, loss, bool(has_w), int(ic), bool(reverse))
    if key not in _CASES:
        ents = list(batch_entities(batch, has_w, ic).values())
        if reverse:
            ents = ents[::-1]
        _CASES[key] = dict(name="tall_edges-" + "-".join(str(k) for k in key), b=assemble(ents, loss, has_w), kw=batch_kw(batch, ic), loss=loss,
                           ic=int(ic), has_w=bool(has_w), entities=ents, names=[e["name"] for e in ents], placed=placed(ents), routing=batch_routing(batch))
    return _CASES[key]


def routed(c):
    """route_tall of every entity of the case -> [E] classes (NOT_TALL where it leaves them)."""
    return np.array([route_tall(e["d"] + c["ic"], int(e["lens"].size), int(e["lens"].sum()), c["kw"]["m"], c["has_w"], c["routing"], c["ic"])
                     for e in c["entities"]])


def reference(c):
    """The reference's own run of a case, computed once -> dict(pk, coef_ptr, ref, strict [E] bool, nit [E]). logistic and squared:
    oracle.solve, strict by re_linear_helpers.oracle_strict; Poisson: scipy by re_poisson_helpers.reference, strict as it says and no
    FACTR stop."""
    name = c["name"]
    if name in _REFS:
        return _REFS[name]
    b, kw = c["b"], c["kw"]
    pk = oracle.pack(b.ent_row_ptr, b.row_nnz_ptr, b.col_global)
    cp = pk["ent_feat_ptr"] + np.arange(b.E + 1) * c["ic"]
    if c["loss"] == "poisson":
        ref = ph.reference(b, pk, kw, None, cp, key=("tall_edges", name), entities=np.arange(b.E))
        strict, nit = ref["strict"] & (ref["status"] != 1), ref["nit"]
    else:
        okw = dict(kw, variance_mode=0, linear=c["loss"] == "squared", sum_loss=False)
        ref, strict, _, _ = lh.oracle_strict(b, pk, oracle.make_opts(**okw), None, int(cp[-1]))
        nit = ref["nit"]
    _REFS[name] = dict(pk=pk, coef_ptr=cp, ref=ref, strict=np.asarray(strict), nit=np.asarray(nit))
    return _REFS[name]


def entity_dense(b, pk, e, ic):
    """Entity e as a dense fp64 matrix [n, d + ic] from the PACKED arrays (pk: row_ptr, csr_col in local indices), intercept first; the
    repeated entries of a cell are summed (np.add.at), as the reference's toarray() does. -> (X~, offset, w)."""
    r0, r1 = int(b.ent_row_ptr[e]), int(b.ent_row_ptr[e + 1])
    z0, z1 = int(pk["ent_nnz_ptr"][e]), int(pk["ent_nnz_ptr"][e + 1])
    n, d = r1 - r0, int(pk["ent_feat_ptr"][e + 1] - pk["ent_feat_ptr"][e])
    rp = pk["row_ptr"][r0 + e:r1 + e + 1].astype(np.int64)      # (entity-relative, n + 1 of them)
    assert rp[0] == 0 and rp[-1] == z1 - z0
    X = np.zeros((n, d + ic))
    if ic:
        X[:, 0] = 1.0
    np.add.at(X, (np.repeat(np.arange(n), np.diff(rp)), ic + pk["csr_col"][z0:z1].astype(np.int64)), b.val[z0:z1].astype(np.float64))
    w = np.ones(n) if b.weight is None else b.weight[r0:r1].astype(np.float64)
    return X, b.offset[r0:r1].astype(np.float64), w


def variance_dense(b, pk, kw, loss, theta, coef_ptr, entities=None):
    """_compute_variance SIMPLE per entity at theta ([P], the device's), from entity_dense — the repeated entries of a cell summed BEFORE
    squaring: 1 / (sum_i D_i X~_ij^2 + l2 [not for an unregularised intercept] + 1e-12), D_i = w rho (1 - rho) | 2 w | w exp(z).
    -> [P] (zeros outside `entities`)."""
    out = np.zeros(int(coef_ptr[-1]))
    for e in (range(b.E) if entities is None else entities):
        X, off, w = entity_dense(b, pk, e, 1 if kw["has_intercept"] else 0)
        s = slice(int(coef_ptr[e]), int(coef_ptr[e + 1]))
        z = X @ theta[s] + off
        if loss == "squared":
            D = 2.0 * w
        elif loss == "poisson":
            D = w * np.exp(z)
        else:
            rho = 1.0 / (1.0 + np.exp(-z))
            D = w * rho * (1.0 - rho)
        out[s] = 1.0 / ((X * X * D[:, None]).sum(0) + lh.reg_vector(X.shape[1], kw["l2"], kw["has_intercept"], kw["regularize_bias"]) + 1e-12)
    return out


def has_duplicates(e):
    """A sample of the entity holds a column twice."""
    row_of = np.repeat(np.arange(e["lens"].size), e["lens"])
    return np.unique(row_of * (e["F"] + 1) + e["col"]).size < e["col"].size
