"""Shared by tests/test_team_edges.py (CPU) and tests/test_gpu_team_edges.py (GPU): entities built to sit ON the constants the team
kernels branch on (re_solve_team_kernel<NW, GRID>, csrc/re_solve_team.hpp: the classes "workgroup", "128 teams", "32 teams", "8 teams"
and "device-wide"), the tests' own statement of what team_fg's column pass does with an entity (column_pass_plan), and of the rules of
re_classify_kernel above the group and wavefront classes (route_large; class_caps_helpers.route is the rule below them).

The four constants are literals ON PURPOSE: one changed in the library and not here fails test_the_constants_are_the_librarys, and
the shapes of edge_entities() are then moved to the new value (tests/test_team_edges.py says which situations they must still show).
Nothing new is compared here: narrow_helpers.compare_with_oracle, re_linear_helpers.judge / oracle_strict and re_poisson_helpers.reference
/ compare / variance_numpy are the rules."""
import numpy as np

import class_caps_helpers as ch
import re_linear_helpers as lh
import re_poisson_helpers as ph
from gdmix_amd import synthetic
from gdmix_amd.batch import RawBatch
from oracle import oracle

WAVE = 64
TEAM_SHORT_COL = 16      # a tile whose non-split columns all have at most this many entries: one lane per column
TEAM_CHUNK = 512         # entries of a tile's CSC run per chunk
TEAM_LONGC = 2048        # a column of at least this many entries is split into 64 slices over the team
TEAM_LONG_CAP = 256      # more such columns in an entity: none is split
CONSTANTS = dict(TEAM_SHORT_COL=TEAM_SHORT_COL, TEAM_CHUNK=TEAM_CHUNK, TEAM_LONGC=TEAM_LONGC, TEAM_LONG_CAP=TEAM_LONG_CAP)

TEAM_NAMES = ["re_solve_team_kernel workgroup", "re_solve_team_kernel 128 teams", "re_solve_team_kernel 32 teams",
              "re_solve_team_kernel 8 teams", "re_solve_team_kernel device-wide"]
BLOCK_CLASS, TEAM128_CLASS, TEAM32_CLASS, TEAM8_CLASS, GIANT_CLASS = 35, 36, 37, 38, 39
TEAM_TIERS = (TEAM128_CLASS, TEAM32_CLASS, TEAM8_CLASS)
TALL_ANY = -1            # route_large: one of the tall classes; which one is decided per batch (class_base_kernel: the tall tests' subject)
TEAM_NNZ_DEFAULT, GIANT_NNZ_DEFAULT = 16384, 16777216

D = 8192
FILLERS = 256            # entities of one sample and one non-zero: the batch then has at least 128 scratch slots (slots_for: never more than entities)
LOSSES = ch.LOSSES
KW = dict(l2=10.0, regularize_bias=False, m=10, max_iter=100, ftol=1e-12)
SEED = 5                 # every edge entity is strict by the reference alone for the three losses, with and without an intercept (tests/test_team_edges.py)


# ---- generators ---------------------------------------------------------------------------------------------------------------------
def entity_by_columns(rng, n, col_lens, D):
    """An entity of n samples whose k-th feature, in ascending global index, has exactly col_lens[k] entries, in distinct random rows
    (rows may end up empty). -> (row_nnz [n], col_global [nnz] row by row, val [nnz] fp32 ~ N(0, 1) / 4)."""
    col_lens = np.asarray(col_lens, np.int64)
    assert col_lens.size <= D and col_lens.min() >= 1 and col_lens.max() <= n
    feats = np.sort(rng.choice(D, size=col_lens.size, replace=False))
    rows = np.concatenate([rng.choice(n, size=int(k), replace=False) for k in col_lens])
    cols = np.repeat(feats, col_lens)
    order = np.lexsort((cols, rows))
    val = (rng.standard_normal(rows.size) / 4.0).astype(np.float32)
    return np.bincount(rows, minlength=n).astype(np.int64), cols[order].astype(np.int64), val


def entity_by_rows(rng, d, row_lens, D):
    """An entity over d features whose row i has exactly row_lens[i] entries in distinct random columns, and one last row that touches
    all d columns (so that every feature occurs). -> as entity_by_columns."""
    row_lens = np.asarray(row_lens, np.int64)
    assert d <= D and row_lens.max() <= d
    feats = np.sort(rng.choice(D, size=d, replace=False))
    cols = np.concatenate([feats[rng.choice(d, size=int(k), replace=False)] for k in row_lens] + [feats])
    val = (rng.standard_normal(cols.size) / 4.0).astype(np.float32)
    return np.concatenate([row_lens, [d]]).astype(np.int64), cols.astype(np.int64), val


def short(k):
    """k column lengths: 1, 7, 8, 9, 15, 16 cycled (gather_dot8's batch of eight and TEAM_SHORT_COL from both sides)."""
    return [(1, 7, 8, 9, 15, 16)[i % 6] for i in range(k)]


ROW_LENS = [0, 1, 7, 8, 9, 15, 16, 17, 63, 64, 65, 0, 299] * 5


def edge_entities():
    """[(name, kind, n or d, lengths)]: the table of the module's entities. Column lists are in coefficient order after the intercept;
    without an intercept they shift by one lane, which is wanted."""
    mixed = (short(63) + [16] * 63 + [17] + short(30) + [2047] + short(33) + short(10) + [2048] + short(53) +
             [2049, 600] + short(20) + [513] + short(41) + list(range(2048, 2057)) + short(55) + [3, 2050, 40, 16, 1])
    return [("mixed", "columns", 2100, mixed),
            ("cap256", "columns", 2100, [2048] * 256 + short(20)),
            ("cap257", "columns", 2100, [2048] * 257 + short(20)),
            ("one_col", "columns", 2049, [2049]),
            ("four_col", "columns", 2048, [2048, 2047, 16, 17]),
            ("wide1101", "columns", 64, short(1100)),
            ("wide1025", "columns", 64, short(1024)),
            ("wide513", "columns", 64, short(512)),
            ("rows", "rows", 300, ROW_LENS)]


EDGE_NAMES = [e[0] for e in edge_entities()]
N_EDGE = len(EDGE_NAMES)


def make_edge_batch(seed=SEED):
    """The edge entities followed by FILLERS one-sample entities. Values N(0, 1) / 4 fp32, offsets N(0, 1), y ~ Bernoulli(sigmoid(x . w*
    + offset)) with a hidden global w* (as narrow_helpers.make_shaped_batch), sample weights in [0.25, 2.25)."""
    rng = np.random.default_rng(seed)
    w_star = 0.5 * rng.standard_normal(D)
    parts = []
    for _, kind, size, lens in edge_entities():
        parts.append(entity_by_columns(rng, size, lens, D) if kind == "columns" else entity_by_rows(rng, size, lens, D))
    parts += [entity_by_columns(rng, 1, [1], D) for _ in range(FILLERS)]
    ent_n = np.array([p[0].size for p in parts], np.int64)
    row_nnz = np.concatenate([p[0] for p in parts])
    col = np.concatenate([p[1] for p in parts])
    val = np.concatenate([p[2] for p in parts])
    N = int(ent_n.sum())
    offset = rng.standard_normal(N).astype(np.float32)
    row_of = np.repeat(np.arange(N), row_nnz)
    logit = np.bincount(row_of, weights=val.astype(np.float64) * w_star[col], minlength=N) + offset      # (empty rows: the offset alone)
    y = (rng.random(N) < 1.0 / (1.0 + np.exp(-logit))).astype(np.float32)
    weight = (0.25 + 2.0 * rng.random(N)).astype(np.float32)
    names = EDGE_NAMES + [f"filler{i}" for i in range(FILLERS)]
    return RawBatch(ent_row_ptr=np.concatenate([[0], np.cumsum(ent_n)]), row_nnz_ptr=np.concatenate([[0], np.cumsum(row_nnz)]), col_global=col,
                    val=val, y=y, offset=offset, weight=weight, uid=np.arange(N, dtype=np.int64), entity_ids=names)


def entity_col_ptr(b, e):
    """The CSC column pointer of entity e in local index space (features in ascending global index), from the raw batch."""
    z0, z1 = int(b.row_nnz_ptr[b.ent_row_ptr[e]]), int(b.row_nnz_ptr[b.ent_row_ptr[e + 1]])
    _, counts = np.unique(b.col_global[z0:z1], return_counts=True)
    return np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)


# ---- what team_fg does with an entity ----------------------------------------------------------------------------------------------------
def column_pass_plan(col_ptr, ic, n_long_cap=TEAM_LONG_CAP):
    """The column pass of an entity with CSC pointer col_ptr [d + 1] and ic intercept coefficients (0 or 1), from the header comment of
    csrc/re_solve_team.hpp: coefficients go by tiles of 64 (the intercept, which has no column, is lane 0 of tile 0).
    -> dict(split: the ascending list of the columns of at least TEAM_LONGC entries, empty when there are more than n_long_cap;
            tiles: per tile dict(path "lane" | "chunked", lens [of its non-split columns], split_lens [of its split columns], n_split,
                                 first_is_split, chunks [dict(owners, masked)] of a chunked tile)).
    A tile is lane-per-column when none of its non-split columns has more than TEAM_SHORT_COL entries. Otherwise its contiguous CSC run,
    from the first feature lane's col_ptr to the last one's end, is cut into chunks of TEAM_CHUNK entries; a chunk has `owners` non-split
    columns with entries in it (0: it lies inside split columns and is skipped) and is `masked` when it also holds entries of a split
    column, which are left out of the owners' sums."""
    col_ptr = np.asarray(col_ptr, np.int64)
    lens = np.diff(col_ptr)
    d = lens.size
    long_cols = np.flatnonzero(lens >= TEAM_LONGC)
    split = long_cols.tolist() if long_cols.size <= n_long_cap else []
    is_split = np.zeros(d, bool)
    is_split[split] = True
    tiles = []
    for j0 in range(0, d + ic, WAVE):
        c0, c1 = max(j0 - ic, 0), min(j0 + WAVE, d + ic) - ic      # the tile's features [c0, c1)
        mine = np.arange(c0, c1)
        flat = mine[~is_split[mine]]
        tile = dict(lens=lens[flat].tolist(), split_lens=lens[mine[is_split[mine]]].tolist(), n_split=int(is_split[mine].sum()),
                    first_is_split=bool(mine.size and is_split[c0]), chunks=[])
        tile["path"] = "lane" if (flat.size == 0 or lens[flat].max() <= TEAM_SHORT_COL) else "chunked"
        if tile["path"] == "chunked":
            for s0 in range(int(col_ptr[c0]), int(col_ptr[c1]), TEAM_CHUNK):
                s1 = min(s0 + TEAM_CHUNK, int(col_ptr[c1]))
                inside = (np.minimum(col_ptr[mine + 1], s1) - np.maximum(col_ptr[mine], s0)) > 0
                tile["chunks"].append(dict(owners=int((inside & ~is_split[mine]).sum()), masked=bool((inside & is_split[mine]).any())))
        tiles.append(tile)
    return dict(split=split, n_long=int(long_cols.size), tiles=tiles)


# ---- the routing rules above the group and wavefront classes ---------------------------------------------------------------------------
def route_large(p, n, nnz, m, has_w, tall_min_n, team_nnz=TEAM_NNZ_DEFAULT, giant_nnz=GIANT_NNZ_DEFAULT, ic=1):
    """The class of an entity by the rules of re_classify_kernel (csrc/re_route.hip), in this order: the tall rule (tall_min_n > 0, p <= 64,
    n >= tall_min_n, m <= 10) wins unless the entity is device-wide; device-wide for giant_nnz > 0 and nnz >= giant_nnz; the team tier for
    team_nnz > 0 and nnz >= team_nnz — 8 teams from 128 x team_nnz, 32 teams from 8 x team_nnz, 128 teams below —, also for an entity a
    group class would hold; otherwise class_caps_helpers.route. More than ten history pairs: both thresholds are off. A tall entity of 512
    samples and more is TALL_ANY (route does not speak for those: the batch decides between the tall classes)."""
    if m > ch.M_REG:
        team_nnz = giant_nnz = 0
    giant = giant_nnz > 0 and nnz >= giant_nnz
    if tall_min_n > 0 and m <= ch.M_REG and p <= ch.TALL_MAX_P and n >= tall_min_n and not giant:
        return TALL_ANY if n >= 512 else ch.route(p, n, nnz, m, has_w, tall_min_n, ic=ic, team_nnz=nnz + 1)
    if giant:
        return GIANT_CLASS
    if team_nnz > 0 and nnz >= team_nnz:
        return TEAM8_CLASS if nnz >= 128 * team_nnz else (TEAM32_CLASS if nnz >= 8 * team_nnz else TEAM128_CLASS)
    return ch.route(p, n, nnz, m, has_w, tall_min_n, ic=ic, team_nnz=nnz + 1)


# ---- cases and references: built once, left unchanged -------------------------------------------------------------------------------------
_BATCH = {}


def edge_batch(loss):
    if "logistic" not in _BATCH:
        _BATCH["logistic"] = make_edge_batch()
    if loss not in _BATCH:
        _BATCH[loss] = ch._with_labels(_BATCH["logistic"], loss, SEED)
    return _BATCH[loss]


_PK = {}


def _pack(key, b):
    if key not in _PK:
        _PK[key] = oracle.pack(b.ent_row_ptr, b.row_nnz_ptr, b.col_global)
    return _PK[key]


def case(loss, ic):
    """The edge batch with the loss's labels and the options of the module -> dict(name, b, kw, loss, ic, edge [indices of the edge entities])."""
    return dict(name=f"team_edges-{loss}-{ic}", b=edge_batch(loss), kw=dict(KW, has_intercept=bool(ic)), loss=loss, ic=ic, edge=np.arange(N_EDGE))


# entities of stated (p, n, nnz) for the tier thresholds (narrow_helpers.make_shaped_batch; cells repeat at these counts, which the pack keeps)
TIER_TEAM_NNZ, TIER_GIANT_NNZ, TIER_TALL_MIN_N = 64, 20000, 32
TIER_SHAPES = {
    "scaled": [(41, 60, z) for z in (63, 64, 511, 512, 8191, 8192, 19999, 20000)] + [(30, 40, 100), (30, 40, 20000)],
    "defaults": [(81, 60, z) for z in (16383, 16384, 131071, 131072)]}


def tier_case(which):
    shapes = TIER_SHAPES[which]
    if ("tier", which) not in _BATCH:
        _BATCH[("tier", which)] = ch.shaped_batch(shapes, SEED, random_weights=True)
    return dict(name=f"team_tiers-{which}", shapes=shapes, b=_BATCH[("tier", which)], kw=dict(KW, has_intercept=True), loss="logistic", ic=1,
                edge=np.arange(len(shapes)), pack_key=("tier", which))


_REFS = {}


def reference(c):
    """The reference's own run of a case, computed once -> dict(pk, coef_ptr, ref, strict [E] bool, nit [E]). logistic (SIMPLE variance
    on: the oracle's variance is the logistic one) and squared: oracle.solve, strict by re_linear_helpers.oracle_strict; Poisson: scipy by
    re_poisson_helpers.reference, strict as it says and no FACTR stop."""
    name = c["name"]
    if name in _REFS:
        return _REFS[name]
    b, kw = c["b"], c["kw"]
    pk = _pack(c.get("pack_key", "edges"), b)      # (the pack does not depend on the labels or the intercept)
    cp = pk["ent_feat_ptr"] + np.arange(b.E + 1) * c["ic"]
    if c["loss"] == "poisson":
        # A filler whose one label is 0 has no minimiser under an unregularised intercept (re_poisson_helpers: f -> 0 as the intercept
        # -> -inf), yet scipy reproduces its own stop there, so the rule would compare f ~ 4e-6 at rtol 1e-9 where f moves with theta in
        # first order: a group class gave 4.124876349e-06 against scipy's 4.124876354e-06 on an MI355X. They are left out of the
        # Poisson comparison (never an edge entity: those are all compared).
        y = b.y[b.ent_row_ptr[:-1]]      # (entities of several samples: only the edge entities, kept whatever this is)
        keep = (np.arange(b.E) < len(c["edge"])) | (y > 0) | (c["ic"] == 0)
        ref = ph.reference(b, pk, kw, None, cp, key=("team_edges", name), entities=np.flatnonzero(keep))
        strict, nit = np.zeros(b.E, bool), np.zeros(b.E, np.int64)
        strict[ref["entities"]], nit[ref["entities"]] = ref["strict"] & (ref["status"] != 1), ref["nit"]
    else:
        okw = dict(kw, variance_mode=0, linear=True, sum_loss=False) if c["loss"] == "squared" else dict(kw, variance_mode=1)
        ref, strict, _, _ = lh.oracle_strict(b, pk, oracle.make_opts(**okw), None, int(cp[-1]))
        nit = ref["nit"]
    _REFS[name] = dict(pk=pk, coef_ptr=cp, ref=ref, strict=np.asarray(strict), nit=np.asarray(nit))
    return _REFS[name]
