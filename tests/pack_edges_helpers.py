"""Shared by tests/test_pack_edges.py (CPU) and tests/test_gpu_pack_edges.py (GPU): the tests' own statement of how the pack
(csrc/re_pack.hip, csrc/re_pack_big.hip) routes an entity — its tier by max(samples, non-zeros), its path inside a wavefront tier by
its non-zero count and its columns, the path of the device-wide tier by the largest column among its entities —, batches whose entities
sit ON those constants and one to either side of them, batches large enough for a wavefront of every tier to walk several entities, a
batch with more big entities than one tile of big_head_kernel, and the arrays a pack must produce, bit for bit, from oracle.pack and one
lexsort.

The constants and the wavefronts a tier's grid holds per CU are literals ON PURPOSE: a constant or a grid changed in the library and not
here fails test_gpu_pack_edges.test_the_constants_are_the_librarys; changed here, tests/test_pack_edges.py names the (tier, path) pairs
and edge values the shapes below no longer show."""
import numpy as np

from gdmix_amd.batch import RawBatch
from oracle import oracle

WAVE = 64
# csrc/re_pack.hip
PACK_WAVES = 4                  # wavefronts per workgroup of the first tier
GDMIX_PACK_LDS_KEYS = 256       # the first tier's capacity (samples and non-zeros)
PACK_CAP2, PACK_CAP3 = 512, 1024
PACK_RANK_MAX = 128             # at most this many non-zeros: bitmap or rank sort; more: count or bitonic
PACK_COUNT_COLS = 64
PACK_BITMAP_COLS = 2048
PACK_PF = 4                     # 64-entry tiles of an entity requested one trip ahead
# csrc/re_pack_big.hip
BIG_CH = 1024
BIG_COUNT_CBITS = 11
BIG_HEAD_MAX = 1 << 16
CONSTANTS = {"re_pack.hip": dict(PACK_WAVES=PACK_WAVES, PACK_CAP2=PACK_CAP2, PACK_CAP3=PACK_CAP3, PACK_RANK_MAX=PACK_RANK_MAX,
                                 PACK_COUNT_COLS=PACK_COUNT_COLS, PACK_BITMAP_COLS=PACK_BITMAP_COLS, PACK_PF=PACK_PF),
             "re_pack_big.hip": dict(BIG_CH=BIG_CH, BIG_COUNT_CBITS=BIG_COUNT_CBITS, BIG_HEAD_MAX=BIG_HEAD_MAX)}
# The wavefronts per CU of a tier's grid (pack_impl): num_cus x occupancy workgroups of PACK_WAVES wavefronts — at most the hardware's 32
# wavefronts per CU, which is what the batches are sized for, so that they do not depend on the occupancy query —, num_cus x 4 workgroups
# of 4, num_cus x 4 workgroups of 2. The lines of pack_impl this was read from, with blanks squeezed:
TIER_WAVES_PER_CU = (32, 16, 8)
GRID_LINES = ("if (eblocks > ctx->num_cus * pack_occupancy) eblocks = ctx->num_cus * pack_occupancy;",
              "hipLaunchKernelGGL((pack_entity_kernel<PACK_LDS_KEYS, PACK_WAVES>), dim3(eblocks), dim3(WAVE * PACK_WAVES), 0, s,",
              "hipLaunchKernelGGL((pack_entity_kernel<PACK_CAP2, 4>), dim3(ctx->num_cus * 4), dim3(WAVE * 4), 0, s2,",
              "hipLaunchKernelGGL((pack_entity_kernel<PACK_CAP3, 2>), dim3(ctx->num_cus * 4), dim3(WAVE * 2), 0, s3,")

TIERS = (1, 2, 3, 4)            # 4: the device-wide tier ("big")
BIG = 4
WAVE_PATHS = ("bitmap", "rank", "count", "bitonic")
BIG_PATHS = ("counting", "sort")
SPACES = (20, 64, 65, 2048, 2049, 2 ** 31)
N_LIST = (1, 63, 64, 65, 128, 255, 256, 257, 511, 512, 513, 1023, 1024, 1025)
NNZ_LIST = (0, 1, 63, 64, 65, 127, 128, 129, 191, 192, 193, 255, 256, 257, 511, 512, 513, 1023, 1024, 1025, 2047, 2048, 2049, 3073)
ROW_KINDS = ("first", "last", "alternate", "one_each", "spread")
MAX_TRIPS_NNZ = 10_000_000


def tier_of(n, nnz):
    mx = max(int(n), int(nnz))
    return 1 if mx <= GDMIX_PACK_LDS_KEYS else (2 if mx <= PACK_CAP2 else (3 if mx <= PACK_CAP3 else BIG))


def plan(n, nnz, cols, bitmap_on=True):
    """(tier, path) of an entity of n samples whose nnz non-zeros have the global columns `cols`, by the library's rules restated. The
    path of a big entity is a property of its batch (big_path): None here."""
    tier = tier_of(n, nnz)
    if tier == BIG:
        return tier, None
    top = int(np.max(cols)) if nnz else -1
    if nnz <= PACK_RANK_MAX:
        return tier, "bitmap" if (bitmap_on and top < PACK_BITMAP_COLS) else "rank"
    return tier, "count" if top < PACK_COUNT_COLS else "bitonic"


def _ent_max_col(b):
    """[E] the largest column of every entity, -1 where it has none."""
    znp = b.row_nnz_ptr[b.ent_row_ptr]
    some = np.diff(znp) > 0
    top = np.full(b.E, -1, np.int64)
    if some.any():
        top[some] = np.maximum.reduceat(b.col_global, znp[:-1][some])
    return top


def batch_plan(b, bitmap_on=True):
    """plan() for every entity of a batch at once -> (tier [E] int, path [E] str, '' for the big ones)."""
    n, nnz, top = b.ent_n(), b.ent_nnz(), _ent_max_col(b)
    mx = np.maximum(n, nnz)
    tier = np.where(mx <= GDMIX_PACK_LDS_KEYS, 1, np.where(mx <= PACK_CAP2, 2, np.where(mx <= PACK_CAP3, 3, BIG)))
    small = np.where(bitmap_on & (top < PACK_BITMAP_COLS), "bitmap", "rank")
    large = np.where(top < PACK_COUNT_COLS, "count", "bitonic")
    path = np.where(tier == BIG, "", np.where(nnz <= PACK_RANK_MAX, small, large))
    return tier, path


def big_path(b, big_count_on=True):
    """The path of the batch's big entities: counting when the largest column among them is below 2^BIG_COUNT_CBITS and
    GDMIX_PACK_BIG_COUNT is not 0, else the radix sort; None without big entities."""
    tier, _ = batch_plan(b)
    if not (tier == BIG).any():
        return None
    top = int(_ent_max_col(b)[tier == BIG].max())
    return "counting" if (big_count_on and top < (1 << BIG_COUNT_CBITS)) else "sort"


# ---- what a pack must produce --------------------------------------------------------------------------------------------------------
def expected(b, has_intercept=True):
    """Every array tests/test_gpu_parity.py::_check_pack compares, for the whole batch at once, and the three maxima: oracle.pack's
    arrays; the CSC copy by ONE lexsort over (entity, local column, position); col_ptr [Z + E] with the d_e + 1 entries of entity e at
    ent_nnz_ptr[e] + e (col_ptr_defined marks them: the pack leaves the rest of an entity's nnz_e + 1 slots unwritten)."""
    pk = oracle.pack(b.ent_row_ptr, b.row_nnz_ptr, b.col_global)
    E, N, Z, D = b.E, b.N, b.Z, pk["D"]
    znp, fp = pk["ent_nnz_ptr"], pk["ent_feat_ptr"]
    nnz_e, d_e, ents = np.diff(znp), np.diff(fp), np.arange(E, dtype=np.int64)
    ent_of_nz = np.repeat(ents, nnz_e)
    local_row = np.repeat(np.arange(N, dtype=np.int64), np.diff(b.row_nnz_ptr)) - b.ent_row_ptr[ent_of_nz]
    order = np.lexsort((np.arange(Z), pk["csr_col"], ent_of_nz))
    before = np.concatenate([[0], np.cumsum(np.bincount(fp[ent_of_nz] + pk["csr_col"], minlength=D))])      # non-zeros in front of a (entity, column) slot
    ent_of_slot = np.repeat(ents, d_e)
    col_ptr, defined = np.zeros(Z + E, np.int32), np.zeros(Z + E, bool)
    at = znp[ent_of_slot] + ent_of_slot + (np.arange(D) - fp[ent_of_slot])
    col_ptr[at] = before[:D] - znp[ent_of_slot]
    close = znp[:-1] + ents + d_e
    col_ptr[close] = nnz_e
    defined[at] = True
    defined[close] = True
    return dict(E=E, N=N, Z=Z, D=D, ent_feat_ptr=fp, ent_nnz_ptr=znp, unique_global=pk["unique_global"], csr_col=pk["csr_col"],
                row_ptr=pk["row_ptr"], col_ptr=col_ptr, col_ptr_defined=defined, csc_row=local_row[order].astype(np.int32),
                csc_val=b.val[order], max_p=int(d_e.max()) + (1 if has_intercept else 0), max_n=int(b.ent_n().max()),
                max_nnz=int(nnz_e.max()))


def restated_entity(b, e):
    """The same for ONE entity, stated independently of expected() and of the oracle: np.unique(cols, return_inverse=True), a stable
    argsort of the local ids, a bincount -> dict(unique_global, csr_col, row_ptr, col_ptr, csc_row, csc_val) of the entity alone."""
    r0, r1 = int(b.ent_row_ptr[e]), int(b.ent_row_ptr[e + 1])
    rp = b.row_nnz_ptr[r0:r1 + 1] - b.row_nnz_ptr[r0]
    z0 = int(b.row_nnz_ptr[r0])
    cols, val = b.col_global[z0:z0 + int(rp[-1])], b.val[z0:z0 + int(rp[-1])]
    uniq, inv = np.unique(cols, return_inverse=True)
    inv = inv.reshape(-1)
    order = np.argsort(inv, kind="stable")
    rows = np.repeat(np.arange(r1 - r0), np.diff(rp))
    return dict(unique_global=uniq, csr_col=inv, row_ptr=rp, col_ptr=np.concatenate([[0], np.cumsum(np.bincount(inv, minlength=uniq.size))]),
                csc_row=rows[order], csc_val=val[order])


# ---- building a batch from per-entity row counts and columns ---------------------------------------------------------------------------
def _assemble(rows, cols, seed):
    """rows: per entity the non-zeros of each sample; cols: per entity its global columns in position order."""
    rng = np.random.default_rng(seed)
    ent_n = np.array([r.size for r in rows], np.int64)
    row_nnz = np.concatenate(rows).astype(np.int64)
    col = np.concatenate(cols).astype(np.int64)
    N, Z = int(ent_n.sum()), int(col.size)
    assert int(row_nnz.sum()) == Z
    return RawBatch(ent_row_ptr=np.concatenate([[0], np.cumsum(ent_n)]), row_nnz_ptr=np.concatenate([[0], np.cumsum(row_nnz)]), col_global=col,
                    val=rng.standard_normal(Z).astype(np.float32), y=(rng.random(N) < 0.5).astype(np.float32), offset=np.zeros(N, np.float32))


def _rows(kind, n, nnz, rng, pair=False):
    """The non-zeros of each of n samples. pair: some sample holds at least two (nnz >= 2, not for one_each)."""
    k = np.zeros(n, np.int64)
    if kind == "first":
        k[0] = nnz
    elif kind == "last":
        k[-1] = nnz
    elif kind == "one_each":
        assert n == nnz
        k[:] = 1
    else:
        slots = np.arange(0, n, 2) if kind == "alternate" else np.arange(n)
        keep = 2 if (pair and nnz >= 2) else 0
        k[slots] = rng.multinomial(nnz - keep, np.full(slots.size, 1.0 / slots.size))
        k[slots[rng.integers(0, slots.size)]] += keep
    return k


def _distinct(count, size, rng):
    if size <= 1 << 16:
        return rng.permutation(size)[:count]
    got = np.unique(rng.integers(0, size, 2 * count + 16))
    return rng.permutation(got)[:count]


def _cols(kind, nnz, size, rng, must, rows):
    """nnz columns below `size` of the given structure; `must` (a column, or None) occurs among them when nnz > 0."""
    if nnz == 0:
        return np.zeros(0, np.int64)
    if kind == "single":
        return np.full(nnz, int(rng.integers(0, size)) if must is None else must, np.int64)
    if kind in ("only0", "only63"):
        return np.full(nnz, 0 if kind == "only0" else 63, np.int64)
    if kind == "all64":
        c = np.concatenate([np.arange(64), rng.integers(0, 64, nnz - 64)])
        return rng.permutation(c).astype(np.int64)
    if kind == "distinct":
        c = _distinct(nnz, size, rng).astype(np.int64)
        if must is not None and must not in c:
            c[rng.integers(0, nnz)] = must
        return c
    if kind in ("d64", "d65"):
        pool = _distinct(int(kind[1:]), size, rng).astype(np.int64)
        if must is not None and must not in pool:
            pool[0] = must
        return rng.permutation(np.concatenate([pool, pool[rng.integers(0, pool.size, nnz - pool.size)]]))
    c = rng.integers(0, size if kind != "border" else min(size, 7), nnz).astype(np.int64)      # "random", "border", "dup"
    taken = []
    if kind == "border":      # equal columns on both sides of every 64-entry tile border
        c[np.arange(64, nnz, 64)] = c[np.arange(64, nnz, 64) - 1]
        taken = list(np.arange(64, nnz, 64)) + list(np.arange(64, nnz, 64) - 1)
    if kind == "dup":         # a column twice in one sample
        start = np.concatenate([[0], np.cumsum(rows)])
        i = int(np.flatnonzero(rows >= 2)[0])
        c[start[i] + 1] = c[start[i]]
        taken = [start[i], start[i] + 1]
    if must is not None:
        free = np.setdiff1d(np.arange(nnz), taken)
        c[free[rng.integers(0, free.size)] if free.size else 0] = must
    return c


def _pool(pool, space, k):
    """(columns are drawn below this, a column the entity must hold) of a pool: 'low' keeps an entity wholly below PACK_COUNT_COLS, 'mid'
    wholly below PACK_BITMAP_COLS with a column of PACK_COUNT_COLS or above in it, 'full' draws from the whole space with a column of
    PACK_BITMAP_COLS or above in it — so that every space shows every path it can reach."""
    if pool == "low":
        return min(space, PACK_COUNT_COLS), None
    if pool == "mid":
        return min(space, PACK_BITMAP_COLS), min(space, PACK_BITMAP_COLS) - 1
    return space, (space - 1 if k % 2 == 0 else PACK_BITMAP_COLS)


def pools(space):
    return ["low"] + (["mid"] if space > PACK_COUNT_COLS else []) + (["full"] if space > PACK_BITMAP_COLS else [])


def _col_kinds(nnz, size, pool, space):
    """The column structures an entity of nnz non-zeros over `size` columns can have."""
    if nnz == 0:
        return ["none"]
    kinds = ["random", "single"]
    if 2 <= nnz <= size:
        kinds.append("distinct")
    if nnz >= 2:
        kinds.append("dup")
    if nnz > WAVE and size >= 2:
        kinds.append("border")
    if nnz <= PACK_RANK_MAX:
        kinds += [k for k, d in (("d64", 64), ("d65", 65)) if d <= nnz and d <= size]
    elif pool == "low":
        kinds += ["only0"] + (["all64", "only63"] if space >= PACK_COUNT_COLS else [])
    return kinds


def _edge_specs(space, rng):
    """[(n, nnz, row kind, column kind, pool)]: the samples-wise list, then the non-zeros-wise list."""
    specs = []
    for n in N_LIST:
        for pool in pools(space):
            size = _pool(pool, space, 0)[0]
            k = [int(x) for x in rng.integers(2, PACK_RANK_MAX + 1, 3)]
            shapes = [(0, "first", "none"), (1, "first", "single"), (1, "last", "single"), (k[0], "spread", "random"),
                      (min(k[1], size), "alternate", "distinct"), (PACK_RANK_MAX, "last", "border"), (k[2], "spread", "dup"), (k[0] // 2 + 2, "alternate", "single"),
                      (100, "first", "d64" if size >= 64 else "random"), (PACK_RANK_MAX, "spread", "d65" if size >= 65 else "single")]
            if n <= PACK_RANK_MAX:
                shapes.append((n, "one_each", "random"))
            specs += [(n, nnz, rk if n > 1 or rk == "one_each" else "first", ck, pool) for nnz, rk, ck in shapes]
    small_n = dict(first=5, last=6, alternate=7, spread=3)
    for i, nnz in enumerate(NNZ_LIST):      # every column structure and every row structure of every (non-zero count, pool)
        for pool in pools(space):
            kinds = _col_kinds(nnz, _pool(pool, space, 0)[0], pool, space)
            for j in range(max(len(kinds), len(ROW_KINDS))):
                rk, ck = ROW_KINDS[(i + j) % len(ROW_KINDS)], kinds[j % len(kinds)]
                if rk == "one_each" and (ck == "dup" or nnz == 0):
                    rk = "spread"
                specs.append((nnz if rk == "one_each" else small_n[rk], nnz, rk, ck, pool))
    return specs


_EDGE = {}


def edge_batch(space):
    """-> dict(b, specs [(n, nnz, row kind, column kind, pool)] per entity, head, tail): entities on and around every constant of the
    pack with columns below `space`. The first four and the last four entities are one of every tier at its capacity (by non-zeros in
    front: 256, 512, 1 024 and 2 049 = two chunks and one entry; by samples behind: 256, 512, 1 024 and 1 025), each holding column
    space - 1, in an order that turns with the space, so that over SPACES every tier is first and last in a batch: the arrays are not
    padded, and what an entity writes past its own lands in its neighbour or behind the array. Built once per space."""
    if space in _EDGE:
        return _EDGE[space]
    rng = np.random.default_rng(space % 1000003)
    turn = SPACES.index(space) if space in SPACES else 0
    top = pools(space)[-1]
    head = [(4, z, "spread", "random", top) for z in (GDMIX_PACK_LDS_KEYS, PACK_CAP2, PACK_CAP3, 2 * BIG_CH + 1)]
    tail = [(n, PACK_RANK_MAX if n <= PACK_CAP3 else 5, "spread", "random", top) for n in (GDMIX_PACK_LDS_KEYS, PACK_CAP2, PACK_CAP3, PACK_CAP3 + 1)]
    head, tail = head[turn % 4:] + head[:turn % 4], tail[(turn + 1) % 4:] + tail[:(turn + 1) % 4]
    middle = _edge_specs(space, rng)
    middle = [middle[i] for i in rng.permutation(len(middle))]
    specs = head + middle + tail
    rows, cols = [], []
    for i, (n, nnz, rk, ck, pool) in enumerate(specs):
        size, must = _pool(pool, space, i)
        if i < 4 or i >= len(specs) - 4:
            must = space - 1
        if ck in ("only0", "only63", "all64"):
            must = None
        r = _rows(rk, n, nnz, rng, pair=ck == "dup")
        c = _cols(ck, nnz, size, rng, must, r)
        assert r.size == n and c.size == nnz and (nnz == 0 or (0 <= c.min() and c.max() < space)) and (must is None or nnz == 0 or must in c)
        rows.append(r)
        cols.append(c)
    _EDGE[space] = dict(b=_assemble(rows, cols, space % 1000003), specs=specs, space=space)
    return _EDGE[space]


_EXPECTED = {}


def expected_of(key, b, has_intercept=True):
    """expected(b), computed once per key and left unchanged (the maxima follow has_intercept)."""
    if key not in _EXPECTED:
        _EXPECTED[key] = expected(b, True)
    x = _EXPECTED[key]
    return x if has_intercept else dict(x, max_p=x["max_p"] - 1)


# ---- wavefronts that walk several entities ---------------------------------------------------------------------------------------------
def trips_sizes(num_cus):
    """Entities per tier: three trips of the first tier's wavefronts at 32 per CU, two and a bit of the 512- and 1 024-key tiers'."""
    w1, w2, w3 = TIER_WAVES_PER_CU
    return 3 * w1 * num_cus, 2 * w2 * num_cus + 600, 2 * w3 * num_cus + 300


_TRIPS = {}


def trips_batch(num_cus):
    """A batch in which every wavefront of every tier's grid walks more than two entities (trips_sizes), the tiers shuffled together so
    that the first tier's walk over ALL entities meets the others' (SKIP) between its own (SMALL). Two thirds of the entities of the 512-
    and 1 024-key tiers are large by their samples only (at most 60 non-zeros: bitmap or rank sort under row marks for up to 1 024 samples,
    row pointers from the in-trip loop), the rest by their non-zeros (count or bitonic beyond the 256 entries requested ahead), so that
    successive trips of a wavefront alternate long and short staging. Columns below 3 000: a tenth of the entities below 64, half of the
    rest below 2 048. One entity of every tier sits at its capacity by samples and one by non-zeros. Built once per CU count."""
    if num_cus in _TRIPS:
        return _TRIPS[num_cus]
    rng = np.random.default_rng(num_cus)
    n, z = [], []
    for t, e in enumerate(trips_sizes(num_cus)):
        lo, cap = (0, GDMIX_PACK_LDS_KEYS, PACK_CAP2)[t], (GDMIX_PACK_LDS_KEYS, PACK_CAP2, PACK_CAP3)[t]
        if t == 0:
            nt, zt = rng.integers(1, 81, e), rng.integers(0, 81, e)
            heavy, tall = rng.random(e) < 0.08, rng.random(e) < 0.05
            zt[heavy] = rng.integers(PACK_RANK_MAX + 1, cap + 1, int(heavy.sum()))
            nt[tall] = rng.integers(PACK_RANK_MAX + 1, cap + 1, int(tall.sum()))
        else:
            by_n = rng.random(e) < 2.0 / 3.0
            nt = np.where(by_n, rng.integers(lo + 1, cap + 1, e), rng.integers(1, 65, e))
            zt = np.where(by_n, rng.integers(0, 61, e), rng.integers(lo + 1, cap + 1, e))
        nt[:4], zt[:4] = [cap, 7, lo + 1, 3], [40, cap, 0, lo + 1]
        n.append(nt)
        z.append(zt)
    order = rng.permutation(sum(x.size for x in n))
    ent_n, ent_z = np.concatenate(n)[order].astype(np.int64), np.concatenate(z)[order].astype(np.int64)
    E, N, Z = ent_n.size, int(ent_n.sum()), int(ent_z.sum())
    erp, znp = np.concatenate([[0], np.cumsum(ent_n)]), np.concatenate([[0], np.cumsum(ent_z)])
    ent_of_nz = np.repeat(np.arange(E), ent_z)
    row = erp[ent_of_nz] + (rng.random(Z) * ent_n[ent_of_nz]).astype(np.int64)       # a sample of its entity for every non-zero
    u = rng.random(E)
    limit = np.where(u < 0.1, PACK_COUNT_COLS, np.where(u < 0.55, PACK_BITMAP_COLS, 3000))
    b = RawBatch(ent_row_ptr=erp, row_nnz_ptr=np.concatenate([[0], np.cumsum(np.bincount(row, minlength=N))]),
                 col_global=(rng.random(Z) * limit[ent_of_nz]).astype(np.int64), val=rng.standard_normal(Z).astype(np.float32),
                 y=(rng.random(N) < 0.5).astype(np.float32), offset=np.zeros(N, np.float32))
    assert np.array_equal(b.row_nnz_ptr[erp], znp)
    _TRIPS[num_cus] = b
    return b


def many_big_batch(space=2000):
    """1 100 big entities, more than one 1 024-entity tile of big_head_kernel: 1 070 of 1 025 samples and 0 to 8 non-zeros (big by their
    samples, one chunk each), 30 of 1 025 to 5 000 non-zeros (half of them with few samples), four of these at the ends of the batch and
    on both sides of entity 1 024 — the sizes, the chunk counts and the row counts all carry over the tile border. Columns below
    `space`, space - 1 among the big entities' (2 000: the counting path; above 2 048: the sort path)."""
    rng = np.random.default_rng(7 + space)
    E = 1100
    ent_n, ent_z = np.full(E, PACK_CAP3 + 1, np.int64), rng.integers(0, 9, E).astype(np.int64)
    heavy = np.concatenate([[0, 1023, 1024, E - 1], rng.choice(np.arange(1, 1023), 26, replace=False)])
    ent_z[heavy] = rng.integers(PACK_CAP3 + 1, 5001, heavy.size)
    ent_n[heavy[::2]] = rng.integers(1, 40, heavy[::2].size)
    erp = np.concatenate([[0], np.cumsum(ent_n)])
    N, Z = int(erp[-1]), int(ent_z.sum())
    ent_of_nz = np.repeat(np.arange(E), ent_z)
    row = erp[ent_of_nz] + (rng.random(Z) * ent_n[ent_of_nz]).astype(np.int64)
    cols = rng.integers(0, space, Z).astype(np.int64)
    cols[int(np.cumsum(ent_z)[heavy[1]]) - 1] = space - 1
    return RawBatch(ent_row_ptr=erp, row_nnz_ptr=np.concatenate([[0], np.cumsum(np.bincount(row, minlength=N))]), col_global=cols,
                    val=rng.standard_normal(Z).astype(np.float32), y=(rng.random(N) < 0.5).astype(np.float32), offset=np.zeros(N, np.float32))


def with_bad_column(tier, value):
    """A small valid batch with one entity of the given tier in the middle, ONE of whose columns is `value` (2^31 or -1: outside
    [0, 2^31)): the only fault of the batch. But for that column the entity would take the path of its tier that addresses by column —
    the bitmap (100 non-zeros below 64), the count (400 below 64), the counting sort (1 500 below 2 000) — or, in the 1 024-key tier, the
    bitonic network; with it the first two must take the rank sort and the bitonic network, which only sort and copy the value, and the
    counting sort masks it (see test_gpu_pack_edges.test_column_range)."""
    rng = np.random.default_rng(100 + tier)
    nnz, size = {1: (100, 64), 2: (400, 64), 3: (900, 5000), BIG: (1500, 2000)}[tier]
    rows = [_rows("spread", 6, 30, rng), _rows("spread", 9, nnz, rng), _rows("spread", 5, 140, rng)]
    cols = [rng.integers(0, s, int(r.sum())) for r, s in zip(rows, (5000, size, 5000))]
    cols[1][nnz // 2] = value
    return _assemble(rows, cols, 100 + tier)
