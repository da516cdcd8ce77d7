"""Shared by tests/test_fe_pass_edges.py (CPU) and tests/test_gpu_fe_pass_edges.py (GPU): the fixed-effect evaluation — fe_scatter_kernel in
all its forms, fe_rows_fix_kernel, fe_finish_kernel with fe_hot_finish_block (csrc/fe_solve.hip) and the copies csrc/fe_copy.hip builds for
them — held to a np.longdouble reference of ONE evaluation, element by element, on shards built on the kernels' own constants.

The constants of the library are literals ON PURPOSE: a constant changed in the library and not here fails
test_fe_pass_edges.test_the_constants_are_the_librarys; changed here first, tests/test_fe_pass_edges.py names the situations the shards
below no longer show, and the shape to move.

THE RESTATEMENT. pass_plans(shard, hooks) restates fe_build_copy / fe_build_column_copy in numpy: per pass the units (block, window, first
entry, length, kbase), which of them take the 6-byte form and with how many trips and fillers, the frequent columns and vbase, nmulti, nred,
and the bytes a pass streams. With GDMIX_FE_CHUNK below 4 096, sparse_chunk equals the chunk, so the sparse rule (a block with fewer than
four entries per 128-byte line of the gathered vector gets shorter units) drops out; it is restated anyway, for the shards that run without
the hook. The coverage assertions of the CPU file work on these plans; the GPU file proves with stream_bytes() of the created problem that
the plan describes what actually ran.

THE TOLERANCE LAW. u = 2^-53. Sample i has m_i = its entries + 2 and Z_i = sum_k |v_ik theta_k| + |theta_b| + |o_i|; r_i is its residual,
D_i the residual's derivative in z. Gradient output j with L_j entries is held to K E_j,

    E_j = u sum_i |v_ij| (L_j |r_i| + m_i D_i Z_i),

the value to K u sum_i (|l_i| + m_i |r_i| Z_i) (its sum is error-free on the device: no factor n), the intercept's entry to the gradient's
bound with v = 1 and L = n, the Hessian diagonal and the product X~' D X~ v to the same first-order bounds of their own terms (evaluate()).
r_ref is the largest err / E that two float64 numpy routes — bincount in source order, reduceat in sorted order — reach against the
longdouble reference over every small case of the suite (measure_r_ref; 51 cases, three quantities each): measured 5.43, reached by
the gradient of the trips shard under the Poisson loss without weights and intercept — samples of one small entry have m Z < 1 there, and
the rounding of exp(z) itself, u D, is then larger than the law's m D Z u; both float64 routes and the device meet the same figure. The
Hessian diagonal reaches 2.96, the product 0.94. R_REF = 5.5 is the measured value rounded up to two digits, and K = 8 max(R_REF, 1) = 44.
The factor 8 is for the device adding the same sums in other groupings (units, strands, replicas, lane order, the pair order of the packed
form) and for nothing else (docs/kernels.md, "The tolerance law").

gdmix_fe_hessian_diag takes D_i = w rho (1 - rho) for the logistic AND the squared loss and w exp(z) for Poisson (include/gdmix_fe.h); the
product takes the loss's own curvature (2 w for the squared loss). The reference follows the header."""
import numpy as np

from gdmix_amd import fixed_effect as fe
from gdmix_amd import synthetic

# ---- the constants: change one HERE first, then run tests/test_fe_pass_edges.py --------------------------------------------------------
WAVE = 64                         # csrc/re_device.hpp
# csrc/fe_internal.hpp
FE_B = 2048                       # accumulators (rows / columns) per block
FE_U = 8                          # entries per lane in flight: a full trip is WAVE * FE_U entries
FE_THREADS = 256
FE_FIN_BLOCKS = 64
FE_LOC_BITS = 11
FE_HOT_MAX = 64
FE_HOT_REP = 32
FE_HOT_MIN = 1 << 16
FE_SPAN_BITS = 32 - FE_LOC_BITS   # 21
FE_CTRIP = WAVE * 8               # 512
FE_CTRIP_BYTES = FE_CTRIP * 6     # 3072
FE_CDELTA_MAX = 31
FE_COMPRESS_DEFAULT = 2
# csrc/fe_solve.hip
FE_STRANDS = 16
FE_RED_OUT = FE_THREADS // FE_STRANDS          # 16
FE_FIX_PER_BLOCK = FE_B // FE_RED_OUT          # 128
FE_HOT_STRANDS = FE_THREADS // FE_HOT_REP      # 8: the strands of fe_hot_finish_block
# csrc/fe_copy.hip
CHUNK_FLOOR = 8192                # fe_chunk_len
CHUNK_CLIP = 1 << 28
CHUNK_HOOK_MIN = 64               # GDMIX_FE_CHUNK below it is no value
TRIP = WAVE * FE_U                # 512
NUM_CUS = 256                     # an MI355X; fe_chunk_len's target only matters above the floor, which no shard here reaches

# lines of the sources the restatement was read from, with blanks squeezed: (file, line); each occurs exactly once
SOURCE_LINES = (
    ("re_device.hpp", "constexpr int WAVE = 64;"),
    ("fe_internal.hpp", "#define GDMIX_FE_B 2048"),
    ("fe_internal.hpp", "#define GDMIX_FE_UNROLL 8"),
    ("fe_internal.hpp", "constexpr int FE_THREADS = 256;"),
    ("fe_internal.hpp", "constexpr int FE_FIN_BLOCKS = 64;"),
    ("fe_internal.hpp", "constexpr int FE_LOC_BITS = 11;"),
    ("fe_internal.hpp", "constexpr int FE_HOT_MAX = 64;"),
    ("fe_internal.hpp", "constexpr int FE_HOT_REP = 32;"),
    ("fe_internal.hpp", "constexpr long FE_HOT_MIN = 1 << 16;"),
    ("fe_internal.hpp", "constexpr int FE_SPAN_BITS = 32 - FE_LOC_BITS;"),
    ("fe_internal.hpp", "constexpr int FE_CTRIP = WAVE * 8;"),
    ("fe_internal.hpp", "constexpr int FE_CTRIP_BYTES = FE_CTRIP * 6;"),
    ("fe_internal.hpp", "constexpr int FE_CDELTA_MAX = 31;"),
    ("fe_internal.hpp", "#define GDMIX_FE_COMPRESS_DEFAULT 2"),
    ("fe_solve.hip", "constexpr int FE_STRANDS = 16;"),
    ("fe_solve.hip", "constexpr int FE_RED_OUT = FE_THREADS / FE_STRANDS;"),
    ("fe_solve.hip", "constexpr int FE_FIX_PER_BLOCK = FE_B / FE_RED_OUT;"),
    ("fe_solve.hip", "constexpr int STR = FE_THREADS / FE_HOT_REP;"),
    ("fe_solve.hip", "for (; base + WAVE * FE_U <= k1; base += WAVE * FE_U) {"),
    ("fe_solve.hip", "const int chunk = (F.nred + FE_FIN_BLOCKS - 1) / FE_FIN_BLOCKS;"),
    ("fe_solve.hip", "for (int b = b0 + tid; b < b1; b += FE_THREADS) {"),
    ("fe_solve.hip", "F.nred = F.rc.nunit + F.nmulti * FE_FIX_PER_BLOCK;"),
    ("fe_solve.hip", "if (strand == 0 && j0 + out < F.d && g != 0.0) F.fg[F.umap[jj]] = g;"),
    ("fe_solve.hip", 'if (const char* e = getenv("GDMIX_FE_CHUNK")) { const long v = atol(e); if (v >= 64) h.chunk = v; }'),
    ("fe_solve.hip", 'if (const char* e = getenv("GDMIX_FE_WINDOW_BITS")) { const int v = atoi(e); if (v >= 1 && v < FE_SPAN_BITS) h.window_bits = v; }'),
    ("fe_copy.hip", "if (c < 8192) c = 8192;"),
    ("fe_copy.hip", "if (c > (1 << 28)) c = 1 << 28;"),
    ("fe_copy.hip", "int64_t c = (avg <= 2 * target) ? 2 * avg : target;"),
    ("fe_copy.hip", "__device__ __forceinline__ int fe_fillers(int gap) { return gap > FE_CDELTA_MAX ? (gap - 1) / FE_CDELTA_MAX : 0; }"),
    ("fe_copy.hip", "if (nu > 0 && trips * FE_CTRIP_BYTES * 10 <= nu * 8 * 9) {"),
    ("fe_copy.hip", "col2[k] = h >= 0 ? vbase + h * FE_HOT_REP + (k % FE_HOT_REP) : c;"),
    ("fe_copy.hip", "return (sparse_chunk > 0 && (int64_t)len * 4 < (int64_t)extent) ? sparse_chunk : chunk;"),
    ("fe_copy.hip", "P.sparse_chunk = src.cut_sparse ? (P.chunk / 8 > 4096 ? P.chunk / 8 : (P.chunk < 4096 ? P.chunk : 4096)) : 0;"),
    ("fe_copy.hip", "nch[b] = b < nblock ? (len == 0 ? (b % nwin == 0 ? 1 : 0) : (len + c - 1) / c) : 0;"),
    ("fe_copy.hip", "B.packed = GDMIX_FE_PACK && B.max_span < (1 << (32 - FE_LOC_BITS)) && B.hooks.pack.value_or(true);"),
    ("fe_copy.hip", "const int vbase = (d + FE_B - 1) / FE_B * FE_B;"),
)

U = 2.0 ** -53
LOSSES = ("logistic", "squared", "poisson")
MODEL_TYPE = {"logistic": fe.LOGISTIC_REGRESSION, "squared": fe.LINEAR_REGRESSION, "poisson": fe.POISSON_REGRESSION}
R_REF = 5.5                       # measured by measure_r_ref(): 5.43, rounded up to two digits (docs/kernels.md, "The fixed-effect passes at their edges")
K = 8.0 * max(R_REF, 1.0)
FIT_RTOL = 1e-9                   # condition (a): no output is held looser than the fit tests hold theta
HOT_H = 48                        # GDMIX_FE_HOT_MIN of the frequent-column shards


# ---- the hooks ---------------------------------------------------------------------------------------------------------------------------
ENV = dict(chunk="GDMIX_FE_CHUNK", window_bits="GDMIX_FE_WINDOW_BITS", pack="GDMIX_FE_PACK", hot_min="GDMIX_FE_HOT_MIN", compress="GDMIX_FE_COMPRESS")


def env_of(hooks):
    """{variable: string, or None = unset} of a hook set (a dict with some of ENV's keys)."""
    assert set(hooks) <= set(ENV), hooks
    return {var: (None if hooks.get(k) is None else str(int(hooks[k]))) for k, var in ENV.items()}


def hook_id(hooks):
    return ",".join(f"{k}={int(v)}" for k, v in hooks.items() if v is not None) or "plain"


# ---- the restatement of fe_build_copy / fe_build_column_copy -----------------------------------------------------------------------------
def fillers(gap):
    """fe_fillers: a key gap g > 31 takes (g - 1) / 31 fillers of delta 31 and leaves a delta in [1, 31] for the entry itself."""
    gap = np.asarray(gap, np.int64)
    return np.where(gap > FE_CDELTA_MAX, (gap - 1) // FE_CDELTA_MAX, 0)


def chunk_len(z, nblock, num_cus, chunk_hook):
    """fe_chunk_len: entries per unit."""
    target = -(-z // (num_cus * 8))
    avg = -(-z // nblock)
    c = 2 * avg if avg <= 2 * target else target
    c = max(c, CHUNK_FLOOR)
    if chunk_hook is not None and chunk_hook >= CHUNK_HOOK_MIN:
        c = int(chunk_hook)
    return min(c, CHUNK_CLIP)


class CopyPlan:
    """One pass's copy: nblock, nwin, chunk, sparse_chunk, nunit; per unit ublock, uwin, ustart [nunit + 1], ulen, kbase, fillers, cnt (entries
    in the 6-byte form, fillers included), trips, taken; ufirst [nblock + 1]; packed; stream_bytes; order (source entry of every sorted
    entry), key and acc (gathered element and accumulator within the block of every sorted entry)."""

    def units_of_block(self, b):
        return int(self.ufirst[b + 1] - self.ufirst[b])


def copy_plan(seg, idx, nseg, length, cut_sparse, compress, hooks, num_cus=NUM_CUS):
    """seg, idx [z]: segment (the gathered element) and output index of every entry in source order, segment-major."""
    P = CopyPlan()
    z = int(seg.size)
    assert z > 0 and length > 0
    P.nblock = -(-length // FE_B)
    P.chunk = chunk_len(z, P.nblock, num_cus, hooks.get("chunk"))
    wb = hooks.get("window_bits")
    wbits = int(wb) if wb is not None and 1 <= wb < FE_SPAN_BITS else FE_SPAN_BITS
    P.nwin = ((nseg - 1) >> wbits) + 1
    nbw = P.nblock * P.nwin
    extent = nseg if nseg < (1 << wbits) else (1 << wbits)
    P.sparse_chunk = (P.chunk // 8 if P.chunk // 8 > 4096 else min(P.chunk, 4096)) if cut_sparse else 0
    skey = (idx // FE_B) * P.nwin + (seg >> wbits)
    P.order = np.argsort(skey, kind="stable")                         # the radix sort is stable: source order survives in a (block, window)
    P.key, P.acc = seg[P.order], idx[P.order] % FE_B
    bp = np.searchsorted(skey[P.order], np.arange(nbw + 1), side="left")
    blen = np.diff(bp)
    c = np.where((P.sparse_chunk > 0) & (blen * 4 < extent), P.sparse_chunk, P.chunk)     # fe_block_chunk
    nch = np.where(blen == 0, (np.arange(nbw) % P.nwin == 0).astype(np.int64), -(-blen // c))      # fe_chunks_kernel
    first = np.concatenate([[0], np.cumsum(nch)])
    ub = np.repeat(np.arange(nbw), nch)
    P.nunit = int(ub.size)
    P.ustart = np.concatenate([bp[ub] + (np.arange(P.nunit) - first[ub]) * c[ub], [z]])
    P.ulen = np.diff(P.ustart)
    P.ublock, P.uwin = ub // P.nwin, ub % P.nwin
    P.ufirst = first[np.arange(P.nblock + 1) * P.nwin]
    live = P.ulen > 0
    P.kbase = np.where(live, P.key[np.minimum(P.ustart[:-1], z - 1)], 0)
    span = np.where(live, P.key[np.maximum(P.ustart[1:] - 1, 0)] - P.kbase, 0)
    pk = hooks.get("pack")
    P.packed = bool(span.max() < (1 << FE_SPAN_BITS)) and (True if pk is None else bool(pk))
    per = 8 if P.packed else 10
    gap = np.diff(P.key, prepend=P.key[0])
    gap[P.ustart[:-1][live]] = 0                                      # a unit's first entry: its key is kbase
    assert gap.min() >= 0, "a unit's keys ascend"
    P.gap = gap
    cf = np.concatenate([[0], np.cumsum(fillers(gap))])
    P.fillers = cf[P.ustart[1:]] - cf[P.ustart[:-1]]
    P.cnt = P.ulen + P.fillers
    P.trips = -(-P.cnt // FE_CTRIP)
    P.pays = live & (P.trips * FE_CTRIP_BYTES * 10 <= P.ulen * 8 * 9)      # fe_choose_compressed
    P.taken = P.pays if compress else np.zeros(P.nunit, bool)
    P.stream_bytes = z * per
    if P.taken.any():
        P.stream_bytes = int(P.trips[P.taken].sum()) * FE_CTRIP_BYTES + int(P.ulen[~P.taken].sum()) * per
    return P


def pick_hot(counts, hot_min):
    """fe_pick_hot: the FE_HOT_MAX most frequent of the columns with at least hot_min entries (ties: the lower column), ascending."""
    if hot_min <= 0:
        return np.zeros(0, np.int64)
    cand = sorted((-int(c), j) for j, c in enumerate(counts) if c >= hot_min)[:FE_HOT_MAX]
    return np.array(sorted(j for _, j in cand), np.int64)


class PassPlans:
    """rows, cols: CopyPlan of the row and the column pass; hot (local columns), vbase; multi (row blocks of several units), nmulti, nred."""


def pass_plans(sh, hooks, num_cus=NUM_CUS):
    cm = hooks.get("compress")
    cm = FE_COMPRESS_DEFAULT if cm is None else int(cm) & 3
    R = PassPlans()
    # the row pass: outputs = rows, gathered = x by local column: from the column-major arrays (by column, then source position)
    R.rows = copy_plan(sh.lcol[sh.csc], sh.row[sh.csc], sh.d, sh.n, False, bool(cm & 1), hooks, num_cus)
    hm = hooks.get("hot_min")
    R.hot = pick_hot(sh.col_count, FE_HOT_MIN if hm is None else int(hm))
    col2, length, R.vbase = sh.lcol, sh.d, 0
    if R.hot.size:
        R.vbase = -(-sh.d // FE_B) * FE_B
        hmap = np.full(sh.d, -1, np.int64)
        hmap[R.hot] = np.arange(R.hot.size)
        h = hmap[sh.lcol]
        col2 = np.where(h >= 0, R.vbase + h * FE_HOT_REP + np.arange(sh.z) % FE_HOT_REP, sh.lcol)      # the replica by the entry's position
        length = R.vbase + R.hot.size * FE_HOT_REP
    R.cols = copy_plan(sh.row, col2, sh.n, length, True, bool(cm & 2), hooks, num_cus)
    R.multi = np.flatnonzero(np.diff(R.rows.ufirst) > 1)
    R.nmulti = int(R.multi.size)
    R.nred = R.rows.nunit + R.nmulti * FE_FIX_PER_BLOCK
    return R


# ---- a shard -----------------------------------------------------------------------------------------------------------------------------
def _seed(name):
    return int.from_bytes(str(name).encode(), "little") % (2 ** 31)


def _signed(rng, lo, hi, size):
    return rng.uniform(lo, hi, size) * rng.choice([-1.0, 1.0], size)


class Shard:
    """n rows, d local columns (every one with an entry), z entries sorted by row (source order otherwise kept); local column c is global
    feature c + 1 below the middle and c + 2 from it on, in a space of D = d + 3: features 0, d // 2 + 1 and D - 1 are absent from the
    shard. Values in +-[0.1, 1], theta0 / theta1 / vec in +-[0.05, 0.5] on every coefficient present or not (intercept last), offsets 0.2 N(0, 1),
    weights U[0.25, 2.25], all float32 but the coefficient vectors. cancel: [(a, b)] positions (in the order given) whose values are v, -v."""

    def __init__(self, name, n, rows, cols, cancel=(), small=True):
        rows, cols = np.asarray(rows, np.int64), np.asarray(cols, np.int64)
        rng = np.random.default_rng(_seed(name))
        val = _signed(rng, 0.1, 1.0, rows.size).astype(np.float32)
        for a, b in cancel:
            val[b] = -val[a]
        o = np.argsort(rows, kind="stable")
        self.name, self.n, self.z = name, int(n), int(rows.size)
        self.row, self.lcol, self.val = rows[o], cols[o], val[o]
        self.d = int(cols.max()) + 1
        self.col_count = np.bincount(self.lcol, minlength=self.d)
        assert self.col_count.min() > 0, f"{name}: local column {int(np.argmin(self.col_count))} has no entry"
        assert 0 <= rows.min() and rows.max() < n
        self.rp = np.concatenate([[0], np.cumsum(np.bincount(self.row, minlength=n))]).astype(np.int64)
        self.row_count = np.diff(self.rp)
        self.csc = np.argsort(self.lcol, kind="stable")
        self.col_ptr = np.concatenate([[0], np.cumsum(self.col_count)])
        self.uniq = np.arange(self.d) + 1 + (np.arange(self.d) >= self.d // 2)
        self.D = self.d + 3
        self.absent = np.array([0, self.d // 2 + 1, self.D - 1])
        self.col = self.uniq[self.lcol]
        self.off = (0.2 * rng.standard_normal(n)).astype(np.float32)
        self.wt = rng.uniform(0.25, 2.25, n).astype(np.float32)
        self.y01 = (rng.random(n) < 0.5).astype(np.float32)
        self.theta0, self.theta1, self.vec = (_signed(rng, 0.05, 0.5, self.D + 1) for _ in range(3))
        self.cancel_cols = sorted({int(cols[a]) for a, _ in cancel})
        self.small = small
        self._y = {}

    def labels(self, loss):
        """0/1 for the logistic loss; the project's own real and count labels over them for the other two."""
        if loss not in self._y:
            if loss == "logistic":
                self._y[loss] = self.y01
            else:
                b, _ = fe.shard_as_batch(self.rp, self.col, self.val, self.y01, self.off, None, True, dummy=False)
                make = synthetic.with_real_labels if loss == "squared" else synthetic.with_count_labels
                self._y[loss] = np.asarray(make(b, seed=_seed(self.name) % 1000).y, np.float32)
        return self._y[loss]

    def point(self, which, ic):
        """theta0 / theta1 / vec as the library takes them: [D + ic], intercept last."""
        return np.ascontiguousarray(getattr(self, which)[:self.D + ic])


# ---- the reference -----------------------------------------------------------------------------------------------------------------------
def _rowsum(x, sh, route):
    if route == "bincount":
        return np.bincount(sh.row, weights=x, minlength=sh.n)
    out = np.zeros(sh.n, x.dtype)
    ne = sh.row_count > 0
    out[ne] = np.add.reduceat(x, sh.rp[:-1][ne])                      # (reduceat over the rows that have entries: an empty segment would repeat an element)
    return out


def _colsum(x, sh, route):
    if route == "bincount":
        return np.bincount(sh.lcol, weights=x, minlength=sh.d)
    return np.add.reduceat(x[sh.csc], sh.col_ptr[:-1])               # a sorted copy: bincount has no longdouble


def loss_parts(loss, z, y, w):
    """-> l_i, r_i = dl/dz, D_i = dr/dz, |dD/dz| in z's dtype."""
    if loss == "squared":
        e = z - y
        return w * e * e, 2 * w * e, 2 * w + 0 * z, 0 * z
    if loss == "poisson":
        e = np.exp(z)
        return w * (e - y * z), w * (e - y), w * e, w * e
    s = 1 / (1 + np.exp(-z))
    return w * (np.log1p(np.exp(-np.abs(z))) + np.maximum(z, 0) - z * y), w * (s - y), w * s * (1 - s), w * s * (1 - s) * np.abs(1 - 2 * s)


def diag_parts(loss, z, w):
    """The curvature weight of gdmix_fe_hessian_diag and |its derivative|: w exp(z) for Poisson, w rho (1 - rho) otherwise (include/gdmix_fe.h)."""
    if loss == "poisson":
        return w * np.exp(z), w * np.exp(z)
    s = 1 / (1 + np.exp(-z))
    return w * s * (1 - s), w * s * (1 - s) * np.abs(1 - 2 * s)


def _global(sh, ic, g, gb, last, T):
    out = np.zeros(sh.D + ic + 1, T)
    out[sh.uniq] = g
    if ic:
        out[sh.D] = gb
    out[sh.D + ic] = last
    return out


def evaluate(sh, loss, weighted, ic, theta0=None, theta1=None, vec=None, route="ld"):
    """One evaluation at theta0, the Hessian diagonal at theta1 and the product X~' D X~ vec at theta1, in the layout of the reduce buffer
    ([D + ic] in the global space, intercept last, then the value; the last slot of the diagonal and of the product reads 0).
    route 'ld': np.longdouble from the float32 arrays widened and float64 coefficients, with the law's bounds E_* and the sums of |terms| S_*
    next to every quantity, and per entry the |term| of the gradient and the diagonal (T_grad, T_diag); 'bincount' / 'reduceat': float64."""
    T = np.longdouble if route == "ld" else np.float64
    if route == "ld":
        assert np.finfo(np.longdouble).eps < 2.0 ** -60, "np.longdouble is no wider than float64 here: there is no reference"
    theta0 = sh.theta0 if theta0 is None else np.concatenate([theta0[:sh.D], [theta0[sh.D] if ic else 0.0]])
    theta1 = sh.theta1 if theta1 is None else np.concatenate([theta1[:sh.D], [theta1[sh.D] if ic else 0.0]])
    vec = sh.vec if vec is None else np.concatenate([vec[:sh.D], [vec[sh.D] if ic else 0.0]])
    v, o, y = sh.val.astype(T), sh.off.astype(T), sh.labels(loss).astype(T)
    w = sh.wt.astype(T) if weighted else np.ones(sh.n, T)
    row, lcol, n = sh.row, sh.lcol, sh.n
    m, L = (sh.row_count + 2).astype(T), sh.col_count.astype(T)
    out = {}

    def margins(theta):
        th = theta.astype(T)
        tl, tb = th[sh.uniq], (th[sh.D] if ic else T(0))
        return _rowsum(v * tl[lcol], sh, route) + tb + o, _rowsum(np.abs(v * tl[lcol]), sh, route) + np.abs(tb) + np.abs(o)

    z0, Z0 = margins(theta0)
    ell, r, D, _ = loss_parts(loss, z0, y, w)
    out["grad"] = _global(sh, ic, _colsum(v * r[row], sh, route), r.sum(), ell.sum(), T)
    z1, Z1 = margins(theta1)
    Dd, Ddp = diag_parts(loss, z1, w)
    out["diag"] = _global(sh, ic, _colsum(v * v * Dd[row], sh, route), Dd.sum(), 0, T)
    _, _, D1, D1p = loss_parts(loss, z1, y, w)
    vl, vb = vec.astype(T)[sh.uniq], (T(vec[sh.D]) if ic else T(0))
    t = _rowsum(v * vl[lcol], sh, route) + vb
    q = D1 * t
    out["hv"] = _global(sh, ic, _colsum(v * q[row], sh, route), q.sum(), 0, T)
    if route != "ld":
        return out
    a = np.abs
    u = T(U)
    s0 = m * D * Z0
    out["E_grad"] = u * _global(sh, ic, _colsum(a(v) * (L[lcol] * a(r)[row] + s0[row]), sh, route), (n * a(r) + s0).sum(), (a(ell) + m * a(r) * Z0).sum(), T)
    out["S_grad"] = _global(sh, ic, _colsum(a(v * r[row]), sh, route), a(r).sum(), a(ell).sum(), T)
    out["T_grad"] = a(v * r[row])
    s1 = m * Ddp * Z1
    out["E_diag"] = u * _global(sh, ic, _colsum(v * v * (L[lcol] * Dd[row] + s1[row]), sh, route), (n * Dd + s1).sum(), 0, T)
    out["S_diag"] = _global(sh, ic, _colsum(v * v * Dd[row], sh, route), Dd.sum(), 0, T)
    out["T_diag"] = v * v * Dd[row]
    Tt = _rowsum(a(v * vl[lcol]), sh, route) + a(vb)
    s2 = m * (D1p * Z1 * a(t) + D1 * Tt)
    out["E_hv"] = u * _global(sh, ic, _colsum(a(v) * (L[lcol] * a(q)[row] + s2[row]), sh, route), (n * a(q) + s2).sum(), 0, T)
    out["S_hv"] = _global(sh, ic, _colsum(a(v * q[row]), sh, route), a(q).sum(), 0, T)
    return out


_REF = {}


def reference(key, loss, weighted, ic):
    """evaluate(shard(key), ...) at the shard's own points, computed once and left unchanged."""
    k = (key, loss, bool(weighted), int(ic))
    if k not in _REF:
        _REF[k] = evaluate(shard(key), loss, weighted, ic)
    return _REF[k]


def law_ratio(got, ref, E):
    """max_j |got_j - ref_j| / E_j over the outputs with a bound; an output without one (no term at all) must be exactly 0. At most K under
    the law, r_ref for a float64 route."""
    g = np.asarray(got).astype(np.longdouble)
    if g.shape != ref.shape or not np.all(np.isfinite(g)):
        return np.inf
    has = E > 0
    if np.any(g[~has] != 0):
        return np.inf
    return float(np.max(np.abs(g[has] - ref[has]) / E[has])) if has.any() else 0.0


QUANTITIES = ("grad", "diag", "hv")


def measure_r_ref():
    """-> (r_ref, the case and quantity that reach it, [(case, quantity, ratio of the bincount route, ratio of the reduceat route)])."""
    rows = []
    for key, loss, weighted, ic in small_cases():
        sh, ref = shard(key), reference(key, loss, weighted, ic)
        r64 = {route: evaluate(sh, loss, weighted, ic, route=route) for route in ("bincount", "reduceat")}
        for q in QUANTITIES:
            rows.append(((key, loss, weighted, ic), q) + tuple(law_ratio(r64[route][q], ref[q], ref["E_" + q]) for route in ("bincount", "reduceat")))
    worst = max(rows, key=lambda r: max(r[2], r[3]))
    return max(worst[2], worst[3]), worst[:2], rows


# ---- the edge shards -----------------------------------------------------------------------------------------------------------------------
def _sym_block(s, total, base=0):
    """`total` entries of a symmetric pattern on [base, base + s)^2 in which every index has an entry: the diagonal (without index 0 when the
    parity asks for it: the pair (0, 1) covers it) and pairs (i, i + o), (i + o, i) for o = 1, 2, ..."""
    assert total >= s >= 1
    odd = (total - s) % 2
    assert not odd or s >= 2
    diag = np.arange(1 if odd else 0, s)
    npair = (total - diag.size) // 2
    ii, jj = [], []
    o = 1
    while len(ii) < npair:
        assert o < s, "no room for the pairs"
        take = min(npair - len(ii), s - o)
        ii += list(range(take))
        jj += list(range(o, o + take))
        o += 1
    ii, jj = np.array(ii, np.int64), np.array(jj, np.int64)
    r = np.concatenate([diag, ii, jj]) + base
    c = np.concatenate([diag, jj, ii]) + base
    assert r.size == total
    return r, c


SQUARE_S = (1, FE_B - 1, FE_B, FE_B + 1, 2 * FE_B + 1)


def _square(s):
    """Point 1: n = d = s; three entries a row (the diagonal keeps every column), one for s = 1."""
    i = np.arange(s)
    if s == 1:
        return Shard("square1", 1, [0], [0])
    rows = np.concatenate([i, i, i])
    cols = np.concatenate([i, (7 * i + 3) % s, (i + s // 2) % s])
    return Shard(f"square{s}", s, rows, cols)


WHOLE_N = 2 * FE_B


def _whole_and_cut():
    """Point 2: n = d = 4 096, rows i hold columns i +- 1 and i +- 7 (mod n): 8 192 entries in either row block and column block; one more on
    the diagonal of the second: 8 193 = two units, the second of one entry, next to a whole block, without a hook."""
    i = np.arange(WHOLE_N)
    rows = np.concatenate([i, i, i, i, [3000]])
    cols = np.concatenate([(i + 1) % WHOLE_N, (i - 1) % WHOLE_N, (i + 7) % WHOLE_N, (i - 7) % WHOLE_N, [3000]])
    return Shard("whole_and_cut", WHOLE_N, rows, cols)


TRIPS_N = FE_B + TRIP                # 2 560 rows and columns: a block of 2 048 and one of 512
TRIPS_BLOCKS = (5 * TRIP + 1, 2 * TRIP + TRIP - 1)       # entries of the two blocks, rows and columns alike: 2 561 (odd: block 1 starts at an odd entry), 1 535
TRIPS_CHUNKS = (64, TRIP, TRIP + 1)


def _trips():
    """Point 3: a symmetric pattern, so both passes see blocks of 2 561 and 1 535 entries. Chunk 512: units of 512 at 0 .. 2 048, one of 1, then
    512, 512 and 511 from the odd entry 2 561 on. Chunk 513: 513 at 0, 513 (odd), ... and 509; then 513 at 2 561 (odd), 513, 509. Row 0 and row
    2 048 (accumulator 0 of either block) hold entries, as do columns 0 and 2 048."""
    B, H = FE_B, TRIP
    i = np.arange(B)
    d0 = i[i != 5]
    j = np.arange(H)
    k = np.arange(H // 2)
    e = np.arange(H - 1)
    rows = np.concatenate([d0, [5, 9], j, B + j, B + e, B + 2 * k, B + 2 * k + 1])
    cols = np.concatenate([d0, [9, 5], B + j, j, B + e, B + 2 * k + 1, B + 2 * k])
    return Shard("trips", TRIPS_N, rows, cols)


STRAND_UNITS_SMALL = (1, 2, 16, 17, 63, 64, 65)      # one block of so many units at chunk 64, rows and columns alike (63 - 65: nred around 192)
STRAND_UNITS_BIG = (48, 49, 64, 65, 81)              # five full blocks in one shard
HOT_UNITS = (1, 8, 9, 32, 33, 41)                    # units of the virtual block: eight strands, unrolled by four


def _units_entries(k):
    return 64 * k - 31


def _strands_small(k):
    t = _units_entries(k)
    s = max(1, t // 3)
    s -= (t - s) % 2
    r, c = _sym_block(s, t)
    return Shard(f"strands{k}", s, r, c)


def _strands_big():
    parts = [_sym_block(FE_B, _units_entries(k), b * FE_B) for b, k in enumerate(STRAND_UNITS_BIG)]
    return Shard("strands_big", FE_B * len(parts), np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts]))


HOTUNITS_N, HOTUNITS_COLD = 600, 300


def hotunits_hot_min(k):
    return 30 if k == 1 else HOT_H


def _hotunits(k):
    """The virtual block of k units at chunk 64: 64 k - 31 entries of frequent columns (one to eight of them, at least 33 entries each) over
    600 rows; 300 other columns of exactly four entries."""
    rng = np.random.default_rng(k)
    t = _units_entries(k)
    nh = min(8, max(1, t // 100))
    counts = np.full(nh, t // nh)
    counts[:t - counts.sum()] += 1
    d = HOTUNITS_COLD + nh
    hot_ids = np.linspace(0, d - 1, nh + 2).astype(np.int64)[1:-1]
    cold_ids = np.setdiff1d(np.arange(d), hot_ids)
    i = np.arange(HOTUNITS_N)
    rows = [i, i]
    cols = [cold_ids[(2 * i) % HOTUNITS_COLD], cold_ids[(2 * i + 1) % HOTUNITS_COLD]]
    for h, c in zip(hot_ids, counts):
        rows.append(rng.choice(HOTUNITS_N, int(c), replace=False))
        cols.append(np.full(int(c), h))
    return Shard(f"hotunits{k}", HOTUNITS_N, np.concatenate(rows), np.concatenate(cols))


EMPTIES_N, EMPTIES_D = 4 * FE_B, 400


def _empties():
    """Point 5: row blocks 1 and 3 (the last) without a non-zero; in blocks 0 and 2 row 0 and every fifth row are empty, the others hold two
    entries. The shard's first and last rows are empty."""
    i = np.concatenate([np.arange(0, FE_B), np.arange(2 * FE_B, 3 * FE_B)])
    i = i[i % 5 != 0]
    return Shard("empties", EMPTIES_N, np.concatenate([i, i]), np.concatenate([i % EMPTIES_D, (7 * i + 13) % EMPTIES_D]))


WINDOWS_N, WINDOWS_D = 2 * FE_B + 1, FE_B + 1
WINDOW_BITS = (1, 6)


def _windows():
    """Point 5, windows: n = 4 097, d = 2 049, two entries a row; windows of 2 and of 64 gathered elements."""
    i = np.arange(WINDOWS_N)
    return Shard("windows", WINDOWS_N, np.concatenate([i, i]), np.concatenate([i % WINDOWS_D, (3 * i + 1) % WINDOWS_D]))


HOT_N = 700
HOT_SHAPES = {"hot2048": (FE_B, 65), "hot2049": (FE_B + 1, 64), "hot2050": (FE_B + 2, 63)}      # name -> (d, candidates)
HOT_COUNT_CYCLE = (HOT_H + 1, HOT_H, HOT_H + 2, HOT_H + 5, HOT_H + 12, HOT_H, HOT_H + 3)


def _hot(name):
    """Point 6: `cand` columns of at least h = 48 entries spread over d columns (counts cycle through HOT_COUNT_CYCLE: h and h + 1 occur, h several
    times), two columns of h - 1, every other column one entry. hot2049: column 2 048 is ordinary; hot2050: columns 2 048 and 2 049 are both
    frequent, so column block 1 is left without entries. Row 0 holds the first entry of candidates 0 .. 31 at positions 0 .. 31: a frequent
    column starts at every residue mod 32. Candidate 1 is twice in one row."""
    d, ncand = HOT_SHAPES[name]
    rng = np.random.default_rng(d)
    cand = np.unique(np.linspace(0, FE_B - 1, ncand).astype(np.int64))
    if name == "hot2050":
        cand = np.concatenate([cand[:-2], [FE_B, FE_B + 1]])
    assert cand.size == ncand
    counts = np.array([HOT_COUNT_CYCLE[j % len(HOT_COUNT_CYCLE)] for j in range(ncand)])
    rows, cols = [], []
    for j, (c, cnt) in enumerate(zip(cand, counts)):
        first = 1 if j < FE_HOT_REP else 0
        r = 1 + rng.choice(HOT_N - 1, cnt - first - (1 if j == 1 else 0), replace=False)
        if j == 1:
            r = np.concatenate([r, r[:1]])                          # twice in one row
        rows.append(np.concatenate([[0], r]) if first else r)
        cols.append(np.full(cnt, c))
    rest = np.setdiff1d(np.arange(d), cand)
    near = rest[[10, 20]]                                            # two columns of h - 1 entries
    for c in near:
        rows.append(1 + rng.choice(HOT_N - 1, HOT_H - 1, replace=False))
        cols.append(np.full(HOT_H - 1, c))
    others = np.setdiff1d(rest, near)
    rows.append(1 + rng.integers(0, HOT_N - 1, others.size))
    cols.append(others)
    rows, cols = np.concatenate(rows), np.concatenate(cols)
    # (the sort by row is stable: row 0 keeps the candidates in the order they were appended, at positions 0 .. 31)
    return Shard(name, HOT_N, rows, cols)


def _hot1():
    """d = 1 with its only column frequent: 100 rows, row 50 empty, row 7 holds the column twice."""
    i = np.arange(100)
    rows = np.concatenate([i[i != 50], [7]])
    return Shard("hot1", 100, rows, np.zeros(rows.size, np.int64))


COMPRESS_WINDOW_BITS = FE_LOC_BITS     # windows of 2 048 gathered elements: a unit is a 2 048 x 2 048 tile of the matrix, in either pass
COMPRESS_N, COMPRESS_D = 5 * FE_B, 4 * FE_B
# tile (row block, column block) -> {key gap: how often}; a chain of entries (r0 + p, c0 + p) whose positions p advance by these gaps, so both
# passes meet the same gaps (0 = the same (row, column) twice)
COMPRESS_TILES = {
    "A": ((0, 0), {0: 10, 31: 20, 1: 396}),                                        # 427 entries, no filler: taken
    "B": ((1, 1), {0: 10, 31: 20, 1: 395}),                                        # 426 entries, no filler: plain
    "C": ((2, 2), {1000: 1, 63: 1, 62: 1, 32: 7, 31: 3, 0: 5, 1: 451}),            # 470 entries + 42 fillers = 512: one trip, taken
    "D": ((3, 3), {1000: 1, 63: 1, 62: 1, 32: 7, 31: 3, 0: 5, 1: 452}),            # 471 + 42 = 513: two trips, which 471 entries do not pay for
    "E": ((0, 1), {32: 5, 1: 894}),                                                # 900 entries + 5 fillers: two trips with padding, taken
}


def _compress():
    """Point 7, with windows of 2 048 so that a unit is a tile (row block, column block) in both passes: the chains of COMPRESS_TILES, and
    for every column c an entry in row 8 192 + c % 2 048 (row block 4: tiles of 2 048 entries of gap 1, four full trips), which keeps every
    column present. A count of 513 makes two trips and 513 entries cannot pay for them (854 can): that boundary is on the choice, not on a
    taken unit; E is the taken unit of two trips."""
    rng = np.random.default_rng(7)
    rows, cols = [], []
    for name, ((rb, cb), gaps) in COMPRESS_TILES.items():
        g = rng.permutation(np.concatenate([np.full(k, gap) for gap, k in gaps.items()]))
        p = np.concatenate([[0], np.cumsum(g)])
        assert p[-1] < FE_B, name
        rows.append(rb * FE_B + p)
        cols.append(cb * FE_B + p)
    c = np.arange(COMPRESS_D)
    rows.append(COMPRESS_D + c % FE_B)
    cols.append(c)
    return Shard("compress", COMPRESS_N, np.concatenate(rows), np.concatenate(cols))


EXACT_N, EXACT_D = 300, 120


def _exact():
    """Point 9: 300 rows of three entries over 120 columns; column 120 has its only two entries, v and -v, in row 17 (next to the row's other
    entries), column 121 in the otherwise empty row 299."""
    i = np.arange(EXACT_N - 1)
    rows = np.concatenate([i, i, i, [17, 17, 299, 299]])
    cols = np.concatenate([i % EXACT_D, (7 * i + 3) % EXACT_D, (11 * i + 50) % EXACT_D, [120, 120, 121, 121]])
    z = rows.size
    return Shard("exact", EXACT_N, rows, cols, cancel=((z - 4, z - 3), (z - 2, z - 1)))


MANY_N, MANY_D, MANY_PER_ROW = 100_000, 20_000, 11


def _many_units():
    """Point 8: 1.1 M entries at chunk 64: about 17 000 units a pass, nred above 64 * 256."""
    rng = np.random.default_rng(11)
    rows = np.repeat(np.arange(MANY_N), MANY_PER_ROW)
    return Shard("many_units", MANY_N, rows, rng.integers(0, MANY_D, rows.size), small=False)


BUILDERS = {f"square{s}": (lambda s=s: _square(s)) for s in SQUARE_S}
BUILDERS.update({"whole_and_cut": _whole_and_cut, "trips": _trips, "strands_big": _strands_big, "empties": _empties, "windows": _windows,
                 "hot1": _hot1, "compress": _compress, "exact": _exact, "many_units": _many_units})
BUILDERS.update({f"strands{k}": (lambda k=k: _strands_small(k)) for k in STRAND_UNITS_SMALL})
BUILDERS.update({f"hotunits{k}": (lambda k=k: _hotunits(k)) for k in HOT_UNITS})
BUILDERS.update({name: (lambda name=name: _hot(name)) for name in HOT_SHAPES})
SMALL_KEYS = tuple(k for k in BUILDERS if k != "many_units")
VARIANT_SHARDS = {"trips": {"chunk": TRIP + 1}, "hot2048": {"hot_min": HOT_H, "chunk": 64}}      # the two shards of the variants, each under one hook set
DEFAULT_CASE = ("logistic", True, 1)                                                              # (loss, weighted, has_intercept) of every other problem
VARIANTS = tuple((loss, w, ic) for loss in LOSSES for w in (True, False) for ic in (1, 0))

_SHARDS = {}


def shard(key):
    if key not in _SHARDS:
        _SHARDS[key] = BUILDERS[key]()
    return _SHARDS[key]


def small_cases():
    """[(shard key, loss, weighted, ic)] of every small case: every shard under DEFAULT_CASE, the two variant shards under every variant."""
    out = [(k,) + DEFAULT_CASE for k in SMALL_KEYS]
    out += [(k,) + v for k in VARIANT_SHARDS for v in VARIANTS if v != DEFAULT_CASE]
    return out


def hook_sets_of(key):
    """Every hook set a shard runs under: its own, each packed and in three arrays; with compress_variants each also under GDMIX_FE_COMPRESS
    0 .. 3. Static tables, so that the GPU file can parametrise without building a shard."""
    base, cv = _HOOK_TABLE[key]
    out = []
    for h in base:
        forms = [dict(h, compress=cm) for cm in (0, 1, 2, 3)] if cv else [h]
        for f in forms:
            out += [f, dict(f, pack=0)]
    return out


_CHUNK64 = ({"chunk": 64},)
_HOT3 = ({"hot_min": HOT_H}, {"hot_min": HOT_H, "chunk": 64}, {"hot_min": 0})
_HOOK_TABLE = {f"square{s}": (({}, {"chunk": 64}), False) for s in SQUARE_S}
_HOOK_TABLE.update({"whole_and_cut": (({},), False), "trips": (tuple({"chunk": c} for c in TRIPS_CHUNKS), True), "strands_big": (_CHUNK64, False),
                    "empties": (({}, {"chunk": 64}), True), "windows": (tuple({"window_bits": b} for b in WINDOW_BITS), True), "hot1": (_HOT3, False),
                    "compress": (tuple({"window_bits": COMPRESS_WINDOW_BITS, "compress": cm} for cm in (3, 0, 1, 2)), False),
                    "exact": (({}, {"chunk": 64}, {"compress": 3}, {"hot_min": 6}), False), "many_units": (_CHUNK64, False)})
_HOOK_TABLE.update({f"strands{k}": (_CHUNK64, False) for k in STRAND_UNITS_SMALL})
_HOOK_TABLE.update({f"hotunits{k}": (({"chunk": 64, "hot_min": hotunits_hot_min(k)},), False) for k in HOT_UNITS})
_HOOK_TABLE.update({name: (_HOT3, False) for name in HOT_SHAPES})


def problems(keys=None):
    """[(shard key, hook set)] of the GPU file: one problem each."""
    return [(k, h) for k in (keys or BUILDERS) for h in hook_sets_of(k)]
