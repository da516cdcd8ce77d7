"""Shared by tests/test_narrow_class.py (CPU) and tests/test_gpu_narrow_class.py (GPU): entities of a stated shape for the narrow kernel
(re_solve_grp_kernel<16,5,24,96>: the entities of the class "re_solve_grp_kernel<32,3> n<=32 nnz<=128" with at most 80 coefficients,
24 samples and 96 non-zeros; include/gdmix_re.h, gdmix_re_set_narrow), and the comparison with the CPU oracle."""
import numpy as np

from gdmix_amd.batch import RawBatch
from oracle import oracle

REL_TOL_DEVICE = 1e-7     # tests/test_gpu_parity.py's bar
HOST_CLASS = "re_solve_grp_kernel<32,3> n<=32 nnz<=128"
NARROW_P, NARROW_N, NARROW_NNZ = 80, 24, 96


def is_narrow(p, n, nnz):
    """The narrow kernel's entities: those of the host class (64 < p <= 96 here: the classes in front of it take p <= 64 at these sample
    and non-zero counts) within the three caps."""
    p, n, nnz = np.asarray(p), np.asarray(n), np.asarray(nnz)
    return (p > 64) & (p <= NARROW_P) & (n <= NARROW_N) & (nnz <= NARROW_NNZ)


def make_shaped_batch(shapes, seed, D=4096, random_weights=False):
    """One entity per (d, n, nnz) of `shapes`: exactly d distinct features, n samples and nnz non-zeros (nnz >= max(d, n): every feature
    and every sample occurs). A cell may repeat inside a sample where nnz > d (the pack sums nothing: the mat-vecs add the repeats, as the
    reference's COO product does). Values, offsets ~ N(0, 1) fp32; y ~ Bernoulli(sigmoid(x . w* + offset)) with a hidden global w*."""
    rng = np.random.default_rng(seed)
    w_star = 0.5 * rng.standard_normal(D)
    ent_n, row_nnz, cols, vals = [], [], [], []
    for d, n, nnz in shapes:
        assert nnz >= max(d, n) and d <= D
        feats = rng.choice(D, size=d, replace=False)
        c = np.concatenate([feats, feats[rng.integers(0, d, size=nnz - d)]])
        c = c[rng.permutation(nnz)]
        rows = np.concatenate([np.arange(n), rng.integers(0, n, size=nnz - n)])
        rows.sort()
        ent_n.append(n)
        row_nnz.append(np.bincount(rows, minlength=n))
        cols.append(c)
        vals.append(rng.standard_normal(nnz).astype(np.float32))
    ent_n = np.asarray(ent_n, np.int64)
    row_nnz = np.concatenate(row_nnz).astype(np.int64)
    col = np.concatenate(cols).astype(np.int64)
    val = np.concatenate(vals)
    N = int(ent_n.sum())
    row_nnz_ptr = np.concatenate([[0], np.cumsum(row_nnz)]).astype(np.int64)
    offset = rng.standard_normal(N).astype(np.float32)
    logit = np.add.reduceat(val.astype(np.float64) * w_star[col], row_nnz_ptr[:-1]) + offset
    y = (rng.random(N) < 1.0 / (1.0 + np.exp(-logit))).astype(np.float32)
    weight = (0.25 + 2.0 * rng.random(N)).astype(np.float32) if random_weights else None
    return RawBatch(ent_row_ptr=np.concatenate([[0], np.cumsum(ent_n)]).astype(np.int64), row_nnz_ptr=row_nnz_ptr, col_global=col, val=val, y=y,
                    offset=offset, weight=weight, uid=np.arange(N, dtype=np.int64), entity_ids=[f"s{i}" for i in range(len(shapes))])


def narrow_shapes(rng, count, ic=1):
    """`count` shapes inside the narrow caps: p in 65 .. 80, n in 1 .. 24, nnz up to 96."""
    out = []
    for _ in range(count):
        d = int(rng.integers(65, NARROW_P + 1)) - ic
        n = int(rng.integers(1, NARROW_N + 1))
        out.append((d, n, int(rng.integers(max(d, n), NARROW_NNZ + 1))))
    return out


def history_batch(E, seed):
    return make_shaped_batch(narrow_shapes(np.random.default_rng([seed, 0x4E]), E), seed)


# (m, l2) -> (seed of the four-entity batch: one wavefront whatever the order; seed of the thirteen-entity batch) of the history test:
# the first seeds at which the ORACLE's own run meets the test's conditions (largest nit >= 15, memory wraps > 0, and for the four a
# spread of nit >= 5) and reproduces its status / nit / nfev from starts moved by 1e-15, 1e-14 and 1e-13
HISTORY_CASES = {(3, 1e-3): (1, 1), (3, 1e-6): (7, 1), (7, 1e-3): (2, 1), (7, 1e-6): (5, 1), (10, 1e-3): (2, 1), (10, 1e-6): (7, 1)}


def history_conditions(b, kw):
    """The oracle on batch b -> (its result, largest nit, nit spread over the batch's first four entities, memory wraps)."""
    pk = oracle.pack(b.ent_row_ptr, b.row_nnz_ptr, b.col_global)
    oracle.branch_counts(reset=True)
    ref = oracle.solve(pk, b.val, b.y, b.offset, b.weight, oracle.make_opts(**kw))
    wraps = oracle.branch_counts(reset=True)["memory_wraps"]
    nit = ref["nit"]
    return ref, int(nit.max()), int(nit[:4].max() - nit[:4].min()), int(wraps)


def compare_with_oracle(res, ref, coef_ptr, wp=None, variance=False):
    """tests/test_gpu_parity.py's _solve_and_compare, the part against the oracle: equal status, nit and nfev, theta within REL_TOL_DEVICE
    per entity, fval to rtol 1e-9 — on the entities of mask wp (None: all). Prints the worst figure before it asserts."""
    E = coef_ptr.size - 1
    wp = np.ones(E, bool) if wp is None else wp
    err = np.zeros(E)
    for e in range(E):
        s = slice(int(coef_ptr[e]), int(coef_ptr[e + 1]))
        err[e] = np.max(np.abs(res["theta"][s] - ref["theta"][s])) / max(float(np.max(np.abs(ref["theta"][s]))), 1e-300)
    print(f"narrow compare: {int(wp.sum())} entities, worst theta rel err {err[wp].max():.3e}, nit {int(ref['nit'][wp].min())} .. {int(ref['nit'][wp].max())}")
    assert np.all(res["status"] >= 0)
    assert np.array_equal(res["status"][wp], ref["status"][wp]), (res["status"][wp], ref["status"][wp])
    assert np.array_equal(res["nit"][wp], ref["nit"][wp]), (res["nit"][wp], ref["nit"][wp])
    assert np.array_equal(res["nfev"][wp], ref["nfev"][wp]), (res["nfev"][wp], ref["nfev"][wp])
    assert err[wp].max() <= REL_TOL_DEVICE, err[wp].max()
    np.testing.assert_allclose(res["fval"][wp], ref["fval"][wp], rtol=1e-9, atol=1e-13)
    if variance:
        np.testing.assert_allclose(res["variance"], ref["variance"], rtol=1e-7)
    return float(err[wp].max())
