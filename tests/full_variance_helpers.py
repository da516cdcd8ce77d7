"""Shared by tests/test_full_variance_edges.py (CPU) and tests/test_gpu_full_variance_edges.py (GPU): the tests' own dense statement of
variance_mode FULL — diag((X~' D X~ + (l2 + 1e-12) I - l2 e0 e0')^-1), binary_logistic_regression.py:181-187 — evaluated in np.longdouble
(a hand-written Cholesky and L^-1) next to two float64 routes, the tolerance law that follows from them, and the batches and matrices
that put the three kernel families (the wavefront kernel of csrc/re_solve.hip, the whole-device path of csrc/re_variance_big.hip and
its two-stage form for fixed-effect workers) on their tile, lane and routing edges.

The constants of the library are literals ON PURPOSE: a constant changed in the library and not here fails
test_full_variance_edges.test_the_constants_are_the_librarys; changed here first, tests/test_full_variance_edges.py names the sizes the
shapes below no longer show.

THE TOLERANCE LAW. An entity's variances are held to  max_j |got_j - ref_j| / |ref_j|  <=  K kappa_2(H) 2^-53,  element by element.
r_ref is the largest such ratio err / (kappa_2 2^-53) that the two float64 routes (the same Cholesky route in float64, and
np.linalg.inv) reach against the longdouble reference over every small case below (measure_r_ref); K = 8 max(r_ref, 1): the device adds
the same sums in other groupings (tiles, wavefront reductions, contraction), and the factor 8 is for that and nothing else. R_REF is
the measured value rounded up to two digits; tests/test_full_variance_edges.py measures it anew and holds the literal to it."""
import numpy as np

from gdmix_amd.batch import RawBatch

WAVE = 64
# csrc/re_internal.hpp
VAR_FULL_MAX_P = 2048             # one wavefront per entity up to here
VAR_FULL_BIG_MAX_P = 16384        # the whole device on one entity up to here
VAR_BIG_BUILD_GROUPS = 128        # workgroups of vf_build_kernel
# csrc/re_variance_big.hip
VF_T = 64                         # tile edge
VF_THREADS = 256
# csrc/re_api.hip, var_slots_for
VAR_SLOTS_MAX = 2048
CONSTANTS = {"re_internal.hpp": dict(VAR_FULL_MAX_P=VAR_FULL_MAX_P, VAR_FULL_BIG_MAX_P=VAR_FULL_BIG_MAX_P, VAR_BIG_BUILD_GROUPS=VAR_BIG_BUILD_GROUPS),
             "re_variance_big.hip": dict(VF_T=VF_T, VF_THREADS=VF_THREADS)}
# lines of the sources the shapes below were read from, with blanks squeezed: (file, line)
SOURCE_LINES = (("re_internal.hpp", "inline size_t var_full_slot_doubles(int64_t max_p) { return (size_t)2 * max_p * max_p + max_p + 8; }"),
                ("re_api.hip", "if (slots > 2048) slots = 2048;"),
                ("re_api.hip", "if ((size_t)vslots * vslot * 8 > avail) vslots = (int)(avail / (vslot * 8)) & ~3;"),
                ("re_solve.hip", "if (p > VAR_FULL_MAX_P) continue;"),
                ("re_solve.hip", "for (int t = lane; t < m * m; t += WAVE) {"),
                ("re_variance_big.hip", "if (d + ic <= min_p) continue;"),
                ("re_variance_big.hip", "for (int k = ka0 + tid; k < ka1; k += VF_THREADS) {"),
                ("re_pack.hip", "out->scratch_bytes = (size_t)(Z + 1) * 8;"))


def slot_doubles(p):
    """var_full_slot_doubles: H and L^-1 (p x p each), a dense row, and 8 doubles of padding."""
    return 2 * p * p + p + 8


U = 2.0 ** -53
LOSSES = ("logistic", "squared", "poisson")
L2 = 0.7
THETA_SD = 0.3
LD_MAX_P = 260                    # up to here the reference is the longdouble route; above it float64 np.linalg.inv
R_REF = 4.1                       # measured by measure_r_ref(), rounded up to two digits (docs/kernels.md, "FULL variances")
K = 8.0 * max(R_REF, 1.0)
RTOL_CAP = 1e-8                   # no entity that is not deliberately ill-conditioned is held looser than the older tests' rtol


# ---- the dense statement -----------------------------------------------------------------------------------------------------------------
def coef_ptr_of(b, ic):
    """[E + 1] the first coefficient of every entity: its distinct columns, and the intercept in front."""
    d = np.array([np.unique(b.col_global[b.row_nnz_ptr[b.ent_row_ptr[e]]:b.row_nnz_ptr[b.ent_row_ptr[e + 1]]]).size for e in range(b.E)], np.int64)
    return np.concatenate([[0], np.cumsum(d + ic)])


def dense_rows(b, e, ic, dtype=np.longdouble):
    """X~ [n, p] of entity e: repeated (row, column) entries summed, the intercept first, the columns in the order of their global ids."""
    r0, r1 = int(b.ent_row_ptr[e]), int(b.ent_row_ptr[e + 1])
    z0, z1 = int(b.row_nnz_ptr[r0]), int(b.row_nnz_ptr[r1])
    uniq, loc = np.unique(b.col_global[z0:z1], return_inverse=True)
    X = np.zeros((r1 - r0, uniq.size + ic), dtype)
    rows = np.repeat(np.arange(r1 - r0), np.diff(b.row_nnz_ptr[r0:r1 + 1]))
    np.add.at(X, (rows, ic + loc.reshape(-1)), b.val[z0:z1].astype(dtype))
    if ic:
        X[:, 0] = 1
    return X


def curvature_weights(loss, z, w):
    """D_i = w rho (1 - rho) for the logistic loss, 2 w for the squared, w exp(z) for Poisson, in z's dtype."""
    if loss == "squared":
        return 2 * w
    if loss == "poisson":
        return w * np.exp(z)
    rho = 1 / (1 + np.exp(-z))
    return w * rho * (1 - rho)


def entity_weights(b, e, X, theta_e, loss, dtype=np.longdouble):
    """D [n] of entity e at theta_e: the float32 values, offsets and weights widened, a float64 theta, everything from z on in dtype."""
    r0, r1 = int(b.ent_row_ptr[e]), int(b.ent_row_ptr[e + 1])
    z = X.astype(dtype) @ theta_e.astype(dtype) + b.offset[r0:r1].astype(dtype)
    w = np.ones(r1 - r0, dtype) if b.weight is None else b.weight[r0:r1].astype(dtype)
    return curvature_weights(loss, z, w)


def regulariser(p, l2, unreg, dtype=np.longdouble):
    """The diagonal that is added to X~' D X~: l2 + 1e-12, without l2 at index `unreg` (-1: everywhere)."""
    add = np.full(p, dtype(l2) + dtype(1e-12), dtype)
    if 0 <= unreg < p:
        add[unreg] = dtype(1e-12)
    return add


def entity_hessian(b, e, theta_e, loss, l2, ic, regularize_bias, dtype=np.longdouble):
    X = dense_rows(b, e, ic, dtype)
    D = entity_weights(b, e, X, theta_e, loss, dtype)
    H = (X.T * D) @ X
    H[np.diag_indices_from(H)] += regulariser(H.shape[0], l2, 0 if (ic and not regularize_bias) else -1, dtype)
    return H


def chol_inv_diag(H):
    """diag(H^-1) of SPD matrices [..., p, p] by a hand-written right-looking Cholesky H = L L', M = L^-1 by forward substitution and
    diag(H^-1)_j = sum_i M_ij^2 — the route of the kernels — in H's dtype."""
    A = np.array(H, copy=True)
    p = A.shape[-1]
    for j in range(p):
        A[..., j, j] = np.sqrt(A[..., j, j])
        if j + 1 < p:
            A[..., j + 1:, j] /= A[..., j, j][..., None]
            col = A[..., j + 1:, j]
            A[..., j + 1:, j + 1:] -= col[..., :, None] * col[..., None, :]
    M = np.zeros_like(A)
    for i in range(p):
        rhs = -np.einsum("...k,...kc->...c", A[..., i, :i], M[..., :i, :]) if i else np.zeros(A.shape[:-2] + (p,), A.dtype)
        rhs[..., i] += 1
        M[..., i, :] = rhs / A[..., i, i][..., None]
    return (M * M).sum(axis=-2)


def kappa2(H64):
    ev = np.linalg.eigvalsh(H64)
    return ev[..., -1] / ev[..., 0]


def variances_of(Hs_ld, Hs_64, routes=False):
    """Hessians of ONE size p (lists of [p, p], longdouble and float64) -> dict(ref [G, p] longdouble (float64 np.linalg.inv above
    LD_MAX_P), kappa [G]; with routes: chol64 and inv64 [G, p], the two float64 routes)."""
    H64 = np.stack(Hs_64)
    p = H64.shape[-1]
    out = dict(kappa=kappa2(H64))
    if p <= LD_MAX_P:
        assert np.finfo(np.longdouble).eps < 2.0 ** -60, "np.longdouble is no wider than float64 here: there is no reference"
        out["ref"] = chol_inv_diag(np.stack(Hs_ld))
        if routes:
            out["chol64"] = chol_inv_diag(H64)
            out["inv64"] = np.diagonal(np.linalg.inv(H64), axis1=-2, axis2=-1).copy()
    else:
        out["ref"] = np.diagonal(np.linalg.inv(H64), axis1=-2, axis2=-1).astype(np.longdouble)
    return out


_REF = {}


def reference(key, b, loss, l2, ic, regularize_bias, routes=False):
    """The per-entity reference of a whole batch at the theta drawn for (key, ic), computed once per (key, loss, l2, ic, regularize_bias)
    and left unchanged -> dict(theta [P], coef_ptr [E + 1], var [P] longdouble, kappa [E], p [E]; with routes: chol64, inv64 [P], NaN where
    p > LD_MAX_P)."""
    k = (key, loss, float(l2), int(ic), bool(regularize_bias))
    if k in _REF and (not routes or "chol64" in _REF[k]):
        return _REF[k]
    cp = coef_ptr_of(b, ic)
    theta = draw_theta((key, ic), cp[-1])
    by_p = {}
    for e in range(b.E):
        p = int(cp[e + 1] - cp[e])
        if p:
            by_p.setdefault(p, []).append(e)
    out = dict(theta=theta, coef_ptr=cp, var=np.full(cp[-1], np.nan, np.longdouble), kappa=np.ones(b.E), p=np.diff(cp))
    if routes:
        out.update(chol64=np.full(cp[-1], np.nan), inv64=np.full(cp[-1], np.nan))
    for p, ents in by_p.items():
        small = p <= LD_MAX_P
        H64 = [entity_hessian(b, e, theta[cp[e]:cp[e + 1]], loss, l2, ic, regularize_bias, np.float64) for e in ents]
        Hld = [entity_hessian(b, e, theta[cp[e]:cp[e + 1]], loss, l2, ic, regularize_bias) for e in ents] if small else None
        v = variances_of(Hld, H64, routes)
        for g, e in enumerate(ents):
            out["var"][cp[e]:cp[e + 1]] = v["ref"][g]
            out["kappa"][e] = v["kappa"][g]
            if routes and small:
                out["chol64"][cp[e]:cp[e + 1]] = v["chol64"][g]
                out["inv64"][cp[e]:cp[e + 1]] = v["inv64"][g]
    _REF[k] = out
    return out


def law_ratio(got, ref, kappa):
    """max_j |got_j - ref_j| / |ref_j| over (kappa 2^-53) of one entity: at most K under the law, r_ref for a float64 route."""
    if ref.size == 0:
        return 0.0
    g = np.asarray(got).astype(np.longdouble)
    if not np.all(np.isfinite(g)):
        return np.inf
    return float(np.max(np.abs(g - ref) / np.abs(ref)) / (kappa * U))


def law_ratios(got, ref):
    """law_ratio of every entity of a batch: got [P] against reference(...)."""
    cp = ref["coef_ptr"]
    return np.array([law_ratio(got[cp[e]:cp[e + 1]], ref["var"][cp[e]:cp[e + 1]], ref["kappa"][e]) for e in range(cp.size - 1)])


def draw_theta(key, P):
    seed = int.from_bytes(str(key).encode(), "little") % (2 ** 31)
    return np.random.default_rng(seed).normal(0.0, THETA_SD, int(P))


# ---- assembling batches ---------------------------------------------------------------------------------------------------------------------
def _assemble(ents, seed, weighted):
    """ents: per entity the list of its rows, each an int array of LOCAL columns (repeats allowed). Global ids are 3 local + 7 + e, so
    that no entity's columns are 0 .. d-1 already. Values N(0, 1), offsets N(0, 0.2), weights U(0.5, 2), all float32."""
    rng = np.random.default_rng(seed)
    ent_n = np.array([len(r) for r in ents], np.int64)
    row_nnz = np.array([len(c) for r in ents for c in r], np.int64)
    col = np.concatenate([np.asarray(c, np.int64) * 3 + 7 + e for e, r in enumerate(ents) for c in r] + [np.zeros(0, np.int64)])
    N, Z = int(ent_n.sum()), int(col.size)
    return RawBatch(ent_row_ptr=np.concatenate([[0], np.cumsum(ent_n)]), row_nnz_ptr=np.concatenate([[0], np.cumsum(row_nnz)]), col_global=col,
                    val=rng.standard_normal(Z).astype(np.float32), y=(rng.random(N) < 0.5).astype(np.float32),
                    offset=(0.2 * rng.standard_normal(N)).astype(np.float32),
                    weight=rng.uniform(0.5, 2.0, N).astype(np.float32) if weighted else None)


def _cover(d, per_row, rng, fill=0):
    """Rows that hold every one of d columns exactly once, per_row at a time in a random order; each then takes `fill` more distinct ones."""
    perm = rng.permutation(d)
    rows = [perm[i:i + per_row] for i in range(0, d, per_row)]
    out = []
    for r in rows:
        rest = np.setdiff1d(np.arange(d), r)
        extra = rng.permutation(rest)[:min(fill, rest.size)]
        out.append(rng.permutation(np.concatenate([r, extra])))
    return out


# ---- case 1: the factor and the inverse alone (gdmix_fe_variance_of_hessian) ----------------------------------------------------------------
FACTOR_P = (1, 2, 63, 64, 65, 127, 128, 129, 192, 193)
FACTOR_WIDE_P = (1, 64, 65)            # these also with ld one tile larger than needed
FACTOR_L2 = (0.0, L2)
FACTOR_CONDS = ("sparse", "spectrum")
SPECTRUM_KAPPA = 1e8


def tiles_ld(p):
    return (p + VF_T - 1) // VF_T * VF_T


def factor_shapes():
    """[(p, ld)]: every size at its own ld, three of them one tile wider."""
    return [(p, tiles_ld(p)) for p in FACTOR_P] + [(p, tiles_ld(p) + VF_T) for p in FACTOR_WIDE_P]


def factor_unregs(p):
    return sorted({-1, 0, p - 1})


_FACTOR_A = {}


def factor_matrix(p, cond):
    """The summed curvature matrix A [p, p] float64 a case uploads. 'sparse': X~' D X~ of a logistic entity of 8 p + 40 samples, six
    non-zeros each and an intercept, at a drawn theta: SPD on its own, kappa of order ten. 'spectrum': Q diag(lambda) Q' with a random
    orthogonal Q and lambda spaced evenly in the logarithm from SPECTRUM_KAPPA down to 1."""
    if (p, cond) in _FACTOR_A:
        return _FACTOR_A[(p, cond)]
    rng = np.random.default_rng(1000 * p + len(cond))
    if cond == "sparse":
        d, n = p - 1, 8 * p + 40
        rows = [rng.permutation(d)[:min(d, 6)] for _ in range(n)]
        b = _assemble([rows], 1000 * p, weighted=True)
        X = dense_rows(b, 0, 1, np.float64)
        assert X.shape == (n, p)
        D = entity_weights(b, 0, X, rng.normal(0.0, THETA_SD, p), "logistic", np.float64)
        A = (X.T * D) @ X
    else:
        Q, _ = np.linalg.qr(rng.standard_normal((p, p)))
        lam = np.logspace(np.log10(SPECTRUM_KAPPA), 0.0, p) if p > 1 else np.array([SPECTRUM_KAPPA])
        A = (Q * lam) @ Q.T
    A = (A + A.T) / 2
    _FACTOR_A[(p, cond)] = A
    return A


def factor_cases(p):
    """[(cond, l2, unreg)] of one size."""
    return [(cond, l2, u) for cond in FACTOR_CONDS for l2 in FACTOR_L2 for u in factor_unregs(p)]


_FACTOR_REF = {}


def factor_reference(p, cond, l2, unreg, routes=False):
    """A + regulariser -> dict(ref [p] longdouble, kappa; with routes chol64, inv64): the regulariser is added in longdouble for the
    reference and in float64, as the device does, for the float64 routes."""
    k = (p, cond, l2, unreg)
    if k in _FACTOR_REF and (not routes or "chol64" in _FACTOR_REF[k]):
        return _FACTOR_REF[k]
    A = factor_matrix(p, cond)
    Hld = A.astype(np.longdouble)
    Hld[np.diag_indices(p)] += regulariser(p, l2, unreg)
    H64 = A.copy()
    H64[np.diag_indices(p)] += regulariser(p, l2, unreg, np.float64)
    v = variances_of([Hld], [H64], routes)
    _FACTOR_REF[k] = {name: (x[0] if name != "kappa" else float(x[0])) for name, x in v.items()}
    return _FACTOR_REF[k]


def padded(A, ld, fill=np.nan):
    """A in the top left of an [ld, ld] matrix of `fill`."""
    H = np.full((ld, ld), fill)
    H[:A.shape[0], :A.shape[0]] = A
    return H


# ---- case 2: the Hessian build (gdmix_fe_hessian_dense) ----------------------------------------------------------------------------------------
# name -> (d, n, structures). 'dense': local column 0 in every sample (more than VF_THREADS entries when n > 256; every sample in one
# column); 'straddle': sample 255 holds column 0 three times, samples 0 .. 254 once each, so the run of equal rows sits on entries 255, 256
# and 257 of its column: in two trips of the run-summing loop; 'dups': one sample with a column twice and one with a column three times;
# 'empty': the first, the last and every seventh sample without non-zeros.
BUILD_CASES = {"d5": (5, 600, ("dense", "dups")),
               "d127": (127, 300, ("dense", "straddle", "dups")),
               "d128": (128, 64, ("empty",)),
               "d129": (129, 300, ("empty", "dups")),
               "d300": (300, 64, ("dense",))}
BUILD_IC = (1, 0)


def build_weighted(name, ic):
    """With weights or without: alternating over the cases and the intercept, so that every d has both."""
    return (list(BUILD_CASES).index(name) + ic) % 2 == 1


_BUILD = {}


def build_batch(name, ic):
    """The one-entity batch of a build case (the same samples with and without an intercept; the weights differ)."""
    if (name, ic) in _BUILD:
        return _BUILD[(name, ic)]
    d, n, st = BUILD_CASES[name]
    rng = np.random.default_rng(d * 7 + n)
    rows = [np.zeros(0, np.int64) for _ in range(n)]
    cover = _cover(d, -(-d // (n // 2 - 1)), rng)                    # every column somewhere among the odd samples in front of the last
    for i in range(n):
        k = int(rng.integers(3, 9))
        rows[i] = rng.permutation(np.arange(1, d))[:min(k, d - 1)]
    for i, c in enumerate(cover):
        rows[2 * i + 1] = np.union1d(rows[2 * i + 1], c[c > 0])
    if "dense" in st:
        rows = [np.concatenate([[0], r[r > 0]]) for r in rows]
    else:
        rows[1] = np.union1d(rows[1], [0])
    if "straddle" in st:
        assert "dense" in st and n > VF_THREADS
        rows[255] = np.concatenate([[0], rows[255][rows[255] > 0][:2], [0], rows[255][rows[255] > 0][2:], [0]])
    if "dups" in st:
        a, c = 11, 23
        rows[a] = np.concatenate([rows[a], rows[a][-1:]])
        rows[c] = np.concatenate([rows[c][-1:], rows[c], rows[c][-1:]])
    if "empty" in st:
        for i in [0, n - 1] + list(range(14, n - 1, 14)):
            rows[i] = np.zeros(0, np.int64)
    b = _assemble([rows], d * 7 + n, weighted=build_weighted(name, ic))
    assert np.unique(b.col_global).size == d, (name, np.unique(b.col_global).size)
    _BUILD[(name, ic)] = b
    return b


def build_reference(name, ic, loss, theta):
    """-> (X~' D X~ [p, p] longdouble, the plain summation bound n 2^-53 sum|terms| [p, p]) of a build case at theta [p]."""
    b = build_batch(name, ic)
    X = dense_rows(b, 0, ic)
    D = entity_weights(b, 0, X, theta, loss)
    H = (X.T * D) @ X
    bound = b.N * U * ((np.abs(X).T * D) @ np.abs(X))
    return H, bound


def column_runs(b):
    """[(column entries, longest run of one sample, does a run of one sample span a multiple of VF_THREADS of its column)] per local column
    of a one-entity batch: what the run-summing loop of vf_build_kernel meets."""
    uniq, loc = np.unique(b.col_global, return_inverse=True)
    rows = np.repeat(np.arange(b.N), np.diff(b.row_nnz_ptr))
    out = []
    for c in range(uniq.size):
        r = np.sort(rows[loc.reshape(-1) == c], kind="stable")
        starts = np.flatnonzero(np.concatenate([[True], r[1:] != r[:-1]]))
        lens = np.diff(np.concatenate([starts, [r.size]]))
        spans = any((s // VF_THREADS) != ((s + l - 1) // VF_THREADS) for s, l in zip(starts, lens))
        out.append((int(r.size), int(lens.max()), bool(spans)))
    return out


# ---- case 4: the wavefront kernel's edges ------------------------------------------------------------------------------------------------------
WAVE_P = (1, 2, 63, 64, 65, 127, 128, 129, 640)
# distinct columns per entity, in batch order (large, small, large ...): with an intercept p = d + 1, without p = d; d = 0 is the entity
# of zero non-zeros with samples (p = 1 with an intercept, no coefficient without)
WAVE_D = (640, 1, 129, 0, 639, 2, 128, 62, 127, 63, 126, 64, 65)
WAVE_ROW_MAX = 32                 # the per-row pattern loop of the wavefront kernel is cubic in the row length
WAVE_M = (6, 7, 8, 9)             # row lengths m: (m + ic)^2 is 49 and 64 and 81 and 100 with an intercept, 36, 49, 64, 81 without
                                  # (63 is no square: 49 is the largest (m + ic)^2 below 64 lanes, 64 fills them, 81 takes a second trip)
WAVE_CASES = ((1, False), (1, True), (0, True), (0, False))      # (has_intercept, regularize_bias)


def _wave_entity(d, rng):
    """Rows of one entity of the wavefront batch and the names of what they show."""
    if d == 0:
        return [np.zeros(0, np.int64)] * 3, {"no_nonzeros"}
    rows, tags = _cover(d, 22, rng, fill=min(8, max(0, d - 22))), set()
    if d >= 12:
        for m in WAVE_M:
            rows.append(rng.permutation(d)[:m])
            tags.add(f"m{m}")
        c = rng.permutation(d)[:12]
        rows.append(np.concatenate([c[:9], c[3:4]]))                  # a column twice
        rows.append(np.concatenate([c[5:6], c[:10], c[5:6]]))         # a column three times
        tags |= {"twice", "thrice"}
    else:
        rows.append(np.array([d - 1, d - 1]))
        rows.append(np.array([0, 0, 0]))
        tags |= {"twice", "thrice"}
    rows = [np.zeros(0, np.int64)] + rows + [np.zeros(0, np.int64)]
    tags |= {"empty_first", "empty_last"}
    return rows, tags


_WAVE = {}


def wave_batch():
    """-> dict(b, d [E], tags [E] of sets): one batch of the entities of WAVE_D, weighted."""
    if not _WAVE:
        rng = np.random.default_rng(640)
        ents, tags = zip(*[_wave_entity(d, rng) for d in WAVE_D])
        _WAVE.update(b=_assemble(list(ents), 640, weighted=True), d=np.array(WAVE_D), tags=list(tags))
    return _WAVE


# ---- case 5: slot re-use and shrinking scratch -------------------------------------------------------------------------------------------------
SLOTS_E = 4200                    # more than two trips of VAR_SLOTS_MAX wavefronts
SLOTS_MAX_P = 40
FOUR_E, FOUR_P = 64, 64           # sixteen trips of four wavefronts

_SLOTS = {}


def slots_batch():
    """4 200 entities of 0 .. 39 columns (p <= 40 with the intercept), one to five samples of at most eight non-zeros: every wavefront of
    the 2 048 walks two or three of them, wider and narrower ones in turn in the same slot."""
    if "b" not in _SLOTS:
        rng = np.random.default_rng(4200)
        ents = []
        for e in range(SLOTS_E):
            d = int(rng.integers(0, SLOTS_MAX_P))
            if d == 0:
                ents.append([np.zeros(0, np.int64)] * int(rng.integers(1, 4)))
                continue
            rows = _cover(d, 8, rng)
            rows += [rng.permutation(d)[:min(d, int(rng.integers(1, 9)))] for _ in range(int(rng.integers(0, 3)))]
            ents.append(rows)
        _SLOTS["b"] = _assemble(ents, 4200, weighted=False)
    return _SLOTS["b"]


_FOUR = {}


def four_slot_batch():
    """64 entities of p = 64 (63 columns and the intercept), eight samples of 24 non-zeros: the batch's own scratch, (Z + 1) 8 bytes,
    is below four slots of var_full_slot_doubles(64), so the context's scratch is the one that counts."""
    if "b" not in _FOUR:
        rng = np.random.default_rng(64)
        ents = [_cover(FOUR_P - 1, 8, rng, fill=16) for _ in range(FOUR_E)]
        _FOUR["b"] = _assemble(ents, 64, weighted=False)
    return _FOUR["b"]


# ---- case 6: the hand-over at VAR_FULL_MAX_P and the tile edges above it -----------------------------------------------------------------------
HAND_OVER_P = (2113, 2049, 2112)       # whole-device entities, a larger one in front of a smaller one
HAND_OVER_SMALL_D = (5, 40, 1)         # a small entity behind each
HAND_OVER_N = 128
AT_CAP_P = (VAR_FULL_MAX_P, VAR_FULL_MAX_P + 1)     # the wavefront kernel's last size and the whole device's first, one batch, no intercept


def _wide_entity(d, rng):
    """HAND_OVER_N samples that hold every one of d columns once: 16 or 17 distinct columns each, scattered over all tiles."""
    lo = d // HAND_OVER_N
    sizes = np.full(HAND_OVER_N, lo)
    sizes[:d - lo * HAND_OVER_N] += 1
    assert set(sizes.tolist()) <= {16, 17} and sizes.sum() == d
    return np.split(rng.permutation(d), np.cumsum(rng.permutation(sizes))[:-1])


_HAND = {}


def hand_over_batch(ic):
    """Entities of HAND_OVER_P coefficients (d = p - ic columns) with small ones between: d = 2 048 occurs with the intercept, as p = 2 049."""
    if ic not in _HAND:
        rng = np.random.default_rng(2048 + ic)
        ents = []
        for p, ds in zip(HAND_OVER_P, HAND_OVER_SMALL_D):
            ents.append(_wide_entity(p - ic, rng))
            ents.append(_cover(ds, 8, rng) + [np.zeros(0, np.int64)])
        _HAND[ic] = _assemble(ents, 2048 + ic, weighted=ic == 0)
    return _HAND[ic]


def at_cap_batch(p_wave=VAR_FULL_MAX_P):
    """No intercept: an entity of p_wave columns (the wavefront kernel), a small one, an entity of VAR_FULL_MAX_P + 1 (the whole device)."""
    if ("cap", p_wave) not in _HAND:
        rng = np.random.default_rng(p_wave)
        lo = p_wave // HAND_OVER_N
        first = np.split(rng.permutation(p_wave), np.arange(lo, p_wave, lo)[:HAND_OVER_N - 1])
        ents = [first, _cover(3, 8, rng), _wide_entity(AT_CAP_P[1], rng)]
        _HAND[("cap", p_wave)] = _assemble(ents, p_wave, weighted=False)
    return _HAND[("cap", p_wave)]


def beyond_batch():
    """One entity, one sample, VAR_FULL_BIG_MAX_P columns: with the intercept max_p is one past what FULL takes."""
    return _assemble([[np.arange(VAR_FULL_BIG_MAX_P)]], 1, weighted=False)


# ---- r_ref ---------------------------------------------------------------------------------------------------------------------------------------
def small_references(routes=True):
    """Every small case of the suite with its two float64 routes: [(name, ref [p] longdouble, kappa, chol64 [p], inv64 [p])]."""
    out = []
    for p in FACTOR_P:
        for cond, l2, u in factor_cases(p):
            r = factor_reference(p, cond, l2, u, routes)
            out.append((f"factor p={p} {cond} l2={l2} unreg={u}", r["ref"], r["kappa"], r.get("chol64"), r.get("inv64")))
    batches = [("wave", wave_batch()["b"], WAVE_CASES), ("slots", slots_batch(), ((1, False),)), ("four", four_slot_batch(), ((1, False),))]
    for key, b, cases in batches:
        for ic, rb in cases:
            for loss in LOSSES:
                r = reference(key, b, loss, L2, ic, rb, routes)
                cp = r["coef_ptr"]
                for e in range(b.E):
                    if 0 < r["p"][e] <= LD_MAX_P:
                        s = slice(cp[e], cp[e + 1])
                        out.append((f"{key} entity {e} p={r['p'][e]} {loss} ic={ic} rb={rb}", r["var"][s], r["kappa"][e],
                                    r["chol64"][s] if routes else None, r["inv64"][s] if routes else None))
    return out


def measure_r_ref():
    """-> (r_ref, the case that reaches it, [(name, kappa, ratio of the Cholesky route, ratio of np.linalg.inv)])."""
    rows = [(name, kappa, law_ratio(c, ref, kappa), law_ratio(i, ref, kappa)) for name, ref, kappa, c, i in small_references()]
    worst = max(rows, key=lambda r: max(r[2], r[3]))
    return max(worst[2], worst[3]), worst[0], rows
