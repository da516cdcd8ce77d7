"""The tests' own statement of the random effect's elastic net (include/gdmix_re.h, "elastic net"): for one entity of n samples, theta in
local index space, the intercept first,

    F(theta) = (1/n) ( sum_i w_i l(y_i, x_i . theta + offset_i) + (l2/2) |theta_R|^2 + l1 |theta_R|_1 )

* EntityProblem: fe_l1_helpers.Problem with the 1/n scaling, the intercept in front and sample weights; owlqn(), reference_fit() and the
  pseudo-gradient are that module's, run on it unchanged,
* seeded batch generators,
* check_batch(): the bars of fe_l1_helpers.check_against_reference taken per entity, with modulus l2 / n in the distance bound:
      |fval - F_numpy(theta)| <= 1e-9 |F|;   fval - F_ref <= 1e-9 |F_ref|;   identical support outside the left-out set;
      |theta - theta_ref| <= (|pg(theta)| + |pg(theta_ref)|) n / l2      (a theorem where every coefficient is regularised and l2 > 0).
  The cap on left-out coefficients is a condition on the inputs: at most 1 per entity and at most 0.5 % of a batch's coefficients.
These bars are about the minimiser: the tests that use them solve with TIGHT (pgtol 1e-9, ftol 1e-14), not with the stage's tolerances.
tests/test_re_l1_host.py asserts that the restatement alone ends at most 1e-10 |F_ref| above the reference on every committed case, and
the cap for the reference alone: the inputs, not the device, keep within the bars.
"""
import dataclasses
import functools

import numpy as np
import scipy.sparse as sp

import fe_l1_helpers as F
from gdmix_amd.batch import RawBatch

LOSSES = F.LOSSES
TIGHT = dict(pgtol=1e-9, ftol=1e-14, max_iter=2000, maxfun=15000, maxls=20)
RESTATEMENT_BAR = 1e-10      # what the restatement alone may end above F_ref, relative (the device's bar is 1e-9)
MAX_LEFT_OUT_ENTITY = 1
MAX_LEFT_OUT_SHARE = 0.005
ARMIJO_MARGIN = 1e-10        # an entity whose restatement has an Armijo test closer than this x max(|F|, 1) is excused from count equality
MAX_EXCUSED_SHARE = 0.01


class EntityProblem(F.Problem):
    """One entity's objective in the conventions of gdmix_re_opts. X has the intercept column in front (when there is one); l1 and l2 are
    the weights of the header's formula: the base class sees them, and the data term, divided by n."""

    def __init__(self, loss, X, y, off, w, l1, l2, has_intercept=True, regularize_bias=True):
        n = X.shape[0]
        mask = np.ones(X.shape[1])
        if has_intercept and not regularize_bias:
            mask[0] = 0.0
        super().__init__(loss, X, y, off, l1 / n, l2 / n, mask)
        self.n, self.w = n, None if w is None else np.asarray(w, np.float64)
        self.raw_l1, self.raw_l2 = float(l1), float(l2)

    def data(self, th):
        if self.w is None:
            f, g = super().data(th)
            return f / self.n, g / self.n
        z = self.X @ th + self.off      # the weighted form of Problem.data
        if self.loss == "logistic":
            f = np.sum(self.w * (np.maximum(z, 0.0) - z * self.y + np.log1p(np.exp(-np.abs(z)))))
            r = self.w * (1.0 / (1.0 + np.exp(-z)) - self.y)
        elif self.loss == "squared":
            e = z - self.y
            f, r = np.sum(self.w * e * e), 2.0 * self.w * e
        else:
            e = np.exp(z)
            f, r = np.sum(self.w * (e - self.y * z)), self.w * (e - self.y)
        return f / self.n, (self.XT @ r) / self.n

    def residual(self, th):
        """r_i = w_i dl/dz at th (the data gradient is X' r / n)."""
        z = self.X @ th + self.off
        w = 1.0 if self.w is None else self.w
        if self.loss == "logistic":
            return w * (1.0 / (1.0 + np.exp(-z)) - self.y)
        return 2.0 * w * (z - self.y) if self.loss == "squared" else w * (np.exp(z) - self.y)

    def pg_rounding(self, th):
        """A bound on what rounding leaves in the pseudo-gradient numpy computes at th, per component: a sum of n + 2 rounded terms."""
        terms = (abs(self.X).T @ np.abs(self.residual(th))) / self.n + self.mask * (self.l2 * np.abs(th) + self.l1)
        return (self.n + 2) * np.finfo(float).eps * terms

    def curvature(self, th):
        """D_i of the variances at th: w rho (1 - rho) | 2 w | w exp(z)."""
        z = self.X @ th + self.off
        w = np.ones(self.n) if self.w is None else self.w
        if self.loss == "logistic":
            rho = 1.0 / (1.0 + np.exp(-z))
            return w * rho * (1.0 - rho)
        return 2.0 * w if self.loss == "squared" else w * np.exp(z)

    def variance(self, th, mode):
        """SIMPLE (1) / FULL (2) variances of the smooth part at th, not divided by n (include/gdmix_re.h, gdmix_re_opts)."""
        D = self.curvature(th)
        reg = self.raw_l2 * self.mask
        if mode == 1:
            return 1.0 / (np.asarray(self.X.multiply(self.X).T @ D).ravel() + reg + 1e-12)
        Xd = np.asarray(self.X.todense())
        return np.diag(np.linalg.inv((Xd.T * D) @ Xd + np.diag(reg + 1e-12)))


# ---- batches ----------------------------------------------------------------------------------------------------------------------------
def _labels(rng, loss, z):
    if loss == "logistic":
        return (rng.random(z.size) < 1.0 / (1.0 + np.exp(-z))).astype(np.float32)
    if loss == "squared":
        return (z + 0.5 * rng.standard_normal(z.size)).astype(np.float32)
    return rng.poisson(np.exp(np.minimum(z, 3.0))).astype(np.float32)


def make_batch(loss, shapes, seed, D=400, weights=False, dup_prob=0.05):
    """shapes: per entity (n, k_max, d_max): n samples of 0 .. k_max non-zeros drawn from d_max of the D global features (k_max = 0: an entity
    without features). Duplicate (row, column) cells with probability dup_prob per non-zero; offsets; labels by `loss` from a sparse w*."""
    rng = np.random.default_rng(seed)
    w_star = np.where(rng.random(D) < 0.4, 0.8 * rng.standard_normal(D), 0.0)
    erp, rnp, cols, vals, ys, offs = [0], [0], [], [], [], []
    for (n, k_max, d_max) in shapes:
        own = rng.choice(D, size=max(1, min(d_max, D)), replace=False)
        bias = 0.5 * rng.standard_normal()
        for i in range(n):      # (the first sample has a non-zero, so that only k_max = 0 makes an entity without features)
            k = int(rng.integers(0 if i > 0 else 1, k_max + 1)) if k_max > 0 else 0
            c = rng.choice(own, size=k, replace=k > own.size)
            if k > 1 and rng.random() < dup_prob * k:
                c[-1] = c[0]
            v = (0.6 * rng.standard_normal(k)).astype(np.float32)
            o = np.float32(0.3 * rng.standard_normal())
            cols.append(c)
            vals.append(v)
            offs.append(o)
            ys.append(float(v.astype(np.float64) @ w_star[c]) + float(o) + bias)
            rnp.append(rnp[-1] + k)
        erp.append(erp[-1] + n)
    z = np.array(ys)
    N = z.size
    return RawBatch(ent_row_ptr=np.array(erp), row_nnz_ptr=np.array(rnp), col_global=np.concatenate(cols + [np.zeros(0, np.int64)]).astype(np.int64),
                    val=np.concatenate(vals + [np.zeros(0, np.float32)]), y=_labels(rng, loss, z), offset=np.array(offs, np.float32),
                    weight=(0.5 + rng.random(N)).astype(np.float32) if weights else None, binary_labels=loss == "logistic")


def mixed_shapes(E, seed, intercept_only=True):
    """n from 1 to 64, p from 1 (an entity without features, when asked for) to more than 64 coefficients (lanes stride)."""
    rng = np.random.default_rng([seed, 7])
    shapes = [(1, 1, 1), (1, 4, 6), (2, 3, 5), (64, 6, 150), (40, 5, 120), (33, 2, 70)]
    if intercept_only:
        shapes += [(5, 0, 1), (1, 0, 1)]
    while len(shapes) < E:
        shapes.append((int(rng.integers(1, 65)), int(rng.integers(1, 7)), int(rng.integers(1, 40))))
    return shapes[:E]


L1, L2 = 0.5, 1.0      # alpha = 1/3, lambda = 1.5
# The option sets of the comparisons. distance: the bound is a theorem (every coefficient regularised). An unregularised intercept needs
# entities that have a minimiser at all: eight samples or more, and labels that are not all equal (not all zero for counts).
VARIANTS = {"plain": dict(weights=False, has_intercept=True, regularize_bias=True, distance=True),
            "weights": dict(weights=True, has_intercept=True, regularize_bias=True, distance=True),
            "no_intercept": dict(weights=False, has_intercept=False, regularize_bias=True, distance=True),
            "free_intercept": dict(weights=True, has_intercept=True, regularize_bias=False, distance=False)}
# seeds chosen so that the restatement alone ends within RESTATEMENT_BAR of the reference and the reference meets the left-out cap
# (tests/test_re_l1_host.py asserts both for every committed case)
SEEDS = {}


@functools.lru_cache(maxsize=None)
def mixed_batch(loss, variant="plain", E=40):
    v = VARIANTS[variant]
    seed = SEEDS.get((loss, variant), 300 + 10 * LOSSES.index(loss) + list(VARIANTS).index(variant))
    if v["regularize_bias"] or not v["has_intercept"]:
        return make_batch(loss, mixed_shapes(E, LOSSES.index(loss), v["has_intercept"]), seed=seed, weights=v["weights"])
    shapes = [(n + 7 if n < 8 else n, k, d) for (n, k, d) in mixed_shapes(E, LOSSES.index(loss), True)]
    b = make_batch(loss, shapes, seed=seed, weights=v["weights"])
    y = b.y.copy()
    for e in range(b.E):      # labels that are not all equal
        r0 = int(b.ent_row_ptr[e])
        y[r0], y[r0 + 1] = (1.0, 0.0) if loss != "squared" else (y[r0], y[r0 + 1])
    return dataclasses.replace(b, y=y)


@functools.lru_cache(maxsize=None)
def block_batch(loss, tiny=2100):
    """The mixed batch, one entity with more samples and more coefficients than the workgroup kernel has threads (256), and more tiny
    entities than its grid has workgroups (1 024 slots at most), so that slots are reused."""
    rng = np.random.default_rng(17)
    shapes = mixed_shapes(24, 5) + [(300, 8, 390)] + [(int(rng.integers(1, 4)), int(rng.integers(1, 3)), 3) for _ in range(tiny)]
    return make_batch(loss, shapes, seed=330 + LOSSES.index(loss))


def entity_problem(batch, e, loss, l1, l2, has_intercept=True, regularize_bias=True):
    """Entity e as an EntityProblem: local indices by np.unique (ascending global index, as the pack orders them), intercept first."""
    r0, r1 = int(batch.ent_row_ptr[e]), int(batch.ent_row_ptr[e + 1])
    z0, z1 = int(batch.row_nnz_ptr[r0]), int(batch.row_nnz_ptr[r1])
    uniq, local = np.unique(batch.col_global[z0:z1], return_inverse=True)
    n, ic = r1 - r0, 1 if has_intercept else 0
    rows = np.repeat(np.arange(n), np.diff(batch.row_nnz_ptr[r0:r1 + 1]))
    cols, vals = local + ic, batch.val[z0:z1].astype(np.float64)
    if ic:
        rows, cols, vals = np.concatenate([np.arange(n), rows]), np.concatenate([np.zeros(n, np.int64), cols]), np.concatenate([np.ones(n), vals])
    X = sp.csr_matrix((vals, (rows, cols)), shape=(n, uniq.size + ic))
    X.sum_duplicates()
    w = None if batch.weight is None else batch.weight[r0:r1]
    return EntityProblem(loss, X, batch.y[r0:r1], batch.offset[r0:r1], w, l1, l2, has_intercept, regularize_bias)


def coef_ptr(batch, has_intercept=True):
    ic = 1 if has_intercept else 0
    out = np.zeros(batch.E + 1, np.int64)
    for e in range(batch.E):
        r0, r1 = int(batch.ent_row_ptr[e]), int(batch.ent_row_ptr[e + 1])
        out[e + 1] = out[e] + ic + np.unique(batch.col_global[int(batch.row_nnz_ptr[r0]):int(batch.row_nnz_ptr[r1])]).size
    return out


_PROBLEMS, _REFERENCES = {}, {}


def problems(key, batch, loss, l1, l2, has_intercept=True, regularize_bias=True, entities=None):
    """The entities' problems, made once per key (key names the batch and the options)."""
    if key not in _PROBLEMS:
        ents = range(batch.E) if entities is None else entities
        _PROBLEMS[key] = {int(e): entity_problem(batch, int(e), loss, l1, l2, has_intercept, regularize_bias) for e in ents}
    return _PROBLEMS[key]


def references(key, pbs):
    """reference_fit of every problem, computed once per key and shared; the arrays are read-only."""
    if key not in _REFERENCES:
        out = {}
        for e, pb in pbs.items():
            th, f = F.reference_fit(pb)
            th.setflags(write=False)
            out[e] = (th, f)
        _REFERENCES[key] = out
    return _REFERENCES[key]


BLOCK_SAMPLE_STEP = 33      # of the block batch's tiny entities every 33rd is held to the reference (all of its first 25: the mixed ones and the large one)


def block_sample(b):
    return list(range(25)) + list(range(25, b.E, BLOCK_SAMPLE_STEP))


def case(loss, variant="plain", which="mixed"):
    """-> (problems, references, batch, option set) of a committed case, shared by every test that asks."""
    v = VARIANTS[variant]
    b = mixed_batch(loss, variant) if which == "mixed" else block_batch(loss)
    key = (which, loss, variant)
    pbs = problems(key, b, loss, L1, L2, v["has_intercept"], v["regularize_bias"], entities=None if which == "mixed" else block_sample(b))
    return pbs, references(key, pbs), b, v


_ONE = {}


def one_iteration(loss, warm):
    """first_iteration() of every entity of the plain mixed case, cold or from half the reference -> {e: (status, nit, nfev, F, margin)}."""
    if (loss, warm) not in _ONE:
        pbs, refs, _, _ = case(loss, "plain", "mixed")
        _ONE[(loss, warm)] = {e: first_iteration(pb, 0.5 * refs[e][0] if warm else None) for e, pb in pbs.items()}
    return _ONE[(loss, warm)]


def restatement(pb, theta0=None, m=10, **kw):
    """fe_l1_helpers.owlqn on an entity's problem -> (theta, F, status, nit, nfev)."""
    return F.owlqn(pb, theta0=theta0, m=m, **dict(TIGHT, **kw))


def left_out(pb, theta_ref):
    g_ref = pb.smooth(theta_ref)[1]
    lam = pb.l1 * pb.mask
    return ((theta_ref == 0) & (np.abs(np.abs(g_ref) - lam) < F.SUPPORT_SLACK * lam)) | ((theta_ref != 0) & (np.abs(theta_ref) < F.SMALL_COEFFICIENT))


def distance_bound(pb, th, th_ref):
    """(|pg(theta)| + |pg(theta_ref)|) / mu, mu = l2 / n: the theorem is about the exact pseudo-gradients, so what rounding leaves in the
    computed ones is added to their norms (at a common zero of both the two points may still differ in their last bits)."""
    return (np.linalg.norm(pb.pseudo_gradient(th)) + np.linalg.norm(pb.pg_rounding(th)) +
            np.linalg.norm(pb.pseudo_gradient(th_ref)) + np.linalg.norm(pb.pg_rounding(th_ref))) / pb.l2


def check_left_out_cap(pbs, refs):
    """The cap on left-out coefficients, for the reference alone: a condition the committed inputs meet."""
    total = coefs = 0
    for e, pb in pbs.items():
        k = int(left_out(pb, refs[e][0]).sum())
        assert k <= MAX_LEFT_OUT_ENTITY, (e, k)
        total, coefs = total + k, coefs + refs[e][0].size
    print(f"left out: {total} of {coefs} coefficients")
    assert total <= MAX_LEFT_OUT_SHARE * coefs, (total, coefs)
    return total


def check_batch(pbs, refs, theta, fval, cp, distance=True, what=""):
    """The bars, per entity. theta [P], fval [E]: a fit's (the device's, or the restatement's); cp: coefficient offsets per entity. Prints the
    worst figures before it asserts. distance: the bound is a theorem (every coefficient regularised, l2 > 0)."""
    worst = dict(f_np=0.0, above=-np.inf, dist=0.0)
    problems_, n_left = [], 0
    for e, pb in pbs.items():
        th = np.asarray(theta[int(cp[e]):int(cp[e + 1])], np.float64)
        th_ref, f_ref = refs[e]
        f, F_np = float(fval[e]), pb.F(th)
        lo = left_out(pb, th_ref)
        n_left += int(lo.sum())
        mism = np.flatnonzero(((th != 0) != (th_ref != 0)) & ~lo)
        a, b = abs(f - F_np) / max(abs(F_np), 1e-300), (f - f_ref) / max(abs(f_ref), 1e-300)
        worst["f_np"], worst["above"] = max(worst["f_np"], a), max(worst["above"], b)
        if not abs(f - F_np) <= 1e-9 * abs(F_np):
            problems_.append(f"entity {e}: fval {f!r}, numpy at theta {F_np!r}")
        if not f - f_ref <= 1e-9 * abs(f_ref):
            problems_.append(f"entity {e}: fval {f!r} is {(f - f_ref) / abs(f_ref):.3e} above the reference {f_ref!r}")
        if mism.size:
            problems_.append(f"entity {e}: support differs at {mism.tolist()}: {th[mism].tolist()} reference {th_ref[mism].tolist()}")
        if distance:
            dist = np.linalg.norm(th - th_ref)
            bound = distance_bound(pb, th, th_ref)
            worst["dist"] = max(worst["dist"], dist / max(bound, 1e-300))
            if not dist <= bound:
                problems_.append(f"entity {e}: |theta - theta_ref| {dist:.3e} above the bound {bound:.3e}")
    print(f"{what}: {len(pbs)} entities; worst |fval - F_numpy| / |F| {worst['f_np']:.3e}, worst (fval - F_ref) / |F_ref| {worst['above']:.3e}, "
          f"worst distance / bound {worst['dist']:.3e}, left out {n_left}, {len(problems_)} problems")
    assert not problems_, problems_[:6]
    return worst


# ---- one iteration: the counts of the restatement and how close its Armijo tests were ----------------------------------------------------
class _Recording:
    """A problem that remembers the points it was evaluated at."""

    def __init__(self, pb):
        self.pb, self.points = pb, []

    def __getattr__(self, k):
        return getattr(self.pb, k)

    def smooth(self, th):
        self.points.append(np.array(th))
        return self.pb.smooth(th)

    def pseudo_gradient(self, th, g=None):
        return self.pb.pseudo_gradient(th, g)


def first_iteration(pb, theta0, m=10, **kw):
    """The restatement with max_iter = 1 -> (status, nit, nfev, F, smallest Armijo margin / max(|F|, 1)): every trial of the one iteration
    is tested against F(x0) + 1e-4 pg(x0)'(x(t) - x0), and the margin says how far from the edge the closest test was."""
    x0 = np.zeros(pb.X.shape[1]) if theta0 is None else np.asarray(theta0, np.float64)
    rec = _Recording(pb)
    _, Fv, status, nit, nfev = F.owlqn(rec, theta0=x0, m=m, **dict(TIGHT, **kw, max_iter=1))
    F0, pg0 = pb.F(x0), pb.pseudo_gradient(x0)
    margin = np.inf
    for xt in rec.points[1:]:
        margin = min(margin, abs(pb.F(xt) - (F0 + 1e-4 * (pg0 @ (xt - x0)))) / max(abs(F0), 1.0))
    return status, nit, nfev, Fv, margin


def lds_bytes(p, n, nnz, d, m, has_w):
    """The OWL-QN LDS footprint of an entity (csrc/re_owlqn.hip, owlqn_lds_bytes): the plain wavefront kernel's (csrc/re_internal.hpp,
    wave_lds_bytes) plus one coefficient vector, each rounded up to 16 bytes."""
    dbl = (5 + 2 * m) * p + n + 2 * m
    w32 = 4 * nnz + (n + 1) + (d + 1) + (3 if has_w else 2) * n
    plain = (dbl * 8 + w32 * 4 + 15) & ~15
    return (plain + 8 * p + 15) & ~15
