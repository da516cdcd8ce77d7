"""The tests' own statement of the fixed effect's L1 / elastic-net objective (include/gdmix_fe.h, "(ABI 23) L1 / elastic net"):

    F(theta) = sum_i l(y_i, x_i . w + b + offset_i) + (l2/2) |theta_R|^2 + l1 |theta_R|_1

* the cases (columns drawn as tests/test_gpu_fe_poisson.py draws them, a sparse w*),
* the numpy objective of the three losses and the pseudo-gradient,
* reference(): a ground truth that is independent of the algorithm — scipy's fmin_l_bfgs_b with bounds on the split problem
  theta = u - v, u, v >= 0, objective smooth(u - v) + l1 sum_R (u + v), factr = 10, pgtol = 1e-9. Its minimiser is the L1 problem's, and
  the bounds return exact zeros,
* owlqn(): a numpy restatement of the header's algorithm section (Andrew & Gao 2007),
* check_against_reference(): the bars a fit is held to against the reference.
"""
import functools

import numpy as np
import scipy.sparse as sp
from scipy.optimize import fmin_l_bfgs_b

LOSSES = ("logistic", "squared", "poisson")
MODEL_TYPE = {"logistic": "logistic_regression", "squared": "linear_regression", "poisson": "poisson_regression"}
SIZES = {"small": dict(n=600, k=8, D=50, seed=61, l1=3.0, l2=1.0),
         "wide": dict(n=20000, k=6, D=5000, seed=62, l1=1.5, l2=1.0)}
# the shapes of tests/step_edges_helpers.py, drawn by case() like the two above; a table of their own: nothing that is parametrised over SIZES grows
EDGE_SIZES = {"share29": dict(n=6000, k=6, D=7199, seed=71, l1=1.0, l2=1.0),
              "share33": dict(n=6000, k=6, D=8199, seed=72, l1=1.0, l2=1.0),
              "capped": dict(n=40000, k=8, D=123200, seed=73, l1=0.5, l2=1.0)}
FIT = dict(has_intercept=True, regularize_bias=True, m=10, max_iter=500, tolerance=1e-12)
PGTOL, MAXFUN, MAXLS = 1e-5, 15000, 20      # the solver's defaults (gdmix_amd.solver.SolverOptions)
SUPPORT_SLACK = 1e-3      # a zero of the reference with | |g_j| - l1 | < SUPPORT_SLACK l1 may be on either side of the support
SMALL_COEFFICIENT = 1e-4  # ... and so may a non-zero below the stage's own sparsity threshold
MAX_LEFT_OUT = 4


def shape(size):
    return SIZES[size] if size in SIZES else EDGE_SIZES[size]


@functools.lru_cache(maxsize=None)
def case(loss, size):
    """-> (row_nnz_ptr, col, val, y, offset, D, l1, l2): no weights, labels by `loss`."""
    c = shape(size)
    n, k, D = c["n"], c["k"], c["D"]
    rng = np.random.default_rng(c["seed"])
    col = rng.integers(0, D, (n, k)).astype(np.int64).ravel()
    val = (0.4 * rng.standard_normal(n * k)).astype(np.float32)
    off = (0.3 * rng.standard_normal(n)).astype(np.float32)
    w_star = np.where(rng.random(D) < 0.3, 0.6 * rng.standard_normal(D), 0.0)
    z = (val.astype(np.float64) * w_star[col]).reshape(n, k).sum(1) + off + 0.4
    if loss == "logistic":
        y = (rng.random(n) < 1.0 / (1.0 + np.exp(-z))).astype(np.float32)
    elif loss == "squared":
        y = (z + 0.5 * rng.standard_normal(n)).astype(np.float32)
    else:
        y = rng.poisson(np.exp(z)).astype(np.float32)
    return np.arange(n + 1, dtype=np.int64) * k, col, val, y, off, D, c["l1"], c["l2"]


def design(rp, col, val, D, has_intercept=True):
    X = sp.csr_matrix((val.astype(np.float64), col, rp), shape=(rp.size - 1, D))      # (duplicates of a cell are summed)
    return sp.hstack([X, sp.csr_matrix(np.ones((rp.size - 1, 1)))], format="csr") if has_intercept else X      # intercept last


class Problem:
    """The numpy objective of one case. mask: 1 on the regularised set R."""

    def __init__(self, loss, X, y, off, l1, l2, mask=None):
        self.loss, self.X, self.XT = loss, X, X.T.tocsr()
        self.y, self.off, self.l1, self.l2 = y.astype(np.float64), off.astype(np.float64), float(l1), float(l2)
        self.mask = np.ones(X.shape[1]) if mask is None else np.asarray(mask, np.float64)

    def data(self, th):
        """(value, gradient) of the data term, not divided by n."""
        z = self.X @ th + self.off
        if self.loss == "logistic":
            f = np.sum(np.maximum(z, 0.0) - z * self.y + np.log1p(np.exp(-np.abs(z))))
            r = 1.0 / (1.0 + np.exp(-z)) - self.y
        elif self.loss == "squared":
            e = z - self.y
            f, r = np.sum(e * e), 2.0 * e
        else:
            e = np.exp(z)
            f, r = np.sum(e - self.y * z), e - self.y
        return f, self.XT @ r

    def smooth(self, th):
        f, g = self.data(th)
        return f + 0.5 * self.l2 * np.sum(self.mask * th * th), g + self.l2 * self.mask * th

    def F(self, th):
        return self.smooth(th)[0] + self.l1 * np.sum(self.mask * np.abs(th))

    def pseudo_gradient(self, th, g=None):
        g = self.smooth(th)[1] if g is None else g
        lam = self.l1 * self.mask
        up, dn = g + lam, g - lam
        return np.where(th > 0, up, np.where(th < 0, dn, np.where(up < 0, up, np.where(dn > 0, dn, 0.0))))


@functools.lru_cache(maxsize=None)
def problem(loss, size):
    rp, col, val, y, off, D, l1, l2 = case(loss, size)
    return Problem(loss, design(rp, col, val, D), y, off, l1, l2)


def reference_fit(pb):
    """-> (theta, F) of the split problem."""
    P = pb.X.shape[1]
    lam = pb.l1 * pb.mask

    def fg(uv):
        u, v = uv[:P], uv[P:]
        f, g = pb.smooth(u - v)
        return f + np.sum(lam * (u + v)), np.concatenate([g + lam, -g + lam])
    uv, _, _ = fmin_l_bfgs_b(fg, np.zeros(2 * P), bounds=[(0.0, None)] * (2 * P), m=10, factr=10.0, pgtol=1e-9, maxiter=15000, maxfun=15000)
    theta = uv[:P] - uv[P:]
    return theta, pb.F(theta)


@functools.lru_cache(maxsize=None)
def reference(loss, size):
    """Computed once per session and shared; the arrays are read-only."""
    theta, f = reference_fit(problem(loss, size))
    theta.setflags(write=False)
    return theta, f


def owlqn(pb, theta0=None, m=10, max_iter=500, ftol=1e-12, pgtol=PGTOL, maxfun=MAXFUN, maxls=MAXLS):
    """The algorithm section of the header, restated -> (theta, F, status, nit, nfev)."""
    x = np.zeros(pb.X.shape[1]) if theta0 is None else np.array(theta0, np.float64)
    fs, g = pb.smooth(x)
    lam = pb.l1 * pb.mask
    F = fs + np.sum(lam * np.abs(x))
    nfev, nit, pairs = 1, 0, []
    pg = pb.pseudo_gradient(x, g)
    if np.max(np.abs(pg)) <= pgtol:
        return x, F, 0, nit, nfev
    while True:
        if pairs:      # two-loop recursion on pg
            q, alphas = pg.copy(), []
            for s, y in reversed(pairs):
                a = (s @ q) / (s @ y)
                alphas.append(a)
                q -= a * y
            s, y = pairs[-1]
            q *= (s @ y) / (y @ y)
            for (s, y), a in zip(pairs, reversed(alphas)):
                q += (a - (y @ q) / (s @ y)) * s
            d = -q
            d[d * pg >= 0] = 0.0
            t = 1.0
        else:
            d, t = -pg, 1.0 / np.sqrt(pg @ pg)
        xi = np.where(x != 0, np.sign(x), np.sign(-pg))
        rejected = 0
        while True:
            xt = x + t * d
            xt[np.sign(xt) != xi] = 0.0
            fs_t, g_t = pb.smooth(xt)
            F_t = fs_t + np.sum(lam * np.abs(xt))
            nfev += 1
            if F_t <= F + 1e-4 * (pg @ (xt - x)):
                break
            rejected += 1
            if rejected >= maxls:
                if not pairs:
                    return x, F, 4, nit, nfev
                pairs, rejected = [], 0
                d, t = -pg, 1.0 / np.sqrt(pg @ pg)
            else:
                t *= 0.5
        s, y = xt - x, g_t - g
        if s @ y > 2.2e-16 * (y @ y):
            pairs = (pairs + [(s, y)])[-m:]
        F_old, x, g, F = F, xt, g_t, F_t
        nit += 1
        pg = pb.pseudo_gradient(x, g)
        if np.max(np.abs(pg)) <= pgtol:
            return x, F, 0, nit, nfev
        if F_old - F <= ftol * max(abs(F_old), abs(F), 1.0):
            return x, F, 1, nit, nfev
        if nit >= max_iter:
            return x, F, 2, nit, nfev
        if nfev > maxfun:
            return x, F, 3, nit, nfev


def check_against_reference(pb, theta, fval, theta_ref, f_ref, what=""):
    """The bars of a fit against the reference; prints each figure before it asserts."""
    theta = np.asarray(theta, np.float64)
    F_np = pb.F(theta)
    g_ref = pb.smooth(theta_ref)[1]
    lam = pb.l1 * pb.mask
    left_out = ((theta_ref == 0) & (np.abs(np.abs(g_ref) - lam) < SUPPORT_SLACK * lam)) | ((theta_ref != 0) & (np.abs(theta_ref) < SMALL_COEFFICIENT))
    r_dev, r_ref = pb.pseudo_gradient(theta), pb.pseudo_gradient(theta_ref)
    dist, bound = np.linalg.norm(theta - theta_ref), (np.linalg.norm(r_dev) + np.linalg.norm(r_ref)) / pb.l2
    mism = np.flatnonzero(((theta != 0) != (theta_ref != 0)) & ~left_out)
    print(f"{what}: F {fval!r} numpy at theta {F_np!r} reference {f_ref!r} (F - F_ref) / |F_ref| {(fval - f_ref) / abs(f_ref):.3e}; non-zeros {np.count_nonzero(theta)} "
          f"reference {np.count_nonzero(theta_ref)}, left out {int(left_out.sum())}, support mismatches {mism.size}; |theta - theta_ref| {dist:.3e} bound {bound:.3e}")
    assert abs(fval - F_np) <= 1e-9 * abs(F_np)
    assert fval - f_ref <= 1e-9 * abs(f_ref)
    assert int(left_out.sum()) <= MAX_LEFT_OUT
    assert mism.size == 0, (mism, theta[mism], theta_ref[mism])
    assert dist <= bound      # strong convexity with modulus l2 (the intercept is regularised): a theorem, not a tolerance
