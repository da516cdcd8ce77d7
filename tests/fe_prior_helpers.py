"""Shared by tests/test_fe_prior_host.py (CPU) and tests/test_gpu_fe_prior.py (GPU): the fixed effect's incremental training
(include/gdmix_fe.h, "incremental training") restated in numpy, dense and in fp64.

    F(theta) = sum_i w_i l(y_i, x_i . w + b + offset_i) + (l2/2) sum_{j in R} (theta_j - mu_j)^2 / v_j        theta = [w (D), b]
    R = every j < D, and the intercept iff regularize_bias;  l = logistic loss, or (z - y)^2 for the squared loss

  * case:            a seeded shard with a prior: columns no sample touches, defaulted coefficients, a sharp intercept prior;
  * objective:       the exact F, its gradient and its Hessian;
  * newton:          the minimiser theta* by Newton's method from mu (at most 60 steps);
  * ridge:           the closed-form minimiser for the squared loss (the cross-check of newton);
  * phi_objective:   F and its gradient in phi = (theta - mu) / s, what the optimiser works in;
  * variances:       diag((H + l2 Lambda_R + 1e-12 Lambda)^-1), Lambda = diag(1 / v), and its SIMPLE form on the per-entry diagonal.
"""
import numpy as np

SHAPES = [(400, 5, 300, 20), (3000, 6, 500, 40)]     # (n, k, D, absent): more than one virtual block of 256 coefficients, untouched columns
L2 = 10.0


def sigmoid(z):
    return 0.5 * (1.0 + np.tanh(0.5 * z))


class Case:
    pass


def case(seed, n, k, D, absent, linear, has_intercept=True):
    rng = np.random.default_rng(seed)
    c = Case()
    c.n, c.k, c.D, c.absent, c.linear, c.ic = n, k, D, absent, bool(linear), 1 if has_intercept else 0
    col = rng.integers(0, D - absent, (n, k))
    val = rng.standard_normal((n, k)).astype(np.float32)
    truth = 0.5 * rng.standard_normal(D + 1)
    offset = (0.2 * rng.standard_normal(n)).astype(np.float32)
    if not has_intercept:
        truth[D] = 0.0
    z = (val.astype(np.float64) * truth[col]).sum(axis=1) + truth[D] + offset
    if linear:
        y = (z + 0.3 * rng.standard_normal(n)).astype(np.float32)
    else:
        y = (rng.random(n) < sigmoid(z)).astype(np.float32)
    weight = (0.5 + rng.random(n)).astype(np.float32)
    mu = truth + 0.3 * rng.standard_normal(D + 1)
    v = np.exp(rng.uniform(np.log(1e-4), np.log(10.0), D + 1))
    none = rng.random(D + 1) < 1.0 / 3.0
    mu[none], v[none] = 0.0, 1.0
    mu[D], v[D] = truth[D] + 0.05, 1e-3
    P = D + c.ic
    c.row_nnz_ptr = np.arange(n + 1, dtype=np.int64) * k
    c.col, c.val = col.astype(np.int64).ravel(), val.ravel()
    c.y, c.offset, c.weight = y, offset, weight
    c.mu, c.v = mu[:P].copy(), v[:P].copy()
    X = np.zeros((n, P))
    np.add.at(X, (np.repeat(np.arange(n), k), c.col), c.val.astype(np.float64))
    if c.ic:
        X[:, D] = 1.0
    c.X = X
    return c


def reg_mask(c, regularize_bias):
    r = np.ones(c.D + c.ic)
    if c.ic and not regularize_bias:
        r[c.D] = 0.0
    return r


def scale(c, regularize_bias):
    """s = sqrt(v); 1 for an unregularised intercept, which has no penalty."""
    s = np.sqrt(c.v)
    if c.ic and not regularize_bias:
        s[c.D] = 1.0
    return s


def data_terms(c, theta, hessian=True):
    """(loss, gradient, Hessian | None) of the data term at theta."""
    X = c.X
    y, off, w = (a.astype(np.float64) for a in (c.y, c.offset, c.weight))
    z = X @ theta + off
    if c.linear:
        return np.sum(w * (z - y) ** 2), X.T @ (2.0 * w * (z - y)), 2.0 * (X.T * w) @ X if hessian else None
    rho = sigmoid(z)
    return np.sum(w * (np.logaddexp(0.0, z) - y * z)), X.T @ (w * (rho - y)), (X.T * (w * rho * (1.0 - rho))) @ X if hessian else None


def logistic_curvature(c, theta):
    """X~' D X~, D_i = w_i rho_i (1 - rho_i): what the variance modes are defined on, whatever the loss."""
    rho = sigmoid(c.X @ theta + c.offset.astype(np.float64))
    return (c.X.T * (c.weight.astype(np.float64) * rho * (1.0 - rho))) @ c.X


def objective(c, theta, l2, regularize_bias, hessian=True):
    """-> (F, grad F, Hessian of F | None) in fp64."""
    lam = l2 * reg_mask(c, regularize_bias) / c.v
    f, g, H = data_terms(c, theta, hessian)
    d = theta - c.mu
    return f + 0.5 * np.sum(lam * d * d), g + lam * d, H + np.diag(lam) if hessian else None


def newton(c, l2, regularize_bias, steps=60):
    """theta* by Newton from mu (F is strictly convex for l2 > 0 and a regularised or data-carrying intercept)."""
    theta = c.mu.copy()
    s = scale(c, regularize_bias)
    for _ in range(steps):
        _, g, H = objective(c, theta, l2, regularize_bias)
        step = np.linalg.solve(H, g)
        theta = theta - step
        if np.max(np.abs(step) / s) <= 1e-15:      # at the rounding floor: further steps only repeat it
            break
    return theta


_CACHE = {}


def case_and_minimiser(seed, shape, linear, regularize_bias, l2=L2, has_intercept=True):
    """(case, theta*) computed once per process and shared by the tests; neither is to be modified."""
    key = (seed, tuple(shape), bool(linear), bool(regularize_bias), l2, has_intercept)
    if key not in _CACHE:
        c = case(seed, *shape, linear, has_intercept=has_intercept)
        _CACHE[key] = (c, newton(c, l2, regularize_bias))
    return _CACHE[key]


def intercept_only(c):
    """The model without a feature bag on c's samples: the intercept alone, with its prior."""
    d = Case()
    d.__dict__.update(c.__dict__)
    d.D, d.ic, d.absent = 0, 1, 0
    d.X = np.ones((c.n, 1))
    d.mu, d.v = c.mu[-1:].copy(), c.v[-1:].copy()
    return d


def with_prior(c, mu, v):
    """c's data under another prior."""
    d = Case()
    d.__dict__.update(c.__dict__)
    d.mu, d.v = np.asarray(mu, np.float64).copy(), np.asarray(v, np.float64).copy()
    return d


def rows_of(c, rows):
    """(row_nnz_ptr, col, val, y, offset, weight) of a subset of c's samples: a worker's shard."""
    k = c.k
    nz = (np.asarray(rows)[:, None] * k + np.arange(k)[None, :]).ravel()
    return np.arange(len(rows) + 1, dtype=np.int64) * k, c.col[nz], c.val[nz], c.y[rows], c.offset[rows], c.weight[rows]


def ridge(c, l2, regularize_bias):
    """argmin F for the squared loss: (2 X~' W X~ + l2 R / v) theta = 2 X~' W (y - offset) + l2 R mu / v."""
    assert c.linear
    lam = l2 * reg_mask(c, regularize_bias) / c.v
    w = c.weight.astype(np.float64)
    A = 2.0 * (c.X.T * w) @ c.X + np.diag(lam)
    return np.linalg.solve(A, 2.0 * c.X.T @ (w * (c.y.astype(np.float64) - c.offset.astype(np.float64))) + lam * c.mu)


def phi_objective(c, l2, regularize_bias):
    """phi -> (F, grad_phi F): the function the optimiser minimises, from phi = 0."""
    s = scale(c, regularize_bias)

    def fun(phi):
        f, g, _ = objective(c, c.mu + s * phi, l2, regularize_bias, hessian=False)
        return f, s * g
    return fun, s


def simple_diagonal(c, theta):
    """What SIMPLE calls the diagonal: sum over the ENTRIES of a column of val^2 d_i, intercept sum_i d_i — the reference's and the device's
    per-entry sum (tests/test_fixed_effect.py, test_device_hessian_diagonal_and_simple_variance). It is diag(X~' D X~) except where a row
    names a column twice — case() draws columns with replacement, a few rows of every case do —: there the dense X holds the sum of the
    two values and its square carries their cross term, which the per-entry sum does not."""
    rho = sigmoid(c.X @ theta + c.offset.astype(np.float64))
    d = c.weight.astype(np.float64) * rho * (1.0 - rho)
    if c.D == 0:
        return np.array([d.sum()])
    rows = np.repeat(np.arange(c.n), c.k)
    h = np.bincount(c.col, weights=c.val.astype(np.float64) ** 2 * d[rows], minlength=c.D)
    return np.concatenate([h, [d.sum()]]) if c.ic else h


def variances(c, theta, l2, regularize_bias, full):
    """Posterior variances at theta. FULL: diag((H + l2 Lambda_R + 1e-12 Lambda)^-1), H = X~' D X~ (logistic_curvature), Lambda = diag(1 / v)
    (an unregularised intercept: v = 1). SIMPLE: 1 / (h_j + (l2 [j in R] + 1e-12) / v_j), h = simple_diagonal."""
    s = scale(c, regularize_bias)
    lam = (l2 * reg_mask(c, regularize_bias) + 1e-12) / (s * s)
    if full:
        return np.diagonal(np.linalg.inv(logistic_curvature(c, theta) + np.diag(lam))).copy()
    return 1.0 / (simple_diagonal(c, theta) + lam)
