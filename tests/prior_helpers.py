"""Shared by tests/test_prior_host.py (CPU) and tests/test_gpu_prior.py (GPU): incremental training (include/gdmix_re.h, "incremental
training") restated in numpy. Test infrastructure: uses oracle/.

    F(theta) = (1/n) ( sum_i w_i l(z_i, y_i) + (l2/2) sum_{j regularised} (theta_j - mu_j)^2 / v_j ),   z = X~ theta + offset
    (v_0 = 1 for the intercept: the header's "The intercept")

  * map_prior_plain: the mapping of a prior model into a batch's index space with the defaults, in plain loops;
  * transform_raw: the transformed batch with the header's roundings — x' = (float)((double)x s), offset' = the fp64 sum rounded once;
  * restore: theta = mu + s phi, the threshold on theta, variance = s^2 var';
  * prior_objective_grad: the exact fp64 F and its gradient on the UNROUNDED data (re_linear_helpers.entity_dense);
  * ridge_with_prior: the closed-form minimiser of F for the squared loss.
"""
import numpy as np

from re_linear_helpers import entity_dense, reg_vector


def coef_ptr(pk, has_intercept):
    E = len(pk["ent_feat_ptr"]) - 1
    return np.asarray(pk["ent_feat_ptr"], np.int64) + np.arange(E + 1, dtype=np.int64) * (1 if has_intercept else 0)


def usable(v):
    """The default of a prior variance: 1 where it is missing (None or 0), not finite or <= 0."""
    v = 0.0 if v is None else float(v)
    return v if np.isfinite(v) and v > 0.0 else 1.0


def map_prior_plain(prior, entity_ids, unique_global, ent_feat_ptr, has_intercept):
    """prior: {entity id: (theta, variance | None, global feature indices)}, theta / variance intercept first when has_intercept.
    -> (mean [P], variance [P]) in the batch's order: mean 0 where the mean is missing, variance 1 where the variance is missing."""
    ic = 1 if has_intercept else 0
    E = len(entity_ids)
    P = int(ent_feat_ptr[-1]) + E * ic
    mean, var = np.zeros(P), np.ones(P)
    for e, eid in enumerate(entity_ids):
        if eid not in prior:
            continue
        theta, variance, idx = prior[eid]
        base = int(ent_feat_ptr[e]) + e * ic
        if ic:
            mean[base] = theta[0]
            var[base] = usable(None if variance is None else variance[0])
        where = {int(g): k for k, g in enumerate(idx)}
        for j, g in enumerate(unique_global[int(ent_feat_ptr[e]):int(ent_feat_ptr[e + 1])]):
            k = where.get(int(g))
            if k is not None:
                mean[base + ic + j] = theta[ic + k]
                var[base + ic + j] = usable(None if variance is None else variance[ic + k])
    return mean, var


def draw_prior(P, seed, cp=None, has_intercept=False):
    """Seeded priors: mu ~ 0.3 N(0, 1), v log-uniform in [1e-4, 10], a third of the coefficients defaulted (mu 0, v 1); v = 1 at the
    intercepts (the header's "The intercept": the intercept column cannot be scaled). -> (mean, variance, scale = sqrt(variance))."""
    rng = np.random.default_rng(seed)
    mean = 0.3 * rng.standard_normal(P)
    var = np.exp(rng.uniform(np.log(1e-4), np.log(10.0), P))
    none = rng.random(P) < 1.0 / 3.0
    mean[none], var[none] = 0.0, 1.0
    if has_intercept and cp is not None:
        var[cp[:-1]] = 1.0
    return mean, var, np.sqrt(var)


def nnz_slots(batch, pk, has_intercept):
    """For every non-zero in raw (= CSR) order: its coefficient slot, its sample."""
    ic = 1 if has_intercept else 0
    cp = coef_ptr(pk, has_intercept)
    ent = np.repeat(np.arange(batch.E, dtype=np.int64), np.diff(pk["ent_nnz_ptr"]))
    row = np.repeat(np.arange(batch.N, dtype=np.int64), np.diff(batch.row_nnz_ptr))
    return cp[:-1][ent] + ic + pk["csr_col"].astype(np.int64), row


def transform_raw(batch, pk, mean, scale, has_intercept):
    """-> (val' [Z] float32 in raw order, offset' [N] float32). One rounding per non-zero; the offsets from an fp64 dot."""
    slot, row = nnz_slots(batch, pk, has_intercept)
    v64 = batch.val.astype(np.float64)
    val2 = (v64 * scale[slot]).astype(np.float32)
    shift = np.bincount(row, weights=v64 * mean[slot], minlength=batch.N)
    if has_intercept:
        ent_of_row = np.repeat(np.arange(batch.E, dtype=np.int64), np.diff(batch.ent_row_ptr))
        shift = shift + mean[coef_ptr(pk, True)[:-1][ent_of_row]]
    return val2, (shift + batch.offset.astype(np.float64)).astype(np.float32)


def restore(mean, scale, phi, var_phi=None, threshold=1e-4):
    theta = mean + scale * phi
    thr = np.where(np.abs(theta) <= threshold, 0.0, theta)
    return theta, thr, None if var_phi is None else scale * scale * var_phi


def prior_objective_grad(batch, pk, e, theta_e, mean_e, var_e, l2, has_intercept, regularize_bias, linear):
    """Exact fp64 F and grad_theta F of entity e at theta_e, on the unrounded data."""
    X, y, off, w = entity_dense(batch, pk, e, has_intercept)
    n = X.shape[0]
    z = X @ theta_e + off
    if linear:
        loss = np.sum(w * (y - z) ** 2)
        r = 2.0 * w * (z - y)
    else:
        loss = np.sum(w * (np.logaddexp(0.0, z) - y * z))
        r = w * (1.0 / (1.0 + np.exp(-z)) - y)
    reg = reg_vector(X.shape[1], l2, has_intercept, regularize_bias) / var_e
    if has_intercept and not regularize_bias:
        reg[0] = 0.0
    d = theta_e - mean_e
    return (loss + 0.5 * np.sum(reg * d * d)) / n, (X.T @ r + reg * d) / n


def scaled_gradient_norms(batch, pk, theta, mean, var, scale, kw, linear):
    """|s (.) grad_theta F|_inf of every entity: the quantity L-BFGS-B's projected-gradient test sees in phi-space."""
    cp = coef_ptr(pk, kw["has_intercept"])
    out = np.zeros(batch.E)
    for e in range(batch.E):
        a, b = int(cp[e]), int(cp[e + 1])
        _, g = prior_objective_grad(batch, pk, e, theta[a:b], mean[a:b], var[a:b], kw["l2"], kw["has_intercept"], kw["regularize_bias"], linear)
        out[e] = np.max(np.abs(scale[a:b] * g)) if b > a else 0.0
    return out


def ridge_with_prior(batch, pk, e, mean_e, var_e, l2, has_intercept, regularize_bias):
    """argmin of F for the squared loss: (2 X~' W X~ + l2 R / v) theta = 2 X~' W (y - offset) + l2 R mu / v."""
    X, y, off, w = entity_dense(batch, pk, e, has_intercept)
    reg = reg_vector(X.shape[1], l2, has_intercept, regularize_bias) / var_e
    if has_intercept and not regularize_bias:
        reg[0] = 0.0
    A = 2.0 * (X.T * w) @ X + np.diag(reg)
    return np.linalg.solve(A, 2.0 * X.T @ (w * (y - off)) + reg * mean_e)
