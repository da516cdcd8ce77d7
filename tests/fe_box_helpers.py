"""The tests' own statement of the fixed effect's box-constrained objective (include/gdmix_fe.h, "(ABI 26) box constraints"):

    F(theta) = sum_i l(y_i, x_i . w + b + offset_i) + (l2/2) |theta_R|^2     subject to  lo <= theta <= hi

* the cases, the design and the numpy objective are those of tests/fe_l1_helpers.py with l1 = 0,
* bounds(): the box of a case — a mix of sign constraints, two-sided boxes, pinned and free coefficients, the intercept free,
* reference(): a ground truth that does not share the device's algorithm — scipy's fmin_l_bfgs_b with those bounds (its own Cauchy point
  and subspace minimisation), m = 10, factr = 10, pgtol = 1e-9, from the clamped zeros,
* box(): a numpy restatement of the header's algorithm section,
* residual(): v(theta), the min-norm element of grad F + normal cone of the box,
* check_against_reference(): the bars a fit is held to against the reference.
"""
import functools

import numpy as np
from scipy.optimize import fmin_l_bfgs_b

import fe_l1_helpers as L1
from fe_l1_helpers import FIT, LOSSES, MAX_LEFT_OUT, MAXFUN, MAXLS, MODEL_TYPE, PGTOL, SIZES, case, design  # noqa: F401  (re-exported)

WEAKLY_ACTIVE = 1e-3      # a reference coefficient at a bound with |g_j| below this may be on either side of the active set
NEAR_BOUND = 1e-4         # ... and so may one within this of a bound without being at it


@functools.lru_cache(maxsize=None)
def problem(loss, size):
    rp, col, val, y, off, D, _, l2 = case(loss, size)
    return L1.Problem(loss, design(rp, col, val, D), y, off, 0.0, l2)


@functools.lru_cache(maxsize=None)
def bounds(size):
    """-> (lower, upper) [D + 1], the intercept last and free; read-only."""
    c = L1.shape(size)
    D = c["D"]
    u = np.random.default_rng([c["seed"], 0xB0]).random(D)
    lo, hi = np.full(D + 1, -np.inf), np.full(D + 1, np.inf)
    a = u < 0.35
    lo[:D][a] = 0.0
    b = (u >= 0.35) & (u < 0.60)
    lo[:D][b], hi[:D][b] = -0.05, 0.05
    p = (u >= 0.60) & (u < 0.65)
    lo[:D][p], hi[:D][p] = 0.1, 0.1
    n = (u >= 0.65) & (u < 0.75)
    hi[:D][n] = -0.02
    lo.setflags(write=False)
    hi.setflags(write=False)
    return lo, hi


def scipy_bounds(lo, hi):
    return [(None if l == -np.inf else float(l), None if h == np.inf else float(h)) for l, h in zip(lo, hi)]


def reference_fit(pb, lo, hi, theta0=None):
    x0 = np.clip(np.zeros(lo.size) if theta0 is None else theta0, lo, hi)
    x, f, _ = fmin_l_bfgs_b(pb.smooth, x0, bounds=scipy_bounds(lo, hi), m=10, factr=10.0, pgtol=1e-9, maxiter=15000, maxfun=15000)
    x = np.clip(x, lo, hi)      # (scipy returns feasible points; this only states it)
    return x, pb.smooth(x)[0]


@functools.lru_cache(maxsize=None)
def reference(loss, size):
    """Computed once per session and shared; the arrays are read-only."""
    theta, f = reference_fit(problem(loss, size), *bounds(size))
    theta.setflags(write=False)
    return theta, f


def projected_gradient_norm(x, g, lo, hi):
    return np.max(np.abs(x - np.clip(x - g, lo, hi)))


def binding(x, g, lo, hi):
    return ((x <= lo) & (g > 0)) | ((x >= hi) & (g < 0)) | (lo == hi)


def box(pb, lo, hi, theta0=None, m=10, max_iter=500, ftol=1e-12, pgtol=PGTOL, maxfun=MAXFUN, maxls=MAXLS):
    """The algorithm section of the header, restated -> (theta, F, status, nit, nfev)."""
    x = np.clip(np.zeros(lo.size) if theta0 is None else np.array(theta0, np.float64), lo, hi)
    F, g = pb.smooth(x)
    nfev, nit, pairs = 1, 0, []
    if projected_gradient_norm(x, g, lo, hi) <= pgtol:
        return x, F, 0, nit, nfev
    while True:
        B = binding(x, g, lo, hi)
        q = np.where(B, 0.0, g)
        if pairs:      # two-loop recursion on q
            r, alphas = q.copy(), []
            for s, y in reversed(pairs):
                a = (s @ r) / (s @ y)
                alphas.append(a)
                r -= a * y
            s, y = pairs[-1]
            r *= (s @ y) / (y @ y)
            for (s, y), a in zip(pairs, reversed(alphas)):
                r += (a - (y @ r) / (s @ y)) * s
            d = -r
            d[B | ((x <= lo) & (d < 0)) | ((x >= hi) & (d > 0))] = 0.0
            t = 1.0
        else:
            d, t = -q, 1.0 / np.sqrt(q @ q)
        rejected = 0
        while True:
            xt = np.clip(x + t * d, lo, hi)
            F_t, g_t = pb.smooth(xt)
            nfev += 1
            if F_t <= F + 1e-4 * (g @ (xt - x)):
                break
            rejected += 1
            if rejected >= maxls:
                if not pairs:
                    return x, F, 4, nit, nfev
                pairs, rejected = [], 0
                d, t = -q, 1.0 / np.sqrt(q @ q)
            else:
                t *= 0.5
        s, y = xt - x, g_t - g
        if s @ y > 2.2e-16 * (y @ y):
            pairs = (pairs + [(s, y)])[-m:]
        F_old, x, g, F = F, xt, g_t, F_t
        nit += 1
        if projected_gradient_norm(x, g, lo, hi) <= pgtol:
            return x, F, 0, nit, nfev
        if F_old - F <= ftol * max(abs(F_old), abs(F), 1.0):
            return x, F, 1, nit, nfev
        if nit >= max_iter:
            return x, F, 2, nit, nfev
        if nfev > maxfun:
            return x, F, 3, nit, nfev


def residual(pb, theta, lo, hi):
    """v(theta): 0 where theta_j is at its lower bound with g_j >= 0 or at its upper bound with g_j <= 0 (pinned: always), else g_j."""
    g = pb.smooth(theta)[1]
    return np.where(((theta == lo) & (g >= 0)) | ((theta == hi) & (g <= 0)) | (lo == hi), 0.0, g)


def at_bound(theta, lo, hi):
    return (theta == lo) | (theta == hi)


def check_against_reference(pb, lo, hi, theta, fval, theta_ref, f_ref, what=""):
    """The bars of a fit against the reference; prints each figure before it asserts."""
    theta = np.asarray(theta, np.float64)
    F_np = pb.smooth(theta)[0]
    g_ref = pb.smooth(theta_ref)[1]
    ref_at = at_bound(theta_ref, lo, hi)
    near = (np.minimum(np.abs(theta_ref - lo), np.abs(theta_ref - hi)) < NEAR_BOUND) & ~ref_at
    left_out = (ref_at & (np.abs(g_ref) < WEAKLY_ACTIVE)) | near
    v_dev, v_ref = np.linalg.norm(residual(pb, theta, lo, hi)), np.linalg.norm(residual(pb, theta_ref, lo, hi))
    dist, bound = np.linalg.norm(theta - theta_ref), (v_dev + v_ref) / pb.l2
    gap, gap_bound = F_np - f_ref, v_dev * (v_dev + v_ref) / pb.l2
    mism = np.flatnonzero((at_bound(theta, lo, hi) != ref_at) & ~left_out)
    pinned = lo == hi
    print(f"{what}: F {fval!r} numpy at theta {F_np!r} reference {f_ref!r} (F - F_ref) / |F_ref| {gap / abs(f_ref):.3e} bound {gap_bound / abs(f_ref):.3e}; "
          f"at a bound {int(at_bound(theta, lo, hi).sum())} reference {int(ref_at.sum())} of {theta.size}, left out {int(left_out.sum())}, "
          f"active-set mismatches {mism.size}; |v| {v_dev:.3e} reference {v_ref:.3e}; |theta - theta_ref| {dist:.3e} bound {bound:.3e}; "
          f"feasible {bool(np.all((lo <= theta) & (theta <= hi)))}, pinned equal {bool(np.array_equal(theta[pinned], lo[pinned]))}")
    assert np.all((lo <= theta) & (theta <= hi))
    assert np.array_equal(theta[pinned], lo[pinned])
    assert abs(fval - F_np) <= 1e-9 * abs(F_np)
    assert gap <= gap_bound      # convexity: F(theta) - F* <= v'(theta - theta*) <= |v| |theta - theta*|
    assert int(left_out.sum()) <= MAX_LEFT_OUT
    assert mism.size == 0, (mism, theta[mism], theta_ref[mism])
    assert dist <= bound         # strong convexity with modulus l2 (the intercept is regularised): a theorem, not a tolerance
