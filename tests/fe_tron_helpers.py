"""The tests' own statement of the fixed effect's trust-region Newton optimiser (include/gdmix_fe.h, "(ABI 24) TRON"):

* the cases: those of tests/fe_l1_helpers.py with l1 = 0 — `small` (n 600, D 50) and `wide` (n 20 000, D 5 000: more than one row block
  and more than one column block of 2048),
* reference(): a ground truth that does not share the algorithm — scipy's fmin_l_bfgs_b on the smooth objective, factr = 10, pgtol = 1e-9,
* tron(): a numpy restatement of the header's algorithm section,
* hv(): X~' (D o X~ v), the data term's Hessian-vector product,
* check_against_reference(): the bars a fit is held to,
* rejecting_case(): a start point from which the restatement rejects trials.
"""
import functools

import numpy as np
from scipy.optimize import fmin_l_bfgs_b

import fe_l1_helpers as L1

LOSSES, MODEL_TYPE, SIZES, FIT = L1.LOSSES, L1.MODEL_TYPE, ("small", "wide"), L1.FIT
PGTOL, MAXFUN, MAXLS = L1.PGTOL, L1.MAXFUN, L1.MAXLS
MAX_CG = 50      # GDMIX_FE_TRON_MAX_CG


def case(loss, size):
    """-> (row_nnz_ptr, col, val, y, offset, D, l2)"""
    rp, col, val, y, off, D, _, l2 = L1.case(loss, size)
    return rp, col, val, y, off, D, l2


@functools.lru_cache(maxsize=None)
def problem(loss, size):
    rp, col, val, y, off, D, l2 = case(loss, size)
    return L1.Problem(loss, L1.design(rp, col, val, D), y, off, 0.0, l2)


@functools.lru_cache(maxsize=None)
def reference(loss, size):
    """(theta, f) of scipy's L-BFGS-B at tolerances far below the solver's; computed once per session, read-only."""
    pb = problem(loss, size)
    theta, f, _ = fmin_l_bfgs_b(pb.smooth, np.zeros(pb.X.shape[1]), m=10, factr=10.0, pgtol=1e-9, maxiter=15000, maxfun=15000)
    theta.setflags(write=False)
    return theta, float(f)


def curvature(pb, theta, weight=None):
    """D_i at theta: w rho (1 - rho) | 2 w | w exp(z)."""
    z = pb.X @ theta + pb.off
    w = np.ones(z.size) if weight is None else np.asarray(weight, np.float64)
    if pb.loss == "logistic":
        rho = 1.0 / (1.0 + np.exp(-z))
        return w * rho * (1.0 - rho)
    if pb.loss == "squared":
        return 2.0 * w
    return w * np.exp(z)


def hv(pb, theta, v, weight=None):
    """X~' (D o X~ v): the data term alone, intercept last, no regulariser."""
    return pb.XT @ (curvature(pb, theta, weight) * (pb.X @ v))


def tron(pb, theta0=None, max_iter=500, ftol=1e-12, pgtol=PGTOL, maxfun=MAXFUN, maxls=MAXLS, max_cg=MAX_CG):
    """The algorithm section of the header, restated -> (theta, f, status, nit, nfev, nhv, rejected trials)."""
    x = np.zeros(pb.X.shape[1]) if theta0 is None else np.array(theta0, np.float64)
    reg = pb.l2 * pb.mask
    f, g = pb.smooth(x)
    nfev, nit, nhv, rejected_all = 1, 0, 0, 0
    if np.max(np.abs(g)) <= pgtol:
        return x, f, 0, nit, nfev, nhv, rejected_all
    delta = np.sqrt(g @ g)
    D = curvature(pb, x)
    moved, rejected = False, 0
    while True:
        gnorm = np.sqrt(g @ g)
        s, r = np.zeros_like(x), -g
        d, rr, ncg = r.copy(), g @ g, 0
        while True:
            h = pb.XT @ (D * (pb.X @ d)) + reg * d
            ncg += 1
            nhv += 1
            dhd, ss, sd, dd = d @ h, s @ s, s @ d, d @ d
            alpha = rr / dhd
            if not dhd > 0.0 or ss + 2.0 * alpha * sd + alpha * alpha * dd > delta * delta:
                gap = max(delta * delta - ss, 0.0)
                rad = np.sqrt(sd * sd + dd * gap)
                tau = gap / (sd + rad) if sd >= 0.0 else (rad - sd) / dd
                s, r = s + tau * d, r - tau * h
                break
            rr_new = max(rr - 2.0 * alpha * (r @ h) + alpha * alpha * (h @ h), 0.0)
            s, r = s + alpha * d, r - alpha * h
            if np.sqrt(rr_new) <= 0.1 * gnorm or ncg >= max_cg:
                break
            d, rr = r + (rr_new / rr) * d, rr_new
        gs, snorm = g @ s, np.sqrt(s @ s)
        prered = -0.5 * (gs - s @ r)
        xt = x + s
        f_new, g_new = pb.smooth(xt)
        nfev += 1
        actred = f - f_new
        if not moved:
            delta = min(delta, snorm)
        curv = f_new - f - gs
        ah = 4.0 if curv <= 0.0 else max(0.25, -0.5 * (gs / curv))
        if not actred >= 1e-4 * prered:
            delta = min(max(ah, 0.25) * snorm, 0.5 * delta)
        elif actred < 0.25 * prered:
            delta = max(0.25 * delta, min(ah * snorm, 0.5 * delta))
        elif actred < 0.75 * prered:
            delta = max(0.25 * delta, min(ah * snorm, 4.0 * delta))
        else:
            delta = max(delta, min(ah * snorm, 4.0 * delta))
        if actred > 1e-4 * prered:
            f_old, x, f, g = f, xt, f_new, g_new
            D = curvature(pb, x)
            nit += 1
            moved, rejected = True, 0
            if np.max(np.abs(g)) <= pgtol:
                return x, f, 0, nit, nfev, nhv, rejected_all
            if f_old - f <= ftol * max(abs(f_old), abs(f), 1.0):
                return x, f, 1, nit, nfev, nhv, rejected_all
            if nit >= max_iter:
                return x, f, 2, nit, nfev, nhv, rejected_all
            if nfev > maxfun:
                return x, f, 3, nit, nfev, nhv, rejected_all
        else:
            rejected += 1
            rejected_all += 1
            if nfev > maxfun:
                return x, f, 3, nit, nfev, nhv, rejected_all
            if rejected >= maxls:
                return x, f, 4, nit, nfev, nhv, rejected_all


def check_against_reference(pb, theta, fval, theta_ref, f_ref, what=""):
    """The bars of a fit against the reference; prints each figure before it asserts."""
    theta = np.asarray(theta, np.float64)
    F_np, g = pb.smooth(theta)
    g_ref = pb.smooth(theta_ref)[1]
    dist, bound = np.linalg.norm(theta - theta_ref), (np.linalg.norm(g) + np.linalg.norm(g_ref)) / pb.l2
    print(f"{what}: f {fval!r} numpy at theta {F_np!r} reference {f_ref!r} (f - f_ref) / |f_ref| {(fval - f_ref) / abs(f_ref):.3e}; "
          f"|g|_inf {np.max(np.abs(g)):.3e}; |theta - theta_ref| {dist:.3e} bound {bound:.3e}")
    assert abs(fval - F_np) <= 1e-9 * abs(F_np)
    assert fval - f_ref <= 1e-9 * abs(f_ref)
    assert dist <= bound      # strong convexity with modulus l2 (the intercept is regularised): a theorem, not a tolerance


# A Poisson fit from a start point of large norm: exp(z) makes the quadratic model of some steps a poor one. Candidates on `small`:
# scale * (a standard-normal draw of seed), seeds 7, 8, 9 x scales 3, 4, 5, 8. The restatement rejects 1 trial at every scale of seed 7,
# none with seed 8, none with seed 9 below scale 8 and 3 trials at seed 9, scale 8 (34 iterations, 38 evaluations, 89 products): kept.
REJECTING = dict(loss="poisson", size="small", seed=9, scale=8.0, rejected=3)


@functools.lru_cache(maxsize=None)
def rejecting_case():
    """-> (theta0, trials the restatement rejects from there)."""
    pb = problem(REJECTING["loss"], REJECTING["size"])
    theta0 = REJECTING["scale"] * np.random.default_rng(REJECTING["seed"]).standard_normal(pb.X.shape[1])
    theta0.setflags(write=False)
    return theta0, tron(pb, theta0=theta0, max_iter=FIT["max_iter"], ftol=FIT["tolerance"])[6]
