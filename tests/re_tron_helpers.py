"""The tests' own statement of the random effect's trust-region Newton solve (include/gdmix_re.h, "TRON"): for one entity of n samples,
theta in local index space, the intercept first,

    F(theta) = (1/n) ( sum_i w_i l(y_i, x_i . theta + offset_i) + (l2/2) |theta_R|^2 ),   H v = (1/n) ( X~' (D o X~ v) + l2 v_R )

* the objective: re_l1_helpers.EntityProblem with l1 = 0 (numpy, three losses, intercept first, sample weights),
* restate(): fe_tron_helpers.tron(), the numpy restatement of include/gdmix_fe.h's "(ABI 24) TRON", run unchanged on a view of the entity's
  problem whose transposed matrix carries w_i / n (so that its product is the H v above),
* reference_fit(): a ground truth that does not share the algorithm — scipy's fmin_l_bfgs_b on the same objective, factr = 10, pgtol = 1e-10,
* the adjudication rule of tests/fuzz_case.py with the restatement in the oracle's place. An entity is STRICT when the restatement
  reproduces its own (status, nit, nfev, nhv) from starts moved by 1e-15, 1e-14 and 1e-13. On strict entities the device must give the
  restatement's four counts, theta within 1e-7 of the coefficient scale, fval to rtol 1e-9 and the same zero pattern of theta_thr. On
  every entity, strict or not: fval is the numpy objective at the device's theta to 1e-9; after a status 0 or 1 at the TIGHT tolerances
  f - f_ref <= 1e-9 max(|f_ref|, 1); and where every coefficient is regularised |theta - theta_ref| <= (|g| + |g_ref|) n / l2 — strong
  convexity with modulus l2 / n, a theorem about the exact gradients, so what rounding leaves in the computed ones is added to their norms.
  An entity with no minimiser (one class only, or all counts 0, under an unregularised intercept) is held to the rule
  re_poisson_helpers.compare has for it: a stop that is one, and 0 <= f <= f(theta0).
  Every comparison asserts that at least half of its compared entities are strict, so that the rule cannot carry it.
"""
import numpy as np
from scipy.optimize import fmin_l_bfgs_b

import fe_tron_helpers as T
import re_l1_helpers as R

LOSSES, VARIANTS, L2 = R.LOSSES, R.VARIANTS, R.L2
# The tolerances of the comparisons. pgtol: a Newton iteration that still has to run at |g|_inf > pgtol must be decided above the rounding of
# f — its actual reduction is about |g|^2 / (2 lambda), and the acceptance test compares that with 1e-4 of the predicted one. At pgtol = 1e-9
# that is 1e-17, below one unit in the last place of an f near 1, so accepted-or-rejected is the order of the evaluation's sums (met on an
# MI355X: an entity of the mixed batch whose last step gained 2 ulps of f in numpy and none on the device, three rejected trials later the
# same point). At 1e-6 it is 1e-11, four decades above that noise, and quadratic convergence still leaves most entities far below 1e-9 of
# the reference's f (tests/test_re_tron_host.py holds the restatement to that bar).
TIGHT = dict(pgtol=1e-6, ftol=1e-14, max_iter=500, maxfun=15000, maxls=20)
THRESHOLD = 1e-4      # SolverOptions' default sparsity threshold
MAX_CG = T.MAX_CG
JIGS = (1e-15, 1e-14, 1e-13)
MIN_STRICT_SHARE = 0.5


class TronView:
    """An EntityProblem as fe_tron_helpers.tron() reads a problem: its product is XT @ (D * (X @ d)) + l2 mask d with D the unweighted
    curvature, so XT carries w_i / n and l2 is the entity's l2 / n (EntityProblem's own)."""

    def __init__(self, pb):
        w = np.ones(pb.n) if pb.w is None else pb.w
        self.pb, self.loss, self.X, self.off, self.l2, self.mask = pb, pb.loss, pb.X, pb.off, pb.l2, pb.mask
        self.XT = pb.X.multiply(w[:, None] / pb.n).T.tocsr()

    def smooth(self, th):
        return self.pb.smooth(th)


def restate(pb, theta0=None, **kw):
    """-> (theta, f, status, nit, nfev, nhv, rejected trials) of the restatement on an entity's problem."""
    o = dict(TIGHT, **kw)
    return T.tron(TronView(pb), theta0=theta0, max_iter=o["max_iter"], ftol=o["ftol"], pgtol=o["pgtol"], maxfun=o["maxfun"], maxls=o["maxls"])


def product(pb, theta, v):
    """H v at theta, as the restatement forms it."""
    tv = TronView(pb)
    return tv.XT @ (T.curvature(tv, theta) * (tv.X @ v)) + tv.l2 * tv.mask * v


def reference_fit(pb):
    """(theta, f) of scipy's L-BFGS-B at tolerances far below the solver's."""
    theta, f, _ = fmin_l_bfgs_b(pb.smooth, np.zeros(pb.X.shape[1]), m=10, factr=10.0, pgtol=1e-10, maxiter=15000, maxfun=15000)
    return theta, float(f)


def no_minimiser(pb):
    """One class only, or all counts 0, under an unregularised intercept: F has an infimum and no minimiser."""
    if pb.mask[0] != 0.0 or pb.loss == "squared":
        return False
    w = np.ones(pb.n) if pb.w is None else pb.w
    if pb.loss == "logistic":
        return not (np.any(w * pb.y > 0.0) and np.any(w * (1.0 - pb.y) > 0.0))
    return not np.any(w * pb.y > 0.0)


def counts(fit):
    return tuple(int(k) for k in fit[2:6])


def is_strict(pb, theta0, fit, **kw):
    """Does the restatement reproduce its own (status, nit, nfev, nhv) from starts moved by 1e-15, 1e-14 and 1e-13?"""
    p = pb.X.shape[1]
    for j, mag in enumerate(JIGS):
        jig = mag * np.random.default_rng(j + 1).standard_normal(p)
        start = jig if theta0 is None else np.asarray(theta0) * (1.0 + jig)
        if counts(restate(pb, start, **kw)) != counts(fit):
            return False
    return True


_CASES, _REFS = {}, {}


def references(key, pbs):
    """reference_fit of every problem, once per key; read-only."""
    if key not in _REFS:
        out = {}
        for e, pb in pbs.items():
            th, f = reference_fit(pb)
            th.setflags(write=False)
            out[e] = (th, f)
        _REFS[key] = out
    return _REFS[key]


def restatements(key, pbs, theta0=None, cp=None, **kw):
    """{e: dict(fit, strict)} of the restatement on every problem from theta0 ([P] with cp, or None), once per key."""
    if key not in _CASES:
        out = {}
        for e, pb in pbs.items():
            x0 = None if theta0 is None else np.asarray(theta0[int(cp[e]):int(cp[e + 1])], np.float64)
            fit = restate(pb, x0, **kw)
            out[e] = dict(fit=fit, strict=is_strict(pb, x0, fit, **kw))
        _CASES[key] = out
    return _CASES[key]


def problems(key, batch, loss, v, entities=None, l2=L2):
    return R.problems(("tron",) + tuple(key), batch, loss, 0.0, l2, v["has_intercept"], v["regularize_bias"], entities=entities)


def case(loss, variant="plain", which="mixed"):
    """-> (problems, references, restatements at TIGHT from a cold start, batch, option set) of a committed case, shared by every test that
    asks. The batches are those of tests/re_l1_helpers.py."""
    v = VARIANTS[variant]
    b = R.mixed_batch(loss, variant) if which == "mixed" else R.block_batch(loss)
    key = (which, loss, variant)
    pbs = problems(key, b, loss, v, entities=None if which == "mixed" else R.block_sample(b))
    return pbs, references(("tron",) + key, pbs), restatements(key, pbs), b, v


def gradient_rounding(pb, th):
    return np.linalg.norm(pb.pg_rounding(th))


def compare(res, pbs, rest, refs, cp, distance=True, tight=True, what="", min_strict_share=MIN_STRICT_SHARE):
    """The rule of the module docstring. res: the device's result (host dict of whole-batch arrays, with nhv); rest: restatements() of the
    same start and options; refs: references() or None (no bars against the minimiser: a solve that is stopped early). Prints the figures,
    then asserts. -> dict(strict share, worst figures)."""
    problems_ = []
    n_strict = 0
    worst = dict(theta=0.0, f_np=0.0, above=-np.inf, dist=0.0)
    for e, pb in pbs.items():
        s = slice(int(cp[e]), int(cp[e + 1]))
        th, f = np.asarray(res["theta"][s], np.float64), float(res["fval"][e])
        got = (int(res["status"][e]), int(res["nit"][e]), int(res["nfev"][e]), int(res["nhv"][e]))
        x, fr = rest[e]["fit"][0], float(rest[e]["fit"][1])
        want = counts(rest[e]["fit"])
        if not np.all(np.isfinite(th)):
            problems_.append(f"entity {e}: theta is not finite")
            continue
        if rest[e]["strict"]:
            n_strict += 1
            if got != want:
                problems_.append(f"entity {e}: status / nit / nfev / nhv {got}, restatement {want}")
                continue
            scale = max(float(np.max(np.abs(x))) if x.size else 0.0, 1e-300)
            err = float(np.max(np.abs(th - x))) / scale if x.size else 0.0
            worst["theta"] = max(worst["theta"], err)
            if err > 1e-7:
                problems_.append(f"entity {e}: theta {err:.3e} of the coefficient scale from the restatement's")
            if abs(f - fr) > 1e-9 * abs(fr):
                problems_.append(f"entity {e}: fval {f!r}, restatement {fr!r}")
            if not np.array_equal(np.asarray(res["theta_thr"][s]) == 0.0, np.abs(x) <= THRESHOLD):
                problems_.append(f"entity {e}: zero pattern of theta_thr differs")
        F_np, g = pb.smooth(th)
        a = abs(f - F_np) / max(abs(F_np), 1e-300)
        worst["f_np"] = max(worst["f_np"], a)
        if not a <= 1e-9:
            problems_.append(f"entity {e}: fval {f!r}, numpy at theta {F_np!r}")
        if refs is None:
            continue
        if no_minimiser(pb):
            f0 = pb.smooth(np.zeros(th.size))[0]
            if not (got[0] in (0, 1, 2) and (got[0] != 0 or float(res["gnorm"][e]) <= TIGHT["pgtol"]) and 0.0 <= f <= f0):
                problems_.append(f"entity {e} (no minimiser): status {got[0]}, |g| {float(res['gnorm'][e]):.3e}, f {f!r}, f(0) {f0!r}")
            continue
        th_ref, f_ref = refs[e]
        if tight and got[0] in (0, 1):
            above = (f - f_ref) / max(abs(f_ref), 1.0)
            worst["above"] = max(worst["above"], above)
            if not above <= 1e-9:
                problems_.append(f"entity {e}: fval {f!r} is {above:.3e} max(|f_ref|, 1) above the reference {f_ref!r}")
        if distance:
            g_ref = pb.smooth(th_ref)[1]
            dist = np.linalg.norm(th - th_ref)
            bound = (np.linalg.norm(g) + gradient_rounding(pb, th) + np.linalg.norm(g_ref) + gradient_rounding(pb, th_ref)) / pb.l2
            worst["dist"] = max(worst["dist"], dist / max(bound, 1e-300))
            if not dist <= bound:
                problems_.append(f"entity {e}: |theta - theta_ref| {dist:.3e} above the bound {bound:.3e}")
    share = n_strict / max(len(pbs), 1)
    print(f"{what}: {len(pbs)} entities, {n_strict} strict ({share:.1%}); worst strict theta error {worst['theta']:.3e}, worst |fval - F_numpy| / |F| "
          f"{worst['f_np']:.3e}, worst (fval - f_ref) / max(|f_ref|, 1) {worst['above']:.3e}, worst distance / bound {worst['dist']:.3e}, "
          f"{len(problems_)} problems")
    assert share >= min_strict_share, share      # the rule may not carry the comparison
    assert not problems_, problems_[:6]
    return dict(share=share, **worst)


def lds_bytes(p, n, nnz, d, has_w):
    """The TRON LDS footprint of an entity (csrc/re_tron.hip, tron_lds_bytes): the plain wavefront kernel's without history (five
    coefficient vectors, one sample vector, the staged block) plus two coefficient vectors and two sample vectors, each rounded up to 16."""
    w32 = 4 * nnz + (n + 1) + (d + 1) + (3 if has_w else 2) * n
    plain = ((5 * p + n) * 8 + w32 * 4 + 15) & ~15
    return (plain + 8 * (2 * p + 2 * n) + 15) & ~15


SMALL_LDS = 20 * 1024      # csrc/re_tron.hip, TRON_SMALL_LDS: the wavefront kernel's entities within it are launched apart


def first_branch(pb, theta0=None):
    """How the first outer iteration's CG ends in the restatement: ("boundary", sign of s'd at the exit) or ("interior", 0). Restated from
    fe_tron_helpers.tron's CG loop on the same view."""
    tv = TronView(pb)
    x = np.zeros(pb.X.shape[1]) if theta0 is None else np.asarray(theta0, np.float64)
    g = pb.smooth(x)[1]
    D = T.curvature(tv, x)
    delta, gnorm = np.sqrt(g @ g), np.sqrt(g @ g)
    s, r = np.zeros_like(x), -g
    d, rr, ncg = r.copy(), g @ g, 0
    while True:
        h = tv.XT @ (D * (tv.X @ d)) + tv.l2 * tv.mask * d
        ncg += 1
        dhd, ss, sd, dd = d @ h, s @ s, s @ d, d @ d
        alpha = rr / dhd
        if not dhd > 0.0 or ss + 2.0 * alpha * sd + alpha * alpha * dd > delta * delta:
            return "boundary", (1 if sd > 0 else (-1 if sd < 0 else 0))
        rr_new = max(rr - 2.0 * alpha * (r @ h) + alpha * alpha * (h @ h), 0.0)
        s, r = s + alpha * d, r - alpha * h
        if np.sqrt(rr_new) <= 0.1 * gnorm or ncg >= MAX_CG:
            return "interior", 0
        d, rr = r + (rr_new / rr) * d, rr_new
