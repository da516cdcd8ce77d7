"""The tests' own statement of the random effect's preconditioned trust-region Newton solve (include/gdmix_re.h, "TRON_PCG"), on the
objective, the views and the batches of tests/re_tron_helpers.py:

* restate(): the header's rule in numpy (a = 0 makes M = 1: the rule of "TRON" in the same arithmetic, which is how the two are counted
  side by side),
* newton_fit(): the minimiser, by a float64 Newton iteration with a dense Hessian run to |g|_inf <= 1e-12 — it shares no optimiser,
* compare(): the bars tests/re_tron_helpers.compare holds TRON to against its reference, on every entity: fval is the numpy objective at
  the device's theta to 1e-9; after a status 0 or 1, f - f_ref <= 1e-9 max(|f_ref|, 1); where every coefficient is regularised,
  |theta - theta_ref| <= (|g| + |g_ref| + their rounding) n / l2,
* the cases: tests/test_gpu_re_tron._exact_batch entities of exactly (p, n) with column scales over 1e-3 .. 1e3, sample weights added.
"""
import dataclasses

import numpy as np

import fe_tron_helpers as FT
import re_tron_helpers as T

A, M_FLOOR, SPREAD = 0.01, 1e-12, 3.0
EDGE_P, EDGE_N = (1, 2, 63, 64, 65, 130), (1, 16, 65)


def restate(pb, a=A, theta0=None, **kw):
    """-> (theta, f, status, nit, nfev, nhv) of the header's rule on an entity's problem."""
    o, tv = dict(T.TIGHT, **kw), T.TronView(pb)
    x = np.zeros(pb.X.shape[1]) if theta0 is None else np.array(theta0, np.float64)
    X2T, reg = tv.XT.multiply(tv.X.T).tocsr(), tv.l2 * tv.mask      # (w_i / n) x_ij^2
    point = lambda x: (np.maximum((1.0 - a) + a * (X2T @ FT.curvature(tv, x) + reg), M_FLOOR) if a > 0.0 else np.ones(x.size), FT.curvature(tv, x))
    (f, g), (M, D) = pb.smooth(x), point(x)
    nfev, nit, nhv, rejected, moved = 1, 0, 0, 0, False
    if np.max(np.abs(g)) <= o["pgtol"]:
        return x, f, 0, nit, nfev, nhv
    delta = np.sqrt(g @ (g / M))
    while True:
        s, r = np.zeros_like(x), -g
        d, rho, ncg = r / M, g @ (g / M), 0
        gnorm = np.sqrt(rho)
        while True:
            h = tv.XT @ (D * (tv.X @ d)) + reg * d
            ncg, nhv = ncg + 1, nhv + 1
            dhd, zh, hh, sd, ss, dd = d @ h, (r / M) @ h, h @ (h / M), s @ (M * d), s @ (M * s), d @ (M * d)
            alpha = rho / dhd
            if not dhd > 0.0 or ss + 2.0 * alpha * sd + alpha * alpha * dd > delta * delta:
                gap = max(delta * delta - ss, 0.0)
                rad = np.sqrt(sd * sd + dd * gap)
                tau = gap / (sd + rad) if sd >= 0.0 else (rad - sd) / dd
                s, r = s + tau * d, r - tau * h
                break
            rho_new = max(rho - 2.0 * alpha * zh + alpha * alpha * hh, 0.0)
            s, r = s + alpha * d, r - alpha * h
            if np.sqrt(rho_new) <= 0.1 * gnorm or ncg >= T.MAX_CG:
                break
            d, rho = r / M + (rho_new / rho) * d, rho_new
        gs, snorm = g @ s, np.sqrt(s @ (M * s))
        prered = -0.5 * (gs - s @ r)
        f_new, g_new = pb.smooth(x + s)
        nfev += 1
        actred, curv = f - f_new, f_new - f - gs
        if not moved:
            delta = min(delta, snorm)
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
            f_old, x, f, g = f, x + s, f_new, g_new
            M, D = point(x)
            nit, moved, rejected = nit + 1, True, 0
            stops = (np.max(np.abs(g)) <= o["pgtol"], f_old - f <= o["ftol"] * max(abs(f_old), abs(f), 1.0), nit >= o["max_iter"], nfev > o["maxfun"])
            if any(stops):
                return x, f, stops.index(True), nit, nfev, nhv
        else:
            rejected += 1
            if nfev > o["maxfun"] or rejected >= o["maxls"]:
                return x, f, 3 if nfev > o["maxfun"] else 4, nit, nfev, nhv


def newton_fit(pb, theta0=None):
    """(theta, f) of the minimiser: Newton with the dense Hessian and step halving, to |g|_inf <= 1e-12."""
    tv = T.TronView(pb)
    x = np.zeros(pb.X.shape[1]) if theta0 is None else np.array(theta0, np.float64)
    Xd, XTd = np.asarray(tv.X.todense()), np.asarray(tv.XT.todense())
    f, g = pb.smooth(x)
    for _ in range(200):
        if np.max(np.abs(g)) <= 1e-12:
            return x, float(f)
        step, t = np.linalg.solve((XTd * FT.curvature(tv, x)) @ Xd + np.diag(tv.l2 * tv.mask), -g), 1.0
        near = abs(g @ step) <= 1e-12 * max(abs(f), 1.0)      # the decrease left is below the rounding of f: pure Newton steps on the gradient
        while not near and not pb.smooth(x + t * step)[0] <= f + 1e-4 * t * (g @ step) and t > 1e-12:
            t *= 0.5
        x = x + t * step
        f, g = pb.smooth(x)
    raise AssertionError(f"Newton stopped at |g|_inf {np.max(np.abs(g)):.3e}")


def compare(res, pbs, refs, cp, distance, what):
    """The bars of the module docstring; prints the worst figures, then asserts."""
    worst, bad = dict(f_np=0.0, above=-np.inf, dist=0.0), []
    for e, pb in pbs.items():
        th, f, (th_ref, f_ref) = np.asarray(res["theta"][int(cp[e]):int(cp[e + 1])], np.float64), float(res["fval"][e]), refs[e]
        F_np, g = pb.smooth(th)
        figs = dict(f_np=abs(f - F_np) / max(abs(F_np), 1e-300), above=(f - f_ref) / max(abs(f_ref), 1.0) if res["status"][e] in (0, 1) else -np.inf, dist=0.0)
        if distance:
            bound = (np.linalg.norm(g) + T.gradient_rounding(pb, th) + np.linalg.norm(pb.smooth(th_ref)[1]) + T.gradient_rounding(pb, th_ref)) / pb.l2
            figs["dist"] = np.linalg.norm(th - th_ref) / max(bound, 1e-300)
        worst = {k: max(worst[k], v) for k, v in figs.items()}
        if not (np.all(np.isfinite(th)) and 0 <= res["status"][e] <= 1 and figs["f_np"] <= 1e-9 and figs["above"] <= 1e-9 and figs["dist"] <= 1.0):
            bad.append((e, int(res["status"][e]), figs))
    print(f"{what}: {len(pbs)} entities, worst |fval - F_numpy| / |F| {worst['f_np']:.3e}, (fval - f_ref) / max(|f_ref|, 1) {worst['above']:.3e}, "
          f"distance / bound {worst['dist']:.3e}, {len(bad)} outside")
    assert not bad, bad[:4]


_CASES = {}


def case(loss, shapes, seed, regularize_bias=True, zero_column=False):
    """-> (batch, problems, Newton references, option set), once per argument set. zero_column: every third entity's first feature is
    stored with value 0 (an all-zero column: H_jj is its L2 term alone). Without a regularised intercept the first two labels of an
    entity differ, so that a minimiser exists."""
    key = (loss, tuple(shapes), seed, regularize_bias, zero_column)
    if key not in _CASES:
        from test_gpu_re_tron import _exact_batch
        b = _exact_batch(loss, shapes, seed, spread=SPREAD)
        rng, val, y = np.random.default_rng(seed + 1), b.val.copy(), b.y.copy()
        for e in range(b.E):
            r0, r1 = int(b.ent_row_ptr[e]), int(b.ent_row_ptr[e + 1])
            z = slice(int(b.row_nnz_ptr[r0]), int(b.row_nnz_ptr[r1]))
            if zero_column and e % 3 == 0 and z.stop > z.start:
                val[z][b.col_global[z] == b.col_global[z].min()] = 0.0
            if not regularize_bias and loss != "squared":
                y[r0], y[r0 + 1] = 1.0, 0.0
        b = dataclasses.replace(b, val=val, y=y, weight=(0.5 + rng.random(y.size)).astype(np.float32))
        v = dict(has_intercept=True, regularize_bias=regularize_bias)
        pbs = T.problems(("pcg",) + key, b, loss, v)
        refs = {e: newton_fit(pb) for e, pb in pbs.items()}
        _CASES[key] = (b, pbs, refs, v)
    return _CASES[key]


def edge_case(loss, regularize_bias):
    """Every p of EDGE_P with every n of EDGE_N (n >= 16 under an unregularised intercept), a zero column in every third entity."""
    shapes = [(p, n) for p in EDGE_P for n in EDGE_N if regularize_bias or n >= 16]
    return case(loss, shapes, 900 + T.LOSSES.index(loss), regularize_bias, zero_column=True)


BATCH_E = 256


def scaled_batch_case(loss="logistic"):
    """256 badly scaled entities of 2 .. 80 coefficients and 4 .. 40 samples."""
    rng = np.random.default_rng(41)
    return case(loss, [(int(rng.integers(2, 81)), int(rng.integers(4, 41))) for _ in range(BATCH_E)], 950)
