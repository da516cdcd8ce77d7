"""The tests' own statement of the random effect's box-constrained fit (include/gdmix_re.h, "box constraints"): for one entity of n samples,
theta in local index space, the intercept first and free,

    F(theta) = (1/n) ( sum_i w_i l(y_i, x_i . theta + offset_i) + (l2/2) |theta_R|^2 )      subject to  lo <= theta <= hi

* the problems are re_l1_helpers.EntityProblem with l1 = 0, the batches that module's make_batch / mixed_shapes / block_batch,
* bounds(): one box per GLOBAL feature id in the mix of fe_box_helpers.bounds (sign constraints, two-sided boxes, pinned, upper-only,
  free), seeded, the ids 0 and num_features - 1 always bounded (the gather's edges); entity_bounds() is an entity's view of them,
* the ground truth does not share the device's algorithm: fe_box_helpers.reference_fit (scipy's fmin_l_bfgs_b with bounds) per entity,
* restatement(): fe_box_helpers.box run on the entity problem with re_l1_helpers.TIGHT,
* check_batch(): the bars of fe_box_helpers.check_against_reference per entity; the modulus of the two convexity bounds is l2 / n (what
  EntityProblem.l2 holds), and they are asserted only where every coefficient is regularised and l2 > 0. As in re_l1_helpers the
  theorems are about exact gradients and values, so what rounding leaves in the computed ones (EntityProblem.pg_rounding; value_rounding,
  a first-order forward bound with the same count of rounded terms) is added to the residual norms and to the bound on F - F_ref. The caps on left-out coefficients are re_l1_helpers' (MAX_LEFT_OUT_ENTITY, MAX_LEFT_OUT_SHARE), count equality is excused by
  its ARMIJO_MARGIN / MAX_EXCUSED_SHARE rule. No number here is new: each is one of those two modules'.
"""
import functools

import numpy as np

import fe_box_helpers as FB
import re_l1_helpers as R

LOSSES = R.LOSSES
TIGHT = R.TIGHT
L2 = R.L2
VARIANTS = R.VARIANTS
D = 400      # global features of re_l1_helpers.make_batch


@functools.lru_cache(maxsize=None)
def bounds(num_features=D, seed=0):
    """-> (lower, upper) [num_features] by global feature id; read-only."""
    u = np.random.default_rng([seed, 0xB0]).random(num_features)
    u[0], u[-1] = 0.1, 0.7      # the first id a sign constraint, the last one upper-only
    lo, hi = np.full(num_features, -np.inf), np.full(num_features, np.inf)
    lo[u < 0.35] = 0.0
    b = (u >= 0.35) & (u < 0.60)
    lo[b], hi[b] = -0.05, 0.05
    p = (u >= 0.60) & (u < 0.65)
    lo[p], hi[p] = 0.1, 0.1
    hi[(u >= 0.65) & (u < 0.75)] = -0.02
    lo.setflags(write=False)
    hi.setflags(write=False)
    return lo, hi


def entity_ids(batch, e):
    r0, r1 = int(batch.ent_row_ptr[e]), int(batch.ent_row_ptr[e + 1])
    return np.unique(batch.col_global[int(batch.row_nnz_ptr[r0]):int(batch.row_nnz_ptr[r1])])


def entity_bounds(batch, e, lower, upper, has_intercept=True):
    """The box of entity e in its local order: the intercept first and free."""
    ids = entity_ids(batch, e)
    free = np.full(1 if has_intercept else 0, np.inf)
    lo = np.full(ids.size, -np.inf) if lower is None else lower[ids]
    hi = np.full(ids.size, np.inf) if upper is None else upper[ids]
    return np.concatenate([-free, lo]), np.concatenate([free, hi])


def batch_bounds(batch, lower, upper, has_intercept=True):
    """(lo, hi) [P] in the packed batch's coefficient order."""
    parts = [entity_bounds(batch, e, lower, upper, has_intercept) for e in range(batch.E)]
    return np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts])


_REFERENCES = {}


def references(key, pbs, boxes):
    """fe_box_helpers.reference_fit of every problem, computed once per key and shared; the arrays are read-only."""
    if key not in _REFERENCES:
        out = {}
        for e, pb in pbs.items():
            th, f = FB.reference_fit(pb, *boxes[e])
            th.setflags(write=False)
            out[e] = (th, f)
        _REFERENCES[key] = out
    return _REFERENCES[key]


def case(loss, variant="plain", which="mixed"):
    """-> (problems, boxes, references, batch, option set) of a committed case, shared by every test that asks. The batches are the
    elastic-net cases' (re_l1_helpers.case) with l1 = 0."""
    v = VARIANTS[variant]
    b = R.mixed_batch(loss, variant) if which == "mixed" else R.block_batch(loss)
    key = ("box", which, loss, variant)
    pbs = R.problems(key, b, loss, 0.0, L2, v["has_intercept"], v["regularize_bias"], entities=None if which == "mixed" else R.block_sample(b))
    lower, upper = bounds()
    boxes = {e: entity_bounds(b, e, lower, upper, v["has_intercept"]) for e in pbs}
    return pbs, boxes, references(key, pbs, boxes), b, v


def restatement(pb, lo, hi, theta0=None, m=10, **kw):
    """fe_box_helpers.box on an entity's problem -> (theta, F, status, nit, nfev)."""
    return FB.box(pb, lo, hi, theta0=theta0, m=m, **dict(TIGHT, **kw))


def left_out(pb, lo, hi, theta_ref):
    """fe_box_helpers' rule: a reference coefficient at a bound with a small gradient, or close to a bound without being at it. WEAKLY_ACTIVE
    is a gradient of the fixed effect's objective, a sum over samples: the entity's gradient is taken in those units, times n."""
    g_ref = pb.n * pb.smooth(theta_ref)[1]
    ref_at = FB.at_bound(theta_ref, lo, hi)
    near = (np.minimum(np.abs(theta_ref - lo), np.abs(theta_ref - hi)) < FB.NEAR_BOUND) & ~ref_at
    return (ref_at & (np.abs(g_ref) < FB.WEAKLY_ACTIVE)) | near


def residual_norm(pb, th, lo, hi):
    """|v(theta)| of fe_box_helpers.residual, plus what rounding leaves in the gradient numpy computes there."""
    return np.linalg.norm(FB.residual(pb, th, lo, hi)) + np.linalg.norm(pb.pg_rounding(th))


def value_rounding(pb, th):
    """A bound on what rounding leaves in the value of F numpy computes at th, to first order: F is a sum of n + 2 rounded terms (the count
    EntityProblem.pg_rounding uses for a gradient component) whose magnitudes — not F itself: a count target's terms e^z - y z cancel —
    add up to `terms`, and each z_i = x_i . th + offset_i is itself a rounded sum of nnz_i + 2 products that F sees through dl/dz."""
    eps = np.finfo(float).eps
    z = pb.X @ th + pb.off
    w = np.ones(pb.n) if pb.w is None else pb.w
    if pb.loss == "logistic":
        pieces = np.maximum(z, 0.0) + np.abs(z * pb.y) + np.log1p(np.exp(-np.abs(z)))
    elif pb.loss == "squared":
        pieces = (z - pb.y) ** 2
    else:
        pieces = np.exp(z) + np.abs(pb.y * z)
    terms = (np.sum(w * pieces) + 0.5 * pb.raw_l2 * np.sum(pb.mask * th * th)) / pb.n
    in_z = (np.diff(pb.X.indptr) + 2) * (abs(pb.X) @ np.abs(th) + np.abs(pb.off))
    return eps * ((pb.n + 2) * terms + np.sum(np.abs(pb.residual(th)) * in_z) / pb.n)


def check_left_out_cap(pbs, boxes, refs):
    """The cap on left-out coefficients, for the reference alone: a condition the committed inputs meet."""
    total = coefs = 0
    for e, pb in pbs.items():
        k = int(left_out(pb, *boxes[e], refs[e][0]).sum())
        assert k <= R.MAX_LEFT_OUT_ENTITY, (e, k)
        total, coefs = total + k, coefs + refs[e][0].size
    print(f"left out: {total} of {coefs} coefficients")
    assert total <= R.MAX_LEFT_OUT_SHARE * coefs, (total, coefs)
    return total


def check_batch(pbs, boxes, refs, theta, fval, cp, convexity=True, what=""):
    """The bars, per entity. theta [P], fval [E]: a fit's (the device's, or the restatement's); cp: coefficient offsets per entity. Prints the
    worst figures before it asserts. convexity: the two bounds are theorems (every coefficient regularised, l2 > 0)."""
    worst = dict(f_np=0.0, gap=-np.inf, dist=0.0)
    problems_, n_left, n_at = [], 0, 0
    for e, pb in pbs.items():
        th = np.asarray(theta[int(cp[e]):int(cp[e + 1])], np.float64)
        (lo, hi), (th_ref, f_ref) = boxes[e], refs[e]
        f, F_np = float(fval[e]), pb.smooth(th)[0]
        out = left_out(pb, lo, hi, th_ref)
        n_left += int(out.sum())
        n_at += int(FB.at_bound(th, lo, hi).sum())
        pinned = lo == hi
        if not np.all((lo <= th) & (th <= hi)):
            problems_.append(f"entity {e}: theta leaves the box")
        if not np.array_equal(th[pinned], lo[pinned]):
            problems_.append(f"entity {e}: a pinned coefficient is not the bound's double")
        a = abs(f - F_np) / max(abs(F_np), 1e-300)
        worst["f_np"] = max(worst["f_np"], a)
        if not abs(f - F_np) <= 1e-9 * abs(F_np):
            problems_.append(f"entity {e}: fval {f!r}, numpy at theta {F_np!r}")
        mism = np.flatnonzero((FB.at_bound(th, lo, hi) != FB.at_bound(th_ref, lo, hi)) & ~out)
        if mism.size:
            problems_.append(f"entity {e}: active set differs at {mism.tolist()}: {th[mism].tolist()} reference {th_ref[mism].tolist()}")
        if convexity:
            v_dev, v_ref = residual_norm(pb, th, lo, hi), residual_norm(pb, th_ref, lo, hi)
            gap, gap_bound = F_np - f_ref, v_dev * (v_dev + v_ref) / pb.l2 + value_rounding(pb, th) + value_rounding(pb, th_ref)
            dist, bound = np.linalg.norm(th - th_ref), (v_dev + v_ref) / pb.l2
            worst["gap"] = max(worst["gap"], gap / max(gap_bound, 1e-300))
            worst["dist"] = max(worst["dist"], dist / max(bound, 1e-300))
            if not gap <= gap_bound:      # convexity: F(theta) - F* <= v'(theta - theta*) <= |v| |theta - theta*|
                problems_.append(f"entity {e}: F - F_ref {gap:.3e} above the bound {gap_bound:.3e}")
            if not dist <= bound:         # strong convexity with modulus l2 / n
                problems_.append(f"entity {e}: |theta - theta_ref| {dist:.3e} above the bound {bound:.3e}")
    print(f"{what}: {len(pbs)} entities; worst |fval - F_numpy| / |F| {worst['f_np']:.3e}, worst gap / bound {worst['gap']:.3e}, "
          f"worst distance / bound {worst['dist']:.3e}, at a bound {n_at}, left out {n_left}, {len(problems_)} problems")
    assert not problems_, problems_[:6]
    return worst


# ---- counts: the restatement's, and how close its Armijo tests were -----------------------------------------------------------------------
def counted_run(pb, lo, hi, theta0, m=10, **kw):
    """The restatement -> (status, nit, nfev, F, theta, smallest Armijo margin / max(|F|, 1)). The evaluations are replayed in their
    order: every trial is tested against F(x) + 1e-4 g(x)'(x(t) - x) at the accepted point x of its time, and the margin says how far from
    the edge the closest test was."""
    x0 = np.clip(np.zeros(lo.size) if theta0 is None else np.asarray(theta0, np.float64), lo, hi)
    rec = R._Recording(pb)
    th, Fv, status, nit, nfev = FB.box(rec, lo, hi, theta0=x0, m=m, **dict(TIGHT, **kw))
    x = rec.points[0]
    Fx, gx = pb.smooth(x)
    margin = np.inf
    for xt in rec.points[1:]:
        Ft, gt = pb.smooth(xt)
        edge = Fx + 1e-4 * (gx @ (xt - x))
        margin = min(margin, abs(Ft - edge) / max(abs(Fx), 1.0))
        if Ft <= edge:
            x, Fx, gx = xt, Ft, gt
    return status, nit, nfev, Fv, th, margin


def first_iteration(pb, lo, hi, theta0, m=10, **kw):
    """counted_run with max_iter = 1, without the point."""
    r = counted_run(pb, lo, hi, theta0, m=m, **dict(kw, max_iter=1))
    return r[:4] + r[5:]


_ONE = {}


def one_iteration(loss, warm):
    """first_iteration() of every entity of the plain mixed case, cold or from twice the reference (a start point outside the box, which
    the solve clamps) -> {e: (status, nit, nfev, F, margin)}."""
    if (loss, warm) not in _ONE:
        pbs, boxes, refs, _, _ = case(loss, "plain", "mixed")
        _ONE[(loss, warm)] = {e: first_iteration(pb, *boxes[e], warm_start(refs[e][0]) if warm else None) for e, pb in pbs.items()}
    return _ONE[(loss, warm)]


def warm_start(theta_ref):
    """A start point that leaves every finite box: twice the reference, moved by one."""
    return 2.0 * theta_ref + 1.0


def lds_bytes(p, n, nnz, d, m, has_w):
    """The bounded step's LDS footprint of an entity (csrc/re_owlqn.hip, owlqn_lds_bytes with seven coefficient vectors): the plain wavefront
    kernel's (csrc/re_internal.hpp, wave_lds_bytes) plus two coefficient vectors, each rounded up to 16 bytes."""
    dbl = (5 + 2 * m) * p + n + 2 * m
    w32 = 4 * nnz + (n + 1) + (d + 1) + (3 if has_w else 2) * n
    plain = (dbl * 8 + w32 * 4 + 15) & ~15
    return (plain + 16 * p + 15) & ~15
