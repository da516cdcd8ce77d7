"""Shared by tests/test_re_poisson.py (CPU) and tests/test_gpu_re_poisson.py (GPU): the Poisson loss of --model_type=poisson_regression
(include/gdmix_re.h, "poisson"). oracle/ does not know this loss, so the ground truth is scipy's fmin_l_bfgs_b — the optimiser the
reference itself calls — run live on a numpy statement of the objective, the way tests/test_oracle_scipy.py pins the oracle:

    z = X~ theta + offset,   f = (1/n) (sum_i w_i (exp(z_i) - y_i z_i) + (l2/2) |theta_reg|^2),   g = (1/n) (X~' (w (exp(z) - y)) + l2 theta_reg)

(the fixed effect: the same sum, not divided by n). Local indices come from oracle.pack, the rows as in re_linear_helpers.entity_dense
(kept sparse: the cells of a row are summed by the matrix product). factr = ftol / eps, pgtol = 1e-5, the same m and maxiter.

The adjudication rule is the one of tests/fuzz_case.py with scipy in the oracle's place. An entity is STRICT when scipy reproduces its
own status, nit and funcalls from starts moved by 1e-15, 1e-14 and 1e-13. On strict entities the device must give identical status, nit
and nfev, theta within 1e-7 of the coefficient scale (1e-5 after a FACTR stop, as test_oracle_scipy.py), fval to rtol 1e-9 and the same
zero pattern of theta_thr. On the rest theta must be within 1e-5 of the minimiser (scipy at ftol = 1e-15, maxiter = 5000). Every
comparison asserts that at least half of its compared entities are strict, so that the rule cannot carry it.
An entity whose labels are all 0 under an unregularised intercept has NO minimiser (f -> 0 as the intercept -> -inf: the Poisson form of
SURVEY 8(d)'s class D; 4 of the 71 sampled entities of ml20m_movie, one or two samples each, and the only non-strict entities met): when
such an entity is not strict there is nothing to be within 1e-5 of, and what is asserted instead is what defines the stop — status 0 with
|g| <= pgtol, a FACTR stop or an iteration limit — and 0 <= f <= f(theta0). On an MI355X the device stopped them at other iterates than scipy
(theta 0.08 .. 0.59 apart, f ~ 1e-7 on both sides).

The device solves whole batches; the reference runs on a seeded sample of a batch (at most 64 entities plus the 8 largest by non-zeros)
and is cached per (batch, option set, warm start) across routings.
"""
import numpy as np
import scipy.optimize as opt
import scipy.sparse as sp

from oracle import oracle

EPS = float(np.finfo(float).eps)
REL_TOL_DEVICE = 1e-7
REL_TOL_FACTR = 1e-5
REL_TOL_MINIMISER = 1e-5
THRESHOLD = 1e-4      # SolverOptions' default sparsity threshold


def entity_sparse(batch, pk, e, has_intercept):
    """Entity e in local index space, intercept first: (X~ csr [n, p], y, offset, w) in fp64; duplicates of a cell are summed."""
    r0, r1 = int(batch.ent_row_ptr[e]), int(batch.ent_row_ptr[e + 1])
    f0, f1 = int(pk["ent_feat_ptr"][e]), int(pk["ent_feat_ptr"][e + 1])
    uniq = np.asarray(pk["unique_global"][f0:f1])
    ic = 1 if has_intercept else 0
    n, d = r1 - r0, f1 - f0
    z0, z1 = int(batch.row_nnz_ptr[r0]), int(batch.row_nnz_ptr[r1])
    rows = np.repeat(np.arange(n), np.diff(batch.row_nnz_ptr[r0:r1 + 1]))
    cols = np.searchsorted(uniq, batch.col_global[z0:z1]) + ic
    vals = batch.val[z0:z1].astype(np.float64)
    if ic:
        rows, cols, vals = np.concatenate([np.arange(n), rows]), np.concatenate([np.zeros(n, np.int64), cols]), np.concatenate([np.ones(n), vals])
    X = sp.csr_matrix((vals, (rows, cols)), shape=(n, d + ic))
    X.sum_duplicates()
    w = np.ones(n) if batch.weight is None else batch.weight[r0:r1].astype(np.float64)
    return X, batch.y[r0:r1].astype(np.float64), batch.offset[r0:r1].astype(np.float64), w


def reg_vector(p, l2, has_intercept, regularize_bias):
    r = np.full(p, float(l2))
    if has_intercept and not regularize_bias:
        r[0] = 0.0
    return r


def objective(X, y, off, w, reg, sum_loss=False, centre=None):
    """-> fg(theta) = (f, g) of the definition above. centre: the prior mean of an incremental fit (the L2 term is (reg/2)(theta - centre)^2)."""
    XT = X.T.tocsr()
    scale = 1.0 if sum_loss else 1.0 / X.shape[0]
    c = 0.0 if centre is None else centre

    def fg(th):
        z = X @ th + off
        ez = np.exp(z)
        d = th - c
        return scale * (np.sum(w * (ez - y * z)) + 0.5 * np.sum(reg * d * d)), scale * (XT @ (w * (ez - y)) + reg * d)
    return fg


def status_of(task):
    task = task.decode() if isinstance(task, bytes) else str(task)
    for word, code in (("PROJECTED GRADIENT", 0), ("REDUCTION", 1), ("ITERATIONS", 2), ("EVALUATIONS", 3), ("ABNORMAL", 4)):
        if word in task.upper():
            return code
    raise AssertionError(f"scipy's task {task!r} is no status of include/gdmix_re.h")


def scipy_fit(fg, x0, m, max_iter, ftol, pgtol=1e-5):
    x, f, info = opt.fmin_l_bfgs_b(fg, np.array(x0, np.float64), m=m, factr=ftol / EPS, pgtol=pgtol, maxiter=max_iter, maxfun=15000, maxls=20)
    return x, float(f), status_of(info["task"]), int(info["nit"]), int(info["funcalls"])


def newton_minimiser(X, y, off, w, reg, sum_loss=False, steps=100):
    """The minimiser of the same objective by damped Newton steps on the dense Hessian (small entities): what the CPU test holds scipy to."""
    Xd = np.asarray(X.todense())
    fg = objective(X, y, off, w, reg, sum_loss)
    th = np.zeros(X.shape[1])
    scale = 1.0 if sum_loss else 1.0 / X.shape[0]
    for _ in range(steps):
        f, g = fg(th)
        if np.max(np.abs(g)) < 1e-14:
            break
        Hm = scale * ((Xd.T * (w * np.exp(Xd @ th + off))) @ Xd + np.diag(reg))
        step = np.linalg.solve(Hm, g)
        t = 1.0
        while fg(th - t * step)[0] > f and t > 1e-10:
            t *= 0.5
        th = th - t * step
    return th


def variance_numpy(batch, pk, kw, mode, theta, coef_ptr, entities=None):
    """_compute_variance with D_i = w_i exp(z_i) at theta ([P], the device's) -> [P] (zeros outside `entities`). mode 1 SIMPLE: 1 / (sum_i D_i
    X~_ij^2 + l2 [- l2 for an unregularised intercept] + 1e-12); mode 2 FULL: diag((X~' D X~ + (l2 + 1e-12) I [- l2 e0 e0'])^-1)."""
    out = np.zeros(int(coef_ptr[-1]))
    for e in (range(batch.E) if entities is None else entities):
        X, _, off, w = entity_sparse(batch, pk, e, kw["has_intercept"])
        s = slice(int(coef_ptr[e]), int(coef_ptr[e + 1]))
        D = w * np.exp(X @ theta[s] + off)
        reg = reg_vector(X.shape[1], kw["l2"], kw["has_intercept"], kw["regularize_bias"])
        if mode == 1:
            out[s] = 1.0 / (np.asarray(X.multiply(X).T @ D).ravel() + reg + 1e-12)
        else:
            Xd = np.asarray(X.todense())
            out[s] = np.diag(np.linalg.inv((Xd.T * D) @ Xd + np.diag(reg + 1e-12)))
    return out


def sample_entities(batch, seed, count=64, largest=8):
    """At most `count` entities drawn with generator seed [seed, 0x5A] plus the `largest` by non-zeros, ascending."""
    E = batch.E
    if E <= count + largest:
        return np.arange(E)
    pick = np.random.default_rng([int(seed), 0x5A]).choice(E, size=count, replace=False)
    big = np.argsort(batch.ent_nnz(), kind="stable")[-largest:]
    return np.unique(np.concatenate([pick, big]))


_CACHE = {}


def reference(batch, pk, kw, th0, coef_ptr, key=None, seed=0, entities=None):
    """scipy on the sampled entities -> dict(entities, theta {e: x}, fval, status, nit, nfev [per sampled entity], strict [bool], fits
    {e: closure for the tight minimiser}). key: cache key (None: not cached)."""
    if key is not None and key in _CACHE:
        return _CACHE[key]
    ents = sample_entities(batch, seed) if entities is None else np.asarray(entities)
    ic = kw["has_intercept"]
    P = int(coef_ptr[-1])
    jigs = [mag * np.random.default_rng(j + 1).standard_normal(P) for j, mag in enumerate((1e-15, 1e-14, 1e-13))]
    ref = dict(entities=ents, theta={}, fval=np.zeros(ents.size), status=np.zeros(ents.size, np.int64), nit=np.zeros(ents.size, np.int64),
               nfev=np.zeros(ents.size, np.int64), strict=np.zeros(ents.size, bool), tight={}, no_minimum=np.zeros(ents.size, bool),
               f_start=np.zeros(ents.size))
    for k, e in enumerate(ents):
        X, y, off, w = entity_sparse(batch, pk, int(e), ic)
        reg = reg_vector(X.shape[1], kw["l2"], ic, kw["regularize_bias"])
        fg = objective(X, y, off, w, reg)
        s = slice(int(coef_ptr[e]), int(coef_ptr[e + 1]))
        x0 = np.zeros(X.shape[1]) if th0 is None else th0[s]
        x, f, st, nit, nfev = scipy_fit(fg, x0, kw["m"], kw["max_iter"], kw["ftol"])
        strict = True
        for jig in jigs:
            _, _, st2, nit2, nfev2 = scipy_fit(fg, jig[s] if th0 is None else x0 * (1.0 + jig[s]), kw["m"], kw["max_iter"], kw["ftol"])
            strict = strict and (st2, nit2, nfev2) == (st, nit, nfev)
        ref["theta"][int(e)] = x
        ref["no_minimum"][k] = bool(ic) and not kw["regularize_bias"] and not np.any(y * w > 0.0)
        ref["f_start"][k] = fg(x0)[0]
        ref["fval"][k], ref["status"][k], ref["nit"][k], ref["nfev"][k], ref["strict"][k] = f, st, nit, nfev, strict
        ref["tight"][int(e)] = (lambda fg=fg, x0=x0: scipy_fit(fg, x0, 10, 5000, 1e-15)[0])
    if key is not None:
        _CACHE[key] = ref
    return ref


def compare(res, ref, coef_ptr, min_strict_share=0.5):
    """The rule of the module docstring. res: the device's result (host dict of whole-batch arrays). Prints the figures, then asserts.
    -> dict(strict share, worst strict error, worst other error)."""
    ents = ref["entities"]
    strict = ref["strict"]
    share = float(strict.mean())
    worst_s = worst_o = 0.0
    problems = []
    for k, e in enumerate(ents):
        s = slice(int(coef_ptr[e]), int(coef_ptr[e + 1]))
        x = ref["theta"][int(e)]
        th = res["theta"][s]
        scale = max(float(np.max(np.abs(x))) if x.size else 0.0, 1e-300)
        if strict[k]:
            counts = (int(res["status"][e]), int(res["nit"][e]), int(res["nfev"][e]))
            want = (int(ref["status"][k]), int(ref["nit"][k]), int(ref["nfev"][k]))
            if counts != want:
                problems.append(f"entity {int(e)}: status / nit / nfev {counts}, scipy {want}")
                continue
            err = float(np.max(np.abs(th - x))) / scale if x.size else 0.0
            worst_s = max(worst_s, err)
            tol = REL_TOL_FACTR if want[0] == 1 else REL_TOL_DEVICE
            if err > tol:
                problems.append(f"entity {int(e)}: theta {err:.3e} from scipy's (status {want[0]}, bar {tol:g})")
            f, fr = float(res["fval"][e]), float(ref["fval"][k])
            if abs(f - fr) > 1e-9 * abs(fr):
                problems.append(f"entity {int(e)}: fval {f!r}, scipy {fr!r}")
            if not np.array_equal(res["theta_thr"][s] == 0.0, np.abs(x) <= THRESHOLD):
                problems.append(f"entity {int(e)}: zero pattern of theta_thr differs")
        elif ref["no_minimum"][k]:
            st, f, gn = int(res["status"][e]), float(res["fval"][e]), float(res["gnorm"][e])
            if not (st in (0, 1, 2) and (st != 0 or gn <= 1e-5) and 0.0 <= f <= ref["f_start"][k]):
                problems.append(f"entity {int(e)} (no minimiser): status {st}, |g| {gn:.3e}, f {f!r}, f(theta0) {float(ref['f_start'][k])!r}")
        else:
            xm = ref["tight"][int(e)]()
            err = float(np.max(np.abs(th - xm))) / max(float(np.max(np.abs(xm))) if xm.size else 0.0, 1e-300)
            worst_o = max(worst_o, err)
            if err > REL_TOL_MINIMISER:
                problems.append(f"entity {int(e)} (not strict): theta {err:.3e} from the minimiser; device status {int(res['status'][e])} nit {int(res['nit'][e])} "
                                f"nfev {int(res['nfev'][e])} f {float(res['fval'][e])!r}, scipy status {int(ref['status'][k])} nit {int(ref['nit'][k])} nfev "
                                f"{int(ref['nfev'][k])} f {float(ref['fval'][k])!r}, scipy's theta {float(np.max(np.abs(x - xm))) / max(float(np.max(np.abs(xm))), 1e-300):.3e} from it")
        if not np.all(np.isfinite(th)):
            problems.append(f"entity {int(e)}: theta is not finite")
    print(f"poisson compare: {ents.size} entities, {share:.1%} strict, worst strict error {worst_s:.3e}, worst other error {worst_o:.3e}, "
          f"{len(problems)} problems")
    assert share >= min_strict_share, share      # the rule may not carry the comparison
    assert not problems, problems[:6]
    return dict(share=share, worst_strict=worst_s, worst_other=worst_o)
