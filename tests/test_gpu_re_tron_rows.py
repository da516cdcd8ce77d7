"""GPU: re_tron_rows_kernel, the trust-region Newton solve with four entities per wavefront (include/gdmix_re.h, "TRON";
REDeviceSolver.set_tron_row_lds_limit, tron_row_count) — against the numpy restatement and the reference of tests/re_tron_helpers.py at
that module's bars, at the row's lane edges (16 lanes: p and n of 1, 2, 15, 16, 17, 33), with rows of one wavefront in different phases
and wavefronts that are not full, at the footprint edge between the row kernel and the wavefront kernel, the variances, the setter's
refusals. The header promises the wavefront kernel's order of sums, so every comparison with a solve under row limit 0 is bit for bit."""
import dataclasses

import numpy as np
import pytest

from gdmix_amd import solver as S
import re_l1_helpers as R
import re_linear_helpers as H
import re_tron_helpers as T
from test_gpu_re_tron import CG_CAP, REJECTING, STATS, _exact_batch, _gnorm_is_the_gradients, _opts

pytestmark = pytest.mark.gpu
ROW_P, ROW_N = (1, 2, 15, 16, 17, 33), (1, 2, 15, 16, 17)
BITS = ("theta", "theta_thr") + STATS


def _solve(solver, b, opts, theta0=None, row_limit=None, lds_limit=None):
    """-> (host results, packed, row kernel's entities, (LDS-resident entities, workgroup kernel's)); the row limit is the default again behind it."""
    packed = solver.pack(b, has_intercept=bool(opts.has_intercept))
    try:
        if row_limit is not None:
            solver.set_tron_row_lds_limit(row_limit)
        if lds_limit is not None:
            solver.set_wave_lds_limit(lds_limit)
        res = solver.solve_tron(packed, opts, theta0=theta0).to_host()
        rows, counts = solver.tron_row_count(packed), solver.tron_counts(packed)
    finally:
        H.reset_routing(solver)
        solver.set_tron_row_lds_limit(S.REDeviceSolver.TRON_ROW_LDS_DEFAULT)
    assert np.array_equal(packed.coef_ptr_host(), R.coef_ptr(b, bool(opts.has_intercept)))
    return res, packed, rows, counts


def _same_bits(a, b, cp_a, cp_b, pairs, keys=BITS):
    """entity ea of result a and entity eb of result b, for (ea, eb) in pairs: equal bits in every key"""
    for ea, eb in pairs:
        for k in keys:
            per_coef = k in ("theta", "theta_thr", "variance")
            xa = a[k][cp_a[ea]:cp_a[ea + 1]] if per_coef else a[k][ea:ea + 1]
            xb = b[k][cp_b[eb]:cp_b[eb + 1]] if per_coef else b[k][eb:eb + 1]
            assert np.array_equal(xa.view(np.uint8), xb.view(np.uint8)), (k, ea, eb)


_EDGE = {}


def _edge_case(loss, variant):
    if (loss, variant) not in _EDGE:
        v = T.VARIANTS[variant]
        b = _exact_batch(loss, [(p, n) for p in ROW_P[0 if v["has_intercept"] else 1:] for n in ROW_N], seed=700 + T.LOSSES.index(loss))
        if v["weights"]:
            b = dataclasses.replace(b, weight=(0.5 + np.random.default_rng(5).random(b.y.size)).astype(np.float32))
        key = ("row edges", loss, variant)
        pbs = T.problems(key, b, loss, v)
        _EDGE[(loss, variant)] = (pbs, T.references(key, pbs), T.restatements(key, pbs), b, v)
    return _EDGE[(loss, variant)]


# 1 ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", ["plain", "weights", "no_intercept"])
@pytest.mark.parametrize("loss", T.LOSSES)
def test_row_edges(device_solver, loss, variant):
    """Every p of 1, 2, 15, 16, 17, 33 with every n of 1, 2, 15, 16, 17: 30 entities in eight wavefronts, the last one half full; p = 1 is
    the intercept alone over empty rows. Without an intercept the coefficients are 1, 14, 15, 16 and 32 (the features of p = 2 ... 33; p = 1
    would be an entity without coefficients, which the restatement does not take): 25 entities, and the 16 | 17 and 32 | 33 edges are the
    intercept variants' alone. All on the row kernel, at the bars, and the bits of row limit 0."""
    pbs, refs, rest, b, v = _edge_case(loss, variant)
    res, packed, rows, counts = _solve(device_solver, b, _opts(loss, v))
    assert rows == b.E and counts == (b.E, 0)
    cp = packed.coef_ptr_host()
    T.compare(res, pbs, rest, refs, cp, distance=v["distance"], what=f"row kernel {loss} {variant}")
    _gnorm_is_the_gradients(res, pbs, cp)
    off, _, rows0, _ = _solve(device_solver, b, _opts(loss, v), row_limit=0)
    assert rows0 == 0
    _same_bits(res, off, cp, cp, [(e, e) for e in range(b.E)])


# 2 ---------------------------------------------------------------------------------------------------------------------------------------
MIX = dict(shapes=[(20, 12), (33, 16), (10, 5), (17, 17), (5, 3)], seed=46, scale=6.0)      # chosen on the CPU: entity 1's restatement rejects 3 trials
_MIX = {}


def _mix_case(E):
    """-> (batch, problems, theta0, restatements, references) of the first E Poisson entities: entity 0 starts at its solution (it stops at
    iteration 0), entity 1 far out (the recipe of test_rejected_trials: trials are rejected), the others at 0."""
    if E not in _MIX:
        b = _exact_batch("poisson", MIX["shapes"], seed=MIX["seed"]).select(np.arange(E))
        key = ("row mix", E)
        pbs = T.problems(key, b, "poisson", T.VARIANTS["plain"])
        refs = T.references(key, pbs)
        cp = R.coef_ptr(b, True)
        theta0 = np.zeros(int(cp[-1]))
        theta0[cp[0]:cp[1]] = refs[0][0]
        if E > 1:
            theta0[cp[1]:cp[2]] = MIX["scale"] * np.random.default_rng(REJECTING["seed"]).standard_normal(int(cp[2] - cp[1]))
        _MIX[E] = (b, pbs, theta0, T.restatements(key, pbs, theta0=theta0, cp=cp), refs)
    return _MIX[E]


def _moved_and_alone(solver, b, opts, theta0, res, cp, seed):
    """the same entities permuted, and each alone in a batch: the same bits"""
    perm = np.random.default_rng(seed).permutation(b.E)
    moved, packed_m, _, _ = _solve(solver, b.select(perm), opts, theta0=np.concatenate([theta0[cp[e]:cp[e + 1]] for e in perm]), row_limit=T.SMALL_LDS)
    _same_bits(moved, res, packed_m.coef_ptr_host(), cp, [(at, int(e)) for at, e in enumerate(perm)])
    for e in range(b.E):
        alone, _, rows, _ = _solve(solver, b.select(np.array([e])), opts, theta0=theta0[cp[e]:cp[e + 1]], row_limit=T.SMALL_LDS)
        assert rows == 1
        _same_bits(alone, res, np.array([0, cp[e + 1] - cp[e]]), cp, [(0, e)])


@pytest.mark.parametrize("E", [1, 2, 3, 4, 5])
def test_rows_in_different_phases_and_partial_wavefronts(device_solver, E):
    """One to five entities: a wavefront with one to four live rows, or a full one and a second with one row. A row that stops at
    iteration 0 next to one that rejects trials and ordinary ones; each at the bars, and the same bits permuted and alone."""
    b, pbs, theta0, rest, refs = _mix_case(E)
    opts = _opts("poisson", T.VARIANTS["plain"])
    assert T.counts(rest[0]["fit"]) == (0, 0, 1, 0) and (E < 2 or (rest[1]["fit"][6] >= 1 and rest[1]["strict"]))
    res, packed, rows, _ = _solve(device_solver, b, opts, theta0=theta0, row_limit=T.SMALL_LDS)
    assert rows == b.E == E
    cp = packed.coef_ptr_host()
    T.compare(res, pbs, rest, refs, cp, what=f"row mix E={E}")
    _moved_and_alone(device_solver, b, opts, theta0, res, cp, E)


def test_the_cg_cap_next_to_other_rows(device_solver):
    """The three ill-conditioned squared-loss entities of test_the_cg_cap in the rows of one wavefront (a batch has one loss, so they cannot
    sit next to the Poisson rows above), within a 20 KB row limit: rows that run into the cap of 50 products while their neighbours are
    elsewhere. The bars are those that test gives this recipe, for the reason it gives: the four counts, fval at the device's theta, downhill;
    and the bits of row limit 0, permuted, and alone."""
    from test_gpu_re_tron import _cg_cap_case
    b, v, pbs, theta0, rest = _cg_cap_case()
    capped = [e for e, r in rest.items() if T.counts(r["fit"]) == (2, 1, 2, T.MAX_CG) and r["strict"]]
    assert len(capped) >= 2
    opts = _opts(CG_CAP["loss"], v, max_iter=1)
    res, packed, rows, _ = _solve(device_solver, b, opts, theta0=theta0, row_limit=T.SMALL_LDS)
    assert rows == b.E
    cp = packed.coef_ptr_host()
    for e in capped:
        s = slice(int(cp[e]), int(cp[e + 1]))
        F_np, F0 = pbs[e].smooth(res["theta"][s])[0], pbs[e].smooth(theta0[s])[0]
        assert (int(res["status"][e]), int(res["nit"][e]), int(res["nfev"][e]), int(res["nhv"][e])) == (2, 1, 2, T.MAX_CG)
        assert abs(res["fval"][e] - F_np) <= 1e-9 * abs(F_np) and res["fval"][e] < F0
    off, _, rows0, _ = _solve(device_solver, b, opts, theta0=theta0, row_limit=0)      # p > 64: the lanes' second trips through their partials
    assert rows0 == 0
    _same_bits(res, off, cp, cp, [(e, e) for e in range(b.E)])
    _moved_and_alone(device_solver, b, opts, theta0, res, cp, 7)


# 3 ---------------------------------------------------------------------------------------------------------------------------------------
def test_the_footprint_edge_between_the_row_and_the_wavefront_kernel(device_solver):
    from test_gpu_re_l1 import _edge_batch
    b, v = _edge_batch(), T.VARIANTS["plain"]
    fp = [T.lds_bytes(p=6, n=4, nnz=z, d=5, has_w=False) for z in (10, 11)]
    assert fp[1] == fp[0] + 16
    pbs = T.problems(("row kernel edge",), b, "logistic", v)
    refs, rest = T.references(("row kernel edge",), pbs), T.restatements(("row kernel edge",), pbs)
    for row_limit, lds_limit, want in ((fp[0], None, (1, 2, 0)), (fp[0] - 16, None, (0, 2, 0)), (fp[1], None, (2, 2, 0)), (0, 0, (0, 0, 2))):
        res, packed, rows, counts = _solve(device_solver, b, _opts("logistic", v), row_limit=row_limit, lds_limit=lds_limit)
        assert (rows,) + counts == want, (row_limit, lds_limit, rows, counts)
        T.compare(res, pbs, rest, refs, packed.coef_ptr_host(), what=f"row footprint edge, row limit {row_limit}")


# 4 ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [1, 2], ids=["simple", "full"])
@pytest.mark.parametrize("loss", T.LOSSES)
def test_variances_at_the_returned_theta(device_solver, loss, mode):
    """The statement and the tolerances of test_gpu_re_tron.test_variances_at_the_returned_theta, on the row kernel's entities."""
    pbs, _, _, b, v = _edge_case(loss, "weights")
    res, packed, rows, _ = _solve(device_solver, b, _opts(loss, v, variance_mode=mode))
    assert rows == b.E
    cp = packed.coef_ptr_host()
    for e, pb in pbs.items():
        s = slice(int(cp[e]), int(cp[e + 1]))
        np.testing.assert_allclose(res["variance"][s], pb.variance(res["theta"][s], mode), rtol=1e-7 if mode == 1 else 1e-4, err_msg=f"entity {e}")


# 5 ---------------------------------------------------------------------------------------------------------------------------------------
def test_the_setters_refusals(device_solver):
    s = device_solver
    try:
        for bad in (-1, T.SMALL_LDS + 1, 65536):
            assert s.lib.gdmix_re_set_tron_row_lds_limit(s._h, bad) == -1
            with pytest.raises(S.GdmixReError):
                s.set_tron_row_lds_limit(bad)
        assert s.lib.gdmix_re_set_tron_row_lds_limit(None, 0) == -1
        for good in (0, 16, T.SMALL_LDS):
            s.set_tron_row_lds_limit(good)
    finally:
        s.set_tron_row_lds_limit(S.REDeviceSolver.TRON_ROW_LDS_DEFAULT)
