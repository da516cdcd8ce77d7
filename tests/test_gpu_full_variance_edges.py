"""variance_mode FULL held to its dense statement where the fixtures and the older tests do not reach — the three kernel families at their
tile, lane and routing edges (docs/kernels.md, "FULL variances"):

  * the tiled Cholesky and the block-column inverse alone (gdmix_fe_variance_of_hessian) on matrices of one, two and three tiles, one
    column past a tile, with padding of a whole tile, well- and ill-conditioned;
  * the Hessian build alone (gdmix_fe_hessian_dense) entry by entry, with fewer, as many and more columns than workgroups, columns longer
    than a workgroup, repeated (sample, column) pairs, empty samples, the three losses;
  * the wavefront kernel (gdmix_re_variance_full) at p = 1 .. 640 around its 64-lane loops, with its slots re-used over three trips and over
    sixteen when the scratch shrinks to four slots, and at its last size 2 048;
  * the whole-device path on a random-effect batch at p = 2 049, 2 112 and 2 113, the three losses, with and without an intercept.

Every comparison is per entity under the law of full_variance_helpers: max_j |got_j - ref_j| / |ref_j| <= K kappa_2(H) 2^-53 against the
longdouble reference (float64 np.linalg.inv above p = 260). There is no blanket rtol in this file. What the batches must show for this to
mean something is checked on the CPU by tests/test_full_variance_edges.py.

A CHANGED CONSTANT of these kernels is changed in full_variance_helpers first."""
import ctypes as C
import time

import numpy as np
import pytest

import full_variance_helpers as fv
from gdmix_amd.batch import RawBatch
from gdmix_amd.solver import GdmixReError, SolverOptions

pytestmark = pytest.mark.gpu

EINVAL, ENOMEM, ERANGE = -1, -3, -4      # include/gdmix_re.h


def _opts(loss, ic, regularize_bias, l2=fv.L2):
    return SolverOptions(l2=l2, regularize_bias=regularize_bias, has_intercept=bool(ic), loss=loss, variance_mode=2)


def _call_variance_full(solver, packed, opts, theta):
    """gdmix_re_variance_full with the scratch the context holds NOW, into an output pre-filled with NaN -> (return code, output [P])."""
    t = solver.torch
    th = t.from_numpy(np.ascontiguousarray(theta, np.float64)).to(solver.device)
    out = t.full((max(int(packed.P), 1),), float("nan"), dtype=t.float64, device=solver.device)
    c_opts = opts.to_c()
    rc = solver.lib.gdmix_re_variance_full(solver._h, C.byref(packed.c), C.byref(c_opts), th.data_ptr(), out.data_ptr(), solver._stream())
    return rc, out.cpu().numpy()[:int(packed.P)]


def _set_scratch(solver, ptr, nbytes):
    assert solver.lib.gdmix_re_set_scratch(solver._h, ptr, nbytes) == 0


def _variance_full(solver, packed, opts, theta):
    """What REDeviceSolver.variance_full does — the context's scratch grown to what the batch asks for — but every coefficient of the
    output is NaN before the call: an entity that no kernel takes shows."""
    t = solver.torch
    c_opts = opts.to_c()
    need = solver.lib.gdmix_re_solve_scratch_bytes(C.byref(packed.c), C.byref(c_opts))
    if need > packed.c.scratch_bytes and (solver._scratch is None or solver._scratch.numel() < need):
        solver._scratch = t.empty(need, dtype=t.uint8, device=solver.device)
    if solver._scratch is not None:
        _set_scratch(solver, solver._scratch.data_ptr(), solver._scratch.numel())
    rc, out = _call_variance_full(solver, packed, opts, theta)
    assert rc == 0, (rc, solver.lib.gdmix_re_last_error().decode("utf-8", "replace"))
    return out


def _hold(got, ref, what, ill_conditioned=False):
    """Every coefficient written, every entity under the law (and the law no looser than 1e-8 where nothing is ill-conditioned on purpose)."""
    assert got.shape == ref["var"].shape, what
    assert not np.isnan(got).any(), f"{what}: {int(np.isnan(got).sum())} coefficients were never written, the first in entity " \
                                    f"{int(np.searchsorted(ref['coef_ptr'], np.flatnonzero(np.isnan(got))[0], side='right') - 1)}"
    ratios = fv.law_ratios(got, ref)
    worst = int(np.argmax(ratios))
    print(f"{what}: largest err / (kappa 2^-53) = {ratios[worst]:.3f} of K = {fv.K:.1f} at entity {worst} (p = {ref['p'][worst]}, "
          f"kappa = {ref['kappa'][worst]:.3g}); largest kappa {ref['kappa'].max():.3g}")
    if not ill_conditioned:
        assert fv.K * ref["kappa"].max() * fv.U <= fv.RTOL_CAP, what
    assert ratios[worst] <= fv.K, (what, worst, int(ref["p"][worst]), ratios[worst])


# ---- 1. the factor and the inverse alone --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("p,ld", fv.factor_shapes())
def test_factor_and_inverse_alone(device_solver, p, ld):
    """A + regulariser on [ld, ld] with NaN all over the padding: the variances under the law at kappa ~ 10 and at kappa = 1e8, and the
    padding rows and columns of the factor exactly the identity's."""
    t = device_solver.torch
    worst = (0.0, None)
    for cond, l2, unreg in fv.factor_cases(p):
        H = t.from_numpy(fv.padded(fv.factor_matrix(p, cond), ld)).to(device_solver.device)
        got = device_solver.variance_of_hessian(H, p, l2, unreg).cpu().numpy()
        r = fv.factor_reference(p, cond, l2, unreg)
        ratio = fv.law_ratio(got, r["ref"], r["kappa"])
        worst = max(worst, (ratio, (cond, l2, unreg, r["kappa"])))
        assert ratio <= fv.K, (p, ld, cond, l2, unreg, r["kappa"], ratio)
        if cond == "sparse":
            assert fv.K * r["kappa"] * fv.U <= fv.RTOL_CAP
        L = H.cpu().numpy()
        eye = np.eye(ld)
        assert np.array_equal(L[p:, :], eye[p:, :]) and np.array_equal(L[:, p:], eye[:, p:]), (p, ld, cond, l2, unreg)
    print(f"p = {p}, ld = {ld}: largest err / (kappa 2^-53) = {worst[0]:.3f} of K = {fv.K:.1f} at (cond, l2, unreg, kappa) = {worst[1]}")


def test_factor_refusals_write_nothing(device_solver):
    """ld no multiple of 64, ld < p and p = 0: GDMIX_RE_EINVAL, and neither the matrix, the work space nor the output is touched."""
    t, dev = device_solver.torch, device_solver.device
    for p, ld in ((10, 65), (70, 64), (0, 64)):
        H = t.full((ld, ld), 3.0, dtype=t.float64, device=dev)
        work = t.full((ld, ld), 5.0, dtype=t.float64, device=dev)
        out = t.full((128,), 7.0, dtype=t.float64, device=dev)
        rc = device_solver.lib.gdmix_fe_variance_of_hessian(device_solver._h, H.data_ptr(), p, ld, 0.7, -1, work.data_ptr(), out.data_ptr(),
                                                            device_solver._stream())
        assert rc == EINVAL, (p, ld, rc)
        t.cuda.synchronize()
        assert bool((H == 3.0).all()) and bool((work == 5.0).all()) and bool((out == 7.0).all()), (p, ld)
    with pytest.raises(GdmixReError, match=rf"\({EINVAL}\)"):
        device_solver.variance_of_hessian(t.zeros((65, 65), dtype=t.float64, device=dev), 10, 0.7)


# ---- 2. the Hessian build ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(fv.BUILD_CASES))
def test_hessian_build_entry_by_entry(device_solver, name):
    """X~' D X~ of a one-entity batch against the longdouble statement under the plain summation bound n 2^-53 sum|terms| per entry; H
    exactly symmetric; the padding rows and columns exactly zero."""
    d = fv.BUILD_CASES[name][0]
    for ic in fv.BUILD_IC:
        b = fv.build_batch(name, ic)
        packed = device_solver.pack(b, has_intercept=bool(ic))
        p = d + ic
        assert (packed.E, packed.D) == (1, d)
        theta = fv.draw_theta(("build", name, ic), p)
        for loss in fv.LOSSES + (None,):
            H = device_solver.hessian_dense(packed, theta, bool(ic), loss=loss).cpu().numpy()
            assert H.shape == (fv.tiles_ld(p),) * 2
            ref, bound = fv.build_reference(name, ic, loss or "logistic", theta)
            assert np.array_equal(H, H.T), (name, ic, loss)
            assert not H[p:, :].any() and not H[:, p:].any(), (name, ic, loss)
            excess = np.abs(H[:p, :p].astype(np.longdouble) - ref) - bound
            a, c = np.unravel_index(int(np.argmax(excess)), excess.shape)
            assert excess[a, c] <= 0, (name, ic, loss, int(a), int(c), float(H[a, c]), float(ref[a, c]), float(bound[a, c]))
            used = np.abs(H[:p, :p].astype(np.longdouble) - ref)[bound > 0] / bound[bound > 0]
            print(f"{name} ic={ic} {loss}: largest error / bound = {float(used.max()):.4f}")


def test_an_empty_shard_cannot_be_packed(device_solver):
    """A one-entity batch of zero samples never reaches gdmix_fe_hessian_dense: gdmix_re_pack refuses a batch with entities whose label and
    offset arrays are NULL, and empty arrays have no address to give (an error RETURN only: the check is in front of every launch)."""
    empty = RawBatch(ent_row_ptr=np.zeros(2, np.int64), row_nnz_ptr=np.zeros(1, np.int64), col_global=np.zeros(0, np.int64),
                     val=np.zeros(0, np.float32), y=np.zeros(0, np.float32), offset=np.zeros(0, np.float32))
    with pytest.raises(GdmixReError, match=rf"\({EINVAL}\)"):
        device_solver.pack(empty)


# ---- 4. the wavefront kernel's edges -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ic,regularize_bias", fv.WAVE_CASES)
def test_wavefront_kernel_edges(device_solver, ic, regularize_bias):
    b = fv.wave_batch()["b"]
    packed = device_solver.pack(b, has_intercept=bool(ic))
    assert packed.max_p == 640 + ic
    for loss in fv.LOSSES:
        ref = fv.reference("wave", b, loss, fv.L2, ic, regularize_bias)
        assert np.array_equal(packed.coef_ptr_host(), ref["coef_ptr"])
        got = _variance_full(device_solver, packed, _opts(loss, ic, regularize_bias), ref["theta"])
        _hold(got, ref, f"wavefront edges, {loss}, intercept {ic}, regularize_bias {regularize_bias}")


# ---- 5. slot re-use and shrinking scratch ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("loss", fv.LOSSES)
def test_a_slot_serves_three_entities(device_solver, loss):
    b = fv.slots_batch()
    packed = device_solver.pack(b)
    ref = fv.reference("slots", b, loss, fv.L2, 1, False)
    assert packed.E > 2 * fv.VAR_SLOTS_MAX and packed.max_p == fv.SLOTS_MAX_P
    got = _variance_full(device_solver, packed, _opts(loss, 1, False), ref["theta"])
    _hold(got, ref, f"4 200 entities over 2 048 slots, {loss}")


def test_scratch_of_exactly_four_slots(device_solver):
    """64 entities of p = 64 with the context's scratch set to four slots of var_full_slot_doubles(64): sixteen trips per wavefront, the
    results bit-equal to the roomy run's; with 8 bytes fewer GDMIX_RE_ENOMEM, the message naming the bytes needed, nothing written."""
    t = device_solver.torch
    b = fv.four_slot_batch()
    packed = device_solver.pack(b)
    four = 4 * fv.slot_doubles(fv.FOUR_P) * 8
    assert packed.max_p == fv.FOUR_P and packed.c.scratch_bytes < four
    roomy = {}
    for loss in fv.LOSSES:
        ref = fv.reference("four", b, loss, fv.L2, 1, False)
        roomy[loss] = _variance_full(device_solver, packed, _opts(loss, 1, False), ref["theta"])
        _hold(roomy[loss], ref, f"64 entities of p = 64, roomy, {loss}")
    small = t.empty(four, dtype=t.uint8, device=device_solver.device)
    try:
        _set_scratch(device_solver, small.data_ptr(), four)
        for loss in fv.LOSSES:
            rc, tight = _call_variance_full(device_solver, packed, _opts(loss, 1, False), fv.reference("four", b, loss, fv.L2, 1, False)["theta"])
            assert rc == 0, (rc, device_solver.lib.gdmix_re_last_error())
            assert np.array_equal(tight, roomy[loss]), loss
        _set_scratch(device_solver, small.data_ptr(), four - 8)
        rc, untouched = _call_variance_full(device_solver, packed, _opts("logistic", 1, False), fv.reference("four", b, "logistic", fv.L2, 1, False)["theta"])
        assert rc == ENOMEM
        assert str(four) in device_solver.lib.gdmix_re_last_error().decode()
        assert np.isnan(untouched).all()
    finally:
        s = device_solver._scratch
        _set_scratch(device_solver, None if s is None else s.data_ptr(), 0 if s is None else s.numel())


# ---- 6. the hand-over at 2 048 and the tile edges above it --------------------------------------------------------------------------------------
@pytest.mark.parametrize("loss", fv.LOSSES)
@pytest.mark.parametrize("ic", [1, 0])
def test_whole_device_entities_at_the_tile_edges(device_solver, ic, loss):
    """p = 2 113, 2 049 and 2 112 on the whole device, a small entity on a wavefront behind each; every coefficient written."""
    b = fv.hand_over_batch(ic)
    packed = device_solver.pack(b, has_intercept=bool(ic))
    assert packed.max_p == max(fv.HAND_OVER_P) and packed.max_n == fv.HAND_OVER_N
    ref = fv.reference("hand", b, loss, fv.L2, ic, False)
    assert np.array_equal(packed.coef_ptr_host(), ref["coef_ptr"])
    got = _variance_full(device_solver, packed, _opts(loss, ic, False), ref["theta"])
    _hold(got, ref, f"whole-device entities, {loss}, intercept {ic}")


def test_the_wavefront_kernels_last_size(device_solver):
    """p = 2 048 (one wavefront factors and inverts 2 048 x 2 048 out of global memory: docs/kernels.md gives the measured time) next to
    p = 2 049 on the whole device, no intercept: the two sides of `p > VAR_FULL_MAX_P` / `d + ic <= min_p`."""
    b = fv.at_cap_batch()
    packed = device_solver.pack(b, has_intercept=False)
    ref = fv.reference("cap", b, "logistic", fv.L2, 0, True)
    assert tuple(ref["p"][[0, 2]]) == fv.AT_CAP_P and packed.max_p == fv.AT_CAP_P[1]
    t0 = time.perf_counter()
    got = _variance_full(device_solver, packed, _opts("logistic", 0, True), ref["theta"])
    print(f"p = 2 048 on one wavefront and p = 2 049 on the whole device: {time.perf_counter() - t0:.2f} s")
    _hold(got, ref, "the hand-over at 2 048")


def test_one_past_the_largest_size_is_refused(device_solver):
    """max_p = VAR_FULL_BIG_MAX_P + 1: GDMIX_RE_ERANGE from the shape check alone — nothing is allocated, nothing written."""
    packed = device_solver.pack(fv.beyond_batch())
    assert packed.max_p == fv.VAR_FULL_BIG_MAX_P + 1
    rc, out = _call_variance_full(device_solver, packed, _opts("logistic", 1, False), np.zeros(int(packed.P)))
    assert rc == ERANGE and str(fv.VAR_FULL_BIG_MAX_P) in device_solver.lib.gdmix_re_last_error().decode()
    assert np.isnan(out).all()
