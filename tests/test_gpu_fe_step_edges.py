"""GPU: the two loops that the fixed effect's three-launch steps share — the strided loop of a products kernel and the eight-in-flight total
of a decide kernel (csrc/fe_step_shares.hpp, csrc/fe_qn.hip, csrc/fe_tron.hip) — at the shapes of tests/step_edges_helpers.py: 29 and 33
virtual blocks, and the block cap with a second trip. OWL-QN and the bounded step run six iterations with m = 3, TRON three, each against the
numpy restatement of its algorithm; tests/test_step_edges.py shows on the CPU what every shape reaches. The steepest-descent action of
OWL-QN gets two cases at `small` through the options' maxls."""
import dataclasses

import numpy as np
import pytest

from gdmix_amd import fixed_effect as fe
import fe_box_helpers as BX
import fe_l1_helpers as L1
import fe_tron_helpers as TR
import step_edges_helpers as H


def fit(s, step, loss, shape, **kw):
    rp, col, val, y, off, D, l1, l2 = L1.case(loss, shape)
    args = dict(H.FIT, offset=off, model_type=L1.MODEL_TYPE[loss], l2=l2)
    args.update({"owlqn": dict(l1=l1), "box": dict(bounds=BX.bounds(shape)), "tron": dict(H.TRON_FIT, optimizer="TRON")}[step])
    args.update(kw)
    return s.fit_stepping(rp, col, val, y, D, **args)


def held_to(what, fval, F_np_at_theta, F_restated):
    print(f"{what}: device F {fval!r}; numpy at the device's theta {F_np_at_theta!r}; restatement {F_restated!r}")
    assert abs(fval - F_restated) <= 1e-9 * abs(F_restated)
    assert abs(fval - F_np_at_theta) <= 1e-9 * abs(F_np_at_theta)


@pytest.mark.gpu
@pytest.mark.parametrize("shape", H.SHAPES)
@pytest.mark.parametrize("loss", H.LOSSES)
@pytest.mark.parametrize("step", H.STEPS)
def test_six_iterations_are_the_restatements(device_solver, step, loss, shape):
    pb = H.problem(step, loss, shape)
    theta_np, F_np, st_np, nit_np, nfev_np = H.restated(step, loss, shape)
    theta, info = fit(fe.FixedEffectDeviceSolver(solver=device_solver), step, loss, shape)
    got = int(info["status"]), int(info["nit"]), int(info["nfev"])
    print(f"{step} {loss} {shape}: (status, nit, nfev) device {got} restatement {(st_np, nit_np, nfev_np)}")
    assert got == (st_np, nit_np, nfev_np)
    held_to(f"{step} {loss} {shape}", float(info["fval"]), H.objective(step, pb, theta), F_np)
    if step == "box":
        lo, hi = BX.bounds(shape)
        assert np.all((lo <= theta) & (theta <= hi))
    start = H.second_trip_start(theta.size)
    if start < theta.size:      # `capped`: what the second trip of the strided loops moved
        want, have = H.free(step, theta_np, shape)[start:], H.free(step, theta, shape)[start:]
        print(f"  second trip: {int(want.sum())} of {want.size} free in the restatement, {int(have.sum())} on the device")
        assert want.sum() > 0 and np.all(have[want])


@pytest.mark.gpu
@pytest.mark.parametrize("shape", H.SHAPES)
@pytest.mark.parametrize("loss", H.LOSSES)
def test_three_tron_iterations_are_the_restatements(device_solver, loss, shape):
    pb = TR.problem(loss, shape)
    _, f_np, st_np, nit_np, nfev_np, nhv_np, _ = H.restated_tron(loss, shape)
    theta, info = fit(fe.FixedEffectDeviceSolver(solver=device_solver), "tron", loss, shape)
    got = int(info["status"]), int(info["nit"]), int(info["nfev"]), int(info["nhv"])
    print(f"tron {loss} {shape}: (status, nit, nfev, nhv) device {got} restatement {(st_np, nit_np, nfev_np, nhv_np)}")
    assert got == (st_np, nit_np, nfev_np, nhv_np)
    held_to(f"tron {loss} {shape}", float(info["fval"]), pb.smooth(theta)[0], f_np)


@pytest.mark.gpu
@pytest.mark.parametrize("which", list(H.STEEPEST))
def test_the_search_fails_with_pairs_stored(device_solver, which):
    """The steepest-descent action: memory cleared, d := -pg, and (maxls = 2) a later backtrack along the direction it stored."""
    c = H.STEEPEST[which]
    theta0, (_, F_np, st_np, nit_np, nfev_np) = H.steepest_case(which)
    pb = L1.problem(c["loss"], c["size"])
    kw = dict(H.FIT, max_iter=c["max_iter"])
    s = fe.FixedEffectDeviceSolver(solver=device_solver)
    _, _, prob = fit(s, "owlqn", c["loss"], c["size"], theta0=theta0, return_problem=True, **kw)
    try:
        opts = fe.fit_options(kw["has_intercept"], pb.l2, kw["regularize_bias"], L1.MODEL_TYPE[c["loss"]], kw["max_iter"], kw["m"], kw["tolerance"])
        prob.restart(dataclasses.replace(opts, maxls=c["maxls"]), prob.theta0)
        status, _ = prob.solve()
        theta, res = prob.result()
        got = int(status), int(res["nit"]), int(res["nfev"])
        print(f"maxls = {c['maxls']}: (status, nit, nfev) device {got} restatement {(st_np, nit_np, nfev_np)}")
        assert got == (st_np, nit_np, nfev_np)
        held_to(f"maxls = {c['maxls']}", float(res["fval"]), pb.F(np.asarray(theta, np.float64)), F_np)
    finally:
        prob.close()
