"""CPU half of the step-edge suite (tests/test_gpu_fe_step_edges.py is the GPU half): the helper's constants are the library's, the shapes
show — by name — each situation of the two loops that the fixed effect's three-launch steps share, and the restatements that the GPU half
holds the device to take the paths they are there for.

CHANGE A CONSTANT IN tests/step_edges_helpers.py FIRST, then run this file: it names what the shapes no longer show."""
import glob
import os
import re

import pytest

import fe_l1_helpers as L1
import step_edges_helpers as H


def test_the_constants_are_the_librarys():
    import gdmix_amd
    src = os.path.join(os.path.dirname(os.path.abspath(gdmix_amd.__file__)), "csrc")
    files = sorted(glob.glob(os.path.join(src, "fe_*")))
    if not files:
        pytest.skip("the sources are not shipped next to the package: the constants cannot be read")
    text = ""
    for f in files + [os.path.join(src, "re_lbfgs_compact.hpp")]:
        with open(f) as fh:
            text += " ".join(fh.read().split()) + " "
    for pat in H.SOURCE_PATTERNS:
        assert re.search(pat, text), pat
    assert "constexpr int TEAM_MCAP = 10;" in text
    assert (H.WAVE, H.FE_THREADS, H.GROUPS, H.IN_FLIGHT, H.QN_BLOCKS, H.FE_DOT_BLOCKS) == (64, 256, 4, 8, 480, 512)
    assert H.QN_K == {"owlqn": 49, "box": 48} and max(H.QN_K.values()) <= H.WAVE and H.TRON_K <= H.WAVE


def test_the_shapes_are_the_smallest_that_reach_each_loop():
    assert H.grid_for(0, 256, 480) == 1 and H.grid_for(256, 256, 480) == 1 and H.grid_for(257, 256, 480) == 2
    assert H.grid_for(480 * 256, 256, 480) == 480 and H.grid_for(10 ** 9, 256, 480) == 480
    # 28 blocks: no group makes a trip of eight loads; the largest case of the other suites (P = 5 001) has 20
    assert all(t == 0 for t, _ in H.total_loads(28)) and H.blocks(5001) == 20
    P = {s: H.coefficients(s) for s in H.SHAPES}
    assert P == {"share29": 7200, "share33": 8200, "capped": 123201}
    assert H.blocks(P["share29"]) == 29, "share29: one more block than the eight-in-flight loop needs"
    assert H.total_loads(29) == [(1, 0), (0, 7), (0, 7), (0, 7)], "share29: one group makes one eight-load trip, the others only the tail"
    assert H.blocks(P["share33"]) == 33
    assert H.total_loads(33) == [(1, 1), (1, 0), (1, 0), (1, 0)], "share33: every group makes one trip, group 0 one tail load behind it"
    for s in ("share29", "share33"):
        assert list(H.strided_trips(P[s], H.blocks(P[s]))[2:]) == [], f"{s}: one trip of the strided loop"
        assert H.blocks(P[s], H.FE_DOT_BLOCKS) == H.blocks(P[s]), f"{s}: TRON's total sees the same blocks"
    nvb = H.blocks(P["capped"])
    assert nvb == H.QN_BLOCKS and -(-P["capped"] // H.FE_THREADS) > H.QN_BLOCKS, "capped: the grid is the cap"
    assert list(H.strided_trips(P["capped"], nvb)) == [0, nvb * H.FE_THREADS - 321, 321], "capped: the first 321 threads make a second trip"
    assert H.second_trip_start(P["capped"]) == 122880 and P["capped"] - 122880 == 321
    assert H.total_loads(nvb) == [(15, 0)] * 4
    # TRON's cap is FE_DOT_BLOCKS: at `capped` its grid is 482, below it — its strided loop makes one trip there, its total 15 trips and a tail
    assert H.blocks(P["capped"], H.FE_DOT_BLOCKS) == 482 and H.total_loads(482) == [(15, 1), (15, 1), (15, 0), (15, 0)]


@pytest.mark.parametrize("shape", H.SHAPES)
@pytest.mark.parametrize("loss", H.LOSSES)
@pytest.mark.parametrize("step", H.STEPS)
def test_the_restatements_take_six_iterations_along_the_history(step, loss, shape):
    """Six iterations with m = 3: the ring wraps, the pair drop shifts the matrices, the direction comes from the history products."""
    theta, F, status, nit, nfev = H.restated(step, loss, shape)
    print(f"{step} {loss} {shape}: F {F!r} status {status} nit {nit} nfev {nfev}")
    assert (status, nit) == (2, H.FIT["max_iter"]) and nit > H.FIT["m"] and nfev >= nit + 2
    if (step, loss, shape) == ("owlqn", "poisson", "capped"):
        assert nfev > nit + 2, "capped: no case backtracks any more (the update's RETRY action over a second trip)"
    if shape == "capped":
        tail = H.free(step, theta, shape)[H.second_trip_start(H.coefficients(shape)):]
        print(f"  coefficients of the second trip that are {'non-zero' if step == 'owlqn' else 'strictly inside their bounds'}: {int(tail.sum())} of {tail.size}")
        assert 0 < tail.sum() < tail.size, "capped: the second trip's coefficients no longer tell a skipped trip from a taken one"


@pytest.mark.parametrize("shape", H.SHAPES)
@pytest.mark.parametrize("loss", H.LOSSES)
def test_the_tron_restatement_is_cut_at_three_iterations(loss, shape):
    _, f, status, nit, nfev, nhv, _ = H.restated_tron(loss, shape)
    print(f"tron {loss} {shape}: f {f!r} status {status} nit {nit} nfev {nfev} nhv {nhv}")
    assert (status, nit) == (2, H.TRON_FIT["max_iter"]) and nhv >= nit


def test_the_steepest_cases_fall_back_with_pairs_stored():
    """maxls = 1: every rejected trial either stops the fit with status 4 (no pair stored) or clears the memory and goes down the
    pseudo-gradient. STEEPEST_STOPS: iterations, then one fallback, whose trial is rejected as well: nfev = 1 + nit + 2. STEEPEST_GOES_ON
    (maxls = 2): the iteration named there takes two rejected trials, which is the fallback, and the fit goes on to max_iter."""
    c = H.STEEPEST_STOPS
    _, (_, _, status, nit, nfev) = H.steepest_case("stops")
    assert c["maxls"] == 1 and (status, nfev) == (4, nit + 3) and nit >= 1, "choose another seed (the helper lists the candidates)"
    c = H.STEEPEST_GOES_ON
    theta0, (_, _, status, nit, nfev) = H.steepest_case("goes on")
    pb = L1.problem(c["loss"], c["size"])
    kw = dict(theta0=theta0, m=H.FIT["m"], ftol=H.FIT["tolerance"], maxls=c["maxls"])
    before, after = (L1.owlqn(pb, max_iter=k, **kw)[4] for k in (c["iteration"] - 1, c["iteration"]))
    assert c["maxls"] == 2 and after - before - 1 >= 2 and (status, nit) == (2, c["max_iter"]) and nit > c["iteration"], "choose another seed"
