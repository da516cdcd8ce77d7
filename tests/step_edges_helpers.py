"""Shared by tests/test_step_edges.py (CPU) and tests/test_gpu_fe_step_edges.py (GPU): the two loops that the fixed effect's three-launch steps
— OWL-QN, the bounded step, TRON — have in common, at the shapes where each can go wrong:

* the strided loop of a products kernel: virtual block vb of nvb takes coefficients (vb * 256 + tid) + k * nvb * 256, nvb = grid_for(P, 256, cap);
  a second trip needs P > cap * 256,
* the fixed-order total of a decide kernel: value v of block b is added by thread (b % 4) * 64 + v, in trips of eight loads while
  b + 28 < nvb, then one load at a time; a trip needs nvb > 28.

The constants of the library are literals ON PURPOSE (test_step_edges.test_the_constants_are_the_librarys reads the sources); the shapes are
L1.EDGE_SIZES, drawn by the case() recipe of tests/fe_l1_helpers.py. Seeds 71, 72, 73: with them every device count below equals the
restatement's. Should a trial ever land on the rounding of the Armijo test, so that a device count differs from the restatement's, change the
seed here — not the assertion.

What a GPU test holds a step to is the numpy restatement of its algorithm (L1.owlqn, BX.box, TR.tron) cut at a few iterations with m = 3, so
that the ring wraps and the history products steer the direction. Full fits at these shapes are NOT asked for: with two to five entries per
feature scipy's reference itself leaves out 18 to 3 436 weakly active coefficients against the helpers' cap of 4, so these shapes never go
through check_against_reference."""
import functools

import numpy as np

import fe_box_helpers as BX
import fe_l1_helpers as L1
import fe_tron_helpers as TR

# ---- the constants: change one HERE first, then run tests/test_step_edges.py ---------------------------------------------------------------
WAVE = 64
FE_THREADS = 256                  # csrc/fe_internal.hpp
FE_DOT_BLOCKS = 512               # TRON's cap: the virtual blocks of its products kernel
QN_BLOCKS = 480                   # the cap of the two quasi-Newton steps
GROUPS = FE_THREADS // WAVE       # 4 partial totals per value
IN_FLIGHT = 8                     # loads of one trip of the total
TEAM_MCAP = 10                    # csrc/re_lbfgs_compact.hpp: history pairs at most
QN_K = {"owlqn": 9 + 4 * TEAM_MCAP, "box": 8 + 4 * TEAM_MCAP}      # values of a block's share: 49 with |x|_1, 48 without
TRON_K = 7

# patterns of the sources the restatement was read from, blanks squeezed; each occurs at least once in csrc/fe_*
SOURCE_PATTERNS = (
    r"constexpr int FE_THREADS = 256;",
    r"constexpr int FE_DOT_BLOCKS = 512;",
    r"constexpr int \w+_BLOCKS = 480;",
    r"for \(; b \+ 28 < nvb; b \+= 32\) \{",
    r"for \(; b < nvb; b \+= 4\)",
    r"for \(int j = vb \* FE_THREADS \+ tid; j < P; j \+= nvb \* FE_THREADS\) \{",
    r"grid_for\(F\.P, FE_THREADS, \w+_BLOCKS\)",
    r"static_assert\(FE_THREADS == 4 \* WAVE,",
)

SHAPES = tuple(L1.EDGE_SIZES)     # share29, share33, capped
LOSSES = ("logistic", "poisson")
STEPS = ("owlqn", "box")
FIT = dict(L1.FIT, m=3, max_iter=6)
TRON_FIT = dict(L1.FIT, max_iter=3)


# ---- the shape of the two loops ------------------------------------------------------------------------------------------------------------
def grid_for(count, per_block, cap):
    g = (count + per_block - 1) // per_block
    return cap if g > cap else (1 if g < 1 else g)


def coefficients(shape):
    return L1.EDGE_SIZES[shape]["D"] + 1      # the intercept last


def blocks(P, cap=QN_BLOCKS):
    return grid_for(P, FE_THREADS, cap)


def total_loads(nvb):
    """-> [(eight-load trips, single loads behind them)] of the four groups of the decide kernel's total."""
    out = []
    for g in range(GROUPS):
        b, trips, tail = g, 0, 0
        while b + GROUPS * (IN_FLIGHT - 1) < nvb:      # b + 28 < nvb
            trips += 1
            b += GROUPS * IN_FLIGHT
        while b < nvb:
            tail += 1
            b += GROUPS
        out.append((trips, tail))
    assert sum(IN_FLIGHT * t + s for t, s in out) == nvb
    return out


def strided_trips(P, nvb):
    """-> [threads (in order of vb * 256 + tid) that make k trips of the products kernel's loop, for k = 0, 1, 2, ...]"""
    first = np.arange(nvb * FE_THREADS)
    trips = np.where(first < P, (P - 1 - first) // (nvb * FE_THREADS) + 1, 0)
    return np.bincount(trips)


def second_trip_start(P, cap=QN_BLOCKS):
    """The first coefficient that a second trip of the strided loop reads (P when there is none)."""
    return min(P, blocks(P, cap) * FE_THREADS)


# ---- the restatements, computed once -------------------------------------------------------------------------------------------------------
def problem(step, loss, shape):
    return (L1 if step == "owlqn" else BX).problem(loss, shape)


def objective(step, pb, theta):
    return pb.F(theta) if step == "owlqn" else pb.smooth(theta)[0]


@functools.lru_cache(maxsize=None)
def restated(step, loss, shape):
    """-> (theta, F, status, nit, nfev) of the restatement under FIT; theta read-only."""
    pb = problem(step, loss, shape)
    kw = dict(m=FIT["m"], max_iter=FIT["max_iter"], ftol=FIT["tolerance"])
    r = L1.owlqn(pb, **kw) if step == "owlqn" else BX.box(pb, *BX.bounds(shape), **kw)
    r[0].setflags(write=False)
    return r


@functools.lru_cache(maxsize=None)
def restated_tron(loss, shape):
    """-> (theta, f, status, nit, nfev, nhv, rejected) of TR.tron under TRON_FIT."""
    r = TR.tron(TR.problem(loss, shape), max_iter=TRON_FIT["max_iter"], ftol=TRON_FIT["tolerance"])
    r[0].setflags(write=False)
    return r


def free(step, theta, shape):
    """What the second trip's coefficients are checked for: non-zero under OWL-QN, strictly inside the bounds under the bounded step."""
    if step == "owlqn":
        return theta != 0
    lo, hi = BX.bounds(shape)
    return (lo < theta) & (theta < hi)


# ---- the steepest-descent action: the search fails with pairs stored -----------------------------------------------------------------------
# The options of a problem carry maxls (gdmix_fe_restart), so the action can be reached: with maxls = 1 every rejected trial either ends the
# fit (status 4: no pair stored) or clears the memory and goes down the pseudo-gradient. OWL-QN on `small`, Poisson, m = 3, from
# scale * (a standard-normal draw of seed); candidates were seeds 1 .. 6 x scales 0.5, 1, 2.
# * maxls = 1, seed 1, scale 1: four iterations, a rejected trial (the fallback), the fallback's trial rejected as well: status 4, nfev 7.
# * maxls = 2, seed 2, scale 1: the sixth iteration rejects two trials, falls back and goes on: status 2 at 12 iterations, nfev 16. A later
#   backtrack reads the direction that the fallback stored.
STEEPEST_STOPS = dict(loss="poisson", size="small", seed=1, scale=1.0, maxls=1, max_iter=12)
STEEPEST_GOES_ON = dict(loss="poisson", size="small", seed=2, scale=1.0, maxls=2, max_iter=12, iteration=6)
STEEPEST = {"stops": STEEPEST_STOPS, "goes on": STEEPEST_GOES_ON}


@functools.lru_cache(maxsize=None)
def steepest_case(which):
    """-> (theta0, (theta, F, status, nit, nfev) of the restatement)."""
    c = STEEPEST[which]
    pb = L1.problem(c["loss"], c["size"])
    theta0 = c["scale"] * np.random.default_rng(c["seed"]).standard_normal(pb.X.shape[1])
    theta0.setflags(write=False)
    return theta0, L1.owlqn(pb, theta0=theta0, m=FIT["m"], max_iter=c["max_iter"], ftol=FIT["tolerance"], maxls=c["maxls"])
