"""--feature_normalization: exact column statistics of a stage's training data, and the factors made from them.

include/gdmix_re.h, "feature normalisation", states the definitions; csrc/feature_stats.hip computes the accumulators on the device.
This module holds what runs on the host around them:

  shifts(count, max_abs)        the per-feature limb width and shifts of pass 2, from pass 1 alone
  finish(...)                   mean and variance from the integer moments, vectorised (D reaches millions in the fixed effect): limbs ->
                                double-double, exact Python integers (object arrays) only where the variance nearly cancels
  factors(kind, stats)          Photon-ML's scale_with_standard_deviation / scale_with_max_magnitude
  DeviceAccumulator             the two kernels behind add(col, val) / shifts() / finish(N)
  NumpyAccumulator              a numpy stand-in of the two kernels behind the same interface (host tests, and workers without the kernels'
                                inputs on a device)
  save / load                   the --feature_statistics_file (.npz)
"""
import logging
import os
from dataclasses import dataclass

import numpy as np

logger = logging.getLogger(__name__)
logger.setLevel(logging.INFO)

NONE = "none"
SCALE_WITH_STANDARD_DEVIATION = "scale_with_standard_deviation"
SCALE_WITH_MAX_MAGNITUDE = "scale_with_max_magnitude"
STANDARDIZATION = "standardization"
KINDS = (NONE, SCALE_WITH_STANDARD_DEVIATION, SCALE_WITH_MAX_MAGNITUDE)
FORMAT_VERSION = 1
MIN_LIMB_BITS = 25          # below this the square of the column's largest value is no longer exact
NO_BAD_INDEX = -1           # bad[1] before a call (an unsigned atomic min on the device)


class FeatureStatsError(ValueError):
    pass


def check_kind(kind):
    """The value of --feature_normalization, refused where it is not one of KINDS."""
    if kind == STANDARDIZATION:
        raise ValueError("--feature_normalization=standardization is not implemented: the mean shift makes the penalty of a regularised intercept "
                         "non-diagonal, and with an unregularised intercept it gives the same coefficients as scale_with_standard_deviation")
    if kind not in KINDS:
        raise ValueError(f"--feature_normalization={kind!r}: one of {', '.join(KINDS)}")
    return kind


def passes(kind):
    """Passes over the data the statistics of this type need: the maximum alone is pass 1."""
    return 1 if kind == SCALE_WITH_MAX_MAGNITUDE else 2


# ---- pass 1 -> the shifts of pass 2 --------------------------------------------------------------------------------------------------
def shifts(count, max_abs):
    """count [D] int64, max_abs [D] float32 -> (limb_bits, shift1, shift2) [D] int32; limb_bits 0 marks a dead feature."""
    count = np.asarray(count, np.int64)
    a = np.asarray(max_abs, np.float32)
    if np.any(count < 0) or not np.all(np.isfinite(a)) or np.any(a < 0):
        raise FeatureStatsError("feature statistics: a negative count or a maximum that is not a finite magnitude")
    live = (count > 0) & (a > 0)
    _, e_count = np.frexp(count.astype(np.float64))       # count = m 2^e with m in [0.5, 1): e is its bit length (exact up to 2^53)
    _, e_a = np.frexp(a.astype(np.float64))               # a = m 2^e: e = floor(log2 a) + 1
    L = np.minimum(31, 62 - e_count.astype(np.int64))
    small = live & (L < MIN_LIMB_BITS)
    if np.any(small):
        j = int(np.flatnonzero(small)[0])
        raise FeatureStatsError(f"feature {j} has {int(count[j])} stored entries: more than 2^37 entries of one feature leave fewer than "
                                f"{MIN_LIMB_BITS} bits per limb, and the square of the column's largest value is no longer exact")
    e1 = e_a.astype(np.int64)
    L = np.where(live, L, 0)
    s1 = np.where(live, 2 * L - e1, 0)
    s2 = np.where(live, 2 * L - 2 * e1, 0)
    return L.astype(np.int32), s1.astype(np.int32), s2.astype(np.int32)


# ---- double-double arithmetic on arrays (no fused multiply-add in numpy: Dekker's split) -------------------------------------------------
def _two_sum(a, b):
    s = a + b
    bb = s - a
    return s, (a - (s - bb)) + (b - bb)


def _split(a):
    t = 134217729.0 * a
    hi = t - (t - a)
    return hi, a - hi


def _two_prod(a, b):
    p = a * b
    ah, al = _split(a)
    bh, bl = _split(b)
    return p, ((ah * bh - p) + ah * bl + al * bh) + al * bl


def _dd_add(ah, al, bh, bl):
    s, e = _two_sum(ah, bh)
    t, f = _two_sum(al, bl)
    e = e + t
    s, e = _two_sum(s, e)
    e = e + f
    return _two_sum(s, e)


def _dd_mul(ah, al, bh, bl):
    p, e = _two_prod(ah, bh)
    e = e + (ah * bl + al * bh)
    return _two_sum(p, e)


def _dd_of_int64(v):
    """int64 -> (hi, lo) with hi + lo = v exactly."""
    v = np.asarray(v, np.int64)
    top = (v >> 32).astype(np.float64) * 4294967296.0
    bot = (v & 0xffffffff).astype(np.float64)
    return _two_sum(top, bot)


def _dd_of_limbs(hi, lo, L):
    """hi 2^L + lo as a double-double: an integer below 2^94, exact in 106 bits."""
    hh, hl = _dd_of_int64(hi)
    hh, hl = np.ldexp(hh, L), np.ldexp(hl, L)
    lh, ll = _dd_of_int64(lo)
    return _dd_add(hh, hl, lh, ll)


def _dd_div_to_double(nh, nl, dh, dl):
    """(nh + nl) / (dh + dl) rounded to a double, to well within 1 ulp (two quotient steps)."""
    q1 = nh / dh
    ph, pl = _dd_mul(dh, dl, q1, np.zeros_like(q1))
    rh, rl = _dd_add(nh, nl, -ph, -pl)
    q2 = rh / dh
    return q1 + q2


def _int_of_limbs(hi, lo, L):
    """The same integers as Python ints (an object array)."""
    return (hi.astype(object) << L.astype(object)) + lo.astype(object)


CANCEL_BITS = 40      # N I2 2^(2L) - I1^2 below 2^-40 of its terms: exact integers decide (the double-double difference keeps ~2^-100 of them)


def finish(count, max_abs, limb_bits, shift1, shift2, limbs, num_samples):
    """The integer moments -> (mean [D], variance [D]) fp64, each within 1 ulp of the exact rational value; the variance exactly 0 when
    N I2 2^(2L) = I1^2 and where that difference is negative. Dead features get 0 and 0. limbs [D, 4] int64: hi1, lo1, hi2, lo2."""
    N = int(num_samples)
    D = int(np.asarray(count).shape[0])
    mean = np.zeros(D, np.float64)
    var = np.zeros(D, np.float64)
    L_all = np.asarray(limb_bits, np.int32)
    idx = np.flatnonzero(L_all > 0)
    if N < 1 or idx.size == 0:
        return mean, var
    limbs = np.asarray(limbs, np.int64).reshape(D, 4)[idx]
    L = L_all[idx].astype(np.int64)
    s1 = np.asarray(shift1, np.int32)[idx].astype(np.int64)
    s2 = np.asarray(shift2, np.int32)[idx].astype(np.int64)
    with np.errstate(all="ignore"):
        i1h, i1l = _dd_of_limbs(limbs[:, 0], limbs[:, 1], L)
        i2h, i2l = _dd_of_limbs(limbs[:, 2], limbs[:, 3], L)
        n = np.full(idx.size, float(N))
        zero = np.zeros(idx.size)
        # mean = I1 2^-shift1 / N
        mean[idx] = np.ldexp(_dd_div_to_double(i1h, i1l, n, zero), -s1)
        if N > 1:
            # var = 2^(-shift2 - 2L) (N I2 2^(2L) - I1^2) / (N (N - 1))
            ah, al = _dd_mul(i2h, i2l, n, zero)
            ah, al = np.ldexp(ah, 2 * L), np.ldexp(al, 2 * L)
            bh, bl = _dd_mul(i1h, i1l, i1h, i1l)
            mh, ml = _dd_add(ah, al, -bh, -bl)
            qh, ql = _two_prod(n, n - 1.0)
            v = _dd_div_to_double(mh, ml, qh, ql)
            near = np.abs(mh) <= np.ldexp(np.abs(ah), -CANCEL_BITS)
            if np.any(near):
                k = np.flatnonzero(near)
                Lk = L[k]
                I1 = _int_of_limbs(limbs[k, 0], limbs[k, 1], Lk)
                I2 = _int_of_limbs(limbs[k, 2], limbs[k, 3], Lk)
                M = ((I2 * N) << (2 * Lk).astype(object)) - I1 * I1
                M = np.where(M > 0, M, 0).astype(object)
                v[k] = (M / (N * (N - 1))).astype(np.float64)      # int / int: correctly rounded
            v = np.where(v > 0, v, 0.0)
            var[idx] = np.ldexp(v, -s2 - 2 * L)
    return mean, var


# ---- the statistics of one bag ---------------------------------------------------------------------------------------------------------
@dataclass
class FeatureStats:
    num_features: int
    num_samples: int
    count: np.ndarray        # [D] int64
    max_abs: np.ndarray      # [D] float32
    mean: np.ndarray         # [D] float64 (zeros when only pass 1 ran)
    variance: np.ndarray     # [D] float64 (NaN when only pass 1 ran: scale_with_standard_deviation refuses such a file)
    limbs: np.ndarray = None     # [D, 4] int64, kept for tests (not written to the file)

    def equal_bits(self, other):
        return (self.num_features == other.num_features and self.num_samples == other.num_samples and np.array_equal(self.count, other.count)
                and np.array_equal(self.max_abs.view(np.uint32), other.max_abs.view(np.uint32))
                and np.array_equal(self.mean.view(np.uint64), other.mean.view(np.uint64))
                and np.array_equal(self.variance.view(np.uint64), other.variance.view(np.uint64)))


def factors(kind, stats):
    """s [D] fp64: 1 / sqrt(var) or 1 / max|x|; 1 where the feature is dead, where the variance is 0 or where the result is not finite."""
    kind = check_kind(kind)
    D = stats.num_features
    s = np.ones(D, np.float64)
    if kind == NONE:
        return s
    live = (stats.count > 0) & (stats.max_abs > 0)
    with np.errstate(all="ignore"):
        if kind == SCALE_WITH_MAX_MAGNITUDE:
            f = 1.0 / stats.max_abs.astype(np.float64)
        else:
            if np.any(np.isnan(stats.variance)):
                raise FeatureStatsError("the feature statistics hold no variances (written by a scale_with_max_magnitude run): "
                                        "scale_with_standard_deviation needs a file with both passes")
            f = 1.0 / np.sqrt(stats.variance)
    ok = live & np.isfinite(f) & (f > 0)
    s[ok] = f[ok]
    return s


def save(path, stats):
    """Written to a temporary name and renamed: a reader never sees half a file."""
    tmp = f"{path}.tmp.{os.getpid()}.npz"
    d = os.path.dirname(os.path.abspath(path))
    os.makedirs(d, exist_ok=True)
    np.savez(tmp, format_version=np.int64(FORMAT_VERSION), num_features=np.int64(stats.num_features), num_samples=np.int64(stats.num_samples),
             count=stats.count.astype(np.int64), max_abs=stats.max_abs.astype(np.float32), mean=stats.mean.astype(np.float64),
             variance=stats.variance.astype(np.float64))
    os.replace(tmp, path)


def load(path, num_features):
    with np.load(path) as z:
        missing = [k for k in ("format_version", "num_features", "num_samples", "count", "max_abs", "mean", "variance") if k not in z.files]
        if missing:
            raise FeatureStatsError(f"--feature_statistics_file={path}: no {', '.join(missing)} in the file")
        if int(z["format_version"]) != FORMAT_VERSION:
            raise FeatureStatsError(f"--feature_statistics_file={path}: format_version {int(z['format_version'])}, this build reads {FORMAT_VERSION}")
        D = int(z["num_features"])
        if D != int(num_features):
            raise FeatureStatsError(f"--feature_statistics_file={path}: num_features {D}, the feature bag has {int(num_features)}")
        st = FeatureStats(D, int(z["num_samples"]), z["count"].astype(np.int64), z["max_abs"].astype(np.float32), z["mean"].astype(np.float64),
                          z["variance"].astype(np.float64))
    for a in (st.count, st.max_abs, st.mean, st.variance):
        if a.shape != (D,):
            raise FeatureStatsError(f"--feature_statistics_file={path}: an array of shape {a.shape}, expected ({D},)")
    return st


def _raise_bad(bad, what):
    """bad: [(count, first index)] per call of one pass, in call order."""
    for call, (n, first) in enumerate(bad):
        if n:
            raise FeatureStatsError(f"feature statistics, {what}: {int(n)} bad entries in call {call}, the first at index {int(first)} of that call "
                                    "(a value that is not finite, a column outside the feature bag, or a value above the maximum of pass 1)")


# ---- the accumulators ------------------------------------------------------------------------------------------------------------------
class _Accumulator:
    """add(col, val) per partition or chunk in pass 1; shifts() ends pass 1 (after an all-reduce of count and max_abs_bits, if any); add()
    again, over the same data, in pass 2; finish(N). With kind scale_with_max_magnitude finish() may follow pass 1 directly."""

    def __init__(self, num_features):
        self.D = int(num_features)
        self.pass_no = 1
        self.limb_bits = self.shift1 = self.shift2 = None
        self._bad = []

    # subclasses: _add1, _add2, host_extent() -> (count int64, bits uint32), set_extent(count, bits), host_limbs(), _read_bad()
    def add(self, col, val):
        (self._add1 if self.pass_no == 1 else self._add2)(col, val)

    def take_bad(self):
        """[(count, first index)] of every call since the last look, read once."""
        bad, self._bad = self._read_bad(), []
        return bad

    def check(self):
        """Read `bad` of every call so far (once per pass) and raise, naming the entry."""
        _raise_bad(self.take_bad(), f"pass {self.pass_no}")

    def shifts(self):
        self.check()
        count, bits = self.host_extent()
        self.limb_bits, self.shift1, self.shift2 = shifts(count, bits.view(np.float32))
        self.pass_no = 2
        self._begin_pass2()
        return self.limb_bits, self.shift1, self.shift2

    def finish(self, num_samples):
        self.check()
        count, bits = self.host_extent()
        a = bits.view(np.float32).copy()
        D = self.D
        if self.pass_no == 1:
            return FeatureStats(D, int(num_samples), count, a, np.zeros(D), np.full(D, np.nan))
        limbs = self.host_limbs()
        mean, var = finish(count, a, self.limb_bits, self.shift1, self.shift2, limbs, num_samples)
        return FeatureStats(D, int(num_samples), count, a, mean, var, limbs=limbs)


class NumpyAccumulator(_Accumulator):
    """The two kernels restated in numpy: the same integers by the same definitions (np.ldexp and np.rint are the IEEE operations)."""

    def __init__(self, num_features):
        super().__init__(num_features)
        self.count = np.zeros(self.D, np.int64)
        self.bits = np.zeros(self.D, np.uint32)
        self.limbs = None

    def _good(self, col, val, extra=None):
        col = np.asarray(col).astype(np.int64)
        val = np.asarray(val, np.float32)
        ok = (col >= 0) & (col < self.D) & np.isfinite(val)
        if extra is not None:
            ok, skip = extra(col, val, ok)
        else:
            skip = np.zeros(col.shape, bool)
        badm = ~ok & ~skip
        self._bad.append((int(badm.sum()), int(np.flatnonzero(badm)[0]) if badm.any() else NO_BAD_INDEX))
        return col[ok], val[ok]

    def _add1(self, col, val):
        c, v = self._good(col, val)
        np.add.at(self.count, c, 1)
        np.maximum.at(self.bits, c, np.abs(v).view(np.uint32))

    def _begin_pass2(self):
        self.limbs = np.zeros((self.D, 4), np.int64)

    def _add2(self, col, val):
        def in_range(col, val, ok):
            cc = np.where(ok, col, 0)
            L = self.limb_bits[cc].astype(np.int64)
            bound = np.ldexp(1.0, (2 * L - self.shift1[cc]).astype(np.int64))
            dead = ok & (L == 0)
            return ok & (L > 0) & (np.abs(val.astype(np.float64)) < bound), dead & (val == 0)
        c, v = self._good(col, val, in_range)
        x = v.astype(np.float64)
        L = self.limb_bits[c].astype(np.int64)
        t1 = np.rint(np.ldexp(x, self.shift1[c])).astype(np.int64)
        t2 = np.rint(np.ldexp(x * x, self.shift2[c])).astype(np.int64)
        m = (np.int64(1) << L) - 1
        for k, t in ((0, t1 >> L), (1, t1 & m), (2, t2 >> L), (3, t2 & m)):
            np.add.at(self.limbs[:, k], c, t)

    def host_extent(self):
        return self.count.copy(), self.bits.copy()

    def set_extent(self, count, bits):
        self.count, self.bits = np.asarray(count, np.int64).copy(), np.asarray(bits, np.uint32).copy()

    def host_limbs(self):
        return self.limbs.copy()

    def set_limbs(self, limbs):
        self.limbs = np.asarray(limbs, np.int64).reshape(self.D, 4).copy()

    def _read_bad(self):
        return list(self._bad)


class DeviceAccumulator(_Accumulator):
    """gdmix_re_feature_extent / gdmix_re_feature_moments on a REDeviceSolver's device. col: a device tensor of int64, int32 or uint16 ids
    (uint16 also as int16: torch's older narrow type, the bits are what counts); val: float32 device tensor. Everything is queued on the
    current stream; the host reads back once per pass (check / shifts / finish)."""

    WIDTHS = {"torch.int64": 8, "torch.int32": 4, "torch.uint16": 2, "torch.int16": 2}

    def __init__(self, solver, num_features):
        super().__init__(num_features)
        t = solver.torch
        self.solver = solver
        D = max(self.D, 1)
        self.count = t.zeros(D, dtype=t.int64, device=solver.device)
        self.bits = t.zeros(D, dtype=t.int32, device=solver.device)
        self.limbs = None
        self._dev_shifts = None

    def _new_bad(self):
        t = self.solver.torch
        b = t.tensor([0, NO_BAD_INDEX], dtype=t.int64).to(self.solver.device, non_blocking=True)
        self._bad.append(b)
        return b

    def _args(self, col, val):
        w = self.WIDTHS.get(str(col.dtype))
        t = self.solver.torch
        if w is None or val.dtype != t.float32 or not col.is_cuda or not val.is_cuda or col.numel() != val.numel() \
                or not col.is_contiguous() or not val.is_contiguous():
            raise FeatureStatsError("feature statistics: col (int64, int32 or uint16) and val (float32) must be contiguous device arrays of one length")
        Z = int(val.numel())
        return w, Z, (col.data_ptr() if Z else None), (val.data_ptr() if Z else None)

    def _add1(self, col, val):
        w, Z, pc, pv = self._args(col, val)
        self.solver.feature_extent(pc, w, pv, Z, self.D, self.count, self.bits, self._new_bad())

    def _begin_pass2(self):
        t, dev = self.solver.torch, self.solver.device
        self.limbs = t.zeros((max(self.D, 1), 4), dtype=t.int64, device=dev)
        self._dev_shifts = tuple(t.from_numpy(np.ascontiguousarray(a)).to(dev) if self.D else t.zeros(1, dtype=t.int32, device=dev)
                                 for a in (self.limb_bits, self.shift1, self.shift2))

    def _add2(self, col, val):
        w, Z, pc, pv = self._args(col, val)
        self.solver.feature_moments(pc, w, pv, Z, self.D, *self._dev_shifts, self.limbs, self._new_bad())

    def host_extent(self):
        return self.count[:self.D].cpu().numpy(), self.bits[:self.D].cpu().numpy().view(np.uint32)

    def set_extent(self, count, bits):
        """After an all-reduce (SUM of count, MAX of the bits): every worker continues from the same pass 1."""
        t = self.solver.torch
        if self.D:
            self.count[:self.D].copy_(t.from_numpy(np.ascontiguousarray(count, np.int64)))
            self.bits[:self.D].copy_(t.from_numpy(np.ascontiguousarray(np.asarray(bits, np.uint32).view(np.int32))))

    def host_limbs(self):
        return self.limbs[:self.D].cpu().numpy()

    def set_limbs(self, limbs):
        t = self.solver.torch
        if self.D:
            self.limbs[:self.D].copy_(t.from_numpy(np.ascontiguousarray(limbs, np.int64).reshape(self.D, 4)))

    def _read_bad(self):
        if not self._bad:
            return []
        t = self.solver.torch
        b = t.stack(self._bad).cpu().numpy()
        return [(int(n), int(i)) for n, i in b]


# ---- one stage's statistics: the passes, the collectives, the file -----------------------------------------------------------------------
def collect(acc, feed, num_samples, kind, all_reduce=None):
    """feed(acc) calls acc.add(col, val) for every partition or chunk of THIS worker's data; it runs once per pass. all_reduce(a, op): an int64
    numpy array reduced over the workers (op "sum" or "max"), or None with one worker. Every worker returns the same FeatureStats: the
    counts, N and the limbs are summed as int64, the bit patterns of the maxima reduced by max — exact on any backend — and everything else
    is derived from them. A bad entry on one worker makes every worker raise (its count travels with the sums: nobody is left waiting)."""
    def finish_pass(own, total, what):
        _raise_bad(own, what)
        if total:
            raise FeatureStatsError(f"feature statistics, {what}: {int(total)} bad entries in another worker's data")

    feed(acc)
    bad = acc.take_bad()
    nbad = sum(n for n, _ in bad)
    N = int(num_samples)
    if all_reduce is not None:
        count, bits = acc.host_extent()
        v = all_reduce(np.concatenate([count, [N, nbad]]).astype(np.int64), "sum")
        count, N, nbad = v[:-2], int(v[-2]), int(v[-1])
        bits = all_reduce(bits.astype(np.int64), "max").astype(np.uint32)
        acc.set_extent(count, bits)
    finish_pass(bad, nbad, "pass 1")
    if passes(kind) == 1:
        return acc.finish(N)
    acc.shifts()
    feed(acc)
    bad = acc.take_bad()
    nbad = sum(n for n, _ in bad)
    if all_reduce is not None:
        v = all_reduce(np.concatenate([acc.host_limbs().ravel(), [nbad]]).astype(np.int64), "sum")
        acc.set_limbs(v[:-1])
        nbad = int(v[-1])
    finish_pass(bad, nbad, "pass 2")
    return acc.finish(N)


def group_all_reduce(group=None, device=None):
    """all_reduce for collect() over torch.distributed's group, or None with one worker. int64 tensors: exact on gloo and on RCCL (there the
    array goes through `device`)."""
    try:
        import torch
        import torch.distributed as dist
    except ImportError:
        return None
    if not (dist.is_available() and dist.is_initialized() and dist.get_world_size(group) > 1):
        return None
    on_device = dist.get_backend(group) == "nccl"

    def all_reduce(a, op):
        t = torch.from_numpy(np.ascontiguousarray(a, np.int64))
        if on_device:
            t = t.to(device)
        dist.all_reduce(t, op=dist.ReduceOp.SUM if op == "sum" else dist.ReduceOp.MAX, group=group)
        return t.cpu().numpy()
    return all_reduce


def all_agree(flag, all_reduce):
    """Does `flag` hold on every worker? (Whether the statistics file is read must be one decision: a worker that reads it takes no part in
    the collectives of those that compute.)"""
    if all_reduce is None:
        return bool(flag)
    return int(all_reduce(np.array([0 if flag else 1], np.int64), "sum")[0]) == 0


def need_two_passes(kind, stats):
    if kind == SCALE_WITH_STANDARD_DEVIATION and np.any(np.isnan(stats.variance)):
        raise FeatureStatsError("the feature statistics file holds no variances (written by a scale_with_max_magnitude run): "
                                "scale_with_standard_deviation needs a file with both passes; remove it or name another")


# ---- the random-effect stage --------------------------------------------------------------------------------------------------------------
def validate(model, execution_context):
    """What the random-effect stage does not do with --feature_normalization, refused before a partition is read or a solver created."""
    mp = model.model_params
    workers = int(execution_context.get("num_workers") or 1)
    path = mp.feature_statistics_file
    if workers > 1 and not (path and os.path.exists(path)):
        raise FeatureStatsError("--feature_normalization with several random-effect workers needs an existing --feature_statistics_file (for instance one "
                                "written by an earlier run with one worker): the random-effect data path has no collective to sum the statistics")


def run(driver, schema_params):
    """The statistics of a random-effect stage, before it trains: the ACTIVE training data of every partition of the partition list, read
    once per pass with one partition decoded ahead; only col / val go to the device, in the wire form when the reader narrowed them.
    Leaves the factors on the model (model.set_feature_factors) -> FeatureStats, or None without --feature_normalization."""
    from . import constants
    from .io.metadata import DatasetMetadata, read_json_file
    model = driver.model
    mp = model.model_params
    kind = check_kind(mp.normalization())
    if kind == NONE or model.feature_bag_name is None:      # (a model without a feature bag has an intercept alone: nothing to scale)
        return None
    ctx = driver.execution_context
    validate(model, {"num_workers": ctx.get(constants.NUM_WORKERS)})
    tensor_metadata = DatasetMetadata(read_json_file(model.metadata_file))
    D = tensor_metadata.get_feature_shape(model.feature_bag_name)[0]
    path = mp.feature_statistics_file
    if path and os.path.exists(path):
        stats = load(path, D)
        need_two_passes(kind, stats)
        logger.info(f"feature statistics read from {path}: no statistics pass")
    else:
        dirs = []
        for p in driver._get_partition_list():
            d = driver._anchor_directory(model.training_data_dir, p)
            if os.path.isdir(d) and os.listdir(d):
                dirs.append(d)
        solver = model._get_solver()
        t = solver.torch
        samples = [0]
        from concurrent.futures import ThreadPoolExecutor
        read = lambda d: model._read_files(d, tensor_metadata, schema_params, D)

        def feed(acc):
            samples[0] = 0
            with ThreadPoolExecutor(max_workers=1, thread_name_prefix="gdmix-stats-read") as pool:      # the next partition is decoded while this one is added
                ahead = pool.submit(read, dirs[0]) if dirs else None
                for i in range(len(dirs)):
                    batch = ahead.result()
                    ahead = pool.submit(read, dirs[i + 1]) if i + 1 < len(dirs) else None
                    samples[0] += batch.N
                    if batch.Z:
                        col = batch.to_wire()["col_global"] if hasattr(batch, "_col") else batch.col_global
                        acc.add(t.from_numpy(np.ascontiguousarray(col)).to(solver.device), t.from_numpy(np.ascontiguousarray(batch.val)).to(solver.device))
                    del batch

        acc = DeviceAccumulator(solver, D)
        feed(acc)                       # N is known after the first pass over the data
        n_first = samples[0]
        first = [True]

        def feed_once(a):               # collect() feeds pass 1 itself: hand it the pass already made
            if first[0]:
                first[0] = False
                return
            feed(a)
        stats = collect(acc, feed_once, n_first, kind)
        if path and ctx.get(constants.IS_CHIEF, True):
            save(path, stats)
            logger.info(f"feature statistics of {stats.num_samples} samples written to {path}")
    model.set_feature_factors(factors(kind, stats))
    return stats


# ---- the fixed-effect stage ----------------------------------------------------------------------------------------------------------------
def fixed_effect_factors(kind, path, solver, num_features, col_dev, val_dev, num_samples, group=None, is_chief=True):
    """Factors [num_features] of a fixed-effect stage, identical on every worker: from the statistics file when every worker finds it,
    otherwise pass 1 and pass 2 on this worker's device shard (col_dev / val_dev: device tensors, or None for an empty shard — the worker
    still takes part in the collectives) with the integers all-reduced in between; the chief writes the file."""
    all_reduce = group_all_reduce(group, solver.device)
    if all_agree(bool(path) and os.path.exists(path), all_reduce):
        stats = load(path, num_features)
        need_two_passes(kind, stats)
        logger.info(f"feature statistics read from {path}: no statistics pass")
    else:
        def feed(acc):
            if col_dev is not None and col_dev.numel():
                acc.add(col_dev, val_dev)
        stats = collect(DeviceAccumulator(solver, num_features), feed, num_samples, kind, all_reduce)
        if path and is_chief:
            save(path, stats)
            logger.info(f"feature statistics of {stats.num_samples} samples written to {path}")
    return factors(kind, stats), stats
