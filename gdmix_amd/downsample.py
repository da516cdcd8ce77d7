"""Down-sampling of a training shard, stated in numpy (include/gdmix_re.h, "down-sampling": this module is the definition).

Photon-ML's downSamplingRate: the fixed-effect stage trains on a sample of its shard that keeps every positive (logistic loss) and a
negative with probability `rate`, kept negatives weighted 1 / rate. A row's fate is a pure function of (seed, uid), so the kept set does
not depend on the partitioning, on the order of the rows or on the number of workers; rows with equal uids share a fate.

Only tests use this module: the product path is REDeviceSolver.downsample (csrc/re_downsample.hip) and has no CPU fallback.
"""
import math

import numpy as np

_M64 = 0xFFFFFFFFFFFFFFFF


def mix(x):
    """splitmix64's output function on uint64, wrapping: a Python int -> int, an array -> uint64 array. mix(0) = 0xE220A8397B1DCDAF."""
    if isinstance(x, (int, np.integer)):
        x = (int(x) + 0x9E3779B97F4A7C15) & _M64
        x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & _M64
        x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & _M64
        return x ^ (x >> 31)
    x = np.asarray(x, np.uint64)
    with np.errstate(over="ignore"):
        x = x + np.uint64(0x9E3779B97F4A7C15)
        x = (x ^ (x >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        x = (x ^ (x >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        return x ^ (x >> np.uint64(31))


def draw(seed, uid):
    """mix((uint64)uid ^ mix(seed)) >> 32 for every uid (int64, reinterpreted as unsigned) -> uint64 array of values below 2^32."""
    u = np.ascontiguousarray(uid, np.int64).view(np.uint64)
    return mix(u ^ np.uint64(mix(int(seed) & _M64))) >> np.uint64(32)


def check_rate(rate):
    """0 < rate <= 1, finite; -> float."""
    r = float(rate)
    if not (math.isfinite(r) and 0.0 < r <= 1.0):
        raise ValueError(f"a down-sampling rate lies in (0, 1], not {rate!r}")
    return r


def threshold(rate):
    """T = (uint64)(rate * 2^32): the product is exact; 0 for a rate below 2^-32, 2^32 at rate 1."""
    return int(check_rate(rate) * 4294967296.0)


def keep_mask(uid, y, rate, seed, negatives_only):
    """bool [N]: the rows a down-sampling pass keeps. negatives_only: rows with label > 0.5 are always kept."""
    kept = draw(seed, uid) < np.uint64(threshold(rate))
    if negatives_only:
        kept = kept | (np.asarray(y, np.float32) > np.float32(0.5))
    return kept


def scaled_weight(weight, y, rate, negatives_only):
    """float32 [N]: the weight a row has IF it is kept — float32(float64(w) / rate) for a row subject to sampling, w for an always-kept
    positive; w = 1 where `weight` is None."""
    y = np.asarray(y, np.float32)
    w = np.ones(y.size, np.float32) if weight is None else np.asarray(weight, np.float32)
    scaled = (w.astype(np.float64) / check_rate(rate)).astype(np.float32)
    if negatives_only:
        return np.where(y > np.float32(0.5), w, scaled)
    return scaled


def apply_host(ent_row_ptr, row_nnz_ptr, col_global, val, y, offset, weight, uid, rate, seed, negatives_only):
    """The filtered raw arrays: dict(ent_row_ptr, row_nnz_ptr, col_global, val, y, offset, weight, kept_rows); kept rows in their order,
    weight always an array."""
    erp = np.asarray(ent_row_ptr, np.int64)
    rp = np.asarray(row_nnz_ptr, np.int64)
    col, v = np.asarray(col_global, np.int64), np.asarray(val, np.float32)
    y = np.asarray(y, np.float32)
    n = rp.size - 1
    off = np.zeros(n, np.float32) if offset is None else np.asarray(offset, np.float32)
    kept = keep_mask(uid, y, rate, seed, negatives_only)
    rows = np.flatnonzero(kept)
    scan = np.concatenate([[0], np.cumsum(kept)]).astype(np.int64)
    k = (rp[1:] - rp[:-1])[rows]
    out_rp = np.concatenate([[0], np.cumsum(k)]).astype(np.int64)
    src = np.repeat(rp[:-1][rows] - out_rp[:-1], k) + np.arange(out_rp[-1], dtype=np.int64)
    return dict(ent_row_ptr=scan[erp], row_nnz_ptr=out_rp, col_global=col[src], val=v[src], y=y[rows], offset=off[rows],
                weight=scaled_weight(weight, y, rate, negatives_only)[rows], kept_rows=rows.astype(np.int64))
