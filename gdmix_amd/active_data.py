"""The active-data cap of a random-effect stage, stated in numpy (include/gdmix_re.h, "active-data cap": this module is the definition).

Photon-ML's activeDataUpperBound: an entity of more than K samples trains on a uniform sample of K of them, each weighted n_e / K, so
that the objective stays an unbiased estimate of the full one. The sample is the K rows smallest by (key(seed, uid), row): with distinct
uids it is a function of (seed, the entity's set of uids, K) alone, nested in K; rows with equal uids tie and are admitted in row order.

Only tests use this module: the product path is REDeviceSolver.cap_samples (csrc/re_cap.hip) and has no CPU fallback.
"""
import math

import numpy as np

from .downsample import _M64, mix


def key(seed, uid):
    """mix((uint64)uid ^ mix(seed)), all 64 bits, for every uid (int64, reinterpreted as unsigned) -> uint64 array (a scalar uid: 0-d)."""
    u = np.ascontiguousarray(uid, np.int64).view(np.uint64)
    return mix(u ^ np.uint64(mix(int(seed) & _M64)))


def check_upper_bound(value):
    """--active_data_upper_bound: an integer >= 1 (an int, an integral float or its text) -> int."""
    bad = ValueError(f"--active_data_upper_bound={value!r}: an integer >= 1")
    if isinstance(value, (bool, np.bool_)):
        raise bad
    if isinstance(value, (int, np.integer)):
        k = int(value)
    else:
        try:
            f = float(value)
        except (TypeError, ValueError):
            raise bad from None
        if not math.isfinite(f) or f != math.floor(f):
            raise bad
        k = int(f)
    if k < 1:
        raise bad
    return k


def keep_mask(ent_row_ptr, uid, K, seed):
    """bool [N]: the rows the cap keeps. Per entity of more than K rows the K smallest by (key, row); every row of any other entity."""
    K = check_upper_bound(K)
    erp = np.asarray(ent_row_ptr, np.int64)
    k = key(seed, uid)
    kept = np.ones(k.size, bool)
    for e in range(erp.size - 1):
        r0, r1 = int(erp[e]), int(erp[e + 1])
        if r1 - r0 > K:
            order = np.argsort(k[r0:r1], kind="stable")      # ties keep their row order
            kept[r0:r1] = False
            kept[r0 + order[:K]] = True
    return kept


def scaled_weight(ent_row_ptr, weight, K, n_rows=None):
    """float32 [N]: the weight a row has IF it is kept — float32((float64(w) * n_e) / K) for a row of an entity of more than K rows, w
    for any other; w = 1 where `weight` is None (n_rows then gives N, default ent_row_ptr[-1])."""
    K = check_upper_bound(K)
    erp = np.asarray(ent_row_ptr, np.int64)
    n = int(erp[-1]) if n_rows is None else int(n_rows)
    w = np.ones(n, np.float32) if weight is None else np.asarray(weight, np.float32).copy()
    ne = np.zeros(n, np.float64)
    for e in range(erp.size - 1):
        r0, r1 = int(erp[e]), int(erp[e + 1])
        ne[r0:r1] = r1 - r0
    capped = ne > K
    w[capped] = ((w[capped].astype(np.float64) * ne[capped]) / np.float64(K)).astype(np.float32)
    return w


def apply_host(ent_row_ptr, row_nnz_ptr, col_global, val, y, offset, weight, uid, K, seed):
    """The capped raw arrays: dict(ent_row_ptr, row_nnz_ptr, col_global, val, y, offset, weight, kept_rows); kept rows in their order,
    weight always an array (what downsample.apply_host returns)."""
    erp = np.asarray(ent_row_ptr, np.int64)
    rp = np.asarray(row_nnz_ptr, np.int64)
    col, v = np.asarray(col_global, np.int64), np.asarray(val, np.float32)
    y = np.asarray(y, np.float32)
    n = rp.size - 1
    off = np.zeros(n, np.float32) if offset is None else np.asarray(offset, np.float32)
    kept = keep_mask(erp, uid, K, seed)
    rows = np.flatnonzero(kept)
    scan = np.concatenate([[0], np.cumsum(kept)]).astype(np.int64)
    k = (rp[1:] - rp[:-1])[rows]
    out_rp = np.concatenate([[0], np.cumsum(k)]).astype(np.int64)
    src = np.repeat(rp[:-1][rows] - out_rp[:-1], k) + np.arange(out_rp[-1], dtype=np.int64)
    return dict(ent_row_ptr=scan[erp], row_nnz_ptr=out_rp, col_global=col[src], val=v[src], y=y[rows], offset=off[rows],
                weight=scaled_weight(erp, weight, K, n_rows=n)[rows], kept_rows=rows.astype(np.int64))
