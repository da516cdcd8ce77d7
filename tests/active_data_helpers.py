"""Shared by tests/test_active_data_host.py (CPU) and tests/test_gpu_active_data.py (GPU): the small batches the active-data cap
(--active_data_upper_bound; include/gdmix_re.h, "active-data cap"; gdmix_amd/active_data.py) is held to, and the host-capped RawBatch.

edge_batch(K): entities of n_e in {1, K - 1, K, K + 1, 2 K, 63, 64, 65, 128, 129, 1024, 1025, 5000} — an entity without rows at K = 1, both
sides of the bound, of a wavefront, of the default limit between the counting path and the radix select (128) and of the largest limit
(1024) — one whose uids are all equal (the order of the rows decides alone), one with a block of equal uids across the K-th position of
the order, and one of 2 100 rows more, so that rows of capped entities lie on both sides of several 2 048-row chunk boundaries of the
scans. Rows have 0 .. 5 non-zeros over 64 features.
"""
import dataclasses
import functools

import numpy as np

from gdmix_amd import active_data as ad
from gdmix_amd.batch import RawBatch

KS = (1, 2, 64, 100)
SEED = 20240603
CHUNK = 2048            # DS_CHUNK of csrc/re_rowsubset.hpp
TIE_ROWS = 150          # the entity whose uids are all equal: above every K of KS
D = 64


def sizes(K):
    return [1, K - 1, K, K + 1, 2 * K, 63, 64, 65, 1024, 1025, 5000, TIE_ROWS, 3 * K + 40, 2100, 128, 129]


TIE_ENTITY, BLOCK_ENTITY = 11, 12      # positions in sizes()


@functools.lru_cache(maxsize=None)
def edge_batch(K, with_weight=True, seed=SEED):
    rng = np.random.default_rng([K, 77])
    n = np.array(sizes(K), np.int64)
    erp = np.concatenate([[0], np.cumsum(n)]).astype(np.int64)
    N = int(erp[-1])
    k = rng.integers(0, 6, N)
    rp = np.concatenate([[0], np.cumsum(k)]).astype(np.int64)
    col = rng.integers(0, D, rp[-1]).astype(np.int64)
    val = rng.standard_normal(rp[-1]).astype(np.float32)
    uid = rng.permutation(np.arange(-N, 2 * N, dtype=np.int64) * 0x9E3779B1 + 12345)[:N]      # distinct, of either sign
    uid[int(erp[8])], uid[int(erp[8]) + 1], uid[int(erp[8]) + 2] = -1, -2 ** 63, 0
    assert np.unique(uid).size == N
    # one entity with one uid: the K first rows are kept
    uid[erp[TIE_ENTITY]:erp[TIE_ENTITY + 1]] = 424242
    # a block of equal uids across the K-th position: the row of rank K - 1, up to three rows in front of it and five behind it share its uid
    r0, r1 = int(erp[BLOCK_ENTITY]), int(erp[BLOCK_ENTITY + 1])
    order = np.argsort(ad.key(seed, uid[r0:r1]), kind="stable")
    block = np.concatenate([order[max(0, K - 1 - 3):K - 1], order[K - 1:K + 5]])
    uid[r0 + block] = uid[r0 + order[K - 1]]
    y = (rng.random(N) < 0.4).astype(np.float32)
    off = (0.5 * rng.standard_normal(N)).astype(np.float32)
    w = (0.25 + rng.random(N)).astype(np.float32) if with_weight else None
    b = RawBatch(ent_row_ptr=erp, row_nnz_ptr=rp, col_global=col, val=val, y=y, offset=off, weight=w, uid=uid,
                 entity_ids=[str(100 + e) for e in range(n.size)])
    kept = ad.keep_mask(erp, uid, K, seed)
    tied = np.zeros(N, bool)
    tied[r0 + block] = True
    assert 0 < (kept & tied).sum() < block.size                                           # the block straddles the K-th position
    assert kept[erp[TIE_ENTITY]:erp[TIE_ENTITY] + K].all() and kept[erp[TIE_ENTITY]:erp[TIE_ENTITY + 1]].sum() == K
    capped = np.flatnonzero(n > K)
    assert any(erp[e] // CHUNK != (erp[e + 1] - 1) // CHUNK for e in capped)              # a capped entity across a chunk boundary
    return b


K_SOLVE = 16


@functools.lru_cache(maxsize=None)
def solve_batch():
    """48 entities of 14 .. 38 rows (four non-zeros a row over 16 features, random weights, scattered uids), for the solves at K_SOLVE =
    16: 46 of them are capped, by factors n_e / K of at most 2.4, so that every fit of the three losses ends by a stopping test inside the
    100 iterations the comparisons run with. (The parity rules compare stopping points: a fit cut off at the iteration limit has none, and
    the edge batch's factors of up to 5000 / K weaken the regulariser against the data that far.)"""
    from gdmix_amd import synthetic
    b = synthetic.make_batch(48, 24, 4, 16, seed=7, size_dist="poisson", random_weights=True, with_uid=True)
    b = dataclasses.replace(b, uid=b.uid * 0x9E3779B1 - 7_000_000_000)
    n = b.ent_n()
    assert 0 < (n <= K_SOLVE).sum() < (n > K_SOLVE).sum()
    return b


def empty_batch():
    z = lambda dt: np.zeros(0, dt)
    return RawBatch(ent_row_ptr=np.zeros(1, np.int64), row_nnz_ptr=np.zeros(1, np.int64), col_global=z(np.int64), val=z(np.float32), y=z(np.float32),
                    offset=z(np.float32), weight=None, uid=z(np.int64), entity_ids=[])


def host_cap(b, K, seed=SEED):
    """active_data.apply_host on a RawBatch -> its dict."""
    return ad.apply_host(b.ent_row_ptr, b.row_nnz_ptr, b.col_global, b.val, b.y, b.offset, b.weight, b.uid, K, seed)


def capped_batch(b, K, seed=SEED):
    """The RawBatch the solver sees under the cap, from the numpy statement."""
    h = host_cap(b, K, seed)
    return RawBatch(ent_row_ptr=h["ent_row_ptr"], row_nnz_ptr=h["row_nnz_ptr"], col_global=h["col_global"], val=h["val"], y=h["y"], offset=h["offset"],
                    weight=h["weight"], uid=b.uid[h["kept_rows"]], entity_ids=b.entity_ids, has_label=b.has_label, binary_labels=b.binary_labels)


def reversed_entities(b):
    """The same entities in the opposite order."""
    return b.select(np.arange(b.E)[::-1])


def counts_of(b, K, h):
    n = b.ent_n()
    return dict(entities=b.E, capped=int((n > K).sum()), rows=b.N, kept=int(h["y"].size), kept_nnz=int(h["val"].size), largest=int(n.max()) if b.E else 0)


def with_labels(b, kind, seed=5):
    """kind: logistic (the planted 0 / 1 labels), squared (real-valued) or poisson (counts)."""
    from gdmix_amd import synthetic
    if kind == "squared":
        return synthetic.with_real_labels(b, seed)
    if kind == "poisson":
        return synthetic.with_count_labels(b, seed)
    return dataclasses.replace(b)
