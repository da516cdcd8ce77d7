"""--features_to_samples_ratio: per-entity feature selection by Pearson correlation, stated in numpy.

The definition is in include/gdmix_re.h, "feature selection"; the device pass is csrc/re_select.hip (REDeviceSolver.select_features).
For one entity with n samples, labels y_i and cells x_ij (the fp64 sum of the entity's duplicates of (sample i, feature j)):

    Sy = sum y_i, Syy = sum y_i^2;  per feature, over its cells in sample order: Sx, Sxx, Sxy
    A = n Sxy - Sx Sy,  Bx = n Sxx - Sx^2,  By = n Syy - Sy^2
    q = A^2 / Bx  if Bx > 2^-30 n Sxx and By > 2^-30 n Syy, else 0;  key = float32(q)
    rank by key descending, then by feature index ascending; keep the first k_e = min(d_e, ceil(R n_e))

Unweighted, offsets ignored; the intercept is not a feature and takes no slot (in Photon-ML's numFeaturesToSamplesRatioUpperBound it
takes one). A feature that occurs in one sample only scores (n y_i - Sy)^2 / (n - 1) whatever its value, so exact ties at the boundary
are the rule: the rank is taken on the fp32 key with the feature index as the tie-break, and select() is exact given the keys. The sums
here are fp64 sums, a column's in the device's order and the label sums in sample order (the device adds those as a tree); the two agree to
the bound the header derives, not bit for bit.
"""
import math

import numpy as np

from .batch import RawBatch

GUARD = 2.0 ** -30


def k_of(ratio, n, d):
    """k_e = min(d_e, (int64)ceil(R * (double)n_e)) for one entity."""
    ratio = float(ratio)
    if not math.isfinite(ratio) or ratio <= 0.0:
        raise ValueError(f"the ratio must be finite and above 0, not {ratio!r}")
    t = ratio * float(int(n))       # (may be infinite)
    return int(d) if t >= float(int(d)) else min(int(d), int(math.ceil(t)))


def k_all(ratio, ent_n, ent_d):
    """k_of for arrays of n_e and d_e -> int64 [E]."""
    ratio = float(ratio)
    if not math.isfinite(ratio) or ratio <= 0.0:
        raise ValueError(f"the ratio must be finite and above 0, not {ratio!r}")
    ent_d = np.asarray(ent_d, np.int64)
    t = np.ceil(ratio * np.asarray(ent_n, np.int64).astype(np.float64))
    return np.where(t >= ent_d.astype(np.float64), ent_d, np.minimum(t, 2.0 ** 62).astype(np.int64))


def slots(batch):
    """The entity features of a batch in the order of the pack's unique_global (entity-major, global index ascending inside an entity)
    -> (ent_feat_ptr int64 [E+1], unique_global int64 [D], nnz_slot int64 [Z]: the slot of every non-zero, nnz_row int64 [Z])."""
    E, N, Z = batch.E, batch.N, batch.Z
    nnz_row = np.repeat(np.arange(N, dtype=np.int64), np.diff(batch.row_nnz_ptr))
    row_ent = np.repeat(np.arange(E, dtype=np.int64), np.diff(batch.ent_row_ptr))
    nnz_ent = row_ent[nnz_row]
    span = int(batch.col_global.max()) + 1 if Z else 1
    uniq, nnz_slot = np.unique(nnz_ent * span + batch.col_global, return_inverse=True)
    ent_feat_ptr = np.zeros(E + 1, np.int64)
    np.cumsum(np.bincount(uniq // span, minlength=E), out=ent_feat_ptr[1:])
    return ent_feat_ptr, uniq % span, nnz_slot.astype(np.int64).ravel(), nnz_row


def moments(batch, sl=None):
    """-> dict(ent_feat_ptr, unique_global, nnz_slot, slot_ent, n [D], Sx, Sxx, Sxy, Sy, Syy [D] fp64): the sums of the definition, per slot."""
    ent_feat_ptr, unique_global, nnz_slot, nnz_row = slots(batch) if sl is None else sl
    E, N, D = batch.E, batch.N, unique_global.size
    # cells: duplicates of (slot, sample) summed in fp64; np.unique sorts them by (slot, sample), i.e. each column in sample order
    cell_key, cell_of = np.unique(nnz_slot * max(N, 1) + nnz_row, return_inverse=True)
    cell = np.bincount(cell_of.ravel(), weights=batch.val.astype(np.float64), minlength=cell_key.size)
    cell_slot, cell_row = cell_key // max(N, 1), cell_key % max(N, 1)
    y = batch.y.astype(np.float64)
    Sx = np.bincount(cell_slot, weights=cell, minlength=D)          # bincount adds one term after another, in order
    Sxx = np.bincount(cell_slot, weights=cell * cell, minlength=D)
    Sxy = np.bincount(cell_slot, weights=cell * y[cell_row], minlength=D)
    row_ent = np.repeat(np.arange(E, dtype=np.int64), np.diff(batch.ent_row_ptr))
    slot_ent = np.repeat(np.arange(E, dtype=np.int64), np.diff(ent_feat_ptr))
    Sy = np.bincount(row_ent, weights=y, minlength=E)
    Syy = np.bincount(row_ent, weights=y * y, minlength=E)
    n = np.diff(batch.ent_row_ptr).astype(np.float64)
    return dict(ent_feat_ptr=ent_feat_ptr, unique_global=unique_global, nnz_slot=nnz_slot, slot_ent=slot_ent, n=n[slot_ent], Sx=Sx, Sxx=Sxx, Sxy=Sxy,
                Sy=Sy[slot_ent], Syy=Syy[slot_ent])


def keys(batch, m=None):
    """-> (ent_feat_ptr [E+1], unique_global [D], key float32 [D])."""
    m = moments(batch) if m is None else m
    n, Sx, Sxx, Sxy, Sy, Syy = (m[k] for k in ("n", "Sx", "Sxx", "Sxy", "Sy", "Syy"))
    A, Bx, By = n * Sxy - Sx * Sy, n * Sxx - Sx * Sx, n * Syy - Sy * Sy
    ok = (Bx > GUARD * n * Sxx) & (By > GUARD * n * Syy)
    with np.errstate(all="ignore"):
        q = np.where(ok, A * A / np.where(ok, Bx, 1.0), 0.0)
        key = q.astype(np.float32)
    key[~(key >= 0)] = 0.0
    return m["ent_feat_ptr"], m["unique_global"], key


def select(ent_feat_ptr, ent_n, key, ratio):
    """The mask, exactly, given the keys: per entity the first k_e slots by (key descending, slot ascending) -> bool [D]."""
    ent_feat_ptr = np.asarray(ent_feat_ptr, np.int64)
    D = int(ent_feat_ptr[-1])
    d = np.diff(ent_feat_ptr)
    k = k_all(ratio, ent_n, d)
    slot_ent = np.repeat(np.arange(d.size, dtype=np.int64), d)
    order = np.lexsort((np.arange(D), -np.asarray(key, np.float32).astype(np.float64), slot_ent))
    keep = np.zeros(D, bool)
    keep[order] = (np.arange(D) - ent_feat_ptr[slot_ent]) < k[slot_ent]     # (lexsort keeps entities in order: slot_ent[order] == slot_ent)
    return keep


def filter_batch(batch, nnz_slot, keep):
    """The raw batch without the non-zeros of dropped slots; rows, labels, offsets and weights stay."""
    kept = np.asarray(keep, bool)[nnz_slot]
    row_nnz_ptr = np.zeros(batch.N + 1, np.int64)
    nnz_row = np.repeat(np.arange(batch.N, dtype=np.int64), np.diff(batch.row_nnz_ptr))
    np.cumsum(np.bincount(nnz_row[kept], minlength=batch.N), out=row_nnz_ptr[1:])
    return RawBatch(batch.ent_row_ptr, row_nnz_ptr, batch.col_global[kept], batch.val[kept], batch.y, batch.offset, batch.weight, uid=batch.uid,
                    entity_ids=batch.entity_ids, has_label=batch.has_label, binary_labels=batch.binary_labels, trusted=batch.trusted)


def counts(ent_feat_ptr, ent_n, keep, nnz_slot, ratio):
    """What gdmix_re_select_plan reports -> dict(entities, affected, features, kept, dropped, kept_nnz)."""
    d = np.diff(np.asarray(ent_feat_ptr, np.int64))
    k = k_all(ratio, ent_n, d)
    keep = np.asarray(keep, bool)
    return dict(entities=int(d.size), affected=int((k < d).sum()), features=int(d.sum()), kept=int(keep.sum()), dropped=int(d.sum() - keep.sum()),
                kept_nnz=int(keep[nnz_slot].sum()))


def select_batch(batch, ratio):
    """The whole statement -> (filtered RawBatch, keep bool [D], key float32 [D], counts)."""
    m = moments(batch)
    fp, _, key = keys(batch, m)
    ent_n = np.diff(batch.ent_row_ptr)
    keep = select(fp, ent_n, key, ratio)
    return filter_batch(batch, m["nnz_slot"], keep), keep, key, counts(fp, ent_n, keep, m["nnz_slot"], ratio)
