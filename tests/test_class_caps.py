"""CPU checks of what tests/test_gpu_class_caps.py stands on, so that it cannot pass by leaving entities out: the generator gives exactly
the stated (p, n, nnz), class_caps_helpers.route places every entity where the shape list says, the wavefront-bucket shapes have the
stated byte counts, and the REFERENCE's own run of every case is reproducible (strict) on every class."""
import numpy as np
import pytest

import class_caps_helpers as ch
from oracle import oracle


def test_the_table_is_in_routing_order():
    """28 group classes: the coefficient cap never falls, and inside a kind both other caps rise (first fit means the smallest that holds)."""
    assert len(ch.GROUP_CLASSES) == 28 and len(ch.class_names()) == 30
    for a, b in zip(ch.GROUP_CLASSES, ch.GROUP_CLASSES[1:]):
        assert a[0] * a[1] <= b[0] * b[1]
        if a[:2] == b[:2]:
            assert a[2] < b[2] and a[3] < b[3]
    assert len({g * epl for g, epl, _, _ in ch.GROUP_CLASSES}) == 12


@pytest.mark.parametrize("name", ["edges", "neighbours", "corners-logistic", "corners_no_intercept-logistic", "wave", "wave_weights"])
def test_shaped_batches_have_the_stated_shapes(name):
    c = ch.case(name)
    b, shapes = c["b"], c["shapes"]
    b.validate()
    pk = oracle.pack(b.ent_row_ptr, b.row_nnz_ptr, b.col_global)
    assert np.array_equal(np.diff(pk["ent_feat_ptr"]) + c["ic"], [s[0] for s in shapes])
    assert np.array_equal(b.ent_n(), [s[1] for s in shapes]) and np.array_equal(b.ent_nnz(), [s[2] for s in shapes])
    assert (b.weight is not None) == (name.startswith("corners") or name == "wave_weights")


def test_route_places_corners_and_edges_in_their_classes():
    corners, edges = ch.corners(), ch.edges()
    assert len(corners) == 28 and len(edges) == 121
    for ic in (1, 0):
        for has_w in (False, True):
            assert [ch.route(p, n, z, 10, has_w, 0, ic=ic) for p, n, z, _ in corners] == list(range(28))
    assert [ch.route(p, n, z, 10, False, 0) for p, n, z, _ in edges] == [k for _, _, _, k in edges]
    per_class = np.bincount([k for _, _, _, k in edges], minlength=28)
    assert per_class.min() >= 3, per_class                     # (the corner, one non-zero per row or column, the middle of the range)
    for k, (g, epl, ncap, zcap) in enumerate(ch.GROUP_CLASSES):
        mine = [(p, n, z) for p, n, z, c in edges if c == k]
        assert (g * epl, ncap, zcap) in mine and max(p for p, _, _ in mine) == g * epl
        assert max(n for _, n, _ in mine) == ncap and max(z for _, _, z in mine) == zcap
    # more than ten pairs: no group class, whatever the shape
    assert all(ch.route(p, n, z, 12, False, 0) >= ch.WAVE_24K for p, n, z, _ in corners)
    # the tall rule takes p <= 64 and n >= 32, and nothing else
    for p, n, z, k in edges:
        tall = ch.route(p, n, z, 10, False, 32)
        assert (tall in (ch.TALL_LEAN_CLASS, ch.TALL_ONE_CLASS)) == (p <= 64 and n >= 32) and (tall == k or (p <= 64 and n >= 32))
    assert sum(ch.route(p, n, z, 10, False, 32) != k for p, n, z, k in edges) >= 9


def test_neighbours_leave_the_class_whose_cap_they_exceed():
    nb = ch.neighbours()
    assert len(nb) == 84
    for p, n, z, c, past in nb:
        g, epl, ncap, zcap = ch.GROUP_CLASSES[past]
        assert c != past and c > past and (p == g * epl + 1) + (n == ncap + 1) + (z == zcap + 1) == 1
        if c < 28:
            g2, epl2, ncap2, zcap2 = ch.GROUP_CLASSES[c]
            assert p <= g2 * epl2 and n <= ncap2 and z <= zcap2
    assert ch.BLOCK_CLASS in {c for _, _, _, c, _ in nb}       # what fits nothing is the workgroup class (m = 10: the wavefront buckets lie in between)


@pytest.mark.parametrize("has_w", [False, True])
def test_wave_bucket_shapes_have_the_stated_bytes(has_w):
    shapes = ch.wave_bucket_shapes(has_w)
    assert sorted({s[4] for s in shapes}) == [24576, 24592, 65536, 65552]
    for p, n, z, c, size in shapes:
        assert ch.wave_lds_bytes(p, n, z, p - 1, 12, has_w) == size
        assert ch.wave_lds_bytes(p, n, z - 1, p - 1, 12, has_w) == size - 16
        assert c == {24576: ch.WAVE_24K, 24592: ch.WAVE_64K, 65536: ch.WAVE_64K, 65552: ch.BLOCK_CLASS}[size]
    for size in (24576, 24592, 65536, 65552):
        assert len({(p, n) for p, n, _, _, s in shapes if s == size}) >= 2
    if not has_w:      # the figures worked out by hand from csrc/re_internal.hpp
        for d, n, z, size in ((59, 8, 628, 24576), (59, 8, 629, 24592), (65, 40, 3060, 65536), (65, 40, 3061, 65552), (257, 8, 268, 65536), (257, 8, 269, 65552)):
            assert ch.wave_lds_bytes(d + 1, n, z, d, 12, False) == size
            assert (d + 1, n, z) in {s[:3] for s in shapes}


@pytest.mark.parametrize("name", ch.case_names())
def test_the_reference_is_strict_on_every_class(name):
    """Every class of the case has an entity the reference reproduces from starts moved by 1e-15, 1e-14 and 1e-13 and that is no FACTR
    stop, and at least 90 % of all entities are such: the GPU test compares those iteration for iteration."""
    c, r = ch.case(name), ch.reference(name)
    cls = np.array([s[3] for s in c["shapes"]])
    strict, nit = r["strict"], r["nit"]
    print(f"{name} ({c['loss']}): {int(strict.sum())} of {strict.size} strict, nit {int(nit.min())} .. {int(nit.max())}")
    assert strict.size == c["b"].E == len(c["shapes"])
    assert all(strict[cls == k].any() for k in np.unique(cls)), sorted(set(cls[~strict].tolist()))
    assert strict.mean() >= 0.9, float(strict.mean())
    if name in ("edges", "neighbours") or name.startswith("corners"):
        assert set(cls.tolist()) >= ({ch.BLOCK_CLASS} if name == "neighbours" else set(range(28)))
    if name == "edges":
        # l2 = 1 is enough (no need for 0.1 or 0.01): in every lane width an entity runs past m = 10 iterations, so the history wraps
        lanes = np.array([ch.GROUP_CLASSES[k][0] for k in cls])
        past = {int(g): int(nit[strict & (lanes == g)].max()) for g in np.unique(lanes)}
        print(f"edges: most iterations per lane width {past}")
        assert sorted(past) == [16, 32, 64, 128, 256, 512] and min(past.values()) > c["kw"]["m"], past
