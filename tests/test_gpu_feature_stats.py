"""The column-statistics kernels (csrc/feature_stats.hip; include/gdmix_re.h, "feature normalisation") on the MI355X against the reference
in Python integers (tests/feature_stats_helpers.py). Equality is exact everywhere: the accumulators are integers, and integer addition
commutes. Runs on the MI355X box only.

Shapes: the smallest that reach each failure — one address for every add with an odd tail; 24 features on the LDS path in all three id
widths; 70 001 Zipf features past uint16 and past LDS; no entry and one entry; seven uneven chunks (device slices: unaligned starts take
the one-entry-per-lane kernels, fresh uploads the 16-byte ones); the LDS threshold forced either way at 24 and at 4 000 features (4 000
needs more LDS than a workgroup has without asking); bad entries planted at known indices; the expansion to coefficient order; and a
few hundred C2-shaped entities solved in normalised units with one column multiplied by 8."""
import numpy as np
import pytest

import feature_stats_helpers as fh
from gdmix_amd import feature_stats as fs
from gdmix_amd import synthetic
from gdmix_amd.solver import SolverOptions

pytestmark = pytest.mark.gpu

_ref_cache = {}


def case(name):
    """(col, val, D, reference) of a case, computed once and left unchanged."""
    if name not in _ref_cache:
        col, val, D = getattr(fh, "case_" + name)()
        _ref_cache[name] = (col, val, D, fh.reference(col, val, D))
    return _ref_cache[name]


def up(solver, a):
    return solver.torch.from_numpy(np.ascontiguousarray(a)).to(solver.device)


def both_passes(solver, D, chunks):
    """chunks: [(col tensor, val tensor)] fed once per pass -> dict(count, bits, L, s1, s2, limbs, bad1, bad2)."""
    acc = fs.DeviceAccumulator(solver, D)
    for c, v in chunks:
        acc.add(c, v)
    bad1 = acc.take_bad()
    count, bits = acc.host_extent()
    L, s1, s2 = acc.shifts()
    for c, v in chunks:
        acc.add(c, v)
    bad2 = acc.take_bad()
    return dict(count=count, bits=bits, L=L, s1=s1, s2=s2, limbs=acc.host_limbs(), bad1=bad1, bad2=bad2, acc=acc)


def assert_equals_reference(got, ref, calls=1):
    assert got["bad1"] == [(0, -1)] * calls and got["bad2"] == [(0, -1)] * calls
    assert np.array_equal(got["count"], ref["count"])
    assert np.array_equal(got["bits"], ref["bits"])
    assert np.array_equal(got["L"], ref["L"]) and np.array_equal(got["s1"], ref["s1"]) and np.array_equal(got["s2"], ref["s2"])
    assert np.array_equal(got["limbs"], ref["limbs"])


# ---- 1 - 3: one address, the LDS path in three widths, Zipf past uint16 and LDS ---------------------------------------------------------
def test_one_address_with_an_odd_tail(device_solver):
    col, val, D, ref = case("one_address")
    assert col.size % 4 == 3
    assert_equals_reference(both_passes(device_solver, D, [(up(device_solver, col), up(device_solver, val))]), ref)


def test_lds_path_and_the_three_id_widths(device_solver):
    col, val, D, ref = case("lds")
    v = up(device_solver, val)
    for dt in (np.uint16, np.int32, np.int64):
        assert_equals_reference(both_passes(device_solver, D, [(up(device_solver, col.astype(dt)), v)]), ref)


def test_zipf_columns_past_uint16_and_past_lds(device_solver):
    col, val, D, ref = case("zipf")
    assert D > 0xffff and D > 5000 and float((ref["count"] == 0).mean()) > 0.25 and int(ref["count"].max()) > col.size // 5
    v = up(device_solver, val)
    got = both_passes(device_solver, D, [(up(device_solver, col), v)])
    assert_equals_reference(got, ref)
    assert_equals_reference(both_passes(device_solver, D, [(up(device_solver, col.astype(np.int32)), v)]), ref)
    # mean and variance from the device's integers: those of the stand-in, bit for bit
    dev = got["acc"].finish(1000)
    cpu = fs.NumpyAccumulator(D)
    stats = fs.collect(cpu, lambda a: a.add(col, val), 1000, fs.SCALE_WITH_STANDARD_DEVIATION)
    assert dev.equal_bits(stats)


# ---- 4: no entry, one entry ---------------------------------------------------------------------------------------------------------------
def test_no_entry_and_one_entry(device_solver):
    t = device_solver.torch
    empty = (t.empty(0, dtype=t.int64, device=device_solver.device), t.empty(0, dtype=t.float32, device=device_solver.device))
    got = both_passes(device_solver, 7, [empty])
    assert not got["count"].any() and not got["bits"].any() and not got["limbs"].any() and not got["L"].any()
    col, val = np.array([5], np.int64), np.array([-0.375], np.float32)
    assert_equals_reference(both_passes(device_solver, 7, [(up(device_solver, col), up(device_solver, val))]), fh.reference(col, val, 7))


# ---- 5: chunks --------------------------------------------------------------------------------------------------------------------------------
def test_seven_uneven_permuted_chunks_have_the_bits_of_one_call(device_solver):
    col, val, D, ref = case("zipf")
    perm, cuts = fh.seven_chunks(col.size)
    assert len(cuts) == 8 and any(a == b for a, b in zip(cuts, cuts[1:])) and any(a % 4 for a in cuts)
    cp, vp = up(device_solver, col[perm]), up(device_solver, val[perm])
    slices = [(cp[a:b], vp[a:b]) for a, b in zip(cuts, cuts[1:])]                    # device slices: unaligned starts
    order = [3, 0, 6, 2, 5, 1, 4]
    assert_equals_reference(both_passes(device_solver, D, [slices[i] for i in order]), ref, calls=7)
    fresh = [(up(device_solver, col[perm][a:b]), up(device_solver, val[perm][a:b])) for a, b in zip(cuts, cuts[1:])]      # aligned starts
    assert_equals_reference(both_passes(device_solver, D, fresh), ref, calls=7)


# ---- 6: the two paths ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["lds", "4000"])
def test_lds_threshold_forced_either_way(device_solver, monkeypatch, name):
    col, val, D, ref = case(name)
    c, v = up(device_solver, col), up(device_solver, val)
    for limit in ("0", "5000"):
        monkeypatch.setenv("GDMIX_STATS_LDS_MAX_FEATURES", limit)
        assert_equals_reference(both_passes(device_solver, D, [(c, v)]), ref)
        assert_equals_reference(both_passes(device_solver, D, [(c[1:], v[1:]), (c[:1], v[:1])]), ref, calls=2)     # the one-entry-per-lane kernels


# ---- 7: bad entries ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["lds", "zipf"])
def test_bad_entries_are_counted_named_and_left_out(device_solver, name):
    col, val, D, _ = case(name)
    at = [1234, 77, 40001, 99999]                 # NaN, +Inf, column -1, column D
    c2, v2 = col.copy(), val.copy()
    v2[at[0]], v2[at[1]], c2[at[2]], c2[at[3]] = np.nan, np.inf, -1, D
    keep = np.ones(col.size, bool)
    keep[at] = False
    ref = fh.reference(col[keep], val[keep], D)
    got = both_passes(device_solver, D, [(up(device_solver, c2), up(device_solver, v2))])
    assert got["bad1"] == [(4, 77)] and got["bad2"] == [(4, 77)]
    for k in ("count", "bits", "L", "s1", "s2", "limbs"):
        assert np.array_equal(got[k], ref[k]), k
    # the host raises once per pass, naming the entry
    acc = fs.DeviceAccumulator(device_solver, D)
    acc.add(up(device_solver, c2), up(device_solver, v2))
    with pytest.raises(fs.FeatureStatsError, match="pass 1: 4 bad entries in call 0, the first at index 77 of that call"):
        acc.shifts()
    # pass 2: a value above the maximum the shifts were made for, and a value on a feature that was dead in pass 1
    acc = fs.DeviceAccumulator(device_solver, D)
    c, v = up(device_solver, col[keep]), up(device_solver, val[keep])
    acc.add(c, v)
    acc.shifts()
    j = int(np.flatnonzero(ref["count"] > 0)[3])
    first = int(np.flatnonzero(col[keep] == j)[0])
    big = val[keep].copy()
    big[first] = np.float32(4) * ref["bits"][j:j + 1].view(np.float32)[0]
    acc.add(c, up(device_solver, big))
    assert acc.take_bad() == [(1, first)]
    want = fh.reference(np.delete(col[keep], first), np.delete(val[keep], first), D)
    if np.array_equal(want["L"], ref["L"]) and np.array_equal(want["s1"], ref["s1"]):      # (the entry left out was not the column's maximum)
        assert np.array_equal(acc.host_limbs(), want["limbs"])


# ---- 8: the expansion to coefficient order ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ic", [False, True])
def test_expansion_to_coefficient_order(device_solver, ic):
    b = synthetic.make_ragged_batch(700, seed=21, D=300, max_n=12, max_k=7)
    packed = device_solver.pack(b, has_intercept=ic)
    factor = np.exp(np.random.default_rng(9).uniform(-8, 8, 300))
    got = device_solver.feature_scale_expand(packed, up(device_solver, factor)).cpu().numpy()
    fp = packed.ent_feat_ptr().cpu().numpy()
    uniq = packed.unique_global().cpu().numpy()
    want = np.ones(packed.P)
    e_of = np.repeat(np.arange(b.E), np.diff(fp))
    want[np.arange(packed.D) + (e_of + 1 if ic else 0)] = factor[uniq]
    assert packed.E > 256 and got.shape == (packed.D + (b.E if ic else 0),)
    assert np.array_equal(got, want)
    if ic:
        assert np.all(got[fp[:-1] + np.arange(b.E)] == 1.0)


# ---- the solve in normalised units --------------------------------------------------------------------------------------------------------
def _normalised_solve(solver, b, kind):
    packed = solver.pack(b, has_intercept=True)
    acc = fs.DeviceAccumulator(solver, 1024)
    stats = fs.collect(acc, lambda a: a.add(up(solver, b.col_global), up(solver, b.val)), b.N, kind)
    s = fs.factors(kind, stats)
    scale = solver.feature_scale_expand(packed, up(solver, s))
    mean = solver.torch.zeros_like(scale)
    work = solver.prior_apply(packed, mean, scale)
    res = solver.solve(work, SolverOptions(l2=1.0, regularize_bias=True, has_intercept=True))
    back = solver.prior_restore(packed, mean, scale, res.theta)
    uniq = packed.unique_global().cpu().numpy()
    fp = packed.ent_feat_ptr().cpu().numpy()
    slot = np.arange(packed.D) + np.repeat(np.arange(b.E), np.diff(fp)) + 1
    return dict(phi=res.theta.cpu().numpy(), nit=res.nit.cpu().numpy(), nfev=res.nfev.cpu().numpy(), status=res.status.cpu().numpy(),
                theta=back["theta"].cpu().numpy(), uniq=uniq, slot=slot, s=s, stats=stats)


@pytest.mark.parametrize("kind", [fs.SCALE_WITH_STANDARD_DEVIATION, fs.SCALE_WITH_MAX_MAGNITUDE])
def test_a_column_multiplied_by_8_leaves_the_normalised_solve_unchanged(device_solver, kind):
    """statistics -> factors -> apply -> solve: bit-identical phi, nit and nfev for the data and for the data with one column times 8,
    and theta of that column exactly one eighth. Without normalisation the L2 optimum of that coefficient moves."""
    import dataclasses
    b = synthetic.make_batch(300, 16, 4, 1024, seed=16, with_uid=False)
    j = int(np.bincount(b.col_global, minlength=1024).argmax())
    v8 = b.val.copy()
    v8[b.col_global == j] *= np.float32(8)
    a = _normalised_solve(device_solver, b, kind)
    c = _normalised_solve(device_solver, dataclasses.replace(b, val=v8), kind)
    assert a["s"][j] == 8 * c["s"][j] and np.array_equal(np.delete(a["s"], j), np.delete(c["s"], j))
    assert np.array_equal(a["phi"].view(np.uint64), c["phi"].view(np.uint64))
    assert np.array_equal(a["nit"], c["nit"]) and np.array_equal(a["nfev"], c["nfev"]) and np.array_equal(a["status"], c["status"])
    at = a["slot"][a["uniq"] == j]
    assert at.size > 5 and np.any(a["theta"][at] != 0)
    assert np.array_equal(c["theta"][at] * 8, a["theta"][at])
    rest = np.ones(a["theta"].size, bool)
    rest[at] = False
    assert np.array_equal(a["theta"][rest].view(np.uint64), c["theta"][rest].view(np.uint64))
    # and without normalisation it does not hold: the penalty means something else for the scaled column
    plain = lambda batch: device_solver.solve(device_solver.pack(batch, has_intercept=True),
                                              SolverOptions(l2=1.0, regularize_bias=True, has_intercept=True)).theta.cpu().numpy()
    p1, p8 = plain(b), plain(dataclasses.replace(b, val=v8))
    assert not np.array_equal(p8[at] * 8, p1[at])
