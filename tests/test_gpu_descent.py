"""GPU: the resident coordinate descent (gdmix_amd/descent.py; include/gdmix_re.h, "row grouping"; csrc/re_group.hip).
The grouping and the three row-value kernels bit for bit against their numpy statements at the edges of the plan chunks and copy tiles;
pass 1 against the file chain's CPU restatement (tests/chain_oracle.py) at the bars of tests/test_gpu_chain.py; every later update against
the oracle solve of what it was given (tests/descent_oracle.py); the joint objective falling at every update for the three losses; two
fits giving the same bits; and the model files read back."""
import numpy as np
import pytest

from gdmix_amd import chain, descent
from gdmix_amd.io import avro

import chain_oracle
import descent_oracle
from test_descent_host import random_bag

pytestmark = pytest.mark.gpu


def _bag_with(rng, n, z, dim=11, empty_front=0, empty_back=0):
    """n rows holding exactly z non-zeros, the first / last rows empty when asked."""
    live = n - empty_front - empty_back
    k = np.zeros(n, np.int64)
    if live > 0:
        k[empty_front:empty_front + live] = rng.multinomial(z, np.ones(live) / live) if z else 0
    ptr = np.concatenate([[0], np.cumsum(k)]).astype(np.int64)
    col = rng.integers(0, dim, int(ptr[-1])).astype(np.int64)
    val = rng.standard_normal(int(ptr[-1])).astype(np.float32)
    return ptr, col, val


def _cases():
    rng = np.random.default_rng(20241021)
    out = {}
    for n in (1, 63, 64, 65):
        out[f"n{n}_mixed"] = (*random_bag(rng, n, 9), rng.integers(-1, 5, n), 5)
    for n in (2047, 2048, 2049):                     # the chunk of the plan kernels (re_rowsubset.hpp: DS_CHUNK = 2048 rows)
        out[f"n{n}_mixed"] = (*random_bag(rng, n, 9), rng.integers(-1, 40, n), 40)
    for z in (1023, 1024, 1025, 4097):               # the tile of the copy (DS_TILE = 1024 output non-zeros), and four tiles and one
        out[f"z{z}_no_minus_one"] = (*_bag_with(rng, 300, z), rng.integers(0, 17, 300), 17)
    out["one_entity"] = (*random_bag(rng, 200, 9), np.zeros(200, np.int64), 1)
    out["every_row_its_own_entity"] = (*random_bag(rng, 130, 9), rng.permutation(130), 130)
    idx = rng.integers(1, 6, 500)
    idx[0] = idx[-1] = 0                             # entity 0 owns the first and the last row and nothing else
    out["first_and_last_row"] = (*random_bag(rng, 500, 9), idx, 6)
    out["empty_rows_front_and_end"] = (*_bag_with(rng, 400, 1500, empty_front=7, empty_back=5), rng.integers(-1, 9, 400), 9)
    out["all_minus_one"] = (*random_bag(rng, 100, 9), np.full(100, -1), 4)
    idx = rng.integers(0, 30, 700) * 3               # entities 1, 2, 4, 5, ... own nothing: E' < E
    out["indices_skip_entities"] = (*random_bag(rng, 700, 9), idx, 90)
    out["no_nonzero_at_all"] = (*_bag_with(rng, 50, 0), rng.integers(-1, 3, 50), 3)
    return out


CASES = _cases()
GROUP_ARRAYS = ("row_of", "present", "ent_row_ptr", "row_nnz_ptr", "col_global", "val")


def _group(solver, ptr, col, val, idx, E):
    t = solver.torch
    up = lambda a, dt: t.from_numpy(np.ascontiguousarray(a, dt)).to(solver.device)
    g, counts = solver.group_rows(up(ptr, np.int64), up(col, np.int64), up(val, np.float32), up(idx, np.int32), E)
    t.cuda.synchronize()
    assert (g["N"], g["Z"], g["E"]) == (counts["grouped"], counts["grouped_nnz"], counts["entities"])
    return {k: g[k].cpu().numpy() for k in GROUP_ARRAYS}, counts


@pytest.mark.parametrize("name", sorted(CASES))
def test_grouping_is_the_numpy_statement_bit_for_bit(device_solver, name):
    ptr, col, val, idx, E = CASES[name]
    want = descent.group_rows_host(ptr, col, val, idx, E)
    got, counts = _group(device_solver, ptr, col, val, idx, E)
    again, counts2 = _group(device_solver, ptr, col, val, idx, E)
    assert counts == want["counts"] == counts2
    for k in GROUP_ARRAYS:
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, (name, k)
        assert np.array_equal(got[k].view(np.uint32) if k == "val" else got[k], want[k].view(np.uint32) if k == "val" else want[k]), (name, k)
        assert np.array_equal(got[k].view(np.uint32) if k == "val" else got[k], again[k].view(np.uint32) if k == "val" else again[k]), (name, k, "second run")
    if name == "all_minus_one":
        assert counts["grouped"] == 0 and counts["left_out"] == 100 and np.array_equal(got["ent_row_ptr"], [0]) and np.array_equal(got["row_nnz_ptr"], [0])
    if name == "indices_skip_entities":
        assert counts["entities"] < E and (np.diff(got["ent_row_ptr"]) > 0).all()      # no empty entity reaches the pack
    if name == "first_and_last_row":
        assert np.array_equal(got["row_of"][:2], [0, 499]) and got["ent_row_ptr"][1] == 2


def test_bad_row_pointers_are_refused_and_nothing_is_copied(device_solver):
    from gdmix_amd.solver import GdmixReError
    ptr, col, val, idx, E = CASES["n65_mixed"]
    bad = ptr.copy()
    bad[10] = ptr[-1] + 1000
    with pytest.raises(GdmixReError, match="the row pointers do not describe"):
        _group(device_solver, bad, col, val, np.zeros_like(idx), E)


def _f32_same(a, b):
    return a.dtype == np.float32 and b.dtype == np.float32 and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def test_the_row_value_kernels_are_numpy_fp32_bit_for_bit(device_solver):
    s, t = device_solver, device_solver.torch
    rng = np.random.default_rng(7)
    n_src, n_map = 2500, 1777                      # several workgroups, the last one partial
    up = lambda a: t.from_numpy(np.ascontiguousarray(a)).to(s.device)
    row_of = rng.permutation(n_src)[:n_map].astype(np.int32)
    src = rng.standard_normal(n_src).astype(np.float32)
    assert _f32_same(s.rows_gather(up(src), up(row_of)).cpu().numpy(), descent.rows_gather_host(src, row_of))
    assert _f32_same(s.rows_scatter(up(src[:n_map]), up(row_of), n_src).cpu().numpy(), descent.rows_scatter_host(src[:n_map], row_of, n_src))
    stale = t.full((n_src,), 9.0, dtype=t.float32, device=s.device)      # rows that are left out read 0, whatever the buffer held
    assert _f32_same(s.rows_scatter(up(src[:n_map]), up(row_of), n_src, out=stale).cpu().numpy(), descent.rows_scatter_host(src[:n_map], row_of, n_src))
    kept = s.rows_scatter(up(src[:n_map]), up(row_of), n_src, out=t.full((n_src,), 9.0, dtype=t.float32, device=s.device), keep_rest=True).cpu().numpy()
    want = np.full(n_src, 9.0, np.float32)                               # ... or, with keep_rest, what it held
    want[row_of] = src[:n_map]
    assert _f32_same(kept, want)
    parts = [(rng.standard_normal(n_src) * 10.0 ** rng.integers(-3, 4)).astype(np.float32) for _ in range(8)]
    base = rng.standard_normal(n_src).astype(np.float32)
    parts_dev, base_dev, map_dev = [up(p) for p in parts], up(base), up(row_of)
    checked = 0
    for K in (1, 3, 8):
        for skip in sorted({0, K // 2, K - 1, -1}):      # first / middle / last / none
            for with_base in (False, True):
                for with_map in (False, True):
                    got = s.offsets_combine(n_src, base_dev if with_base else None, parts_dev[:K], skip=skip, row_of=map_dev if with_map else None)
                    want = descent.offsets_combine_host(n_src, base if with_base else None, parts[:K], skip, row_of if with_map else None)
                    assert _f32_same(got.cpu().numpy(), want), (K, skip, with_base, with_map)
                    checked += 1
    assert checked == (2 + 4 + 4) * 4      # (K = 1: its one part left out, or none)
    from gdmix_amd.solver import GdmixReError
    with pytest.raises(GdmixReError, match="at most 8 parts"):
        s.offsets_combine(n_src, None, parts_dev + parts_dev[:1])


# ---- the descent ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def data():
    return chain.make_dataset(120, 200, 8000)


def _ulps(a, b):
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    return np.abs(a.astype(np.float64) - b.astype(np.float64)) / np.spacing(np.maximum(np.abs(a), np.abs(b)).astype(np.float32)).astype(np.float64)


def _dense_models(m):
    """CoordinateModel of a random effect -> (intercept [E], coefficients [E, dim]) of the thresholded model."""
    E = m.present.size
    icpt = m.theta_thr[m.coef_ptr[:-1]]
    coef = np.zeros((E, m.dim))
    ent = np.repeat(np.arange(E), np.diff(m.feat_ptr))
    coef[ent, m.unique_global] = np.delete(m.theta_thr, m.coef_ptr[:-1])
    return icpt, coef


def test_pass_one_is_the_chain(device_solver, data):
    """fit(passes=1) with the chain's settings (regularize_bias=False, l2 = 1, threshold 1e-4) held to tests/chain_oracle.py at the bars of
    tests/test_gpu_chain.py: the global coefficients to 1e-5 of their scale; each random effect, with the oracle fed the product's own
    offsets, to 1e-5 of the scale with the same thresholded pattern on well-posed entities (at most 5 % of a coordinate's entities may be
    set aside as ill-posed: all labels equal), and its accumulated and per-coordinate scores to 1 ulp of float32."""
    res = chain.run_resident(data, passes=1, solver=device_solver, record=True)
    tr, va = np.flatnonzero(data["train"]), np.flatnonzero(~data["train"])
    hist = {e["coordinate"]: e for e in res.history}
    assert [e["coordinate"] for e in res.history] == list(chain.STAGES) and all(e["pass"] == 0 and e["theta0"] is None for e in res.history)
    g = chain_oracle.global_stage(data)
    theta = res.models["global"].theta_thr
    assert np.abs(theta - g["theta"]).max() / np.abs(g["theta"]).max() <= 1e-5
    for w, key in (("train", "score"), ("validation", "validation_score")):
        want = g[w]["score"]
        assert np.abs(hist["global"][key].astype(np.float64) - want).max() <= 2e-5 * max(1.0, float(np.abs(want).max()))
    prev = hist["global"]
    for stage in ("per_user", "per_movie"):
        e, m = hist[stage], res.models[stage]
        # the oracle is fed the product's own offsets: what the update trained on, back in sample order. They are the fp32 sum of the
        # contributions so far — for the first random effect the previous accumulated score bit for bit, for the second within an ulp of it
        # (the previous stage's score is float32(x . theta + offset) with the sum in fp64, the sum of contributions rounds x . theta first)
        offsets = descent.rows_scatter_host(e["offsets"], res.row_of[stage], tr.size)
        assert np.array_equal(np.sort(res.row_of[stage]), np.arange(tr.size))
        if stage == "per_user":
            assert _f32_same(offsets, prev["score"]) and _f32_same(e["validation_offsets"], prev["validation_score"])
        fed = {"train": {"uid": data["uid"][tr], "score": offsets}, "validation": {"uid": data["uid"][va], "score": e["validation_offsets"]}}
        ora = chain_oracle.random_effect_stage(data, stage, fed)
        assert np.array_equal(m.present, ora["entities"])
        assert (~ora["well_posed"]).mean() <= 0.05, (stage, int((~ora["well_posed"]).sum()))
        icpt, coef = _dense_models(m)
        have = np.concatenate([icpt[:, None], coef], axis=1)
        want = np.concatenate([ora["intercept"][:, None], ora["coef"]], axis=1)
        ok = ora["well_posed"]
        assert np.array_equal(have[ok] == 0.0, want[ok] == 0.0), stage
        worst = (np.abs(have[ok] - want[ok]).max(axis=1) / np.maximum(1.0, np.abs(want[ok]).max(axis=1))).max()
        assert worst <= 1e-5, (stage, float(worst))
        for w, skey, ckey in (("train", "score", "contribution"), ("validation", "validation_score", None)):
            strict = ora[w]["strict"]
            assert strict.mean() > 0.9
            u = _ulps(e[skey][strict], ora[w]["score"][strict])
            assert u.max() <= 1.0, (stage, w, float(u.max()))
            if ckey:
                assert _ulps(e[ckey][strict], ora[w]["per_coord"][strict]).max() <= 1.0, (stage, w)
            if (~strict).any():
                sig = lambda x: 1.0 / (1.0 + np.exp(-x.astype(np.float64)))
                assert np.abs(sig(e[skey][~strict]) - sig(ora[w]["score"][~strict])).max() <= 1e-4
        prev = e
    aucs = [e["validation_auc"] for e in res.history]
    assert aucs[0] < aucs[1] < aucs[2]
    assert np.isclose(aucs[2], chain.auc(data["response"][va], res.history[-1]["validation_score"]), rtol=0, atol=1e-12)


def _objectives(res, coordinates, loss, label):
    """The joint objective after every update, in fp64 on the host from the recorded contributions and thresholded models; entry 0: the
    zero model."""
    parts = {c.name: np.zeros(label.size, np.float32) for c in coordinates}
    models = {}
    F = [descent.joint_objective(loss, label, None, np.zeros(label.size), [])]
    for e in res.history:
        c = next(c for c in coordinates if c.name == e["coordinate"])
        parts[c.name] = e["contribution"]
        mask = np.ones(e["theta_thr"].size, bool)
        if not c.regularize_bias:
            mask[-1 if not c.random_effect else res.models[c.name].coef_ptr[:-1]] = False
        models[c.name] = (e["theta_thr"], mask, c.l2)
        score = np.sum([p.astype(np.float64) for p in parts.values()], axis=0)
        F.append(descent.joint_objective(loss, label, None, score, list(models.values())))
    return np.array(F)


@pytest.fixture(scope="module")
def three_passes(device_solver, data):
    return chain.run_resident(data, passes=3, solver=device_solver, record=True, re_regularize_bias=True)


def test_every_later_update_is_what_a_stage_would_compute_from_what_it_was_given(three_passes, data):
    """passes=3 with the random effects' intercepts regularised (every block has a finite optimum: no entity is set aside). For each of
    the 9 updates the oracle's solve on the recorded offsets, from the recorded start point, agrees with the device to 1e-5 of the scale
    (the project's bars: a fixed effect against its largest coefficient, a random effect against max(1, largest)). The comparison is per
    update: a free-running one drifts with the fixed effect's rounding-level FACTR stop (tests/test_gpu_chain.py)."""
    res = three_passes
    tr = np.flatnonzero(data["train"])
    label = data["response"][tr].astype(np.float32)
    coordinates = chain.resident_coordinates(data, re_regularize_bias=True)
    blocks = {c.name: descent_oracle.Block(c, label) for c in coordinates}
    assert len(res.history) == 9
    for e in res.history:
        b = blocks[e["coordinate"]]
        assert (e["theta0"] is None) == (e["pass"] == 0)
        theta, _, _ = b.solve(e["offsets"], b.from_device_layout(e["theta0"]))
        want = b.to_device_layout(theta)
        scale = max(1.0, float(np.abs(want).max())) if b.c.random_effect else float(np.abs(want).max())
        assert np.abs(e["theta"] - want).max() / scale <= 1e-5, (e["pass"], e["coordinate"], float(np.abs(e["theta"] - want).max() / scale))
    # a later pass starts where the coordinate's previous update ended
    for k in range(3, 9):
        assert np.array_equal(res.history[k]["theta0"], res.history[k - 3]["theta"])


def test_the_joint_objective_falls_at_every_update(three_passes, data):
    tr = np.flatnonzero(data["train"])
    F = _objectives(three_passes, chain.resident_coordinates(data, re_regularize_bias=True), "logistic", data["response"][tr].astype(np.float32))
    assert F.size == 10 and (np.diff(F) < 0).all(), F
    e = three_passes.history
    assert e[-1]["train_auc"] > e[2]["train_auc"] > e[0]["train_auc"]


@pytest.mark.parametrize("model_type,loss", [(chain.LINEAR, "squared"), (chain.POISSON, "poisson")])
def test_linear_and_poisson_descend_and_repeat(device_solver, data, model_type, loss):
    runs = [chain.run_resident(data, passes=2, model_type=model_type, solver=device_solver, record=True, re_regularize_bias=True) for _ in range(2)]
    tr = np.flatnonzero(data["train"])
    label = chain.labels_of(data, model_type)[tr].astype(np.float32)
    F = _objectives(runs[0], chain.resident_coordinates(data, re_regularize_bias=True), loss, label)
    assert F.size == 7 and (np.diff(F) < 0).all(), F
    metric = {"squared": "mse", "poisson": "poisson_loss"}[loss]
    assert runs[0].metric == metric and runs[0].history[-1][f"train_{metric}"] < runs[0].history[0][f"train_{metric}"]
    for a, b in zip(runs[0].history, runs[1].history):
        for k in ("theta", "theta_thr", "offsets", "contribution", "score", "validation_score"):
            assert np.array_equal(a[k].view(np.uint8), b[k].view(np.uint8)), (a["pass"], a["coordinate"], k)
        assert a[f"validation_{metric}"] == b[f"validation_{metric}"]


def test_write_models_files_are_the_thresholded_models(three_passes, tmp_path):
    res = three_passes
    paths = descent.write_models(res, str(tmp_path))
    assert sorted(paths) == sorted(chain.STAGES)
    rec = list(avro.read_file(paths["global"]))
    m = res.models["global"]
    assert len(rec) == 1 and rec[0]["modelId"] == "global model"
    theta = np.zeros(m.dim + 1)
    for ntv in rec[0]["means"]:
        theta[m.dim if ntv["name"] == "(INTERCEPT)" else int(ntv["name"][1:])] = ntv["value"]
    assert np.array_equal(theta, m.theta_thr)
    for stage in ("per_user", "per_movie"):
        m = res.models[stage]
        icpt, coef = _dense_models(m)
        recs = list(avro.read_file(paths[stage]))
        assert [r["modelId"] for r in recs] == [str(e) for e in m.present]
        for i, r in enumerate(recs):
            assert r["means"][0]["name"] == "(INTERCEPT)" and r["means"][0]["value"] == icpt[i]
            got = np.zeros(m.dim)
            for ntv in r["means"][1:]:
                got[int(ntv["name"][1:])] = ntv["value"]
            assert np.array_equal(got, coef[i]), (stage, i)
