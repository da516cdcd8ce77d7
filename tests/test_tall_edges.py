"""CPU checks of what tests/test_gpu_tall_edges.py stands on, so that it cannot pass by missing the edges it is about: the restated
constants of csrc/re_solve_tall.hip give the five arena figures, the generators give the stated shapes, pass_plan / slice_plan /
route_tall show every situation of the issue's six points on a NAMED entity (trip borders, arenas, accumulator sets, the tail,
structures, teams whose members differ), the REFERENCE's own run of every case is reproducible (strict) on every entity, and the dense
statement of the SIMPLE variance agrees with the existing helpers where no cell repeats. When a constant of the library moves
(test_the_constants_are_the_librarys) and the helper follows, the assertion that fails here names the situation that is gone."""
import numpy as np
import pytest

import class_caps_helpers as ch
import re_linear_helpers as lh
import re_poisson_helpers as ph
import tall_edges_helpers as th

WI = [(w, ic) for w in (True, False) for ic in (1, 0)]


def _plans(batch, has_w, ic):
    """{name: (entity, class by route_tall, pass_plan on the variant of that class — a team: the four slice plans)}."""
    c = th.case(batch, "logistic", has_w, ic)
    by_class = {k[3]: v for v, k in th.VARIANTS.items()}
    out = {}
    for e, k in zip(c["entities"], th.routed(c)):
        pl = c["placed"][e["name"]]
        if k == th.NOT_TALL:
            out[e["name"]] = (e, k, None)
        elif k == th.TALL_TEAM_CLASS:
            out[e["name"]] = (e, k, th.slice_plan(pl, has_w, ic))
        else:
            out[e["name"]] = (e, k, th.pass_plan(pl, by_class[k], has_w, ic))
    return out


def test_constant_arithmetic():
    assert [th.tall_lds_sizeof(nw) for nw in (1, 4, 8)] == [816 + 528 * nw for nw in (1, 4, 8)] == [1344, 2928, 5040]
    assert {v: th.arena(v) for v in th.VARIANTS} == th.ARENA_FIGURES == dict(one=18624, lean=11792, mid=78480, large=158288, team=158288)
    assert th.TALL_LEAN_ARENA == ch.TALL_LEAN_ARENA == 11728 and th.arena("lean") >= th.TALL_LEAN_ARENA, "the lean kernel stages whatever is routed to it"
    assert [th.tall_sets(nw, p) for nw, p in ((1, 1), (1, 32), (4, 32), (4, 33), (8, 32), (8, 33), (8, 64))] == [16, 16, 32, 16, 32, 16, 16]
    assert th.tall_sets(8, 32) % th.TALL_REDUCE == 0 and th.tall_sets(1, 1) % th.TALL_REDUCE == 0, "tall_pass reads the sets sixteen at a time"
    # the issue's own shapes at 24 features
    for n, z, w, want in ((400, 1092, True, 18624), (400, 1292, False, 18624), (200, 630, True, 11728), (200, 730, False, 11728)):
        assert th.tall_resident_bytes(1, 16, 24, n, z, w) == want
    assert th.tall_resident_bytes(8, 32, 24, 0, 0, True) == 52800 + 64 + 8 + 16
    assert th.team_slices(10401) == (2601, [(0, 2601), (2601, 5202), (5202, 7803), (7803, 10401)]) and th.team_slices(2)[1] == [(0, 1), (1, 2), (2, 2), (2, 2)]
    # route_tall on hand-made shapes: (p, n, nnz, has_w, routing) -> class
    T, L, O, M, G = th.TALL_TEAM_CLASS, th.TALL_LEAN_CLASS, th.TALL_ONE_CLASS, th.TALL_MID_CLASS, th.TALL_LARGE_CLASS
    assert (T, L, O, M, G) == (30, 31, 32, 33, 34) == (ch.TALL_CLASSES[0], ch.TALL_LEAN_CLASS, ch.TALL_ONE_CLASS, 33, ch.TALL_CLASSES[-1])
    for args, want in (((25, 200, 630, True, "one"), L), ((25, 200, 631, True, "one"), O), ((25, 200, 631, True, "mid"), M), ((25, 200, 630, True, "mid"), L),
                       ((25, 4095, 9000, True, "one"), O), ((25, 4096, 9000, True, "one"), G), ((25, 1, 1, True, "large"), G), ((25, 64, 64, True, "team"), T),
                       ((25, 63, 63, True, "team"), G), ((65, 400, 900, True, "large"), th.NOT_TALL), ((64, 400, 900, True, "large"), G),
                       ((25, 299, 2000, True, "ladder"), M), ((25, 300, 2000, True, "ladder"), G), ((25, 599, 2000, True, "ladder"), G), ((25, 600, 2000, True, "ladder"), T)):
        p, n, z, w, r = args
        assert th.route_tall(p, n, z, 10, w, th.ROUTING[r]) == want, (args, want)
        if want in (L, O) and n < 512:
            assert ch.route(p, n, z, 10, w, 1) == want      # (the rule of class_caps_helpers below the split)
    assert th.route_tall(25, 400, 900, 11, True, th.ROUTING["large"]) == th.NOT_TALL


def test_generators_give_the_stated_shapes():
    from oracle import oracle
    for batch in th.BATCHES:
        for has_w, ic in ((True, 1), (False, 0)):
            c = th.case(batch, "logistic", has_w, ic)
            b = c["b"]
            b.validate()
            pk = oracle.pack(b.ent_row_ptr, b.row_nnz_ptr, b.col_global)
            assert (b.weight is not None) == has_w and b.entity_ids == c["names"] and len(set(c["names"])) == b.E
            assert np.array_equal(np.diff(pk["ent_feat_ptr"]), [e["d"] for e in c["entities"]]), batch
            assert np.array_equal(b.ent_n(), [e["lens"].size for e in c["entities"]]) and np.array_equal(b.ent_nnz(), [e["lens"].sum() for e in c["entities"]])
            for e in c["entities"]:
                if e["lens"].sum() >= e["F"]:
                    assert e["d"] == e["F"], e["name"]      # every feature of its space occurs
                assert th.has_duplicates(e) == (e["rule"] in ("dup", "same")), e["name"]      # (else a sample's columns are distinct)
    # an entity is the same arrays wherever it stands
    x = [th.case(f"positions:one,{p}", "logistic", True, 1) for p in th.POSITIONS]
    assert [c["names"].index("pos-one") for c in x] == [0, 1, 2]
    e = [c["entities"][c["names"].index("pos-one")] for c in x]
    assert e[0] is e[1] is e[2] and e[0]["lens"][-1] == 1


@pytest.mark.parametrize("has_w,ic", WI)
def test_every_entity_routes_where_its_name_says(has_w, ic):
    for batch in th.BATCHES:
        for name, (e, k, _) in _plans(batch, has_w, ic).items():
            want = th.NOT_TALL if e["want"] is None else th.VARIANTS[e["want"]][3]
            assert k == want, (batch, name, k, want, int(e["lens"].size), int(e["lens"].sum()), e["d"])


@pytest.mark.parametrize("has_w,ic", WI)
def test_trips_cover_every_border_of_every_pass(has_w, ic):
    trips_of = dict(zip(th.TRIP_SITUATIONS, (1, 1, 2, 2, 2, 3, 4)))
    largest = 0
    for v in th.SOLO:
        nw, pf, _, cls = th.VARIANTS[v]
        plans = _plans(f"trips:{v}", has_w, ic)
        for width in th.WIDTHS_OF_TRIPS:
            R = (2 if pf else 1) if width == 4 else 1
            for sit, n in th.trip_counts(v, width).items():
                what = f"{th.TALL_NAMES[cls - 30]}, width class {width}, n = {sit} (T = {R} x {64 * nw})"
                assert f"trips-{v}-w{width}-{sit}" in plans, what
                e, k, pl = plans[f"trips-{v}-w{width}-{sit}"]
                assert k == cls and e["lens"].size == n and (pl["NT"], pl["R"], pl["width"], pl["trips"]) == (64 * nw, R, width, trips_of[sit]), (what, pl)
                if width == 8:
                    assert 5 <= e["lens"].max() <= 8, what
                if width == 0:
                    assert (e["lens"] == 9).sum() == 1 and np.sort(e["lens"])[-2] <= 8, what
                largest = max(largest, n)
        T4 = th.trip_counts(v, 4)["T"]
        assert T4 == (2 if pf else 1) * 64 * nw, f"{v}: R x NT of the 4-wide pass"
        if v in ("lean", "large"):
            for n in (1, 2):
                e, k, pl = plans[f"trips-{v}-n{n}"]
                assert k == cls and e["lens"].size == n and pl["trips"] == 1, f"{v}: an entity of {n} sample(s)"
    assert largest == 3073, "the largest trips entity: 3 R NT + 1 on <8> at width 4"
    # both homes occur among the trips of <1>, <4> and <8>; every lean one is resident
    for v in ("one", "mid", "large"):
        homes = {pl["resident"] for _, _, pl in _plans(f"trips:{v}", has_w, ic).values()}
        assert homes == {True, False}, (v, homes)
    assert all(pl["resident"] for _, _, pl in _plans("trips:lean", has_w, ic).values())


@pytest.mark.parametrize("has_w,ic", WI)
def test_arenas_have_an_entity_on_them_and_one_above(has_w, ic):
    w = "w" if has_w else "u"
    one = _plans("arena:one", has_w, ic)
    for tag, target in (("leanroute", th.TALL_LEAN_ARENA), ("leanarena", th.arena("lean")), ("one", th.arena("one"))):
        e, k, pl = one[f"arena-{tag}-{w}{ic}-exact"]
        assert th.tall_resident_bytes(1, 16, e["d"], e["lens"].size, e["lens"].sum(), has_w) == target and pl["resident"], f"an entity of exactly {target} B ({tag})"
        for kind in ("entry", "sample"):
            e2, k2, pl2 = one[f"arena-{tag}-{w}{ic}-{kind}"]
            assert target < th.tall_resident_bytes(1, 16, e2["d"], e2["lens"].size, e2["lens"].sum(), has_w) <= target + 16, f"the next entity above {target} B ({tag}, {kind})"
        assert e2["lens"].size == e["lens"].size + 1 and e2["lens"].sum() == e["lens"].sum()
    assert one[f"arena-leanroute-{w}{ic}-exact"][1] == th.TALL_LEAN_CLASS and one[f"arena-leanroute-{w}{ic}-entry"][1] == th.TALL_ONE_CLASS, "the lean routing threshold, both sides"
    assert one[f"arena-one-{w}{ic}-exact"][2]["resident"] and not one[f"arena-one-{w}{ic}-entry"][2]["resident"] and not one[f"arena-one-{w}{ic}-sample"][2]["resident"]
    last = th.ARENA_LAST.format(w=w, ic=ic)
    assert list(one)[-1] == last and one[last][2]["tail"] and not one[last][2]["resident"], "the entity just above the <1> arena ends the batch and reads the tail"
    if has_w and ic:
        e = one["arena-one-w1-exact"][0]
        assert (e["lens"].size, int(e["lens"].sum())) == (400, 1092) and (one["arena-leanroute-w1-exact"][0]["lens"].size, int(one["arena-leanroute-w1-exact"][0]["lens"].sum())) == (200, 630)
    for v in ("mid", "large"):
        plans = _plans(f"arena:{v}", has_w, ic)
        for S, tag in ((32, "S32"), (16, "S16")):
            e, k, pl = plans[f"arena-{v}-{tag}-{w}{ic}-exact"]
            assert pl["S"] == S and pl["bytes"] == th.arena(v) and pl["resident"], f"{v}: an entity of exactly the arena at S = {S}"
            assert e["d"] + ic == (33 if S == 16 else 24 + ic)
            for kind in ("entry", "sample"):
                pl2 = plans[f"arena-{v}-{tag}-{w}{ic}-{kind}"][2]
                assert pl2["S"] == S and th.arena(v) < pl2["bytes"] <= th.arena(v) + 16 and not pl2["resident"], f"{v}: the next entity above the arena at S = {S} ({kind})"
    team = _plans("arena:team", has_w, ic)
    for S, tag in ((32, "team-S32"), (16, "team-S16")):
        assert [(pl["bytes"], pl["resident"], pl["S"]) for pl in team[f"arena-{tag}-{w}{ic}-exact"][2]] == [(th.arena("team"), True, S)] * 4, f"a team whose four slices have exactly the arena, S = {S}"
        assert [pl["resident"] for pl in team[f"arena-{tag}-{w}{ic}-entry0"][2]] == [False, True, True, True]
        assert [pl["resident"] for pl in team[f"arena-{tag}-{w}{ic}-entry3"][2]] == [True, True, True, False]
        assert [pl["bytes"] for pl in team[f"arena-{tag}-{w}{ic}-entry3"][2]][3] == th.arena("team") + 8


@pytest.mark.parametrize("has_w,ic", WI)
def test_widths_sets_and_the_tail(has_w, ic):
    plans = _plans("widths", has_w, ic)
    for v in ("mid", "large", "team"):
        seen = {}
        for p in (32, 33, 64):
            e, k, pl = plans[f"widths-{v}-p{p}-ic{ic}"]
            assert e["d"] + ic == p and k == th.VARIANTS[v][3], f"p = {p} on {v}"
            seen[p] = {q["S"] for q in pl} if v == "team" else {pl["S"]}
        assert seen == {32: {32}, 33: {16}, 64: {16}}, f"{v}: S = 32 at p = 32, 16 at p = 33 and 64"
    assert plans[f"widths-large-p64-ic{ic}"][0]["d"] == 64 - ic, "p = 64 as d = 64 without an intercept and d = 63 with one"
    assert plans[f"widths-p65-ic{ic}"][1] == th.NOT_TALL and plans[f"widths-p65-ic{ic}"][0]["d"] + ic == 65, "p = 65 leaves the tall classes"
    for v in ("lean", "large", "team"):
        e = plans[f"widths-{v}-lastcol"][0]
        assert e["d"] == th.F and np.all(e["col"][th.F:] == th.F - 1) and e["lens"].size > th.F, "an entity that uses only column d - 1"
        if ic:
            e, k, _ = plans[f"widths-{v}-d0"]
            assert e["d"] == 0 and e["lens"].sum() == 0 and k == th.VARIANTS[v][3], "d = 0 with an intercept (p = 1)"
    # the tail path: a streamed workgroup whose last windows start within W entries of the batch's end
    tails = {"one": [], "large": [], "team": []}
    for batch in th.BATCHES:
        for name, (e, k, pl) in _plans(batch, has_w, ic).items():
            if k == th.TALL_ONE_CLASS and pl["tail"]:
                tails["one"].append(name)
            if k == th.TALL_LARGE_CLASS and pl["tail"]:
                tails["large"].append(name)
            if k == th.TALL_TEAM_CLASS and any(q["tail"] for q in pl):
                tails["team"].append(name)
            if pl is not None and k != th.TALL_TEAM_CLASS and pl["tail"]:
                assert name == list(_plans(batch, has_w, ic))[-1], "only the batch's last entity reads the tail"
    assert tails["one"] and tails["large"] and tails["team"], tails
    assert "pos-one" in tails["one"] and "pos-large" in tails["large"] and "team-ssss" in tails["team"], tails
    for which in ("one", "large"):
        t = [_plans(f"positions:{which},{p}", has_w, ic)[f"pos-{which}"][2] for p in th.POSITIONS]
        assert [pl["tail"] for pl in t] == [False, False, True] and not any(pl["resident"] for pl in t), f"positions: {which} is streamed, and reads the tail in the last place only"


@pytest.mark.parametrize("has_w,ic", WI)
def test_structures_in_both_homes_and_mixed_teams(has_w, ic):
    for v in ("one", "large"):
        plans = _plans(f"structures:{v}", has_w, ic)
        for home in ("resident", "streamed"):
            for kind, width in zip(th.STRUCTURES, (8, 4, 4, 8, 0, 0)):
                e, k, pl = plans[f"struct-{v}-{home}-{kind}"]
                assert k == th.VARIANTS[v][3] and pl["resident"] == (home == "resident") and pl["width"] == width, f"{kind}, {home}, on {v}"
            lens = plans[f"struct-{v}-{home}-empties"][0]["lens"]
            assert lens[0] == 0 and lens[-1] == 0 and np.all(lens[0::2] == 0) and np.all(lens[1:-1:2] > 0), "samples without entries: first, last and every other"
            assert np.all(plans[f"struct-{v}-{home}-tail3"][0]["lens"][-3:] == 0) and plans[f"struct-{v}-{home}-tail3"][0]["lens"][-4] == 3, "the last three samples empty, three entries in the one before"
            for kind in ("dup-w4", "dup-w8", "dup-w0"):
                e = plans[f"struct-{v}-{home}-{kind}"][0]
                starts = np.concatenate([[0], np.cumsum(e["lens"])])
                twice = [i for i in range(e["lens"].size) if e["lens"][i] >= 2 and e["col"][starts[i]] == e["col"][starts[i + 1] - 1]]
                assert len(twice) >= 10 and (kind != "dup-w0" or any(e["lens"][i] == 9 for i in twice)), f"{kind}: a column at a sample's first and last entry"
            e = plans[f"struct-{v}-{home}-same9"][0]
            starts = np.concatenate([[0], np.cumsum(e["lens"])])
            nine = np.flatnonzero(e["lens"] == 9)
            assert nine.size == 2 and all(np.unique(e["col"][starts[i]:starts[i + 1]]).size == 1 for i in nine), "a sample of nine entries that is one column nine times"
        last = list(plans)[-1]
        assert last == f"struct-{v}-streamed-tail3" and plans[last][2]["tail"], "the streamed entity whose last three samples are empty ends the batch and reads the zero half of the tail"
    team = _plans("team_mixed", has_w, ic)
    seen = set()
    for key, (n, homes) in th.TEAM_MIXED.items():
        e, k, pls = team[f"team-{key}"]
        assert k == th.TALL_TEAM_CLASS and e["lens"].size == n
        assert "".join("r" if pl["resident"] else "s" for pl in pls) == homes, f"a team with members {homes}"
        assert all(pl["trips"] > 1 and pl["R"] * pl["NT"] == 1024 for pl in pls), "every slice takes more than one trip of 1 024"
        seen.add(n % 4)
    assert seen == {0, 1, 2, 3}, "n mod 4"
    assert {"rrrs", "sssr", "ssss"} <= {h for _, h in th.TEAM_MIXED.values()}
    assert team["team-n64"][1] == th.TALL_TEAM_CLASS and team["team-n63"][1] == th.TALL_LARGE_CLASS, "tall_team_n = -1 is clamped to 64"
    assert list(team)[-1] == "team-ssss" and team["team-ssss"][2][3]["tail"]


@pytest.mark.parametrize("batch", th.BATCHES)
def test_the_reference_is_strict_on_every_entity(batch):
    """Every entity is reproduced by the reference from starts moved by 1e-15, 1e-14 and 1e-13 and is no FACTR stop, for the three
    losses with and without an intercept (`trips`: also without weights): the GPU tests compare all of them iteration for iteration."""
    combos = th.cases_of(batch) + [(loss, True, 0) for loss in th.LOSSES if not batch.startswith("trips") and loss != "logistic"]
    for loss, has_w, ic in combos:
        c = th.case(batch, loss, has_w, ic)
        r = th.reference(c)
        print(f"{c['name']}: nit {int(r['nit'].min())} .. {int(r['nit'].max())}")
        assert r["strict"].all(), (loss, has_w, ic, [n for n, s in zip(c["names"], r["strict"]) if not s])
        assert r["nit"].max() < c["kw"]["max_iter"], r["nit"]


def test_the_dense_variance_is_the_helpers_where_no_cell_repeats():
    """variance_dense against re_linear_helpers.variance_numpy (squared) and re_poisson_helpers.variance_numpy (Poisson) at an arbitrary
    theta; and on the entities of `structures` with a repeated cell, the sum it takes — (v1 + v2)^2 per cell — is not the entry-wise
    sum of squares, so a pass that squared the entries one by one would fail the GPU comparison."""
    for batch in ("trips:lean", "structures:one"):
        for loss in ("squared", "poisson"):
            c = th.case(batch, loss, True, 1)
            b, kw = c["b"], dict(c["kw"], variance_mode=1)
            r = th.reference(c)
            theta = np.random.default_rng(3).standard_normal(int(r["coef_ptr"][-1])) * 0.1
            clean = np.array([not th.has_duplicates(e) for e in c["entities"]])
            assert clean.any() and clean.all() == (batch == "trips:lean")
            mine = th.variance_dense(b, r["pk"], kw, loss, theta, r["coef_ptr"])
            theirs = lh.variance_numpy(b, r["pk"], kw, 1) if loss == "squared" else ph.variance_numpy(b, r["pk"], kw, 1, theta, r["coef_ptr"])
            keep = np.repeat(clean, np.diff(r["coef_ptr"]))
            np.testing.assert_allclose(mine[keep], theirs[keep], rtol=1e-12)
    c = th.case("structures:one", "squared", True, 1)
    r = th.reference(c)
    for k, e in enumerate(c["entities"]):
        X, _, w = th.entity_dense(c["b"], r["pk"], k, 1)
        assert np.array_equal(X, lh.entity_dense(c["b"], r["pk"], k, True)[0]), e["name"]      # (from the packed arrays and from the raw ones)
        if th.has_duplicates(e):
            row_of = np.repeat(np.arange(e["lens"].size), e["lens"])
            cells = (X[:, 1:] ** 2 * w[:, None]).sum(0)
            entries = np.bincount(np.searchsorted(np.unique(e["col"]), e["col"]), weights=e["val"].astype(np.float64) ** 2 * w[row_of], minlength=e["d"])
            assert np.max(np.abs(cells - entries) / cells) > 1e-3, e["name"]
