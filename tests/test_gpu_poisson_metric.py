"""GPU: the Poisson loss of a scored set on the device (include/gdmix_re.h, "poisson evaluation"; csrc/re_evaluate_poisson.hip),
PL = sum (exp(s) - y s), per entity on both paths (entities of up to 64 samples in registers, larger ones by a workgroup) and
accumulated over a stage's batches, against math.fsum of the numpy statement (metrics.poisson_loss_terms). The bound is the header's:
|PL - fsum| <= 3e-13 * sum (exp(s) + |y s|) — SSE's 2.5e-13 plus two roundings per term."""
import math

import numpy as np
import pytest

from gdmix_amd import metrics

pytestmark = pytest.mark.gpu

SIZES = [1, 63, 64, 65, 2049, 5000, 0, 17, 5]      # the issue's sizes, an empty entity, and two more for the 16- / 32-lane widths


def _case(seed=3):
    rng = np.random.default_rng(seed)
    n = np.array(SIZES)
    rp = np.concatenate([[0], np.cumsum(n)]).astype(np.int64)
    N = int(rp[-1])
    s = (1.5 * rng.standard_normal(N)).astype(np.float32)
    y = rng.poisson(np.exp(0.5 * s.astype(np.float64))).astype(np.float32)
    s[int(rp[3]) + 7] = np.nan                      # one NaN score, in the entity of 65 samples
    y[int(rp[4]):int(rp[5])] = 0.0                  # one entity with all labels 0 (2 049 samples)
    return rp, s, y


def _want(s, y):
    ok = ~np.isnan(s)
    t = metrics.poisson_loss_terms(s[ok], y[ok])
    mag = np.exp(s[ok].astype(np.float64)) + np.abs(y[ok].astype(np.float64) * s[ok].astype(np.float64))
    return math.fsum(t), math.fsum(mag), int(ok.sum()), int((~ok).sum())


@pytest.mark.parametrize("small_max", [64, 0])
def test_poisson_loss_per_entity_on_both_paths(device_solver, small_max):
    rp, s, y = _case()
    ev = metrics.PoissonEvaluator(device_solver)
    ev.set_small_max(small_max)
    try:
        got = ev.entities(rp, s, y)
        again = ev.entities(rp, s, y)
    finally:
        ev.set_small_max(64)
    h = metrics.poisson_entities_to_host(got)
    assert np.array_equal(again["pl"].cpu().numpy().view(np.uint64), got["pl"].cpu().numpy().view(np.uint64))      # the same bits from run to run
    worst = 0.0
    for e in range(rp.size - 1):
        a, b = int(rp[e]), int(rp[e + 1])
        want, mag, n, n_nan = _want(s[a:b], y[a:b])
        assert int(h["n"][e]) == b - a and int(h["n_nan"][e]) == n_nan, e
        assert abs(h["pl"][e] - want) <= 3e-13 * mag, (e, float(h["pl"][e]), want)
        worst = max(worst, abs(h["pl"][e] - want) / max(mag, 1e-300))
        if b == a or n_nan:
            assert np.isnan(h["poisson_loss"][e])
        else:
            assert abs(h["poisson_loss"][e] - want / n) <= 1e-15 * mag / n + abs(h["pl"][e] - want) / n
    print(f"per entity (small_max {small_max}): worst |PL - fsum| / sum of magnitudes {worst:.3e}")
    # E = 1
    one = metrics.poisson_entities_to_host(ev.entities(np.array([0, 65], np.int64), s[int(rp[3]):int(rp[4])], y[int(rp[3]):int(rp[4])]))
    want, mag, n, n_nan = _want(s[int(rp[3]):int(rp[4])], y[int(rp[3]):int(rp[4])])
    assert abs(one["pl"][0] - want) <= 3e-13 * mag and int(one["n_nan"][0]) == 1 and int(one["n"][0]) == 65


def test_poisson_loss_accumulated_over_batches_in_two_orders(device_solver):
    rp, s, y = _case(seed=4)
    cuts = [0, 1500, 1501, s.size]
    want, mag, n, n_nan = _want(s, y)
    results = []
    for order in ([0, 1, 2], [2, 0, 1]):
        ev = metrics.PoissonEvaluator(device_solver)
        for k in order:
            ev.add(s[cuts[k]:cuts[k + 1]], y[cuts[k]:cuts[k + 1]])
        r = ev.finish()
        assert (r["n"], r["n_nan"]) == (s.size, 1) and math.isnan(r["poisson_loss"])
        assert abs(r["pl"] - want) <= 3e-13 * mag, (r["pl"], want)
        results.append(r["pl"])
    print(f"accumulated: |PL - fsum| / sum of magnitudes {abs(results[0] - want) / mag:.3e}")
    assert np.float64(results[0]).view(np.uint64) == np.float64(results[1]).view(np.uint64)      # the two orders give the same bits
    # without the NaN: the mean, and E = 1 through the accumulator of one batch
    ok = ~np.isnan(s)
    ev = metrics.PoissonEvaluator(device_solver)
    ev.add(s[ok], y[ok])
    r = ev.finish()
    assert r["n_nan"] == 0 and abs(r["poisson_loss"] - want / n) <= 3e-13 * mag / n
    ev.reset()
    assert ev.count == 0 and math.isnan(ev.finish()["poisson_loss"])


def test_evaluate_cli_reports_poisson_loss(tmp_path, device_solver):
    from gdmix_amd import evaluate
    from gdmix_amd.io import avro
    rng = np.random.default_rng(6)
    s = rng.standard_normal(3000).astype(np.float32)
    y = rng.poisson(1.0, 3000).astype(np.float32)
    schema = {"type": "record", "name": "S", "fields": [{"name": "response", "type": "float"}, {"name": "predictionScore", "type": "float"}]}
    (tmp_path / "in").mkdir()
    avro.write_file(str(tmp_path / "in" / "part-0.avro"), schema, [{"response": float(a), "predictionScore": float(b)} for a, b in zip(y, s)])
    v = evaluate.run(["--metricsInputDir", str(tmp_path / "in"), "--outputMetricFile", str(tmp_path / "out"), "--labelColumnName", "response",
                      "--predictionColumnName", "predictionScore", "--metricName=poisson_loss"], solver=device_solver)
    want = math.fsum(metrics.poisson_loss_terms(s, y)) / 3000
    assert abs(v - want) <= 1e-12 * abs(want)
    import json
    assert json.load(open(tmp_path / "out" / "evalSummary.json")) == {"poisson_loss": v}
