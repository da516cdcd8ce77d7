"""Host side of the device evaluator (gdmix_amd/metrics.py, gdmix_amd/evaluate.py): the sortable key, the numpy reference the GPU
tests lean on (tests/metrics_reference.py), and the command line's argument handling. No device is touched."""
import os
import subprocess
import sys

import numpy as np
import pytest

from gdmix_amd import chain, evaluate, metrics

from metrics_reference import auc_reference, two_u_reference

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _key_cases():
    tiny = np.float32(1e-45)            # the smallest denormal
    fixed = np.array([0.0, -0.0, tiny, -tiny, np.float32(1.1754942e-38), -np.float32(1.1754942e-38), np.float32(1.17549435e-38),
                      np.inf, -np.inf, 1.0, np.nextafter(np.float32(1.0), np.float32(2.0)), np.nextafter(np.float32(1.0), np.float32(0.0)),
                      -1.0, np.nextafter(np.float32(-1.0), np.float32(-2.0)), np.nextafter(np.float32(-1.0), np.float32(0.0)),
                      np.finfo(np.float32).max, -np.finfo(np.float32).max, 0.1, -0.1], np.float32)
    return np.concatenate([fixed, np.random.default_rng(7).standard_normal(100_000).astype(np.float32)])


def test_sortable_key_orders_as_the_floats_do():
    s = _key_cases()
    k = metrics.sortable_key(s)
    assert k.dtype == np.uint32 and k.shape == s.shape
    order = np.argsort(s, kind="stable")
    ss, ks = s[order], k[order].astype(np.int64)
    d = np.diff(ks)
    assert np.array_equal(d > 0, ss[1:] > ss[:-1]) and np.array_equal(d == 0, ss[1:] == ss[:-1])
    # all pairs of the fixed list, both directions
    f, kf = s[:19], k[:19].astype(np.int64)
    assert np.array_equal(f[:, None] < f[None, :], kf[:, None] < kf[None, :])
    assert np.array_equal(f[:, None] == f[None, :], kf[:, None] == kf[None, :])


def test_negative_zero_and_positive_zero_share_a_key():
    k = metrics.sortable_key(np.array([0.0, -0.0], np.float32))
    assert k[0] == k[1] == 0x80000000
    assert metrics.sortable_key(np.array([np.inf], np.float32))[0] < 0xFFFFFFFF     # the device's key for "no score" is above every score's


def _tied_case(seed, n):
    rng = np.random.default_rng(seed)
    s = np.round(rng.standard_normal(n), 1).astype(np.float32)
    y = (rng.random(n) < 1.0 / (1.0 + np.exp(-s))).astype(np.float32)
    return s, y


@pytest.mark.parametrize("seed", range(20))
def test_reference_agrees_with_chain_auc_on_heavy_ties(seed):
    s, y = _tied_case(seed, 500 + 137 * seed)
    assert np.unique(s).size < s.size / 4
    assert abs(auc_reference(s, y) - chain.auc(y, s)) <= 1e-12
    two_u, n_pos, n_neg, n_nan = two_u_reference(s, y)
    assert n_pos + n_neg == s.size and n_nan == 0
    assert metrics.auc_from_counts(two_u, n_pos, n_neg) == auc_reference(s, y)


@pytest.mark.parametrize("seed", range(8))
def test_reference_is_the_quadratic_definition(seed):
    s, y = _tied_case(100 + seed, 200 - 23 * seed)
    if seed == 3:
        s[:5] = [0.0, -0.0, np.inf, -np.inf, np.inf]
    pos = y > 0.5
    want = sum(2 * int((s[~pos] < si).sum()) + int((s[~pos] == si).sum()) for si in s[pos])
    assert two_u_reference(s, y)[:3] == (want, int(pos.sum()), int((~pos).sum()))


def test_reference_leaves_nan_scores_out():
    s, y = _tied_case(5, 100)
    want = two_u_reference(s, y)
    s2 = np.concatenate([s, [np.nan, np.nan, np.nan]]).astype(np.float32)
    y2 = np.concatenate([y, [1.0, 0.0, 1.0]]).astype(np.float32)
    assert two_u_reference(s2, y2) == want[:3] + (3,)


def test_auc_from_counts():
    assert metrics.auc_from_counts(3, 1, 2) == 0.75
    assert np.isnan(metrics.auc_from_counts(0, 0, 5)) and np.isnan(metrics.auc_from_counts(0, 5, 0))
    # correctly rounded from integers that no longer fit a double
    from fractions import Fraction
    tu, p, n = (1 << 61) + 1, (1 << 30) + 1, (1 << 30) + 3
    assert metrics.auc_from_counts(tu, p, n) == float(Fraction(tu, 2 * p * n))


GOOD = ["--metricsInputDir", "in", "--outputMetricFile", "out", "--labelColumnName", "response", "--predictionColumnName", "predictionScore",
        "--metricName", "auc"]


def test_parse_takes_the_spark_jobs_flags():
    p = evaluate.parse(GOOD)
    assert p == dict(metricsInputDir="in", outputMetricFile="out", labelColumnName="response", predictionColumnName="predictionScore", metricName="auc")
    assert evaluate.parse([f"{GOOD[i]}={GOOD[i + 1]}" for i in range(0, len(GOOD), 2)]) == p
    assert evaluate.parse(GOOD[:-1] + ["mse"])["metricName"] == "mse"


@pytest.mark.parametrize("drop", range(0, len(GOOD), 2))
def test_parse_refuses_a_missing_flag(drop):
    with pytest.raises(ValueError, match=GOOD[drop][2:]):
        evaluate.parse(GOOD[:drop] + GOOD[drop + 2:])


def test_unknown_metric_name_has_the_evaluators_wording():
    with pytest.raises(ValueError, match="Do not support metric rmse, currently only support 'auc' and 'mse'."):
        evaluate.parse(GOOD[:-1] + ["rmse"])


def test_command_line_fails_before_the_device_is_touched(tmp_path):
    """An unknown metric and a missing flag end the process with a message and no output, whether or not a device is present: the
    arguments are checked first (the input directory does not even exist)."""
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""), HIP_VISIBLE_DEVICES="")
    out = str(tmp_path / "metric")
    for argv, word in ((GOOD[:-1] + ["rmse"], "Do not support metric rmse"), (GOOD[2:], "metricsInputDir")):
        argv = [a if a != "out" else out for a in argv]
        cp = subprocess.run([sys.executable, "-m", "gdmix_amd.evaluate"] + argv, cwd=ROOT, env=env, capture_output=True, text=True)
        assert cp.returncode != 0 and word in cp.stderr, cp.stderr
        assert not os.path.exists(out)
