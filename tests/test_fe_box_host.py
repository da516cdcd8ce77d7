"""--coefficient_constraints of the fixed-effect stage on the host (gdmix_amd/fe_model.py, params.py, fixed_effect.fit_stepping,
solver.EXPORTED_SYMBOLS): the constraint file as arrays, what the flag refuses and where it is ignored, the plain fit left alone without it, and
the tests' own numpy restatement of the projected L-BFGS step (tests/fe_box_helpers.py) against the algorithm-independent reference on the cases
the GPU tests run. None of it needs a device."""
import json
import os
import types

import numpy as np
import pytest

from gdmix_amd import fixed_effect as fe
from gdmix_amd import params, solver
from gdmix_amd.fe_model import FixedLRParams
from gdmix_amd.params import REParams
import fe_box_helpers as H
from test_fe_sweep_host import HostFe, _scores, _stage

BASE = ["--metadata_file=m.json", "--output_model_dir=out"]
BAG = BASE + ["--feature_bag=global", "--feature_file=features.csv"]
FEATURES = [("age", "young"), ("age", "old"), ("price", ""), ("distance", "km"), ("clicks", "7d")]
INF = float("inf")


# ---- the constraint file as arrays ---------------------------------------------------------------------------------------------------
def test_records_become_the_right_arrays():
    records = [{"name": "price", "term": "", "upperBound": 0.0},                             # a sign constraint, by an exact record
               {"name": "age", "term": "*", "lowerBound": -1.0, "upperBound": 1.0},          # every term of a name
               {"name": "age", "term": "old", "lowerBound": 0.25, "upperBound": 0.25},       # an exact record beats the term wildcard: pinned
               {"name": "*", "term": "*", "lowerBound": -5}]                                 # everything not named otherwise
    lo, hi = params.coefficient_bounds(records, FEATURES, has_intercept=True)
    assert lo.dtype == hi.dtype == np.float64
    assert lo.tolist() == [-1.0, 0.25, -INF, -5.0, -5.0, -INF] and hi.tolist() == [1.0, 0.25, 0.0, INF, INF, INF]      # the intercept, last, is infinite
    again = params.coefficient_bounds(records[::-1], FEATURES, has_intercept=True)      # precedence is by specificity, not by order
    assert again[0].tolist() == lo.tolist() and again[1].tolist() == hi.tolist()
    lo, hi = params.coefficient_bounds([{"name": "*", "term": "*", "lowerBound": 0}], FEATURES, has_intercept=False)
    assert lo.tolist() == [0.0] * 5 and hi.tolist() == [INF] * 5
    lo, hi = params.coefficient_bounds([], FEATURES, has_intercept=True)
    assert np.all(lo == -INF) and np.all(hi == INF) and lo.size == 6


@pytest.mark.parametrize("records, message", [
    ([{"name": "height", "term": "", "lowerBound": 0}], "matches no feature"),
    ([{"name": "height", "term": "*", "lowerBound": 0}], "matches no feature"),
    ([{"name": "age", "term": "old", "lowerBound": 0}, {"name": "age", "term": "old", "upperBound": 1}], "same features"),
    ([{"name": "age", "term": "*", "lowerBound": 0}, {"name": "age", "term": "*", "upperBound": 1}], "same features"),
    ([{"name": "*", "term": "*", "lowerBound": 0}, {"name": "*", "term": "*", "upperBound": 1}], "same features"),
    ([{"name": "price", "term": "", "lowerBound": 1, "upperBound": 0.5}], "lowerBound > upperBound"),
    ([{"name": "price", "term": "", "lowerBound": "0"}], "finite number"),
    ([{"name": "(INTERCEPT)", "term": "", "lowerBound": 0}], "intercept"),
    ([{"name": "*", "term": "km", "lowerBound": 0}], "wildcard"),
    ([{"name": "price", "lowerBound": 0}], "name.*term"),
    ([{"name": "price", "term": "", "lower": 0}], "unknown keys"),
    ({"name": "price", "term": ""}, "array")])
def test_a_bad_record_is_refused_and_named(records, message):
    with pytest.raises(ValueError, match=message) as e:
        params.coefficient_bounds(records, FEATURES, has_intercept=True)
    if isinstance(records, list):
        assert any(repr(r) in str(e.value) for r in records)      # the message names the record


@pytest.mark.parametrize("literal", ["NaN", "Infinity", "-Infinity", "1e999"])
def test_a_non_finite_number_in_the_file_is_refused(tmp_path, literal):
    path = tmp_path / "c.json"
    path.write_text('[{"name": "price", "term": "", "upperBound": %s}]' % literal)
    with pytest.raises(ValueError, match="finite number"):
        params.read_coefficient_constraints(str(path), FEATURES, True)
    path.write_text('[{"name": "price", "term": "", "upperBound": -0.5}]')
    lo, hi = params.read_coefficient_constraints(str(path), FEATURES, True)
    assert hi[2] == -0.5 and lo[2] == -INF
    path.write_text("[{")
    with pytest.raises(ValueError, match="not JSON"):
        params.read_coefficient_constraints(str(path), FEATURES, True)


# ---- the flag ------------------------------------------------------------------------------------------------------------------------
def test_the_flag_parses_and_defaults_to_none():
    p = FixedLRParams.__from_argv__(BAG + ["--coefficient_constraints=c.json"], error_on_unknown=True)
    assert p.coefficient_constraints == "c.json"
    assert FixedLRParams.__from_argv__(p.__to_argv__()) == p
    assert FixedLRParams.__from_argv__(BAG).coefficient_constraints is None


@pytest.mark.parametrize("other", ["--l1_reg_weight=3", "--optimizer=TRON", "--optimizer=tron", "--incremental_training=true",
                                   "--feature_normalization=scale_with_standard_deviation", "--feature_normalization=scale_with_max_magnitude"])
def test_each_refusal_names_both_flags(other):
    with pytest.raises(ValueError) as e:
        FixedLRParams.__from_argv__(BAG + ["--coefficient_constraints=c.json", other])
    assert "--coefficient_constraints" in str(e.value) and other.split("=")[0] in str(e.value)
    FixedLRParams.__from_argv__(BAG + [other])      # without the constraints the other flag is today's


def test_what_the_flag_composes_with():
    for other in (["--feature_normalization=none"], ["--l1_reg_weight=0"], ["--optimizer=LBFGS"], ["--l2_reg_weights=10,1"], ["--down_sampling_rate=0.5"],
                  ["--fixed_effect_variance_mode=simple"], ["--metric_output_dir=m"]):
        assert FixedLRParams.__from_argv__(BAG + ["--coefficient_constraints=c.json"] + other).coefficient_constraints == "c.json"


def test_the_flag_without_a_feature_file_is_refused():
    with pytest.raises(ValueError) as e:
        FixedLRParams.__from_argv__(BASE + ["--coefficient_constraints=c.json"])
    assert "--coefficient_constraints" in str(e.value) and "--feature_file" in str(e.value)
    with pytest.raises(ValueError, match="--feature_file"):
        FixedLRParams.__from_argv__(BASE + ["--feature_bag=global", "--coefficient_constraints=c.json"])


def test_the_random_effect_refuses_the_flag():
    assert REParams.__from_argv__(BASE).coefficient_constraints is None
    with pytest.raises(ValueError, match="random effect has no box constraints"):
        REParams.__from_argv__(BASE + ["--coefficient_constraints=c.json"])


def test_the_symbol_is_exported():
    assert "gdmix_fe_set_bounds" in solver.EXPORTED_SYMBOLS


# ---- the stage, over a stand-in solver -------------------------------------------------------------------------------------------------
class BoxFe(HostFe):
    """Records the bounds a stage asks for; the fit itself is the stand-in's ridge fit (this file does not test the optimiser through it)."""

    def __init__(self):
        super().__init__()
        self.bounds = []

    def fit_stepping(self, *a, **k):
        self.bounds.append(k.pop("bounds", None))
        return super().fit_stepping(*a, **k)

    def fit_sweep(self, *a, **k):
        self.bounds.append(k.pop("bounds", None))
        return super().fit_sweep(*a, **k)


def _constraints(tmp_path, records):
    path = tmp_path / "constraints.json"
    path.write_text(json.dumps(records))
    return f"--coefficient_constraints={path}"


def test_the_stage_passes_the_bounds_and_only_when_the_flag_is_set(tmp_path, monkeypatch):
    flag = _constraints(tmp_path, [{"name": "f1", "term": "t1", "upperBound": 0.0}, {"name": "*", "term": "*", "lowerBound": -2.0, "upperBound": 2.0}])
    driver, schema, model, c = _stage(tmp_path / "a", monkeypatch, extra=[flag])
    model._fe = BoxFe()
    driver.run_training(schema)
    (lo, hi), = model._fe.bounds
    D = int(c["num_features"])
    assert lo.shape == hi.shape == (D + 1,) and lo[-1] == -INF and hi[-1] == INF      # the intercept, last, is free
    assert (lo[1], hi[1]) == (-INF, 0.0) and np.all(lo[[0] + list(range(2, D))] == -2.0) and np.all(hi[[0] + list(range(2, D))] == 2.0)
    driver, schema, model, _ = _stage(tmp_path / "b", monkeypatch)
    model._fe = BoxFe()
    driver.run_training(schema)
    assert model._fe.bounds == [None]      # no flag: fit_stepping is called as it was before the flag existed


def test_the_sweep_passes_the_bounds(tmp_path, monkeypatch):
    flag = _constraints(tmp_path, [{"name": "*", "term": "*", "lowerBound": 0.0}])
    driver, schema, model, c = _stage(tmp_path, monkeypatch, extra=[flag, "--l2_reg_weights=10,1", f"--metric_output_dir={tmp_path / 'metrics'}"])
    model._fe = BoxFe()
    driver.run_training(schema)
    (lo, hi), = model._fe.bounds
    assert np.all(lo[:-1] == 0.0) and lo[-1] == -INF and np.all(hi == INF) and model._fe.fits == [10.0, 1.0]


def test_a_bad_file_is_refused_before_any_data_is_read(tmp_path, monkeypatch):
    flag = _constraints(tmp_path, [{"name": "no_such_feature", "term": "", "lowerBound": 0.0}])
    driver, schema, model, _ = _stage(tmp_path, monkeypatch, extra=[flag])
    model._fe = BoxFe()
    monkeypatch.setattr(model, "_read", lambda *a, **k: (_ for _ in ()).throw(AssertionError("a shard was read")))
    with pytest.raises(ValueError, match="no_such_feature.*matches no feature"):
        driver.run_training(schema)
    assert model._fe.bounds == []


def test_inference_accepts_the_flag_and_ignores_it(tmp_path, monkeypatch):
    driver, schema, model, c = _stage(tmp_path, monkeypatch)
    driver.run_training(schema)      # a model to score with
    plain = tmp_path / "plain"
    os.rename(tmp_path / "vs", plain)
    os.makedirs(tmp_path / "vs")
    # the file does not exist, next to a flag a training run refuses: inference does not look at either
    drv, sch, m2, _ = _stage(tmp_path, monkeypatch, extra=[f"--coefficient_constraints={tmp_path / 'no_such_file.json'}"], action="inference")
    m2._fe = BoxFe()
    drv.run_inference(sch)
    assert m2._fe.bounds == [] and m2._fe.fits == []
    (s0, y0), (s1, y1) = _scores(plain / "part-00000.avro"), _scores(tmp_path / "vs" / "part-00000.avro")
    assert s0.size == c["v_y"].size and np.array_equal(s0, s1) and np.array_equal(y0, y1)      # (the trained model's scores, bit for bit)


# ---- fit_stepping: without bounds the problem never sees set_bounds ---------------------------------------------------------------------------
class _StubProblem:
    def __init__(self):
        self.calls, self.theta0 = [], "theta0"

    def set_bounds(self, lower, upper):
        self.calls.append(("set_bounds", lower.tolist(), upper.tolist()))
        self.theta0 = None

    def restart(self, opts, theta0):
        self.calls.append(("restart", theta0))

    def close(self):
        self.calls.append(("close",))


class _StubFit:
    last = None

    def __init__(self, *a, **k):
        self.prob = _StubProblem()
        type(self).last = self

    def device_bounds(self, bounds):
        return bounds

    def run(self):
        self.prob.calls.append(("run",))
        return np.array([0.0, 1.5, 0.25, -2.0]), {"fval": 1.0, "nit": 1, "nfev": 2, "status": 0}

    def stage_result(self, theta, info, l2, threshold):
        return theta, info


def _stub_fit(monkeypatch, **kw):
    monkeypatch.setattr(fe, "_SteppingFit", _StubFit)
    s = fe.FixedEffectDeviceSolver(solver=types.SimpleNamespace())
    theta, info = s.fit_stepping(np.array([0, 1]), np.array([0]), np.array([1.0], np.float32), np.array([1.0], np.float32), 3, **kw)
    return info, _StubFit.last.prob.calls


def test_without_bounds_a_stubbed_problem_never_sees_set_bounds(monkeypatch):
    info, calls = _stub_fit(monkeypatch)
    assert calls == [("run",), ("close",)] and "at_bound" not in info
    info, calls = _stub_fit(monkeypatch, bounds=None)
    assert calls == [("run",), ("close",)]
    lo, hi = [0.0, -INF, 0.25, -INF], [INF, 1.5, 0.25, INF]
    info, calls = _stub_fit(monkeypatch, bounds=(lo, hi))      # set_bounds leaves the problem at the clamped zeros: the start point is put back behind it
    assert calls == [("set_bounds", lo, hi), ("restart", "theta0"), ("run",), ("close",)] and info["at_bound"] == 3


def test_fit_stepping_refuses_bad_bounds_and_what_does_not_compose(monkeypatch):
    ok = ([0.0, -INF, 0.25, -INF], [INF, 1.5, 0.25, INF])
    for bad, message in ((([0.0, float("nan"), 0.0, -INF], ok[1]), "coefficient 1.*not a number"), (([0.0, 2.0, 0.25, -INF], ok[1]), "coefficient 1.*lower"),
                         ((ok[0], [INF, 1.5, 0.25, 3.0]), "intercept"), (([0.0, 0.0, -INF], [INF, INF, INF]), "4 entries"), (ok[0], "pair")):
        with pytest.raises(ValueError, match=message):
            _stub_fit(monkeypatch, bounds=bad)
    for kw in (dict(l1=1.0), dict(optimizer="TRON"), dict(prior=(np.zeros(4), np.ones(4))), dict(feature_scale=np.ones(3))):
        with pytest.raises(ValueError, match="bounds"):
            _stub_fit(monkeypatch, bounds=ok, **kw)


# ---- the restatement against the reference ----------------------------------------------------------------------------------------------
AT_BOUND = {("logistic", "small"): 19, ("squared", "small"): 19, ("poisson", "small"): 20, ("logistic", "wide"): 2560, ("squared", "wide"): 2455,
            ("poisson", "wide"): 2473}      # coefficients of the reference's minimiser at a bound


@pytest.mark.parametrize("m", [10, 3])
@pytest.mark.parametrize("size", ["small", "wide"])
@pytest.mark.parametrize("loss", H.LOSSES)
def test_the_restatement_finds_the_reference_minimiser(loss, size, m):
    pb = H.problem(loss, size)
    lo, hi = H.bounds(size)
    theta_ref, f_ref = H.reference(loss, size)
    assert int(H.at_bound(theta_ref, lo, hi).sum()) == AT_BOUND[loss, size] and np.all((lo <= theta_ref) & (theta_ref <= hi))
    x, F, status, nit, nfev = H.box(pb, lo, hi, m=m, max_iter=H.FIT["max_iter"], ftol=H.FIT["tolerance"])
    print(f"{loss} {size} m = {m}: restatement status {status} nit {nit} nfev {nfev}")
    assert status in (0, 1)
    H.check_against_reference(pb, lo, hi, x, F, theta_ref, f_ref, f"{loss} {size} m = {m}")


def test_the_binding_set_and_the_residual_by_cases():
    lo, hi = np.array([0.0, 0.0, -1.0, -1.0, 0.5, -INF]), np.array([INF, INF, 1.0, 1.0, 0.5, INF])
    x = np.array([0.0, 0.0, 1.0, 1.0, 0.5, 3.0])
    g = np.array([2.0, -2.0, -3.0, 3.0, 7.0, 0.5])
    assert H.binding(x, g, lo, hi).tolist() == [True, False, True, False, True, False]
    assert H.projected_gradient_norm(x, g, lo, hi) == 2.0      # coefficient 1 may move up by 2, coefficient 3 down by 2 to its lower bound
    pb = types.SimpleNamespace(smooth=lambda th: (0.0, g))
    assert H.residual(pb, x, lo, hi).tolist() == [0.0, -2.0, 0.0, 3.0, 0.0, 0.5]
