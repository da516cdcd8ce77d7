"""--l1_reg_weight of the fixed-effect stage on the host (gdmix_amd/fe_model.py, params.py, fixed_effect.fit_stepping, solver.EXPORTED_SYMBOLS):
the flag, what it refuses and where it is ignored, the plain fit left alone at l1 = 0, and the tests' own numpy restatement of OWL-QN
(tests/fe_l1_helpers.py) against the algorithm-independent reference on the six cases the GPU tests run. None of it needs a device."""
import os
import types

import numpy as np
import pytest

from gdmix_amd import fixed_effect as fe
from gdmix_amd import solver
from gdmix_amd.fe_model import FixedLRParams
from gdmix_amd.params import REParams
import fe_l1_helpers as H
from test_fe_sweep_host import HostFe, _scores, _stage

BASE = ["--metadata_file=m.json", "--output_model_dir=out"]


# ---- the flag ------------------------------------------------------------------------------------------------------------------------
def test_the_flag_parses_and_defaults_to_zero():
    p = FixedLRParams.__from_argv__(BASE + ["--l1_reg_weight=3"], error_on_unknown=True)
    assert p.l1_reg_weight == 3.0 and isinstance(p.l1_reg_weight, float)
    assert FixedLRParams.__from_argv__(p.__to_argv__()) == p
    assert FixedLRParams.__from_argv__(BASE).l1_reg_weight == 0.0
    assert FixedLRParams.__from_argv__(BASE + ["--l1_reg_weight", "0.25", "--l2_reg_weight=0.75"]).l1_reg_weight == 0.25


@pytest.mark.parametrize("bad", ["-1", "nan", "inf", "-inf", "-1e-300"])
def test_a_bad_weight_is_refused_at_parse_time(bad):
    with pytest.raises(ValueError, match="l1_reg_weight"):
        FixedLRParams.__from_argv__(BASE + [f"--l1_reg_weight={bad}"])


@pytest.mark.parametrize("other", ["--l2_reg_weights=10,1", "--incremental_training=true", "--feature_normalization=scale_with_standard_deviation",
                                   "--feature_normalization=scale_with_max_magnitude"])
def test_each_refusal_names_both_flags(other):
    with pytest.raises(ValueError) as e:
        FixedLRParams.__from_argv__(BASE + ["--l1_reg_weight=3", other])
    assert "--l1_reg_weight" in str(e.value) and other.split("=")[0] in str(e.value)
    assert FixedLRParams.__from_argv__(BASE + ["--l1_reg_weight=0", other]).l1_reg_weight == 0.0      # without an L1 term the other flag is today's
    assert FixedLRParams.__from_argv__(BASE + ["--l1_reg_weight=3", "--feature_normalization=none"]).l1_reg_weight == 3.0


def test_the_random_effect_refuses_a_non_zero_value():
    assert REParams.__from_argv__(BASE).l1_reg_weight == 0.0
    assert REParams.__from_argv__(BASE + ["--l1_reg_weight=0"]).l1_reg_weight == 0.0
    with pytest.raises(ValueError, match="random effect has no L1 term"):
        REParams.__from_argv__(BASE + ["--l1_reg_weight=0.5"])
    with pytest.raises(ValueError, match="l1_reg_weight"):
        REParams.__from_argv__(BASE + ["--l1_reg_weight=nan"])


def test_the_symbol_is_exported():
    assert "gdmix_fe_set_l1" in solver.EXPORTED_SYMBOLS


# ---- the stage, over a stand-in solver -------------------------------------------------------------------------------------------------
class L1Fe(HostFe):
    """Records the l1 a stage asks for; the fit itself is the stand-in's ridge fit (this file does not test the optimiser through it)."""

    def __init__(self):
        super().__init__()
        self.l1 = []

    def fit_stepping(self, *a, **k):
        self.l1.append(k.pop("l1", None))
        return super().fit_stepping(*a, **k)


def test_the_stage_passes_the_weight_and_only_when_it_is_set(tmp_path, monkeypatch):
    driver, schema, model, _ = _stage(tmp_path / "a", monkeypatch, extra=["--l1_reg_weight=3"])
    model._fe = L1Fe()
    driver.run_training(schema)
    assert model._fe.l1 == [3.0]
    driver, schema, model, _ = _stage(tmp_path / "b", monkeypatch)
    model._fe = L1Fe()
    driver.run_training(schema)
    assert model._fe.l1 == [None]      # l1 = 0: fit_stepping is called as it was before the flag existed


def test_inference_accepts_the_flag_and_ignores_it(tmp_path, monkeypatch):
    driver, schema, model, c = _stage(tmp_path, monkeypatch)
    driver.run_training(schema)      # a model to score with
    plain = tmp_path / "plain"
    os.rename(tmp_path / "vs", plain)
    os.makedirs(tmp_path / "vs")
    # with flags next to it that a training run refuses: inference does not look at any of them
    drv, sch, m2, _ = _stage(tmp_path, monkeypatch, extra=["--l1_reg_weight=3"], action="inference")
    m2._fe = L1Fe()
    drv.run_inference(sch)
    assert m2._fe.l1 == [] and m2._fe.fits == []
    (s0, y0), (s1, y1) = _scores(plain / "part-00000.avro"), _scores(tmp_path / "vs" / "part-00000.avro")
    assert s0.size == c["v_y"].size and np.array_equal(s0, s1) and np.array_equal(y0, y1)      # (the trained model's scores, bit for bit)


# ---- fit_stepping: l1 = 0 never reaches set_l1 ----------------------------------------------------------------------------------------
class _StubProblem:
    def __init__(self):
        self.calls, self.theta0 = [], "theta0"

    def set_l1(self, l1):
        self.calls.append(("set_l1", l1))
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

    def run(self):
        self.prob.calls.append(("run",))
        return np.array([0.0, 1.5, 0.0, -2.0]), {"fval": 1.0, "nit": 1, "nfev": 2, "status": 0}

    def stage_result(self, theta, info, l2, threshold):
        return theta, info


def _stub_fit(monkeypatch, **kw):
    monkeypatch.setattr(fe, "_SteppingFit", _StubFit)
    s = fe.FixedEffectDeviceSolver(solver=types.SimpleNamespace())
    theta, info = s.fit_stepping(np.array([0, 1]), np.array([0]), np.array([1.0], np.float32), np.array([1.0], np.float32), 3, **kw)
    return info, _StubFit.last.prob.calls


def test_with_l1_zero_a_stubbed_problem_never_sees_set_l1(monkeypatch):
    info, calls = _stub_fit(monkeypatch)
    assert calls == [("run",), ("close",)] and info["l1"] == 0.0 and info["nnz"] == 2
    info, calls = _stub_fit(monkeypatch, l1=0.0)
    assert calls == [("run",), ("close",)]
    info, calls = _stub_fit(monkeypatch, l1=2.5)      # set_l1 leaves the problem at zeros: the start point is put back behind it
    assert calls == [("set_l1", 2.5), ("restart", "theta0"), ("run",), ("close",)] and info["l1"] == 2.5 and info["nnz"] == 2


@pytest.mark.parametrize("bad", [-1.0, float("nan"), float("inf")])
def test_fit_stepping_refuses_a_bad_weight_and_what_does_not_compose(monkeypatch, bad):
    with pytest.raises(ValueError, match="l1"):
        _stub_fit(monkeypatch, l1=bad)
    with pytest.raises(ValueError, match="prior"):
        _stub_fit(monkeypatch, l1=1.0, prior=(np.zeros(4), np.ones(4)))
    with pytest.raises(ValueError, match="normalisation"):
        _stub_fit(monkeypatch, l1=1.0, feature_scale=np.ones(3))


# ---- the restatement against the reference ----------------------------------------------------------------------------------------------
NNZ = {("logistic", "small"): 9, ("logistic", "wide"): 605, ("squared", "small"): 24, ("squared", "wide"): 2567, ("poisson", "small"): 30,
       ("poisson", "wide"): 2758}      # features in the reference's support (the intercept, non-zero in every case, comes on top)


@pytest.mark.parametrize("size", ["small", "wide"])
@pytest.mark.parametrize("loss", H.LOSSES)
def test_the_restatement_finds_the_reference_minimiser(loss, size):
    pb = H.problem(loss, size)
    theta_ref, f_ref = H.reference(loss, size)
    assert np.count_nonzero(theta_ref[:-1]) == NNZ[loss, size] and theta_ref[-1] != 0.0
    x, F, status, nit, nfev = H.owlqn(pb, m=H.FIT["m"], max_iter=H.FIT["max_iter"], ftol=H.FIT["tolerance"])
    print(f"{loss} {size}: restatement status {status} nit {nit} nfev {nfev}")
    assert status in (0, 1)
    H.check_against_reference(pb, x, F, theta_ref, f_ref, f"{loss} {size}")


def test_the_pseudo_gradient_by_cases():
    pb = H.Problem("squared", H.design(np.array([0, 1]), np.array([0]), np.array([1.0], np.float32), 5, has_intercept=False), np.zeros(1), np.zeros(1), 2.0, 0.0,
                   mask=[1, 1, 1, 1, 0])
    th = np.array([1.0, -1.0, 0.0, 0.0, 0.0])
    g = np.array([0.5, 0.5, -3.0, 1.0, 0.5])
    assert pb.pseudo_gradient(th, g).tolist() == [2.5, -1.5, -1.0, 0.0, 0.5]
    assert pb.pseudo_gradient(np.zeros(5), np.array([3.0, -3.0, 2.0, -2.0, -0.1])).tolist() == [1.0, -1.0, 0.0, 0.0, -0.1]
