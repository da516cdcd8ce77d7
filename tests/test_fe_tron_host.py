"""--optimizer of the fixed-effect stage on the host (gdmix_amd/fe_model.py, params.py, chain.py, fixed_effect.fit_stepping,
solver.EXPORTED_SYMBOLS): the flag, what it refuses and where it is ignored, the plain fit left alone under the default, and the tests'
own numpy restatement of TRON (tests/fe_tron_helpers.py) against the algorithm-independent reference on the six cases the GPU tests run.
None of it needs a device."""
import os
import types

import numpy as np
import pytest

from gdmix_amd import chain
from gdmix_amd import fixed_effect as fe
from gdmix_amd import solver
from gdmix_amd.fe_model import FixedLRParams
from gdmix_amd.params import REParams
import fe_tron_helpers as H
from test_fe_sweep_host import HostFe, _scores, _stage

BASE = ["--metadata_file=m.json", "--output_model_dir=out"]


# ---- the flag ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("text, want", [("TRON", "TRON"), ("tron", "TRON"), ("Tron", "TRON"), ("LBFGS", "LBFGS"), ("lbfgs", "LBFGS")])
def test_the_flag_parses_in_any_case_and_defaults_to_lbfgs(text, want):
    p = FixedLRParams.__from_argv__(BASE + [f"--optimizer={text}"], error_on_unknown=True)
    assert p.optimizer == want
    assert FixedLRParams.__from_argv__(p.__to_argv__()) == p
    assert FixedLRParams.__from_argv__(BASE).optimizer == "LBFGS"


@pytest.mark.parametrize("bad", ["OWLQN", "newton", "", "TRON2"])
def test_an_unknown_optimizer_is_refused_at_parse_time(bad):
    with pytest.raises(ValueError, match="optimizer"):
        FixedLRParams.__from_argv__(BASE + [f"--optimizer={bad}"])


@pytest.mark.parametrize("other", ["--l1_reg_weight=3", "--incremental_training=true", "--feature_normalization=scale_with_standard_deviation",
                                   "--feature_normalization=scale_with_max_magnitude"])
def test_each_refusal_names_both_flags(other):
    with pytest.raises(ValueError) as e:
        FixedLRParams.__from_argv__(BASE + ["--optimizer=TRON", other])
    assert "--optimizer" in str(e.value) and other.split("=")[0] in str(e.value)
    assert FixedLRParams.__from_argv__(BASE + ["--optimizer=LBFGS", other]).optimizer == "LBFGS"      # under the default the other flag is today's


def test_what_tron_runs_with():
    for ok in ("--l1_reg_weight=0", "--feature_normalization=none", "--l2_reg_weights=10,1", "--down_sampling_rate=0.5", "--fixed_effect_variance_mode=simple",
               "--model_type=linear_regression", "--model_type=poisson_regression", "--metric_output_dir=m"):
        assert FixedLRParams.__from_argv__(BASE + ["--optimizer=tron", ok]).optimizer == "TRON", ok


def test_the_random_effect_refuses_tron():
    assert REParams.__from_argv__(BASE).optimizer == "LBFGS"
    assert REParams.__from_argv__(BASE + ["--optimizer=lbfgs"]).optimizer == "lbfgs"
    with pytest.raises(ValueError, match="random effect trains by L-BFGS-B only"):
        REParams.__from_argv__(BASE + ["--optimizer=TRON"])


def test_the_symbols_are_exported():
    assert {"gdmix_fe_set_optimizer", "gdmix_fe_products", "gdmix_fe_hessian_vec"} <= set(solver.EXPORTED_SYMBOLS)


def test_the_chain_passes_the_flag_to_the_global_stage_only():
    assert chain.stage_argv("r", "global", optimizer="TRON")[-1] == "--optimizer=TRON" or "--optimizer=TRON" in chain.stage_argv("r", "global", optimizer="TRON")
    assert not any(a.startswith("--optimizer") for a in chain.stage_argv("r", "per_user", optimizer="TRON"))
    assert chain.stage_argv("r", "global", optimizer=None) == chain.stage_argv("r", "global")
    assert not any(a.startswith("--optimizer") for a in chain.stage_argv("r", "global"))


# ---- the stage, over a stand-in solver -------------------------------------------------------------------------------------------------
class OptFe(HostFe):
    """Records the optimizer a stage asks for; the fit itself is the stand-in's (this file does not test the optimiser through it)."""

    def __init__(self):
        super().__init__()
        self.optimizer = []

    def fit_stepping(self, *a, **k):
        self.optimizer.append(k.pop("optimizer", None))
        return super().fit_stepping(*a, **k)


def test_the_stage_passes_the_optimizer_and_only_when_it_is_set(tmp_path, monkeypatch):
    driver, schema, model, _ = _stage(tmp_path / "a", monkeypatch, extra=["--optimizer=tron"])
    model._fe = OptFe()
    driver.run_training(schema)
    assert model._fe.optimizer == ["TRON"]
    for extra in ([], ["--optimizer=LBFGS"]):
        driver, schema, model, _ = _stage(tmp_path / ("b" + str(len(extra))), monkeypatch, extra=extra)
        model._fe = OptFe()
        driver.run_training(schema)
        assert model._fe.optimizer == [None]      # the default: fit_stepping is called as it was before the flag existed


def test_inference_accepts_the_flag_and_ignores_it(tmp_path, monkeypatch):
    driver, schema, model, c = _stage(tmp_path, monkeypatch)
    driver.run_training(schema)      # a model to score with
    plain = tmp_path / "plain"
    os.rename(tmp_path / "vs", plain)
    os.makedirs(tmp_path / "vs")
    drv, sch, m2, _ = _stage(tmp_path, monkeypatch, extra=["--optimizer=TRON"], action="inference")
    m2._fe = OptFe()
    drv.run_inference(sch)
    assert m2._fe.optimizer == [] and m2._fe.fits == []
    (s0, y0), (s1, y1) = _scores(plain / "part-00000.avro"), _scores(tmp_path / "vs" / "part-00000.avro")
    assert s0.size == c["v_y"].size and np.array_equal(s0, s1) and np.array_equal(y0, y1)      # (the trained model's scores, bit for bit)


# ---- fit_stepping: the default never reaches set_optimizer -------------------------------------------------------------------------------
class _StubProblem:
    def __init__(self):
        self.calls, self.theta0 = [], "theta0"

    def set_optimizer(self, optimizer):
        self.calls.append(("set_optimizer", optimizer))
        self.theta0 = None

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
        return np.array([0.0, 1.5, 0.0, -2.0]), {"fval": 1.0, "nit": 1, "nfev": 2, "status": 0, "nhv": 0}

    def stage_result(self, theta, info, l2, threshold):
        return theta, info


def _stub_fit(monkeypatch, **kw):
    monkeypatch.setattr(fe, "_SteppingFit", _StubFit)
    s = fe.FixedEffectDeviceSolver(solver=types.SimpleNamespace())
    theta, info = s.fit_stepping(np.array([0, 1]), np.array([0]), np.array([1.0], np.float32), np.array([1.0], np.float32), 3, **kw)
    return info, _StubFit.last.prob.calls


def test_under_the_default_a_stubbed_problem_never_sees_set_optimizer(monkeypatch):
    info, calls = _stub_fit(monkeypatch)
    assert calls == [("run",), ("close",)] and info["optimizer"] == "LBFGS"
    info, calls = _stub_fit(monkeypatch, optimizer="lbfgs")
    assert calls == [("run",), ("close",)] and info["optimizer"] == "LBFGS"
    info, calls = _stub_fit(monkeypatch, optimizer="tron")      # set_optimizer leaves the problem at zeros: the start point is put back behind it
    assert calls == [("set_optimizer", "TRON"), ("restart", "theta0"), ("run",), ("close",)] and info["optimizer"] == "TRON"


def test_fit_stepping_refuses_an_unknown_optimizer_and_what_does_not_compose(monkeypatch):
    with pytest.raises(ValueError, match="optimizer"):
        _stub_fit(monkeypatch, optimizer="OWLQN")
    with pytest.raises(ValueError, match="L1 term"):
        _stub_fit(monkeypatch, optimizer="TRON", l1=1.0)
    with pytest.raises(ValueError, match="prior"):
        _stub_fit(monkeypatch, optimizer="TRON", prior=(np.zeros(4), np.ones(4)))
    with pytest.raises(ValueError, match="normalisation"):
        _stub_fit(monkeypatch, optimizer="TRON", feature_scale=np.ones(3))


# ---- the restatement against the reference ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", H.SIZES)
@pytest.mark.parametrize("loss", H.LOSSES)
def test_the_restatement_finds_the_reference_minimiser(loss, size):
    pb = H.problem(loss, size)
    theta_ref, f_ref = H.reference(loss, size)
    x, f, status, nit, nfev, nhv, rejected = H.tron(pb, max_iter=H.FIT["max_iter"], ftol=H.FIT["tolerance"])
    print(f"{loss} {size}: restatement status {status} nit {nit} nfev {nfev} nhv {nhv} rejected {rejected}")
    assert status == 0 and 6 <= nit <= 15 and nfev == nit + 1 + rejected
    assert np.max(np.abs(pb.smooth(x)[1])) <= H.PGTOL
    H.check_against_reference(pb, x, f, theta_ref, f_ref, f"{loss} {size}")


def test_the_product_against_a_finite_difference_of_the_gradient():
    """hv() is what the device's product is held to: it is itself held to the gradient it is the derivative of."""
    rng = np.random.default_rng(3)
    for loss in H.LOSSES:
        pb = H.problem(loss, "small")
        theta, v = 0.3 * rng.standard_normal(pb.X.shape[1]), rng.standard_normal(pb.X.shape[1])
        eps = 1e-6
        fd = (pb.data(theta + eps * v)[1] - pb.data(theta - eps * v)[1]) / (2 * eps)
        got = H.hv(pb, theta, v)
        assert np.max(np.abs(got - fd)) <= 1e-6 * np.max(np.abs(got)), loss


def test_the_rejecting_case_rejects_what_the_helper_states():
    theta0, rejected = H.rejecting_case()
    assert rejected == H.REJECTING["rejected"] >= 1 and np.linalg.norm(theta0) > 10.0


def test_the_stops_of_the_restatement():
    pb = H.problem("logistic", "small")
    theta_ref, _ = H.reference("logistic", "small")
    assert H.tron(pb, max_iter=2)[2:5] == (2, 2, 3)
    assert H.tron(pb, theta0=theta_ref)[2:6] == (0, 0, 1, 0)
    assert H.tron(pb, maxfun=3)[2] == 3
