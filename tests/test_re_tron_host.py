"""--entity_optimizer of the random-effect stage on the host (gdmix_amd/params.py, fe_model.py, model.py, chain.py, solver.EXPORTED_SYMBOLS,
include/gdmix_re.h): the flag, what it refuses and where it is ignored, the stage left alone without it, the argument checks of
gdmix_re_solve_tron that need no device, and the tests' own statement (tests/re_tron_helpers.py) against the algorithm-independent
reference on every case the GPU tests run. None of it needs a device."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from gdmix_amd import chain
from gdmix_amd import gdmix as cli
from gdmix_amd import model as model_mod
from gdmix_amd import solver
from gdmix_amd.fe_model import FixedLRParams
from gdmix_amd.params import REParams
from helpers import OracleSolverDouble, _Arr
import re_l1_helpers as R
import re_linear_helpers as H
import re_tron_helpers as T

BASE = ["--metadata_file=m.json", "--output_model_dir=out"]
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the flag ------------------------------------------------------------------------------------------------------------------------
def test_the_flag_parses_in_any_case_with_its_default():
    for text in ("TRON", "tron", "Tron"):
        p = REParams.__from_argv__(BASE + [f"--entity_optimizer={text}"])
        assert p.entity_optimizer == "TRON" and p.entity_tron()
        assert REParams.__from_argv__(p.__to_argv__()) == p
    for text in ("LBFGS", "lbfgs"):
        p = REParams.__from_argv__(BASE + ["--entity_optimizer", text])
        assert p.entity_optimizer == "LBFGS" and not p.entity_tron()
    p = REParams.__from_argv__(BASE)
    assert p.entity_optimizer is None and not p.entity_tron()


@pytest.mark.parametrize("bad", ["NEWTON", "OWLQN", "TRON2"])
def test_another_optimiser_is_refused_at_parse_time(bad):
    with pytest.raises(ValueError, match="entity_optimizer"):
        REParams.__from_argv__(BASE + [f"--entity_optimizer={bad}"])


OTHERS = [["--elastic_net_alpha=0.5"], ["--entity_coefficient_constraints=c.json", "--feature_file=f", "--feature_bag=b"], ["--incremental_training=True"],
          ["--feature_normalization=scale_with_standard_deviation"], ["--feature_normalization=scale_with_max_magnitude"], ["--rebalance_entities=True"],
          ["--l2_reg_weights=1,0.1", "--validation_data_dir=v", "--metric_output_dir=m"]]


@pytest.mark.parametrize("other", OTHERS, ids=lambda o: o[0].split("=")[0])
def test_each_refusal_names_both_flags_and_lbfgs_runs_with_all_of_them(other):
    with pytest.raises(ValueError) as e:
        REParams.__from_argv__(BASE + ["--entity_optimizer=TRON"] + other)
    assert "--entity_optimizer" in str(e.value) and other[0].split("=")[0] in str(e.value)
    assert REParams.__from_argv__(BASE + ["--entity_optimizer=LBFGS"] + other).entity_optimizer == "LBFGS"
    assert REParams.__from_argv__(BASE + other).entity_optimizer is None


def test_what_tron_runs_with():
    p = REParams.__from_argv__(BASE + ["--entity_optimizer=TRON", "--random_effect_variance_mode=full", "--metric_output_dir=m", "--partition_entity=user_id",
                                       "--evaluators=AUC:user_id", "--active_data_upper_bound=10", "--features_to_samples_ratio=0.5",
                                       "--feature_normalization=none", "--elastic_net_alpha=0"])
    assert p.entity_tron()


def test_the_fixed_effects_flag_is_still_refused_by_the_random_effect():
    with pytest.raises(ValueError, match="L-BFGS-B only"):
        REParams.__from_argv__(BASE + ["--optimizer=TRON"])
    with pytest.raises(ValueError, match="L-BFGS-B only"):
        REParams.__from_argv__(BASE + ["--optimizer=TRON", "--entity_optimizer=TRON"])


def test_the_fixed_effect_refuses_the_new_flag():
    with pytest.raises(ValueError) as e:
        FixedLRParams.__from_argv__(BASE + ["--entity_optimizer=TRON"])
    assert "--entity_optimizer" in str(e.value) and "--optimizer" in str(e.value)
    assert FixedLRParams.__from_argv__(BASE + ["--entity_optimizer=LBFGS"]).optimizer == "LBFGS"
    assert FixedLRParams.__from_argv__(BASE).entity_optimizer is None


def test_the_chain_hands_the_flag_to_the_random_effect_stages_only():
    for stage in chain.STAGES:
        plain = chain.stage_argv("/r", stage)
        flagged = chain.stage_argv("/r", stage, entity_optimizer="TRON")
        assert not any(a.startswith("--entity_optimizer") for a in plain)
        if stage == "global":
            assert flagged == plain
        else:
            assert [a for a in flagged if a not in plain] == ["--entity_optimizer=TRON"]


# ---- the library -----------------------------------------------------------------------------------------------------------------------
NEW_SYMBOLS = ("gdmix_re_solve_tron", "gdmix_re_solve_tron_scratch_bytes")


def test_the_symbols_are_declared_and_exported():
    with open(os.path.join(ROOT, "include", "gdmix_re.h")) as f:
        text = f.read()
    declared = set(re.findall(r"GDMIX_API[^;(]*?(gdmix_\w+)\s*\(", text))
    for name in NEW_SYMBOLS:
        assert name in solver.EXPORTED_SYMBOLS and name in declared
    assert "#define GDMIX_RE_ABI_VERSION 27" in text


@pytest.fixture(scope="module")
def lib():
    from gdmix_amd import build
    build.build_library()
    return solver.load_library()


def test_argument_checks_need_no_device(lib):
    """An empty batch returns 0 right behind the argument checks; sum_loss, a bad loss code and a NULL batch are GDMIX_RE_EINVAL. The
    context is never looked into before those checks, so a stand-in pointer will do."""
    ctx = C.cast(C.create_string_buffer(64), C.c_void_p)
    packed, res = solver._Packed(), solver._Result()      # E = 0
    opts = solver.SolverOptions().to_c()
    call = lambda o: lib.gdmix_re_solve_tron(ctx, C.byref(packed), C.byref(o), None, C.byref(res), None, None)
    assert call(opts) == 0
    summed = solver.SolverOptions(sum_loss=True).to_c()
    assert call(summed) == -1 and b"sum_loss" in lib.gdmix_re_last_error() and b"gdmix_fe_set_optimizer" in lib.gdmix_re_last_error()
    bad_loss = solver.SolverOptions().to_c()
    bad_loss.loss = 3
    assert call(bad_loss) == -1
    assert lib.gdmix_re_solve_tron(ctx, None, C.byref(opts), None, C.byref(res), None, None) == -1
    assert lib.gdmix_re_solve_tron(None, C.byref(packed), C.byref(opts), None, C.byref(res), None, None) == -1
    assert lib.gdmix_re_solve_tron_scratch_bytes(C.byref(packed), C.byref(opts)) == 0
    assert lib.gdmix_re_abi_version() == 27


# ---- the stage, with a solver stand-in ----------------------------------------------------------------------------------------------------
class RecordingSolver(OracleSolverDouble):
    """The oracle stand-in of tests/test_host.py; records which of solve() and solve_tron() the stage called (both solve the plain problem:
    what is tested here is what reaches the solver, the TRON solve itself is tested on the GPU)."""
    seen = []

    def __init__(self, device=0):
        pass

    def solve(self, packed, opts, theta0=None, out=None, **kw):
        type(self).seen.append(("solve", dict(kw), theta0 is not None))
        return super().solve(packed, opts, theta0=theta0, out=out)

    def solve_tron(self, packed, opts, theta0=None, out=None):
        type(self).seen.append(("solve_tron", {}, theta0 is not None))
        solved = super().solve(packed, opts, theta0=theta0, out=out)
        solved.nhv = _Arr(np.zeros(packed.E, np.int32))
        return solved

    def close(self):
        pass


@pytest.fixture
def stand_in(monkeypatch):
    RecordingSolver.seen = []
    monkeypatch.setattr(model_mod, "REDeviceSolver", RecordingSolver)
    monkeypatch.delenv("TF_CONFIG", raising=False)
    monkeypatch.setenv("GDMIX_PARTITIONS_PER_BATCH", "1")
    return RecordingSolver


def _job(tmp_path):
    b = H.small_job_batch(E=12, seed=42, real=False)
    H.write_job(str(tmp_path), b)
    return b


@pytest.mark.parametrize("extra", [[], ["--entity_optimizer=LBFGS"], ["--entity_optimizer=lbfgs"]])
def test_the_default_never_reaches_solve_tron(tmp_path, stand_in, extra):
    _job(tmp_path)
    cli.run(H.job_argv(str(tmp_path), model_type="logistic_regression", extra=extra))
    assert stand_in.seen and all(call == ("solve", {}, False) for call in stand_in.seen)


def test_the_flag_sends_the_stage_through_solve_tron_and_logs_the_counts(tmp_path, stand_in, caplog):
    _job(tmp_path)
    argv = H.job_argv(str(tmp_path), model_type="logistic_regression", extra=["--entity_optimizer=tron"])
    with caplog.at_level("INFO"):
        cli.run(argv)
    assert [c[0] for c in stand_in.seen] == ["solve_tron"] and not stand_in.seen[0][2]
    assert any("evaluations" in r.getMessage() and "Hessian-vector" in r.getMessage() and "status 0" in r.getMessage() for r in caplog.records)
    cli.run(argv)      # the model of the first run is in output_model_dir: a warm start
    assert [(c[0], c[2]) for c in stand_in.seen] == [("solve_tron", False), ("solve_tron", True)]


def test_inference_accepts_the_flag_and_ignores_it(tmp_path, stand_in):
    _job(tmp_path)
    cli.run(H.job_argv(str(tmp_path), model_type="logistic_regression"))
    n = len(stand_in.seen)
    cli.run(H.job_argv(str(tmp_path), action="inference", model_type="logistic_regression"))
    plain = chain.read_scores(os.path.join(str(tmp_path), "inferenceScores"))
    cli.run(H.job_argv(str(tmp_path), action="inference", model_type="logistic_regression", extra=["--entity_optimizer=TRON"]))
    flagged = chain.read_scores(os.path.join(str(tmp_path), "inferenceScores"))
    assert len(stand_in.seen) == n      # no solve
    for a, b in zip(plain, flagged):
        assert np.array_equal(np.asarray(a), np.asarray(b))


# ---- the statement ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", ["weights", "free_intercept", "no_intercept"])
@pytest.mark.parametrize("loss", T.LOSSES)
def test_the_product_is_the_derivative_of_the_gradient(loss, variant):
    """H v of the restatement's view (weights and the 1/n in the transposed matrix) against a central difference of the numpy gradient."""
    pbs, _, _, b, v = T.case(loss, variant, "mixed")
    rng = np.random.default_rng(5)
    worst = 0.0
    for e in (3, 4, 5, 10):
        pb = pbs[e]
        p = pb.X.shape[1]
        th, d = 0.3 * rng.standard_normal(p), rng.standard_normal(p)
        h = 1e-5
        fd = (pb.smooth(th + h * d)[1] - pb.smooth(th - h * d)[1]) / (2.0 * h)
        hv = T.product(pb, th, d)
        worst = max(worst, np.max(np.abs(fd - hv)) / max(np.max(np.abs(hv)), 1e-300))
    print(f"{loss} {variant}: worst |finite difference - H v| / |H v|_inf {worst:.3e}")
    assert worst <= 1e-7      # the difference quotient's own truncation and cancellation: h^2 |f''''| + eps / h


def _cases():
    for loss in T.LOSSES:
        for variant in T.VARIANTS:
            yield loss, variant, "mixed"
        yield loss, "plain", "block"


@pytest.mark.parametrize("loss,variant,which", list(_cases()), ids=lambda v: str(v))
def test_the_restatement_against_the_reference_and_its_strict_share(loss, variant, which):
    """The check that the inputs, not the device, keep within the bars: the restatement's own fits, put through compare() in the device's
    place, meet every bar on every entity the GPU tests compare (n from 1, p from 1 to more than 64 and, in the block case, more than 256),
    and at least half of them are strict. The share is printed."""
    pbs, refs, rest, b, v = T.case(loss, variant, which)
    cp = R.coef_ptr(b, v["has_intercept"])
    P = int(cp[-1])
    res = dict(theta=np.zeros(P), theta_thr=np.zeros(P), fval=np.zeros(b.E), gnorm=np.zeros(b.E), status=np.zeros(b.E, int), nit=np.zeros(b.E, int),
               nfev=np.zeros(b.E, int), nhv=np.zeros(b.E, int))
    for e, r in rest.items():
        th, f, status, nit, nfev, nhv, _ = r["fit"]
        s = slice(int(cp[e]), int(cp[e + 1]))
        res["theta"][s], res["theta_thr"][s] = th, np.where(np.abs(th) <= T.THRESHOLD, 0.0, th)
        res["fval"][e], res["status"][e], res["nit"][e], res["nfev"][e], res["nhv"][e] = f, status, nit, nfev, nhv
        res["gnorm"][e] = np.max(np.abs(pbs[e].smooth(th)[1]))
    out = T.compare(res, pbs, rest, refs, cp, distance=v["distance"], what=f"restatement {loss} {variant} {which}")
    assert out["share"] >= T.MIN_STRICT_SHARE


def test_the_footprint_is_the_plain_kernels_without_history_plus_two_and_two():
    assert T.lds_bytes(p=3, n=2, nnz=4, d=2, has_w=False) == (((7 * 3 + 3 * 2) * 8 + (16 + 3 + 3 + 4) * 4 + 15) & ~15)
    assert T.lds_bytes(4, 2, 5, 3, False) - T.lds_bytes(4, 2, 4, 3, False) == 16      # one non-zero more: four 4-byte entries
    # half of OWL-QN's for a mean C2 entity (16 samples, ~64 coefficients, ~6 non-zeros per sample)
    assert 2 * T.lds_bytes(65, 16, 96, 64, False) < R.lds_bytes(65, 16, 96, 64, 10, False)
