"""--elastic_net_alpha of the random-effect stage on the host (gdmix_amd/params.py, model.py, solver.EXPORTED_SYMBOLS, include/gdmix_re.h): the
flag, what it refuses and where it is ignored, the stage left alone without it, the argument checks of gdmix_re_solve_l1 that need no
device, and the tests' own statement (tests/re_l1_helpers.py) against the algorithm-independent reference on every case the GPU tests
run. None of it needs a device."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from gdmix_amd import gdmix as cli
from gdmix_amd import model as model_mod
from gdmix_amd import params, solver
from gdmix_amd.params import REParams
from helpers import OracleSolverDouble
import fe_l1_helpers as F
import re_l1_helpers as R
import re_linear_helpers as H

BASE = ["--metadata_file=m.json", "--output_model_dir=out"]
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the flag ------------------------------------------------------------------------------------------------------------------------
def test_the_flag_parses_with_its_default_and_range():
    p = REParams.__from_argv__(BASE + ["--elastic_net_alpha=0.5"])
    assert p.elastic_net_alpha == 0.5 and isinstance(p.elastic_net_alpha, float)
    assert REParams.__from_argv__(p.__to_argv__()) == p
    assert REParams.__from_argv__(BASE).elastic_net_alpha is None
    for text, want in (("0", 0.0), ("1", 1.0), ("0.25", 0.25)):
        assert REParams.__from_argv__(BASE + ["--elastic_net_alpha", text]).elastic_net_alpha == want


@pytest.mark.parametrize("bad", ["nan", "-0.1", "1.5", "inf"])
def test_a_bad_alpha_is_refused_at_parse_time(bad):
    with pytest.raises(ValueError, match="elastic_net_alpha"):
        REParams.__from_argv__(BASE + [f"--elastic_net_alpha={bad}"])


OTHERS = ["--incremental_training=True", "--feature_normalization=scale_with_standard_deviation", "--feature_normalization=scale_with_max_magnitude",
          "--rebalance_entities=True"]


@pytest.mark.parametrize("other", OTHERS)
def test_each_refusal_names_both_flags_and_alpha_zero_is_todays_behaviour(other):
    with pytest.raises(ValueError) as e:
        REParams.__from_argv__(BASE + ["--elastic_net_alpha=0.5", other])
    assert "--elastic_net_alpha" in str(e.value) and other.split("=")[0] in str(e.value)
    without = REParams.__from_argv__(BASE + [other])
    with_zero = REParams.__from_argv__(BASE + ["--elastic_net_alpha=0", other])
    assert with_zero.elastic_net_alpha == 0.0 and with_zero.elastic_net() == without.elastic_net() == (0.0, 1.0)
    assert REParams.__from_argv__(BASE + ["--elastic_net_alpha=0.5", "--feature_normalization=none"]).elastic_net_alpha == 0.5


def test_the_sweep_is_refused_and_names_both_flags():
    sweep = ["--l2_reg_weights=1,0.1", "--validation_data_dir=v", "--metric_output_dir=m"]
    with pytest.raises(ValueError) as e:
        REParams.__from_argv__(BASE + ["--elastic_net_alpha=0.5"] + sweep)
    assert "--elastic_net_alpha" in str(e.value) and "--l2_reg_weights" in str(e.value)
    assert REParams.__from_argv__(BASE + ["--elastic_net_alpha=0"] + sweep).l2_grid() == (1.0, 0.1)


def test_the_other_flags_it_runs_with():
    p = REParams.__from_argv__(BASE + ["--elastic_net_alpha=0.5", "--random_effect_variance_mode=full", "--metric_output_dir=m", "--partition_entity=user_id",
                                       "--evaluators=AUC:user_id", "--active_data_upper_bound=10", "--features_to_samples_ratio=0.5"])
    assert p.elastic_net_alpha == 0.5


def test_the_fixed_effects_flag_is_still_refused():
    with pytest.raises(ValueError, match="random effect has no L1 term"):
        REParams.__from_argv__(BASE + ["--l1_reg_weight=0.5", "--elastic_net_alpha=0.5"])


def test_the_conversion():
    assert params.elastic_net_weights(0.5, 1.0) == (0.5, 0.5)
    assert params.elastic_net_weights(0.25, 8.0) == (2.0, 6.0)
    assert params.elastic_net_weights(1.0, 3.0) == (3.0, 0.0)
    p = REParams.__from_argv__(BASE + ["--elastic_net_alpha=0.25", "--l2_reg_weight=8"])
    assert p.elastic_net() == (2.0, 6.0)
    # from the fixed effect's (l1, l2): lambda = l1 + l2, alpha = l1 / (l1 + l2)
    l1, l2 = 3.0, 1.0
    assert params.elastic_net_weights(l1 / (l1 + l2), l1 + l2) == (l1, l2)
    assert REParams.__from_argv__(BASE + ["--l2_reg_weight=0.75"]).elastic_net() == (0.0, 0.75)


# ---- the library -----------------------------------------------------------------------------------------------------------------------
NEW_SYMBOLS = ("gdmix_re_solve_l1", "gdmix_re_solve_l1_scratch_bytes")


def test_the_symbols_are_declared_and_exported():
    with open(os.path.join(ROOT, "include", "gdmix_re.h")) as f:
        declared = set(re.findall(r"GDMIX_API[^;(]*?(gdmix_\w+)\s*\(", f.read()))
    for name in NEW_SYMBOLS:
        assert name in solver.EXPORTED_SYMBOLS and name in declared
    assert "#define GDMIX_RE_ABI_VERSION 27" in open(os.path.join(ROOT, "include", "gdmix_re.h")).read()


@pytest.fixture(scope="module")
def lib():
    from gdmix_amd import build
    build.build_library()
    return solver.load_library()


def test_argument_checks_need_no_device(lib):
    """An empty batch returns 0 right behind the argument checks; a bad l1 and sum_loss are GDMIX_RE_EINVAL with their messages. The context
    is never looked into before those checks, so a stand-in pointer will do."""
    ctx = C.create_string_buffer(64)
    packed, res = solver._Packed(), solver._Result()      # E = 0
    opts = solver.SolverOptions().to_c()
    call = lambda o, l1: lib.gdmix_re_solve_l1(C.cast(ctx, C.c_void_p), C.byref(packed), C.byref(o), l1, None, C.byref(res), None)
    assert call(opts, 0.5) == 0 and call(opts, 0.0) == 0
    for bad in (-0.5, float("nan"), float("inf")):
        assert call(opts, bad) == -1 and b"l1 must be finite and >= 0" in lib.gdmix_re_last_error()
    summed = solver.SolverOptions(sum_loss=True).to_c()
    assert call(summed, 0.5) == -1 and b"sum_loss" in lib.gdmix_re_last_error()
    bad_loss = solver.SolverOptions().to_c()
    bad_loss.loss = 3
    assert call(bad_loss, 0.5) == -1
    assert lib.gdmix_re_solve_l1(None, C.byref(packed), C.byref(opts), 0.5, None, C.byref(res), None) == -1
    assert lib.gdmix_re_solve_l1_scratch_bytes(C.byref(packed), C.byref(opts)) == 0
    assert lib.gdmix_re_abi_version() == 27


# ---- the stage, with a solver stand-in ----------------------------------------------------------------------------------------------------
class RecordingSolver(OracleSolverDouble):
    """The oracle stand-in of tests/test_host.py; records how solve() was called (it solves the plain problem whatever l1 is: what is
    tested here is what reaches the solver, the elastic-net solve itself is tested on the GPU)."""
    seen = []

    def __init__(self, device=0):
        pass

    def solve(self, packed, opts, theta0=None, out=None, **kw):
        type(self).seen.append((dict(kw), float(opts.l2), theta0 is not None))
        return super().solve(packed, opts, theta0=theta0, out=out)

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


def test_the_stage_passes_l1_and_the_reduced_l2(tmp_path, stand_in, caplog):
    _job(tmp_path)
    with caplog.at_level("INFO"):
        cli.run(H.job_argv(str(tmp_path), model_type="logistic_regression", extra=["--elastic_net_alpha=0.25", "--l2_reg_weight=2.0"]))
    assert stand_in.seen and all(kw == {"l1": 0.5} and l2 == 1.5 for kw, l2, _ in stand_in.seen)
    assert any("coefficients" in r.getMessage() and "non-zero" in r.getMessage() for r in caplog.records)


@pytest.mark.parametrize("extra", [[], ["--elastic_net_alpha=0"]])
def test_without_the_flag_the_solver_is_called_as_before(tmp_path, stand_in, extra):
    _job(tmp_path)
    cli.run(H.job_argv(str(tmp_path), model_type="logistic_regression", extra=extra))
    assert stand_in.seen and all(kw == {} and l2 == 1.0 for kw, l2, _ in stand_in.seen)


def test_a_second_run_starts_from_the_first_runs_model(tmp_path, stand_in):
    _job(tmp_path)
    argv = H.job_argv(str(tmp_path), model_type="logistic_regression", extra=["--elastic_net_alpha=0.5"])
    cli.run(argv)
    assert [warm for _, _, warm in stand_in.seen] == [False]
    cli.run(argv)
    assert [warm for _, _, warm in stand_in.seen] == [False, True]


def test_inference_accepts_the_flag_and_ignores_it(tmp_path, stand_in):
    _job(tmp_path)
    cli.run(H.job_argv(str(tmp_path), model_type="logistic_regression"))
    n = len(stand_in.seen)
    from gdmix_amd import chain
    cli.run(H.job_argv(str(tmp_path), action="inference", model_type="logistic_regression"))
    plain = chain.read_scores(os.path.join(str(tmp_path), "inferenceScores"))
    cli.run(H.job_argv(str(tmp_path), action="inference", model_type="logistic_regression", extra=["--elastic_net_alpha=0.5"]))
    flagged = chain.read_scores(os.path.join(str(tmp_path), "inferenceScores"))
    assert len(stand_in.seen) == n      # no solve
    for a, b in zip(plain, flagged):
        assert np.array_equal(np.asarray(a), np.asarray(b))


# ---- the statement ------------------------------------------------------------------------------------------------------------------------
def test_the_unweighted_problem_is_the_fixed_effects_divided_by_n():
    b = R.mixed_batch("poisson", "plain")
    pb = R.entity_problem(b, 3, "poisson", R.L1, R.L2)
    base = F.Problem("poisson", pb.X, pb.y, pb.off, R.L1, R.L2)
    th = 0.1 * np.random.default_rng(0).standard_normal(pb.X.shape[1])
    assert np.isclose(pb.F(th), base.F(th) / pb.n, rtol=1e-14)
    assert np.allclose(pb.pseudo_gradient(th), base.pseudo_gradient(th) / pb.n, rtol=1e-13, atol=0)
    assert pb.mask[0] == 1.0 and np.all(pb.X[:, 0].toarray() == 1.0)      # the intercept is coefficient 0
    free = R.entity_problem(b, 3, "poisson", R.L1, R.L2, regularize_bias=False)
    assert free.mask[0] == 0.0 and free.mask[1:].all()
    ones = R.EntityProblem("poisson", pb.X, pb.y, pb.off, np.ones(pb.n), R.L1, R.L2)
    assert np.isclose(ones.F(th), pb.F(th), rtol=1e-14) and np.allclose(ones.smooth(th)[1], pb.smooth(th)[1], rtol=1e-13)


def _cases():
    for loss in R.LOSSES:
        for variant in R.VARIANTS:
            yield loss, variant, "mixed"
        yield loss, "plain", "block"


@pytest.mark.parametrize("loss,variant,which", list(_cases()), ids=lambda v: str(v))
def test_the_restatement_stays_within_the_bars_on_every_committed_case(loss, variant, which):
    """The check that the inputs, not the device, keep within the bars: with the tests' tolerances (R.TIGHT) the restatement alone ends at
    most 1e-10 |F_ref| above the reference on every entity the GPU tests compare, meets every bar of check_batch, and the reference alone
    meets the cap on left-out coefficients."""
    pbs, refs, b, v = R.case(loss, variant, which)
    R.check_left_out_cap(pbs, refs)
    cp = R.coef_ptr(b, v["has_intercept"])
    theta, fval = np.zeros(int(cp[-1])), np.zeros(b.E)
    worst = -np.inf
    for e, pb in pbs.items():
        th, Fv, status, nit, nfev = R.restatement(pb)
        theta[int(cp[e]):int(cp[e + 1])], fval[e] = th, Fv
        worst = max(worst, (Fv - refs[e][1]) / abs(refs[e][1]))
        assert status in (0, 1), (e, status)
    print(f"{loss} {variant} {which}: the restatement ends at most {worst:.3e} |F_ref| above the reference")
    assert worst <= R.RESTATEMENT_BAR
    R.check_batch(pbs, refs, theta, fval, cp, distance=v["distance"], what=f"restatement {loss} {variant} {which}")


@pytest.mark.parametrize("loss", R.LOSSES)
def test_the_one_iteration_cases_excuse_few_entities(loss):
    """max_iter = 1 from a cold start and from half the reference: at most 1 % of the entities have an Armijo test within 1e-10 max(|F|, 1)
    of its edge (the GPU test excuses exactly those from equal counts)."""
    pbs, refs, b, v = R.case(loss, "plain", "mixed")
    for warm in (False, True):
        one = R.one_iteration(loss, warm)
        excused = [e for e, r in one.items() if not r[4] > R.ARMIJO_MARGIN]
        print(f"{loss} warm={warm}: {len(excused)} of {len(one)} entities excused")
        assert len(excused) <= R.MAX_EXCUSED_SHARE * len(one)
        assert all(r[1] <= 1 for r in one.values())


def test_the_footprint_is_the_plain_kernels_plus_one_vector():
    assert R.lds_bytes(p=3, n=2, nnz=4, d=2, m=10, has_w=False) == ((25 * 3 + 2 + 20) * 8 + (16 + 3 + 3 + 4) * 4 + 15 & ~15) + 32
    assert R.lds_bytes(4, 2, 5, 3, 10, False) - R.lds_bytes(4, 2, 4, 3, 10, False) == 16      # one non-zero more: four 4-byte entries
