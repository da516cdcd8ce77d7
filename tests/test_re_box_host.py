"""--entity_coefficient_constraints of the random-effect stage on the host (gdmix_amd/params.py, model.py, solver.EXPORTED_SYMBOLS,
include/gdmix_re.h): the flag, what it refuses and where it is ignored, the stage left alone without it, the argument checks of
gdmix_re_solve_box that need no device, and the tests' own statement (tests/re_box_helpers.py) against the algorithm-independent reference
on every case the GPU tests run. None of it needs a device."""
import ctypes as C
import json
import os
import re

import numpy as np
import pytest

from gdmix_amd import gdmix as cli
from gdmix_amd import model as model_mod
from gdmix_amd import params, solver
from gdmix_amd.params import REParams
from helpers import OracleSolverDouble
import re_box_helpers as B
import re_l1_helpers as R
import re_linear_helpers as H

BASE = ["--metadata_file=m.json", "--output_model_dir=out", "--feature_file=f", "--feature_bag=per_user"]
FLAG = "--entity_coefficient_constraints"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the flag ------------------------------------------------------------------------------------------------------------------------
def test_the_flag_parses_and_is_absent_by_default():
    p = REParams.__from_argv__(BASE + [f"{FLAG}=c.json"])
    assert p.entity_coefficient_constraints == "c.json"
    assert REParams.__from_argv__(p.__to_argv__()) == p
    assert REParams.__from_argv__(BASE).entity_coefficient_constraints is None


OTHERS = ["--elastic_net_alpha=0.5", "--incremental_training=True", "--feature_normalization=scale_with_standard_deviation",
          "--feature_normalization=scale_with_max_magnitude", "--rebalance_entities=True"]


@pytest.mark.parametrize("other", OTHERS)
def test_each_refusal_names_both_flags(other):
    with pytest.raises(ValueError) as e:
        REParams.__from_argv__(BASE + [f"{FLAG}=c.json", other])
    assert FLAG in str(e.value) and other.split("=")[0] in str(e.value)
    REParams.__from_argv__(BASE + [other])      # the other flag alone is fine


def test_the_sweep_is_refused_and_names_both_flags():
    sweep = ["--l2_reg_weights=1,0.1", "--validation_data_dir=v", "--metric_output_dir=m"]
    with pytest.raises(ValueError) as e:
        REParams.__from_argv__(BASE + [f"{FLAG}=c.json"] + sweep)
    assert FLAG in str(e.value) and "--l2_reg_weights" in str(e.value)


@pytest.mark.parametrize("missing", ["--feature_file=f", "--feature_bag=per_user"])
def test_the_flag_needs_the_feature_file_and_the_bag(missing):
    with pytest.raises(ValueError, match="--feature_file and --feature_bag"):
        REParams.__from_argv__([a for a in BASE if a != missing] + [f"{FLAG}=c.json"])


def test_what_it_runs_with():
    p = REParams.__from_argv__(BASE + [f"{FLAG}=c.json", "--random_effect_variance_mode=full", "--metric_output_dir=m", "--partition_entity=user_id",
                                       "--evaluators=AUC:user_id", "--active_data_upper_bound=10", "--features_to_samples_ratio=0.5",
                                       "--elastic_net_alpha=0", "--feature_normalization=none"])
    assert p.entity_coefficient_constraints == "c.json"


def test_the_fixed_effects_flag_is_still_refused():
    with pytest.raises(ValueError, match="random effect has no box constraints"):
        REParams.__from_argv__(BASE + ["--coefficient_constraints=c.json", f"{FLAG}=c.json"])


def test_the_file_is_the_fixed_effects_format_under_this_flags_name(tmp_path):
    feats = [("a", ""), ("a", "t"), ("b", "")]
    path = tmp_path / "c.json"
    path.write_text(json.dumps([{"name": "a", "term": "*", "lowerBound": 0}, {"name": "b", "term": "", "lowerBound": -1, "upperBound": 1}]))
    lo, hi = params.read_coefficient_constraints(str(path), feats, False, flag=FLAG)
    assert lo.tolist() == [0.0, 0.0, -1.0] and hi.tolist() == [np.inf, np.inf, 1.0]
    path.write_text(json.dumps([{"name": "nobody", "term": "", "lowerBound": 0}]))
    with pytest.raises(ValueError, match=f"{FLAG}={re.escape(str(path))}.*matches no feature"):
        params.read_coefficient_constraints(str(path), feats, False, flag=FLAG)
    with pytest.raises(ValueError, match=f"^--coefficient_constraints={re.escape(str(path))}"):      # the default names the fixed effect's flag
        params.read_coefficient_constraints(str(path), feats, False)
    path.write_text('[{"name": "a", "term": "", "lowerBound": NaN}]')
    with pytest.raises(ValueError, match=f"{FLAG}=.*not a finite number"):
        params.read_coefficient_constraints(str(path), feats, False, flag=FLAG)


# ---- the library -----------------------------------------------------------------------------------------------------------------------
NEW_SYMBOLS = ("gdmix_re_solve_box", "gdmix_re_solve_box_scratch_bytes")


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
    """An empty batch returns 0 right behind the argument checks; sum_loss, a loss code outside the three and a negative table length are
    GDMIX_RE_EINVAL. The context is never looked into before those checks, so a stand-in pointer will do (the tables are never read on
    the host: any non-NULL pointer stands for one)."""
    ctx = C.create_string_buffer(64)
    table = C.cast(C.create_string_buffer(64), C.c_void_p)
    packed, res = solver._Packed(), solver._Result()      # E = 0
    opts = solver.SolverOptions().to_c()
    call = lambda o, lo=table, hi=table, n=8: lib.gdmix_re_solve_box(C.cast(ctx, C.c_void_p), C.byref(packed), C.byref(o), lo, hi, n, None, C.byref(res), None)
    assert call(opts) == 0 and call(opts, hi=None) == 0 and call(opts, lo=None) == 0
    assert call(opts, None, None) == 0      # both NULL: the plain solve's own empty batch
    assert call(opts, n=-1) == -1 and b"num_features" in lib.gdmix_re_last_error()
    summed = solver.SolverOptions(sum_loss=True).to_c()
    assert call(summed) == -1 and b"sum_loss" in lib.gdmix_re_last_error()
    bad_loss = solver.SolverOptions().to_c()
    bad_loss.loss = 3
    assert call(bad_loss) == -1
    assert lib.gdmix_re_solve_box(None, C.byref(packed), C.byref(opts), table, table, 8, None, C.byref(res), None) == -1
    assert lib.gdmix_re_solve_box_scratch_bytes(C.byref(packed), C.byref(opts)) == 0
    assert lib.gdmix_re_abi_version() == 27


# ---- the stage, with a solver stand-in ----------------------------------------------------------------------------------------------------
class RecordingSolver(OracleSolverDouble):
    """The oracle stand-in of tests/test_host.py; records how solve() and upload_bounds() were called (it solves the plain problem whatever
    the bounds are: what is tested here is what reaches the solver, the bounded solve itself is tested on the GPU)."""
    seen, uploads = [], []

    def __init__(self, device=0):
        pass

    def upload_bounds(self, lower, upper):
        type(self).uploads.append((np.array(lower), np.array(upper)))
        return ("lower on the device", "upper on the device")

    def solve(self, packed, opts, theta0=None, out=None, **kw):
        type(self).seen.append((dict(kw), float(opts.l2), theta0 is not None))
        return super().solve(packed, opts, theta0=theta0, out=out)

    def close(self):
        pass


@pytest.fixture
def stand_in(monkeypatch):
    RecordingSolver.seen, RecordingSolver.uploads = [], []
    monkeypatch.setattr(model_mod, "REDeviceSolver", RecordingSolver)
    monkeypatch.delenv("TF_CONFIG", raising=False)
    monkeypatch.setenv("GDMIX_PARTITIONS_PER_BATCH", "1")
    return RecordingSolver


def _job(tmp_path, records=None):
    b = H.small_job_batch(E=12, seed=42, real=False)
    H.write_job(str(tmp_path), b)
    path = os.path.join(str(tmp_path), "constraints.json")
    with open(path, "w") as f:
        json.dump([{"name": "f0", "term": "", "lowerBound": 0.0}, {"name": "f3", "term": "", "lowerBound": -0.05, "upperBound": 0.05}] if records is None else records, f)
    return b, path


def test_the_stage_passes_the_tables_and_uploads_them_once(tmp_path, stand_in, caplog):
    b, path = _job(tmp_path)
    dim = int(b.col_global.max()) + 1
    with caplog.at_level("INFO"):
        cli.run(H.job_argv(str(tmp_path), model_type="logistic_regression", extra=[f"{FLAG}={path}"]))
    assert stand_in.seen and all(kw == {"bounds": ("lower on the device", "upper on the device")} and l2 == 1.0 for kw, l2, _ in stand_in.seen)
    assert len(stand_in.uploads) == 1
    lower, upper = stand_in.uploads[0]
    assert lower.shape == upper.shape == (dim,)      # by global feature id: no intercept slot
    want_lo, want_hi = np.full(dim, -np.inf), np.full(dim, np.inf)
    want_lo[0], want_lo[3], want_hi[3] = 0.0, -0.05, 0.05
    assert np.array_equal(lower, want_lo) and np.array_equal(upper, want_hi)
    assert any("entity_coefficient_constraints" in r.getMessage() and "equal a bound" in r.getMessage() for r in caplog.records)


def test_without_the_flag_the_solver_is_called_as_before(tmp_path, stand_in):
    _job(tmp_path)
    cli.run(H.job_argv(str(tmp_path), model_type="logistic_regression"))
    assert stand_in.seen and all(kw == {} and l2 == 1.0 for kw, l2, _ in stand_in.seen) and not stand_in.uploads


def test_a_list_of_another_length_than_the_bag_is_refused(tmp_path, stand_in):
    b, path = _job(tmp_path)
    with open(os.path.join(str(tmp_path), "partition", "featureList"), "a") as f:
        f.write("one_more,\n")
    with pytest.raises(ValueError, match="--entity_coefficient_constraints: --feature_file lists"):
        cli.run(H.job_argv(str(tmp_path), model_type="logistic_regression", extra=[f"{FLAG}={path}"]))


def test_inference_ignores_the_flag_and_a_missing_file(tmp_path, stand_in):
    _job(tmp_path)
    cli.run(H.job_argv(str(tmp_path), model_type="logistic_regression"))
    n = len(stand_in.seen)
    from gdmix_amd import chain
    cli.run(H.job_argv(str(tmp_path), action="inference", model_type="logistic_regression"))
    plain = chain.read_scores(os.path.join(str(tmp_path), "inferenceScores"))
    cli.run(H.job_argv(str(tmp_path), action="inference", model_type="logistic_regression", extra=[f"{FLAG}={tmp_path}/no_such_file.json"]))
    flagged = chain.read_scores(os.path.join(str(tmp_path), "inferenceScores"))
    assert len(stand_in.seen) == n and not stand_in.uploads      # no solve, no table
    for a, b in zip(plain, flagged):
        assert np.array_equal(np.asarray(a), np.asarray(b))


def test_descent_does_not_know_the_flag():
    with open(os.path.join(ROOT, "gdmix_amd", "descent.py")) as f:
        assert "entity_coefficient_constraints" not in f.read()


# ---- the statement ------------------------------------------------------------------------------------------------------------------------
def test_the_tables_bound_the_gathers_edges_and_hold_every_kind():
    lo, hi = B.bounds()
    assert lo.size == hi.size == B.D and np.isfinite(lo[0]) and np.isfinite(hi[-1])
    kinds = [(lo == 0.0) & np.isinf(hi), (lo == -0.05) & (hi == 0.05), (lo == hi), np.isinf(lo) & (hi == -0.02), np.isinf(lo) & np.isinf(hi)]
    assert all(k.any() for k in kinds) and sum(int(k.sum()) for k in kinds) == B.D
    b = R.mixed_batch("logistic", "plain")
    elo, ehi = B.entity_bounds(b, 3, lo, hi)
    ids = B.entity_ids(b, 3)
    assert elo[0] == -np.inf and ehi[0] == np.inf and np.array_equal(elo[1:], lo[ids]) and np.array_equal(ehi[1:], hi[ids])
    plo, phi = B.batch_bounds(b, lo, hi)
    assert plo.size == phi.size == int(R.coef_ptr(b)[-1])


def _cases():
    for loss in B.LOSSES:
        for variant in B.VARIANTS:
            yield loss, variant, "mixed"
        yield loss, "plain", "block"


@pytest.mark.parametrize("loss,variant,which", list(_cases()), ids=lambda v: str(v))
def test_the_restatement_stays_within_the_bars_on_every_committed_case(loss, variant, which):
    """The check that the inputs, not the device, keep within the bars: with the tests' tolerances the restatement alone ends at most
    RESTATEMENT_BAR |F_ref| above the reference on every entity the GPU tests compare, meets every bar of check_batch, and the reference
    alone meets the cap on left-out coefficients."""
    pbs, boxes, refs, b, v = B.case(loss, variant, which)
    B.check_left_out_cap(pbs, boxes, refs)
    cp = R.coef_ptr(b, v["has_intercept"])
    theta, fval = np.zeros(int(cp[-1])), np.zeros(b.E)
    worst, statuses = -np.inf, {}
    for e, pb in pbs.items():
        th, Fv, status, nit, nfev = B.restatement(pb, *boxes[e])
        theta[int(cp[e]):int(cp[e + 1])], fval[e] = th, Fv
        worst = max(worst, (Fv - refs[e][1]) / abs(refs[e][1]))
        statuses[status] = statuses.get(status, 0) + 1
        assert status in (0, 1, 4), (e, status)      # (4: a search that ends at the rounding of F; the bars decide whatever the status is)
    print(f"{loss} {variant} {which}: the restatement ends at most {worst:.3e} |F_ref| above the reference; statuses {statuses}")
    assert worst <= R.RESTATEMENT_BAR
    assert statuses.get(4, 0) <= int(np.ceil(0.01 * len(pbs)))
    B.check_batch(pbs, boxes, refs, theta, fval, cp, convexity=v["distance"], what=f"restatement {loss} {variant} {which}")


@pytest.mark.parametrize("loss", B.LOSSES)
def test_the_one_iteration_cases_excuse_few_entities(loss):
    """max_iter = 1 from a cold start and from a start point outside the box: at most 1 % of the entities have an Armijo test within
    ARMIJO_MARGIN max(|F|, 1) of its edge (the GPU test excuses exactly those from equal counts)."""
    for warm in (False, True):
        one = B.one_iteration(loss, warm)
        excused = [e for e, r in one.items() if not r[4] > R.ARMIJO_MARGIN]
        print(f"{loss} warm={warm}: {len(excused)} of {len(one)} entities excused")
        assert len(excused) <= R.MAX_EXCUSED_SHARE * len(one)
        assert all(r[1] <= 1 for r in one.values())


def test_the_footprint_is_the_plain_kernels_plus_two_vectors():
    assert B.lds_bytes(p=3, n=2, nnz=4, d=2, m=10, has_w=False) == ((25 * 3 + 2 + 20) * 8 + (16 + 3 + 3 + 4) * 4 + 15 & ~15) + 48
    assert B.lds_bytes(6, 4, 10, 5, 10, False) - R.lds_bytes(6, 4, 10, 5, 10, False) == 48      # one coefficient vector more than OWL-QN
    assert B.lds_bytes(4, 2, 5, 3, 10, False) - B.lds_bytes(4, 2, 4, 3, 10, False) == 16        # one non-zero more: four 4-byte entries
