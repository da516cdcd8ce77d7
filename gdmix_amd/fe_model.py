"""FixedEffectLRModelLBFGS on an MI355X: the Python mirror of the reference's fixed-effect model class
(gdmix-trainer/src/gdmix/models/custom/fixed_effect_lr_lbfgs_model.py:57-812) around the device solver of
gdmix_amd/fixed_effect.py. Same constructor, attributes, train / predict / export signatures and files:

  in   <training_data_dir>/*.tfrecord[.gz|.deflate]   one tf.train.Example per sample (per_record_input_fn,
       io/input_data_pipeline.py:129-221): dense columns (uid, label, offset, weight) as scalars, the sparse bag as
       `<bag>_indices` / `<bag>_values`; files are sorted and worker w of W reads files[w::W] (or file w when there
       are fewer files than workers; util/distribution_utils.py:11-47)
  out  <output_model_dir>/part-00000.avro             one BayesianLinearModelAvro, modelId "global model" (:690-728),
       written by the chief after thresholding |theta| <= 1e-4 -> 0 (:648-649)
       <training_score_dir>/part-{task:05d}.avro, <validation_score_dir>/part-{task:05d}.avro   (:406-440)

Training with W > 1 workers: every worker runs this with torch.distributed initialised; gradient and value are
all-reduced once per L-BFGS evaluation (fixed_effect.py: run_stepping_loop), the step is replicated.
Not carried over: copy_to_local and the TF server knobs (accepted, unused). fixed_effect_variance_mode is carried over: SIMPLE and FULL
are computed on the training data after the fit and written next to the means (fixed_effect._variances).

Not in the reference, one worker only (both refused with several, before anything is read):
  --metric_output_dir=DIR   everything the stage scores is also fed, from HBM, into an exact AUC (logistic_regression) or MSE
       (linear_regression) on the device (metrics.DeviceEvaluator): DIR/evalSummary.json in the random-effect stage's layout
       (metrics.StageMetrics.write_summary; no perEntity/: a fixed effect has no entities). --action=inference reports what it scores.
  --l2_reg_weights=w0,w1,.. the stage sweeps l2_reg_weight itself: shards read, uploaded and packed once, gdmix_fe_create once, per
       weight a cold gdmix_fe_restart + solve, the validation shard scored under all the models in one pass over its non-zeros
       (gdmix_fe_score_models), one exact metric per weight, the files of sweep.py under DIR/sweep/. The winner's coefficients then go
       through the rest of train() as if fit_stepping had returned them: the stage's files are those of a plain run at that weight.
Not in the reference either, any number of workers:
  --incremental_training=True   with a prior model in output_model_dir the L2 term is centred on its means and weighted by its precisions
       (the variances --fixed_effect_variance_mode wrote into the same file; 1 where there is none), the fit starts at the prior means, and
       the variances written are the posterior's: training on a new day's data alone is the Bayesian update of yesterday's model
       (include/gdmix_fe.h, "incremental training"; the reference leaves it open, :361-367). Every worker reads the same model file.
       Without a prior model the stage is a plain cold run. Refused with --l2_reg_weights and with --action=inference.
  --l1_reg_weight=W   the objective gains W |theta_R|_1 (R: what l2_reg_weight regularises) and the stage trains by OWL-QN on the device
       (include/gdmix_fe.h, "(ABI 23) L1 / elastic net"): coefficients outside the support are exactly 0 and stay out of the model file; the
       number of non-zeros is logged. Photon-ML's elastic net (lambda, alpha) is W = alpha lambda, l2_reg_weight = (1 - alpha) lambda.
       Refused with --l2_reg_weights, --incremental_training and --feature_normalization; --action=inference ignores it.
  --optimizer=LBFGS|TRON   (case-insensitive; Photon-ML's OptimizerType; default LBFGS, a stage without the flag is bit for bit what it was)
       TRON trains the stage by trust-region Newton on the device (include/gdmix_fe.h, "(ABI 24) TRON"): conjugate gradients on
       Hessian-vector products, each the same two streaming passes as an evaluation. The number of products is logged. With
       --l2_reg_weights the sweep keeps the optimiser. Refused with a non-zero --l1_reg_weight, --incremental_training and
       --feature_normalization; --action=inference ignores it.
  --coefficient_constraints=PATH   box constraints on coefficients (Photon-ML's coefficient constraints): the stage minimises its smooth
       objective subject to lowerBound <= theta <= upperBound by projected L-BFGS on the device (include/gdmix_fe.h, "(ABI 26) box
       constraints"). PATH is a JSON array of {"name", "term", "lowerBound", "upperBound"} in the names and terms of --feature_file; either
       bound may be absent (infinite); "term": "*" covers every term of a name, "name": "*", "term": "*" every feature not named otherwise,
       an exact record beats a wildcard (params.coefficient_bounds). The intercept is never bounded. The bounds are in original feature
       units; a warm start is clamped into the box; with --l2_reg_weights every model of the sweep keeps them. How many coefficients ended
       at a bound is logged. The stage does not threshold to 0 a coefficient whose box excludes 0. Refused without --feature_file, with a non-zero
       --l1_reg_weight, --optimizer=TRON, --incremental_training and a --feature_normalization other than none; --action=inference ignores it.
"""
import glob
import logging
import os
from dataclasses import dataclass
from typing import Optional

import numpy as np

from . import constants
from .fixed_effect import LINEAR_REGRESSION, LOGISTIC_REGRESSION, POISSON_REGRESSION, FixedEffectDeviceSolver
from .io import avro, native_reader, tfrecord
from .io.features import read_feature_list
from .io.grouped_reader import resolve_input_files
from .io.metadata import DatasetMetadata
from .params import LRParams, check_evaluators_model_type, check_feature_normalization, check_l1_reg_weight, parse_l2_grid, read_coefficient_constraints

logger = logging.getLogger(__name__)
logger.setLevel(logging.INFO)

GLOBAL_MODEL_ID = "global model"
MODEL_CLASS = {LOGISTIC_REGRESSION: "com.linkedin.photon.ml.supervised.classification.LogisticRegressionModel",
               LINEAR_REGRESSION: "com.linkedin.photon.ml.supervised.regression.LinearRegressionModel",
               POISSON_REGRESSION: constants.PHOTON_POISSON_MODEL_CLASS}


@dataclass
class FixedLRParams(LRParams):
    """fixed_effect_lr_lbfgs_model.py:57-71."""
    copy_to_local: bool = True
    num_server_creation_retries: int = 50
    retry_interval: int = 2
    delayed_exit_in_seconds: int = 60
    disable_fixed_effect_scoring_after_training: bool = False
    fixed_effect_variance_mode: Optional[str] = None
    # not in the reference (the random-effect stage's flags of the same names, params.REParams): the stage metric on the device, and
    # a sweep over l2_reg_weight inside the stage; l2_reg_weight is ignored when the list is given
    metric_output_dir: Optional[str] = None
    l2_reg_weights: Optional[str] = None
    # not in the reference (which leaves it open, fixed_effect_lr_lbfgs_model.py:361-367); the random-effect stage's flag of the same
    # name (params.REParams): the L2 term centred on the prior model in output_model_dir and weighted by its precisions
    incremental_training: bool = False
    # not in the reference; the random-effect stage's flags of the same names (params.REParams): the L2 term penalises coefficients in
    # normalised units, the factors from exact column statistics of all workers' training data (all-reduced integers)
    feature_normalization: Optional[str] = None
    feature_statistics_file: Optional[str] = None
    # not in the reference: Photon-ML's downSamplingRate. The solver's training shard is down-sampled on the device (include/gdmix_re.h,
    # "down-sampling"): a row is kept by a hash of (seed, uid) with probability `rate` and then weighs 1 / rate; a logistic stage keeps
    # every positive as it is. Scores, metrics, feature statistics and validation data see every row. 1.0: no sampling. The random-effect
    # stage has no such flag.
    down_sampling_rate: float = 1.0
    down_sampling_seed: int = 0
    # not in the reference: Photon-ML's regularizationType = L1 / ELASTIC_NET. The objective gains l1 |theta_R|_1 (R as for the L2 term) and
    # the stage trains by OWL-QN on the device (include/gdmix_fe.h, "(ABI 23) L1 / elastic net"): coefficients outside the support are
    # exactly 0 and stay out of the model file. Photon-ML's (lambda, alpha) is l1 = alpha lambda, l2 = (1 - alpha) lambda. 0: no L1 term.
    # --action=inference accepts and ignores the flag.
    l1_reg_weight: float = 0.0
    # not in the reference: Photon-ML's OptimizerType. TRON: trust-region Newton on the device (include/gdmix_fe.h, "(ABI 24) TRON"); LBFGS: the
    # stage as it was. Any case. --action=inference accepts and ignores the flag.
    optimizer: str = "LBFGS"
    # not in the reference: Photon-ML's coefficient box constraints, a JSON file of {"name", "term", "lowerBound", "upperBound"} records
    # (params.coefficient_bounds). The stage trains by projected L-BFGS on the device (include/gdmix_fe.h, "(ABI 26) box constraints").
    # --action=inference accepts and ignores the flag.
    coefficient_constraints: Optional[str] = None
    # not in the reference; the random-effect stage's flag of the same name (params.REParams). A fixed effect has no entities: the list
    # holds LOGISTIC_LOSS only, and the stage's evalSummary.json gains "logistic_loss" and "ll". Needs metric_output_dir and
    # --model_type=logistic_regression; does not run with l2_reg_weights.
    evaluators: Optional[str] = None
    # the random-effect stage's flag (params.REParams). This stage's parser ignores flags it does not know, so the field exists to refuse
    # TRON instead of training by L-BFGS in silence: the fixed effect's flag is --optimizer.
    entity_optimizer: Optional[str] = None

    def evaluator_spec(self):
        """What --evaluators asks for (params.EvaluatorSpec), or None without the flag."""
        from .params import check_evaluators
        return check_evaluators(self, None, fixed_effect=True)

    def l2_grid(self):
        """The weights of --l2_reg_weights in the order given, or None without the flag."""
        return None if self.l2_reg_weights is None else parse_l2_grid(self.l2_reg_weights)

    def normalization(self):
        """The value of --feature_normalization ("none" without the flag)."""
        return "none" if self.feature_normalization is None else self.feature_normalization

    def down_sampling_given(self):
        """Was one of the two down-sampling flags set to something other than its default?"""
        return self.down_sampling_rate != 1.0 or self.down_sampling_seed != 0

    def __post_init__(self):
        super().__post_init__()
        self.l2_grid()      # a bad list is an error at parse time
        self.evaluator_spec()
        if self.entity_optimizer is not None and str(self.entity_optimizer).strip().upper() != "LBFGS":
            raise ValueError(f"--entity_optimizer={self.entity_optimizer}: the flag belongs to the random-effect stage (the fixed effect's is --optimizer)")
        from .downsample import check_rate
        try:
            self.down_sampling_rate = check_rate(self.down_sampling_rate)
        except TypeError:
            raise ValueError(f"--down_sampling_rate={self.down_sampling_rate!r} is not a number") from None
        if isinstance(self.down_sampling_seed, bool) or not isinstance(self.down_sampling_seed, int):
            raise ValueError(f"--down_sampling_seed={self.down_sampling_seed!r} is not an integer")
        check_feature_normalization(self, (
            (self.incremental_training, "--incremental_training", "prior variances are in the original feature units, and composing the two is not implemented"),
            (self.l2_reg_weights is not None, "--l2_reg_weights", "a sweep in normalised units is not implemented")))
        self.l1_reg_weight = check_l1_reg_weight(self.l1_reg_weight)
        if self.l1_reg_weight > 0.0:
            for is_set, flag, why in (
                    (self.l2_reg_weights is not None, "--l2_reg_weights", "a sweep with an L1 term is not implemented"),
                    (self.incremental_training, "--incremental_training", "the L1 term is not invariant under the prior's change of variables"),
                    (self.normalization() != "none", "--feature_normalization", "the L1 term is not invariant under the change to normalised units")):
                if is_set:
                    raise ValueError(f"--l1_reg_weight does not run with {flag}: {why}")
        from .fixed_effect import TRON, check_optimizer
        self.optimizer = check_optimizer(self.optimizer)
        if self.optimizer == TRON:
            for is_set, flag, why in (
                    (self.l1_reg_weight > 0.0, "--l1_reg_weight", "TRON minimises a smooth objective; the L1 term has its own optimiser, OWL-QN"),
                    (self.incremental_training, "--incremental_training", "the Hessian-vector product has no variant for the prior's change of variables yet"),
                    (self.normalization() != "none", "--feature_normalization", "the Hessian-vector product has no variant for normalised units yet")):
                if is_set:
                    raise ValueError(f"--optimizer=TRON does not run with {flag}: {why}")
        if self.coefficient_constraints is not None:
            if not (self.feature_bag and self.feature_file):
                raise ValueError("--coefficient_constraints names features by the names and terms of --feature_file: it does not run without --feature_file")
            for is_set, flag, why in (
                    (self.l1_reg_weight > 0.0, "--l1_reg_weight", "the bounded step minimises a smooth objective"),
                    (self.optimizer == TRON, "--optimizer=TRON", "TRON minimises without constraints"),
                    (self.incremental_training, "--incremental_training", "the bounds are not carried through the prior's change of variables yet"),
                    (self.normalization() != "none", "--feature_normalization", "the bounds are in original units and are not carried into normalised units yet")):
                if is_set:
                    raise ValueError(f"--coefficient_constraints does not run with {flag}: {why}")
        if self.incremental_training and self.l2_reg_weights is not None:
            raise ValueError("--incremental_training does not run with --l2_reg_weights: the sweep is defined for a cold start")
        assert self.fixed_effect_variance_mode is None or self.fixed_effect_variance_mode in (constants.FULL, constants.SIMPLE), \
            f"Action: {self.fixed_effect_variance_mode} must be in {(constants.FULL, constants.SIMPLE)}"


def shard_input_files(input_path, num_shards, shard_index):
    """util/distribution_utils.py:11-47: every entry of the directory (glob '*': whatever its suffix, dot-files
    excluded), sorted, strided over the workers; with fewer files than workers, worker w gets file w (or nothing).
    Entries that are not record files (Spark's zero-byte `_SUCCESS` marker, sub-directories: upstream's glob returns them too)
    take part in the striding exactly as they do upstream and then contribute no records (read_per_record_files)."""
    assert 0 <= shard_index < num_shards and num_shards >= 1
    pattern = os.path.join(input_path, "*") if os.path.isdir(input_path) else input_path
    files = sorted(glob.glob(pattern))
    assert len(files) > 0, f"{input_path} is empty"
    if len(files) < num_shards:
        return [files[shard_index]] if shard_index < len(files) else []
    return files[shard_index::num_shards]


def read_per_record_files(files, metadata: DatasetMetadata, feature_bag, num_features, uid_name, label_name, offset_name,
                          weight_name, native=None):
    """tf.train.Example records -> flat sample arrays (CSR over samples). Columns that the metadata does not list are
    defaults: offset 0, weight 1, label 0 (fixed_effect_lr_lbfgs_model.py:255-258,345-346). native None: libgdmix_io.so
    when built (same rules; tests/test_fe_model.py compares the two)."""
    files = [f for f in files if os.path.isfile(f) and os.path.getsize(f) > 0]   # zero-byte entries (`_SUCCESS`) and directories hold no records
    names = set(metadata.get_feature_names()) | set(metadata.get_label_names())
    has = lambda n: n is not None and n in names
    has_label, has_offset, has_weight = has(label_name), has(offset_name), has(weight_name)
    if native is None:
        native = native_reader.available()
    if native:
        d = native_reader.read_example_files(files, feature_bag, num_features, uid_name, label_name if has_label else None,
                                             offset_name if has_offset else None, weight_name if has_weight else None)
        d["has_label"], d["has_weight"] = has_label, has_weight
        return d
    uid, y, off, w, k, cols, vals = [], [], [], [], [], [], []
    ikey, vkey = (f"{feature_bag}_indices", f"{feature_bag}_values") if feature_bag else (None, None)

    def scalar(feats, name, what):
        if name not in feats:
            raise KeyError(f"column {name!r} is missing from a record")
        kind, v = feats[name]
        if len(v) != 1:
            raise ValueError(f"{what} column {name!r} must hold one value per record, got {len(v)}")
        return v[0]

    for fn in files:
        for rec in tfrecord.iter_records(fn):
            feats = tfrecord.decode_example(rec)
            uid.append(int(scalar(feats, uid_name, "uid")))
            y.append(float(scalar(feats, label_name, "label")) if has_label else 0.0)
            off.append(float(scalar(feats, offset_name, "offset")) if has_offset else 0.0)
            w.append(float(scalar(feats, weight_name, "weight")) if has_weight else 1.0)
            if feature_bag:
                ci = feats.get(ikey, ("int64", np.zeros(0, np.int64)))[1]
                cv = feats.get(vkey, ("float", np.zeros(0, np.float32)))[1]
                if len(ci) != len(cv):
                    raise ValueError(f"{ikey} and {vkey} differ in length in a record of {fn}")
                ci = np.asarray(ci, np.int64)
                if ci.size and (ci.min() < 0 or ci.max() >= num_features):
                    raise ValueError(f"feature index outside [0, {num_features}) in {fn}")
                k.append(len(ci))
                cols.append(ci)
                vals.append(np.asarray(cv, np.float32))
            else:
                k.append(0)
    n = len(uid)
    cat = lambda parts, dt: np.concatenate(parts).astype(dt) if parts else np.zeros(0, dt)
    return dict(n=n, row_nnz_ptr=np.concatenate([[0], np.cumsum(np.array(k, np.int64))]).astype(np.int64),
                col=cat(cols, np.int64), val=cat(vals, np.float32), y=np.array(y, np.float32), offset=np.array(off, np.float32),
                weight=np.array(w, np.float32), uid=np.array(uid, np.int64), has_label=has_label, has_weight=has_weight)


class FixedEffectLRModelLBFGS:
    """Linear / logistic regression over the whole data set, trained on the device."""

    def __init__(self, raw_model_params, base_training_params, device=None):
        self.model_params: FixedLRParams = self._parse_parameters(raw_model_params)
        p = self.model_params
        self.fixed_effect_variance_mode = p.fixed_effect_variance_mode
        self.variances = None
        self.training_output_dir = base_training_params.training_score_dir
        self.validation_output_dir = base_training_params.validation_score_dir
        self.model_type = base_training_params.model_type
        self.evaluator_spec = p.evaluator_spec()      # --evaluators (params.EvaluatorSpec: LOGISTIC_LOSS only here), or None
        check_evaluators_model_type(self.evaluator_spec, self.model_type)
        self.training_data_dir = p.training_data_dir
        self.validation_data_dir = p.validation_data_dir
        self.metadata_file = p.metadata_file
        self.checkpoint_path = p.output_model_dir
        self.data_format = p.data_format
        self.offset_column_name = p.offset_column_name
        self.feature_bag_name = p.feature_bag
        self.feature_file = p.feature_file if self.feature_bag_name else None
        self.has_intercept = p.has_intercept
        self.is_regularize_bias = p.regularize_bias
        self.max_iteration = p.num_of_lbfgs_iterations
        self.l2_reg_weight = p.l2_reg_weight
        self.sparsity_threshold = p.sparsity_threshold
        self.num_correction_pairs = p.num_of_lbfgs_curvature_pairs
        if self.model_type == constants.LOGISTIC_REGRESSION:
            self.disable_fixed_effect_scoring_after_training = p.disable_fixed_effect_scoring_after_training
        else:   # no inference after training for plain linear regression (:110-113)
            self.disable_fixed_effect_scoring_after_training = True
        self.metadata = DatasetMetadata(self.metadata_file)
        self.num_features = self._get_num_features()
        self.model_coefficients = None
        self.last_training_info = None
        self._device = device
        self._fe = None
        self.metric_output_dir = p.metric_output_dir
        self._metrics = None      # metrics.StageMetrics while a stage with --metric_output_dir runs
        self._coefficient_bounds = None      # (lower, upper) of --coefficient_constraints once the file has been read

    # ---- helpers ------------------------------------------------------------------------------------------------
    def _parse_parameters(self, raw_model_parameters):
        return FixedLRParams.__from_argv__(raw_model_parameters, error_on_unknown=False)

    def _get_num_features(self):
        if self.feature_bag_name is None:
            return 1   # intercept only model: a dummy feature (:157-165)
        return self.metadata.get_feature_shape(self.feature_bag_name)[0]

    def _solver(self):
        if self._fe is None:
            device = self._device if self._device is not None else int(os.environ.get("LOCAL_RANK", "0"))
            self._fe = FixedEffectDeviceSolver(device)
        return self._fe

    def _read(self, input_path, num_workers, task_index, schema_params):
        files = shard_input_files(input_path, num_workers, task_index)
        return read_per_record_files(files, self.metadata, self.feature_bag_name, self.num_features,
                                     schema_params.uid_column_name, schema_params.label_column_name, self.offset_column_name,
                                     schema_params.weight_column_name)

    # ---- what the two flags refuse ---------------------------------------------------------------------------------
    def check_request(self, execution_context, action=constants.ACTION_TRAIN):
        """--metric_output_dir / --l2_reg_weights: everything they do not do is refused here, before a file is read, a process group
        is formed or a solver created (as sweep.validate does for the random effect). Inference ignores --l2_reg_weights."""
        from . import sweep
        mp = self.model_params
        if action != constants.ACTION_TRAIN and mp.down_sampling_given():
            raise ValueError("--down_sampling_rate / --down_sampling_seed sample the training shard of a fit: they do not run with --action=inference")
        grid = mp.l2_grid() if action == constants.ACTION_TRAIN else None
        if grid is not None:
            sweep.refuse_poisson(self.model_type)
        if grid is None and not mp.metric_output_dir:
            return
        sweep.refuse_several_workers(execution_context, "--l2_reg_weights" if grid is not None else "--metric_output_dir")
        if grid is not None:
            sweep.refuse_blind_or_warm(mp, sorted(glob.glob(os.path.join(mp.output_model_dir, "*.avro"))) if mp.output_model_dir else [],
                                       " the stage would warm-start from")

    # ---- the stage metric (--metric_output_dir) ---------------------------------------------------------------------
    def _metric_name(self):
        from . import metrics
        if self.model_type == constants.POISSON_REGRESSION:
            return metrics.POISSON_LOSS
        return metrics.MSE if self.model_type == constants.LINEAR_REGRESSION else metrics.AUC

    def _begin_metrics(self):
        self._metrics = None
        if self.metric_output_dir:
            from . import metrics
            fe = self._solver()
            if not hasattr(fe, "score_device"):
                raise NotImplementedError("--metric_output_dir needs the device scoring path (FixedEffectDeviceSolver.score_device)")
            self._metrics = metrics.StageMetrics(getattr(fe, "solver", None), self.metric_output_dir, self._metric_name(), self.evaluator_spec)

    def _finish_metrics(self):
        m, self._metrics = self._metrics, None
        return None if m is None else m.write_summary()

    def _shard_arrays(self, data, fit=False):
        """(row_nnz_ptr, col, val) of the shard. A model without a feature bag has none: Nones as upload / score take them, or with
        `fit` the empty rows fit_* and shard_as_batch take."""
        if self.feature_bag_name is not None:
            return data["row_nnz_ptr"], data["col"], data["val"]
        return (np.zeros(data["n"] + 1, np.int64), [], []) if fit else (None, None, None)

    def _device_shard(self, data):
        """The shard's sample-major arrays (and labels) in HBM, uploaded once per shard read."""
        if "_dev" not in data:
            bag = self.feature_bag_name is not None
            data["_dev"] = self._solver().upload(*self._shard_arrays(data), data["offset"], self.num_features if bag else 0,
                                                 label=data["y"] if data["has_label"] else None)
        return data["_dev"]

    # ---- feature normalisation (--feature_normalization) ------------------------------------------------------------------
    def _feature_factors(self, kind, data, is_chief):
        """The factors [num_features] of this stage, the same bits on every worker: the statistics of all workers' training samples, from
        --feature_statistics_file or from two passes over this worker's device shard with the integers all-reduced (feature_stats.py).
        A worker whose shard is empty still takes part."""
        from . import feature_stats
        fe = self._solver()
        shard = self._device_shard(data) if data["n"] > 0 else None
        factor, self.feature_statistics = feature_stats.fixed_effect_factors(
            kind, self.model_params.feature_statistics_file, fe.solver, self.num_features, None if shard is None else shard.cg,
            None if shard is None else shard.vl, data["n"], is_chief=is_chief)
        return factor

    # ---- down-sampling (--down_sampling_rate) -----------------------------------------------------------------------------
    def _down_sampling(self, data):
        """fit_stepping's / fit_sweep's down_sampling argument for this stage's training shard: {} at rate 1.0 (the call is skipped)."""
        mp = self.model_params
        if mp.down_sampling_rate == 1.0:
            if mp.down_sampling_seed != 0:
                logger.warning(f"--down_sampling_seed={mp.down_sampling_seed} has no effect: --down_sampling_rate is 1.0, the stage trains on every row")
            return {}
        return {"down_sampling": (mp.down_sampling_rate, mp.down_sampling_seed, data["uid"])}

    # ---- the sweep (--l2_reg_weights) ----------------------------------------------------------------------------------
    def _stage_coefficients(self, theta):
        """fit_stepping's coefficients as the stage keeps them: the dummy weight of an intercept-only model in front
        (add_dummy_weight), then threshold_coefficients (:648-649)."""
        if self.feature_bag_name is None:
            theta = np.concatenate([[0.0], theta])
        return np.where(np.abs(theta) <= self.sparsity_threshold, 0.0, theta)

    def _sweep(self, data, vdata, grid):
        """-> (theta, info) of the weight with the best validation metric, as fit_stepping returns them; model_params.l2_reg_weight is
        the winner's from here on."""
        from . import sweep
        if not vdata["has_label"]:
            raise sweep.SweepError("the validation data carries no labels: the sweep has nothing to compare")
        fe = self._solver()
        bag = self.feature_bag_name is not None
        metric = self._metric_name()
        K = len(grid)
        logger.info(f"sweeping l2_reg_weight over {list(grid)} by validation {metric}; --l2_reg_weight={self.l2_reg_weight} is ignored")

        def select(thetas):
            blocks = []
            if vdata["n"] > 0:
                shard = self._device_shard(vdata)
                stage = [self._stage_coefficients(th) for th in thetas]
                chunk = fe.models_per_chunk(K, stage[0].size, vdata["n"])
                for first in range(0, K, chunk):
                    _, per = fe.score_models(shard, [th if bag else th[1:] for th in stage[first:first + chunk]], self.has_intercept, per_coord=True)
                    for j in range(per.shape[0]):
                        ev = fe.new_evaluator()
                        ev.add(fe.file_scores(shard, per[j]), shard.y)
                        blocks.append(ev.finish())
                    del per
            else:
                blocks = [fe.new_evaluator().finish() for _ in grid]
            return sweep.conclude(self.metric_output_dir, metric, grid, blocks)

        theta, info, best = fe.fit_sweep(
            *self._shard_arrays(data, fit=True), data["y"], self.num_features, l2_grid=grid, select=select, offset=data["offset"],
            weight=data["weight"] if data["has_weight"] else None, has_intercept=self.has_intercept, regularize_bias=self.is_regularize_bias, model_type=self.model_type, max_iter=self.max_iteration,
            m=self.num_correction_pairs, tolerance=self.model_params.lbfgs_tolerance, dummy=not bag,
            variance_mode=self.fixed_effect_variance_mode, threshold=self.sparsity_threshold, **self._optimizer(), **self._bounds(), **self._down_sampling(data))
        self.l2_reg_weight = self.model_params.l2_reg_weight = float(grid[best])
        return theta, info

    def _optimizer(self):
        """{"optimizer": ...} for fit_stepping / fit_sweep, or {} with the default: the call is then what it was before the flag existed."""
        opt = self.model_params.optimizer
        return {} if opt == "LBFGS" else {"optimizer": opt}

    def _bounds(self):
        """{"bounds": (lower, upper)} for fit_stepping / fit_sweep from --coefficient_constraints, or {} without the flag: the call is then
        what it was before the flag existed. The file is read once per stage; every worker reads the same file."""
        path = self.model_params.coefficient_constraints
        if path is None:
            return {}
        if self._coefficient_bounds is None:
            lower, upper = read_coefficient_constraints(path, read_feature_list(self.feature_file), self.has_intercept)
            if lower.size != self.num_features + (1 if self.has_intercept else 0):
                raise ValueError(f"--coefficient_constraints: --feature_file lists {lower.size - (1 if self.has_intercept else 0)} features, the metadata's "
                                 f"feature bag has {self.num_features}")
            self._coefficient_bounds = (lower, upper)
        return {"bounds": self._coefficient_bounds}

    # ---- train ----------------------------------------------------------------------------------------------------
    def train(self, training_data_dir, validation_data_dir, metadata_file, checkpoint_path, execution_context, schema_params):
        task_index = execution_context[constants.TASK_INDEX]
        num_workers = execution_context[constants.NUM_WORKERS]
        is_chief = execution_context[constants.IS_CHIEF]
        self.check_request(execution_context, constants.ACTION_TRAIN)
        grid = self.model_params.l2_grid()
        self._bounds()      # a bad constraints file is an error before any data is read
        self._begin_metrics()
        data = self._read(training_data_dir, num_workers, task_index, schema_params)
        D = self.num_features
        bag = self.feature_bag_name is not None
        vdata = None
        if grid is not None:
            # --l2_reg_weights: the validation shard is read here, once, and chooses the weight; no prior model (check_request)
            vdata = self._read(validation_data_dir, num_workers, task_index, schema_params)
            theta, info = self._sweep(data, vdata, grid)
        else:
            incremental = bool(self.model_params.incremental_training)
            prev_model = self._load_model(catch_exception=True, with_variance=incremental)
            prev_var = None
            if incremental and prev_model is not None:
                prev_model, prev_var = prev_model
            expected = self.num_features + 1 if self.has_intercept else self.num_features
            x0 = prior = None
            if prev_model is not None and len(prev_model) == expected:
                x0 = np.asarray(prev_model, np.float64)
                if incremental:
                    # the L2 term is centred on the prior model (include/gdmix_fe.h, "incremental training"); the fit starts at its means
                    logger.info("Found a previous model, loaded as the prior of incremental training")
                    if prev_var is None:
                        logger.info("The previous model carries no variances: every prior variance defaults to 1")
                    prior = (x0 if bag else x0[1:], prev_var if (bag or prev_var is None) else prev_var[1:])
                    x0 = None
                else:
                    logger.info("Found a previous model, loaded as the initial point for training")
            elif prev_model is not None:
                logger.info(f"Initial model size is {len(prev_model)}, expected {expected}, use all zeros instead.")
            extra = {} if prior is None else {"prior": prior}
            kind = self.model_params.normalization()
            if kind != "none" and bag:
                extra["feature_scale"] = self._feature_factors(kind, data, is_chief)      # (the statistics of every row, sampled or not)
            extra.update(self._down_sampling(data))
            if self.model_params.l1_reg_weight > 0.0:
                extra["l1"] = self.model_params.l1_reg_weight
            extra.update(self._optimizer())
            extra.update(self._bounds())
            theta, info = self._solver().fit_stepping(
                *self._shard_arrays(data, fit=True), data["y"], D, offset=data["offset"], weight=data["weight"] if data["has_weight"] else None,
                has_intercept=self.has_intercept, l2=self.l2_reg_weight, regularize_bias=self.is_regularize_bias,
                model_type=self.model_type, theta0=self._strip_dummy(x0) if not bag else x0, max_iter=self.max_iteration,
                m=self.num_correction_pairs, tolerance=self.model_params.lbfgs_tolerance, dummy=not bag,
                variance_mode=self.fixed_effect_variance_mode, threshold=self.sparsity_threshold, **extra)
        self.variances = info.pop("variances", None)
        if not bag and self.variances is not None:
            self.variances = np.concatenate([[0.0], self.variances])   # next to the dummy weight of an intercept-only model
        self.last_training_info = info
        if "down_sampling" in info:
            c = info["down_sampling"]
            logger.info(f"down-sampling at rate {c['rate']} (seed {c['seed']}): {c['kept']} of {c['rows']} rows kept, {c['positives']} positives in the "
                        f"shard, {c['negatives_kept']} negatives kept, {c['kept_nnz']} non-zeros")
        logger.info(f"f_min: {info['fval']} num of funcalls: {info['nfev']} status: {info['status']}")
        if self.model_params.l1_reg_weight > 0.0:
            logger.info(f"l1_reg_weight {self.model_params.l1_reg_weight}: {int(np.count_nonzero(theta))} of {theta.size} coefficients are non-zero")
        if self._optimizer():
            logger.info(f"optimizer {self.model_params.optimizer}: {info['nit']} iterations, {info['nfev']} evaluations, {info.get('nhv', 0)} Hessian-vector products")
        if self._bounds():
            lower, upper = self._coefficient_bounds
            at_bound = info.get("at_bound", int(np.count_nonzero((theta == lower) | (theta == upper))))
            logger.info(f"coefficient_constraints: {at_bound} of {theta.size} coefficients ended at a bound")
            kept = self._stage_coefficients(theta)
            self.model_coefficients = theta = np.where((kept < lower) | (kept > upper), theta, kept)      # 0 outside the box: not thresholded
        else:
            self.model_coefficients = theta = self._stage_coefficients(theta)
        # the reference's variance computation rides on the scoring pass over the training data, which therefore runs (and writes
        # its scores) whenever a variance mode is set (:650-661)
        if not self.disable_fixed_effect_scoring_after_training or self.fixed_effect_variance_mode is not None:
            self._score_and_write(theta, data, task_index, schema_params, self.training_output_dir, which="training")
        if validation_data_dir:
            if vdata is None:
                vdata = self._read(validation_data_dir, num_workers, task_index, schema_params)
            self._score_and_write(theta, vdata, task_index, schema_params, self.validation_output_dir, which="validation")
        if is_chief:
            self._save_model()
        self._finish_metrics()

    @staticmethod
    def _strip_dummy(x0):
        return None if x0 is None else x0[1:]

    # ---- scoring ---------------------------------------------------------------------------------------------------
    def _score_and_write(self, theta, data, task_index, schema_params, output_dir, which="validation"):
        """logits = X w + b (per-coordinate score), + offset (score); :214-306,406-440. With --metric_output_dir the scores stay in HBM
        long enough to enter `which`'s accumulator of the stage metric: the very floats the score file holds."""
        from .fixed_effect import shard_as_batch, to_local
        n = data["n"]
        bag = self.feature_bag_name is not None
        if self._metrics is not None and not data["has_label"]:
            self._metrics.no_labels(f"the {which} data")
        if n == 0:
            per_coord = np.zeros(0, np.float32)
        elif self._metrics is not None:
            fe = self._solver()
            shard = self._device_shard(data)
            _, per_dev = fe.score_device(shard, theta if bag else theta[1:], self.has_intercept)
            if data["has_label"]:
                if which not in self._metrics.ev:
                    poisson = self._metrics.metric == "poisson_loss"
                    self._metrics.ev[which] = fe.new_evaluator(self._metrics.metric) if poisson else fe.new_evaluator()
                file_scores = fe.file_scores(shard, per_dev)
                self._metrics.ev[which].add(file_scores, shard.y)
                self._metrics.add_log_loss(which, file_scores, shard.y)      # (--evaluators=LOGISTIC_LOSS; nothing without it)
            per_coord = fe.to_host(per_dev)
        else:
            fe = self._solver()
            if hasattr(fe, "score"):      # the device path: one pass over the sample-major arrays, no pack
                _, per_coord = fe.score(*self._shard_arrays(data), data["offset"], theta if bag else theta[1:], self.num_features if bag else 0,
                                        self.has_intercept)
            else:
                batch, dummy = shard_as_batch(*self._shard_arrays(data, fit=True), np.zeros(n, np.float32), data["offset"], None, self.has_intercept,
                                              dummy=not bag)
                packed = fe.solver.pack(batch, has_intercept=self.has_intercept)
                uniq = packed.unique_global().cpu().numpy()
                th = theta if bag else theta[1:]
                local = to_local(th, uniq, self.num_features if bag else 0, self.has_intercept, dummy)
                logit, per = fe.solver.score(packed, local)
                per_coord = per.cpu().numpy()[:n]    # (a shard without any non-zero carries one padding sample of weight 0)
        score = (per_coord.astype(np.float64) + data["offset"].astype(np.float64)).astype(np.float32)
        self._write_inference_result(data["uid"], data["y"] if data["has_label"] else None,
                                     data["weight"] if data["has_weight"] else None, score, per_coord, task_index, schema_params,
                                     output_dir)

    def _write_inference_result(self, sample_ids, labels, weights, prediction_score, prediction_score_per_coordinate, task_index,
                                schema_params, output_dir):
        schema = avro.inference_output_schema(schema_params, has_weight=weights is not None)
        output_file = os.path.join(output_dir, f"part-{task_index:05d}.avro")
        # the reference writes int(weight) into the float field (:427-428)
        w = None if weights is None else np.trunc(weights).astype(np.float32)
        header, sync = avro.container_header(schema, "null")
        if native_reader.available():
            native_reader.write_scores_avro(output_file, header, sync, sample_ids, prediction_score, labels, w,
                                            prediction_score_per_coordinate)
        else:
            from .model import _write_scores
            _write_scores(output_file, schema, schema_params, sample_ids, prediction_score, labels, w,
                          prediction_score_per_coordinate, native=False)
        logger.info(f"Worker {task_index} has written inference result to {output_file}")

    # ---- model file -------------------------------------------------------------------------------------------------
    def _save_model(self):
        """One BayesianLinearModelAvro: (INTERCEPT) first, then the features with |value| > threshold (:690-728,
        util/io_utils.py:102-160)."""
        from .model import ModelTable, _export_models_to_avro
        theta = self.model_coefficients
        D = self.num_features
        ic = 1 if self.has_intercept else 0
        bag = self.feature_bag_name is not None
        weights = theta[:D] if bag else np.zeros(0)
        local = np.concatenate([theta[D:D + ic], weights])   # intercept first, as the export helper expects
        var_local = None
        if self.variances is not None:
            var_local = np.concatenate([self.variances[D:D + ic], self.variances[:D] if bag else np.zeros(0)])
        table = ModelTable()
        table.add_chunk([GLOBAL_MODEL_ID], local, [0, local.size], np.arange(weights.size, dtype=np.int64), [0, weights.size],
                        variance=var_local)
        feature_list = self._feature_prefixes() if self.feature_file else None
        output_file = os.path.join(self.checkpoint_path, "part-00000.avro")
        _export_models_to_avro(output_file, table, feature_list, self.has_intercept, self.variances is not None, self.sparsity_threshold,
                               model_class=MODEL_CLASS[self.model_type])
        logger.info(f"dumped the global model to {output_file}")

    def _feature_prefixes(self):
        """(feature list, its Avro-encoded form) as _export_models_to_avro and the native model reader take them; for a plain feature
        file straight from its bytes (native_reader.EncodedFeatures.from_feature_file: 100 k features in milliseconds instead of 0.2 s)."""
        if native_reader.available():
            fast = native_reader.EncodedFeatures.from_feature_file(self.feature_file)
            if fast is not None:
                return (None, fast)
        fl = read_feature_list(self.feature_file)
        enc = [avro.enc_string(n) + avro.enc_string(t) for (n, t) in fl]
        return (fl, native_reader.EncodedFeatures(enc) if native_reader.available() else enc)

    def _load_model(self, catch_exception=False, with_variance=False):
        """-> coefficients [num_features (+1, intercept last)] or None (:730-747, load_linear_models_from_avro). with_variance: ->
        (coefficients, variances | None) — the record's variances mapped by the same join, 0 where the record has none for a coefficient
        (fixed_effect.usable_variance puts the default in), None for a record without variances."""
        if not (self.checkpoint_path and os.path.exists(self.checkpoint_path)):
            if catch_exception:
                return None
            raise FileNotFoundError(f"checkpoint path {self.checkpoint_path} doesn't exist")
        files = sorted(glob.glob(os.path.join(self.checkpoint_path, "*.avro")))
        if len(files) != 1:
            if catch_exception:
                return None
            raise ValueError(f"Load model failed, no model file or multiple model files found in the model directory {self.checkpoint_path}")
        D = self.num_features
        ic = 1 if self.has_intercept else 0
        theta = self._load_model_native(files[0], D, ic, with_variance=with_variance)
        if theta is not None:
            return theta
        return self._load_model_python(files[0], D, ic, with_variance=with_variance)

    def _load_model_python(self, path, D, ic, with_variance=False):
        """The record-by-record decoder with the reference's lenient rules: every file the native reader declines."""
        from .io.features import get_feature_map
        fmap = get_feature_map(self.feature_file) if self.feature_file else {}
        rec = next(iter(avro.read_file(path)))

        def joined(triples):
            out = np.zeros(D + ic)
            for m in triples:
                if m["name"] == constants.INTERCEPT and m["term"] == "":
                    if ic:
                        out[D] = m["value"]
                else:
                    j = fmap.get((m["name"], m["term"]))
                    if j is not None and j < D:
                        out[j] = m["value"]
            return out
        theta = joined(rec["means"])
        if not with_variance:
            return theta
        return theta, None if rec.get("variances") is None else joined(rec["variances"])

    def _load_model_native(self, path, D, ic, with_variance=False):
        """The same coefficients through libgdmix_io.so (a million (name, term, value) triples decode in milliseconds instead
        of seconds); None when the file is not of the plain layout this trainer and photon-ml write — intercept first, every
        feature in the feature file — and the record-by-record Python decoder has to apply the reference's lenient rules."""
        if not (self.feature_file and ic and native_reader.available()):
            return None
        try:
            schema, codec, sync, data_offset = avro.read_header(path)
            if codec not in ("null", "deflate") or not avro.is_model_schema(schema):
                return None
            prefix = self._feature_prefixes()[1]
            m = native_reader.read_models_avro(path, data_offset, sync, codec == "deflate", prefix,
                                               avro.enc_string(constants.INTERCEPT) + avro.enc_string(""), True)
        except (KeyError, AssertionError, ValueError):
            return None
        if len(m["ids"]) < 1:
            return None
        c0, c1 = int(m["coef_ptr"][0]), int(m["coef_ptr"][1])       # the first record, as next(iter(...)) takes
        idx = m["feat_idx"][c0:c1 - 1]
        if idx.size and int(idx.max()) >= D:
            return None
        theta = np.zeros(D + ic)
        theta[D] = m["mean"][c0]
        theta[idx] = m["mean"][c0 + 1:c1]      # of a feature listed twice the later value, as the Python loop leaves it
        if not with_variance:
            return theta
        if m["variance"] is None or not m["has_variance"][0]:
            return theta, None
        var = np.zeros(D + ic)
        var[D] = m["variance"][c0]
        var[idx] = m["variance"][c0 + 1:c1]
        return theta, var

    def export(self, output_model_dir):
        logger.info("No need model export for LR model.")

    # ---- predict ----------------------------------------------------------------------------------------------------
    def predict(self, output_dir, input_data_path, metadata_file, checkpoint_path, execution_context, schema_params):
        task_index = execution_context[constants.TASK_INDEX]
        num_workers = execution_context[constants.NUM_WORKERS]
        if self.model_params.incremental_training:
            raise ValueError("--incremental_training does not run with --action inference: it defines how a model is trained, scoring reads "
                             "the model as it is")
        self.check_request(execution_context, constants.ACTION_INFERENCE)      # (--l2_reg_weights is ignored here)
        self._begin_metrics()
        data = self._read(input_data_path, num_workers, task_index, schema_params)
        theta = self._load_model()
        self._score_and_write(theta, data, task_index, schema_params, output_dir, which="validation")
        self._finish_metrics()
