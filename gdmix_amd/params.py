"""Parameter classes of the random-effect stage, field for field as the reference declares them:
GDMixParams / SchemaParams / Params (gdmix-trainer/src/gdmix/params.py:12-50), LRParams
(models/custom/base_lr_params.py:5-42) and REParams (models/custom/random_effect_lr_lbfgs_model.py:34-53).
"""
import math
from dataclasses import dataclass
from typing import ClassVar, Optional

import numpy as np

from . import constants
from .argv import from_argv, to_argv

_ACTIONS = (constants.ACTION_INFERENCE, constants.ACTION_TRAIN)
_STAGES = (constants.FIXED_EFFECT, constants.RANDOM_EFFECT)
_MODEL_TYPES = (constants.LOGISTIC_REGRESSION, constants.LINEAR_REGRESSION, constants.POISSON_REGRESSION, constants.DETEXT)
_VARIANCE_MODE = (constants.FULL, constants.SIMPLE)


def check_feature_normalization(p, stage_flags):
    """--feature_normalization / --feature_statistics_file of a stage's parameters: what needs no context is refused at parse time.
    stage_flags: the other flags of this stage the feature does not run with, as (set?, flag, why)."""
    from . import feature_stats
    kind = feature_stats.check_kind(feature_stats.NONE if p.feature_normalization is None else p.feature_normalization)
    if kind == feature_stats.NONE:
        return kind
    for is_set, flag, why in stage_flags:
        if is_set:
            raise ValueError(f"--feature_normalization={kind} does not run with {flag}: {why}")
    return kind


def check_features_to_samples_ratio(p, stage_flags):
    """--features_to_samples_ratio of a random-effect stage's parameters: a finite ratio above 0, and none of the stage's flags the
    selection does not run with, given as (set?, flag, why). -> the ratio, or None without the flag."""
    ratio = p.features_to_samples_ratio
    if ratio is None:
        return None
    ratio = float(ratio)
    if not math.isfinite(ratio) or ratio <= 0.0:
        raise ValueError(f"--features_to_samples_ratio={ratio!r}: a finite ratio above 0")
    for is_set, flag, why in stage_flags:
        if is_set:
            raise ValueError(f"--features_to_samples_ratio does not run with {flag}: {why}")
    return ratio


def check_active_data_upper_bound(p, stage_flags):
    """--active_data_upper_bound of a random-effect stage's parameters: an integer >= 1, and none of the stage's flags the cap does not
    run with, given as (set?, flag, why). -> the bound, or None without the flag."""
    if p.active_data_upper_bound is None:
        return None
    from . import active_data
    bound = active_data.check_upper_bound(p.active_data_upper_bound)
    for is_set, flag, why in stage_flags:
        if is_set:
            raise ValueError(f"--active_data_upper_bound does not run with {flag}: {why}")
    return bound


def check_l1_reg_weight(value):
    """--l1_reg_weight: a finite weight >= 0 -> float."""
    try:
        w = float(value)
    except (TypeError, ValueError):
        raise ValueError(f"--l1_reg_weight={value!r} is not a number") from None
    if not math.isfinite(w) or w < 0.0:
        raise ValueError(f"--l1_reg_weight={value!r}: a finite weight >= 0")
    return w


def check_elastic_net_alpha(p, stage_flags):
    """--elastic_net_alpha of a random-effect stage's parameters: a finite alpha in [0, 1], and (for alpha > 0) none of the stage's flags
    the L1 term does not run with, given as (set?, flag, why). -> alpha as a float (0.0 without the flag)."""
    if p.elastic_net_alpha is None:
        return 0.0
    try:
        alpha = float(p.elastic_net_alpha)
    except (TypeError, ValueError):
        raise ValueError(f"--elastic_net_alpha={p.elastic_net_alpha!r} is not a number") from None
    if not math.isfinite(alpha) or alpha < 0.0 or alpha > 1.0:
        raise ValueError(f"--elastic_net_alpha={p.elastic_net_alpha!r}: a finite alpha in [0, 1]")
    if alpha > 0.0:
        for is_set, flag, why in stage_flags:
            if is_set:
                raise ValueError(f"--elastic_net_alpha={alpha} does not run with {flag}: {why}")
    return alpha


ENTITY_OPTIMIZERS = ("LBFGS", "TRON")


def check_entity_optimizer(p, stage_flags):
    """--entity_optimizer of a random-effect stage's parameters: LBFGS or TRON in any case, and (for TRON) none of the stage's flags the
    trust-region Newton solve does not run with, given as (set?, flag, why). -> "LBFGS" / "TRON", or None without the flag."""
    if p.entity_optimizer is None:
        return None
    value = str(p.entity_optimizer).strip().upper()
    if value not in ENTITY_OPTIMIZERS:
        raise ValueError(f"--entity_optimizer={p.entity_optimizer!r}: one of {', '.join(ENTITY_OPTIMIZERS)}")
    if value == "TRON":
        for is_set, flag, why in stage_flags:
            if is_set:
                raise ValueError(f"--entity_optimizer=TRON does not run with {flag}: {why}")
    return value


def elastic_net_weights(alpha, lam):
    """Photon-ML's elastic net (alpha, lambda) -> (l1, l2) = (alpha lambda, (1 - alpha) lambda)."""
    alpha, lam = float(alpha), float(lam)
    return alpha * lam, (1.0 - alpha) * lam


def coefficient_bounds(records, features, has_intercept, where="--coefficient_constraints"):
    """Photon-ML's coefficient constraints as arrays. records: a list of {"name", "term", "lowerBound", "upperBound"} (either bound may be
    absent: infinite); features: the (name, term) list of --feature_file, in coefficient order. "term": "*" covers every term of a name,
    "name": "*" with "term": "*" every feature not named otherwise; an exact record beats a term wildcard, which beats the all-wildcard.
    -> (lower, upper), float64 [len(features) + has_intercept], the intercept last and infinite. Every refusal names the record."""
    if not isinstance(records, list):
        raise ValueError(f"{where}: the file holds a JSON array of records, not {type(records).__name__}")
    D = len(features)
    lower, upper = np.full(D + (1 if has_intercept else 0), -np.inf), np.full(D + (1 if has_intercept else 0), np.inf)
    by_name = {}
    index = {}
    for j, (name, term) in enumerate(features):
        index[(name, term)] = j
        by_name.setdefault(name, []).append(j)
    level = np.full(D, -1)      # specificity of the record that set a feature's bounds: 0 all-wildcard, 1 term wildcard, 2 exact
    seen = {}
    for r in records:
        if not isinstance(r, dict) or not isinstance(r.get("name"), str) or not isinstance(r.get("term"), str):
            raise ValueError(f"{where}: record {r!r} needs a \"name\" and a \"term\", both strings")
        unknown = set(r) - {"name", "term", "lowerBound", "upperBound"}
        if unknown:
            raise ValueError(f"{where}: record {r!r} has unknown keys {sorted(unknown)}")
        lo, hi = r.get("lowerBound"), r.get("upperBound")
        for key, v in (("lowerBound", lo), ("upperBound", hi)):
            if v is not None and (isinstance(v, bool) or not isinstance(v, (int, float)) or not math.isfinite(v)):
                raise ValueError(f"{where}: record {r!r}: {key} must be a finite number (leave it out for no bound)")
        lo, hi = -np.inf if lo is None else float(lo), np.inf if hi is None else float(hi)
        if lo > hi:
            raise ValueError(f"{where}: record {r!r}: lowerBound > upperBound")
        name, term = r["name"], r["term"]
        if name == constants.INTERCEPT:
            raise ValueError(f"{where}: record {r!r} names the intercept, which is never bounded")
        if name == "*" and term != "*":
            raise ValueError(f"{where}: record {r!r}: a wildcard name goes with a wildcard term")
        if (name, term) in seen:
            raise ValueError(f"{where}: records {seen[name, term]!r} and {r!r} are for the same features")
        seen[name, term] = r
        if name == "*":
            spec, cover = 0, range(D)
        elif term == "*":
            spec, cover = 1, by_name.get(name, [])
        else:
            spec, cover = 2, [index[name, term]] if (name, term) in index else []
        if len(cover) == 0:
            raise ValueError(f"{where}: record {r!r} matches no feature of the feature file")
        for j in cover:
            if spec > level[j]:
                level[j], lower[j], upper[j] = spec, lo, hi
    return lower, upper


def read_coefficient_constraints(path, features, has_intercept, flag="--coefficient_constraints"):
    """--coefficient_constraints=PATH -> (lower, upper) of coefficient_bounds; the file is a JSON array in the shape of Photon-ML's
    constraint string. Python's NaN / Infinity literals are refused like any non-finite number. flag: the name the messages give the
    flag (the random effect's is --entity_coefficient_constraints)."""
    import json

    def refuse(literal):
        raise ValueError(f"{flag}={path}: {literal} is not a finite number (leave the bound out for no bound)")
    with open(path) as f:
        try:
            records = json.load(f, parse_constant=refuse)
        except json.JSONDecodeError as e:
            raise ValueError(f"{flag}={path}: not JSON ({e})") from None
    return coefficient_bounds(records, features, has_intercept, where=f"{flag}={path}")


def parse_l2_grid(text):
    """'100,10,3,1,0.1' -> (100.0, 10.0, 3.0, 1.0, 0.1): comma-separated finite floats >= 0, at least one, no duplicates."""
    out = []
    for item in str(text).split(","):
        item = item.strip()
        if not item:
            raise ValueError(f"--l2_reg_weights={text!r}: an empty item")
        try:
            w = float(item)
        except ValueError:
            raise ValueError(f"--l2_reg_weights={text!r}: {item!r} is not a number") from None
        if not math.isfinite(w) or w < 0.0:
            raise ValueError(f"--l2_reg_weights={text!r}: {item!r} is not a finite weight >= 0")
        if w in out:
            raise ValueError(f"--l2_reg_weights={text!r}: {item!r} is listed twice")
        out.append(w)
    return tuple(out)


@dataclass(frozen=True)
class EvaluatorSpec:
    """What --evaluators asks for: the logistic loss, the mean per-entity AUC, precision@k for these k (in the order given)."""
    log_loss: bool = False
    auc: bool = False
    ks: tuple = ()
    entity: Optional[str] = None

    @property
    def ranking(self):
        return self.auc or len(self.ks) > 0


MAX_PRECISION_KS = 4      # values of K in one list: what one device call ranks (include/gdmix_re.h, "ranking evaluation")


def parse_evaluators(text, entity, fixed_effect=False):
    """--evaluators=LIST (Photon-ML's evaluator names, any case, comma-separated): LOGISTIC_LOSS, AUC:<id>, PRECISION@K:<id>, with <id>
    the stage's --partition_entity (`entity`), K an integer >= 1, at most four distinct K, no item twice. A fixed-effect stage takes
    LOGISTIC_LOSS only. -> EvaluatorSpec; ValueError for anything else."""
    log_loss, auc, ks, seen = False, False, [], set()
    for raw in str(text).split(","):
        item = raw.strip()
        if not item:
            raise ValueError(f"--evaluators={text!r}: an empty item")
        name, colon, ident = item.partition(":")
        kind = name.strip().upper()
        if kind.startswith("PRECISION@"):
            k_text = kind[len("PRECISION@"):]
            if not k_text.isdigit() or int(k_text) < 1:      # (a sign, a point or nothing: not an integer >= 1)
                raise ValueError(f"--evaluators={text!r}: {item!r}: K is an integer >= 1")
            k = int(k_text)
            if k >= 1 << 31:
                raise ValueError(f"--evaluators={text!r}: {item!r}: K is below 2^31")
            key = ("PRECISION", k)
        elif kind in ("AUC", "LOGISTIC_LOSS"):
            key = (kind,)
        else:
            raise ValueError(f"--evaluators={text!r}: {item!r} is none of LOGISTIC_LOSS, AUC:<id>, PRECISION@K:<id>")
        if key[0] == "LOGISTIC_LOSS":
            if colon:
                raise ValueError(f"--evaluators={text!r}: {item!r}: LOGISTIC_LOSS is taken over all samples and names no entity")
        else:
            if fixed_effect:
                raise ValueError(f"--evaluators={text!r}: {item!r}: a fixed effect has no entities (it takes LOGISTIC_LOSS only)")
            if not colon or not ident.strip():
                raise ValueError(f"--evaluators={text!r}: {item!r} names no entity: {name.strip()}:<id>, with <id> the stage's --partition_entity")
            if entity is None or ident.strip() != entity:
                raise ValueError(f"--evaluators={text!r}: {item!r} groups by {ident.strip()!r}; this stage's entity is --partition_entity={entity}")
        if key in seen:
            raise ValueError(f"--evaluators={text!r}: {item!r} is listed twice")
        seen.add(key)
        if key[0] == "LOGISTIC_LOSS":
            log_loss = True
        elif key[0] == "AUC":
            auc = True
        else:
            ks.append(key[1])
            if len(ks) > MAX_PRECISION_KS:
                raise ValueError(f"--evaluators={text!r}: more than {MAX_PRECISION_KS} distinct K")
    return EvaluatorSpec(log_loss, auc, tuple(ks), None if fixed_effect else entity)


def check_evaluators(p, entity, fixed_effect=False):
    """--evaluators of a stage's parameters: the list itself, and the flags it needs or does not run with. -> EvaluatorSpec, or None
    without the flag."""
    if p.evaluators is None:
        return None
    spec = parse_evaluators(p.evaluators, entity, fixed_effect)
    if not p.metric_output_dir:
        raise ValueError("--evaluators needs --metric_output_dir: the values go into its evalSummary.json")
    if p.l2_reg_weights is not None:
        raise ValueError("--evaluators does not run with --l2_reg_weights: choosing a sweep's winner by these metrics is not implemented")
    return spec


def check_evaluators_model_type(spec, model_type):
    """--evaluators rank and weigh a probability: the stage is a logistic regression."""
    if spec is not None and model_type != constants.LOGISTIC_REGRESSION:
        raise ValueError(f"--evaluators needs --model_type={constants.LOGISTIC_REGRESSION}: this stage is a {model_type}")


class _ArgvMixin:
    @classmethod
    def __from_argv__(cls, argv, error_on_unknown=False):
        return from_argv(cls, argv, error_on_unknown=error_on_unknown)

    def __to_argv__(self):
        return to_argv(self)


@dataclass
class SchemaParams(_ArgvMixin):
    uid_column_name: str                                    # Unique id column name in the train/validation data.
    weight_column_name: Optional[str] = None                # weight column name in the train/validation data.
    label_column_name: Optional[str] = None                 # Label column name in the train/validation data.
    prediction_score_column_name: Optional[str] = None      # Prediction score column name in the generated result file.
    prediction_score_per_coordinate_column_name: str = "predictionScorePerCoordinate"


@dataclass
class Params(_ArgvMixin):
    """GDMix driver parameters = SchemaParams + GDMixParams (params.py:12-50)."""
    uid_column_name: str
    weight_column_name: Optional[str] = None
    label_column_name: Optional[str] = None
    prediction_score_column_name: Optional[str] = None
    prediction_score_per_coordinate_column_name: str = "predictionScorePerCoordinate"
    action: str = constants.ACTION_TRAIN
    stage: str = constants.FIXED_EFFECT
    model_type: str = constants.LOGISTIC_REGRESSION
    training_score_dir: Optional[str] = None
    validation_score_dir: Optional[str] = None
    partition_list_file: Optional[str] = None

    def __post_init__(self):
        assert self.action in _ACTIONS, f"Action: {self.action} must be in {_ACTIONS}"
        assert self.stage in _STAGES, f"Stage: {self.stage} must be in {_STAGES}"
        assert self.model_type in _MODEL_TYPES, f"Model type: {self.model_type} must be in {_MODEL_TYPES}"
        assert (self.action == constants.ACTION_TRAIN and self.label_column_name) or \
               (self.action == constants.ACTION_INFERENCE and self.prediction_score_column_name)


@dataclass
class LRParams(_ArgvMixin):
    """Base linear model parameters (base_lr_params.py:5-42)."""
    metadata_file: str
    output_model_dir: str
    training_data_dir: Optional[str] = None
    validation_data_dir: Optional[str] = None
    feature_bag: Optional[str] = None
    feature_file: Optional[str] = None
    regularize_bias: bool = True
    l2_reg_weight: float = 1.0
    lbfgs_tolerance: float = 1e-12
    num_of_lbfgs_curvature_pairs: int = 10
    num_of_lbfgs_iterations: int = 100
    has_intercept: bool = True
    offset_column_name: str = "offset"
    batch_size: int = 16
    data_format: str = "tfrecord"
    # un-annotated in the reference, hence not settable from argv (base_lr_params.py:32)
    sparsity_threshold: ClassVar[float] = 1.0e-4

    def __post_init__(self):
        assert self.batch_size > 0, "Batch size must be positive number"
        if self.regularize_bias:
            assert self.has_intercept, "Intercept must be used when it is regularized"
        assert self.feature_bag or self.has_intercept, "Either intercept or feature bag much be used"


@dataclass
class REParams(LRParams):
    """Random-effect model parameters (random_effect_lr_lbfgs_model.py:34-53). The queue / consumer knobs
    are accepted for CLI compatibility; the device solver has no job queue and ignores them."""
    partition_entity: Optional[str] = None
    enable_local_indexing: bool = False
    max_training_queue_size: int = 10
    training_queue_timeout_in_seconds: int = 300
    num_of_consumers: int = 2
    random_effect_variance_mode: Optional[str] = None
    disable_random_effect_scoring_after_training: bool = False
    # not in the reference: move entities between the workers of a node when partitions are skewed (rebalance.py)
    rebalance_entities: bool = False
    # not in the reference: the stage writes its metric (evalSummary.json: auc, mse for linear_regression, poisson_loss for poisson_regression) and the per-entity
    # metrics of everything it scores under this directory, computed on the device while the scores are there (metrics.py)
    metric_output_dir: Optional[str] = None
    # not in the reference: --action=train sweeps these weights inside the stage (sweep.py: every partition solved once per weight, the
    # validation data scored under all of them, the stage metric of each on the device), then trains the stage as usual with the best one.
    # Comma-separated; l2_reg_weight is ignored when it is given. Needs validation_data_dir and metric_output_dir.
    l2_reg_weights: Optional[str] = None
    # not in the reference (which leaves it open, random_effect_lr_lbfgs_model.py:155-160: "revisit it when we implement incremental
    # learning"): with a prior model in output_model_dir the L2 term is centred on the prior means and weighted by the prior precisions
    # (the variances --random_effect_variance_mode wrote), so that training on a new day's data alone is the Bayesian update of
    # yesterday's model, as Photon-ML defines incremental training (include/gdmix_re.h, "incremental training"). A prior feature an
    # entity's new data lacks keeps its prior mean and variance. Without a prior model the stage trains as without the flag.
    incremental_training: bool = False
    # not in the reference (Photon-ML's NormalizationType): none (the default, also when the flag is absent), scale_with_standard_deviation
    # or scale_with_max_magnitude — the L2 term penalises coefficients in normalised units, (l2/2) sum (theta_j / s_j)^2 with s_j from
    # exact column statistics of the stage's training data (include/gdmix_re.h, "feature normalisation"; feature_stats.py). Models, scores
    # and metrics stay in the original feature units. --action=inference accepts and ignores both flags.
    feature_normalization: Optional[str] = None
    # the statistics as an .npz: read and used when the file exists (no statistics pass runs), computed and written there otherwise
    feature_statistics_file: Optional[str] = None
    # not in the reference (Photon-ML's numFeaturesToSamplesRatioUpperBound): before an entity is trained it keeps only the
    # ceil(ratio * n_e) features of its bag whose Pearson correlation with the label is largest in magnitude (include/gdmix_re.h, "feature
    # selection"; feature_selection.py). The intercept is kept apart and takes no slot (in Photon-ML it takes one). A dropped feature is
    # from there on a feature the entity's data does not contain. --action=inference accepts and ignores the flag.
    features_to_samples_ratio: Optional[float] = None
    # not in the reference (Photon-ML's activeDataUpperBound): an entity of more than this many samples trains on a uniform sample of that
    # many, each weighted n_e / bound, chosen by a hash of (active_data_seed, uid) (include/gdmix_re.h, "active-data cap"; active_data.py).
    # Only the solver's batch is cut: scores and metrics see every row. Runs before the feature selection, which then sees the capped
    # batch. --action=inference accepts and ignores both flags.
    active_data_upper_bound: Optional[int] = None
    active_data_seed: int = 0
    # the fixed-effect stage's flag (fe_model.FixedLRParams). This stage's parser ignores flags it does not know, so the field exists to
    # refuse a non-zero value instead of training a ridge model in silence.
    l1_reg_weight: float = 0.0
    # ... and so is --optimizer: anything but LBFGS is refused. The random effect's optimiser is chosen by --entity_optimizer (below).
    optimizer: str = "LBFGS"
    # ... and so is --coefficient_constraints: this stage's box constraints are --entity_coefficient_constraints (below).
    coefficient_constraints: Optional[str] = None
    # not in the reference (Photon-ML's evaluator names): LOGISTIC_LOSS, AUC:<id>, PRECISION@K:<id>, comma-separated, any case, <id> this
    # stage's partition_entity. The stage's evalSummary.json gains the logistic loss and the means of the per-entity AUC and precision@K,
    # its perEntity records precision_at_K (include/gdmix_re.h, "ranking evaluation"; metrics.py). Needs metric_output_dir and
    # --model_type=logistic_regression; does not run with l2_reg_weights. --action=inference honours it when the data has labels.
    evaluators: Optional[str] = None
    # not in the reference (Photon-ML's elastic net per random-effect coordinate): alpha in [0, 1], with l2_reg_weight as its lambda: every
    # entity minimises (1/n)(loss + (l2/2)|theta_R|^2 + l1 |theta_R|_1) with l1 = alpha lambda, l2 = (1 - alpha) lambda, by OWL-QN on the device
    # (include/gdmix_re.h, "elastic net"). Coefficients at exactly 0 stay out of the model file. Absent or 0: the stage is what it was. The
    # stage has a flag of its own because --l1_reg_weight is the fixed effect's: this stage's parser drops flags it does not know, so that
    # field exists here to refuse a value that would otherwise train a ridge model in silence, and that refusal stays. From the fixed
    # effect's (l1, l2): l2_reg_weight = l1 + l2, elastic_net_alpha = l1 / (l1 + l2). Does not run with incremental_training or a
    # feature_normalization (the L1 term is not invariant under their diagonal substitution), l2_reg_weights or rebalance_entities.
    # --action=inference accepts and ignores the flag.
    elastic_net_alpha: Optional[float] = None
    # not in the reference (Photon-ML's coefficient box constraints per random-effect coordinate): a JSON file in the format of the fixed
    # effect's --coefficient_constraints (read_coefficient_constraints: records, wildcards and refusals are the same), names and terms those
    # of this stage's --feature_file. Every entity minimises its smooth objective subject to lo_j <= theta_j <= hi_j, one box per feature
    # for all entities, the intercept free, by projected L-BFGS on the device (include/gdmix_re.h, "box constraints"). The stage has a flag
    # of its own for the reason --elastic_net_alpha has: --coefficient_constraints is the fixed effect's, this stage's parser drops flags
    # it does not know, and the field above refuses it; that refusal stays. Needs --feature_file and --feature_bag. Does not run with
    # elastic_net_alpha > 0, incremental_training or a feature_normalization (the bounds are in original units; the substitution is a
    # follow-up, as in the fixed effect), l2_reg_weights or rebalance_entities. --action=inference accepts and ignores the flag: it does not
    # open the file. These refusals are made where the parameters are parsed, whatever the action, as --elastic_net_alpha's are.
    entity_coefficient_constraints: Optional[str] = None
    # not in the reference (Photon-ML's OptimizerType per random-effect coordinate): LBFGS (the default, also when the flag is absent: the
    # stage is byte for byte what it was) or TRON, any case: every entity minimises the stage's smooth objective by trust-region Newton on
    # the device (include/gdmix_re.h, "TRON"). The stage has a flag of its own for the reason --elastic_net_alpha has: --optimizer is the
    # fixed effect's, this stage's parser drops flags it does not know, and the field above refuses --optimizer=TRON; that refusal stays.
    # Does not run with elastic_net_alpha > 0 or entity_coefficient_constraints (the objective must be smooth and unconstrained),
    # incremental_training or a feature_normalization (both are changes of variables on the packed batch and compose in principle: a
    # follow-up), l2_reg_weights or rebalance_entities. --action=inference accepts and ignores the flag.
    entity_optimizer: Optional[str] = None

    def l2_grid(self):
        """The weights of --l2_reg_weights in the order given, or None without the flag."""
        return None if self.l2_reg_weights is None else parse_l2_grid(self.l2_reg_weights)

    def normalization(self):
        """The value of --feature_normalization ("none" without the flag)."""
        return "none" if self.feature_normalization is None else self.feature_normalization

    def evaluator_spec(self):
        """What --evaluators asks for (EvaluatorSpec), or None without the flag."""
        return check_evaluators(self, self.partition_entity)

    def entity_tron(self):
        """Does --entity_optimizer ask for the trust-region Newton solve?"""
        return self.entity_optimizer == "TRON"

    def elastic_net(self):
        """(l1, l2) of the stage's solves: Photon-ML's (alpha, lambda) = (elastic_net_alpha, l2_reg_weight); (0, l2_reg_weight) without the flag."""
        alpha = 0.0 if self.elastic_net_alpha is None else float(self.elastic_net_alpha)
        return elastic_net_weights(alpha, self.l2_reg_weight) if alpha > 0.0 else (0.0, float(self.l2_reg_weight))

    def __post_init__(self):
        self.l2_grid()      # a bad list is an error at parse time
        self.evaluator_spec()
        if self.coefficient_constraints is not None:
            raise ValueError(f"--coefficient_constraints={self.coefficient_constraints}: the random effect has no box constraints (the flag belongs to the fixed-effect stage)")
        if check_l1_reg_weight(self.l1_reg_weight) != 0.0:
            raise ValueError(f"--l1_reg_weight={self.l1_reg_weight}: the random effect has no L1 term (the flag belongs to the fixed-effect stage)")
        if str(self.optimizer).strip().upper() != "LBFGS":
            raise ValueError(f"--optimizer={self.optimizer}: the random effect trains by L-BFGS-B only (the flag belongs to the fixed-effect stage)")
        check_feature_normalization(self, (
            (self.incremental_training, "--incremental_training", "prior variances are in the original feature units, and composing the two is not implemented"),
            (self.l2_reg_weights is not None, "--l2_reg_weights", "a sweep in normalised units is not implemented"),
            (self.rebalance_entities, "--rebalance_entities", "the factors do not travel with the exchange")))
        check_features_to_samples_ratio(self, (
            (self.incremental_training, "--incremental_training", "a prior feature the selection drops would keep its prior mean, and composing the two is not implemented"),
            (self.l2_reg_weights is not None, "--l2_reg_weights", "a sweep over selected features is not implemented"),
            (self.feature_normalization not in (None, "none"), "--feature_normalization", "the correlation is taken in the original feature units, and composing the two is not implemented"),
            (self.rebalance_entities, "--rebalance_entities", "the selection does not travel with the exchange")))
        bound = check_active_data_upper_bound(self, (
            (self.l2_reg_weights is not None, "--l2_reg_weights", "a sweep over capped entities is not implemented"),
            (self.rebalance_entities, "--rebalance_entities", "sample uids do not travel with the exchange"),
            (self.incremental_training, "--incremental_training", "the prior precisions were fitted on uncapped data, and composing the two is not implemented"),
            (self.feature_normalization not in (None, "none"), "--feature_normalization", "the column statistics are those of the uncapped data, and composing the two is not implemented")))
        if bound is not None:
            self.active_data_upper_bound = bound
        if self.elastic_net_alpha is not None:
            self.elastic_net_alpha = check_elastic_net_alpha(self, (
                (self.incremental_training, "--incremental_training", "the L1 term is not invariant under the substitution that centres the L2 term on the prior"),
                (self.feature_normalization not in (None, "none"), "--feature_normalization", "the L1 term is not invariant under the diagonal substitution of the normalised units"),
                (self.l2_reg_weights is not None, "--l2_reg_weights", "a sweep of elastic-net models is not implemented"),
                (self.rebalance_entities, "--rebalance_entities", "the elastic-net solve of exchanged entities is not implemented")))
        if self.entity_coefficient_constraints is not None:
            flag = "--entity_coefficient_constraints"
            if not self.feature_file or not self.feature_bag:
                raise ValueError(f"{flag} names features by the names and terms of --feature_file: it does not run without --feature_file and --feature_bag")
            for is_set, other, why in (
                    (bool(self.elastic_net_alpha), "--elastic_net_alpha", "bounds with an L1 term are not implemented"),
                    (self.incremental_training, "--incremental_training", "the bounds are in original units, and bounds under the prior's substitution are not implemented"),
                    (self.feature_normalization not in (None, "none"), "--feature_normalization", "the bounds are in original units, and bounds under the normalisation's substitution are not implemented"),
                    (self.l2_reg_weights is not None, "--l2_reg_weights", "a sweep of bounded models is not implemented"),
                    (self.rebalance_entities, "--rebalance_entities", "the bounded solve of exchanged entities is not implemented")):
                if is_set:
                    raise ValueError(f"{flag} does not run with {other}: {why}")
        self.entity_optimizer = check_entity_optimizer(self, (
            (bool(self.elastic_net_alpha), "--elastic_net_alpha", "TRON minimises a smooth objective; the L1 term has its own optimiser, OWL-QN"),
            (self.entity_coefficient_constraints is not None, "--entity_coefficient_constraints", "TRON minimises without constraints"),
            (self.incremental_training, "--incremental_training", "TRON under the substitution that centres the L2 term on the prior is not implemented"),
            (self.feature_normalization not in (None, "none"), "--feature_normalization", "TRON under the diagonal substitution of the normalised units is not implemented"),
            (self.l2_reg_weights is not None, "--l2_reg_weights", "a sweep of TRON solves is not implemented"),
            (self.rebalance_entities, "--rebalance_entities", "the TRON solve of exchanged entities is not implemented")))
        if self.incremental_training and self.l2_reg_weights is not None:
            raise ValueError("--incremental_training does not run with --l2_reg_weights: the sweep is defined for a cold start")
        if self.incremental_training and self.rebalance_entities:
            raise ValueError("--incremental_training does not run with --rebalance_entities: prior variances do not travel with the exchange")
        # the reference's REParams.__post_init__ does NOT chain to LRParams.__post_init__ (random_effect_lr_lbfgs_model.py:
        # 48-53): `--has_intercept False` with regularize_bias left at its default True is a valid random-effect
        # configuration upstream (test_random_effect_lr_lbfgs_model.py: warm start without intercept)
        assert self.max_training_queue_size > self.num_of_consumers, \
            "queue size limit must be larger than the number of consumers"
        assert self.random_effect_variance_mode is None or self.random_effect_variance_mode in _VARIANCE_MODE, \
            f"Action: {self.random_effect_variance_mode} must be in {_VARIANCE_MODE}"
