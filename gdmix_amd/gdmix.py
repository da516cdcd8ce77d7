"""CLI entry of the random-effect stage, flag-compatible with the reference's
`python -m gdmix.gdmix --stage=random_effect ...` (gdmix-trainer/src/gdmix/gdmix.py:13-36): one flat argv is
shared by Params, SchemaParams and REParams, unknown flags are ignored, any failure exits non-zero.

    python -m gdmix_amd.gdmix --stage=random_effect --action=train --model_type=logistic_regression \\
        --partition_list_file=... --training_data_dir=... --metadata_file=... --output_model_dir=... ...

--model_type=linear_regression trains the per-entity squared loss on real-valued labels, --model_type=poisson_regression the Poisson loss
on count labels (model.py). --stage=fixed_effect runs the linear / logistic / Poisson fixed-effect model (fe_model.py); the DeText stage is
out of scope.
"""
import logging
import sys

from . import constants
from .driver import FixedEffectDriver, RandomEffectDriver
from .model import RandomEffectLRLBFGSModel
from .params import Params, SchemaParams

logging.basicConfig(level=logging.INFO)
logger = logging.getLogger(__name__)


def run(args):
    params = Params.__from_argv__(args, error_on_unknown=False)
    schema_params = SchemaParams.__from_argv__(args, error_on_unknown=False)
    logger.info(f"Parsed schema params amd gdmix args (params): {params}")
    if params.stage == constants.FIXED_EFFECT:
        if params.model_type not in constants.LBFGS_MODEL_TYPES:
            raise NotImplementedError(f"model type {params.model_type!r}: the fixed effect runs logistic_regression and linear_regression, and poisson_regression on count labels")
        from .fe_model import FixedEffectLRModelLBFGS
        driver = FixedEffectDriver(base_training_params=params, model=FixedEffectLRModelLBFGS(raw_model_params=args, base_training_params=params))
    elif params.stage == constants.RANDOM_EFFECT:
        if params.model_type not in constants.LBFGS_MODEL_TYPES:
            raise ValueError(f"model type {params.model_type!r}: the random effect runs logistic_regression and linear_regression, and poisson_regression on count labels")
        driver = RandomEffectDriver(base_training_params=params,
                                    model=RandomEffectLRLBFGSModel(raw_model_params=args, base_training_params=params))
    else:
        raise NotImplementedError(f"stage {params.stage!r} does not run on this library")
    if params.action == constants.ACTION_TRAIN:
        driver.run_training(schema_params=schema_params, export_model=True)
    elif params.action == constants.ACTION_INFERENCE:
        driver.run_inference(schema_params=schema_params)
    else:
        raise Exception(f"Unsupported action {params.action}")


if __name__ == "__main__":
    run(sys.argv)
