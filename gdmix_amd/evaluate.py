"""Drop-in for gdmix-data's metric job (com.linkedin.gdmix.evaluation.Evaluator), on the device:

    python -m gdmix_amd.evaluate --metricsInputDir D --outputMetricFile F --labelColumnName response \\
        --predictionColumnName predictionScore --metricName auc|mse|poisson_loss|logistic_loss

reads every Avro file under D, evaluates (score, label) with gdmix_amd.metrics.DeviceEvaluator and writes F/evalSummary.json =
{"<metricName>": value}: the Spark job's flags (all required) and its output. The score files are read with the Python Avro decoder
(the native reader has no entry point for score files); the evaluation itself runs on the MI355X and nowhere else.
"""
import json
import os
import sys

import numpy as np

from . import metrics

FLAGS = ("metricsInputDir", "outputMetricFile", "labelColumnName", "predictionColumnName", "metricName")
EVAL_SUMMARY_JSON = "evalSummary.json"


def parse(argv) -> dict:
    """--flag value or --flag=value for the five required flags -> dict. ValueError for anything else, a missing flag, or a metric
    other than auc / mse / poisson_loss / logistic_loss (the Evaluator's wording for its two). Touches no device. The grouped metrics of a
    stage's --evaluators (auc:<id>, precision@K:<id>) are not offered here: score files carry no entity id."""
    out = {}
    it = iter(argv)
    for a in it:
        if not a.startswith("--"):
            raise ValueError(f"unexpected argument {a!r}")
        name, eq, val = a[2:].partition("=")
        if name not in FLAGS:
            raise ValueError(f"unknown option --{name}")
        if not eq:
            try:
                val = next(it)
            except StopIteration:
                raise ValueError(f"missing value after --{name}") from None
        out[name] = val.strip()
    for f in FLAGS:
        if f not in out:
            raise ValueError(f"Missing option --{f}")
    check_metric(out["metricName"])
    return out


def check_metric(name):
    if name not in (metrics.AUC, metrics.MSE, metrics.POISSON_LOSS, metrics.LOGISTIC_LOSS):      # (the two losses are this library's: the Evaluator has no such metric)
        raise ValueError(f"Do not support metric {name}, currently only support 'auc' and 'mse'.")


def read_columns(input_dir, label_name, score_name):
    """Every *.avro under input_dir (sorted walk) -> (score float32, label float32)."""
    from .io import avro
    sc, lab = [], []
    for r, _, fs in sorted(os.walk(input_dir)):
        for fn in sorted(fs):
            if fn.endswith(".avro"):
                for rec in avro.read_file(os.path.join(r, fn)):
                    y = rec[label_name]
                    if y is None:
                        raise ValueError(f"{os.path.join(r, fn)}: a record without {label_name!r}")
                    sc.append(rec[score_name])
                    lab.append(y)
    return np.array(sc, np.float32), np.array(lab, np.float32)


def evaluate(score, label, metric_name, solver=None) -> dict:
    """(score, label) float32 host arrays -> DeviceEvaluator.finish() of one accumulator holding them."""
    check_metric(metric_name)
    own = solver is None
    if own:
        from .solver import REDeviceSolver
        solver = REDeviceSolver(0)
    try:
        ev = {metrics.POISSON_LOSS: metrics.PoissonEvaluator, metrics.LOGISTIC_LOSS: metrics.LogLossEvaluator}.get(metric_name, metrics.DeviceEvaluator)(solver)
        ev.add(score, label)
        return ev.finish()
    finally:
        if own:
            solver.close()


def write_summary(output_dir, summary: dict):
    os.makedirs(output_dir, exist_ok=True)
    with open(os.path.join(output_dir, EVAL_SUMMARY_JSON), "w") as f:
        json.dump(summary, f)


def run(argv, solver=None) -> float:
    p = parse(argv)
    score, label = read_columns(p["metricsInputDir"], p["labelColumnName"], p["predictionColumnName"])
    value = evaluate(score, label, p["metricName"], solver)[p["metricName"]]
    write_summary(p["outputMetricFile"], {p["metricName"]: value})
    return value


if __name__ == "__main__":
    try:
        run(sys.argv[1:])
    except ValueError as e:
        print(f"gdmix_amd.evaluate: {e}", file=sys.stderr)
        sys.exit(2)
