"""Mirror of the reference's ``training`` package: the multi-task loss of ``BathymetricGNN`` (fused HIP kernels on float32 device
tensors, the same formulas as torch operations elsewhere), the two helpers that derive its class weights and Huber delta from the
training data, the last two lines of a step -- ``clip_grad_norm_`` and ``optimizer.step()`` -- as ``FusedAdamW`` (HIP kernels over the
flat weight blob, the packed model refreshed in place), and the reference's ``Trainer`` over device-resident ``TileStore`` s
(``tile_store.py``, ``trainer.py``: per-node targets and per-step bookkeeping as kernels of ``include/bgnn_trainer.h``), and the metrics of
``scripts/evaluate_model.py`` counted on the device (``evaluation.py``: ``Evaluator``, ``compute_metrics``).  The reference's dataset
classes themselves (torch_geometric loaders, GDAL, tqdm) stay outside the path.  ``operating_curve.py`` sweeps every confidence
threshold of a table in one pass over a classified survey and its ground truth (``OperatingCurve``, ``curve_from_block``,
``recommend_thresholds``).  ``huber_delta.py`` is the adaptive Huber delta the reference defers: the per-epoch percentile of the
correction errors measured on the device (``CorrectionErrorTracker``, ``device_percentile``) and the policy that turns it into the
next epoch's delta (``AdaptiveHuberDelta``; ``Trainer(adaptive_delta=...)``)."""
from .losses import (BathymetricGNNLoss, ClassificationLoss, ConfidenceCalibrationLoss, CorrectionLoss, FeaturePreservationLoss,
                     ShoalSafetyLoss, compute_class_weights, compute_correction_delta)
from .huber_delta import AdaptiveHuberDelta, CorrectionErrorTracker, device_percentile, percentile_from_ranks
from .evaluation import Evaluator, compute_metrics, metrics_from_block
from .operating_curve import OperatingCurve, curve_accumulate, curve_from_block, recommend_thresholds
from .optim import FusedAdamW
from .tile_store import (TileStore, cut_tile_boxes, dihedral_ops, keep_ground_truth_boxes, plan_ground_truth_tiles, plan_tile_boxes,
                         scan_tile_boxes, transformed_tile_table)
from .trainer import EpochMetrics, StopRule, Trainer, training_settings

# (the names the reference's ``training`` package exports on its loss side; ``FusedAdamW``, the trainer's classes and the evaluation are importable from here without being listed)
__all__ = ["BathymetricGNNLoss", "ClassificationLoss", "CorrectionLoss", "ConfidenceCalibrationLoss", "FeaturePreservationLoss",
           "ShoalSafetyLoss", "compute_class_weights", "compute_correction_delta"]
