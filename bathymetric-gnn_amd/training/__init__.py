"""Mirror of the loss side of the reference's ``training`` package: the multi-task loss of ``BathymetricGNN`` (fused HIP kernels
on float32 device tensors, the same formulas as torch operations elsewhere) and the two helpers that derive its class weights and
Huber delta from the training data.  The reference's ``Trainer`` and datasets (torch_geometric loaders, GDAL, tqdm) are outside
the path; its last two lines of a step -- ``clip_grad_norm_`` and ``optimizer.step()`` -- are ``FusedAdamW`` (HIP kernels over the flat
weight blob, the packed model refreshed in place)."""
from .losses import (BathymetricGNNLoss, ClassificationLoss, ConfidenceCalibrationLoss, CorrectionLoss, FeaturePreservationLoss,
                     ShoalSafetyLoss, compute_class_weights, compute_correction_delta)
from .optim import FusedAdamW

# (the names the reference's ``training`` package exports on its loss side; ``FusedAdamW`` is this package's own addition)
__all__ = ["BathymetricGNNLoss", "ClassificationLoss", "CorrectionLoss", "ConfidenceCalibrationLoss", "FeaturePreservationLoss",
           "ShoalSafetyLoss", "compute_class_weights", "compute_correction_delta"]
