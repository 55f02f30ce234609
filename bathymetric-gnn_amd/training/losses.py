"""Loss functions for bathymetric GNN training (reference ``training/losses.py``): classification, correction, confidence
calibration, feature preservation and shoal safety, and their weighted sum ``BathymetricGNNLoss``.

``BathymetricGNNLoss.forward`` on float32 device tensors is one autograd node over the kernels of ``include/bgnn_loss.h``
(``csrc/loss.hip``): a per-node pass and a finish for the six values, one launch for the three input gradients, float64
arithmetic and sums in a fixed order, each value rounded to float32 once, nothing read back to the host.  On anything else (CPU
tensors, other dtypes, an empty batch) the five component modules below run the same formulas as torch operations.
INTEGRATION.md ("Training loss") has the formulas.
"""
from __future__ import annotations

import ctypes as C
from typing import Dict, Optional

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F
from torch.autograd.function import once_differentiable

from .. import runtime as rt

# rows behind one partial sum of the per-node pass, and partials the finish workgroup reads per pass (include/bgnn_loss.h)
ROWS_PER_WORKGROUP = rt.LOSS_ROWS_PER_WG
FINISH_WIDTH = rt.LOSS_FINISH_WIDTH
MAX_CLASSES = rt.LOSS_MAX_CLASSES
TERMS = rt.LOSS_TERMS


class ClassificationLoss(nn.Module):
    """Weighted, label-smoothed cross-entropy over the nodes (mean over the class weights of the rows that are not ``-100``)."""

    def __init__(self, class_weights: Optional[torch.Tensor] = None, label_smoothing: float = 0.0):
        super().__init__()
        self.class_weights = class_weights
        self.label_smoothing = label_smoothing

    def forward(self, logits: torch.Tensor, targets: torch.Tensor) -> torch.Tensor:
        w = self.class_weights
        if w is not None:
            w = w.to(device=logits.device, dtype=logits.dtype)
        return F.cross_entropy(logits, targets, weight=w, label_smoothing=self.label_smoothing)


class CorrectionLoss(nn.Module):
    """Huber loss of the predicted depth correction, over the rows of ``mask`` (all rows without one); 0 for no rows."""

    def __init__(self, delta: float = 1.0):
        super().__init__()
        self.delta = delta

    def forward(self, predicted: torch.Tensor, target: torch.Tensor, mask: Optional[torch.Tensor] = None) -> torch.Tensor:
        if mask is not None:
            predicted, target = predicted[mask], target[mask]
        if predicted.shape[0] == 0:
            return torch.zeros((), device=predicted.device)
        return F.huber_loss(predicted, target, delta=self.delta)


class ConfidenceCalibrationLoss(nn.Module):
    """Binary cross-entropy of the confidence against "the predicted class is the true one"."""

    def __init__(self):
        super().__init__()

    def forward(self, confidence: torch.Tensor, predicted_class: torch.Tensor, true_class: torch.Tensor) -> torch.Tensor:
        hit = (predicted_class == true_class).to(confidence.dtype)
        return F.binary_cross_entropy(confidence, hit)


class FeaturePreservationLoss(nn.Module):
    """``penalty_weight`` times the share of nodes that are real features and were classified as noise."""

    def __init__(self, feature_class: int = 1, noise_class: int = 2, penalty_weight: float = 2.0):
        super().__init__()
        self.feature_class = feature_class
        self.noise_class = noise_class
        self.penalty_weight = penalty_weight

    def forward(self, predicted_class: torch.Tensor, true_class: torch.Tensor) -> torch.Tensor:
        lost = (true_class == self.feature_class) & (predicted_class == self.noise_class)
        return self.penalty_weight * lost.float().mean()


class ShoalSafetyLoss(nn.Module):
    """Penalty on seafloor classified as noise, heavier where the correction target is negative (depths positive down: the
    noisy sounding is shallower than the clean one, and removing a real shoal is the dangerous mistake): the mean of
    ``shoal_penalty`` / ``deep_penalty`` over the false positives, 0 without any."""

    def __init__(self, seafloor_class: int = 0, noise_class: int = 2, shoal_penalty: float = 3.0, deep_penalty: float = 1.0):
        super().__init__()
        self.seafloor_class = seafloor_class
        self.noise_class = noise_class
        self.shoal_penalty = shoal_penalty
        self.deep_penalty = deep_penalty

    def forward(self, predicted_class: torch.Tensor, true_class: torch.Tensor, correction_targets: torch.Tensor) -> torch.Tensor:
        fp = (true_class == self.seafloor_class) & (predicted_class == self.noise_class)
        shoal = fp & (correction_targets < 0)
        n_fp, n_shoal = fp.sum().float(), shoal.sum().float()
        # (no false positive: 0 / 1; the count never goes to the host)
        return (self.shoal_penalty * n_shoal + self.deep_penalty * (n_fp - n_shoal)) / torch.clamp(n_fp, min=1.0)


class _FusedLoss(torch.autograd.Function):
    """The six values of ``BathymetricGNNLoss`` as one autograd node.  Differentiable inputs: class_logits, confidence and (when
    present) correction; outputs: the terms in ``TERMS`` order, ``feature_preservation`` and ``shoal_safety`` not differentiable."""

    @staticmethod
    def forward(fctx, params, ctx, box, logits, confidence, correction, predicted, labels, targets, mask):
        n, dev = logits.shape[0], logits.device
        c = params.num_classes
        inp = rt.LossInputs(logits.data_ptr(), confidence.data_ptr(), None if correction is None else correction.data_ptr(),
                            predicted.data_ptr(), labels.data_ptr(), None if targets is None else targets.data_ptr(),
                            None if mask is None else mask.data_ptr())
        lib = ctx.lib
        ws_bytes = int(lib.bgnn_loss_workspace_bytes(n))
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
        terms = torch.empty(6, dtype=torch.float32, device=dev)
        counts = torch.empty(c * c + len(rt.LOSS_COUNTS), dtype=torch.int64, device=dev)
        ctx.begin()
        rt.check(lib.bgnn_loss_forward(ctx.handle, C.byref(params), n, C.byref(inp), rt.ptr(ws), ws_bytes, rt.ptr(terms),
                                       rt.ptr(counts)))
        ctx.end()
        box["counts"] = counts
        fctx.params, fctx.ctx, fctx.n = params, ctx, n
        fctx.save_for_backward(logits, confidence, correction, predicted, labels, targets, mask, ws)
        out = terms.unbind(0)
        fctx.mark_non_differentiable(out[3], out[4])
        return out

    @staticmethod
    @once_differentiable
    def backward(fctx, g_cls, g_corr, g_conf, g_feat, g_shoal, g_total):
        logits, confidence, correction, predicted, labels, targets, mask, ws = fctx.saved_tensors
        params, ctx, n = fctx.params, fctx.ctx, fctx.n
        tw = params.term_weights
        # d(loss) / d(classification, confidence, correction): the term's own upstream plus the total's share, on the device
        upstream = torch.stack((g_cls + g_total * tw[0], g_conf + g_total * tw[2], g_corr + g_total * tw[1])).to(torch.float32)
        need = fctx.needs_input_grad
        gl = torch.empty_like(logits) if need[3] else None
        gc = torch.empty_like(confidence) if need[4] else None
        gr = torch.empty_like(correction) if correction is not None and need[5] else None
        inp = rt.LossInputs(logits.data_ptr(), confidence.data_ptr(), None if correction is None else correction.data_ptr(),
                            predicted.data_ptr(), labels.data_ptr(), None if targets is None else targets.data_ptr(),
                            None if mask is None else mask.data_ptr())
        ctx.begin()
        rt.check(ctx.lib.bgnn_loss_backward(ctx.handle, C.byref(params), n, C.byref(inp), rt.ptr(ws), rt.ptr(upstream),
                                            rt.ptr(gl), rt.ptr(gc), rt.ptr(gr)))
        ctx.end()
        return None, None, None, gl, gc, gr, None, None, None, None


class BathymetricGNNLoss(nn.Module):
    """Combined multi-task loss for bathymetric GNN training: classification, correction (optional), confidence calibration,
    feature preservation and shoal safety, and ``total``, their sum under the five weights.

    After a call on the device path ``last_stats`` holds what the pass counted, as device tensors: ``confusion`` ([C, C] int64,
    rows true, columns predicted), ``n_masked``, ``false_positives``, ``shoal_false_positives``, ``deep_false_positives``,
    ``n_ignored``, ``n_invalid`` -- accuracy and the confusion matrix of the step without another pass.  It is None after a call
    on the torch path."""

    def __init__(
        self,
        class_weights: Optional[torch.Tensor] = None,
        classification_weight: float = 1.0,
        correction_weight: float = 0.5,
        confidence_weight: float = 0.2,
        feature_preservation_weight: float = 0.3,
        shoal_safety_weight: float = 0.5,
        label_smoothing: float = 0.0,
        correction_delta: float = 1.0,
    ):
        super().__init__()
        self.classification_loss = ClassificationLoss(class_weights=class_weights, label_smoothing=label_smoothing)
        self.correction_loss = CorrectionLoss(delta=correction_delta)
        self.confidence_loss = ConfidenceCalibrationLoss()
        self.feature_preservation_loss = FeaturePreservationLoss()
        self.shoal_safety_loss = ShoalSafetyLoss()
        self.classification_weight = classification_weight
        self.correction_weight = correction_weight
        self.confidence_weight = confidence_weight
        self.feature_preservation_weight = feature_preservation_weight
        self.shoal_safety_weight = shoal_safety_weight
        self.last_stats: Optional[Dict[str, torch.Tensor]] = None
        self._host_weights = None            # (tensor, version, list of floats): the class weights as the kernels take them

    # ---- the device path --------------------------------------------------------------------------------------------------
    def _class_weights_host(self):
        """The class weights as host floats.  Read from the device once per weight tensor (and again if it is modified in
        place), never per step."""
        w = self.classification_loss.class_weights
        if w is None:
            return None
        hw = self._host_weights
        if hw is None or hw[0] is not w or hw[1] != w._version:
            hw = self._host_weights = (w, w._version, [float(v) for v in w.detach().to("cpu", torch.float64).reshape(-1).tolist()])
        return hw[2]

    def _params(self, num_classes: int) -> rt.LossParams:
        p = rt.LossParams()
        p.num_classes = num_classes
        w = self._class_weights_host()
        p.has_class_weights = 0 if w is None else 1
        if w is not None:
            if len(w) != num_classes:
                raise ValueError(f"class_weights has {len(w)} entries, class_logits has {num_classes} classes")
            for i, v in enumerate(w):
                p.class_weights[i] = v
        p.label_smoothing = float(self.classification_loss.label_smoothing)
        p.delta = float(self.correction_loss.delta)
        f, s = self.feature_preservation_loss, self.shoal_safety_loss
        p.feature_class, p.feature_noise_class = int(f.feature_class), int(f.noise_class)
        p.seafloor_class, p.shoal_noise_class = int(s.seafloor_class), int(s.noise_class)
        p.penalty_weight, p.shoal_penalty, p.deep_penalty = float(f.penalty_weight), float(s.shoal_penalty), float(s.deep_penalty)
        for i, v in enumerate((self.classification_weight, self.correction_weight, self.confidence_weight,
                               self.feature_preservation_weight, self.shoal_safety_weight)):
            p.term_weights[i] = float(v)
        return p

    @staticmethod
    def _on_device_path(logits, confidence, correction) -> bool:
        ts = [logits, confidence] + ([correction] if correction is not None else [])
        return all(t.is_cuda and t.dtype == torch.float32 for t in ts) and logits.dim() == 2 and logits.shape[0] > 0

    def _forward_device(self, logits, confidence, correction, predicted, labels, targets, mask) -> Dict[str, torch.Tensor]:
        n, c = logits.shape
        if not 2 <= c <= MAX_CLASSES:
            raise ValueError(f"the fused loss takes 2 .. {MAX_CLASSES} classes, class_logits has {c}")
        if n > (1 << 30):
            raise NotImplementedError("the fused loss takes at most 2^30 rows")
        dev = logits.device
        ctx = rt.get_context(dev)

        def rows(t, dtype, what):
            t = t.detach().to(device=dev, dtype=dtype).reshape(-1).contiguous()
            if t.numel() != n:
                raise ValueError(f"{what} has {t.numel()} entries for {n} nodes")
            return t
        if confidence.numel() != n or (correction is not None and correction.numel() != n):
            raise ValueError(f"confidence / correction do not have one entry per node ({n})")
        predicted, labels = rows(predicted, torch.int64, "predicted_class"), rows(labels, torch.int64, "class_labels")
        if targets is not None:
            targets = rows(targets, torch.float32, "correction_targets")
        if mask is not None:
            if mask.dtype not in (torch.bool, torch.uint8):
                raise TypeError(f"noise_mask must be a bool (or uint8) tensor, got {mask.dtype}")
            mask = rows(mask, mask.dtype, "noise_mask")
            mask = mask.view(torch.uint8) if mask.dtype == torch.bool else mask
        if correction is None or targets is None:       # the correction term is absent: its gradient is not asked for
            corr_in = None if correction is None else correction.detach()
        else:
            corr_in = correction
        box = {}
        out = _FusedLoss.apply(self._params(c), ctx, box, logits.contiguous(), confidence.reshape(-1).contiguous(),
                               None if corr_in is None else corr_in.reshape(-1).contiguous(), predicted, labels, targets, mask)
        counts = box["counts"]
        self.last_stats = {"confusion": counts[:c * c].view(c, c), **{k: counts[c * c + i] for i, k in enumerate(rt.LOSS_COUNTS)}}
        return dict(zip(TERMS, out))

    # ---- reference API ----------------------------------------------------------------------------------------------------
    def forward(self, outputs: Dict[str, torch.Tensor], targets: Dict[str, torch.Tensor]) -> Dict[str, torch.Tensor]:
        """``outputs``: class_logits [N, C], predicted_class [N], confidence [N], correction [N] (optional).  ``targets``:
        class_labels [N], correction_targets [N] (optional), noise_mask [N] (optional).  Returns the five terms and ``total``
        as 0-dim tensors."""
        logits, confidence, correction = outputs["class_logits"], outputs["confidence"], outputs.get("correction")
        if self._on_device_path(logits, confidence, correction):
            return self._forward_device(logits, confidence, correction, outputs["predicted_class"], targets["class_labels"],
                                        targets.get("correction_targets"), targets.get("noise_mask"))
        return self.forward_torch(outputs, targets)

    def forward_torch(self, outputs: Dict[str, torch.Tensor], targets: Dict[str, torch.Tensor]) -> Dict[str, torch.Tensor]:
        """The same six values composed from the five component modules as separate torch operations, in the inputs' dtype and on
        their device: what ``forward`` runs for CPU tensors, other dtypes and an empty batch."""
        logits, confidence = outputs["class_logits"], outputs["confidence"]
        predicted, labels = outputs["predicted_class"], targets["class_labels"]
        correction, ctargets = outputs.get("correction"), targets.get("correction_targets")
        mask = targets.get("noise_mask")
        self.last_stats = None
        losses = {"classification": self.classification_loss(logits, labels)}
        zero = torch.zeros((), device=logits.device)
        if correction is not None and ctargets is not None:
            losses["correction"] = self.correction_loss(correction, ctargets, mask=mask)
        else:
            losses["correction"] = zero
        losses["confidence"] = self.confidence_loss(confidence, predicted, labels)
        losses["feature_preservation"] = self.feature_preservation_loss(predicted, labels)
        losses["shoal_safety"] = self.shoal_safety_loss(predicted, labels, ctargets) if ctargets is not None else zero
        losses["total"] = (self.classification_weight * losses["classification"] + self.correction_weight * losses["correction"] +
                           self.confidence_weight * losses["confidence"] +
                           self.feature_preservation_weight * losses["feature_preservation"] +
                           self.shoal_safety_weight * losses["shoal_safety"])
        return losses


def compute_class_weights(labels: torch.Tensor, num_classes: int = 3, smoothing: float = 0.1) -> torch.Tensor:
    """Inverse-frequency class weights on the labels' device: counts + smoothing * total, inverted, normalised to sum to
    ``num_classes``."""
    counts = torch.bincount(labels.reshape(-1), minlength=num_classes).float()
    smoothed = counts + smoothing * counts.sum()
    inverse = 1.0 / smoothed
    return inverse / inverse.sum() * num_classes


def compute_correction_delta(corrections, percentile: float = 95.0, min_delta: float = 1.0) -> float:
    """The Huber delta from the training data (host, numpy): the ``percentile`` of |corrections|, at least ``min_delta``, so that
    all but the tail of the corrections fall in the quadratic range; ``min_delta`` for an empty array.

    A float32 device tensor stays on the device (``huber_delta.device_percentile``: an exact selection, 104 bytes read back):
    the percentile of its finite entries as numpy gives it for the same values cast to float64."""
    if isinstance(corrections, torch.Tensor) and corrections.is_cuda:
        from .huber_delta import device_percentile
        value = device_percentile(corrections.detach().to(torch.float32), percentile, absolute=True)["values"][0]
        return min_delta if value is None else max(value, min_delta)
    corrections = np.asarray(corrections)
    if corrections.size == 0:
        return min_delta
    return max(float(np.percentile(np.abs(corrections), percentile)), min_delta)
