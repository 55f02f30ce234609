"""Model evaluation on the device: the reference's ``scripts/evaluate_model.py::compute_metrics`` over planes that stay in HBM.

``Evaluator`` owns one accumulator block of ``bgnn_eval_accumulate`` (include/bgnn_eval.h): every integer the reference counts
(total, correct, the confusion matrix over the classes 0 / 1 / 2 / ">= 3", coverage at the five confidence thresholds) and the
float64 sums behind its confidence statistics, added up over as many calls as the caller likes -- row bands of one survey, or
several surveys.  ``metrics()`` copies the block to the host once and ``metrics_from_block`` forms the reference's dictionary from
it: the ratios of integers are exactly numpy's (``tp / (tp + fp)``, ``np.mean(bool)``) below 2^53 cells; the confidence means and
standard deviation come from float64 sums where the reference uses float32 pairwise sums."""
from __future__ import annotations

import ctypes as C
import math
from typing import Any, Dict, Optional

import numpy as np
import torch

from .. import runtime as rt

CLASS_NAMES = ["seafloor", "feature", "noise"]


def metrics_from_block(block, with_confidence: Optional[bool] = None) -> Dict[str, Any]:
    """The dictionary of the reference's ``compute_metrics`` from an accumulator block on the host (a record of
    ``runtime.EVAL_ACC_DTYPE``).  ``with_confidence`` None: the confidence part is present when every counted cell came with a
    confidence (``conf_cells == total``), as it is when the reference is given a confidence plane."""
    total, correct = int(block["total"]), int(block["correct"])
    m = np.asarray(block["confusion"], dtype=np.int64).reshape(4, 4)
    metrics: Dict[str, Any] = {
        "total_samples": total,
        "overall_accuracy": correct / total if total > 0 else float("nan"),       # np.mean of an empty array
    }
    for k, name in enumerate(CLASS_NAMES):
        true_pos = int(m[k, k])
        false_pos = int(m[:, k].sum()) - true_pos
        false_neg = int(m[k, :].sum()) - true_pos
        precision = true_pos / (true_pos + false_pos) if (true_pos + false_pos) > 0 else 0
        recall = true_pos / (true_pos + false_neg) if (true_pos + false_neg) > 0 else 0
        f1 = 2 * precision * recall / (precision + recall) if (precision + recall) > 0 else 0
        metrics[name] = {
            "true_positives": true_pos,
            "false_positives": false_pos,
            "false_negatives": false_neg,
            "precision": float(precision),
            "recall": float(recall),
            "f1": float(f1),
            "support": int(m[k, :].sum()),
        }
    metrics["confusion_matrix"] = [[int(v) for v in row] for row in m[:3, :3]]
    if with_confidence is None:
        with_confidence = int(block["conf_cells"]) == total
    if with_confidence and total > 0:
        if int(block["conf_cells"]) != total:
            raise ValueError("confidence statistics need a confidence plane in every call that was accumulated")
        incorrect = total - correct
        mean_c = float(block["conf_sum"]) / total
        var = float(block["conf_sq"]) / total - mean_c * mean_c
        conf: Dict[str, Any] = {
            "mean": 0.5 + mean_c,
            "std": math.sqrt(var) if var > 0 else (float("nan") if var != var else 0.0),
            "mean_correct": 0.5 + float(block["conf_correct_sum"]) / correct if correct > 0 else 0,
            "mean_incorrect": 0.5 + float(block["conf_incorrect_sum"]) / incorrect if incorrect > 0 else 0,
        }
        for j, thresh in enumerate(rt.EVAL_THRESHOLDS):
            covered = int(block["covered"][j])
            if covered > 0:
                conf[f"accuracy_at_{thresh}"] = int(block["covered_correct"][j]) / covered
                conf[f"coverage_at_{thresh}"] = covered / total
        metrics["confidence"] = conf
    return metrics


def _labels_to_device(y, device) -> torch.Tensor:
    """Labels as the int32 plane the kernel takes.  A float plane (band 1 of a ground-truth raster) is masked as the reference
    masks it -- ``y >= 0`` on the floats, then truncated -- with -1 standing for what the comparison drops."""
    t = y if isinstance(y, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(np.asarray(y)))
    t = t.to(device)
    if t.dtype.is_floating_point:
        t = torch.where(t >= 0, t, torch.full_like(t, -1.0))
    elif t.dtype == torch.bool:
        t = t.to(torch.uint8)
    return t.to(torch.int32).contiguous().view(-1)


def _plane_to_device(p, device) -> torch.Tensor:
    t = p if isinstance(p, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(np.asarray(p)))
    return t.to(device=device, dtype=torch.float32).contiguous().view(-1)


class Evaluator:
    """``add(labels, classification, confidence=None)`` as often as needed, then ``metrics()``.  The planes are host arrays or
    device tensors of one shape: labels as integers (or the float band of a ground-truth raster), classification and confidence as
    floats -- rows 0 and 1 of the ``[4, H, W]`` output of ``process_survey_device`` as they stand (NaN where nothing was
    predicted)."""

    def __init__(self, device=None):
        self.device = rt.resolve_device(device)
        self._ctx = rt.get_context(self.device)
        self._acc = torch.zeros(rt.EVAL_ACC_BYTES // 8, dtype=torch.int64, device=self.device)
        self._ws = None
        self._calls = 0
        self._conf_calls = 0

    def reset(self):
        ctx = self._ctx
        ctx.begin()
        rt.check(ctx.lib.bgnn_eval_reset(ctx.handle, rt.ptr(self._acc)))
        ctx.end()
        self._calls = self._conf_calls = 0

    def add(self, labels, classification, confidence=None):
        """Count one set of planes into the block.  No host wait."""
        y = _labels_to_device(labels, self.device)
        p = _plane_to_device(classification, self.device)
        c = None if confidence is None else _plane_to_device(confidence, self.device)
        if p.numel() != y.numel() or (c is not None and c.numel() != y.numel()):
            raise ValueError(f"planes disagree on the number of cells: labels {y.numel()}, classification {p.numel()}"
                             + ("" if c is None else f", confidence {c.numel()}"))
        self._calls += 1
        self._conf_calls += c is not None
        cells = y.numel()
        if cells == 0:
            return
        ctx = self._ctx
        need = int(ctx.lib.bgnn_eval_workspace_bytes(cells))
        if self._ws is None or self._ws.numel() * 8 < need:
            self._ws = torch.empty((need + 7) // 8, dtype=torch.int64, device=self.device)
        ctx.begin()
        rt.check(ctx.lib.bgnn_eval_accumulate(ctx.handle, rt.ptr(y), rt.ptr(p), rt.ptr(c), cells, rt.ptr(self._ws),
                                              C.c_size_t(self._ws.numel() * 8), rt.ptr(self._acc)))
        ctx.end()

    def block(self):
        """The accumulator block on the host (``runtime.EVAL_ACC_DTYPE``): the one device-to-host copy."""
        raw = self._acc.cpu().numpy().tobytes()
        return np.frombuffer(raw, dtype=np.dtype(rt.EVAL_ACC_DTYPE))[0]

    def metrics(self) -> Dict[str, Any]:
        """The reference's ``compute_metrics`` dictionary over everything added since the last ``reset``.  The confidence part is
        there when every ``add`` came with a confidence plane."""
        return metrics_from_block(self.block(), with_confidence=self._calls > 0 and self._conf_calls == self._calls)


def compute_metrics(y_true, y_pred, confidence=None, device=None) -> Dict[str, Any]:
    """Drop-in for the reference's ``compute_metrics(y_true, y_pred, confidence=None)``: the same keys and Python types, counted
    on the device.  Inputs are host arrays or device tensors."""
    if device is None:
        for t in (y_true, y_pred, confidence):
            if isinstance(t, torch.Tensor) and t.is_cuda:
                device = t.device
                break
    ev = Evaluator(device)
    ev.add(y_true, y_pred, confidence)
    return ev.metrics()
