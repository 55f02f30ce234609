"""Operating curves on the device: what every confidence threshold would select, from planes that stay in HBM.

The reference's documents ask for this after each training run and do it by hand: ``docs/LESSONS_LEARNED.md`` ("Run inference at
0.5 threshold, review sidecar ... then adjust based on false positive rate", "Track precision/recall separately; tune
classification threshold"), its "Visual Validation Checklist" step 5 ("Create a diff layer (predicted corrections minus actual
difference) to quantify residual error"), ``docs/HOW_IT_WORKS.md`` "Operational Confidence Thresholds" (``auto_correct_threshold``,
``review_threshold``) and ``docs/TRAINING_PLAN.md`` "Metrics to Track" (noise precision > 0.90, recall > 0.85).

``OperatingCurve`` owns one block of ``bgnn_curve_accumulate`` (include/bgnn_curve.h): a histogram of the counted cells over
(confidence code, true class, predicted class) with fixed-point sums of the residual before and after the predicted correction
beside it, added up over as many calls as the caller likes.  The code of a confidence ``c`` against the table ``t`` is
``2 * #{k : t_k < c} + [c == t_k]`` (``2T + 1`` for NaN), so ``c > t_k``, ``c >= t_k`` and ``c < t_k`` are exact functions of it and
one pass answers every threshold.  ``curve()`` copies the block to the host once; ``curve_from_block`` forms every figure from its
integers: ratios of Python ints, so equal to numpy's on the same masks; mean absolute errors exact to the 1/65536 m of the fixed
point.  Limits: 1 .. 128 thresholds, at most 2^32 counted cells per block, residuals of 32768 m and more enter no sum."""
from __future__ import annotations

from typing import Any, Dict, List, Optional

import numpy as np
import torch

from .. import runtime as rt
from .evaluation import CLASS_NAMES, _labels_to_device, _plane_to_device

WG_CELLS = rt.CURVE_WG_CELLS           # the cells of one workgroup's share (BGNN_CURVE_WG_CELLS)
MAX_THRESHOLDS = rt.CURVE_MAX_THRESHOLDS


def default_thresholds() -> np.ndarray:
    """``np.linspace(0, 1, 101)`` as float32, duplicates after rounding removed."""
    return np.unique(np.linspace(0, 1, 101).astype(np.float32))


def check_thresholds(thresholds) -> np.ndarray:
    """The table as the kernel takes it: a float32 vector of 1 .. 128 finite, strictly increasing entries (compared after the
    rounding to float32).  ``ValueError`` otherwise."""
    if isinstance(thresholds, torch.Tensor):
        thresholds = thresholds.detach().cpu().numpy()
    t = np.asarray(thresholds)
    if t.ndim != 1 or t.dtype == object or not (np.issubdtype(t.dtype, np.floating) or np.issubdtype(t.dtype, np.integer)):
        raise ValueError("thresholds: a vector of numbers expected")
    if not 1 <= t.size <= MAX_THRESHOLDS:
        raise ValueError(f"thresholds: {t.size} entries, 1 .. {MAX_THRESHOLDS} expected")
    with np.errstate(over="ignore"):
        t = np.ascontiguousarray(t, dtype=np.float32)
    if not np.isfinite(t).all():
        raise ValueError("thresholds: every entry must be finite")
    if not (t[1:] > t[:-1]).all():
        raise ValueError("thresholds: strictly increasing float32 values expected (duplicates after rounding to float32 count)")
    return t


def curve_accumulate(thresholds: torch.Tensor, labels: torch.Tensor, classification: torch.Tensor, confidence: torch.Tensor,
                     difference: Optional[torch.Tensor], correction: Optional[torch.Tensor], block: torch.Tensor, ctx=None):
    """``bgnn_curve_accumulate`` on device tensors: ``thresholds`` float32 (already checked: ``check_thresholds``), ``labels``
    int32, the other planes float32, all contiguous, on the block's device and of one number of cells; ``block`` int64 of
    ``bgnn_curve_block_bytes(T) / 8`` entries.  Asynchronous on the context's stream, ordered against the caller's current stream."""
    dev = block.device
    ctx = ctx if ctx is not None else rt.get_context(dev)
    if (difference is None) != (correction is None):
        raise ValueError("difference and correction must both be given or both be None")
    planes = [("thresholds", thresholds, torch.float32), ("labels", labels, torch.int32), ("classification", classification, torch.float32),
              ("confidence", confidence, torch.float32), ("difference", difference, torch.float32),
              ("correction", correction, torch.float32), ("block", block, torch.int64)]
    for name, t, dtype in planes:
        if t is None:
            continue
        if not isinstance(t, torch.Tensor) or t.dtype != dtype or t.device != dev or not t.is_contiguous():
            raise TypeError(f"{name} must be a contiguous {dtype} tensor on {dev}")
    n_thr, cells = thresholds.numel(), labels.numel()
    if thresholds.dim() != 1 or not 1 <= n_thr <= MAX_THRESHOLDS:
        raise ValueError(f"thresholds: {n_thr} entries, 1 .. {MAX_THRESHOLDS} expected")
    if block.numel() * 8 != int(ctx.lib.bgnn_curve_block_bytes(n_thr)):
        raise ValueError(f"block of {block.numel() * 8} bytes, {int(ctx.lib.bgnn_curve_block_bytes(n_thr))} expected for {n_thr} thresholds")
    for name, t, _ in planes[2:6]:
        if t is not None and t.numel() != cells:
            raise ValueError(f"planes disagree on the number of cells: labels {cells}, {name} {t.numel()}")
    if cells == 0:
        return
    ctx.begin()
    rt.check(ctx.lib.bgnn_curve_accumulate(ctx.handle, rt.ptr(thresholds), n_thr, rt.ptr(labels), rt.ptr(classification),
                                           rt.ptr(confidence), rt.ptr(difference), rt.ptr(correction), cells, rt.ptr(block)))
    ctx.end()


def _ratio(num: int, den: int):
    return num / den if den > 0 else 0


def curve_from_block(block, thresholds, with_residual: Optional[bool] = None) -> Dict[str, Any]:
    """Every figure of the curve from a block on the host (a record of ``runtime.curve_block_dtype(T)``) and its table.  Lists of
    length T, entry k for threshold ``t_k``:

    ``auto_correct`` (predicted noise with ``conf > t``, what the pipeline corrects): ``cells``, ``true_noise``, ``on_seafloor``,
    ``on_feature`` (the feature-protection count), ``precision``, ``recall`` (against the noise support), ``f1``, ``share_of_valid``.
    ``review`` (``conf < t``): ``cells``, ``share``, ``errors_caught`` (the misclassified cells inside), ``errors_caught_share``.
    ``coverage`` (``conf >= t``): ``coverage``, ``accuracy`` -- ``Evaluator``'s ``coverage_at_*`` / ``accuracy_at_*`` for any t.
    ``residual`` (when every counted cell came with residual planes; ``with_residual`` None decides by the block):
    ``mae_before``, ``mae_after[k]`` = (base_abs + the sum over the auto-corrected cells of abs_after - abs_before) / base_cells /
    65536, ``corrected_cells[k]``, ``per_class`` (the same per true class: the benefit on true noise, the damage on true seafloor
    and feature), ``skipped``.

    And the totals that need no threshold: ``total``, ``confusion_matrix`` (4 x 4: classes 0, 1, 2, ">= 3"), ``support``,
    ``nan_confidence_cells``.  A cell is an error when its clamped classes differ.  Ratios are ratios of Python ints, 0 for an
    empty denominator."""
    thr = check_thresholds(thresholds)
    T = thr.size
    counts = np.asarray(block["counts"], dtype=np.int64).reshape(2 * T + 2, 4, 4)
    ranked = counts[:2 * T + 1]                                 # (the last code holds the NaN confidences: in no set)
    zero = np.zeros((1, 4, 4), np.int64)
    above = np.concatenate([np.cumsum(ranked[::-1], axis=0)[::-1], zero])      # above[c]: codes c .. 2T
    below = np.concatenate([zero, np.cumsum(ranked, axis=0)])                  # below[c]: codes 0 .. c - 1
    confusion = counts.sum(axis=0)
    total = int(confusion.sum())
    errors = total - int(np.trace(confusion))
    noise_support = int(confusion[2].sum())
    auto: Dict[str, List] = {k: [] for k in ("cells", "true_noise", "on_seafloor", "on_feature", "precision", "recall", "f1",
                                             "share_of_valid")}
    review: Dict[str, List] = {k: [] for k in ("cells", "share", "errors_caught", "errors_caught_share")}
    coverage: Dict[str, List] = {k: [] for k in ("coverage", "accuracy")}
    for k in range(T):
        a = above[2 * k + 2][:, 2]                              # conf > t_k, predicted noise, by true class
        cells, true_noise = int(a.sum()), int(a[2])
        precision, recall = _ratio(true_noise, cells), _ratio(true_noise, noise_support)
        f1 = 2 * precision * recall / (precision + recall) if (precision + recall) > 0 else 0
        for name, v in (("cells", cells), ("true_noise", true_noise), ("on_seafloor", int(a[0])), ("on_feature", int(a[1])),
                        ("precision", float(precision)), ("recall", float(recall)), ("f1", float(f1)),
                        ("share_of_valid", float(_ratio(cells, total)))):
            auto[name].append(v)
        r = below[2 * k + 1]                                    # conf < t_k: codes 0 .. 2k
        r_cells = int(r.sum())
        caught = r_cells - int(np.trace(r))
        for name, v in (("cells", r_cells), ("share", float(_ratio(r_cells, total))), ("errors_caught", caught),
                        ("errors_caught_share", float(_ratio(caught, errors)))):
            review[name].append(v)
        c = above[2 * k + 1]                                    # conf >= t_k
        covered = int(c.sum())
        coverage["coverage"].append(float(_ratio(covered, total)))
        coverage["accuracy"].append(float(_ratio(int(np.trace(c)), covered)))
    out: Dict[str, Any] = {
        "thresholds": [float(t) for t in thr],
        "total": total,
        "confusion_matrix": [[int(v) for v in row] for row in confusion],
        "support": {name: int(confusion[j].sum()) for j, name in enumerate(CLASS_NAMES)},
        "nan_confidence_cells": int(counts[2 * T + 1].sum()),
        "auto_correct": auto,
        "review": review,
        "coverage": coverage,
    }
    base_cells = [int(v) for v in block["base_cells"]]
    base_abs = [int(v) for v in block["base_abs"]]
    skipped = int(block["res_skipped"])
    if with_residual is None:
        with_residual = total > 0 and sum(base_cells) + skipped == total
    if with_residual:
        if sum(base_cells) + skipped != total:
            raise ValueError("residual figures need the residual planes in every call that was accumulated")
        res_cells = np.asarray(block["res_cells"], dtype=np.int64).reshape(2 * T + 2, 4)[:2 * T + 1]
        gain = (np.asarray(block["abs_after"], dtype=np.int64) - np.asarray(block["abs_before"], dtype=np.int64)).reshape(2 * T + 2, 4)
        zero4 = np.zeros((1, 4), np.int64)
        gain_above = np.concatenate([np.cumsum(gain[:2 * T + 1][::-1], axis=0)[::-1], zero4])
        res_above = np.concatenate([np.cumsum(res_cells[::-1], axis=0)[::-1], zero4])
        scale = rt.CURVE_RES_SCALE

        def mae(q: int, n: int):
            return float(_ratio(q, n) / scale)

        per_class = {}
        for j, name in enumerate(CLASS_NAMES):
            per_class[name] = {
                "cells": base_cells[j],
                "mae_before": mae(base_abs[j], base_cells[j]),
                "mae_after": [mae(base_abs[j] + int(gain_above[2 * k + 2][j]), base_cells[j]) for k in range(T)],
                "corrected_cells": [int(res_above[2 * k + 2][j]) for k in range(T)],
            }
        out["residual"] = {
            "cells": sum(base_cells),
            "mae_before": mae(sum(base_abs), sum(base_cells)),
            "mae_after": [mae(sum(base_abs) + int(gain_above[2 * k + 2].sum()), sum(base_cells)) for k in range(T)],
            "corrected_cells": [int(res_above[2 * k + 2].sum()) for k in range(T)],
            "per_class": per_class,
            "skipped": skipped,
        }
    return out


def recommend_thresholds(curve: Dict[str, Any], min_noise_precision: float = 0.90,
                         max_review_share: Optional[float] = None) -> Dict[str, Any]:
    """The two policy knobs of ``docs/HOW_IT_WORKS.md`` read off a curve, against ``docs/TRAINING_PLAN.md`` "Metrics to Track"
    (noise precision > 0.90 beside recall > 0.85: the precision is the bound here, the recall that comes with it is reported).

    ``auto_correct_threshold``: the smallest threshold whose auto-corrected set is not empty and has a noise precision of at least
    ``min_noise_precision`` -- the one with the highest recall among those that qualify, since the set only shrinks as the
    threshold grows; None when no threshold qualifies.  ``precision`` / ``recall`` are that threshold's (None with it).
    With ``max_review_share``: ``review_threshold``, the largest threshold whose review set (``conf < t``) holds at most that share
    of the counted cells; None when even the smallest holds more.  Pure host logic."""
    thr, auto = curve["thresholds"], curve["auto_correct"]
    out: Dict[str, Any] = {"auto_correct_threshold": None, "precision": None, "recall": None}
    for k, t in enumerate(thr):
        if auto["cells"][k] > 0 and auto["precision"][k] >= min_noise_precision:
            out.update(auto_correct_threshold=t, precision=auto["precision"][k], recall=auto["recall"][k])
            break
    if max_review_share is not None:
        out["review_threshold"] = None
        out["review_share"] = None
        for k, t in enumerate(thr):
            if curve["review"]["share"][k] <= max_review_share:
                out.update(review_threshold=t, review_share=curve["review"]["share"][k])
    return out


class OperatingCurve:
    """``add(labels, classification, confidence, difference=None, correction=None)`` as often as needed, then ``curve()``.  The
    planes are host arrays or device tensors of one shape: labels as integers (``GroundTruth.labels``) or the float band of a
    ground-truth raster (masked as ``Evaluator`` masks it), the others as floats -- rows 0, 1 and 2 of the ``[4, H, W]`` output of
    ``process_survey_device`` and ``GroundTruth.difference`` as they stand (NaN where nothing was predicted or measured).
    ``thresholds``: 1 .. 128 finite, strictly increasing values (``ValueError`` otherwise); ``np.linspace(0, 1, 101)`` by default."""

    def __init__(self, thresholds=None, device=None):
        self.thresholds = check_thresholds(default_thresholds() if thresholds is None else thresholds)
        self.device = rt.resolve_device(device)
        self._ctx = rt.get_context(self.device)
        self._thr = torch.from_numpy(self.thresholds.copy()).to(self.device)
        self._dtype = np.dtype(rt.curve_block_dtype(self.thresholds.size))
        nbytes = int(self._ctx.lib.bgnn_curve_block_bytes(self.thresholds.size))
        assert nbytes == self._dtype.itemsize
        self._block = torch.zeros(nbytes // 8, dtype=torch.int64, device=self.device)
        self._calls = 0
        self._res_calls = 0

    def reset(self):
        ctx = self._ctx
        ctx.begin()
        rt.check(ctx.lib.bgnn_curve_reset(ctx.handle, rt.ptr(self._block), self.thresholds.size))
        ctx.end()
        self._calls = self._res_calls = 0

    def add(self, labels, classification, confidence, difference=None, correction=None):
        """Count one set of planes into the block.  No host wait."""
        if (difference is None) != (correction is None):
            raise ValueError("difference and correction must both be given or both be None")
        shapes = {name: tuple(p.shape if hasattr(p, "shape") else np.shape(p)) for name, p in (("labels", labels), ("classification", classification),
                                                       ("confidence", confidence), ("difference", difference),
                                                       ("correction", correction)) if p is not None}
        if len(set(shapes.values())) != 1:
            raise ValueError(f"planes of one shape expected: {shapes}")
        y = _labels_to_device(labels, self.device)
        p = _plane_to_device(classification, self.device)
        c = _plane_to_device(confidence, self.device)
        d = None if difference is None else _plane_to_device(difference, self.device)
        r = None if correction is None else _plane_to_device(correction, self.device)
        curve_accumulate(self._thr, y, p, c, d, r, self._block, ctx=self._ctx)
        self._calls += 1
        self._res_calls += d is not None

    def block(self):
        """The block on the host (``runtime.curve_block_dtype(T)``): the one device-to-host copy."""
        raw = self._block.cpu().numpy().tobytes()
        return np.frombuffer(raw, dtype=self._dtype)[0]

    def curve(self) -> Dict[str, Any]:
        """``curve_from_block`` over everything added since the last ``reset``; the residual part is there when every ``add`` came
        with the residual planes."""
        return curve_from_block(self.block(), self.thresholds, with_residual=self._calls > 0 and self._res_calls == self._calls)
