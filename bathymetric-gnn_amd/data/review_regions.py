"""Low-confidence regions for review: the reference's ``scripts/export_for_review.py`` (training plan, step 5.1) with the planes in HBM.

``export_review_regions`` takes the classification and confidence planes of a finished inference -- device tensors where they lie,
host arrays, or a ``SidecarBuilder`` -- keeps the cells with ``confidence_low <= confidence <= confidence_high`` whose confidence is
finite, labels their 4-connected regions (``scipy.ndimage.label``'s default structure), drops the regions below
``min_region_size`` and returns a ``ReviewRegions``: the reference's list of region dictionaries, the review mask as a device plane,
and the three bands its GeoTIFF holds.  Everything per cell runs as ``bgnn_review_regions`` (include/bgnn_review.h): a union-find
labelling, integer aggregates per region and an ordered compaction, with one read of the counts and the record table.

Against the reference: the bounds must lie in [0, 1] (the confidence is a sigmoid output; the device sums it in 32.32 fixed point),
and ``mean_confidence`` is that exact sum over the size, within 2^-33 of the true mean, where the reference rounds a float32 sum.
Reading the sidecar GeoTIFF and writing the 3-band review GeoTIFF (GDAL) stay with the reference: ``bands()`` are the arrays to
write, ``save_json`` writes the region list as the reference does."""
from __future__ import annotations

import ctypes as C
import json
import math
from typing import Any, Dict, List, Optional

import numpy as np
import torch

from .. import runtime as rt

FIRST_CAPACITY_MAX = 1 << 16       # records of the first call's table (40 bytes each); a second call follows when more regions are kept


def check_bounds(confidence_low, confidence_high, min_region_size):
    """The float32 bounds the device compares with, as numpy rounds a Python float against a float32 array.  ``ValueError`` for
    bounds that are not finite, not ordered or outside [0, 1], and for ``min_region_size < 1``."""
    low, high = np.float32(confidence_low), np.float32(confidence_high)
    if not (math.isfinite(confidence_low) and math.isfinite(confidence_high)) or not (0.0 <= low <= high <= 1.0):
        raise ValueError(f"confidence bounds [{confidence_low}, {confidence_high}]: finite, ordered and inside [0, 1] expected")
    if int(min_region_size) != min_region_size or int(min_region_size) < 1:
        raise ValueError(f"min_region_size {min_region_size}: an integer >= 1 expected")
    return low, high, int(min_region_size)


def check_shape(shape):
    """``(rows, cols)`` of a confidence plane; ``NotImplementedError`` beyond ``runtime.RV_MAX_CELLS``."""
    if len(shape) != 2:
        raise ValueError(f"confidence has shape {tuple(shape)}: a [rows, cols] plane expected")
    rows, cols = int(shape[0]), int(shape[1])
    if rows < 1 or cols < 1:
        raise ValueError(f"a grid of {rows} x {cols}")
    if rows * cols > rt.RV_MAX_CELLS:
        raise NotImplementedError(f"{rows} x {cols} cells exceed the limit of {rt.RV_MAX_CELLS} (int32 region labels)")
    return rows, cols


def regions_from_records(records: np.ndarray) -> List[Dict[str, Any]]:
    """The reference's list of region dictionaries from a record table on the host (``runtime.RV_RECORD_DTYPE``, in the device's
    order): ``id`` from 1, ``mean_confidence`` the fixed-point sum over the size (one correctly rounded division)."""
    return [{"id": k + 1,
             "size": int(r["size"]),
             "mean_confidence": int(r["conf_sum"]) / (int(r["size"]) << 32),
             "bounds": {"min_row": int(r["min_row"]), "max_row": int(r["max_row"]),
                        "min_col": int(r["min_col"]), "max_col": int(r["max_col"])}}
            for k, r in enumerate(records)]


class ReviewRegions:
    """What ``export_review_regions`` found.

    ``regions``      the reference's list: ``id``, ``size``, ``mean_confidence``, ``bounds`` (``min_row``, ``max_row``, ``min_col``,
                     ``max_col``, inclusive), in ``ndimage.label``'s order
    ``records``      the device's record table on the host (``runtime.RV_RECORD_DTYPE``), one entry per region
    ``review_mask``  float32 device plane: 1 on the cells of the kept regions, 0 elsewhere
    ``counts``       ``uncertain_cells``, ``regions`` (all 4-connected regions of the uncertain cells), ``kept_regions``, ``kept_cells``
    ``confidence``, ``classification``   the planes as used (device tensors) / as given (``classification`` is only passed through)"""

    def __init__(self, records, counts, review_mask, confidence, classification):
        self.records = records
        self.regions = regions_from_records(records)
        self.counts = counts
        self.review_mask = review_mask
        self.confidence = confidence
        self.classification = classification

    def __len__(self):
        return len(self.regions)

    def bands(self) -> list:
        """The three bands of the reference's review GeoTIFF as host arrays, in its order: ``review_mask``, ``confidence``,
        ``classification`` (``None`` when none was given)."""
        host = lambda p: None if p is None else (p.cpu().numpy() if isinstance(p, torch.Tensor) else np.asarray(p))
        return [host(self.review_mask), host(self.confidence), host(self.classification)]

    def save_json(self, path) -> None:
        """The region list as the reference saves it beside the GeoTIFF."""
        with open(path, "w") as f:
            json.dump(self.regions, f, indent=2)


def review_regions_build(confidence: torch.Tensor, low, high, min_region_size: int, capacity: int, review_mask: Optional[torch.Tensor],
                         ctx=None) -> torch.Tensor:
    """``bgnn_review_regions`` on a contiguous float32 device plane: an int64 device tensor holding ``counts [4]``, then
    ``capacity`` records (``runtime.RV_RECORD_DTYPE``).  Asynchronous on the context's stream, ordered against the caller's
    current stream."""
    dev = confidence.device
    ctx = ctx if ctx is not None else rt.get_context(dev)
    for name, t in (("confidence", confidence), ("review_mask", review_mask)):
        if t is not None and (t.dtype != torch.float32 or t.device != dev or not t.is_contiguous() or t.shape != confidence.shape):
            raise TypeError(f"{name} must be a contiguous float32 tensor of shape {tuple(confidence.shape)} on {dev}")
    rows, cols = check_shape(confidence.shape)
    ws_bytes = int(ctx.lib.bgnn_review_workspace_bytes(rows, cols))
    ws = torch.empty((ws_bytes + 7) // 8, dtype=torch.int64, device=dev)
    out = torch.empty(rt.RV_COUNTS + capacity * (rt.RV_RECORD_BYTES // 8), dtype=torch.int64, device=dev)
    base = out.data_ptr()
    ctx.begin()
    rt.check(ctx.lib.bgnn_review_regions(ctx.handle, rt.ptr(confidence), rows, cols, C.c_float(low), C.c_float(high), min_region_size,
                                         rt.ptr(ws), C.c_size_t(ws.numel() * 8),
                                         C.c_void_p(base + 8 * rt.RV_COUNTS) if capacity > 0 else None, capacity, C.c_void_p(base),
                                         rt.ptr(review_mask)))
    ctx.end()
    return out


def split_result(host: np.ndarray):
    """``(counts, records)`` from the host copy of what ``review_regions_build`` returned: the four counts as a dictionary, the
    written part of the record table."""
    counts = {k: int(v) for k, v in zip(rt.RV_COUNT_NAMES, host[:rt.RV_COUNTS])}
    table = host[rt.RV_COUNTS:].view(rt.RV_RECORD_DTYPE)
    return counts, table[:min(counts["kept_regions"], len(table))].copy()


def _planes_of(classification, confidence):
    """A ``SidecarBuilder`` alone stands for its two planes: the device planes after a device run, else the host planes."""
    if confidence is None and hasattr(classification, "planes_device"):
        builder = classification
        dev = builder.planes_device()
        if dev is not None:
            return dev[0], dev[1]
        return builder.classification, builder.confidence
    if confidence is None:
        raise ValueError("a confidence plane, or a SidecarBuilder as the only argument, expected")
    return classification, confidence


def export_review_regions(classification, confidence=None, confidence_low: float = 0.4, confidence_high: float = 0.7,
                          min_region_size: int = 100, device=None, first_capacity: Optional[int] = None) -> ReviewRegions:
    """The reference's ``export_review_regions`` (export_for_review.py) with its parameters and defaults, on planes instead of
    files.  ``classification`` and ``confidence`` are ``[rows, cols]`` device tensors (used where they lie) or host arrays
    (uploaded); ``classification`` may be ``None`` -- it is only passed through to ``bands()`` -- or a ``SidecarBuilder``, given
    alone.  One synchronisation: the read of the counts and the record table.  When more regions are kept than the first table
    holds (``cells // min_region_size``, at most ``FIRST_CAPACITY_MAX``; ``first_capacity`` overrides it), the call runs once more
    with a table of the reported size.  Raises ``ValueError`` for bounds outside [0, 1] or ``low > high``, ``NotImplementedError``
    for a raster beyond ``runtime.RV_MAX_CELLS`` cells."""
    classification, confidence = _planes_of(classification, confidence)
    low, high, min_region_size = check_bounds(confidence_low, confidence_high, min_region_size)
    rows, cols = check_shape(confidence.shape)
    if classification is not None and tuple(classification.shape) != (rows, cols):
        raise ValueError(f"classification has shape {tuple(classification.shape)}, confidence {(rows, cols)}")
    if device is None and isinstance(confidence, torch.Tensor) and confidence.is_cuda:
        device = confidence.device
    device = rt.resolve_device(device)
    if isinstance(confidence, torch.Tensor):
        conf = confidence.to(device=device, dtype=torch.float32).contiguous()      # (no copy where it already is all that)
    else:
        conf = torch.from_numpy(np.array(confidence, dtype=np.float32, order="C")).to(device)
    mask = torch.empty((rows, cols), dtype=torch.float32, device=device)
    capacity = first_capacity if first_capacity is not None else min(rows * cols // min_region_size, FIRST_CAPACITY_MAX)
    capacity = max(1, int(capacity))
    counts, records = split_result(review_regions_build(conf, low, high, min_region_size, capacity, mask).cpu().numpy())
    if counts["kept_regions"] > capacity:
        counts, records = split_result(review_regions_build(conf, low, high, min_region_size, counts["kept_regions"], mask).cpu().numpy())
    if len(records) != counts["kept_regions"]:
        raise rt.BgnnError(f"{counts['kept_regions']} regions kept, {len(records)} records read")
    return ReviewRegions(records, counts, mask, conf, classification)
