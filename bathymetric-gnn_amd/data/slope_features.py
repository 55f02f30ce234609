"""Slope-based feature labels (class 1): the reference's ``scripts/prepare_feature_labels.py`` (training plan, phase 3) with the
survey plane in HBM.

``create_feature_mask_from_slope`` marks the cells whose slope, from ``numpy.gradient`` of the raw float32 plane (nodata and NaN
included), exceeds ``slope_threshold`` degrees, labels their 4-connected clusters (``scipy.ndimage.label``'s default structure) and
clears the clusters below ``min_cluster_size``.  ``add_feature_labels`` turns that mask into a label plane (-1 no data, 0 seafloor,
1 feature) and paints a disc of ``wreck_radius`` pixels around every known wreck.  Everything per cell runs as
``bgnn_slope_features`` (include/bgnn_slope.h): a union-find labelling with integer sizes; the discs go through the existing
``rasterize_features`` in overlay mode.

The threshold reaches the device as a *cut*: ``s = gx * gx + gy * gy`` is three float32 operations the device reproduces bit for
bit, and ``degrees(arctan(sqrt(s)))`` is monotone in ``s``, so ``slope_cut`` finds, with this machine's numpy, the smallest float32
``s`` whose slope exceeds the threshold; the kernel tests ``s >= cut`` and needs no transcendental.

Reading the wrecks shapefile (``load_wrecks_shapefile``, OGR) and the GeoTIFF writer stay with the reference:
``FeatureLabels.bands()`` hands its writer the two bands."""
from __future__ import annotations

import ctypes as C
import logging
import operator
from typing import Any, Dict, Optional, Sequence, Tuple

import numpy as np
import torch

from .. import runtime as rt
from .feature_labels import FEATURE_LABELS_NODATA, FeatureLabels, _plane_to_device, rasterize_features
from .grid import BathymetricGrid

logger = logging.getLogger(__name__)

_INF_BITS = 0x7F800000


def _exceeds(bits: int, slope_threshold: float) -> bool:
    """The reference's predicate on the float32 with these bits standing for ``gx**2 + gy**2``, evaluated by numpy on a
    one-element float32 array as the reference evaluates it on the plane."""
    s = np.array([bits], dtype=np.uint32).view(np.float32)
    with np.errstate(all="ignore"):
        return bool((np.degrees(np.arctan(np.sqrt(s))) > slope_threshold)[0])


def slope_cut(slope_threshold: float) -> np.float32:
    """The smallest non-negative float32 ``s`` with ``np.degrees(np.arctan(np.sqrt(np.float32(s)))) > slope_threshold``: a
    bisection over the non-negative bit patterns up to +inf (31 steps; ``sqrt``, ``arctan`` and ``degrees`` are monotone).  NaN
    when no ``s`` qualifies (a threshold of 90 or more, or NaN): the mask is then empty.  0 when ``s = 0`` qualifies (a negative
    threshold): every cell with a non-NaN ``s`` is then in the mask."""
    slope_threshold = float(slope_threshold)          # (a Python float: numpy compares it in float32, as in the reference)
    if not _exceeds(_INF_BITS, slope_threshold):
        return np.float32(np.nan)
    if _exceeds(0, slope_threshold):
        return np.float32(0.0)
    lo, hi = 0, _INF_BITS                             # the predicate is false at lo, true at hi
    while hi - lo > 1:
        mid = (lo + hi) // 2
        if _exceeds(mid, slope_threshold):
            hi = mid
        else:
            lo = mid
    return np.array([hi], dtype=np.uint32).view(np.float32)[0]


def _check_plane_shape(shape) -> Tuple[int, int]:
    if len(shape) != 2:
        raise ValueError(f"the depth plane has shape {tuple(shape)}, a [H, W] plane is needed")
    rows, cols = int(shape[0]), int(shape[1])
    if rows < 2 or cols < 2:
        # numpy.gradient's refusal, in its words
        raise ValueError("Shape of array too small to calculate a numerical gradient, at least (edge_order + 1) elements are "
                         f"required: the plane is {rows} x {cols}")
    if rows * cols > rt.SL_MAX_CELLS:
        raise NotImplementedError(f"{rows} x {cols} cells exceed the limit of {rt.SL_MAX_CELLS} (int32 cluster labels)")
    return rows, cols


def slope_features_build(depth: torch.Tensor, cut, min_cluster_size: int, base_labels: Optional[torch.Tensor] = None,
                         want_mask: bool = True, nodata: float = FEATURE_LABELS_NODATA, ctx=None):
    """``bgnn_slope_features`` on a contiguous float32 device plane: ``(labels, slope_mask or None, stats_block)``: int32
    ``[H, W]``, uint8 ``[H, W]`` and int64 ``[6]`` (``runtime.SL_STATS_NAMES``).  ``base_labels`` (int32, same shape) selects overlay
    mode: only zeros may become 1.  Asynchronous on the context's stream, ordered against the caller's current stream."""
    if not isinstance(depth, torch.Tensor) or depth.dtype != torch.float32 or not depth.is_cuda or not depth.is_contiguous():
        raise TypeError("depth must be a contiguous float32 tensor on a GPU")
    rows, cols = _check_plane_shape(depth.shape)
    dev = depth.device
    if base_labels is not None and (not isinstance(base_labels, torch.Tensor) or base_labels.dtype != torch.int32
                                    or base_labels.device != dev or not base_labels.is_contiguous()
                                    or base_labels.shape != depth.shape):
        raise TypeError(f"base_labels must be a contiguous int32 tensor of shape {tuple(depth.shape)} on {dev}")
    min_cluster_size = operator.index(min_cluster_size)
    ctx = ctx if ctx is not None else rt.get_context(dev)
    ws_bytes = int(ctx.lib.bgnn_slope_features_workspace_bytes(rows, cols))
    ws = torch.empty((ws_bytes + 3) // 4, dtype=torch.int32, device=dev)
    labels = torch.empty((rows, cols), dtype=torch.int32, device=dev)
    mask = torch.empty((rows, cols), dtype=torch.uint8, device=dev) if want_mask else None
    stats = torch.empty(rt.SL_STATS, dtype=torch.int64, device=dev)
    ctx.begin()
    rt.check(ctx.lib.bgnn_slope_features(ctx.handle, rt.ptr(depth), rt.ptr(base_labels), rows, cols, float(nodata),
                                         C.c_float(float(cut)), min_cluster_size, rt.ptr(ws), C.c_size_t(ws.numel() * 4),
                                         rt.ptr(labels), rt.ptr(mask), rt.ptr(stats)))
    ctx.end()
    return labels, mask, stats


def slope_stats(stats_block: torch.Tensor) -> Dict[str, int]:
    """The six counts of a slope statistics block by name (``runtime.SL_STATS_NAMES``; synchronises)."""
    return {k: int(v) for k, v in zip(rt.SL_STATS_NAMES, stats_block.cpu().tolist())}


def _resolve(depth, device):
    if isinstance(depth, torch.Tensor) and depth.is_cuda and device is None:
        device = depth.device
    return rt.resolve_device(device)


def create_feature_mask_from_slope(depth, slope_threshold: float = 15.0, min_cluster_size: int = 100, device=None) -> torch.Tensor:
    """The reference's ``create_feature_mask_from_slope`` with its parameters and defaults: the boolean mask of the steep cells in
    clusters of at least ``min_cluster_size`` cells, invalid cells included, as a device tensor.  ``depth`` is a ``[H, W]`` host
    array or device tensor (a float32 plane already on the device is not copied).  ``ValueError`` for an axis shorter than 2, as
    ``numpy.gradient`` raises."""
    _check_plane_shape(depth.shape)
    plane = _plane_to_device(depth, _resolve(depth, device))
    _, mask, _ = slope_features_build(plane, slope_cut(slope_threshold), min_cluster_size)
    return mask.view(torch.bool)


def _xy(wreck) -> Tuple[float, float]:
    if isinstance(wreck, dict):
        return wreck["x"], wreck["y"]
    return wreck.x, wreck.y


def wreck_pixel_table(wrecks: Sequence[Any], transform, shape, wreck_radius: int = 50) -> Tuple[np.ndarray, int]:
    """The host arithmetic of the reference's ``add_feature_labels``: ``(table, count)`` with ``table`` int32
    ``[F', 4] = (row, col, radius, 1)`` of the wrecks whose centre lies on the grid, in list order, and their number (the
    reference's "Added N wrecks").  ``wrecks`` are dictionaries or objects with ``x`` and ``y``.  ``col`` and ``row`` are Python
    ``int()`` of the float64 quotient: they truncate towards zero, so a centre up to one pixel left of or above the origin lands
    in column or row 0, as in the reference.  ``wreck_radius`` is in pixels and an integer (``TypeError`` otherwise); it is clamped
    to ``rows + cols``, beyond which the disc covers the grid anyway."""
    radius = operator.index(wreck_radius)
    gt = transform
    rows, cols = int(shape[0]), int(shape[1])
    radius = min(radius, rows + cols, 2 ** 31 - 1)
    if radius < -(2 ** 31):
        raise ValueError("the radius does not fit int32")
    out = []
    for wreck in wrecks:
        x, y = _xy(wreck)
        col = int((x - gt[0]) / gt[1])
        row = int((y - gt[3]) / gt[5])
        if 0 <= row < rows and 0 <= col < cols:
            out.append((row, col, radius, 1))
    return np.ascontiguousarray(np.asarray(out, dtype=np.int64).reshape(-1, 4), dtype=np.int32), len(out)


def add_feature_labels(survey, wrecks: Optional[Sequence[Any]] = None, slope_threshold: float = 15.0, wreck_radius: int = 50,
                       min_cluster_size: int = 100, transform=None, device=None) -> FeatureLabels:
    """The reference's ``add_feature_labels`` without the file I/O.  ``survey`` is a ``BathymetricGrid`` (its ``transform`` and
    ``crs`` are used unless ``transform`` is given), a ``[H, W]`` host array or a device tensor; a transform is needed only when
    ``wrecks`` are given.  Labels: -1 where the depth is 1.0e6 or not finite, 1 on the valid cells of the filtered slope mask and
    inside a disc of ``wreck_radius`` pixels around every wreck whose centre lies on the grid, else 0.  The result is a
    ``FeatureLabels``: ``applied_features`` is the wreck count, ``bands()`` the two bands the script writes, ``slope_stats()`` the
    counts of the slope step.  A plane already on the device is not copied; nothing synchronises until ``stats()``,
    ``slope_stats()`` or ``bands()``."""
    crs = None
    if isinstance(survey, BathymetricGrid):
        depth, crs = survey.depth, survey.crs
        transform = survey.transform if transform is None else transform
    else:
        depth = survey
    radius = operator.index(wreck_radius)
    if wrecks and transform is None:
        raise ValueError("a geotransform is needed to place the wrecks: pass transform= or a BathymetricGrid that has one")
    _check_plane_shape(depth.shape)
    plane = _plane_to_device(depth, _resolve(depth, device))
    logger.info("Computing slope-based features...")
    labels, _, block = slope_features_build(plane, slope_cut(slope_threshold), min_cluster_size, want_mask=False)
    applied = 0
    if wrecks:
        table, applied = wreck_pixel_table(wrecks, transform, tuple(plane.shape), radius)
        labels, stats = rasterize_features(table, base_labels=labels)
        logger.info(f"Added {applied} wrecks from database")
    else:
        # the block rasterize_features would write with an empty table: valid cells, cells labelled 1, painted cells
        stats = torch.stack([block[0], block[5], torch.zeros_like(block[0])])
    return FeatureLabels(labels, plane, None if transform is None else tuple(transform), crs, applied, stats, slope_block=block)
