"""Ground truth from a clean / noisy survey pair: the reference's ``scripts/prepare_ground_truth.py`` with the planes in HBM.

``align_survey_pair`` is the host arithmetic of ``find_intersection`` / ``extract_region`` (a handful of scalars);
``compute_ground_truth`` runs the per-cell part -- the raw difference, the validity mask, the exact median of the difference over
every valid cell, the labels, the masked planes and the statistics -- as ``bgnn_ground_truth_build`` (include/bgnn_eval.h): a radix
selection on the device, no sort and no host round trip.  Reading the surveys and writing the GeoTIFF (GDAL) stay with the
reference: ``GroundTruth.bands()`` hands its writer the five bands, ``GroundTruth.training_planes()`` hands
``TileStore.from_ground_truth`` the device planes."""
from __future__ import annotations

import ctypes as C
import dataclasses
from typing import Any, Dict, List, NamedTuple, Optional, Tuple

import numpy as np
import torch

from .. import runtime as rt
from .grid import BathymetricGrid

CLASS_SEAFLOOR, CLASS_FEATURE, CLASS_NOISE = 0, 1, 2
GROUND_TRUTH_NODATA = 1.0e6          # prepare_ground_truth.py:163 (the script's own constant, not the grid's nodata_value)


class Alignment(NamedTuple):
    """The overlap of a survey pair: ``(row_start, row_end, col_start, col_end)`` in either grid, already cut to the common
    shape, and the geotransform of the cut (the clean survey's)."""
    clean_window: Tuple[int, int, int, int]
    noisy_window: Tuple[int, int, int, int]
    shape: Tuple[int, int]
    transform: Tuple[float, float, float, float, float, float]


def find_intersection(bounds1, bounds2):
    """``(min_x, min_y, max_x, max_y)`` of the overlap of two such boxes, or None (prepare_ground_truth.py:39-52)."""
    min_x = max(bounds1[0], bounds2[0])
    min_y = max(bounds1[1], bounds2[1])
    max_x = min(bounds1[2], bounds2[2])
    max_y = min(bounds1[3], bounds2[3])
    if min_x < max_x and min_y < max_y:
        return (min_x, min_y, max_x, max_y)
    return None


def _region_window(shape, transform, intersection):
    """The index window ``extract_region`` slices (prepare_ground_truth.py:65-94) and the transform of its corner."""
    min_x, min_y, max_x, max_y = intersection
    res_x = abs(transform[1])
    res_y = abs(transform[5])
    origin_x = transform[0]
    origin_y = transform[3]
    col_start = int(round((min_x - origin_x) / res_x))
    col_end = int(round((max_x - origin_x) / res_x))
    row_start = int(round((origin_y - max_y) / res_y))
    row_end = int(round((origin_y - min_y) / res_y))
    col_start = max(0, col_start)
    col_end = min(shape[1], col_end)
    row_start = max(0, row_start)
    row_end = min(shape[0], row_end)
    new_transform = (origin_x + col_start * res_x, transform[1], transform[2], origin_y - row_start * res_y, transform[4], transform[5])
    # (a slice whose end lies before its start is empty)
    return row_start, max(row_end, row_start), col_start, max(col_end, col_start), new_transform


def align_survey_pair(clean: BathymetricGrid, noisy: BathymetricGrid) -> Alignment:
    """Where a clean and a noisy survey overlap (prepare_ground_truth.py:124-155): the intersection of their bounds, the
    resolution check, each grid's window by ``extract_region``'s rounding and clamping, and the crop of both to the smaller
    shape.  Raises ``ValueError`` with the reference's messages."""
    intersection = find_intersection(clean.bounds, noisy.bounds)
    if intersection is None:
        raise ValueError("Surveys do not overlap geographically")
    clean_res = clean.resolution
    noisy_res = noisy.resolution
    if abs(clean_res[0] - noisy_res[0]) > 0.01 or abs(clean_res[1] - noisy_res[1]) > 0.01:
        raise ValueError(
            f"Resolution mismatch: clean {clean_res} vs noisy {noisy_res}. "
            "Surveys must have the same resolution."
        )
    cr0, cr1, cc0, cc1, transform = _region_window(tuple(clean.depth.shape), clean.transform, intersection)
    nr0, nr1, nc0, nc1, _ = _region_window(tuple(noisy.depth.shape), noisy.transform, intersection)
    rows = min(cr1 - cr0, nr1 - nr0)
    cols = min(cc1 - cc0, nc1 - nc0)
    return Alignment((cr0, cr0 + rows, cc0, cc0 + cols), (nr0, nr0 + rows, nc0, nc0 + cols), (rows, cols), transform)


def ground_truth_stats(block, noise_threshold: float, grid_shape, clean_survey: str = "None", noisy_survey: str = "None") -> Dict[str, Any]:
    """The reference's statistics JSON (prepare_ground_truth.py:268-281) from a statistics block on the host (a record of
    ``runtime.GT_STATS_DTYPE``).  The counts and the maximum are the reference's own; ``mean_noise_magnitude`` is the float64 sum
    over the count where the reference takes a float32 pairwise mean."""
    valid, noise, seafloor = int(block["valid"]), int(block["noise"]), int(block["seafloor"])
    stats = {
        "clean_survey": str(clean_survey),
        "noisy_survey": str(noisy_survey),
        "noise_threshold": noise_threshold,
        "grid_shape": [int(v) for v in grid_shape],
        "valid_cells": valid,
        "noise_cells": noise,
        "noise_percentage": float(100 * noise / valid) if valid > 0 else 0,
        "seafloor_cells": seafloor,
    }
    if noise > 0:
        stats["mean_noise_magnitude"] = float(block["noise_abs_sum"]) / noise
        stats["max_noise_magnitude"] = float(block["noise_abs_max"])
    return stats


@dataclasses.dataclass
class GroundTruth:
    """What ``compute_ground_truth`` leaves on the device: ``[H, W]`` tensors (``labels`` int32, the rest float32; ``uncertainty``
    None when the noisy survey has none), the cut's ``transform`` / ``crs``, and the statistics block."""
    labels: torch.Tensor
    difference: torch.Tensor
    noisy_depth: torch.Tensor
    clean_depth: torch.Tensor
    uncertainty: Optional[torch.Tensor]
    transform: Any
    crs: Any
    noise_threshold: float
    stats_block: torch.Tensor            # int64 [6] holding the BGNN_GT_STATS_BYTES of the block
    clean_survey: str = "None"
    noisy_survey: str = "None"
    _host_block: Any = None
    applied_features: Optional[int] = None          # set by with_features: the features that were applied ...
    feature_block: Optional[torch.Tensor] = None    # ... and the statistics block of that call (int64 [3], runtime.FL_STATS_DTYPE)
    slope_block: Optional[torch.Tensor] = None      # set by with_slope_features: int64 [6], runtime.SL_STATS_NAMES

    def block(self):
        """The statistics block on the host (``runtime.GT_STATS_DTYPE``).  The first call synchronises; later ones do not."""
        if self._host_block is None:
            raw = self.stats_block.cpu().numpy().tobytes()
            self._host_block = np.frombuffer(raw, dtype=np.dtype(rt.GT_STATS_DTYPE))[0]
        return self._host_block

    def stats(self) -> Dict[str, Any]:
        """The reference's ``*_ground_truth_stats.json`` dictionary."""
        return ground_truth_stats(self.block(), self.noise_threshold, self.labels.shape, self.clean_survey, self.noisy_survey)

    @property
    def systematic_offset(self) -> float:
        """The median that was removed (NaN without a valid cell)."""
        return float(self.block()["offset"])

    @property
    def seafloor_mean_difference(self) -> float:
        """The reference's "should be ~0" log line (NaN without a seafloor cell)."""
        b = self.block()
        return float(b["seafloor_sum"]) / int(b["seafloor"]) if int(b["seafloor"]) > 0 else float("nan")

    def bands(self) -> List[np.ndarray]:
        """The five float32 host arrays the reference writes as bands 1-5: labels, difference, noisy depth, clean depth,
        uncertainty (all NaN without one)."""
        unc = (np.full(tuple(self.labels.shape), np.nan, dtype=np.float32) if self.uncertainty is None
               else self.uncertainty.cpu().numpy())
        return [self.labels.to(torch.float32).cpu().numpy(), self.difference.cpu().numpy(), self.noisy_depth.cpu().numpy(),
                self.clean_depth.cpu().numpy(), unc]

    def training_planes(self):
        """``(labels, difference, noisy_depth, uncertainty)``: the leading arguments of ``TileStore.from_ground_truth``."""
        return self.labels, self.difference, self.noisy_depth, self.uncertainty

    def with_features(self, features, feature_radius: Optional[Dict[str, float]] = None) -> "GroundTruth":
        """This ground truth with charted features painted over its seafloor (``feature_labels``, overlay mode, with this ground
        truth's own ``transform``): a cell labelled 0 inside a feature's disc takes the feature's label (class 1); noise (2) and
        no data (-1) stay what they are.  Only ``labels`` is new, the other planes are shared, not copied.  ``stats()`` of the
        result is that of the pair as prepared; the feature counts come from ``feature_stats()``."""
        from .feature_labels import feature_pixel_table, rasterize_features
        table, applied = feature_pixel_table(features, self.transform, tuple(self.labels.shape), feature_radius)
        labels, block = rasterize_features(table, base_labels=self.labels)
        return dataclasses.replace(self, labels=labels, applied_features=applied, feature_block=block)

    def feature_stats(self) -> Dict[str, int]:
        """``{"applied_features", "feature_cells", "valid_cells", "painted_cells"}`` of ``with_features`` (synchronises)."""
        if self.feature_block is None:
            raise ValueError("no features were applied: this ground truth does not come from with_features")
        from .feature_labels import feature_stats
        return feature_stats(self.feature_block, self.applied_features)

    def with_slope_features(self, slope_threshold: float = 15.0, min_cluster_size: int = 100,
                            source: str = "clean_depth") -> "GroundTruth":
        """This ground truth with steep terrain painted over its seafloor (``slope_features``, overlay mode): the slope comes from
        the depth plane named by ``source`` (``"clean_depth"`` or ``"noisy_depth"``); a cell labelled 0 in a cluster of at least
        ``min_cluster_size`` steep cells becomes class 1; noise (2) and no data (-1) stay what they are.  Only ``labels`` is new,
        the other planes are shared, not copied.  The counts come from ``slope_stats()``."""
        from .slope_features import slope_cut, slope_features_build
        if source not in ("clean_depth", "noisy_depth"):
            raise ValueError(f"source {source!r}: 'clean_depth' or 'noisy_depth' expected")
        labels, _, block = slope_features_build(getattr(self, source), slope_cut(slope_threshold), min_cluster_size,
                                                base_labels=self.labels, want_mask=False)
        return dataclasses.replace(self, labels=labels, slope_block=block)

    def slope_stats(self) -> Dict[str, int]:
        """The counts of ``with_slope_features`` by name (``runtime.SL_STATS_NAMES``; synchronises)."""
        if self.slope_block is None:
            raise ValueError("no slope step: this ground truth does not come from with_slope_features")
        from .slope_features import slope_stats
        return slope_stats(self.slope_block)

    def analyze(self, **kw) -> Dict[str, Any]:
        """The reference's noise pattern analysis of this ground truth (``noise_analysis.analyze_noise_patterns``)."""
        from .noise_analysis import analyze_noise_patterns
        return analyze_noise_patterns(self, **kw)


def _window_to_device(plane, window, device) -> torch.Tensor:
    r0, r1, c0, c1 = window
    if isinstance(plane, torch.Tensor):
        return plane[r0:r1, c0:c1].to(device=device, dtype=torch.float32).contiguous()
    return torch.from_numpy(np.ascontiguousarray(np.asarray(plane)[r0:r1, c0:c1], dtype=np.float32)).to(device)


def ground_truth_build(clean_depth: torch.Tensor, noisy_depth: torch.Tensor, noisy_unc: Optional[torch.Tensor] = None,
                       noise_threshold: float = 0.15, nodata: float = GROUND_TRUTH_NODATA, ctx=None):
    """``bgnn_ground_truth_build`` on float32 device planes of one shape: ``(labels, difference, uncertainty or None,
    stats_block)``.  Asynchronous on the context's stream, ordered against the caller's current stream."""
    dev = clean_depth.device
    ctx = ctx if ctx is not None else rt.get_context(dev)
    for name, t in (("clean", clean_depth), ("noisy", noisy_depth), ("uncertainty", noisy_unc)):
        if t is None:
            continue
        if t.dtype != torch.float32 or t.device != dev or not t.is_contiguous():
            raise TypeError(f"{name} must be a contiguous float32 tensor on {dev}")
        if t.shape != clean_depth.shape:
            raise ValueError(f"{name} has shape {tuple(t.shape)}, clean {tuple(clean_depth.shape)}")
    cells = clean_depth.numel()
    labels = torch.empty(clean_depth.shape, dtype=torch.int32, device=dev)
    difference = torch.empty(clean_depth.shape, dtype=torch.float32, device=dev)
    unc_out = None if noisy_unc is None else torch.empty_like(noisy_unc)
    stats = torch.zeros(rt.GT_STATS_BYTES // 8, dtype=torch.int64, device=dev)
    if cells == 0:
        stats.view(torch.float32)[10] = float("nan")          # the offset of an empty selection
        return labels, difference, unc_out, stats
    ws_bytes = int(ctx.lib.bgnn_ground_truth_workspace_bytes(cells))
    ws = torch.empty((ws_bytes + 7) // 8, dtype=torch.int64, device=dev)
    ctx.begin()
    rt.check(ctx.lib.bgnn_ground_truth_build(ctx.handle, rt.ptr(clean_depth), rt.ptr(noisy_depth), rt.ptr(noisy_unc), cells,
                                             float(nodata), float(noise_threshold), rt.ptr(ws), C.c_size_t(ws.numel() * 8),
                                             rt.ptr(labels), rt.ptr(difference), rt.ptr(unc_out), rt.ptr(stats)))
    ctx.end()
    return labels, difference, unc_out, stats


def compute_ground_truth(clean: BathymetricGrid, noisy: BathymetricGrid, noise_threshold: float = 0.15, device=None) -> GroundTruth:
    """The reference's ``compute_ground_truth`` from two loaded surveys (prepare_ground_truth.py:124-255, without the file I/O):
    ``depth`` / ``uncertainty`` of either grid may be host arrays or device tensors.  The overlap is cut on the host
    (``align_survey_pair``), everything per cell runs on the device; nothing synchronises until ``stats()`` or ``bands()``."""
    device = rt.resolve_device(device)
    al = align_survey_pair(clean, noisy)
    clean_depth = _window_to_device(clean.depth, al.clean_window, device)
    noisy_depth = _window_to_device(noisy.depth, al.noisy_window, device)
    noisy_unc = None if noisy.uncertainty is None else _window_to_device(noisy.uncertainty, al.noisy_window, device)
    labels, difference, unc, stats = ground_truth_build(clean_depth, noisy_depth, noisy_unc, noise_threshold)
    return GroundTruth(labels, difference, noisy_depth, clean_depth, unc, al.transform, clean.crs, noise_threshold, stats,
                       str(clean.source_path), str(noisy.source_path))
