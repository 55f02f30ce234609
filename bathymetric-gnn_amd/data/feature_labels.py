"""Feature labels (class 1) from charted objects: the reference's ``scripts/extract_s57_features.py::create_feature_labels`` with
the survey plane in HBM.

Every charted wreck, rock and obstruction paints a disc of ``ceil(radius_m / resolution)`` pixels of its class's label onto the
survey grid; later features overwrite earlier ones.  ``feature_pixel_table`` is the reference's float64 geo arithmetic, on the host
and written as the reference writes it (radius, centre by ``int()`` truncation, bounds check, label lookup): a handful of scalars
per feature.  ``rasterize_features`` runs the per-cell part as ``bgnn_feature_labels`` (include/bgnn_features.h): a host plan that
lists, per 64 x 64 bin, the features that can show there, and one kernel that gathers each cell's label from its bin's list.

Two modes.  *Depth mode* is the reference's function: validity comes from the depth plane.  *Overlay mode* is this package's
extension (the reference has no merge step): the input is an existing label plane, e.g. a ground truth's, and **only cells whose
label is 0 (seafloor) may be painted**; ``-1`` (no data) and ``2`` (noise) pass through unchanged.  Noise stays noise because a
noise label is a measured disagreement between two surveys at that cell while a charted disc is a generous circle around a
position of chart accuracy; no data stays no data as in the reference.

Querying ENC Direct (REST), reading S-57 files (OGR), ``features_to_geojson`` and the GeoTIFF writer stay with the reference:
``FeatureLabels.bands()`` hands its writer the two bands.  Nothing here opens a network connection."""
from __future__ import annotations

import ctypes as C
import dataclasses
import logging
from dataclasses import asdict, dataclass
from typing import Any, Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from .. import runtime as rt
from .grid import BathymetricGrid

logger = logging.getLogger(__name__)

FEATURE_LABELS_NODATA = 1.0e6        # extract_s57_features.py:825 (the function's own constant, not the grid's nodata_value)

# S-57 object classes relevant for bathymetric feature training (extract_s57_features.py:413-439)
FEATURE_CLASSES = {
    "WRECKS": {"description": "Wrecks", "label": 1, "default_radius": 50},
    "UWTROC": {"description": "Underwater rocks", "label": 1, "default_radius": 25},
    "OBSTRN": {"description": "Obstructions", "label": 1, "default_radius": 30},
    "SBDARE": {"description": "Seabed area", "label": None, "default_radius": 0},      # context, not direct labeling
    "SOUNDG": {"description": "Soundings", "label": None, "default_radius": 0},        # validation points
}


@dataclass
class S57Feature:
    """Represents a feature extracted from S-57 ENC or REST API."""
    object_class: str
    geometry_type: str
    x: float
    y: float
    depth: Optional[float] = None
    attributes: Optional[Dict] = None
    wkt: Optional[str] = None

    def to_dict(self):
        return asdict(self)


def feature_pixel_table(features: Sequence[Any], transform, shape, feature_radius: Optional[Dict[str, float]] = None,
                        feature_classes: Optional[Dict[str, Dict]] = None) -> Tuple[np.ndarray, int]:
    """The host arithmetic of ``create_feature_labels`` (extract_s57_features.py:833-862): ``(table, applied_count)`` with
    ``table`` int32 ``[F', 4] = (row, col, radius_px, label)`` of the applied features in list order.

    A feature is skipped when its centre falls outside the grid, and also when its class's label is ``None``; neither is counted.
    ``col`` and ``row`` are Python ``int()`` of the float64 quotient: they truncate towards zero, so a centre up to one pixel left
    of or above the origin lands in column or row 0, as in the reference.  ``radius_px`` is clamped to ``rows + cols`` (beyond that
    the disc covers the grid anyway; to ``2**31 - 1`` on the one shape where that is smaller); a negative radius stays negative:
    such a feature paints nothing and is still counted.  ``feature_classes`` replaces ``FEATURE_CLASSES`` (tests)."""
    classes = FEATURE_CLASSES if feature_classes is None else feature_classes
    gt = transform
    rows, cols = int(shape[0]), int(shape[1])
    resolution = abs(gt[1])
    rmax = min(rows + cols, 2 ** 31 - 1)
    out: List[Tuple[int, int, int, int]] = []
    for f in features:
        obj_class = f.object_class
        if feature_radius and obj_class in feature_radius:
            radius_m = feature_radius[obj_class]
        else:
            radius_m = classes.get(obj_class, {}).get("default_radius", 30)
        radius_px = int(np.ceil(radius_m / resolution))
        col = int((f.x - gt[0]) / gt[1])
        row = int((f.y - gt[3]) / gt[5])
        if row < 0 or row >= rows or col < 0 or col >= cols:
            continue
        label_value = classes.get(obj_class, {}).get("label", 1)
        if label_value is not None:
            out.append((row, col, min(radius_px, rmax), int(label_value)))
    table = np.asarray(out, dtype=np.int64).reshape(-1, 4)
    if table.size and (np.abs(table) > 2 ** 31 - 1).any():
        raise ValueError("a radius or a label does not fit int32")
    return np.ascontiguousarray(table, dtype=np.int32), len(out)


def feature_plan(table: np.ndarray, shape) -> Tuple[np.ndarray, np.ndarray]:
    """The host plan of ``table`` on a grid of ``shape`` (``bgnn_feature_labels_plan``; needs no GPU): ``(bin_ptr, bin_feat)``,
    int64 ``[bins + 1]`` and int32 ``[entries]``, views of one buffer.  Bin ``b`` (row-major over ``ceil(rows / 64) x
    ceil(cols / 64)``) looks at the features ``bin_feat[bin_ptr[b]:bin_ptr[b + 1]]``, in descending index."""
    raw, bins = _plan_buffer(table, shape)
    bin_ptr = raw[:bins + 1]
    return bin_ptr, raw[bins + 1:].view(np.int32)[:int(bin_ptr[bins])]


def _check_table(table) -> np.ndarray:
    table = np.asarray(table)
    if table.dtype != np.int32 or table.ndim != 2 or table.shape[1] != 4:
        raise TypeError("table must be an int32 array of shape [F, 4]")
    return np.ascontiguousarray(table)


def _plan_buffer(table: np.ndarray, shape):
    lib = rt.load_library()
    table = _check_table(table)
    rows, cols = int(shape[0]), int(shape[1])
    n = table.shape[0]
    tp = table.ctypes.data_as(C.c_void_p) if n else None
    nbytes = int(lib.bgnn_feature_labels_plan_bytes(tp, n, rows, cols))
    raw = np.zeros((nbytes + 7) // 8 if nbytes else 1, dtype=np.int64)
    rt.check(lib.bgnn_feature_labels_plan(tp, n, rows, cols, raw.ctypes.data_as(C.c_void_p), C.c_size_t(raw.nbytes)))
    return raw, -(-rows // rt.FL_BIN) * -(-cols // rt.FL_BIN)


def rasterize_features(table: np.ndarray, depth: Optional[torch.Tensor] = None, base_labels: Optional[torch.Tensor] = None,
                       nodata: float = FEATURE_LABELS_NODATA, ctx=None):
    """``bgnn_feature_labels`` on a device plane: ``(labels, stats_block)``, int32 ``[H, W]`` and int64 ``[3]`` (valid cells,
    cells labelled 1, painted cells: ``runtime.FL_STATS_DTYPE``).  Exactly one of ``depth`` (float32: depth mode, the reference's
    function) and ``base_labels`` (int32: overlay mode, only zeros are painted; -1 and 2 pass through) is given; ``table`` is the
    int32 ``[F, 4]`` host array of ``feature_pixel_table``.  Asynchronous on the context's stream, ordered against the caller's
    current stream.  An empty plane returns without a launch."""
    if (depth is None) == (base_labels is None):
        raise ValueError("exactly one of depth and base_labels is given")
    plane, want = (depth, torch.float32) if depth is not None else (base_labels, torch.int32)
    name = "depth" if depth is not None else "base_labels"
    if not isinstance(plane, torch.Tensor) or plane.dtype != want or not plane.is_cuda or not plane.is_contiguous():
        raise TypeError(f"{name} must be a contiguous {str(want).replace('torch.', '')} tensor on a GPU")
    if plane.dim() != 2:
        raise ValueError(f"{name} has shape {tuple(plane.shape)}, a [H, W] plane is needed")
    table = _check_table(table)
    dev = plane.device
    labels = torch.empty(plane.shape, dtype=torch.int32, device=dev)
    stats = torch.zeros(rt.FL_STATS_BYTES // 8, dtype=torch.int64, device=dev)
    if plane.numel() == 0:
        return labels, stats
    ctx = ctx if ctx is not None else rt.get_context(dev)
    rows, cols = plane.shape
    n = table.shape[0]
    raw, _ = _plan_buffer(table, (rows, cols))
    ws_bytes = int(ctx.lib.bgnn_feature_labels_workspace_bytes(n, C.c_size_t(raw.nbytes)))
    ws = torch.empty((ws_bytes + 7) // 8, dtype=torch.int64, device=dev)
    ctx.begin()
    rt.check(ctx.lib.bgnn_feature_labels(ctx.handle, rt.ptr(depth), rt.ptr(base_labels), rows, cols, float(nodata),
                                         table.ctypes.data_as(C.c_void_p) if n else None, n, raw.ctypes.data_as(C.c_void_p),
                                         C.c_size_t(raw.nbytes), rt.ptr(ws), C.c_size_t(ws.numel() * 8), rt.ptr(labels),
                                         rt.ptr(stats)))
    ctx.end()
    return labels, stats


def feature_stats(stats_block: torch.Tensor, applied_features: int) -> Dict[str, int]:
    """``{"applied_features", "feature_cells", "valid_cells", "painted_cells"}`` from a statistics block (synchronises)."""
    b = np.frombuffer(stats_block.cpu().numpy().tobytes(), dtype=np.dtype(rt.FL_STATS_DTYPE))[0]
    return {"applied_features": int(applied_features), "feature_cells": int(b["feature"]), "valid_cells": int(b["valid"]),
            "painted_cells": int(b["painted"])}


@dataclasses.dataclass
class FeatureLabels:
    """What ``create_feature_labels`` leaves on the device: ``labels`` (int32 ``[H, W]``: -1 no data, 0 seafloor, else the class
    label of the last feature whose disc holds the cell), the survey's ``depth`` plane (float32, as given), its ``transform`` /
    ``crs`` and the number of applied features (the reference's "Applied N feature labels")."""
    labels: torch.Tensor
    depth: torch.Tensor
    transform: Any
    crs: Any
    applied_features: int
    stats_block: torch.Tensor = None      # int64 [3] holding the BGNN_FL_STATS_BYTES of the block
    _host_stats: Any = None
    slope_block: torch.Tensor = None      # set by slope_features.add_feature_labels: int64 [6], runtime.SL_STATS_NAMES

    def slope_stats(self) -> Dict[str, int]:
        """The counts of the slope step of ``add_feature_labels``: valid cells, steep cells, clusters, kept clusters, their cells
        and the cells labelled 1 from the slope (the reference's "Slope-based features").  Synchronises."""
        if self.slope_block is None:
            raise ValueError("no slope step: these labels do not come from add_feature_labels")
        from .slope_features import slope_stats
        return slope_stats(self.slope_block)

    def stats(self) -> Dict[str, int]:
        """Applied features, cells labelled 1 (the reference's "Feature cells"), valid cells, painted cells.  The first call
        synchronises; later ones do not."""
        if self._host_stats is None:
            self._host_stats = feature_stats(self.stats_block, self.applied_features)
        return dict(self._host_stats)

    def bands(self) -> List[np.ndarray]:
        """The two float32 host arrays the reference writes as bands 1-2: labels (nodata -1), depth."""
        return [self.labels.to(torch.float32).cpu().numpy(), self.depth.cpu().numpy()]


def _plane_to_device(plane, device) -> torch.Tensor:
    """A float32 contiguous device plane; one that already is such a plane on ``device`` is returned as it is (no copy)."""
    if isinstance(plane, torch.Tensor):
        return plane.to(device=device, dtype=torch.float32).contiguous()
    return torch.from_numpy(np.ascontiguousarray(np.asarray(plane), dtype=np.float32)).to(device)


def create_feature_labels(features: Sequence[Any], survey, transform=None, feature_radius: Optional[Dict[str, float]] = None,
                          device=None) -> Optional[FeatureLabels]:
    """The reference's ``create_feature_labels`` without the file I/O (extract_s57_features.py:784-865).  ``survey`` is a
    ``BathymetricGrid`` (its ``transform`` and ``crs`` are used unless ``transform`` is given; ``depth`` may be a host array or a
    device tensor), a host array or a device tensor (``transform`` is then required): ``[H, W]`` depths.  ``features`` have
    ``object_class``, ``x`` and ``y`` (``S57Feature``).  An empty feature list logs the reference's warning and returns ``None``.
    A plane already on the device is not copied; nothing synchronises until ``stats()`` or ``bands()``."""
    if not features:
        logger.warning("No features to label")
        return None
    crs = None
    if isinstance(survey, BathymetricGrid):
        depth, crs = survey.depth, survey.crs
        transform = survey.transform if transform is None else transform
    else:
        depth = survey
    if transform is None:
        raise ValueError("a geotransform is needed: pass transform= or a BathymetricGrid that has one")
    if isinstance(depth, torch.Tensor) and depth.is_cuda and device is None:
        device = depth.device
    device = rt.resolve_device(device)
    depth = _plane_to_device(depth, device)
    if depth.dim() != 2:
        raise ValueError(f"the survey has shape {tuple(depth.shape)}, a [H, W] plane is needed")
    table, applied = feature_pixel_table(features, transform, tuple(depth.shape), feature_radius)
    logger.info(f"Survey shape: {tuple(depth.shape)}, resolution: {abs(transform[1])}m")
    labels, stats = rasterize_features(table, depth=depth)
    logger.info(f"Applied {applied} feature labels")
    return FeatureLabels(labels, depth, tuple(transform), crs, applied, stats)
