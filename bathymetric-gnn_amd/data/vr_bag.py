"""Variable-resolution BAG refinement grids behind an array interface (reference ``data/vr_bag.py``).

The reference reads ``BAG_root/varres_metadata`` and ``BAG_root/varres_refinements`` with h5py and walks the
base grid in Python (``VRBagHandler.iterate_refinements``, :243-298), writing corrected values back one grid
at a time (``VRBagWriter.update_refinement_batch``, :550-588).  h5py and GDAL are not part of this path:
the handlers here work on the two structured arrays themselves (``from_arrays``), which is also what the
device path (``NativeVRProcessor.process_refinements``) uploads as they are.  Opening a file needs h5py and
raises ``ImportError`` without it, as the reference does (:118-119).

``SidecarBuilder`` (reference :609-835) rasterises classification / confidence / correction / valid mask of the processed
grids onto one georeferenced raster.  Only its constructor (shape, geotransform and CRS of GDAL's resampled view) and ``save``
(GeoTIFF) need GDAL and stay with the reference; ``SidecarBuilder.from_georef`` takes those three values as arguments, and the
rasterisation runs either on the host (``add_refinement_results``, vectorised) or on the device
(``NativeVRProcessor.process_refinements(..., sidecar=builder)``: include/bgnn_sidecar.h, csrc/vr_sidecar.hip).

Array formats (BAG 1.6, the fields the reference reads at :262-290):
  varres_metadata     [rows, cols] records: index u32, dimensions_x u32, dimensions_y u32, resolution_x f32,
                      resolution_y f32, sw_corner_x f32, sw_corner_y f32
  varres_refinements  [1, N] records: depth f32, depth_uncrt f32
"""
from __future__ import annotations

import logging
import shutil
from dataclasses import dataclass
from pathlib import Path
from typing import Dict, Generator, Optional, Tuple

import numpy as np

try:                                  # pragma: no cover - not installed in this image
    import h5py
    H5PY_AVAILABLE = True
except ImportError:
    H5PY_AVAILABLE = False

logger = logging.getLogger(__name__)

VARRES_METADATA_DTYPE = np.dtype([("index", "<u4"), ("dimensions_x", "<u4"), ("dimensions_y", "<u4"),
                                  ("resolution_x", "<f4"), ("resolution_y", "<f4"),
                                  ("sw_corner_x", "<f4"), ("sw_corner_y", "<f4")])
VARRES_REFINEMENT_DTYPE = np.dtype([("depth", "<f4"), ("depth_uncrt", "<f4")])


@dataclass
class RefinementGrid:
    """One refinement grid of a VR BAG (reference :67-97)."""
    base_row: int
    base_col: int
    depth: np.ndarray
    uncertainty: np.ndarray
    resolution: Tuple[float, float]      # (x_res, y_res)
    dimensions: Tuple[int, int]          # (rows, cols)
    sw_corner: Tuple[float, float]
    start_index: int                     # into varres_refinements

    @property
    def shape(self) -> Tuple[int, int]:
        return self.depth.shape

    @property
    def valid_mask(self) -> np.ndarray:
        return (self.depth != 1.0e6) & np.isfinite(self.depth)

    @property
    def num_valid(self) -> int:
        nv = self.__dict__.get("_num_valid")             # set by the handler's iterator, which counts all grids in one pass
        return int(np.sum(self.valid_mask)) if nv is None else nv


def refinement_table(varres_metadata: np.ndarray):
    """Flat table of the refined base cells in iteration order (row-major over the base grid, cells with
    a zero dimension skipped, reference :265-273): dict of 1-D arrays ``base_row, base_col, index, dims_y,
    dims_x, res_x, res_y, sw_x, sw_y`` plus ``contiguous`` -- True when the grids' record ranges tile
    ``[index[0], index[0] + total)`` back to back in that order, i.e. the records are already the
    concatenated tile layout."""
    md = np.asarray(varres_metadata)
    dx = md["dimensions_x"].astype(np.int64); dy = md["dimensions_y"].astype(np.int64)
    rows, cols = np.nonzero((dx != 0) & (dy != 0))
    sel = md[rows, cols]
    t = {"base_row": rows, "base_col": cols, "index": sel["index"].astype(np.int64),
         "dims_y": sel["dimensions_y"].astype(np.int64), "dims_x": sel["dimensions_x"].astype(np.int64),
         "res_x": sel["resolution_x"], "res_y": sel["resolution_y"],
         "sw_x": sel["sw_corner_x"], "sw_y": sel["sw_corner_y"]}
    cells = t["dims_y"] * t["dims_x"]
    t["cells"] = cells
    if len(cells):
        t["contiguous"] = bool(np.all(t["index"][1:] == t["index"][:-1] + cells[:-1]))
    else:
        t["contiguous"] = True
    return t


class VRBagHandler:
    """Iterate refinement grids and hand out writers (reference :100-316)."""

    NODATA = 1.0e6
    INVALID_INDEX = 4294967295

    def __init__(self, path):
        if not H5PY_AVAILABLE:
            raise ImportError("h5py is required for VR BAG handling")
        self.path = Path(path)                                       # pragma: no cover - needs h5py
        with h5py.File(str(self.path), "r") as f:                    # pragma: no cover
            if "BAG_root" not in f:
                raise ValueError(f"Not a valid BAG file: {self.path}")
            root = f["BAG_root"]
            if "varres_refinements" not in root:
                raise ValueError(f"Not a VR BAG (no varres_refinements): {self.path}")
            if "varres_metadata" not in root:
                raise ValueError(f"Not a VR BAG (no varres_metadata): {self.path}")
            self._init_arrays(root["varres_metadata"][:], root["varres_refinements"][:], root["elevation"].shape)
        self.geotransform = None; self.crs = None                    # pragma: no cover (GDAL is outside the path)

    @classmethod
    def from_arrays(cls, varres_metadata: np.ndarray, varres_refinements: np.ndarray, base_shape=None,
                    geotransform=None, crs=None) -> "VRBagHandler":
        self = object.__new__(cls)
        self.path = None
        self._init_arrays(varres_metadata, varres_refinements, base_shape)
        self.geotransform = geotransform; self.crs = crs
        return self

    def _init_arrays(self, varres_metadata, varres_refinements, base_shape):
        md = np.asarray(varres_metadata)
        if md.ndim != 2 or md.dtype.names is None or not {"index", "dimensions_x", "dimensions_y", "resolution_x",
                                                            "resolution_y", "sw_corner_x", "sw_corner_y"} <= set(md.dtype.names):
            raise ValueError("varres_metadata must be a 2-D structured array with the BAG varres_metadata fields")
        ref = np.asarray(varres_refinements)
        if ref.dtype.names is None or not {"depth", "depth_uncrt"} <= set(ref.dtype.names):
            raise ValueError("varres_refinements must be a structured array with depth / depth_uncrt")
        if ref.ndim == 1:
            ref = ref[None, :]
        if ref.ndim != 2 or ref.shape[0] != 1:
            raise ValueError("varres_refinements must have shape (1, N)")
        self.varres_metadata = md
        self.varres_refinements = ref
        self.base_shape = tuple(base_shape) if base_shape is not None else md.shape
        self.min_depth = None; self.max_depth = None

    # ---- summary properties (reference :152-240) ---------------------------------------------------------
    @property
    def base_cell_size(self) -> Tuple[float, float]:
        if self.geotransform:
            return (abs(self.geotransform[1]), abs(self.geotransform[5]))
        res_x = self.varres_metadata["resolution_x"]; dims_x = self.varres_metadata["dimensions_x"]
        valid = dims_x > 0
        if np.any(valid):
            m = np.max(res_x[valid] * dims_x[valid])
            return (float(m), float(m))
        return (50.0, 50.0)

    @property
    def finest_resolution(self) -> float:
        res_x = self.varres_metadata["resolution_x"]
        valid = res_x > 0
        return float(np.min(res_x[valid])) if np.any(valid) else 1.0

    @property
    def bounds(self) -> Tuple[float, float, float, float]:
        if self.geotransform:
            gt = self.geotransform
            min_x, max_y = gt[0], gt[3]
            return (min_x, max_y + self.base_shape[0] * gt[5], min_x + self.base_shape[1] * gt[1], max_y)
        return (0, 0, self.base_shape[1] * 50, self.base_shape[0] * 50)

    @property
    def resampled_shape(self) -> Tuple[int, int]:
        b, res = self.bounds, self.finest_resolution
        return (int(np.ceil((b[3] - b[1]) / res)), int(np.ceil((b[2] - b[0]) / res)))

    @property
    def num_refinement_cells(self) -> int:
        return int(np.sum(self.varres_metadata["dimensions_x"] > 0))

    @property
    def total_refinement_nodes(self) -> int:
        md = self.varres_metadata
        return int(np.sum(md["dimensions_x"].astype(np.int64) * md["dimensions_y"].astype(np.int64)))

    def get_refinement_info(self) -> Dict:
        md = self.varres_metadata
        dx, dy, rx = md["dimensions_x"], md["dimensions_y"], md["resolution_x"]
        has = dx > 0
        return {"base_shape": self.base_shape, "num_refined_cells": int(np.sum(has)),
                "total_refinement_nodes": self.total_refinement_nodes,
                "unique_dimensions": sorted(set(zip(dx[has].flatten(), dy[has].flatten()))),
                "unique_resolutions": sorted(set(rx[has].flatten()))}

    def refinement_table(self):
        return refinement_table(self.varres_metadata)

    # ---- iteration (reference :243-298) -------------------------------------------------------------------
    def iterate_refinements(self, min_valid_ratio: float = 0.0) -> Generator[RefinementGrid, None, None]:
        """Same grids, same order (row-major over the base grid, cells with a zero dimension skipped), same ``min_valid_ratio``
        test as the reference's loop (:243-298).  What a grid needs is prepared for ALL grids in a few vectorised passes -- the
        depth / uncertainty planes copied out of the interleaved records once, the valid-cell counts by one cumulative sum, the
        metadata columns as Python lists -- so that per grid only the ``RefinementGrid`` itself is made: ``depth`` /
        ``uncertainty`` are 2-D views of those private planes (not of the handler's records: writing into them does not touch the
        BAG), and ``num_valid`` is known without another pass."""
        tab = self.refinement_table()
        n_grids = len(tab["cells"])
        if n_grids == 0:
            return
        ref = self.varres_refinements[0, :]
        depth_all = np.ascontiguousarray(ref["depth"], dtype=np.float32)        # (a field view is strided: these are copies)
        unc_all = np.ascontiguousarray(ref["depth_uncrt"], dtype=np.float32)
        valid_all = (depth_all != np.float32(1.0e6)) & np.isfinite(depth_all)                       # RefinementGrid.valid_mask
        start = tab["index"]; cells = tab["cells"]
        if tab["contiguous"] and int(start[0] + cells.sum()) == valid_all.shape[0]:
            nvalid = np.add.reduceat(valid_all, start, dtype=np.int64).tolist()     # the grids tile the records back to back
        else:
            csum = np.zeros(valid_all.shape[0] + 1, np.int64)
            np.cumsum(valid_all, out=csum[1:])
            nvalid = (csum[start + cells] - csum[start]).tolist()
        rows, cols = tab["base_row"].tolist(), tab["base_col"].tolist()
        starts, ncell = start.tolist(), cells.tolist()
        dys, dxs = tab["dims_y"].tolist(), tab["dims_x"].tolist()
        rxs, rys = [float(v) for v in tab["res_x"]], [float(v) for v in tab["res_y"]]
        sxs, sys_ = [float(v) for v in tab["sw_x"]], [float(v) for v in tab["sw_y"]]
        new_grid = object.__new__
        for i in range(n_grids):
            nv, n = nvalid[i], ncell[i]
            if nv / n >= min_valid_ratio:
                s0, dy, dx = starts[i], dys[i], dxs[i]
                e0 = s0 + n
                grid = new_grid(RefinementGrid)          # (the dataclass's fields, set directly: its __init__ costs as much as the rest)
                grid.__dict__ = {"base_row": rows[i], "base_col": cols[i], "depth": depth_all[s0:e0].reshape(dy, dx),
                                 "uncertainty": unc_all[s0:e0].reshape(dy, dx), "resolution": (rxs[i], rys[i]),
                                 "dimensions": (dy, dx), "sw_corner": (sxs[i], sys_[i]), "start_index": s0, "_num_valid": nv}
                yield grid

    def copy_and_open_for_writing(self, output_path=None) -> "VRBagWriter":
        """File-backed: copy the BAG and open the copy (reference :300-316).  Array-backed (``from_arrays``):
        a writer over a copy of the refinement records; ``output_path`` is ignored."""
        if self.path is None:
            return VRBagWriter.from_arrays(self.varres_refinements.copy(), self.varres_metadata)
        logger.info(f"Copying VR BAG: {self.path} -> {output_path}")      # pragma: no cover - needs h5py
        shutil.copy(str(self.path), str(output_path))                     # pragma: no cover
        return VRBagWriter(output_path)                                   # pragma: no cover


class VRBagWriter:
    """Write corrected refinement values back (reference :478-609)."""

    NODATA = 1.0e6

    def __init__(self, path):
        if not H5PY_AVAILABLE:
            raise ImportError("h5py is required for VR BAG handling")
        self.path = Path(path)                                       # pragma: no cover - needs h5py
        self._file = h5py.File(str(self.path), "r+")                 # pragma: no cover
        root = self._file["BAG_root"]                                # pragma: no cover
        self._refinements = root["varres_refinements"]               # pragma: no cover
        self._metadata = root["varres_metadata"][:]                  # pragma: no cover
        self._corrections_applied = 0; self._uncertainty_updates = 0   # pragma: no cover

    @classmethod
    def from_arrays(cls, varres_refinements: np.ndarray, varres_metadata: Optional[np.ndarray] = None) -> "VRBagWriter":
        self = object.__new__(cls)
        self.path = None; self._file = None
        ref = np.asarray(varres_refinements)
        self._refinements = ref[None, :] if ref.ndim == 1 else ref
        self._metadata = varres_metadata
        self._corrections_applied = 0; self._uncertainty_updates = 0
        return self

    @property
    def refinements(self) -> np.ndarray:
        """The (1, N) record array being modified (array-backed writers)."""
        return self._refinements

    def _check(self, grid, corrected_depth):
        if corrected_depth.shape != grid.shape:
            raise ValueError(f"Shape mismatch: corrected {corrected_depth.shape} vs grid {grid.shape}")

    def update_refinement(self, grid: RefinementGrid, corrected_depth: np.ndarray,
                          corrected_uncertainty: Optional[np.ndarray] = None):
        """Reference :502-548 (element-wise writes there; same end state and counters)."""
        self._check(grid, corrected_depth)
        s, n = grid.start_index, grid.dimensions[0] * grid.dimensions[1]
        cur = self._refinements[0, s:s + n]
        cur["depth"] = corrected_depth.flatten()
        self._corrections_applied += int(np.sum((corrected_depth != grid.depth) & grid.valid_mask))
        if corrected_uncertainty is not None:
            cur["depth_uncrt"] = corrected_uncertainty.flatten()
            self._uncertainty_updates += int(np.sum((corrected_uncertainty != grid.uncertainty) & grid.valid_mask))
        self._refinements[0, s:s + n] = cur

    def update_refinement_batch(self, grid: RefinementGrid, corrected_depth: np.ndarray,
                                corrected_uncertainty: Optional[np.ndarray] = None):
        """Reference :550-588: read the grid's records, replace depth (and uncertainty), write back."""
        self._check(grid, corrected_depth)
        s, n = grid.start_index, grid.dimensions[0] * grid.dimensions[1]
        cur = self._refinements[0, s:s + n]
        cur["depth"] = corrected_depth.flatten()
        if corrected_uncertainty is not None:
            cur["depth_uncrt"] = corrected_uncertainty.flatten()
        self._refinements[0, s:s + n] = cur
        self._corrections_applied += int(np.sum((corrected_depth != grid.depth) & grid.valid_mask))

    def update_refinements_bulk(self, grids, depth_flat: np.ndarray, uncertainty_flat: Optional[np.ndarray], changed: int = 0):
        """``update_refinement_batch`` for many grids at once: ``depth_flat`` / ``uncertainty_flat`` hold the grids' corrected
        values back to back (row-major each), ``changed`` the number of valid cells whose depth changed (what the per-grid calls
        would have added to the corrections counter).  One scatter into the record array instead of a read-modify-write per grid;
        array-backed writers only (a file-backed one takes the per-grid path)."""
        if self._file is not None:                                   # pragma: no cover - needs h5py
            off = 0
            for g in grids:
                n = g.dimensions[0] * g.dimensions[1]
                self.update_refinement_batch(g, depth_flat[off:off + n].reshape(g.dimensions),
                                             None if uncertainty_flat is None else uncertainty_flat[off:off + n].reshape(g.dimensions))
                off += n
            return
        starts = np.fromiter((g.start_index for g in grids), np.int64, len(grids))
        cells = np.fromiter((g.dimensions[0] * g.dimensions[1] for g in grids), np.int64, len(grids))
        total = int(cells.sum())
        if depth_flat.shape[0] != total:
            raise ValueError(f"Shape mismatch: {depth_flat.shape[0]} corrected values for {total} cells")
        rec = self._refinements[0]
        if len(grids) == 1 or bool(np.all(starts[1:] == starts[:-1] + cells[:-1])):    # a run of consecutive grids: one slice
            s0 = int(starts[0])
            rec["depth"][s0:s0 + total] = depth_flat
            if uncertainty_flat is not None:
                rec["depth_uncrt"][s0:s0 + total] = uncertainty_flat
        else:
            offs = np.zeros(len(grids), np.int64); np.cumsum(cells[:-1], out=offs[1:])
            idx = np.repeat(starts - offs, cells) + np.arange(total, dtype=np.int64)
            rec["depth"][idx] = depth_flat
            if uncertainty_flat is not None:
                rec["depth_uncrt"][idx] = uncertainty_flat
        self._corrections_applied += int(changed)

    def write_records(self, start: int, records: np.ndarray, corrections_applied: int = 0):
        """Bulk write-back used by the device path: ``records`` (structured or float32 [n, 2]) replace
        ``varres_refinements[0, start:start+n]`` in one slice assignment."""
        rec = np.asarray(records)
        n = rec.shape[0]
        tgt = self._refinements
        if self._file is None and rec.dtype == np.float32 and rec.ndim == 2 and rec.shape[1] == 2 and tgt.dtype == VARRES_REFINEMENT_DTYPE \
                and tgt.flags.c_contiguous:
            # array-backed, plain {depth, depth_uncrt} float32 records: ONE memcpy through a float32 view (numpy assigns structured
            # arrays field by field: 10x slower)
            np.copyto(tgt.reshape(-1).view(np.float32).reshape(-1, 2)[start:start + n], rec)
            self._corrections_applied += int(corrections_applied)
            return
        if rec.dtype.names is None:
            rec = np.ascontiguousarray(rec, dtype=np.float32).reshape(-1, 2).view(VARRES_REFINEMENT_DTYPE).reshape(-1)
        cur = self._refinements[0, start:start + n]
        cur["depth"] = rec["depth"]; cur["depth_uncrt"] = rec["depth_uncrt"]
        self._refinements[0, start:start + n] = cur
        self._corrections_applied += int(corrections_applied)

    def close(self):
        if self._file is not None:                                   # pragma: no cover - needs h5py
            self._file.close(); self._file = None
        logger.info("VR BAG modifications complete:")
        logger.info(f"  - Depth corrections applied: {self._corrections_applied:,}")
        if self._uncertainty_updates > 0:
            logger.info(f"  - Uncertainty updates: {self._uncertainty_updates:,}")

    def __enter__(self):
        return self

    def __exit__(self, exc_type, exc_val, exc_tb):
        self.close()
        return False


class SRBagHandler:
    """Single-resolution BAG as one "refinement grid" (reference :319-428), array-backed."""

    NODATA = 1.0e6

    def __init__(self, path):
        if not H5PY_AVAILABLE:
            raise ImportError("h5py is required for native BAG processing")
        raise NotImplementedError("file-backed SR BAGs: read elevation / uncertainty with h5py and use from_arrays")  # pragma: no cover

    @classmethod
    def from_arrays(cls, elevation: np.ndarray, uncertainty: Optional[np.ndarray] = None, resolution: float = 1.0) -> "SRBagHandler":
        self = object.__new__(cls)
        self.path = None
        self._depth = np.asarray(elevation).astype(np.float32)
        self._uncertainty = (np.asarray(uncertainty).astype(np.float32) if uncertainty is not None
                             else np.zeros_like(self._depth))
        self._shape = self._depth.shape
        self._resolution = float(resolution)
        return self

    @property
    def base_shape(self) -> Tuple[int, int]:
        return self._shape

    def get_refinement_info(self) -> Dict:
        valid = (self._depth != 1.0e6) & np.isfinite(self._depth)
        return {"base_shape": self._shape, "num_refined_cells": 1, "total_refinement_nodes": int(np.sum(valid)),
                "unique_resolutions": [self._resolution]}

    def iterate_refinements(self, min_valid_ratio: float = 0.0) -> Generator[RefinementGrid, None, None]:
        valid = (self._depth != 1.0e6) & np.isfinite(self._depth)
        if np.sum(valid) / self._depth.size >= min_valid_ratio:
            yield RefinementGrid(base_row=0, base_col=0, depth=self._depth.copy(), uncertainty=self._uncertainty.copy(),
                                 resolution=(self._resolution, self._resolution), dimensions=self._shape,
                                 sw_corner=(0.0, 0.0), start_index=0)

    def copy_and_open_for_writing(self, output_path=None) -> "SRBagWriter":
        return SRBagWriter.from_arrays(self._depth.copy(), self._uncertainty.copy())


class SRBagWriter:
    """Reference :431-475: the whole elevation / uncertainty grid is replaced."""

    def __init__(self, path):
        if not H5PY_AVAILABLE:
            raise ImportError("h5py is required for native BAG processing")
        raise NotImplementedError("file-backed SR BAGs: use from_arrays")   # pragma: no cover

    @classmethod
    def from_arrays(cls, elevation: np.ndarray, uncertainty: Optional[np.ndarray]) -> "SRBagWriter":
        self = object.__new__(cls)
        self.elevation = elevation; self.uncertainty = uncertainty
        return self

    def update_refinement_batch(self, grid, corrected_depth, corrected_uncertainty):
        self.elevation[:] = corrected_depth
        if self.uncertainty is not None:
            self.uncertainty[:] = corrected_uncertainty

    def close(self):
        pass

    def __enter__(self):
        return self

    def __exit__(self, exc_type, exc_val, exc_tb):
        self.close()
        return False


class SidecarBuilder:
    """Sidecar raster of a native VR run (reference :609-835): float32 ``classification``, ``confidence``, ``correction`` (NaN where
    nothing was painted) and ``valid_mask`` (0 / 1) on one grid ``shape`` with ``geotransform`` / ``crs``.

    Every processed refinement grid is painted at its geographic position, each cell as a ``scale x scale`` block of pixels,
    refinement row 0 at the south (``add_refinement_results``, reference :695-778).  Grids are applied in iteration order: where two
    cover a pixel the later one's values stay; the valid mask is sticky (1 where any covering cell was valid); pixels outside the
    raster are dropped.

    ``SidecarBuilder(handler)`` is the reference's constructor: it reads the raster's georeferencing from GDAL's resampled view of
    the BAG and raises ``ImportError`` without GDAL.  ``from_georef`` is the array interface.  After a device run
    (``process_refinements(..., sidecar=self)``) the four planes live on the GPU (``planes_device()``); the host attributes are
    filled from there on first access."""

    MAX_PIXELS = 1 << 28            # BGNN_SIDECAR_MAX_PIXELS (include/bgnn_sidecar.h): the device images are 24 B per pixel

    def __init__(self, handler):
        self.handler = handler
        try:
            from osgeo import gdal  # noqa: F401
        except ImportError:
            raise ImportError("GDAL required for SidecarBuilder")
        raise NotImplementedError("reading the resampled view's georeferencing with GDAL stays with the reference: "
                                  "use SidecarBuilder.from_georef(handler, shape, geotransform, crs)")    # pragma: no cover

    @classmethod
    def from_georef(cls, handler, shape, geotransform, crs: str = "") -> "SidecarBuilder":
        """A builder for a raster of ``shape`` = (rows, cols) with GDAL-style ``geotransform`` (origin x, pixel width, 0, origin y,
        0, -pixel height) and ``crs`` -- what the reference reads from the resampled view (:679-691).  ``handler`` only has to
        offer ``base_shape``."""
        self = object.__new__(cls)
        self.handler = handler
        self.shape = (int(shape[0]), int(shape[1]))
        if self.shape[0] < 1 or self.shape[1] < 1:
            raise ValueError(f"raster shape {self.shape}: both sides must be at least 1")
        self.geotransform = tuple(float(v) for v in geotransform)
        if len(self.geotransform) != 6 or self.geotransform[1] == 0 or self.geotransform[5] == 0:
            raise ValueError("geotransform: six values with non-zero pixel sizes")
        self.crs = crs
        gt = self.geotransform
        self.resolution = abs(gt[1])
        min_x, max_y = gt[0], gt[3]
        self.bounds = (min_x, max_y + self.shape[0] * gt[5], min_x + self.shape[1] * gt[1], max_y)
        self._planes = None            # [4, H, W] host planes, made on first access (a device run may never need them)
        self._device = None            # [4, H, W] device tensor of a device run not yet downloaded
        self._device_planes = self._device_ready = None
        self._used = False
        logger.info(f"SidecarBuilder initialized: {self.shape} at {self.resolution}m")
        return self

    # ---- the four planes ------------------------------------------------------------------------------------
    def _host(self) -> np.ndarray:
        if self._device is not None:
            dev, self._device = self.planes_device(), None
            self._planes = dev.cpu().numpy()
        elif self._planes is None:
            self._planes = np.empty((4,) + self.shape, np.float32)
            self._planes[:3] = np.nan
            self._planes[3] = 0
        return self._planes

    classification = property(lambda self: self._host()[0])
    confidence = property(lambda self: self._host()[1])
    correction = property(lambda self: self._host()[2])
    valid_mask = property(lambda self: self._host()[3])

    @property
    def fresh(self) -> bool:
        """True until something has been added (a device run needs a fresh builder)."""
        return not self._used

    def planes(self) -> np.ndarray:
        """float32 [4, H, W] on the host: classification, confidence, correction, valid_mask (the builder's own storage)."""
        return self._host()

    def planes_device(self):
        """The [4, H, W] device tensor a device run left (no download); ``None`` when there has been none."""
        if self._device_ready is not None:                 # (written on the library's stream: wait for it once)
            self._device_ready.synchronize()
            self._device_ready = None
        return self._device_planes

    def _adopt_device(self, planes_t, ready=None):
        """``process_refinements`` hands over the device planes and the event behind the kernel that completes them."""
        self._device = self._device_planes = planes_t
        self._device_ready = ready
        self._used = True

    # ---- placement (reference :711-752) -----------------------------------------------------------------------
    def placement(self, table) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
        """``(out_row_start, out_col_start, scale)`` as int64 arrays for every grid of a ``refinement_table()`` (the keys used:
        ``base_row, base_col, dims_y, dims_x, res_x, res_y, sw_x, sw_y``), in float64 like the reference's per-grid Python
        expressions: the float32 metadata widened, ``round`` half-to-even, the scale from ``res_x`` alone and at least 1, the
        grid's height from ``res_y``."""
        f8 = lambda k: np.asarray(table[k]).astype(np.float64)
        base_shape = self.handler.base_shape
        b, gt = self.bounds, self.geotransform
        base_cell_width = (b[2] - b[0]) / base_shape[1]
        base_cell_height = (b[3] - b[1]) / base_shape[0]
        ref_x = (b[0] + f8("base_col") * base_cell_width) + f8("sw_x")
        ref_y = (b[1] + f8("base_row") * base_cell_height) + f8("sw_y")
        ref_top_y = ref_y + f8("dims_y") * f8("res_y")
        col0 = np.rint((ref_x - gt[0]) / gt[1])
        row0 = np.rint((gt[3] - ref_top_y) / abs(gt[5]))
        scale = np.maximum(1, np.rint(f8("res_x") / self.resolution))
        return row0.astype(np.int64), col0.astype(np.int64), scale.astype(np.int64)

    @staticmethod
    def _grid_table(grid):
        one = lambda v, dt: np.array([v], dt)
        return {"base_row": one(grid.base_row, np.int64), "base_col": one(grid.base_col, np.int64),
                "dims_y": one(grid.dimensions[0], np.int64), "dims_x": one(grid.dimensions[1], np.int64),
                "res_x": one(grid.resolution[0], np.float64), "res_y": one(grid.resolution[1], np.float64),
                "sw_x": one(grid.sw_corner[0], np.float64), "sw_y": one(grid.sw_corner[1], np.float64)}

    # ---- host rasterisation -------------------------------------------------------------------------------------
    def add_refinement_results(self, grid: RefinementGrid, classification: np.ndarray, confidence: np.ndarray,
                               correction: np.ndarray):
        """Paint one processed grid (reference :695-778; same end state).  The raster window the grid's footprint overlaps is
        assigned in one piece per plane: raster row ``R`` takes refinement row ``h - 1 - (R - row0) // scale``, raster column
        ``C`` takes refinement column ``(C - col0) // scale``."""
        planes = self._host()
        self._used = True
        self._device_planes = None                         # (a device run's tensor no longer holds the builder's state)
        row0, col0, scale = (int(v[0]) for v in self.placement(self._grid_table(grid)))
        h, w = int(grid.dimensions[0]), int(grid.dimensions[1])
        r_lo, r_hi = max(0, row0), min(self.shape[0], row0 + h * scale)
        c_lo, c_hi = max(0, col0), min(self.shape[1], col0 + w * scale)
        if r_hi <= r_lo or c_hi <= c_lo:
            return
        src_r = (h - 1) - (np.arange(r_lo, r_hi) - row0) // scale
        src_c = (np.arange(c_lo, c_hi) - col0) // scale
        ix = np.ix_(src_r, src_c)
        win = (slice(r_lo, r_hi), slice(c_lo, c_hi))
        planes[0][win] = np.asarray(classification)[ix]
        planes[1][win] = np.asarray(confidence)[ix]
        planes[2][win] = np.asarray(correction)[ix]
        np.putmask(planes[3][win], np.asarray(grid.valid_mask)[ix], np.float32(1.0))

    def save(self, path):
        """GeoTIFF export needs GDAL and stays with the reference (:780-834); without it: an error in the log, as there."""
        try:
            from osgeo import gdal  # noqa: F401
        except ImportError:
            logger.error("GDAL required for GeoTIFF export")
            return
        raise NotImplementedError("GeoTIFF export with GDAL stays with the reference: write planes() with "
                                  "geotransform / crs")    # pragma: no cover


def detect_bag_type(path) -> str:
    """Reference :29-64; needs h5py."""
    if not H5PY_AVAILABLE:
        raise ImportError("h5py is required for BAG type detection")
    with h5py.File(Path(path), "r") as f:                            # pragma: no cover - needs h5py
        root = f["BAG_root"]
        if "varres_metadata" in root and "varres_refinements" in root:
            if np.any(root["varres_metadata"][:]["dimensions_x"] > 0):
                return "VR"
        return "SR"
