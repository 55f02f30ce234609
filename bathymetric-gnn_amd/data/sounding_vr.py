"""Gridding soundings at variable resolution on the device: a point cloud in, the refinement records of a VR layout out.

``SoundingGridder`` and ``RobustSoundingGridder`` grid onto one uniform raster.  The reference's main mode is native VR
(``scripts/inference_native.py``, ``process_refinements``; training plan steps 1.2 and 4.1), and everything here that reads a VR
BAG takes ``varres_metadata`` / ``varres_refinements``.  This module joins the two: a cloud is filed straight into the
refinement records of a layout that is planned from the cloud's own density (``VRLayoutPlanner``, ``plan_vr_layout``) or taken
from an existing BAG (``VRLayout.from_metadata``), and the result is handed over as a ``VRBagHandler``.  A clean / noisy pair of
one cloud -- ``compute_ground_truth_native(clean=robust.handler("kept_mean"), noisy=plain.handler("mean"))`` -- is noise that
"exists in the point cloud but not in the gridded surface" (``docs/LESSONS_LEARNED.md`` section 6).

The contract in short (include/bgnn_soundings_vr.h has all of it).  The base grid has ``BH x BW`` cells of ``B`` metres,
``(x0, y0)`` the SOUTH-WEST corner, base row 0 and refinement row 0 the southmost: the BAG's order, the opposite of
``SoundingGridder``'s north-up origin.  In float64 with true divisions ``u = (x - x0) / B``, ``bc = floor(u)``, ``fu = u - bc``,
``sc = floor(fu * dx)`` (and the same in y), ``record = index + sr * dx + sc``.  A sounding enters exactly one of ``nonfinite``,
``outside`` (off the base grid), ``unrefined`` (a base cell without a grid), ``out_of_range`` (``|z| >= 32768``), ``accepted``,
checked in that order.  Per record the statistics, quantisation and planes are those of the uniform gridders: a layout of
``total`` records is a ``1 x total`` grid to both ``finalize`` passes, which are reused as they are.

The planner, all in integers: a base cell with ``n`` soundings (finite, in range) gets ``d = max{d_i : n >= target_count * d_i^2}``
from the ladder, 0 when ``n < min_base_count`` or no rung fits; ``index`` is the exclusive sum of ``d * d`` in row-major order from
the south-west, so the grids tile the records back to back.  Limits: ``BH * BW <= 2^31 - 1``, ``total <= 2^31 - 1``."""
from __future__ import annotations

import dataclasses
import math
from typing import Dict, Optional, Sequence, Tuple

import numpy as np
import torch

from .. import runtime as rt
from .sounding_grid import (DEPTH_PLANES, _GridderBase, _OfferedSoundings, _check_coordinates, _check_min_count, _check_origin,
                            _check_resolution, _check_robust_rule, _check_shape, _finalize_plain, _finalize_robust, _new_stage,
                            _new_state, _on_device, _pick_plane, density_from_count, sounding_extent)
from .sounding_robust import DEFAULT_K, ROBUST_DEPTH_PLANES, ROBUST_UNCERTAINTY_PLANES
from .vr_bag import VARRES_METADATA_DTYPE, VARRES_REFINEMENT_DTYPE, VRBagHandler

DEFAULT_LADDER = (1, 2, 4, 8, 16, 32, 64)
RECORD_NODATA = 1.0e6                # what a VR BAG holds where a record has no depth (VRBagHandler.NODATA)
UNREFINED_INDEX = 0xFFFFFFFF         # varres_metadata.index of a base cell without a grid (VRBagHandler.INVALID_INDEX)
UNCERTAINTY_PLANES = ("std",)


def _check_base(base_shape, origin, base_resolution):
    shape = _check_shape(base_shape, "base shape")
    res = _check_resolution(base_resolution)
    if shape[0] * shape[1] > rt.VR_MAX_BASE_CELLS:
        raise NotImplementedError(f"base shape {shape}: more than {rt.VR_MAX_BASE_CELLS} base cells")
    return shape, _check_origin(origin), res


def _check_ladder(ladder) -> Tuple[int, ...]:
    rungs = tuple(int(d) for d in ladder)
    if not 1 <= len(rungs) <= rt.VR_MAX_RUNGS:
        raise ValueError(f"ladder {ladder!r}: 1 .. {rt.VR_MAX_RUNGS} rungs expected")
    if any(not 1 <= d <= rt.VR_MAX_DIM for d in rungs):
        raise ValueError(f"ladder {ladder!r}: rungs of 1 .. {rt.VR_MAX_DIM} expected")
    if any(b <= a for a, b in zip(rungs, rungs[1:])):
        raise ValueError(f"ladder {ladder!r}: strictly ascending rungs expected")
    return rungs


class VRLayout:
    """A base grid and the refinement grid of every base cell.  ``base_shape = (BH, BW)``, ``origin = (x0, y0)`` the south-west
    corner, ``base_resolution = B``; host arrays ``index`` (int64), ``dx``, ``dy`` (int32), ``[BH, BW]`` each, base row 0 the
    southmost, ``dx == dy == 0`` where the cell is not refined; ``total`` records; ``table``: the 16-byte entries (int64 index,
    int32 dx, int32 dy) on the device, as an int64 tensor of ``2 * BH * BW``."""

    def __init__(self, base_shape, origin, base_resolution, index, dx, dy, total, device=None, table: Optional[torch.Tensor] = None):
        self.base_shape, self.origin, self.base_resolution = _check_base(base_shape, origin, base_resolution)
        self.index = np.ascontiguousarray(index, np.int64).reshape(self.base_shape)
        self.dx = np.ascontiguousarray(dx, np.int32).reshape(self.base_shape)
        self.dy = np.ascontiguousarray(dy, np.int32).reshape(self.base_shape)
        self.total = int(total)
        self._check_records()
        self.device = rt.resolve_device(device) if table is None else table.device
        if table is None:
            host = np.zeros(self.base_shape, rt.VR_ENTRY_DTYPE)
            host["index"], host["dx"], host["dy"] = self.index, self.dx, self.dy
            table = torch.from_numpy(host.reshape(-1).view(np.int64).copy()).to(self.device)
        self.table = table

    def _check_records(self):
        """Dimensions 0 .. 32768, record ranges inside ``0 .. total`` that do not overlap, ``total <= 2^31 - 1``."""
        dx, dy = self.dx.astype(np.int64).reshape(-1), self.dy.astype(np.int64).reshape(-1)
        if np.any((dx < 0) | (dx > rt.VR_MAX_DIM) | (dy < 0) | (dy > rt.VR_MAX_DIM)):
            raise ValueError(f"layout: dimensions of 0 .. {rt.VR_MAX_DIM} expected")
        if not 0 <= self.total <= rt.VR_MAX_RECORDS:
            raise ValueError(f"layout: {self.total} records, at most {rt.VR_MAX_RECORDS} expected")
        refined = (dx > 0) & (dy > 0)
        first = self.index.reshape(-1)[refined]
        last = first + dx[refined] * dy[refined]
        if first.size and (first.min() < 0 or last.max() > self.total):
            raise ValueError(f"layout: a refinement grid leaves the {self.total} records")
        order = np.argsort(first, kind="stable")
        if np.any(first[order][1:] < last[order][:-1]):
            raise ValueError("layout: the record ranges of two refinement grids overlap")

    @property
    def refined(self) -> np.ndarray:
        return (self.dx > 0) & (self.dy > 0)

    @property
    def state_bytes(self) -> int:
        return rt.SOUNDINGS_HEADER_BYTES + rt.SOUNDINGS_CELL_BYTES * self.total

    @property
    def geotransform(self) -> Tuple[float, float, float, float, float, float]:
        """GDAL's north-up transform of the base grid: ``(x0, B, 0, y0 + BH * B, 0, -B)``."""
        (x0, y0), B = self.origin, self.base_resolution
        return (x0, B, 0.0, y0 + self.base_shape[0] * B, 0.0, -B)

    def metadata(self) -> np.ndarray:
        """The ``VARRES_METADATA_DTYPE`` array ``[BH, BW]``: ``index`` (0xFFFFFFFF where not refined), the dimensions,
        ``resolution_x = float32(B / dx)``, ``resolution_y = float32(B / dy)`` and ``sw_corner = 0``: the grid's footprint is the
        whole base cell."""
        md = np.zeros(self.base_shape, VARRES_METADATA_DTYPE)
        ref = self.refined
        md["index"] = np.where(ref, self.index, UNREFINED_INDEX).astype(np.uint32)
        md["dimensions_x"] = np.where(ref, self.dx, 0)
        md["dimensions_y"] = np.where(ref, self.dy, 0)
        B = np.float64(self.base_resolution)
        md["resolution_x"] = np.where(ref, B / np.maximum(self.dx, 1), 0.0).astype(np.float32)
        md["resolution_y"] = np.where(ref, B / np.maximum(self.dy, 1), 0.0).astype(np.float32)
        return md

    @classmethod
    def from_metadata(cls, varres_metadata, origin, base_resolution, device=None) -> "VRLayout":
        """The layout of an existing BAG: ``index`` and the dimensions of its ``varres_metadata``, every grid's footprint taken to
        be the whole base cell; ``total`` is the end of the last record range.  Record ranges that overlap or exceed the limits
        are refused (``ValueError``).  A new cloud can so be gridded onto the layout of a file that exists."""
        md = np.asarray(varres_metadata)
        if md.ndim != 2 or md.dtype.names is None or not {"index", "dimensions_x", "dimensions_y"} <= set(md.dtype.names):
            raise ValueError("varres_metadata must be a 2-D structured array with index, dimensions_x and dimensions_y")
        dx, dy = md["dimensions_x"].astype(np.int64), md["dimensions_y"].astype(np.int64)
        if np.any(dx > rt.VR_MAX_DIM) or np.any(dy > rt.VR_MAX_DIM):
            raise ValueError(f"varres_metadata: dimensions of 0 .. {rt.VR_MAX_DIM} expected")
        ref = (dx > 0) & (dy > 0)
        index = np.where(ref, md["index"].astype(np.int64), 0)
        total = int((index + dx * dy)[ref].max()) if ref.any() else 0
        return cls(md.shape, origin, base_resolution, index, np.where(ref, dx, 0), np.where(ref, dy, 0), total, device=device)

    def grid_slice(self, base_row: int, base_col: int) -> Tuple[int, int, int]:
        """``(first record, dy, dx)`` of one base cell's refinement grid (``IndexError`` off the base grid, ``KeyError`` where the
        cell is not refined)."""
        BH, BW = self.base_shape
        if not (0 <= base_row < BH and 0 <= base_col < BW):
            raise IndexError(f"base cell ({base_row}, {base_col}) of a {BH} x {BW} base grid")
        dy, dx = int(self.dy[base_row, base_col]), int(self.dx[base_row, base_col])
        if dx < 1 or dy < 1:
            raise KeyError(f"base cell ({base_row}, {base_col}) is not refined")
        return int(self.index[base_row, base_col]), dy, dx


class VRLayoutPlanner(_OfferedSoundings):
    """``add(x, y, z)`` as often as the survey has line files (the density pass: a count per base cell of the soundings that are
    finite, on the base grid and in range), then ``plan(...)``.  The density is a pass of its own under the base-cell arithmetic
    of the add pass: the plan sees the cells the soundings will be filed under."""

    def __init__(self, base_shape, origin, base_resolution, device=None):
        self.base_shape, self.origin, self.base_resolution = _check_base(base_shape, origin, base_resolution)
        self.device = rt.resolve_device(device)
        self._ctx = rt.get_context(self.device)
        self._counts = torch.zeros(self.base_shape, dtype=torch.int32, device=self.device)      # (uint32 bits)

    def _offer(self, x, y, z, n):
        self._call("bgnn_vr_soundings_density", rt.ptr(x), rt.ptr(y), rt.ptr(z), n, self.origin[0], self.origin[1], self.base_resolution,
                   self.base_shape[0], self.base_shape[1], rt.ptr(self._counts))

    def counts(self) -> torch.Tensor:
        """The soundings per base cell so far, ``[BH, BW]`` int64 on the device, base row 0 the southmost."""
        return self._counts.to(torch.int64) & 0xFFFFFFFF

    def plan(self, target_count: int = 4, ladder: Sequence[int] = DEFAULT_LADDER, min_base_count: int = 1) -> VRLayout:
        """The layout of the counts so far: scan and table on the device.  The table and ``total`` come back in one copy, the one
        host wait: no state can be sized without ``total``.  ``ValueError`` for a bad ladder or count before anything is launched,
        and for a ``total`` beyond 2^31 - 1."""
        rungs = _check_ladder(ladder)
        target_count, min_base_count = int(target_count), int(min_base_count)
        if not 1 <= target_count <= rt.VR_MAX_TARGET:
            raise ValueError(f"target_count {target_count}: 1 .. {rt.VR_MAX_TARGET} expected")
        if not 1 <= min_base_count <= rt.VR_MAX_TARGET:
            raise ValueError(f"min_base_count {min_base_count}: 1 .. {rt.VR_MAX_TARGET} expected")
        ctx, dev, (BH, BW) = self._ctx, self.device, self.base_shape
        cells = BH * BW
        ws_bytes = int(ctx.lib.bgnn_vr_soundings_plan_workspace_bytes(BH, BW))
        ws = torch.empty(ws_bytes // 8, dtype=torch.int64, device=dev)
        out = torch.empty(2 * cells + 1, dtype=torch.int64, device=dev)                      # the table, total behind it
        host_ladder = np.asarray(rungs, np.int32)
        self._call("bgnn_vr_soundings_plan", rt.ptr(self._counts), BH, BW, host_ladder.ctypes.data, len(rungs), target_count,
                   min_base_count, rt.ptr(ws), ws_bytes, rt.ptr(out), rt.ptr(out[2 * cells:]))
        host = out.cpu().numpy()
        total = int(host[2 * cells])
        if total > rt.VR_MAX_RECORDS:
            raise ValueError(f"the planned layout has {total} records, more than {rt.VR_MAX_RECORDS}: a coarser ladder or a higher "
                             "target_count is needed")
        entries = host[:2 * cells].view(rt.VR_ENTRY_DTYPE)
        return VRLayout(self.base_shape, self.origin, self.base_resolution, entries["index"], entries["dx"], entries["dy"], total,
                        table=out[:2 * cells])


def plan_vr_base_grid(x, y, base_resolution) -> Tuple[Tuple[int, int], Tuple[float, float]]:
    """The smallest base grid on the lattice of multiples of ``base_resolution`` that holds every finite coordinate:
    ``((BH, BW), (x0, y0))``, ``(x0, y0)`` the south-west corner; a corner moves one cell outward where rounding would leave the
    extreme sounding on its wrong side.  Device tensors."""
    B = _check_resolution(base_resolution)
    e = sounding_extent(x, y)
    if e["finite_x"] == 0 or e["finite_y"] == 0:
        raise ValueError("plan_vr_base_grid: no finite coordinate")
    x0 = math.floor(e["min_x"] / B) * B
    while x0 > e["min_x"]:
        x0 -= B
    y0 = math.floor(e["min_y"] / B) * B
    while y0 > e["min_y"]:
        y0 -= B
    BW = math.floor((e["max_x"] - x0) / B) + 1
    BH = math.floor((e["max_y"] - y0) / B) + 1
    return (int(BH), int(BW)), (float(x0), float(y0))


def plan_vr_layout(x, y, z, base_resolution, target_count: int = 4, ladder: Sequence[int] = DEFAULT_LADDER,
                   min_base_count: int = 1, base_shape=None, origin=None) -> VRLayout:
    """Base grid from the cloud's extent (unless ``base_shape`` and ``origin`` are given), density, plan: device tensors in, a
    ``VRLayout`` on their device out."""
    if (base_shape is None) != (origin is None):
        raise ValueError("base_shape and origin must both be given or both be None")
    _check_coordinates(x, y, z)
    if not isinstance(x, torch.Tensor) or x.device.type != "cuda":
        raise TypeError("plan_vr_layout: device tensors expected")
    if base_shape is None:
        base_shape, origin = plan_vr_base_grid(x, y, base_resolution)
    planner = VRLayoutPlanner(base_shape, origin, base_resolution, device=x.device)
    planner.add(x, y, z)
    return planner.plan(target_count, ladder, min_base_count)


class _VRPlanes:
    """What the two results share: flat ``[total]`` planes over the records of ``layout``."""
    layout: VRLayout
    valid: torch.Tensor

    def grid(self, base_row: int, base_col: int, plane: str) -> torch.Tensor:
        """One base cell's refinement grid of a plane as a ``[dy, dx]`` view, row 0 the southmost."""
        t = getattr(self, plane, None)
        if not isinstance(t, torch.Tensor) or t.shape != self.valid.shape:
            raise ValueError(f"plane={plane!r}: not a plane of this result")
        first, dy, dx = self.layout.grid_slice(base_row, base_col)
        return t[first:first + dy * dx].view(dy, dx)

    def _records(self, depth_t: torch.Tensor, unc_t: torch.Tensor) -> torch.Tensor:
        ok = self.valid != 0
        nodata = torch.tensor(RECORD_NODATA, dtype=torch.float32, device=depth_t.device)
        return torch.stack([torch.where(ok, depth_t, nodata), torch.where(ok, unc_t, nodata)], dim=1).contiguous()

    def _handler(self, records: torch.Tensor) -> VRBagHandler:
        host = np.ascontiguousarray(records.cpu().numpy()).view(VARRES_REFINEMENT_DTYPE).reshape(1, -1)
        return VRBagHandler.from_arrays(self.layout.metadata(), host, base_shape=self.layout.base_shape,
                                        geotransform=self.layout.geotransform)


@dataclasses.dataclass
class VRSoundingGrid(_VRPlanes):
    """What ``VRSoundingGridder.finalize`` leaves on the device: the planes of ``SoundingGrid`` as flat ``[total]`` tensors, one
    entry per record of ``layout``; ``counters`` with five entries."""
    count: torch.Tensor
    mean: torch.Tensor
    std: torch.Tensor
    min: torch.Tensor
    max: torch.Tensor
    valid: torch.Tensor
    counters: Dict[str, int]
    layout: VRLayout
    nodata_value: float = 1.0e6
    min_count: int = 1

    def density_plane(self) -> torch.Tensor:
        """``density_from_count(count)``, one entry per record of ``layout``."""
        return density_from_count(self.count)

    def records(self, depth: str = "mean", uncertainty: str = "std") -> torch.Tensor:
        """The ``[total, 2]`` float32 device tensor of (depth, depth_uncrt) records, 1.0e6 in both where the record is not valid."""
        return self._records(_pick_plane(self, depth, DEPTH_PLANES, "depth"), _pick_plane(self, uncertainty, UNCERTAINTY_PLANES, "uncertainty"))

    def handler(self, depth: str = "mean", uncertainty: str = "std") -> VRBagHandler:
        """A ``VRBagHandler`` over ``layout.metadata()`` and the records (one copy to the host), geotransform
        ``(x0, B, 0, y0 + BH * B, 0, -B)``: what ``compute_ground_truth_native`` and ``process_refinements`` take."""
        return self._handler(self.records(depth, uncertainty))


@dataclasses.dataclass
class RobustVRSoundingGrid(_VRPlanes):
    """What ``RobustVRSoundingGridder.finalize`` leaves on the device: the planes of ``RobustSoundingGrid`` as flat ``[total]``
    tensors, ``sorted_q`` and ``start`` (``total + 1``) as there."""
    count: torch.Tensor
    kept: torch.Tensor
    median: torch.Tensor
    mad: torch.Tensor
    kept_mean: torch.Tensor
    kept_std: torch.Tensor
    kept_min: torch.Tensor
    kept_max: torch.Tensor
    valid: torch.Tensor
    center2: torch.Tensor
    limit: torch.Tensor
    sorted_q: torch.Tensor
    start: torch.Tensor
    counters: Dict[str, int]
    layout: VRLayout
    nodata_value: float = 1.0e6
    min_count: int = 1
    k: float = DEFAULT_K
    floor_m: float = 0.0

    def hypotheses(self, gap_m, rule: str = "count", guide=None, min_count=None, records: bool = True):
        """As ``RobustSoundingGrid.hypotheses``, per record of ``layout`` (``guide``: a flat ``[total]`` tensor): a
        ``VRHypothesisGrid``.  ``rule="locale"`` is for uniform grids: ``ValueError`` here."""
        from .sounding_hypotheses import hypotheses_of_records
        return hypotheses_of_records(self, gap_m, rule, guide, min_count, records)

    def density_plane(self) -> torch.Tensor:
        """``density_from_count(kept)``, one entry per record of ``layout``."""
        return density_from_count(self.kept)

    def records(self, depth: str = "median", uncertainty: str = "kept_std") -> torch.Tensor:
        """The ``[total, 2]`` float32 device tensor of (depth, depth_uncrt) records, 1.0e6 in both where the record is not valid."""
        return self._records(_pick_plane(self, depth, ROBUST_DEPTH_PLANES, "depth"),
                             _pick_plane(self, uncertainty, ROBUST_UNCERTAINTY_PLANES, "uncertainty"))

    def handler(self, depth: str = "median", uncertainty: str = "kept_std") -> VRBagHandler:
        """As ``VRSoundingGrid.handler``."""
        return self._handler(self.records(depth, uncertainty))


class _VRGridderBase(_GridderBase):
    """The geometry and the ``unrefined`` counter of the two gridders."""

    def _init_layout(self, layout: VRLayout, device, min_count, nodata_value):
        if not isinstance(layout, VRLayout):
            raise TypeError("layout: a VRLayout expected")
        if layout.total < 1:
            raise ValueError("layout: no refinement grid, nothing to file soundings under")
        self.layout = layout
        self.min_count = _check_min_count(min_count)
        self.nodata_value = float(nodata_value)
        self.device = layout.device if device is None else rt.resolve_device(device)
        if layout.table.device != self.device:
            raise TypeError(f"the layout is on {layout.table.device}, the gridder on {self.device}")
        self._ctx = rt.get_context(self.device)
        self._unrefined = torch.zeros(1, dtype=torch.int64, device=self.device)

    def _cloud_args(self, x, y, z):
        lay = self.layout
        return (rt.ptr(x), rt.ptr(y), rt.ptr(z), int(x.shape[0]), lay.origin[0], lay.origin[1], lay.base_resolution, lay.base_shape[0],
                lay.base_shape[1], rt.ptr(lay.table), lay.total)


class VRSoundingGridder(_VRGridderBase):
    """``SoundingGridder`` on a ``VRLayout``: ``add(x, y, z)`` as often as the survey has line files, then ``finalize()``; more may
    be added after a ``finalize``.  The state takes 40 bytes per record of the layout.  At most 2^31 - 1 soundings in all."""

    def __init__(self, layout: VRLayout, device=None, min_count: int = 1, nodata_value: float = 1.0e6):
        self._init_layout(layout, device, min_count, nodata_value)
        self._state = self._buffer = _new_state(self._ctx, 1, layout.total, self.device)
        assert self._state.numel() * 8 == layout.state_bytes
        self._reset_call = ("bgnn_soundings_reset", rt.ptr(self._state), 1, layout.total)

    def _offer(self, x, y, z, n):
        self._call("bgnn_vr_soundings_add", *self._cloud_args(x, y, z), self.offered, rt.ptr(self._state), rt.ptr(self._unrefined))

    def finalize(self) -> VRSoundingGrid:
        """The planes of everything added so far (``bgnn_soundings_finalize`` on a ``1 x total`` grid).  Reads the state only."""
        total = self.layout.total
        planes = _finalize_plain(self._ctx, self._state, 1, total, total, self.min_count, self.nodata_value)
        return VRSoundingGrid(**planes, counters=self.counters(), layout=self.layout, nodata_value=self.nodata_value,
                              min_count=self.min_count)


class RobustVRSoundingGridder(_VRGridderBase):
    """``RobustSoundingGridder`` on a ``VRLayout``: up to ``capacity`` soundings staged as (record, q), ``finalize`` sorts every
    record's soundings and reads median, MAD and the kept statistics off them; ``flag`` applies a result's rule to any soundings."""

    def __init__(self, layout: VRLayout, capacity, device=None, k: float = DEFAULT_K, floor_m: float = 0.0, min_count: int = 1,
                 nodata_value: float = 1.0e6):
        self.capacity, self.k, self.floor_m = _check_robust_rule(capacity, k, floor_m)
        self._init_layout(layout, device, min_count, nodata_value)
        self._stage = self._buffer = _new_stage(self._ctx, self.capacity, self.device)
        self._reset_call = ("bgnn_soundings_robust_reset", rt.ptr(self._stage))

    def _offer(self, x, y, z, n):
        self._call("bgnn_vr_soundings_stage", *self._cloud_args(x, y, z), self.offered, self.capacity, rt.ptr(self._stage),
                   rt.ptr(self._unrefined))

    def finalize(self) -> RobustVRSoundingGrid:
        """The planes and the per-record sounding lists of everything added so far (``bgnn_soundings_robust_finalize`` on a
        ``1 x total`` grid).  Reads the stage only."""
        total = self.layout.total
        out = _finalize_robust(self._ctx, self._stage, self.offered, self.capacity, 1, total, total, self.k, self.floor_m, self.min_count,
                               self.nodata_value)
        return RobustVRSoundingGrid(**out, counters=self.counters(), layout=self.layout, nodata_value=self.nodata_value,
                                    min_count=self.min_count, k=self.k, floor_m=self.floor_m)

    def flag(self, x, y, z, grid: RobustVRSoundingGrid) -> torch.Tensor:
        """One uint8 per sounding under the rule of ``grid`` (a ``finalize`` on this gridder's layout): 0 kept, 1 accepted but
        farther than the record's limit from its median, 2 not accepted (nonfinite, outside, unrefined, out of range).
        Stateless.  Device tensors."""
        _check_coordinates(x, y, z)
        if not isinstance(x, torch.Tensor):
            raise TypeError("flag: device tensors expected")
        if grid.layout is not self.layout or int(grid.center2.shape[0]) != self.layout.total:
            raise ValueError("flag: the grid is not one of this gridder's layout")
        x, y, z = _on_device(x, y, z, self.device)
        flags = torch.empty(int(x.shape[0]), dtype=torch.uint8, device=self.device)
        self._call("bgnn_vr_soundings_flag", *self._cloud_args(x, y, z), rt.ptr(grid.center2), rt.ptr(grid.limit), rt.ptr(flags))
        return flags
