"""Gridding soundings on the device: a point cloud (x, y, z) in, the depth, spread and density planes out, in HBM.

The reference's loader stops in front of this step (``BathymetricLoader._load_xyz`` raises ``NotImplementedError("XYZ point cloud
loading requires gridding...")``), and its documents keep asking for what it gives: ``docs/TRAINING_DASHBOARD.md`` "Next Steps" 5
(a per-cell sounding count "would be the strongest noise discriminator"), ``docs/LESSONS_LEARNED.md`` section 6 (noise that
"exists in the point cloud but not in the gridded surface").

``SoundingGridder`` owns one state of ``bgnn_soundings_add`` (include/bgnn_soundings.h): per cell the count, the exact integer sums
of ``q = rint(z * 65536)`` and of ``q * q``, and the exact float32 extremes, added up over as many ``add`` calls as the survey has
line files.  ``finalize`` forms the planes (``count``, ``mean``, ``std``, ``min``, ``max``, ``valid``) and leaves the state as it
is.  Every sum is an integer, so the planes are the same bits in any order of the points, in any split over calls, on every run.

The contract in short (the header has all of it): x, y float64 projected metres (float32 coordinates are refused: at UTM
magnitudes float32 resolves 3 cm), z float32; ``col = floor((x - x0) / res)``, ``row = floor((y0 - y) / res)`` in float64 with a true
division, (x0, y0) the upper-left corner; cells half-open; a sounding is accepted when x, y, z are finite, the cell is on the grid
and ``|z| < 32768``; the others are counted (``nonfinite``, ``outside``, ``out_of_range``, checked in that order), never silently
dropped.  ``mean`` of a one-sounding cell is the sounding rounded to 2^-16 m (at most 7.6 um off); ``min`` / ``max`` return it
exactly.  ``std`` is the population standard deviation (0 for one sounding).  Limits: at most 2^31 - 1 soundings offered to one
gridder over all ``add`` calls; the state takes 40 bytes per cell."""
from __future__ import annotations

import dataclasses
import math
from typing import Dict, Optional, Tuple

import numpy as np
import torch

from .. import runtime as rt
from .grid import BathymetricGrid

UPLOAD_CHUNK = 1 << 24          # soundings per upload of a host array: 320 MB of x, y, z on the device at a time
MAX_TOTAL = rt.SOUNDINGS_MAX_TOTAL
CELL_BYTES = rt.SOUNDINGS_CELL_BYTES
DEPTH_PLANES = ("mean", "min", "max")


def _check_resolution(resolution) -> float:
    res = float(resolution)
    if not (math.isfinite(res) and res > 0):
        raise ValueError(f"resolution {resolution!r}: a finite number above 0 expected")
    return res


def _check_coordinates(x, y, z=None):
    """x, y: float64 vectors of one length (numpy or torch); z, when given, float32 of that length."""
    def is_dtype(a, np_type, torch_type):
        return a.dtype == torch_type if isinstance(a, torch.Tensor) else a.dtype == np_type
    for name, a in (("x", x), ("y", y)):
        if not isinstance(a, (np.ndarray, torch.Tensor)) or a.ndim != 1:
            raise TypeError(f"{name}: a 1-D numpy array or torch tensor expected")
        if not is_dtype(a, np.float64, torch.float64):
            raise TypeError(f"{name}: float64 coordinates expected, got {a.dtype} (float32 resolves 3 cm at UTM magnitudes)")
    if x.shape[0] != y.shape[0]:
        raise ValueError(f"x and y disagree on the number of soundings: {x.shape[0]} and {y.shape[0]}")
    if z is not None:
        if not isinstance(z, (np.ndarray, torch.Tensor)) or z.ndim != 1:
            raise TypeError("z: a 1-D numpy array or torch tensor expected")
        if not is_dtype(z, np.float32, torch.float32):
            raise TypeError(f"z: float32 depths expected, got {z.dtype}")
        if z.shape[0] != x.shape[0]:
            raise ValueError(f"x and z disagree on the number of soundings: {x.shape[0]} and {z.shape[0]}")
    kinds = {isinstance(a, torch.Tensor) for a in (x, y) + (() if z is None else (z,))}
    if len(kinds) != 1:
        raise TypeError("x, y and z must be all numpy arrays or all torch tensors")


def _on_device(x, y, z, device):
    """x, y, z as contiguous tensors, all of them on ``device`` already (``TypeError`` otherwise)."""
    for name, t in (("x", x), ("y", y), ("z", z)):
        if t.device != device:
            raise TypeError(f"{name} is on {t.device}, the gridder on {device}")
    return x.contiguous(), y.contiguous(), z.contiguous()


def _feed(x, y, z, device, add_device):
    """The checked x, y, z to ``add_device(x, y, z)``: device tensors as they lie, host arrays ``UPLOAD_CHUNK`` soundings at a time
    (one call each); nothing for an empty set.  Shared by the gridders."""
    n = int(x.shape[0])
    if n == 0:
        return
    if isinstance(x, torch.Tensor) and x.device.type == "cuda":
        add_device(x, y, z)
        return
    as_tensor = (lambda a: a) if isinstance(x, torch.Tensor) else (lambda a: torch.from_numpy(np.ascontiguousarray(a)))
    for lo in range(0, n, UPLOAD_CHUNK):
        hi = min(n, lo + UPLOAD_CHUNK)
        add_device(*(as_tensor(a[lo:hi]).to(device) for a in (x, y, z)))


def _check_shape(shape, what: str = "shape") -> Tuple[int, int]:
    shape = (int(shape[0]), int(shape[1]))
    if shape[0] < 1 or shape[1] < 1:
        raise ValueError(f"{what} {shape}: at least one row and one column expected")
    return shape


def _check_origin(origin) -> Tuple[float, float]:
    origin = (float(origin[0]), float(origin[1]))
    if not all(math.isfinite(v) for v in origin):
        raise ValueError(f"origin {origin}: finite coordinates expected")
    return origin


def _check_min_count(min_count) -> int:
    if int(min_count) < 1:
        raise ValueError(f"min_count {min_count}: at least 1 expected")
    return int(min_count)


def _check_robust_rule(capacity, k, floor_m) -> Tuple[int, float, float]:
    """The capacity of a stage and the rule of the robust gridders, as ``(int, float, float)``."""
    if not 1 <= int(capacity) <= rt.ROBUST_MAX_CAPACITY:
        raise ValueError(f"capacity {capacity}: 1 .. {rt.ROBUST_MAX_CAPACITY} soundings expected")
    if not (math.isfinite(float(k)) and float(k) >= 1):
        raise ValueError(f"k {k!r}: a finite number of at least 1 expected")
    if not (math.isfinite(float(floor_m)) and float(floor_m) >= 0):
        raise ValueError(f"floor_m {floor_m!r}: a finite number of at least 0 expected")
    return int(capacity), float(k), float(floor_m)


def _pick_plane(result, name: str, allowed, what: str) -> torch.Tensor:
    """The plane ``name`` of a finalize result, one of ``allowed``; ``what``: the argument the name came in."""
    if name not in allowed:
        raise ValueError(f"{what}={name!r}: one of {allowed} expected")
    return getattr(result, name)


def _call(ctx, fn: str, *args):
    ctx.begin()
    rt.check(getattr(ctx.lib, fn)(ctx.handle, *args))
    ctx.end()


class _OfferedSoundings:
    """Something that is offered soundings over many ``add`` calls, on ``self.device`` under ``self._ctx``: ``offered`` so far, of
    at most ``self.capacity`` where the class has one and ``MAX_TOTAL`` otherwise.  A subclass hands one set of device tensors on
    in ``_offer(x, y, z, n)``."""
    offered = 0
    capacity = None

    def _call(self, fn: str, *args):
        _call(self._ctx, fn, *args)

    def _add_device(self, x: torch.Tensor, y: torch.Tensor, z: torch.Tensor):
        n = int(x.shape[0])
        self._offer(*_on_device(x, y, z, self.device), n)
        self.offered += n

    def add(self, x, y, z):
        """Offer one set of soundings (``ValueError`` beyond the limit, before anything is launched).  No host wait for device
        tensors."""
        _check_coordinates(x, y, z)
        n = int(x.shape[0])
        limit, what = (MAX_TOTAL, f"a total above {MAX_TOTAL}") if self.capacity is None else \
            (self.capacity, f"more than the capacity of {self.capacity}")
        if self.offered + n > limit:
            raise ValueError(f"{n} soundings after {self.offered} offered before: {what}")
        _feed(x, y, z, self.device, self._add_device)


class _GridderBase(_OfferedSoundings):
    """A gridder: ``self._buffer`` is its state or stage with the four counters in front, ``self._reset_call`` the arguments of
    ``_call`` that empty it; ``self._unrefined``, where the gridder has one, is the fifth counter."""
    _unrefined = None

    def reset(self):
        self._call(*self._reset_call)
        if self._unrefined is not None:
            self._unrefined.zero_()
        self.offered = 0

    def counters(self) -> Dict[str, int]:
        """``accepted``, ``nonfinite``, ``outside``, ``out_of_range`` (and ``unrefined`` on a VR layout) over everything added:
        one small copy to the host."""
        assert rt.ROBUST_STAGE_HEADER_BYTES == rt.SOUNDINGS_HEADER_BYTES        # a state and a stage begin alike
        head = self._buffer[:rt.SOUNDINGS_HEADER_BYTES // 8]
        if self._unrefined is None:
            return {name: int(v) for name, v in zip(rt.SOUNDINGS_COUNTERS, head.cpu().numpy())}
        return {name: int(v) for name, v in zip(rt.VR_SOUNDINGS_COUNTERS, torch.cat([head, self._unrefined]).cpu().numpy())}


def _new_state(ctx, height: int, width: int, device) -> torch.Tensor:
    """An empty state of ``bgnn_soundings_add`` (all zero), or ``None`` where there is none of that size."""
    nbytes = int(ctx.lib.bgnn_soundings_state_bytes(height, width))
    assert nbytes in (0, rt.SOUNDINGS_HEADER_BYTES + CELL_BYTES * height * width)
    return torch.zeros(nbytes // 8, dtype=torch.int64, device=device) if nbytes else None


def _new_stage(ctx, capacity: int, device) -> torch.Tensor:
    """An empty stage of ``bgnn_soundings_robust_add``: an all-zero header in front of ``capacity`` slots."""
    nbytes = int(ctx.lib.bgnn_soundings_robust_stage_bytes(capacity))
    assert nbytes == rt.ROBUST_STAGE_HEADER_BYTES + rt.ROBUST_SLOT_BYTES * capacity
    stage = torch.empty(nbytes // 8, dtype=torch.int64, device=device)
    stage[:rt.ROBUST_STAGE_HEADER_BYTES // 8].zero_()
    return stage


def _finalize_plain(ctx, state, height, width, shape, min_count, nodata) -> Dict[str, torch.Tensor]:
    """``bgnn_soundings_finalize`` on a ``height x width`` state: the six planes, each of ``shape``.  Reads the state only."""
    dev = state.device
    p = {name: torch.empty(shape, dtype=dtype, device=dev) for name, dtype in (
        ("count", torch.int32), ("valid", torch.uint8), ("mean", torch.float32), ("std", torch.float32), ("min", torch.float32),
        ("max", torch.float32))}
    _call(ctx, "bgnn_soundings_finalize", rt.ptr(state), height, width, min_count, nodata,
          *(rt.ptr(p[name]) for name in ("count", "mean", "std", "min", "max", "valid")))
    return p


def _finalize_robust(ctx, stage, offered, capacity, height, width, shape, k, floor_m, min_count, nodata) -> Dict[str, torch.Tensor]:
    """``bgnn_soundings_robust_finalize`` on a stage of ``height x width`` cells: the eleven planes, each of ``shape`` (a tuple, or
    the number of records of a flat result), ``sorted_q`` and ``start``.  Reads the stage only."""
    dev, cells = stage.device, height * width
    ws_bytes = int(ctx.lib.bgnn_soundings_robust_workspace_bytes(height, width, capacity))
    if ws_bytes == 0:
        what = f"shape {shape}" if isinstance(shape, tuple) else f"{shape} records"
        raise ValueError(f"{what}, capacity {capacity}: no workspace of that size")
    ws = torch.empty(ws_bytes // 8, dtype=torch.int64, device=dev)
    out = {"start": torch.empty(cells + 1, dtype=torch.int32, device=dev), "sorted_q": torch.empty(capacity, dtype=torch.int32, device=dev)}
    out.update((name, torch.empty(shape, dtype=dtype, device=dev)) for name, dtype in (
        ("count", torch.int32), ("kept", torch.int32), ("median", torch.float32), ("mad", torch.float32), ("kept_mean", torch.float32),
        ("kept_std", torch.float32), ("kept_min", torch.float32), ("kept_max", torch.float32), ("valid", torch.uint8),
        ("center2", torch.int64), ("limit", torch.int64)))
    _call(ctx, "bgnn_soundings_robust_finalize", rt.ptr(stage), offered, capacity, height, width, k, floor_m, min_count, nodata, rt.ptr(ws),
          ws_bytes, *(rt.ptr(t) for t in out.values()))       # (the workspace may go: the caller's stream waits)
    return out


def sounding_extent(x: torch.Tensor, y: torch.Tensor) -> Dict[str, float]:
    """``bgnn_soundings_extent`` on device tensors: the float64 ``min_x``, ``max_x``, ``min_y``, ``max_y`` over the finite values of
    each coordinate and their counts ``finite_x``, ``finite_y`` (+inf / -inf / 0 where none is finite).  One small copy to the host."""
    _check_coordinates(x, y)
    dev = x.device
    if dev.type != "cuda" or y.device != dev:
        raise TypeError("sounding_extent: x and y on one GPU expected")
    ctx = rt.get_context(dev)
    x, y = x.contiguous(), y.contiguous()
    buf = torch.empty(rt.SOUNDINGS_EXTENT_BUFFER_BYTES // 8, dtype=torch.int64, device=dev)
    ctx.begin()
    rt.check(ctx.lib.bgnn_soundings_extent(ctx.handle, rt.ptr(x), rt.ptr(y), int(x.shape[0]), rt.ptr(buf)))
    ctx.end()
    words = rt.SOUNDINGS_EXTENT_DTYPE.itemsize // 8
    rec = np.frombuffer(buf[:words].cpu().numpy().tobytes(), dtype=rt.SOUNDINGS_EXTENT_DTYPE)[0]
    return {k: (int(rec[k]) if k.startswith("finite") else float(rec[k])) for k in rt.SOUNDINGS_EXTENT_DTYPE.names}


def plan_sounding_grid(x, y, resolution) -> Tuple[Tuple[int, int], Tuple[float, float]]:
    """The smallest grid on the lattice of multiples of ``resolution`` that holds every finite coordinate:
    ``((H, W), (x0, y0))`` with ``x0 = floor(min_x / res) * res``, ``y0 = ceil(max_y / res) * res``,
    ``W = floor((max_x - x0) / res) + 1`` and ``H = floor((y0 - min_y) / res) + 1``.  Where the rounding of ``k * res`` would leave
    the extreme point on the wrong side of the corner, the corner moves one cell outward: every sounding with finite x and y falls
    inside under the gridder's own arithmetic.  numpy arrays are planned with numpy (no GPU needed), device tensors with the extent
    kernel.  ``ValueError`` when x or y has no finite value."""
    res = _check_resolution(resolution)
    _check_coordinates(x, y)
    if isinstance(x, torch.Tensor) and x.device.type == "cuda":
        e = sounding_extent(x, y)
        nx, ny = e["finite_x"], e["finite_y"]
        min_x, max_x, min_y, max_y = e["min_x"], e["max_x"], e["min_y"], e["max_y"]
    else:
        xn = x.numpy() if isinstance(x, torch.Tensor) else x
        yn = y.numpy() if isinstance(y, torch.Tensor) else y
        fx, fy = xn[np.isfinite(xn)], yn[np.isfinite(yn)]
        nx, ny = fx.size, fy.size
        if nx and ny:
            min_x, max_x, min_y, max_y = float(fx.min()), float(fx.max()), float(fy.min()), float(fy.max())
    if nx == 0 or ny == 0:
        raise ValueError("plan_sounding_grid: no finite coordinate")
    x0 = math.floor(min_x / res) * res
    while x0 > min_x:
        x0 -= res
    y0 = math.ceil(max_y / res) * res
    while y0 < max_y:
        y0 += res
    width = math.floor((max_x - x0) / res) + 1
    height = math.floor((y0 - min_y) / res) + 1
    return (int(height), int(width)), (float(x0), float(y0))


def density_from_count(count: torch.Tensor) -> torch.Tensor:
    """The sounding density plane of a per-cell count: float32 ``1 / count`` where ``count >= 1``, ``0`` elsewhere -- one correctly
    rounded float32 division per cell, on the device the count lives on.  Bounded in (0, 1] and largest on single-hit cells, the
    cells the reference's dashboard calls "almost certainly noise"."""
    c = count.to(torch.float32)
    hit = count >= 1
    return torch.where(hit, torch.ones_like(c) / torch.where(hit, c, torch.ones_like(c)), torch.zeros_like(c))


@dataclasses.dataclass
class SoundingGrid:
    """What ``SoundingGridder.finalize`` leaves on the device: ``[H, W]`` tensors ``count`` (int32, the true count also where the
    cell is not valid), ``mean``, ``std``, ``min``, ``max`` (float32, ``nodata_value`` where not valid) and ``valid`` (uint8:
    ``count >= min_count``); the ``counters`` of the gridder at that moment; the GDAL ``transform`` ``(x0, res, 0, y0, 0, -res)``."""
    count: torch.Tensor
    mean: torch.Tensor
    std: torch.Tensor
    min: torch.Tensor
    max: torch.Tensor
    valid: torch.Tensor
    counters: Dict[str, int]
    transform: Tuple[float, float, float, float, float, float]
    resolution: Tuple[float, float]
    nodata_value: float = 1.0e6
    min_count: int = 1

    def density_plane(self) -> torch.Tensor:
        """``density_from_count(count)``: the node plane "sounding_density"."""
        return density_from_count(self.count)

    def survey_tensors(self, depth: str = "mean", density: bool = False):
        """``(depth_t, valid_t, unc_t)`` as ``BathymetricPipeline.process_survey_device`` takes them: the chosen surface
        (``"mean"``, the shoalest ``"min"`` or the deepest ``"max"`` of the raw z), the valid plane and ``std`` as uncertainty.
        ``density=True``: ``density_plane()`` as a fourth element (``process_survey_device(..., density_t=...)``)."""
        if density:
            return _pick_plane(self, depth, DEPTH_PLANES, "depth"), self.valid, self.std, self.density_plane()
        return _pick_plane(self, depth, DEPTH_PLANES, "depth"), self.valid, self.std

    def to_grid(self, depth: str = "mean") -> BathymetricGrid:
        """A host ``BathymetricGrid``: the chosen surface, ``std`` as uncertainty, ``density_plane()`` as density, the nodata
        value, transform, resolution and bounds ``(min_x, min_y, max_x, max_y)``."""
        height, width = (int(v) for v in self.count.shape)
        x0, res, _, y0, _, _ = self.transform
        return BathymetricGrid(depth=_pick_plane(self, depth, DEPTH_PLANES, "depth").cpu().numpy(), uncertainty=self.std.cpu().numpy(),
                               nodata_value=self.nodata_value, transform=self.transform, resolution=self.resolution,
                               bounds=(x0, y0 - height * res, x0 + width * res, y0), density=self.density_plane().cpu().numpy())


class SoundingGridder(_GridderBase):
    """``add(x, y, z)`` as often as the survey has line files, then ``finalize()``; more may be added after a ``finalize``.
    ``shape = (H, W)``, ``origin = (x0, y0)`` the upper-left corner, ``resolution`` the cell size in metres.  Device tensors are
    taken as they lie; host arrays are uploaded ``UPLOAD_CHUNK`` (2^24) soundings at a time.  ``min_count``: the soundings a
    cell needs to be valid.  At most 2^31 - 1 soundings may be offered in all (``ValueError`` beyond, before anything is launched)."""

    def __init__(self, shape, origin, resolution, device=None, min_count: int = 1, nodata_value: float = 1.0e6):
        self.resolution = _check_resolution(resolution)
        self.shape = _check_shape(shape)
        self.min_count = _check_min_count(min_count)
        self.origin = _check_origin(origin)
        self.nodata_value = float(nodata_value)
        self.device = rt.resolve_device(device)
        self._ctx = rt.get_context(self.device)
        self._state = self._buffer = _new_state(self._ctx, *self.shape, self.device)
        if self._state is None:
            raise ValueError(f"shape {self.shape}: no state of that size")
        self._reset_call = ("bgnn_soundings_reset", rt.ptr(self._state), *self.shape)

    def _offer(self, x, y, z, n):
        self._call("bgnn_soundings_add", rt.ptr(x), rt.ptr(y), rt.ptr(z), n, self.origin[0], self.origin[1], self.resolution,
                   self.shape[0], self.shape[1], self.offered, rt.ptr(self._state))

    def finalize(self) -> SoundingGrid:
        """The planes of everything added so far.  Reads the state only."""
        planes = _finalize_plain(self._ctx, self._state, self.shape[0], self.shape[1], self.shape, self.min_count, self.nodata_value)
        res = self.resolution
        return SoundingGrid(**planes, counters=self.counters(), transform=(self.origin[0], res, 0.0, self.origin[1], 0.0, -res),
                            resolution=(res, res), nodata_value=self.nodata_value, min_count=self.min_count)


def grid_soundings(x, y, z, resolution, shape=None, origin=None, device=None, min_count: int = 1,
                   nodata_value: float = 1.0e6) -> SoundingGrid:
    """Plan (unless ``shape`` and ``origin`` are given), add, finalize in one call."""
    if (shape is None) != (origin is None):
        raise ValueError("shape and origin must both be given or both be None")
    _check_coordinates(x, y, z)
    if shape is None:
        shape, origin = plan_sounding_grid(x, y, resolution)
    if device is None and isinstance(x, torch.Tensor) and x.device.type == "cuda":
        device = x.device
    g = SoundingGridder(shape, origin, resolution, device=device, min_count=min_count, nodata_value=nodata_value)
    g.add(x, y, z)
    return g.finalize()
