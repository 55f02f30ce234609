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

    def _depth(self, depth: str) -> torch.Tensor:
        if depth not in DEPTH_PLANES:
            raise ValueError(f"depth={depth!r}: one of {DEPTH_PLANES} expected")
        return getattr(self, depth)

    def density_plane(self) -> torch.Tensor:
        """``density_from_count(count)``: the node plane "sounding_density"."""
        return density_from_count(self.count)

    def survey_tensors(self, depth: str = "mean", density: bool = False):
        """``(depth_t, valid_t, unc_t)`` as ``BathymetricPipeline.process_survey_device`` takes them: the chosen surface
        (``"mean"``, the shoalest ``"min"`` or the deepest ``"max"`` of the raw z), the valid plane and ``std`` as uncertainty.
        ``density=True``: ``density_plane()`` as a fourth element (``process_survey_device(..., density_t=...)``)."""
        if density:
            return self._depth(depth), self.valid, self.std, self.density_plane()
        return self._depth(depth), self.valid, self.std

    def to_grid(self, depth: str = "mean") -> BathymetricGrid:
        """A host ``BathymetricGrid``: the chosen surface, ``std`` as uncertainty, ``density_plane()`` as density, the nodata
        value, transform, resolution and bounds ``(min_x, min_y, max_x, max_y)``."""
        height, width = (int(v) for v in self.count.shape)
        x0, res, _, y0, _, _ = self.transform
        return BathymetricGrid(depth=self._depth(depth).cpu().numpy(), uncertainty=self.std.cpu().numpy(),
                               nodata_value=self.nodata_value, transform=self.transform, resolution=self.resolution,
                               bounds=(x0, y0 - height * res, x0 + width * res, y0), density=self.density_plane().cpu().numpy())


class SoundingGridder:
    """``add(x, y, z)`` as often as the survey has line files, then ``finalize()``; more may be added after a ``finalize``.
    ``shape = (H, W)``, ``origin = (x0, y0)`` the upper-left corner, ``resolution`` the cell size in metres.  Device tensors are
    taken as they lie; host arrays are uploaded ``UPLOAD_CHUNK`` (2^24) soundings at a time.  ``min_count``: the soundings a
    cell needs to be valid.  At most 2^31 - 1 soundings may be offered in all (``ValueError`` beyond, before anything is launched)."""

    def __init__(self, shape, origin, resolution, device=None, min_count: int = 1, nodata_value: float = 1.0e6):
        self.shape = (int(shape[0]), int(shape[1]))
        self.origin = (float(origin[0]), float(origin[1]))
        self.resolution = _check_resolution(resolution)
        self.min_count = int(min_count)
        self.nodata_value = float(nodata_value)
        if self.shape[0] < 1 or self.shape[1] < 1:
            raise ValueError(f"shape {self.shape}: at least one row and one column expected")
        if self.min_count < 1:
            raise ValueError(f"min_count {min_count}: at least 1 expected")
        if not all(math.isfinite(v) for v in self.origin):
            raise ValueError(f"origin {self.origin}: finite coordinates expected")
        self.device = rt.resolve_device(device)
        self._ctx = rt.get_context(self.device)
        nbytes = int(self._ctx.lib.bgnn_soundings_state_bytes(*self.shape))
        if nbytes == 0:
            raise ValueError(f"shape {self.shape}: no state of that size")
        assert nbytes == rt.SOUNDINGS_HEADER_BYTES + CELL_BYTES * self.shape[0] * self.shape[1]
        self._state = torch.zeros(nbytes // 8, dtype=torch.int64, device=self.device)       # an all-zero state is the empty one
        self.offered = 0

    def reset(self):
        ctx = self._ctx
        ctx.begin()
        rt.check(ctx.lib.bgnn_soundings_reset(ctx.handle, rt.ptr(self._state), *self.shape))
        ctx.end()
        self.offered = 0

    def _add_device(self, x: torch.Tensor, y: torch.Tensor, z: torch.Tensor):
        n = int(x.shape[0])
        x, y, z = _on_device(x, y, z, self.device)
        ctx = self._ctx
        ctx.begin()
        rt.check(ctx.lib.bgnn_soundings_add(ctx.handle, rt.ptr(x), rt.ptr(y), rt.ptr(z), n, self.origin[0], self.origin[1],
                                            self.resolution, self.shape[0], self.shape[1], self.offered, rt.ptr(self._state)))
        ctx.end()
        self.offered += n

    def add(self, x, y, z):
        """File one set of soundings.  No host wait for device tensors."""
        _check_coordinates(x, y, z)
        n = int(x.shape[0])
        if self.offered + n > MAX_TOTAL:
            raise ValueError(f"{n} soundings after {self.offered} offered before: a total above {MAX_TOTAL}")
        _feed(x, y, z, self.device, self._add_device)

    def counters(self) -> Dict[str, int]:
        """``accepted``, ``nonfinite``, ``outside``, ``out_of_range`` over everything added: one 32-byte copy to the host."""
        head = self._state[:rt.SOUNDINGS_HEADER_BYTES // 8].cpu().numpy()
        return {name: int(v) for name, v in zip(rt.SOUNDINGS_COUNTERS, head)}

    def finalize(self) -> SoundingGrid:
        """The planes of everything added so far.  Reads the state only."""
        ctx, dev = self._ctx, self.device
        f32 = lambda: torch.empty(self.shape, dtype=torch.float32, device=dev)
        count = torch.empty(self.shape, dtype=torch.int32, device=dev)
        valid = torch.empty(self.shape, dtype=torch.uint8, device=dev)
        mean, std, zmin, zmax = f32(), f32(), f32(), f32()
        ctx.begin()
        rt.check(ctx.lib.bgnn_soundings_finalize(ctx.handle, rt.ptr(self._state), self.shape[0], self.shape[1], self.min_count,
                                                 self.nodata_value, rt.ptr(count), rt.ptr(mean), rt.ptr(std), rt.ptr(zmin), rt.ptr(zmax),
                                                 rt.ptr(valid)))
        ctx.end()
        res = self.resolution
        return SoundingGrid(count=count, mean=mean, std=std, min=zmin, max=zmax, valid=valid, counters=self.counters(),
                            transform=(self.origin[0], res, 0.0, self.origin[1], 0.0, -res), resolution=(res, res),
                            nodata_value=self.nodata_value, min_count=self.min_count)


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
