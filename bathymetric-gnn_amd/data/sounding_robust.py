"""Robust gridding of soundings on the device: per cell the median, the median absolute deviation and a kept / rejected flag per
sounding, where ``SoundingGridder`` (data/sounding_grid.py) streams sums that one bad sounding moves.

The reference rejects survey pairs because their noise "exists in the point cloud but not in the gridded surface"
(``docs/LESSONS_LEARNED.md`` section 6) and wants per-cell sounding evidence as "the strongest noise discriminator"
(``docs/TRAINING_DASHBOARD.md`` "Next Steps" 5).  With the soundings of a cell together there is a surface that outliers do not
move (``median``), a robust spread (``mad``), and point-cloud cleaning: ``flag`` says which soundings a cell's rule rejects, and
``SoundingGrid.mean`` against ``RobustSoundingGrid.kept_mean`` of one cloud is a noisy / clean pair for ``compute_ground_truth``.

``RobustSoundingGridder`` owns one stage of ``bgnn_soundings_robust_add`` (include/bgnn_soundings_robust.h): ``capacity`` slots
of (cell, q), q = rint(z * 65536), 8 bytes per sounding, filled over as many ``add`` calls as the survey has line files.
``finalize`` files the stage by cell, sorts every cell's soundings and reads the planes off the sorted segments; it leaves the
stage as it is, so more may be added and ``finalize`` run again.  Grid, acceptance, counters and quantisation are those of
``SoundingGridder``.  The rule of a cell, all in integers but the limit: ``m2`` = twice the median, ``d = |2q - m2|``, ``D`` =
twice the MAD of the ``d``, kept iff ``d <= floor(max(k * D / 2, floor_m * 2^17))``.  ``k`` is the multiplier of the MAD itself
(the default 3 * 1.4826 is three sigma of a normal spread), ``floor_m`` a distance in metres inside which nothing is rejected.
Every plane and every flag is a function of the multiset of soundings: equal bits in any order, in any split over calls, on
every run.  Limits: ``H * W <= 2^31 - 1`` cells, ``capacity <= 2^31 - 1`` soundings."""
from __future__ import annotations

import dataclasses
from typing import Dict, Tuple

import torch

from .. import runtime as rt
from .grid import BathymetricGrid
from .sounding_grid import (_GridderBase, _check_coordinates, _check_min_count, _check_origin, _check_resolution, _check_robust_rule,
                            _check_shape, _finalize_robust, _new_stage, _on_device, _pick_plane, density_from_count, plan_sounding_grid)

DEFAULT_K = 3 * 1.4826
ROBUST_DEPTH_PLANES = ("median", "kept_mean", "kept_min", "kept_max")
ROBUST_UNCERTAINTY_PLANES = ("kept_std", "mad")
FLAG_KEPT, FLAG_REJECTED, FLAG_NOT_ACCEPTED = 0, 1, 2


@dataclasses.dataclass
class RobustSoundingGrid:
    """What ``RobustSoundingGridder.finalize`` leaves on the device.  ``[H, W]`` planes: ``count`` and ``kept`` (int32, true also
    where the cell is not valid), ``median``, ``mad`` (not scaled by 1.4826), ``kept_mean``, ``kept_std``, ``kept_min``,
    ``kept_max`` (float32, ``nodata_value`` where not valid), ``valid`` (uint8: ``kept >= min_count``), ``center2`` and ``limit``
    (int64: the rule ``flag`` applies; ``limit == -1`` in an empty cell).  The per-cell sounding lists: ``sorted_q`` (int32,
    ``capacity`` entries, units of 2^-16 m) holds cell ``c``'s soundings ascending at ``start[c] .. start[c + 1]`` (``start``: uint32
    bits in an int32 tensor of ``H * W + 1``)."""
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
    transform: Tuple[float, float, float, float, float, float]
    resolution: Tuple[float, float]
    nodata_value: float = 1.0e6
    min_count: int = 1
    k: float = DEFAULT_K
    floor_m: float = 0.0

    def cell_soundings(self, row: int, col: int) -> torch.Tensor:
        """The soundings of one cell, ascending, in metres (float64: ``q * 2^-16`` is exact).  Two small copies to the host."""
        height, width = (int(v) for v in self.count.shape)
        if not (0 <= row < height and 0 <= col < width):
            raise IndexError(f"cell ({row}, {col}) of a {height} x {width} grid")
        cell = row * width + col
        lo, hi = (int(v) & 0xFFFFFFFF for v in self.start[cell:cell + 2].tolist())
        return self.sorted_q[lo:hi].to(torch.float64) * (2.0 ** -16)

    def hypotheses(self, gap_m, rule: str = "count", guide=None, min_count=None, records: bool = True, radius=None, min_support=None):
        """The depth hypotheses of every cell (data/sounding_hypotheses.py): the runs of its sorted soundings without a gap of
        more than ``gap_m`` metres (required, finite, 0 .. 65536: what separates two surfaces is the survey's to say), and one
        chosen per cell -- ``rule="count"``: the most soundings, then the nearest to the cell's median; ``rule="guide"``: the
        nearest to ``guide`` (a float32 device tensor ``[H, W]``), then the most soundings; ``rule="locale"``
        (data/locale_guide.py): by a guide made here, the median of the cells within ``radius`` (default 2, 1 .. 8) that have
        one hypothesis only, by count where fewer than ``min_support`` (default 3) of them are found; the result carries that
        ``guide`` and its ``support``.  ``radius`` and ``min_support`` go with ``rule="locale"`` alone, which takes no ``guide``.
        ``min_count`` defaults to this grid's; ``records=False`` leaves the per-hypothesis records out.  A ``HypothesisGrid``."""
        from .sounding_hypotheses import hypotheses_of_grid
        return hypotheses_of_grid(self, gap_m, rule, guide, min_count, records, radius, min_support)

    def density_plane(self) -> torch.Tensor:
        """``density_from_count(kept)``: the node plane "sounding_density" over the soundings the rule kept."""
        return density_from_count(self.kept)

    def survey_tensors(self, depth: str = "median", uncertainty: str = "kept_std", density: bool = False):
        """``(depth_t, valid_t, unc_t)`` as ``BathymetricPipeline.process_survey_device`` takes them; ``density=True``:
        ``density_plane()`` as a fourth element."""
        t = (_pick_plane(self, depth, ROBUST_DEPTH_PLANES, "depth"), self.valid,
             _pick_plane(self, uncertainty, ROBUST_UNCERTAINTY_PLANES, "uncertainty"))
        return t + (self.density_plane(),) if density else t

    def to_grid(self, depth: str = "median", uncertainty: str = "kept_std") -> BathymetricGrid:
        """A host ``BathymetricGrid`` of the chosen surface and uncertainty, as ``SoundingGrid.to_grid``."""
        height, width = (int(v) for v in self.count.shape)
        x0, res, _, y0, _, _ = self.transform
        depth_t, _, unc_t = self.survey_tensors(depth, uncertainty)
        return BathymetricGrid(depth=depth_t.cpu().numpy(), uncertainty=unc_t.cpu().numpy(), nodata_value=self.nodata_value,
                               transform=self.transform, resolution=self.resolution,
                               bounds=(x0, y0 - height * res, x0 + width * res, y0), density=self.density_plane().cpu().numpy())


class RobustSoundingGridder(_GridderBase):
    """``add(x, y, z)`` as often as the survey has line files, up to ``capacity`` soundings in all (``ValueError`` beyond, before
    anything is launched), then ``finalize()``; more may be added after a ``finalize``.  ``shape``, ``origin``, ``resolution``,
    ``min_count``, ``nodata_value`` as for ``SoundingGridder``; ``k`` (finite, >= 1) and ``floor_m`` (finite, >= 0) set the rule.
    Memory: 8 bytes per sounding of capacity for the stage; ``finalize`` returns 4 more per sounding (``sorted_q``) and 49 per cell
    (the planes and ``start``) and uses a workspace of 4 per sounding and 4 per cell while it runs."""

    def __init__(self, shape, origin, resolution, capacity, device=None, k: float = DEFAULT_K, floor_m: float = 0.0,
                 min_count: int = 1, nodata_value: float = 1.0e6):
        self.resolution = _check_resolution(resolution)
        self.shape = _check_shape(shape)
        if self.shape[0] * self.shape[1] > rt.ROBUST_MAX_CELLS:
            raise NotImplementedError(f"shape {self.shape}: more than {rt.ROBUST_MAX_CELLS} cells")
        self.capacity, self.k, self.floor_m = _check_robust_rule(capacity, k, floor_m)
        self.min_count = _check_min_count(min_count)
        self.origin = _check_origin(origin)
        self.nodata_value = float(nodata_value)
        self.device = rt.resolve_device(device)
        self._ctx = rt.get_context(self.device)
        self._stage = self._buffer = _new_stage(self._ctx, self.capacity, self.device)
        self._reset_call = ("bgnn_soundings_robust_reset", rt.ptr(self._stage))

    def _offer(self, x, y, z, n):
        self._call("bgnn_soundings_robust_add", rt.ptr(x), rt.ptr(y), rt.ptr(z), n, self.origin[0], self.origin[1], self.resolution,
                   self.shape[0], self.shape[1], self.offered, self.capacity, rt.ptr(self._stage))

    def finalize(self) -> RobustSoundingGrid:
        """The planes and the per-cell sounding lists of everything added so far.  Reads the stage only."""
        out = _finalize_robust(self._ctx, self._stage, self.offered, self.capacity, self.shape[0], self.shape[1], self.shape, self.k,
                               self.floor_m, self.min_count, self.nodata_value)
        res = self.resolution
        return RobustSoundingGrid(**out, counters=self.counters(), transform=(self.origin[0], res, 0.0, self.origin[1], 0.0, -res),
                                  resolution=(res, res), nodata_value=self.nodata_value, min_count=self.min_count, k=self.k,
                                  floor_m=self.floor_m)

    def flag(self, x, y, z, grid: RobustSoundingGrid) -> torch.Tensor:
        """One uint8 per sounding under the rule of ``grid`` (a ``finalize`` of this gridder's geometry): 0 kept, 1 accepted but
        farther than the cell's limit from its median (every accepted sounding of a cell that ``finalize`` saw empty), 2 not
        accepted (nonfinite, outside, out of range).  Stateless: any soundings, those that were added or others.  Device tensors."""
        _check_coordinates(x, y, z)
        if not isinstance(x, torch.Tensor):
            raise TypeError("flag: device tensors expected")
        if tuple(grid.center2.shape) != self.shape or grid.transform[:4] != (self.origin[0], self.resolution, 0.0, self.origin[1]):
            raise ValueError("flag: the grid is not one of this gridder's geometry")
        x, y, z = _on_device(x, y, z, self.device)
        n = int(x.shape[0])
        flags = torch.empty(n, dtype=torch.uint8, device=self.device)
        self._call("bgnn_soundings_robust_flag", rt.ptr(x), rt.ptr(y), rt.ptr(z), n, self.origin[0], self.origin[1], self.resolution,
                   self.shape[0], self.shape[1], rt.ptr(grid.center2), rt.ptr(grid.limit), rt.ptr(flags))
        return flags


def grid_soundings_robust(x, y, z, resolution, shape=None, origin=None, capacity=None, device=None, k: float = DEFAULT_K,
                          floor_m: float = 0.0, min_count: int = 1, nodata_value: float = 1.0e6) -> RobustSoundingGrid:
    """Plan (unless ``shape`` and ``origin`` are given), add, finalize in one call; ``capacity`` defaults to the number of soundings."""
    if (shape is None) != (origin is None):
        raise ValueError("shape and origin must both be given or both be None")
    _check_coordinates(x, y, z)
    if shape is None:
        shape, origin = plan_sounding_grid(x, y, resolution)
    if device is None and isinstance(x, torch.Tensor) and x.device.type == "cuda":
        device = x.device
    g = RobustSoundingGridder(shape, origin, resolution, capacity=max(1, int(x.shape[0])) if capacity is None else capacity,
                              device=device, k=k, floor_m=floor_m, min_count=min_count, nodata_value=nodata_value)
    g.add(x, y, z)
    return g.finalize()
