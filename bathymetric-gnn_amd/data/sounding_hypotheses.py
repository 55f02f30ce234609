"""Depth hypotheses per cell on the device: CUBE-style disambiguation from the sorted sounding lists of a robust gridding.

Both gridders return one depth per cell.  A cell that straddles a real step (a wreck, a pier face, a rock edge) or holds a dense
false cluster (a fish school, multipath) holds two surfaces; the mean and the median / MAD rule both land between them or on the
wrong one.  ``RobustSoundingGrid.hypotheses(gap_m)`` (and the same on ``RobustVRSoundingGrid``) cuts every cell's sorted soundings
into runs without a gap of more than ``gap_m`` -- one run, one depth hypothesis -- and chooses one per cell
(include/bgnn_hypotheses.h): under ``rule="count"`` the run with the most soundings, then the one nearest to the cell's median;
under ``rule="guide"`` the run nearest to a guide surface, then the one with the most soundings.  A guide is any float32 plane of
the result's shape; the usual one is the ``median`` of a coarser robust gridding of the same cloud, ``repeat_interleave``d to
this resolution (``guide_from_coarser``).  Cells whose guide is not finite or out of range fall back to the count rule.
``rule="locale"`` (uniform grids only, data/locale_guide.py) makes the guide itself: per cell the median of the neighbouring
cells that have exactly one hypothesis.

Everything is an integer function of the sorted lists: equal bits in any order of the cloud, in any split over ``add`` calls, on
every run.  ``center2`` / ``limit`` follow the robust planes' convention (``|2q - center2| <= limit`` iff the sounding lies inside
the chosen run), so ``RobustSoundingGridder.flag`` and ``RobustVRSoundingGridder.flag`` take a hypothesis result as they are: the
point cloud is cleaned by hypothesis without another pass.

Out of scope: CUBE's sequential Kalman estimator (it depends on the order of arrival), spreading a sounding over neighbouring
nodes, iterating the locale rule so that resolved cells become witnesses, the locale rule on variable-resolution layouts,
``ambiguity`` as a node plane of the model, and the streamed and sharded routes."""
from __future__ import annotations

import dataclasses
import math
from typing import Dict, List, Optional, Tuple

import numpy as np
import torch

from .. import runtime as rt
from .grid import BathymetricGrid
from .sounding_grid import _call, _check_min_count, _pick_plane, density_from_count
from .sounding_vr import VRLayout, _VRPlanes
from .vr_bag import VRBagHandler

HYPOTHESIS_PLANES = ("n_hyp", "chosen", "kept", "depth", "std", "min", "max", "share", "valid", "center2", "limit")
HYPOTHESIS_RECORDS = ("hyp_start", "hyp_first", "hyp_count")
HYPOTHESIS_DEPTH_PLANES = ("depth", "min", "max")
HYPOTHESIS_UNCERTAINTY_PLANES = ("std",)
MAX_GAP_M = 65536.0
_PLANE_DTYPES = (("n_hyp", torch.int32), ("chosen", torch.int32), ("kept", torch.int32), ("depth", torch.float32), ("std", torch.float32),
                 ("min", torch.float32), ("max", torch.float32), ("share", torch.float32), ("valid", torch.uint8),
                 ("center2", torch.int64), ("limit", torch.int64))


def _check_gap(gap_m) -> Tuple[float, int]:
    """``(gap_m, gap_q)``: the gap as a float and in units of 2^-16 m, ``llrint(gap_m * 65536)``."""
    if isinstance(gap_m, (bool, str)) or not isinstance(gap_m, (int, float, np.integer, np.floating)):
        raise TypeError(f"gap_m {gap_m!r}: a number of metres expected")
    gap_m = float(gap_m)
    if not (math.isfinite(gap_m) and 0.0 <= gap_m <= MAX_GAP_M):
        raise ValueError(f"gap_m {gap_m!r}: a finite number in 0 .. {MAX_GAP_M:g} expected")
    gap_q = int(np.rint(np.float64(gap_m) * np.float64(65536.0)))
    assert 0 <= gap_q <= rt.HYP_MAX_GAP_Q
    return gap_m, gap_q


def _check_rule(rule, guide, shape, device) -> Tuple[int, Optional[torch.Tensor]]:
    if rule not in rt.HYP_RULES:
        raise ValueError(f"rule={rule!r}: one of {rt.HYP_RULES} expected")
    if rule == "count":
        if guide is not None:
            raise ValueError('rule="count" takes no guide')
        return 0, None
    if guide is None:
        raise ValueError('rule="guide" needs a guide plane')
    if not isinstance(guide, torch.Tensor):
        raise TypeError("guide: a float32 device tensor expected")
    if guide.dtype != torch.float32:
        raise TypeError(f"guide: float32 expected, not {guide.dtype}")
    if guide.device != device:
        raise TypeError(f"guide is on {guide.device}, the soundings on {device}")
    if tuple(guide.shape) != tuple(shape):
        raise ValueError(f"guide of shape {tuple(guide.shape)}: the planes' shape {tuple(shape)} expected")
    return 1, guide.contiguous()


def build_hypotheses(robust, gap_m, rule="count", guide=None, min_count=None, records=True) -> Dict[str, object]:
    """``bgnn_hypotheses_build`` on the ``start`` / ``sorted_q`` of a robust result: the eleven planes in the shape of the result's
    own, the three record tensors (or ``None``) and the checked arguments.  ``ValueError`` / ``TypeError`` before anything is
    launched."""
    gap_m, gap_q = _check_gap(gap_m)
    shape = tuple(robust.count.shape)
    dev = robust.sorted_q.device
    code, guide = _check_rule(rule, guide, shape, dev)
    min_count = _check_min_count(robust.min_count if min_count is None else min_count)
    cells, capacity = int(robust.start.numel()) - 1, int(robust.sorted_q.numel())
    ctx = rt.get_context(dev)
    ws_bytes = int(ctx.lib.bgnn_hypotheses_workspace_bytes(cells, capacity))
    if ws_bytes == 0:
        raise ValueError(f"{cells} cells, capacity {capacity}: no workspace of that size")
    ws = torch.empty(ws_bytes // 8, dtype=torch.int64, device=dev)
    planes = {name: torch.empty(shape, dtype=dtype, device=dev) for name, dtype in _PLANE_DTYPES}
    recs = dict.fromkeys(HYPOTHESIS_RECORDS)
    if records:
        recs = {"hyp_start": torch.empty(cells + 1, dtype=torch.int32, device=dev),        # (uint32 bits)
                "hyp_first": torch.empty(capacity, dtype=torch.int32, device=dev),         # (uint32 bits)
                "hyp_count": torch.empty(capacity, dtype=torch.int32, device=dev)}
    _call(ctx, "bgnn_hypotheses_build", rt.ptr(robust.start), rt.ptr(robust.sorted_q), cells, capacity, gap_q, code, rt.ptr(guide),
          min_count, float(robust.nodata_value), rt.ptr(ws), ws_bytes, *(rt.ptr(planes[name]) for name in HYPOTHESIS_PLANES),
          *(rt.ptr(recs[name]) for name in HYPOTHESIS_RECORDS))       # (the workspace may go: the caller's stream waits)
    return dict(**planes, **recs, gap_m=gap_m, rule=rule, nodata_value=float(robust.nodata_value), min_count=min_count,
                sorted_q=robust.sorted_q, start=robust.start)


class _HypothesisPlanes:
    """What the uniform and the variable-resolution result share."""

    def _counts(self) -> torch.Tensor:
        start = self.start.to(torch.int64) & 0xFFFFFFFF
        return (start[1:] - start[:-1]).view(self.kept.shape)

    def density_plane(self) -> torch.Tensor:
        """``density_from_count(kept)``: the node plane "sounding_density" over the soundings of the chosen hypothesis."""
        return density_from_count(self.kept)

    def ambiguity_plane(self) -> torch.Tensor:
        """The share of a cell's soundings that lie outside the chosen hypothesis: float32 ``(n - kept) / n`` where ``n >= 1``,
        formed in float64 on the device and rounded once; 0 in an empty cell."""
        n = self._counts()
        hit = n >= 1
        d = torch.where(hit, n, torch.ones_like(n)).to(torch.float64)
        return torch.where(hit, ((n - self.kept.to(torch.int64)).to(torch.float64) / d).to(torch.float32),
                           torch.zeros(n.shape, dtype=torch.float32, device=n.device))

    def _hypotheses_of_cell(self, cell: int) -> List[Dict[str, object]]:
        if self.hyp_start is None:
            raise ValueError("hypotheses_of: the records were not kept (records=False)")
        lo, hi, b, e = (int(v) & 0xFFFFFFFF for v in torch.cat([self.hyp_start[cell:cell + 2], self.start[cell:cell + 2]]).tolist())
        host = torch.cat([self.hyp_first[lo:hi], self.hyp_count[lo:hi], self.sorted_q[b:e]]).tolist()
        k = hi - lo
        first, count, s = [v & 0xFFFFFFFF for v in host[:k]], host[k:2 * k], host[2 * k:]
        out = []
        for f, nh in zip(first, count):
            run = s[f - b:f - b + nh]                                        # Python integers from here
            m2 = run[(nh - 1) // 2] + run[nh // 2]
            out.append({"first": f, "count": nh, "min": run[0] / 65536, "max": run[-1] / 65536, "median": m2 / 131072,
                        "mean": sum(run) / (nh * 65536)})
        return out


@dataclasses.dataclass
class HypothesisGrid(_HypothesisPlanes):
    """What ``RobustSoundingGrid.hypotheses`` leaves on the device.  ``[H, W]`` planes: ``n_hyp`` (int32: the number of hypotheses,
    true also where the cell is not valid), ``chosen`` (int32: the index of the chosen one in ascending depth, -1 where none has
    ``min_count`` soundings), ``kept`` (int32: its soundings), ``depth``, ``std``, ``min``, ``max`` (float32: the mean, the
    standard deviation and the ends of the chosen run), ``share`` (float32: ``kept / count``), ``valid`` (uint8), ``center2`` and
    ``limit`` (int64: the rule ``flag`` applies, ``limit == -1`` where none is chosen); the float planes hold ``nodata_value``
    where not valid.  The records, or ``None``: the hypotheses of cell ``c`` are entries ``hyp_start[c] .. hyp_start[c + 1]`` of
    ``hyp_first`` (the index into ``sorted_q`` of each one's first sounding) and ``hyp_count`` (uint32 bits in int32 tensors, as
    ``start``).  ``sorted_q`` and ``start`` are those of the robust result, by reference.  ``guide`` and ``support``: ``None`` but
    under ``rule="locale"``, where they are the ``[H, W]`` planes of ``data.locale_guide`` the result was chosen by."""
    n_hyp: torch.Tensor
    chosen: torch.Tensor
    kept: torch.Tensor
    depth: torch.Tensor
    std: torch.Tensor
    min: torch.Tensor
    max: torch.Tensor
    share: torch.Tensor
    valid: torch.Tensor
    center2: torch.Tensor
    limit: torch.Tensor
    hyp_start: Optional[torch.Tensor]
    hyp_first: Optional[torch.Tensor]
    hyp_count: Optional[torch.Tensor]
    sorted_q: torch.Tensor
    start: torch.Tensor
    gap_m: float
    rule: str
    transform: Tuple[float, float, float, float, float, float]
    resolution: Tuple[float, float]
    nodata_value: float = 1.0e6
    min_count: int = 1
    guide: Optional[torch.Tensor] = None               # rule="locale": the float32 guide the result was built with (NaN: by count)
    support: Optional[torch.Tensor] = None             # rule="locale": int32, the witnesses in each cell's window

    def hypotheses_of(self, row: int, col: int) -> List[Dict[str, object]]:
        """The hypotheses of one cell in ascending depth, a host list of dicts: ``first`` (index into ``sorted_q``), ``count``,
        and ``min``, ``max``, ``median``, ``mean`` in metres (float64 from the exact integers).  Two small copies to the host.
        ``ValueError`` where the records were not kept."""
        height, width = (int(v) for v in self.kept.shape)
        if not (0 <= row < height and 0 <= col < width):
            raise IndexError(f"cell ({row}, {col}) of a {height} x {width} grid")
        return self._hypotheses_of_cell(row * width + col)

    def survey_tensors(self, depth: str = "depth", uncertainty: str = "std", density: bool = False):
        """``(depth_t, valid_t, unc_t)`` as ``BathymetricPipeline.process_survey_device`` takes them; ``density=True``:
        ``density_plane()`` as a fourth element."""
        t = (_pick_plane(self, depth, HYPOTHESIS_DEPTH_PLANES, "depth"), self.valid,
             _pick_plane(self, uncertainty, HYPOTHESIS_UNCERTAINTY_PLANES, "uncertainty"))
        return t + (self.density_plane(),) if density else t

    def to_grid(self, depth: str = "depth", uncertainty: str = "std") -> BathymetricGrid:
        """A host ``BathymetricGrid`` of the chosen surface and uncertainty, as ``RobustSoundingGrid.to_grid``."""
        height, width = (int(v) for v in self.kept.shape)
        x0, res, _, y0, _, _ = self.transform
        depth_t, _, unc_t = self.survey_tensors(depth, uncertainty)
        return BathymetricGrid(depth=depth_t.cpu().numpy(), uncertainty=unc_t.cpu().numpy(), nodata_value=self.nodata_value,
                               transform=self.transform, resolution=self.resolution,
                               bounds=(x0, y0 - height * res, x0 + width * res, y0), density=self.density_plane().cpu().numpy())


@dataclasses.dataclass
class VRHypothesisGrid(_HypothesisPlanes, _VRPlanes):
    """What ``RobustVRSoundingGrid.hypotheses`` leaves on the device: the planes and records of ``HypothesisGrid`` as flat
    ``[total]`` tensors, one entry per record of ``layout``."""
    n_hyp: torch.Tensor
    chosen: torch.Tensor
    kept: torch.Tensor
    depth: torch.Tensor
    std: torch.Tensor
    min: torch.Tensor
    max: torch.Tensor
    share: torch.Tensor
    valid: torch.Tensor
    center2: torch.Tensor
    limit: torch.Tensor
    hyp_start: Optional[torch.Tensor]
    hyp_first: Optional[torch.Tensor]
    hyp_count: Optional[torch.Tensor]
    sorted_q: torch.Tensor
    start: torch.Tensor
    gap_m: float
    rule: str
    layout: VRLayout
    nodata_value: float = 1.0e6
    min_count: int = 1

    def hypotheses_of(self, record: int) -> List[Dict[str, object]]:
        """As ``HypothesisGrid.hypotheses_of``, for one record of the layout."""
        if not 0 <= record < int(self.kept.shape[0]):
            raise IndexError(f"record {record} of {int(self.kept.shape[0])}")
        return self._hypotheses_of_cell(int(record))

    def records(self, depth: str = "depth", uncertainty: str = "std") -> torch.Tensor:
        """The ``[total, 2]`` float32 device tensor of (depth, depth_uncrt) records, 1.0e6 in both where the record is not valid."""
        return self._records(_pick_plane(self, depth, HYPOTHESIS_DEPTH_PLANES, "depth"),
                             _pick_plane(self, uncertainty, HYPOTHESIS_UNCERTAINTY_PLANES, "uncertainty"))

    def handler(self, depth: str = "depth", uncertainty: str = "std") -> VRBagHandler:
        """As ``VRSoundingGrid.handler``: what ``compute_ground_truth_native`` and ``process_refinements`` take."""
        return self._handler(self.records(depth, uncertainty))


def hypotheses_of_grid(robust, gap_m, rule="count", guide=None, min_count=None, records=True, radius=None,
                       min_support=None) -> HypothesisGrid:
    """``RobustSoundingGrid.hypotheses``."""
    if rule == "locale":
        if guide is not None:
            raise ValueError('rule="locale" makes its own guide: it takes none')
        from .locale_guide import hypotheses_by_locale
        return hypotheses_by_locale(robust, gap_m, radius, min_support, min_count, records)
    if radius is not None or min_support is not None:
        raise ValueError(f'radius and min_support go with rule="locale", not with rule={rule!r}')
    out = build_hypotheses(robust, gap_m, rule, guide, min_count, records)
    return HypothesisGrid(**out, transform=robust.transform, resolution=robust.resolution)


def hypotheses_of_records(robust, gap_m, rule="count", guide=None, min_count=None, records=True) -> VRHypothesisGrid:
    """``RobustVRSoundingGrid.hypotheses``."""
    if rule == "locale":
        raise ValueError('rule="locale" is for uniform grids: the neighbours of a record across refinement grids are not defined')
    out = build_hypotheses(robust, gap_m, rule, guide, min_count, records)
    return VRHypothesisGrid(**out, layout=robust.layout)
