"""Guide planes for ``rule="guide"`` of the depth hypotheses (data/sounding_hypotheses.py), and the locale rule on top of them.

The count rule sees one cell at a time: where a fish school of 40 soundings hangs over 25 of the seabed it takes the school, in
every cell the school covers.  CUBE's third disambiguation rule asks the neighbourhood instead.  A cell is a *witness* where it
has exactly one hypothesis and that one was chosen; its value is the cell's median.  ``locale_guide`` (include/bgnn_locale.h)
gives every cell the median of the witnesses within ``radius`` cells of it, the cell itself left out, as a float32 guide, and
their number as ``support``; with fewer than ``min_support`` witnesses the guide is NaN, which the guide rule reads as "by
count".  ``RobustSoundingGrid.hypotheses(gap_m, rule="locale")`` runs the three steps: a count build, the guide, a guide build.
All in integers on the device, one rounding per cell: equal bits on every run and for every order of the cloud.

``guide_from_coarser`` is the other usual guide, a coarser gridding of the same cloud brought to this resolution, as a checked
helper in plain torch.

Out of scope: iterating the rule so that resolved cells become witnesses, variable-resolution layouts (neighbours across
refinement grids), and the streamed and sharded routes."""
from __future__ import annotations

import numpy as np
import torch

from .. import runtime as rt
from .sounding_grid import _call
from .sounding_hypotheses import HYPOTHESIS_DEPTH_PLANES, HypothesisGrid, build_hypotheses
from .sounding_robust import ROBUST_DEPTH_PLANES, RobustSoundingGrid

DEFAULT_RADIUS = 2
DEFAULT_MIN_SUPPORT = 3


def _check_window(radius, min_support):
    for name, v in (("radius", radius), ("min_support", min_support)):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)):
            raise TypeError(f"{name} {v!r}: an integer expected")
    radius, min_support = int(radius), int(min_support)
    if not 1 <= radius <= rt.LOCALE_MAX_RADIUS:
        raise ValueError(f"radius {radius}: 1 .. {rt.LOCALE_MAX_RADIUS} expected")
    window = (2 * radius + 1) ** 2 - 1
    if not 1 <= min_support <= window:
        raise ValueError(f"min_support {min_support}: 1 .. {window} expected at radius {radius}")
    return radius, min_support


def locale_guide_planes(n_hyp, chosen, center2, radius=DEFAULT_RADIUS, min_support=DEFAULT_MIN_SUPPORT):
    """``bgnn_locale_guide`` on raw device planes: ``n_hyp`` and ``chosen`` (int32) of a hypotheses result and ``center2`` (int64)
    of the robust result under it, all contiguous ``[H, W]`` on one GPU.  ``(guide, support)``: float32 and int32 ``[H, W]``.
    ``TypeError`` / ``ValueError`` before anything is launched."""
    planes = (("n_hyp", n_hyp, torch.int32), ("chosen", chosen, torch.int32), ("center2", center2, torch.int64))
    for name, t, dtype in planes:
        if not isinstance(t, torch.Tensor):
            raise TypeError(f"{name}: a device tensor expected")
        if t.dtype != dtype:
            raise TypeError(f"{name}: {dtype} expected, not {t.dtype}")
    dev, shape = n_hyp.device, tuple(n_hyp.shape)
    if dev.type != "cuda":
        raise TypeError(f"n_hyp is on {dev}: a GPU tensor expected")
    if len(shape) != 2 or shape[0] < 1 or shape[1] < 1:
        raise ValueError(f"n_hyp of shape {shape}: a plane [H, W] of at least 1 x 1 expected")
    if shape[0] * shape[1] > rt.LOCALE_MAX_CELLS:
        raise ValueError(f"shape {shape}: more than {rt.LOCALE_MAX_CELLS} cells")
    for name, t, _ in planes:
        if t.device != dev:
            raise TypeError(f"{name} is on {t.device}, n_hyp on {dev}")
        if tuple(t.shape) != shape:
            raise ValueError(f"{name} of shape {tuple(t.shape)}: the shape {shape} of n_hyp expected")
        if not t.is_contiguous():
            raise ValueError(f"{name} is not contiguous")
    radius, min_support = _check_window(radius, min_support)
    guide = torch.empty(shape, dtype=torch.float32, device=dev)
    support = torch.empty(shape, dtype=torch.int32, device=dev)
    _call(rt.get_context(dev), "bgnn_locale_guide", rt.ptr(n_hyp), rt.ptr(chosen), rt.ptr(center2), shape[0], shape[1], radius,
          min_support, rt.ptr(guide), rt.ptr(support))
    return guide, support


def locale_guide(robust, hyp=None, radius=DEFAULT_RADIUS, min_support=DEFAULT_MIN_SUPPORT, gap_m=None):
    """``(guide, support)`` for the cells of ``robust`` (a ``RobustSoundingGrid``): the witnesses are read off ``hyp``, a
    ``HypothesisGrid`` of the same shape and device built under any rule; with ``hyp=None`` one is built by count, without
    records, at ``gap_m`` (required then, refused otherwise).  The witness values are ``robust.center2``, twice the cell medians."""
    if not isinstance(robust, RobustSoundingGrid):
        raise TypeError("locale_guide: a RobustSoundingGrid expected (the locale rule is for uniform grids)")
    _check_window(radius, min_support)
    if hyp is None:
        if gap_m is None:
            raise ValueError("locale_guide: without hyp= it needs gap_m= to build the hypotheses by count")
        hyp = robust.hypotheses(gap_m, records=False)
    else:
        if gap_m is not None:
            raise ValueError("locale_guide: gap_m= goes with hyp=None only")
        if not isinstance(hyp, HypothesisGrid):
            raise TypeError("locale_guide: hyp: a HypothesisGrid expected")
        if tuple(hyp.n_hyp.shape) != tuple(robust.center2.shape):
            raise ValueError(f"hyp of shape {tuple(hyp.n_hyp.shape)}: the robust grid's shape {tuple(robust.center2.shape)} expected")
        if hyp.n_hyp.device != robust.center2.device:
            raise TypeError(f"hyp is on {hyp.n_hyp.device}, the robust grid on {robust.center2.device}")
    return locale_guide_planes(hyp.n_hyp, hyp.chosen, robust.center2, radius, min_support)


def hypotheses_by_locale(robust, gap_m, radius=None, min_support=None, min_count=None, records=True) -> HypothesisGrid:
    """``RobustSoundingGrid.hypotheses(rule="locale")``: a count build without records, the locale guide, a guide build.  The
    result carries ``rule="locale"``, the ``guide`` it was built with and its ``support``."""
    radius, min_support = _check_window(DEFAULT_RADIUS if radius is None else radius,
                                        DEFAULT_MIN_SUPPORT if min_support is None else min_support)
    by_count = HypothesisGrid(**build_hypotheses(robust, gap_m, "count", None, min_count, False), transform=robust.transform,
                              resolution=robust.resolution)
    guide, support = locale_guide(robust, by_count, radius, min_support)
    out = build_hypotheses(robust, gap_m, "guide", guide, min_count, records)
    out["rule"] = "locale"
    return HypothesisGrid(**out, transform=robust.transform, resolution=robust.resolution, guide=guide, support=support)


def _geometry(grid, what):
    if not isinstance(grid, (RobustSoundingGrid, HypothesisGrid)):
        raise TypeError(f"{what}: a RobustSoundingGrid or a HypothesisGrid expected")
    return tuple(int(v) for v in grid.valid.shape), (float(grid.transform[0]), float(grid.transform[3])), float(grid.resolution[0])


def guide_from_coarser(coarse, like, plane="median") -> torch.Tensor:
    """A guide for ``like`` from a coarser gridding of the same cloud: ``plane`` of ``coarse`` (``"median"``, ``"kept_mean"``,
    ``"kept_min"`` or ``"kept_max"`` of a ``RobustSoundingGrid``; ``"depth"``, ``"min"`` or ``"max"`` of a ``HypothesisGrid``),
    NaN where ``coarse.valid == 0``, every cell repeated ``f`` times on both axes and cropped to ``like``'s shape.  ``f`` is the
    ratio of the two resolutions.  ``ValueError`` where it is not a whole number, where the two origins differ or where ``coarse``
    does not cover ``like``.  Plain torch on the tensors' device."""
    (ch, cw), c_origin, c_res = _geometry(coarse, "coarse")
    (lh, lw), l_origin, l_res = _geometry(like, "like")
    allowed = ROBUST_DEPTH_PLANES if isinstance(coarse, RobustSoundingGrid) else HYPOTHESIS_DEPTH_PLANES
    if plane not in allowed:
        raise ValueError(f"plane={plane!r}: one of {allowed} expected")
    ratio = c_res / l_res
    f = int(round(ratio))
    if f < 1 or abs(ratio - f) > 1e-9 * max(f, 1):
        raise ValueError(f"resolutions {c_res:g} and {l_res:g}: the coarse one is not a whole multiple of the other")
    if c_origin != l_origin:
        raise ValueError(f"origins {c_origin} and {l_origin} differ")
    if ch * f < lh or cw * f < lw:
        raise ValueError(f"coverage: {ch} x {cw} cells times {f} do not cover {lh} x {lw}")
    values = getattr(coarse, plane)
    values = torch.where(coarse.valid != 0, values, torch.full((), float("nan"), dtype=values.dtype, device=values.device))
    rows, cols = -(-lh // f), -(-lw // f)
    return values[:rows, :cols].repeat_interleave(f, dim=0).repeat_interleave(f, dim=1)[:lh, :lw].contiguous()
