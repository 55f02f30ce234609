"""``TileStore`` -- the tiles of a training set resident in HBM, and what fills and reads it: the reference's tile planning
(``plan_ground_truth_tiles``, ``plan_tile_boxes``, ``keep_ground_truth_boxes``), the bindings of include/bgnn_tilestore.h
(``scan_tile_boxes``, ``cut_tile_boxes``) the device constructors are assembled from, the gather of a batch under the eight
symmetries of the square (``dihedral_ops``, ``TileStore.gather`` over ``bgnn_tile_gather``, include/bgnn_augment.h) and the
per-node targets of a batch (``training_targets_fused`` over ``bgnn_training_targets``).  ``trainer.py`` holds the loop over it."""
from __future__ import annotations

import ctypes as C
import logging
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from .. import runtime as rt

logger = logging.getLogger(__name__)


def plan_ground_truth_tiles(labels: np.ndarray, tile_size: int = 512, overlap: int = 64,
                            min_valid_ratio: float = 0.1) -> Tuple[List[Tuple[int, int, int, int]], Dict[int, int]]:
    """The reference's scan of a ground-truth label band (``GroundTruthDataset._scan_ground_truth``, trainer.py:133-171), host
    only: ``(row_start, col_start, row_end, col_end)`` of every full tile on the stride grid whose share of labelled cells
    (``label >= 0``) reaches ``min_valid_ratio``, then the scan's single far-corner edge tile when the raster is larger than a tile
    both ways and either extent is no multiple of the stride, and the class counts 0 / 1 / 2 over the labelled cells of the
    tiles that were kept (overlaps counted as often as they are cut)."""
    labels = np.asarray(labels)
    if labels.ndim != 2:
        raise ValueError(f"labels must be a 2-D grid, got shape {labels.shape}")
    boxes: List[Tuple[int, int, int, int]] = []
    counts = {0: 0, 1: 0, 2: 0}
    for r0, c0, r1, c1 in plan_tile_boxes(*labels.shape, tile_size, overlap):
        t = labels[r0:r1, c0:c1]
        valid = t >= 0
        if np.sum(valid) / valid.size >= min_valid_ratio:
            boxes.append((r0, c0, r1, c1))
            for c in (0, 1, 2):
                counts[c] += int(np.sum(t[valid] == c))
    return boxes, counts


def plan_tile_boxes(height: int, width: int, tile_size: int = 512, overlap: int = 64) -> List[Tuple[int, int, int, int]]:
    """The candidate boxes of ``plan_ground_truth_tiles`` on a ``height x width`` raster BEFORE its validity test, in the
    reference's order: the stride grid of full tiles, row-major, then the single far-corner tile when the raster is larger than a
    tile both ways and either extent is no multiple of the stride.  A raster smaller than a tile in either extent yields no box.
    Pure host arithmetic: the boxes ``scan_tile_boxes`` counts on the device."""
    height, width, tile_size = int(height), int(width), int(tile_size)
    stride = tile_size - int(overlap)
    if stride <= 0:
        raise ValueError("Tile size must be larger than overlap")
    boxes = [(r0, c0, r0 + tile_size, c0 + tile_size)
             for r0 in range(0, height - tile_size + 1, stride) for c0 in range(0, width - tile_size + 1, stride)]
    if height > tile_size and width > tile_size and (height % stride != 0 or width % stride != 0):
        boxes.append((height - tile_size, width - tile_size, height, width))
    return boxes


def _kept_rows(boxes, counts, min_valid_ratio: float) -> List[int]:
    """The rows ``i`` of a scan whose box stays: ``valid / (h * w) >= min_valid_ratio`` -- the float64 quotient
    ``np.sum(valid) / valid.size`` forms, so no tolerance is involved."""
    return [i for i, ((r0, c0, r1, c1), row) in enumerate(zip(boxes, counts))
            if int(row[0]) / ((r1 - r0) * (c1 - c0)) >= min_valid_ratio]


def keep_ground_truth_boxes(boxes, counts, min_valid_ratio: float = 0.1):
    """The keep rule of ``plan_ground_truth_tiles`` on scanned counts (``_kept_rows``).  ``counts``: ``[n, 4]`` integers (valid,
    class 0, class 1, class 2) per box.  Returns the kept boxes and the class counts summed over them (overlaps counted as often
    as they are cut)."""
    rows = _kept_rows(boxes, counts, min_valid_ratio)
    return [tuple(boxes[i]) for i in rows], {c: sum(int(counts[i][1 + c]) for i in rows) for c in (0, 1, 2)}


def _box_table(boxes, dst=None) -> np.ndarray:
    """``(r0, c0, r1, c1)`` boxes as the ``bgnn_tile_box`` table; ``dst``: the cell offset of every tile (default 0)."""
    table = np.zeros(len(boxes), dtype=rt.TILE_BOX_DTYPE)
    if len(boxes):
        b = np.asarray(boxes, dtype=np.int64).reshape(-1, 4)
        table["row0"], table["col0"] = b[:, 0], b[:, 1]
        extent = np.stack([b[:, 2] - b[:, 0], b[:, 3] - b[:, 1]], axis=1)
        if (np.abs(extent) > np.iinfo(np.int32).max).any():
            raise ValueError("a tile extent beyond int32")
        table["h"], table["w"] = extent[:, 0], extent[:, 1]          # (an empty or inverted box stays <= 0: the library refuses it)
        if dst is not None:
            table["dst"] = np.asarray(dst, dtype=np.int64)
    return table


def _tile_offsets(hw: np.ndarray) -> np.ndarray:
    """The first cell of every tile of an ``[n, 2]`` extent table in a flat store, and the store's size last: int64 ``[n + 1]``."""
    return np.concatenate([[0], np.cumsum(hw[:, 0].astype(np.int64) * hw[:, 1])]).astype(np.int64)


def _workspace(ws_bytes: int, device) -> torch.Tensor:
    """The 8-byte-aligned device workspace of a ``*_workspace_bytes`` result."""
    return torch.empty(int(ws_bytes) // 8, dtype=torch.int64, device=device)


def _pointers(tensors):
    """The ``void *`` array of a list of tensors, NULL for None."""
    return (C.c_void_p * len(tensors))(*[None if t is None else t.data_ptr() for t in tensors])


def _tile_plane(t: torch.Tensor, name: str) -> torch.Tensor:
    if not isinstance(t, torch.Tensor) or t.dim() != 2 or t.dtype not in (torch.int32, torch.float32) or not t.is_cuda or \
            not t.is_contiguous():
        raise TypeError(f"{name} must be a contiguous [H, W] int32 or float32 tensor on the GPU")
    return t


def scan_tile_boxes(plane: torch.Tensor, boxes, nodata: Optional[float] = None, ctx=None) -> torch.Tensor:
    """``bgnn_tile_scan`` (include/bgnn_tilestore.h): the ``[n, 4]`` int64 device table of counts (valid, class 0, class 1,
    class 2) of the ``(r0, c0, r1, c1)`` boxes of an ``[H, W]`` device plane.  An int32 plane is scanned as labels (valid: ``>= 0``),
    a float32 plane as depths (valid: finite and ``!= nodata``; ``nodata`` None or NaN: finite only; class counts 0).  Asynchronous
    on the context's stream, ordered against the caller's current stream; the caller's ``.cpu()`` is the synchronisation."""
    plane = _tile_plane(plane, "plane")
    dev = plane.device
    ctx = ctx if ctx is not None else rt.get_context(dev)
    table = _box_table(boxes)
    n = len(table)
    counts = torch.empty((n, rt.TILE_COUNTS), dtype=torch.int64, device=dev)
    if n == 0:
        return counts
    ws_bytes = int(ctx.lib.bgnn_tile_workspace_bytes(n))
    ws = _workspace(ws_bytes, dev)
    mode = rt.TILE_VALID_LABEL if plane.dtype == torch.int32 else rt.TILE_VALID_DEPTH
    ctx.begin()
    rt.check(ctx.lib.bgnn_tile_scan(ctx.handle, rt.ptr(plane), int(plane.shape[0]), int(plane.shape[1]), mode,
                                    float("nan") if nodata is None else float(nodata), C.c_void_p(table.ctypes.data), n, rt.ptr(ws),
                                    C.c_size_t(ws_bytes), rt.ptr(counts)))
    ctx.end()
    return counts


def cut_tile_boxes(planes: Sequence[Optional[torch.Tensor]], stores: Sequence[Optional[torch.Tensor]], boxes, offsets,
                   mask: Optional[torch.Tensor] = None, mask_plane: int = 0, nodata: Optional[float] = None, ctx=None) -> None:
    """``bgnn_tile_cut``: the ``(r0, c0, r1, c1)`` boxes of up to four ``[H, W]`` device planes of one shape, written row-major into
    the flat ``stores`` (one per plane, same dtype, ``None`` beside a ``None`` plane) from cell ``offsets[i]`` on, and into ``mask``
    (uint8) the validity of ``planes[mask_plane]`` under the predicate of its dtype (see ``scan_tile_boxes``).  One launch."""
    given = [p for p in planes if p is not None]
    if not given or len(planes) != len(stores) or len(planes) > rt.TILE_MAX_PLANES:
        raise ValueError(f"1 to {rt.TILE_MAX_PLANES} planes, a store for each")
    dev, shape = given[0].device, tuple(given[0].shape)
    cells = None
    for i, (p, s) in enumerate(zip(planes, stores)):
        if (p is None) != (s is None):
            raise ValueError(f"plane {i} and its store: both or neither")
        if p is None:
            continue
        _tile_plane(p, f"plane {i}")
        if tuple(p.shape) != shape or p.device != dev:
            raise ValueError(f"plane {i} has shape {tuple(p.shape)} on {p.device}, plane 0 {shape} on {dev}")
        if not isinstance(s, torch.Tensor) or s.dtype != p.dtype or s.device != dev or not s.is_contiguous():
            raise TypeError(f"store {i} must be a contiguous {p.dtype} tensor on {dev}")
        cells = s.numel() if cells is None else cells
        if s.numel() != cells:
            raise ValueError("the stores disagree on the number of cells")
    mode = rt.TILE_VALID_LABEL
    if mask is not None:
        if mask.dtype != torch.uint8 or mask.device != dev or not mask.is_contiguous() or mask.numel() != cells:
            raise TypeError(f"mask must be a contiguous uint8 tensor of {cells} cells on {dev}")
        if not 0 <= mask_plane < len(planes) or planes[mask_plane] is None:
            raise ValueError(f"mask_plane {mask_plane} names no given plane")
        mode = rt.TILE_VALID_LABEL if planes[mask_plane].dtype == torch.int32 else rt.TILE_VALID_DEPTH
    table = _box_table(boxes, offsets)
    n = len(table)
    if n == 0:
        return
    ctx = ctx if ctx is not None else rt.get_context(dev)
    ws_bytes = int(ctx.lib.bgnn_tile_workspace_bytes(n))
    ws = _workspace(ws_bytes, dev)
    ctx.begin()
    rt.check(ctx.lib.bgnn_tile_cut(ctx.handle, _pointers(planes), _pointers(stores), len(planes), shape[0], shape[1], rt.ptr(mask),
                                   int(mask_plane), mode, float("nan") if nodata is None else float(nodata),
                                   C.c_void_p(table.ctypes.data), n, int(cells), rt.ptr(ws), C.c_size_t(ws_bytes)))
    ctx.end()


def _cut_store(sources, mask_plane: int = 0, nodata: Optional[float] = None, ctx=None):
    """A store assembled on the device from ``sources``, in store order: ``(planes, boxes)`` per source -- up to
    ``rt.TILE_MAX_PLANES`` ``[H, W]`` planes of that source (``None`` at the same places in every source) and its kept
    ``(r0, c0, r1, c1)`` boxes.  One flat store per plane (of its dtype) and the uint8 mask are allocated once for all sources,
    and every source that has boxes gets one ``cut_tile_boxes`` at its running offset.  Returns ``(hw, stores, mask)``: the boxes'
    extents (int32 ``[n, 2]``), the flat stores in the order of the planes, and the validity of plane ``mask_plane``."""
    boxes = np.concatenate([np.asarray(b, dtype=np.int64).reshape(-1, 4) for _, b in sources])
    hw = np.stack([boxes[:, 2] - boxes[:, 0], boxes[:, 3] - boxes[:, 1]], axis=1)
    offsets = _tile_offsets(hw)
    cells, first = int(offsets[-1]), sources[0][0]
    dev = next(p for p in first if p is not None).device
    stores = [None if p is None else torch.empty(cells, dtype=p.dtype, device=dev) for p in first]
    mask = torch.empty(cells, dtype=torch.uint8, device=dev)
    at = 0
    for planes, b in sources:
        if len(b):
            cut_tile_boxes(planes, stores, b, offsets[at:at + len(b)], mask=mask, mask_plane=mask_plane, nodata=nodata, ctx=ctx)
        at += len(b)
    return hw.astype(np.int32), stores, mask


def _plane_to_device(plane, dtype: torch.dtype, device) -> torch.Tensor:
    """A host array (uploaded once) or a tensor as a contiguous ``dtype`` tensor on ``device``."""
    if isinstance(plane, torch.Tensor):
        return plane.to(device=device, dtype=dtype).contiguous()
    npdt = np.int32 if dtype == torch.int32 else np.float32
    return torch.from_numpy(np.ascontiguousarray(np.asarray(plane).astype(npdt, copy=False))).to(device)


def dihedral_ops(n: int, rotations: bool, flips: bool, rng: np.random.Generator) -> np.ndarray:
    """``n`` ops of include/bgnn_augment.h (``op = k + 4 * f``: ``np.rot90(np.fliplr(t) if f else t, k)``) as int8, drawn from
    ``rng`` as the two flags of the training settings ask:

    both        ``k = rng.integers(0, 4, n)``, ``f = rng.integers(0, 2, n)``: uniform over the eight symmetries of the square
    rotations   ``op = k``
    flips       ``fh = rng.integers(0, 2, n)``, ``fv = rng.integers(0, 2, n)``, a horizontal and a vertical mirror drawn
                independently: ``fh`` alone is op 4 (``fliplr``), ``fv`` alone op 6 (``flipud``), both op 2 (their product, the
                turn by 180 degrees), neither op 0
    neither     all zeros; nothing is drawn from ``rng``"""
    n = int(n)
    if rotations and flips:
        k = rng.integers(0, 4, n)
        f = rng.integers(0, 2, n)
        return (k + 4 * f).astype(np.int8)
    if rotations:
        return rng.integers(0, 4, n).astype(np.int8)
    if flips:
        fh = rng.integers(0, 2, n)
        fv = rng.integers(0, 2, n)
        return np.array([0, 4, 6, 2], np.int8)[fh + 2 * fv]
    return np.zeros(n, np.int8)


def _ops_array(ops, n: int) -> np.ndarray:
    ops = np.asarray(ops).reshape(-1)
    if ops.size != n or (ops.size and not np.issubdtype(ops.dtype, np.integer)):
        raise ValueError(f"ops must hold one integer op per tile ({n}), got {ops.size} of dtype {ops.dtype}")
    ops = ops.astype(np.int32)
    if ops.size and (ops.min() < 0 or ops.max() >= rt.AUG_OPS):
        raise ValueError(f"ops {ops.tolist()} outside 0 .. {rt.AUG_OPS - 1}")
    return ops


def transformed_tile_table(hw, res, ops) -> Tuple[np.ndarray, np.ndarray]:
    """``hw`` (int32 ``[n, 2]``) and ``res`` (float64 ``[n, 2]``) of a batch after ``ops``: an op with odd ``k`` (``op & 1``)
    swaps the tile's extent and its resolution pair, every other op leaves both."""
    hw = np.ascontiguousarray(hw, np.int32).reshape(-1, 2)
    res = np.ascontiguousarray(res, np.float64).reshape(-1, 2)
    if len(hw) != len(res):
        raise ValueError("hw and res disagree on the number of tiles")
    odd = (_ops_array(ops, len(hw)) & 1).astype(bool)
    return (np.ascontiguousarray(np.where(odd[:, None], hw[:, ::-1], hw)),
            np.ascontiguousarray(np.where(odd[:, None], res[:, ::-1], res)))


class TileStore:
    """The tiles of a training set, flat in HBM with the ``hw`` / ``res`` tables ``GraphBuilder.build_from_device`` takes: the
    device-resident form of the reference's ``BathymetricGraphDataset(cache_tiles=True)`` (clean tiles, noise added per sample)
    and of its ``GroundTruthDataset`` (label / difference / noisy-depth planes).  ``batch`` turns a list of tile indices into the
    batch's graph and the target dict of ``BathymetricGNNLoss``, without leaving the device.  ``from_ground_truths``,
    ``from_survey`` and ``from_refinement_pairs`` build the store from planes that already lie in HBM (include/bgnn_tilestore.h:
    a scan of the candidate boxes, a gather of the kept ones, ``_cut_store``); the other constructors plan on the host.

    ``node_counts`` (host int64, one per tile): the valid cells of every tile, which are its graph's nodes.  Every constructor
    fills it from counts it has on the host anyway (the masks of ``from_tiles``, the scan counts, a truth's ``grid_counts``); a
    store assembled by hand may leave it None.  ``Trainer`` plans its steps with it (``step_plan``)."""

    def __init__(self, kind: str, hw, res, depth, mask, unc=None, labels=None, difference=None, class_counts=None,
                 graph_builder=None, noise_generator=None, augment: bool = True, seed: int = 0, device=None, node_counts=None,
                 density=None):
        from ..data import GraphBuilder, NoiseAugmentor, SyntheticNoiseGenerator
        assert kind in ("synthetic", "ground_truth")
        self.kind = kind
        self.device = rt.resolve_device(device)
        self.hw = np.ascontiguousarray(hw, np.int32).reshape(-1, 2)
        self.res = np.ascontiguousarray(res, np.float64).reshape(-1, 2)
        self.offsets = _tile_offsets(self.hw)
        self.depth, self.mask, self.unc, self.labels, self.difference = depth, mask, unc, labels, difference
        # per-cell sounding density (SoundingGrid.density_plane), float32, or None: one more node-feature column behind the others,
        # taken as it is (the synthetic noise leaves it untouched)
        self.density = density
        for t in (depth, mask, unc, labels, difference, density):
            if t is not None and t.numel() != int(self.offsets[-1]):
                raise ValueError("tile table and planes disagree on the number of cells")
        self.uniform = len(self.hw) > 0 and bool((self.hw == self.hw[0]).all())
        # the valid cells (= graph nodes) of every tile, on the host: what the constructors counted anyway (None: not known)
        self.node_counts = None if node_counts is None else np.ascontiguousarray(node_counts, np.int64).reshape(-1)
        if self.node_counts is not None and len(self.node_counts) != len(self.hw):
            raise ValueError("tile table and node counts disagree on the number of tiles")
        self.seed = int(seed)
        self.graph_builder = graph_builder if graph_builder is not None else GraphBuilder(device=self.device)
        self.augment = bool(augment)
        self.noise_generator = self.noise_augmentor = None
        if kind == "synthetic":
            self.noise_generator = noise_generator if noise_generator is not None else SyntheticNoiseGenerator(seed=self.seed)
            self.noise_generator.device = self.device
            self.noise_augmentor = NoiseAugmentor(self.noise_generator, seed=self.seed) if augment else None
        else:
            self._class_counts = dict(class_counts or {0: 0, 1: 0, 2: 0})

    # ---- constructors --------------------------------------------------------------------------------------------------
    @classmethod
    def from_tiles(cls, depths, valid_masks=None, uncertainties=None, resolutions=None, device=None, densities=None,
                   **kw) -> "TileStore":
        """Clean tiles (host arrays) for synthetic noise.  ``valid_masks[i]`` None: ``isfinite(depth)``; ``uncertainties``: for
        every tile or for none, and so ``densities`` (the tiles' sounding density); ``resolutions``: one ``(x, y)`` per tile
        (default 1.0).  Keywords: ``graph_builder``,
        ``noise_generator``, ``augment`` (True: ``NoiseAugmentor`` with a drawn intensity per sample), ``seed``."""
        from ..data import GraphBuilder
        device = rt.resolve_device(device)
        gb = kw.get("graph_builder") or GraphBuilder(device=device)
        kw["graph_builder"] = gb
        n = len(depths)
        if n == 0:
            raise ValueError("a TileStore needs at least one tile")
        resolutions = [(1.0, 1.0)] * n if resolutions is None else list(resolutions)
        a = gb.upload_density(None if densities is None else list(densities), list(depths))
        hw, res, d, m, u = gb.upload_tiles(list(depths), None if valid_masks is None else list(valid_masks), uncertainties, resolutions)
        masks = [None] * n if valid_masks is None else list(valid_masks)
        nodes = [int(np.count_nonzero(np.isfinite(np.asarray(t, dtype=np.float32)) if v is None else np.asarray(v, dtype=bool)))
                 for t, v in zip(depths, masks)]                               # (the masks upload_tiles stores)
        return cls("synthetic", hw, res, d.to(device), m.to(device), None if u is None else u.to(device), device=device,
                   node_counts=nodes, density=a[0].to(device) if a else None, **kw)

    @classmethod
    def from_grid(cls, grid, tile_manager, device=None, **kw) -> "TileStore":
        """The tiles ``tile_manager.iterate_tiles(grid, skip_empty=True)`` yields (trainer.py:351), at the grid's resolution."""
        tiles = list(tile_manager.iterate_tiles(grid, skip_empty=True))
        unc = [t.uncertainty for t in tiles] if tiles and tiles[0].uncertainty is not None else None
        den = getattr(grid, "density", None)                   # (BathymetricGrid.density: the tiles' windows of it)
        den = None if den is None else [np.asarray(den)[t.row_start:t.row_end, t.col_start:t.col_end] for t in tiles]
        return cls.from_tiles([t.data for t in tiles], [t.valid_mask for t in tiles], unc, [grid.resolution] * len(tiles),
                              device=device, densities=den, **kw)

    @classmethod
    def from_ground_truth(cls, labels, difference, noisy_depth, uncertainty=None, resolution=(1.0, 1.0), tile_size: int = 512,
                          overlap: int = 64, min_valid_ratio: float = 0.1, device=None, density=None, **kw) -> "TileStore":
        """A ground-truth raster as its bands hold it: 1 labels (0 seafloor, 2 noise, -1 nodata), 2 difference (noisy - clean),
        3 noisy depth, 5 uncertainty (optional); ``density``: the raster's sounding density plane (optional, of the same kind as
        the other planes).  Cut with ``plan_ground_truth_tiles``; a cell is valid where its label is
        >= 0.  The planes are host arrays, or device tensors (``GroundTruth.training_planes()``): then only the label plane is
        copied to the host, to plan the tiles, and the tiles are cut on the device; the store is the same bit for bit."""
        device = rt.resolve_device(device)
        on_device = isinstance(labels, torch.Tensor)
        if on_device:
            if any(p is not None and not isinstance(p, torch.Tensor) for p in (difference, noisy_depth, uncertainty, density)):
                raise TypeError("labels is a tensor: the other planes must be tensors too")
            labels_dev = labels.to(device=device, dtype=torch.int32)
            labels = labels_dev.cpu().numpy()
        else:
            labels = np.asarray(labels).astype(np.int32)
        boxes, counts = plan_ground_truth_tiles(labels, tile_size, overlap, min_valid_ratio)
        if not boxes:
            raise ValueError("the ground-truth raster yields no tile")
        planes = {"labels": (labels_dev if on_device else labels, np.int32), "difference": (difference, np.float32),
                  "depth": (noisy_depth, np.float32)}
        if uncertainty is not None:
            planes["unc"] = (uncertainty, np.float32)
        if density is not None:
            planes["density"] = (density, np.float32)
        flat = {}
        for k, (arr, dt) in planes.items():
            if not on_device:
                arr = np.asarray(arr)
            if tuple(arr.shape) != tuple(labels.shape):
                raise ValueError(f"{k} has shape {tuple(arr.shape)}, labels {labels.shape}")
            if on_device:
                arr = arr.to(device=device, dtype=torch.int32 if dt is np.int32 else torch.float32)
                flat[k] = torch.cat([arr[r0:r1, c0:c1].reshape(-1) for r0, c0, r1, c1 in boxes])
            else:
                flat[k] = torch.from_numpy(np.concatenate([np.ascontiguousarray(arr[r0:r1, c0:c1], dt).ravel()
                                                           for r0, c0, r1, c1 in boxes])).to(device)
        hw = np.array([(r1 - r0, c1 - c0) for r0, c0, r1, c1 in boxes], np.int32)
        res = np.array([(float(resolution[0]), float(resolution[1]))] * len(boxes), np.float64)
        store = cls("ground_truth", hw, res, flat["depth"], (flat["labels"] >= 0).view(torch.uint8), flat.get("unc"),
                    labels=flat["labels"], difference=flat["difference"], class_counts=counts, device=device,
                    node_counts=[int(np.count_nonzero(labels[r0:r1, c0:c1] >= 0)) for r0, c0, r1, c1 in boxes],
                    density=flat.get("density"), **kw)
        store.boxes = boxes
        return store

    @classmethod
    def from_ground_truths(cls, rasters, tile_size: int = 512, overlap: int = 64, min_valid_ratio: float = 0.1, device=None,
                           densities=None, **kw) -> "TileStore":
        """One ``"ground_truth"`` store from several ground-truth rasters (the reference's ``GroundTruthDataset`` takes a list
        of them), planned and cut on the device: no plane leaves HBM.  ``rasters``: a sequence whose items are a
        ``data.GroundTruth`` (its ``training_planes()``, at the resolution ``(abs(transform[1]), abs(transform[5]))``, or
        ``(1.0, 1.0)`` without a transform) or a tuple ``(labels, difference, noisy_depth, uncertainty_or_None, resolution)`` of
        device tensors; host arrays are accepted too and uploaded once per plane.  The rasters need not share a shape or a
        resolution; either all of them have an uncertainty plane or none has.

        Per raster: ``plan_tile_boxes``, one ``bgnn_tile_scan`` of the label plane, one copy of the counts to the host (32 bytes
        per box: the only synchronisation), ``keep_ground_truth_boxes``, one ``bgnn_tile_cut``.  The store's planes are allocated
        ONCE for all rasters, after a first pass that scans every raster; the second pass cuts at running offsets.  A raster that
        yields no tile is skipped with a logged warning; no tile at all raises.

        The store is ``from_ground_truth`` of every raster, concatenated, bit for bit (tiles in raster order and in the reference's
        scan order inside a raster; the mask is ``labels >= 0``); ``boxes`` lists ``(r0, c0, r1, c1)`` per tile, ``sources`` (int32)
        the index of its raster in ``rasters``, the class counts are summed over the rasters.

        ``densities``: one sounding density plane per raster (of the raster's shape; all or none), cut with the same boxes in a
        second ``bgnn_tile_cut`` per raster (the first one's four planes are taken)."""
        from ..data.ground_truth import GroundTruth
        device = rt.resolve_device(device)
        ctx = rt.get_context(device)
        names = ("labels", "difference", "depth", "unc")
        scanned = []
        for k, item in enumerate(rasters):
            if isinstance(item, GroundTruth):
                labels, difference, depth, unc = item.training_planes()
                tr = item.transform
                resolution = (1.0, 1.0) if tr is None else (abs(tr[1]), abs(tr[5]))
            else:
                labels, difference, depth, unc, resolution = item
            given = [p for p in (labels, difference, depth, unc) if p is not None]
            if len({isinstance(p, torch.Tensor) for p in given}) != 1:
                raise TypeError(f"raster {k}: its planes must be all tensors or all host arrays")
            planes = [_plane_to_device(labels, torch.int32, device), _plane_to_device(difference, torch.float32, device),
                      _plane_to_device(depth, torch.float32, device), None if unc is None else _plane_to_device(unc, torch.float32, device)]
            if planes[0].dim() != 2:
                raise ValueError(f"raster {k}: labels must be a 2-D grid, got shape {tuple(planes[0].shape)}")
            for name, p in zip(names, planes):
                if p is not None and tuple(p.shape) != tuple(planes[0].shape):
                    raise ValueError(f"raster {k}: {name} has shape {tuple(p.shape)}, labels {tuple(planes[0].shape)}")
            scanned.append({"index": k, "planes": planes, "res": (float(resolution[0]), float(resolution[1]))})
        if len({r["planes"][3] is None for r in scanned}) > 1:
            raise ValueError("some rasters have an uncertainty plane and some have none: the graphs would differ in in_channels")
        if densities is not None:
            densities = list(densities)
            if len(densities) != len(scanned) or len({a is None for a in densities}) > 1:
                raise ValueError("densities: one sounding density plane per raster, for every raster or for none")
            if densities[0] is None:
                densities = None
        if densities is not None:
            for r, a in zip(scanned, densities):
                r["density"] = _plane_to_device(a, torch.float32, device)
                if tuple(r["density"].shape) != tuple(r["planes"][0].shape):
                    raise ValueError(f"raster {r['index']}: density has shape {tuple(r['density'].shape)}, labels "
                                     f"{tuple(r['planes'][0].shape)}")
        for r in scanned:                                # first pass: every raster's scan is queued before any count is read
            height, width = r["planes"][0].shape
            r["candidates"] = plan_tile_boxes(height, width, tile_size, overlap)
            r["counts"] = scan_tile_boxes(r["planes"][0], r["candidates"], ctx=ctx)
        class_counts = {0: 0, 1: 0, 2: 0}
        for r in scanned:
            scan = r["counts"].cpu().numpy()
            rows = _kept_rows(r["candidates"], scan, min_valid_ratio)
            r["boxes"], r["nodes"] = [r["candidates"][i] for i in rows], [int(scan[i][0]) for i in rows]
            for c in class_counts:
                class_counts[c] += sum(int(scan[i][1 + c]) for i in rows)
            if not rows:
                logger.warning(f"raster {r['index']} ({tuple(r['planes'][0].shape)}) yields no tile, skipping")
        boxes = [b for r in scanned for b in r["boxes"]]
        if not boxes:
            raise ValueError("the ground-truth rasters yield no tile")
        hw, stores, mask = _cut_store([(r["planes"], r["boxes"]) for r in scanned], ctx=ctx)      # second pass: one cut per raster
        res = np.array([r["res"] for r in scanned for _ in r["boxes"]], np.float64)
        den = None if densities is None else _cut_store([([r["density"]], r["boxes"]) for r in scanned], ctx=ctx)[1][0]
        store = cls("ground_truth", hw, res, stores[2], mask, stores[3], labels=stores[0], difference=stores[1],
                    class_counts=class_counts, device=device, node_counts=[v for r in scanned for v in r["nodes"]], density=den, **kw)
        store.boxes = boxes
        store.sources = np.array([r["index"] for r in scanned for _ in r["boxes"]], np.int32)
        return store

    @classmethod
    def from_survey(cls, depth, tile_manager, uncertainty=None, nodata_value: Optional[float] = 1.0e6, resolution=(1.0, 1.0),
                    device=None, density=None, **kw) -> "TileStore":
        """The device form of ``from_grid``: a ``"synthetic"`` store of the tiles ``tile_manager.iterate_tiles(grid,
        skip_empty=True)`` yields for ``BathymetricGrid(depth, uncertainty, nodata_value, resolution=resolution)``, without the
        survey leaving HBM.  ``depth`` / ``uncertainty``: ``[H, W]`` float32 device tensors (host arrays are uploaded once).

        The boxes are ``tile_manager.compute_tile_grid((H, W))`` (ragged at the plane's edges); one ``bgnn_tile_scan`` in depth
        mode counts the cells that are finite and ``!= nodata_value`` (None or NaN: finite only -- ``BathymetricGrid.valid_mask``);
        a tile is dropped when ``valid / size < tile_manager.min_valid_ratio`` (the strict ``<`` of ``iterate_tiles``); one
        ``bgnn_tile_cut`` gathers the rest.

        What ``from_grid`` stores, restated: ``GraphBuilder.upload_tiles`` concatenates each tile's float32 depth AS IT IS --
        invalid cells keep their value, nodata sentinel, NaN payload and infinities included -- the tile's crop of the grid's valid
        mask as uint8, and the uncertainty as it is.  So here the depth and uncertainty words are moved untouched and the mask is
        the predicate on the depth.  The store equals ``from_grid``'s bit for bit: ``hw``, ``res``, ``offsets``, depth, mask,
        uncertainty, ``uniform``.  ``density`` (the survey's sounding density plane, ``SoundingGrid.density_plane``) is a third plane
        of the same cut, moved untouched like the uncertainty."""
        device = rt.resolve_device(device)
        ctx = rt.get_context(device)
        planes = [_plane_to_device(depth, torch.float32, device),
                  None if uncertainty is None else _plane_to_device(uncertainty, torch.float32, device),
                  None if density is None else _plane_to_device(density, torch.float32, device)]
        if planes[2] is not None and tuple(planes[2].shape) != tuple(planes[0].shape):
            raise ValueError(f"density has shape {tuple(planes[2].shape)}, depth {tuple(planes[0].shape)}")
        if planes[0].dim() != 2:
            raise ValueError(f"depth must be a 2-D grid, got shape {tuple(planes[0].shape)}")
        if planes[1] is not None and tuple(planes[1].shape) != tuple(planes[0].shape):
            raise ValueError(f"uncertainty has shape {tuple(planes[1].shape)}, depth {tuple(planes[0].shape)}")
        _, _, specs = tile_manager.compute_tile_grid(tuple(planes[0].shape))
        candidates = [(s.row_start, s.col_start, s.row_end, s.col_end) for s in specs]
        counts = scan_tile_boxes(planes[0], candidates, nodata=nodata_value, ctx=ctx).cpu().numpy()
        kept = [(b, int(row[0])) for b, row in zip(candidates, counts)
                if not int(row[0]) / ((b[2] - b[0]) * (b[3] - b[1])) < tile_manager.min_valid_ratio]
        boxes = [b for b, _ in kept]
        if not boxes:
            raise ValueError("a TileStore needs at least one tile")
        hw, stores, mask = _cut_store([(planes, boxes)], nodata=nodata_value, ctx=ctx)
        res = np.array([(float(resolution[0]), float(resolution[1]))] * len(boxes), np.float64)
        store = cls("synthetic", hw, res, stores[0], mask, stores[1], device=device, node_counts=[v for _, v in kept],
                    density=stores[2], **kw)
        store.boxes = boxes
        return store

    @classmethod
    def from_refinement_pairs(cls, truths, min_valid_ratio: float = 0.0, device=None, **kw) -> "TileStore":
        """A ``"ground_truth"`` store whose tiles are the refinement grids of clean / noisy VR BAG pairs at their native resolution
        (docs/TRAINING_PLAN.md step 4.1).  ``truths``: one ``data.NativeGroundTruth`` (``compute_ground_truth_native``) or a
        sequence of them; either all carry an uncertainty or none does.

        A grid is kept when it is paired, has at least one valid cell, and ``valid / cells >= min_valid_ratio`` in float64 -- and
        when it has at least two cells a side: a narrower grid has no gradient features and ``batch`` would refuse it with
        numpy.gradient's message, as the reference's graph construction does.  The only thing read back is every truth's ``grid_counts`` (32 bytes per grid); the kept grids are compacted on the device, one
        ``bgnn_tile_cut`` per truth over its flat planes viewed as ``[1][T]`` with one-row boxes: ``depth`` is the noisy depth,
        ``hw`` / ``res`` are the grids' own, the mask is ``labels >= 0`` (the truth's own mask), the class counts are summed over the
        kept grids.  ``store.grids``: per truth the indices of its kept grids (int64), ``store.sources`` (int32) the truth of every
        tile.  No grid kept at all raises ``ValueError``."""
        from ..data.vr_ground_truth import NativeGroundTruth
        if kw.get("density") is not None or kw.pop("densities", None) is not None:
            raise NotImplementedError("from_refinement_pairs does not carry the sounding density plane yet: VR refinement grids "
                                      "train without it")
        device = rt.resolve_device(device)
        ctx = rt.get_context(device)
        truths = [truths] if isinstance(truths, NativeGroundTruth) else list(truths)
        for k, t in enumerate(truths):
            if not isinstance(t, NativeGroundTruth):
                raise TypeError(f"truths[{k}] is a {type(t).__name__}: NativeGroundTruth expected (compute_ground_truth_native)")
            if t.labels.device != device:
                raise ValueError(f"truths[{k}] lies on {t.labels.device}, the store on {device}")
        if len({t.uncertainty is None for t in truths}) > 1:
            raise ValueError("some truths carry an uncertainty and some carry none: the graphs would differ in in_channels")
        host_counts = [t.grid_counts.cpu().numpy().reshape(-1, rt.TILE_COUNTS) for t in truths]      # (the only read-back)
        kept, nodes, class_counts = [], [], {0: 0, 1: 0, 2: 0}
        for t, cnt in zip(truths, host_counts):
            cells = np.diff(t.offsets)
            valid = cnt[:, 0]
            keep = np.asarray(t.paired, bool) & (valid >= 1) & (valid / np.maximum(cells, 1) >= min_valid_ratio) & \
                (t.hw.min(axis=1) >= 2)
            kept.append(np.nonzero(keep)[0].astype(np.int64))
            nodes.append(valid[keep])
            for c in class_counts:
                class_counts[c] += int(cnt[keep, 1 + c].sum())
        if sum(len(k) for k in kept) == 0:
            raise ValueError("the refinement pairs yield no grid to train on")
        hw = np.concatenate([t.hw[k] for t, k in zip(truths, kept)]).astype(np.int32).reshape(-1, 2)
        res = np.concatenate([t.res[k] for t, k in zip(truths, kept)]).astype(np.float64).reshape(-1, 2)
        # one gather per truth: its flat planes viewed as [1][T], a kept grid the one-row box of its cells (whose hw is not the grid's)
        _, stores, mask = _cut_store(
            [([p if p is None else p.view(1, -1) for p in (t.labels, t.difference, t.noisy_depth, t.uncertainty)],
              np.stack([np.zeros_like(k), t.offsets[k], np.ones_like(k), t.offsets[k + 1]], axis=1))
             for t, k in zip(truths, kept)], ctx=ctx)
        store = cls("ground_truth", hw, res, stores[2], mask, stores[3], labels=stores[0], difference=stores[1],
                    class_counts=class_counts, device=device, node_counts=np.concatenate(nodes), **kw)
        store.grids = kept
        store.sources = np.concatenate([np.full(len(k), i, np.int32) for i, k in enumerate(kept)])
        return store

    # ---- access ----------------------------------------------------------------------------------------------------------
    def __len__(self) -> int:
        return int(self.hw.shape[0])

    @property
    def in_channels(self) -> int:
        return self.graph_builder.n_node_columns(self.unc is not None, 0 if self.density is None else 1)

    @property
    def node_planes(self) -> List[str]:
        """The planes the store's graphs carry beside the computed node features, in column order: what a checkpoint states as
        ``"node_planes"`` (a sublist of ``rt.NODE_PLANES``)."""
        return [name for name, t in zip(rt.NODE_PLANES, (self.unc, self.density)) if t is not None]

    def gather(self, indices: Sequence[int], ops=None):
        """``(hw, res, planes)`` of the tiles ``indices``, tile ``k`` of them under ``ops[k]`` (``dihedral_ops``;
        include/bgnn_augment.h; None: every tile as it is stored, op 0): ``hw`` / ``res`` as ``transformed_tile_table`` gives
        them, ``planes`` the dict ``depth``, ``mask``, ``unc``, ``labels``, ``difference`` (None where the store has none), every
        plane's tiles concatenated in the order of ``indices``.  One ``bgnn_tile_gather`` launch for all planes, from a table of
        one entry per tile; a tile may be named more than once.  A store with a ``density`` plane returns it as ``density`` too, from
        a second launch with the same table (the first one's four word planes are taken).  Asynchronous on the context's stream, ordered against the
        caller's current stream."""
        idx = np.asarray(list(indices), dtype=np.int64).reshape(-1)
        if idx.size == 0 or idx.min() < 0 or idx.max() >= len(self):
            raise IndexError(f"tile indices {idx.tolist()} outside a store of {len(self)} tiles")
        ops = _ops_array(np.zeros(idx.size, np.int32) if ops is None else ops, idx.size)
        words = {"depth": self.depth, "unc": self.unc, "labels": self.labels, "difference": self.difference}
        for k, t in list(words.items()) + [("mask", self.mask), ("density", self.density)]:
            if t is None:
                continue
            want = (torch.uint8, torch.bool) if k == "mask" else (torch.float32, torch.int32)
            if t.dtype not in want or not t.is_contiguous() or t.device != self.device:
                raise TypeError(f"the store's {k} plane must be a contiguous tensor of {' or '.join(str(w) for w in want)} on {self.device}")
        table = np.zeros(idx.size, dtype=rt.TILE_ENTRY_DTYPE)
        cells = self.offsets[idx + 1] - self.offsets[idx]
        table["src"], table["dst"] = self.offsets[idx], np.cumsum(cells) - cells
        table["h"], table["w"], table["op"] = self.hw[idx, 0], self.hw[idx, 1], ops
        total, store_cells = int(cells.sum()), int(self.offsets[-1])
        out = {k: None if t is None else torch.empty(total, dtype=t.dtype, device=self.device)
               for k, t in list(words.items()) + [("mask", self.mask)]}
        ctx = rt.get_context(self.device)
        ws_bytes = int(ctx.lib.bgnn_tile_gather_workspace_bytes(idx.size))
        ws = _workspace(ws_bytes, self.device)
        ctx.begin()
        rt.check(ctx.lib.bgnn_tile_gather(ctx.handle, _pointers(list(words.values())), _pointers([out[k] for k in words]), len(words),
                                          rt.ptr(self.mask), rt.ptr(out["mask"]), store_cells, total, C.c_void_p(table.ctypes.data),
                                          idx.size, rt.ptr(ws), C.c_size_t(ws_bytes)))
        if self.density is not None:                    # (the key exists only for a store that has the plane)
            out["density"] = torch.empty(total, dtype=self.density.dtype, device=self.device)
            rt.check(ctx.lib.bgnn_tile_gather(ctx.handle, _pointers([self.density]), _pointers([out["density"]]), 1, None, None,
                                              store_cells, total, C.c_void_p(table.ctypes.data), idx.size, rt.ptr(ws),
                                              C.c_size_t(ws_bytes)))
        ctx.end()
        hw, res = transformed_tile_table(self.hw[idx], self.res[idx], ops)
        return hw, res, out

    def batch(self, indices: Sequence[int], epoch: int = 0, noise=None, ops=None):
        """``(graph, targets)`` of the tiles ``indices`` in epoch ``epoch``.  A synthetic store adds noise first
        (``NoiseAugmentor.augment_batch``, or ``generate_batch`` with ``augment=False``; ``noise``: another augmentor or
        generator for this call) with the sample index ``epoch * len(store) + i`` for tile ``i``, so the noise is a function of
        (seed, epoch, tile) alone; the graph is built from the noisy depth.  ``targets``: ``class_labels`` (int64),
        ``correction_targets`` (float32), ``noise_mask`` (bool), one row per node.

        ``ops`` (None: the tiles as they are stored): one op of ``dihedral_ops`` per tile of ``indices``.  The planes come from
        ``gather`` either way, turned under ``ops``; everything after is the same code, so the noise of a synthetic store is added
        AFTER the transform (with the same sample indices), and gradients, slopes, ``local_std`` and the targets are those of the
        turned tile."""
        idx = np.asarray(list(indices), dtype=np.int64).reshape(-1)
        hw, res, p = self.gather(idx, ops)                 # (refuses an empty batch and an index outside the store)
        ctx = rt.get_context(self.device)
        if self.kind == "synthetic":
            source = noise if noise is not None else (self.noise_augmentor if self.noise_augmentor is not None else self.noise_generator)
            samples = [int(epoch) * len(self) + int(i) for i in idx]
            if hasattr(source, "augment_batch"):
                nb = source.augment_batch(hw, p["depth"], p["mask"], sample_indices=samples, ctx=ctx)
            else:
                nb = source.generate_batch(hw, p["depth"], p["mask"], sample_indices=samples, ctx=ctx)
            depth, mode = nb.noisy_depth, rt.TARGETS_SYNTHETIC
            a, b, labels, nmask = nb.noisy_depth, p["depth"], nb.classification, nb.noise_mask.view(torch.uint8)
        else:
            depth, mode = p["depth"], rt.TARGETS_GROUND_TRUTH
            a, b, labels, nmask = p["difference"], None, p["labels"], None
        graph = self.graph_builder.build_from_device(hw, res, depth, p["mask"], p["unc"], ctx=ctx,
                                                     aux_t=[p["density"]] if "density" in p else None)
        targets = training_targets_fused(graph, mode, a, b, labels, nmask)
        return graph, targets


def training_targets_fused(graph, mode: int, a: torch.Tensor, b: Optional[torch.Tensor], labels: torch.Tensor,
                           noise_mask: Optional[torch.Tensor]) -> Dict[str, torch.Tensor]:
    """``bgnn_training_targets`` on a graph from ``build_from_device`` and the flat per-cell planes of its batch (mode 0: noisy,
    clean, int64 classification, uint8 / bool noise mask -- what ``data.training_targets`` takes; mode 1: difference, None, int32
    labels, None).  Returns the loss's target dict."""
    ctx = graph._ctx
    dev = ctx.device
    cells = int((graph._hw[:, 0].astype(np.int64) * graph._hw[:, 1]).sum())
    want = {"a": torch.float32, "b": torch.float32, "labels": torch.int64 if mode == rt.TARGETS_SYNTHETIC else torch.int32}
    planes = {"a": a, "b": b, "labels": labels, "noise_mask": noise_mask}
    for k, t in list(planes.items()):
        if t is None:
            continue
        if k == "noise_mask":
            if t.dtype not in (torch.uint8, torch.bool):
                raise TypeError(f"noise_mask must be uint8 or bool, got {t.dtype}")
            t = t.view(torch.uint8) if t.dtype == torch.bool else t
        elif t.dtype != want[k]:
            raise TypeError(f"{k} must be {want[k]}, got {t.dtype}")
        if t.numel() != cells or t.device != dev:
            raise ValueError(f"{k} must hold one entry per cell of the graph's batch ({cells}) on {dev}")
        planes[k] = t.contiguous().view(-1)
    if mode == rt.TARGETS_SYNTHETIC and (planes["b"] is None or planes["noise_mask"] is None):
        raise ValueError("mode 0 takes the clean plane and the noise mask")
    n = graph.num_nodes
    y = torch.empty(n, dtype=torch.int64, device=dev)
    target = torch.empty(n, dtype=torch.float32, device=dev)
    mask = torch.empty(n, dtype=torch.uint8, device=dev)
    if n > 0:
        ctx.begin()
        rt.check(ctx.lib.bgnn_training_targets(ctx.handle, graph._handle, int(mode), rt.ptr(planes["a"]), rt.ptr(planes["b"]),
                                               rt.ptr(planes["labels"]), rt.ptr(planes["noise_mask"]), rt.ptr(y), rt.ptr(target),
                                               rt.ptr(mask)))
        ctx.end()
    return {"class_labels": y, "correction_targets": target, "noise_mask": mask.view(torch.bool)}
