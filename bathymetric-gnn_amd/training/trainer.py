"""``Trainer`` -- the reference's ``training/trainer.py`` on this package's device path: tiles resident in HBM (``TileStore``),
per-node targets gathered by one kernel (``bgnn_training_targets``), the step's bookkeeping added up on the device
(``EpochMetrics`` over ``bgnn_epoch_accumulate``), and the reference's epoch loop with validation, scheduler, early stopping
(``StopRule``) and checkpoints around the taped forward, ``BathymetricGNNLoss`` and ``FusedAdamW``.

What stays out: GDAL / survey file reading, torch_geometric loaders (``num_workers``, ``pin_memory``), progress bars, wandb,
multi-GPU training, and the models the backward refuses (GCN, zero-padded shapes, layers wider than 256 columns: ``Trainer``
raises at construction).

Geometric augmentation.  The reference's ``augment_rotations`` / ``augment_flips`` flags, which it never reads, are honoured by
``Trainer(augment_geometry=True)``: every training tile is gathered from the store under one of the eight symmetries of the square
(``dihedral_ops``, ``TileStore.gather`` over ``bgnn_tile_gather``, include/bgnn_augment.h) before its graph is built, all planes
alike, so features and targets are those of the turned tile.  Off by default; validation and the training statistics never turn.

Determinism.  An epoch draws from three places only: ``Trainer.step_plan(epoch)`` (the shuffle and the dropout seed of every
step), ``Trainer.augment_plan(epoch)`` (the op of every tile, when ``augment_geometry`` is on) and the noise of a synthetic store,
a function of ``(seed, epoch, tile)``.  Two runs with equal seeds give equal bits, whatever ran before, and a resumed run continues
the run it was saved from bit for bit."""
from __future__ import annotations

import ctypes as C
import dataclasses
import logging
from pathlib import Path
from types import SimpleNamespace
from typing import Any, Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch
from torch.optim.lr_scheduler import CosineAnnealingWarmRestarts, ReduceLROnPlateau

from .. import runtime as rt
from ..config.constants import CORRECTION_NORM_CAP, CORRECTION_NORM_FLOOR
from .losses import BathymetricGNNLoss, compute_class_weights, compute_correction_delta
from .optim import FusedAdamW

logger = logging.getLogger(__name__)

# the reference's TrainingConfig (config/config.py:53-81): what an empty ``Config.training`` dict stands for
TRAINING_DEFAULTS: Dict[str, Any] = {
    "learning_rate": 1e-3, "weight_decay": 1e-4, "batch_size": 4, "epochs": 100, "scheduler": "cosine", "warmup_epochs": 5,
    "patience": 15, "min_delta": 1e-4, "classification_weight": 1.0, "correction_weight": 0.5, "confidence_weight": 0.2,
    "class_weights": None, "augment_rotations": True, "augment_flips": True, "augment_noise_intensity": True,
}


def training_settings(training: Any = None) -> SimpleNamespace:
    """The training settings as attributes, with the reference's defaults filled in.  ``training``: the plain dict this package's
    ``Config.training`` carries, an object with attributes (the reference's ``TrainingConfig``), a ``Config`` of either kind
    (its ``training`` member is taken), or None.  Keys the reference does not know are ignored."""
    if training is not None and not isinstance(training, dict) and hasattr(training, "training"):
        training = training.training
    out = dict(TRAINING_DEFAULTS)
    for k in TRAINING_DEFAULTS:
        if isinstance(training, dict):
            if k in training:
                out[k] = training[k]
        elif training is not None and hasattr(training, k):
            out[k] = getattr(training, k)
    return SimpleNamespace(**out)


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
    height, width = labels.shape
    stride = tile_size - overlap
    if stride <= 0:
        raise ValueError("Tile size must be larger than overlap")
    boxes: List[Tuple[int, int, int, int]] = []
    counts = {0: 0, 1: 0, 2: 0}

    def consider(r0, c0, r1, c1):
        t = labels[r0:r1, c0:c1]
        valid = t >= 0
        if np.sum(valid) / valid.size >= min_valid_ratio:
            boxes.append((r0, c0, r1, c1))
            for c in (0, 1, 2):
                counts[c] += int(np.sum(t[valid] == c))

    for r0 in range(0, height - tile_size + 1, stride):
        for c0 in range(0, width - tile_size + 1, stride):
            consider(r0, c0, r0 + tile_size, c0 + tile_size)
    if height > tile_size and width > tile_size and (height % stride != 0 or width % stride != 0):
        consider(height - tile_size, width - tile_size, height, width)
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


def keep_ground_truth_boxes(boxes, counts, min_valid_ratio: float = 0.1):
    """The keep rule of ``plan_ground_truth_tiles`` on scanned counts: ``boxes[i]`` stays when ``valid / (h * w) >=
    min_valid_ratio`` -- the float64 quotient ``np.sum(valid) / valid.size`` forms, so no tolerance is involved.  ``counts``:
    ``[n, 4]`` integers (valid, class 0, class 1, class 2) per box.  Returns the kept boxes and the class counts summed over them
    (overlaps counted as often as they are cut)."""
    kept: List[Tuple[int, int, int, int]] = []
    total = {0: 0, 1: 0, 2: 0}
    for (r0, c0, r1, c1), row in zip(boxes, counts):
        if int(row[0]) / ((r1 - r0) * (c1 - c0)) >= min_valid_ratio:
            kept.append((r0, c0, r1, c1))
            for c in (0, 1, 2):
                total[c] += int(row[1 + c])
    return kept, total


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
    ws = torch.empty(ws_bytes // 8, dtype=torch.int64, device=dev)
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
    ws = torch.empty(ws_bytes // 8, dtype=torch.int64, device=dev)
    src = (C.c_void_p * len(planes))(*[None if p is None else p.data_ptr() for p in planes])
    dst = (C.c_void_p * len(planes))(*[None if s is None else s.data_ptr() for s in stores])
    ctx.begin()
    rt.check(ctx.lib.bgnn_tile_cut(ctx.handle, src, dst, len(planes), shape[0], shape[1], rt.ptr(mask), int(mask_plane), mode,
                                   float("nan") if nodata is None else float(nodata), C.c_void_p(table.ctypes.data), n, int(cells),
                                   rt.ptr(ws), C.c_size_t(ws_bytes)))
    ctx.end()


def _plane_to_device(plane, dtype: torch.dtype, device) -> torch.Tensor:
    """A host array (uploaded once) or a tensor as a contiguous ``dtype`` tensor on ``device``."""
    if isinstance(plane, torch.Tensor):
        return plane.to(device=device, dtype=dtype).contiguous()
    npdt = np.int32 if dtype == torch.int32 else np.float32
    return torch.from_numpy(np.ascontiguousarray(np.asarray(plane).astype(npdt, copy=False))).to(device)


def ragged_cell_index(offsets: np.ndarray, idx: np.ndarray) -> np.ndarray:
    """The cells ``offsets[i] .. offsets[i + 1] - 1`` of every tile ``i`` of ``idx``, in that order, as one int64 index -- without
    a loop over tiles (a batch of refinement grids holds thousands)."""
    idx = np.asarray(idx, dtype=np.int64)
    first, cells = offsets[idx], offsets[idx + 1] - offsets[idx]
    run0 = np.cumsum(cells) - cells                      # where tile k's run starts in the index
    return np.repeat(first - run0, cells) + np.arange(int(cells.sum()), dtype=np.int64)


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


def dropout_seed(seed: int, global_step: int) -> int:
    """The dropout seed of training step ``global_step`` (epoch * steps per epoch + step) of a run seeded ``seed``:
    ``(seed mod 2^31) * 2^32 + (global_step mod 2^32)``."""
    return ((int(seed) % (1 << 31)) << 32) | (int(global_step) % (1 << 32))


class TileStore:
    """The tiles of a training set, flat in HBM with the ``hw`` / ``res`` tables ``GraphBuilder.build_from_device`` takes: the
    device-resident form of the reference's ``BathymetricGraphDataset(cache_tiles=True)`` (clean tiles, noise added per sample)
    and of its ``GroundTruthDataset`` (label / difference / noisy-depth planes).  ``batch`` turns a list of tile indices into the
    batch's graph and the target dict of ``BathymetricGNNLoss``, without leaving the device.  ``from_ground_truths`` and
    ``from_survey`` build the store from planes that already lie in HBM (include/bgnn_tilestore.h: a scan of the candidate boxes, a
    gather of the kept ones); the other constructors plan on the host.

    ``node_counts`` (host int64, one per tile): the valid cells of every tile, which are its graph's nodes.  Every constructor
    fills it from counts it has on the host anyway (the masks of ``from_tiles``, the scan counts, a truth's ``grid_counts``); a
    store assembled by hand may leave it None.  ``Trainer`` plans its steps with it (``step_plan``)."""

    def __init__(self, kind: str, hw, res, depth, mask, unc=None, labels=None, difference=None, class_counts=None,
                 graph_builder=None, noise_generator=None, augment: bool = True, seed: int = 0, device=None, node_counts=None):
        from ..data import GraphBuilder, NoiseAugmentor, SyntheticNoiseGenerator
        assert kind in ("synthetic", "ground_truth")
        self.kind = kind
        self.device = rt.resolve_device(device)
        self.hw = np.ascontiguousarray(hw, np.int32).reshape(-1, 2)
        self.res = np.ascontiguousarray(res, np.float64).reshape(-1, 2)
        cells = self.hw[:, 0].astype(np.int64) * self.hw[:, 1]
        self.offsets = np.concatenate([[0], np.cumsum(cells)]).astype(np.int64)
        self.depth, self.mask, self.unc, self.labels, self.difference = depth, mask, unc, labels, difference
        for t in (depth, mask, unc, labels, difference):
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
    def from_tiles(cls, depths, valid_masks=None, uncertainties=None, resolutions=None, device=None, **kw) -> "TileStore":
        """Clean tiles (host arrays) for synthetic noise.  ``valid_masks[i]`` None: ``isfinite(depth)``; ``uncertainties``: for
        every tile or for none; ``resolutions``: one ``(x, y)`` per tile (default 1.0).  Keywords: ``graph_builder``,
        ``noise_generator``, ``augment`` (True: ``NoiseAugmentor`` with a drawn intensity per sample), ``seed``."""
        from ..data import GraphBuilder
        device = rt.resolve_device(device)
        gb = kw.get("graph_builder") or GraphBuilder(device=device)
        kw["graph_builder"] = gb
        n = len(depths)
        if n == 0:
            raise ValueError("a TileStore needs at least one tile")
        resolutions = [(1.0, 1.0)] * n if resolutions is None else list(resolutions)
        hw, res, d, m, u = gb.upload_tiles(list(depths), None if valid_masks is None else list(valid_masks), uncertainties, resolutions)
        masks = [None] * n if valid_masks is None else list(valid_masks)
        nodes = [int(np.count_nonzero(np.isfinite(np.asarray(t, dtype=np.float32)) if v is None else np.asarray(v, dtype=bool)))
                 for t, v in zip(depths, masks)]                               # (the masks upload_tiles stores)
        return cls("synthetic", hw, res, d.to(device), m.to(device), None if u is None else u.to(device), device=device,
                   node_counts=nodes, **kw)

    @classmethod
    def from_grid(cls, grid, tile_manager, device=None, **kw) -> "TileStore":
        """The tiles ``tile_manager.iterate_tiles(grid, skip_empty=True)`` yields (trainer.py:351), at the grid's resolution."""
        tiles = list(tile_manager.iterate_tiles(grid, skip_empty=True))
        unc = [t.uncertainty for t in tiles] if tiles and tiles[0].uncertainty is not None else None
        return cls.from_tiles([t.data for t in tiles], [t.valid_mask for t in tiles], unc, [grid.resolution] * len(tiles),
                              device=device, **kw)

    @classmethod
    def from_ground_truth(cls, labels, difference, noisy_depth, uncertainty=None, resolution=(1.0, 1.0), tile_size: int = 512,
                          overlap: int = 64, min_valid_ratio: float = 0.1, device=None, **kw) -> "TileStore":
        """A ground-truth raster as its bands hold it: 1 labels (0 seafloor, 2 noise, -1 nodata), 2 difference (noisy - clean),
        3 noisy depth, 5 uncertainty (optional).  Cut with ``plan_ground_truth_tiles``; a cell is valid where its label is
        >= 0.  The planes are host arrays, or device tensors (``GroundTruth.training_planes()``): then only the label plane is
        copied to the host, to plan the tiles, and the tiles are cut on the device; the store is the same bit for bit."""
        device = rt.resolve_device(device)
        on_device = isinstance(labels, torch.Tensor)
        if on_device:
            if any(p is not None and not isinstance(p, torch.Tensor) for p in (difference, noisy_depth, uncertainty)):
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
                    node_counts=[int(np.count_nonzero(labels[r0:r1, c0:c1] >= 0)) for r0, c0, r1, c1 in boxes], **kw)
        store.boxes = boxes
        return store

    @classmethod
    def from_ground_truths(cls, rasters, tile_size: int = 512, overlap: int = 64, min_valid_ratio: float = 0.1, device=None,
                           **kw) -> "TileStore":
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
        the index of its raster in ``rasters``, the class counts are summed over the rasters."""
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
        for r in scanned:                                # first pass: every raster's scan is queued before any count is read
            height, width = r["planes"][0].shape
            r["candidates"] = plan_tile_boxes(height, width, tile_size, overlap)
            r["counts"] = scan_tile_boxes(r["planes"][0], r["candidates"], ctx=ctx)
        class_counts = {0: 0, 1: 0, 2: 0}
        for r in scanned:
            scan = r["counts"].cpu().numpy()
            r["boxes"], counts = keep_ground_truth_boxes(r["candidates"], scan, min_valid_ratio)
            r["nodes"] = [int(row[0]) for (r0, c0, r1, c1), row in zip(r["candidates"], scan)      # (the keep rule, on the same rows)
                          if int(row[0]) / ((r1 - r0) * (c1 - c0)) >= min_valid_ratio]
            for c in class_counts:
                class_counts[c] += counts[c]
            if not r["boxes"]:
                logger.warning(f"raster {r['index']} ({tuple(r['planes'][0].shape)}) yields no tile, skipping")
        boxes = [b for r in scanned for b in r["boxes"]]
        if not boxes:
            raise ValueError("the ground-truth rasters yield no tile")
        hw = np.array([(r1 - r0, c1 - c0) for r0, c0, r1, c1 in boxes], np.int32)
        offsets = np.concatenate([[0], np.cumsum(hw[:, 0].astype(np.int64) * hw[:, 1])])
        cells = int(offsets[-1])
        with_unc = scanned[0]["planes"][3] is not None
        stores = [torch.empty(cells, dtype=torch.int32, device=device), torch.empty(cells, dtype=torch.float32, device=device),
                  torch.empty(cells, dtype=torch.float32, device=device),
                  torch.empty(cells, dtype=torch.float32, device=device) if with_unc else None]
        mask = torch.empty(cells, dtype=torch.uint8, device=device)
        first = 0
        for r in scanned:                                # second pass: one cut per raster at its running offset
            n = len(r["boxes"])
            cut_tile_boxes(r["planes"], stores, r["boxes"], offsets[first:first + n], mask=mask, mask_plane=0, ctx=ctx)
            first += n
        res = np.array([r["res"] for r in scanned for _ in r["boxes"]], np.float64)
        store = cls("ground_truth", hw, res, stores[2], mask, stores[3], labels=stores[0], difference=stores[1],
                    class_counts=class_counts, device=device, node_counts=[v for r in scanned for v in r["nodes"]], **kw)
        store.boxes = boxes
        store.sources = np.array([r["index"] for r in scanned for _ in r["boxes"]], np.int32)
        return store

    @classmethod
    def from_survey(cls, depth, tile_manager, uncertainty=None, nodata_value: Optional[float] = 1.0e6, resolution=(1.0, 1.0),
                    device=None, **kw) -> "TileStore":
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
        uncertainty, ``uniform``."""
        device = rt.resolve_device(device)
        ctx = rt.get_context(device)
        planes = [_plane_to_device(depth, torch.float32, device),
                  None if uncertainty is None else _plane_to_device(uncertainty, torch.float32, device)]
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
        hw = np.array([(r1 - r0, c1 - c0) for r0, c0, r1, c1 in boxes], np.int32)
        offsets = np.concatenate([[0], np.cumsum(hw[:, 0].astype(np.int64) * hw[:, 1])])
        cells = int(offsets[-1])
        stores = [torch.empty(cells, dtype=torch.float32, device=device),
                  None if planes[1] is None else torch.empty(cells, dtype=torch.float32, device=device)]
        mask = torch.empty(cells, dtype=torch.uint8, device=device)
        cut_tile_boxes(planes, stores, boxes, offsets[:-1], mask=mask, mask_plane=0, nodata=nodata_value, ctx=ctx)
        res = np.array([(float(resolution[0]), float(resolution[1]))] * len(boxes), np.float64)
        store = cls("synthetic", hw, res, stores[0], mask, stores[1], device=device, node_counts=[v for _, v in kept], **kw)
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
        offsets = np.concatenate([[0], np.cumsum(hw[:, 0].astype(np.int64) * hw[:, 1])])
        cells = int(offsets[-1])
        with_unc = truths[0].uncertainty is not None
        stores = [torch.empty(cells, dtype=torch.int32, device=device), torch.empty(cells, dtype=torch.float32, device=device),
                  torch.empty(cells, dtype=torch.float32, device=device),
                  torch.empty(cells, dtype=torch.float32, device=device) if with_unc else None]
        mask = torch.empty(cells, dtype=torch.uint8, device=device)
        first = 0
        for t, k in zip(truths, kept):                   # one gather per truth at its running offset
            if len(k) == 0:
                continue
            src = t.offsets[k]
            boxes = np.stack([np.zeros_like(src), src, np.ones_like(src), t.offsets[k + 1]], axis=1)
            planes = [p if p is None else p.view(1, -1) for p in (t.labels, t.difference, t.noisy_depth, t.uncertainty)]
            cut_tile_boxes(planes, stores, boxes, offsets[first:first + len(k)], mask=mask, mask_plane=0, ctx=ctx)
            first += len(k)
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
        return self.graph_builder.n_node_columns(self.unc is not None)

    def _gather(self, idx: np.ndarray):
        """hw, res and the planes of the tiles ``idx``, concatenated in that order (one index-copy per plane)."""
        planes = {"depth": self.depth, "mask": self.mask, "unc": self.unc, "labels": self.labels, "difference": self.difference}
        if self.uniform:
            cells = int(self.hw[0, 0]) * int(self.hw[0, 1])
            sel = torch.as_tensor(idx, dtype=torch.int64).to(self.device)
            out = {k: None if p is None else p.view(len(self), cells).index_select(0, sel).reshape(-1) for k, p in planes.items()}
        else:
            sel = torch.from_numpy(ragged_cell_index(self.offsets, idx)).to(self.device)
            out = {k: None if p is None else p.index_select(0, sel) for k, p in planes.items()}
        return np.ascontiguousarray(self.hw[idx]), np.ascontiguousarray(self.res[idx]), out

    def gather(self, indices: Sequence[int], ops):
        """``(hw, res, planes)`` of the tiles ``indices``, tile ``k`` of them under ``ops[k]`` (``dihedral_ops``;
        include/bgnn_augment.h): ``hw`` / ``res`` as ``transformed_tile_table`` gives them, ``planes`` the dict ``depth``,
        ``mask``, ``unc``, ``labels``, ``difference`` (None where the store has none), every plane's tiles concatenated in the
        order of ``indices``.  One ``bgnn_tile_gather`` launch for all planes, from a table of one entry per tile; a tile may be
        named more than once.  Asynchronous on the context's stream, ordered against the caller's current stream."""
        idx = np.asarray(list(indices), dtype=np.int64).reshape(-1)
        if idx.size == 0 or idx.min() < 0 or idx.max() >= len(self):
            raise IndexError(f"tile indices {idx.tolist()} outside a store of {len(self)} tiles")
        ops = _ops_array(ops, idx.size)
        words = {"depth": self.depth, "unc": self.unc, "labels": self.labels, "difference": self.difference}
        for k, t in list(words.items()) + [("mask", self.mask)]:
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
        ws = torch.empty(ws_bytes // 8, dtype=torch.int64, device=self.device)
        src = (C.c_void_p * len(words))(*[None if t is None else t.data_ptr() for t in words.values()])
        dst = (C.c_void_p * len(words))(*[None if out[k] is None else out[k].data_ptr() for k in words])
        ctx.begin()
        rt.check(ctx.lib.bgnn_tile_gather(ctx.handle, src, dst, len(words), rt.ptr(self.mask), rt.ptr(out["mask"]), store_cells, total,
                                          C.c_void_p(table.ctypes.data), idx.size, rt.ptr(ws), C.c_size_t(ws_bytes)))
        ctx.end()
        hw, res = transformed_tile_table(self.hw[idx], self.res[idx], ops)
        return hw, res, out

    def batch(self, indices: Sequence[int], epoch: int = 0, noise=None, ops=None):
        """``(graph, targets)`` of the tiles ``indices`` in epoch ``epoch``.  A synthetic store adds noise first
        (``NoiseAugmentor.augment_batch``, or ``generate_batch`` with ``augment=False``; ``noise``: another augmentor or
        generator for this call) with the sample index ``epoch * len(store) + i`` for tile ``i``, so the noise is a function of
        (seed, epoch, tile) alone; the graph is built from the noisy depth.  ``targets``: ``class_labels`` (int64),
        ``correction_targets`` (float32), ``noise_mask`` (bool), one row per node.

        ``ops`` (None: the tiles as they are stored): one op of ``dihedral_ops`` per tile of ``indices``.  The planes then come
        from ``gather``, turned; everything after is the same code, so the noise of a synthetic store is added AFTER the transform
        (with the same sample indices), and gradients, slopes, ``local_std`` and the targets are those of the turned tile."""
        idx = np.asarray(list(indices), dtype=np.int64).reshape(-1)
        if idx.size == 0 or idx.min() < 0 or idx.max() >= len(self):
            raise IndexError(f"tile indices {idx.tolist()} outside a store of {len(self)} tiles")
        ctx = rt.get_context(self.device)
        hw, res, p = self._gather(idx) if ops is None else self.gather(idx, ops)
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
        graph = self.graph_builder.build_from_device(hw, res, depth, p["mask"], p["unc"], ctx=ctx)
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


class EpochMetrics:
    """One accumulator block of ``bgnn_epoch_accumulate`` (include/bgnn_trainer.h) and its single read-back."""

    def __init__(self, device=None):
        self.device = rt.resolve_device(device)
        self._ctx = rt.get_context(self.device)
        self._acc = torch.zeros(rt.EPOCH_ACC_BYTES // 8, dtype=torch.int64, device=self.device)
        self._idle = None            # zero terms / counts for a step that has no loss statistics (an empty batch)
        self.num_classes = None

    def reset(self):
        ctx = self._ctx
        ctx.begin()
        rt.check(ctx.lib.bgnn_epoch_reset(ctx.handle, rt.ptr(self._acc)))
        ctx.end()

    def accumulate(self, graph, terms: torch.Tensor, counts: torch.Tensor, num_classes: int):
        """The raw entry point: ``terms`` float32 [6], ``counts`` int64 [C * C + 7] on the device; n comes from ``graph``."""
        if terms.dtype != torch.float32 or terms.numel() < 6 or counts.dtype != torch.int64 or \
                counts.numel() < num_classes * num_classes + len(rt.LOSS_COUNTS) or not terms.is_contiguous() or not counts.is_contiguous():
            raise ValueError("terms must be float32 [6] and counts int64 [C * C + 7], contiguous")
        ctx = self._ctx
        self.num_classes = int(num_classes)
        ctx.begin()
        rt.check(ctx.lib.bgnn_epoch_accumulate(ctx.handle, graph._handle, rt.ptr(terms), rt.ptr(counts), int(num_classes),
                                               rt.ptr(self._acc)))
        ctx.end()

    def update(self, graph, losses: Dict[str, torch.Tensor], criterion: BathymetricGNNLoss):
        """Add one step: ``losses`` as ``criterion`` returned them for ``graph``'s batch, ``criterion.last_stats`` from that call.
        No host wait."""
        stats = criterion.last_stats
        if stats is None:
            # the loss took its torch path: an empty batch (nothing to add; the kernel sees n = 0 and reads nothing)
            if graph.num_nodes != 0:
                raise rt.BgnnError("EpochMetrics.update: the loss call left no device statistics (BathymetricGNNLoss ran its torch path)")
            if self._idle is None:
                c = rt.EPOCH_MAX_CLASSES
                self._idle = (torch.zeros(6, dtype=torch.float32, device=self.device),
                              torch.zeros(c * c + len(rt.LOSS_COUNTS), dtype=torch.int64, device=self.device))
            known = self.num_classes
            self.accumulate(graph, self._idle[0], self._idle[1], known or 2)
            self.num_classes = known
            return
        conf = stats["confusion"]
        c = int(conf.shape[0])
        if stats["n_masked"].data_ptr() != conf.data_ptr() + 8 * c * c:       # not the loss pass's own block: assemble one
            counts = torch.cat([conf.reshape(-1)] + [stats[k].reshape(1) for k in rt.LOSS_COUNTS])
        else:
            counts = torch.as_strided(conf, (c * c + len(rt.LOSS_COUNTS),), (1,))
        first = losses[rt.LOSS_TERMS[0]]
        if all(losses[k].data_ptr() == first.data_ptr() + 4 * i and losses[k].dtype == torch.float32
               for i, k in enumerate(rt.LOSS_TERMS)):
            terms = torch.as_strided(first.detach(), (6,), (1,))
        else:
            terms = torch.stack([losses[k].detach().to(torch.float32) for k in rt.LOSS_TERMS])
        self.accumulate(graph, terms, counts, c)

    def result(self) -> Dict[str, Any]:
        """The epoch's single device-to-host copy: ``loss`` (sum of total * n over the nodes, 0 when empty), ``accuracy``, the
        five term means, ``confusion`` [C, C], ``nodes``, ``steps``."""
        host = self._acc.cpu().numpy()
        sums = host[:6].view(np.float64)
        nodes, correct, steps = (int(v) for v in host[6:9])
        c = self.num_classes or 0
        out = {"loss": float(sums[5]) / nodes if nodes > 0 else 0, "accuracy": correct / nodes if nodes > 0 else 0}
        for i, k in enumerate(rt.LOSS_TERMS[:5]):
            out[k] = float(sums[i]) / nodes if nodes > 0 else 0
        out["confusion"] = host[9:9 + c * c].reshape(c, c).copy()
        out["nodes"], out["steps"] = nodes, steps
        return out


class StopRule:
    """Early stopping as the reference's loop does it (trainer.py:698-706): an epoch improves when its validation loss is below
    the best so far by more than ``min_delta``; ``patience`` epochs in a row without improvement stop the run."""

    def __init__(self, patience: int, min_delta: float):
        self.patience, self.min_delta = patience, min_delta
        self.best = float("inf")
        self.counter = 0

    def update(self, val_loss: float) -> Tuple[bool, bool]:
        """``(improved, stop)``."""
        if val_loss < self.best - self.min_delta:
            self.best = val_loss
            self.counter = 0
            return True, False
        self.counter += 1
        return False, self.counter >= self.patience


class Trainer:
    """Training manager for bathymetric GNN (the reference's ``Trainer``), over ``TileStore`` s.

    ``config``: a ``Config`` of this package (``training`` a plain dict) or of the reference; the training settings are read
    through ``training_settings``.  The model is moved to the store's GPU.  A model the backward pass refuses (GCN, a
    zero-padded shape, layers wider than 256 columns) raises here, with the backward's message.

    ``batch_nodes`` (None: steps of ``batch_size`` tiles, as the reference cuts them): steps cut by cell count instead, for stores
    whose tiles differ widely in size (``TileStore.from_refinement_pairs``: refinement grids of 9 to 2500 cells); see
    ``step_plan``.  Under either rule a step whose tiles would hold fewer than two nodes is joined to a neighbouring step, which
    may then pass ``batch_nodes`` by that tile's cells; a training store whose tiles hold fewer than two nodes altogether raises
    ``ValueError`` here.

    ``augment_geometry`` (None or False: off, the tiles train as they are stored): True turns every training tile by one of the
    eight symmetries of the square per epoch, as the settings' ``augment_rotations`` / ``augment_flips`` allow (``augment_plan``;
    both flags False: every op is the identity, through the same path)."""

    def __init__(self, config, model, train_store: TileStore, val_store: Optional[TileStore] = None, output_dir=None,
                 seed: int = 0, batch_nodes: Optional[int] = None, augment_geometry: Optional[bool] = None):
        if batch_nodes is not None and int(batch_nodes) < 1:
            raise ValueError(f"batch_nodes {batch_nodes}: a positive number of cells, or None")
        nodes = getattr(train_store, "node_counts", None)
        if nodes is not None and int(np.sum(nodes)) < 2:
            raise ValueError(f"the training store's {len(train_store)} tiles hold {int(np.sum(nodes))} node(s) altogether: a training "
                             "step needs at least 2 (BatchNorm's batch statistics)")
        self.batch_nodes = None if batch_nodes is None else int(batch_nodes)
        self.augment_geometry = bool(augment_geometry)
        self.config = config
        self.model = model
        self.train_dataset = self.train_store = train_store
        self.val_dataset = self.val_store = val_store
        self.output_dir = Path(output_dir) if output_dir else Path("./outputs")
        self.output_dir.mkdir(parents=True, exist_ok=True)
        self.seed = int(seed)
        self.settings = training_settings(config)
        self.device = train_store.device
        self.model.to(self.device)
        self._refuse_untrainable()

        self.optimizer = FusedAdamW(model, lr=self.settings.learning_rate, weight_decay=self.settings.weight_decay,
                                    max_grad_norm=1.0)
        if self.settings.scheduler == "cosine":
            self.scheduler = CosineAnnealingWarmRestarts(self.optimizer, T_0=10, T_mult=2)
        elif self.settings.scheduler == "plateau":
            self.scheduler = ReduceLROnPlateau(self.optimizer, mode="min", factor=0.5, patience=5)
        else:
            self.scheduler = None

        class_weights, correction_delta = self._compute_training_stats()
        if class_weights is not None:
            class_weights = class_weights.to(self.device)
            logger.info(f"Class weights: {class_weights.tolist()}")
        logger.info(f"Correction Huber delta: {correction_delta:.3f}")
        self.criterion = BathymetricGNNLoss(
            class_weights=class_weights,
            classification_weight=self.settings.classification_weight,
            correction_weight=self.settings.correction_weight,
            confidence_weight=self.settings.confidence_weight,
            correction_delta=correction_delta,
        )

        self.current_epoch = 0
        self.stop_rule = StopRule(self.settings.patience, self.settings.min_delta)
        self.history: Dict[str, List[float]] = {"train_loss": [], "val_loss": [], "train_acc": [], "val_acc": []}
        self._next_epoch = 0
        self.train_metrics = EpochMetrics(self.device)
        self.val_metrics = EpochMetrics(self.device)
        logger.info(f"Trainer initialized, device: {self.device}")

    # (the reference keeps these two as plain members; here they live in the stop rule)
    best_val_loss = property(lambda self: self.stop_rule.best, lambda self, v: setattr(self.stop_rule, "best", v))
    patience_counter = property(lambda self: self.stop_rule.counter, lambda self, v: setattr(self.stop_rule, "counter", v))

    def _refuse_untrainable(self):
        """Ask the library whether this model has a backward pass (``bgnn_tape_bytes`` on a 4 x 4 graph)."""
        from ..data import GraphBuilder
        ctx = rt.get_context(self.device)
        gb = self.train_store.graph_builder
        probe = GraphBuilder(connectivity=gb.connectivity, include_self_loops=gb.include_self_loops, node_features=gb.node_features,
                             edge_features=gb.edge_features, device=self.device)
        g = probe.build_graphs([np.zeros((4, 4), np.float32)], None, None, [(1.0, 1.0)])
        handle = self.model.native(ctx, g.edge_dim)
        if int(ctx.lib.bgnn_tape_bytes(handle, g._handle)) == 0:
            raise NotImplementedError(ctx.lib.bgnn_last_error().decode(errors="replace"))

    # ---- statistics of the training set ----------------------------------------------------------------------------------
    def _compute_training_stats(self) -> Tuple[Optional[torch.Tensor], float]:
        """Class weights and the Huber delta from the training store (trainer.py:549-660): a synthetic store's first
        ``min(len, 50)`` samples (epoch 0) give the class counts and the normalised corrections of their noise cells; a
        ground-truth store brings its scanned class counts and ``linspace`` of ``min(len, 100)`` samples give the corrections.
        Counting and selection run on the device; the selected magnitudes come to the host once."""
        num_classes = int(self.config.model.num_classes) if hasattr(self.config, "model") else int(self.model.num_classes)
        try:
            store = self.train_store
            counts = torch.zeros(num_classes, dtype=torch.long, device=self.device)
            selected = []
            scanned = hasattr(store, "_class_counts")
            if scanned:
                counts = torch.tensor([int(store._class_counts.get(c, 0)) for c in range(num_classes)], dtype=torch.long,
                                      device=self.device)
                num_samples = min(len(store), 100)
                logger.info(f"Sampling {num_samples} tiles for correction statistics...")
                sample_indices = [int(i) for i in np.linspace(0, len(store) - 1, num_samples, dtype=int)]
            else:
                sample_indices = list(range(min(len(store), 50)))
            for piece in self._pieces(store, np.asarray(sample_indices, dtype=np.int64)):
                _, t = store.batch(piece, epoch=0)
                y, mask, target = t["class_labels"], t["noise_mask"], t["correction_targets"]
                if not scanned and y.numel() > 0:
                    ok = (y >= 0) & (y < num_classes)
                    counts += torch.bincount(y[ok], minlength=num_classes)
                norm = target[mask]
                selected.append(norm[torch.isfinite(norm)])
            counts = counts.cpu()
            class_weights = None
            if counts.sum() > 0:
                logger.info(f"Class distribution: {dict(enumerate(counts.tolist()))}")
                # (on the host, as the reference computes them: the weights are then the same bits as a host replay's)
                class_weights = compute_class_weights(torch.arange(num_classes).repeat_interleave(counts.clamp(min=1)),
                                                      num_classes=num_classes, smoothing=0.1)
            else:
                logger.warning("No valid labels found, skipping class weights")
            combined = torch.cat(selected).cpu().numpy() if selected else np.zeros(0, np.float32)
            if combined.size > 0:
                capped = np.clip(combined, -CORRECTION_NORM_CAP, CORRECTION_NORM_CAP)
                correction_delta = compute_correction_delta(capped, percentile=95.0, min_delta=1.0)
                logger.info(f"Correction stats (normalized by local_std): mean |correction|={np.mean(np.abs(combined)):.3f}, "
                            f"max |correction|={np.max(np.abs(combined)):.3f}, "
                            f"95th percentile={np.percentile(np.abs(combined), 95):.3f}")
            else:
                correction_delta = 1.0
                logger.warning("No noise corrections found, using default delta=1.0")
            return class_weights, correction_delta
        except Exception as e:
            logger.warning(f"Failed to compute training stats: {e}")
            return None, 1.0

    # ---- the plan of an epoch --------------------------------------------------------------------------------------------
    def _pieces(self, store, order: np.ndarray, trainable: bool = False) -> List[np.ndarray]:
        """``order`` cut into the tile lists of consecutive steps: ``batch_size`` tiles each, or, with ``batch_nodes``, greedily by
        the tiles' cell counts.  ``trainable``: no piece may hold fewer than two nodes (BatchNorm's batch statistics need two
        rows, and ``train()`` refuses one); such a piece is joined to the piece before it, the first one to the piece after
        it, and every other piece stays as it was cut.  Needs ``store.node_counts``; without them the cut stands."""
        limit = getattr(self, "batch_nodes", None)
        if limit is None:
            bs = max(1, int(self.settings.batch_size))
            pieces = [order[k:k + bs] for k in range(0, len(order), bs)]
        else:
            cells = np.diff(np.asarray(store.offsets, dtype=np.int64))[order].tolist()
            cuts, run = [0], 0
            for k, c in enumerate(cells):
                if k > cuts[-1] and run + c > limit:
                    cuts.append(k); run = 0
                run += c
            cuts.append(len(cells))
            pieces = [order[a:b] for a, b in zip(cuts[:-1], cuts[1:]) if b > a]
        nodes = getattr(store, "node_counts", None) if trainable else None
        if nodes is None or len(pieces) < 2:
            return pieces
        nodes = np.asarray(nodes, dtype=np.int64)
        joined: List[np.ndarray] = []
        for p in pieces:
            if joined and int(nodes[p].sum()) < 2:
                joined[-1] = np.concatenate([joined[-1], p])
            else:
                joined.append(p)
        if len(joined) > 1 and int(nodes[joined[0]].sum()) < 2:
            joined[1] = np.concatenate([joined[0], joined[1]])
            del joined[0]
        return joined

    def step_plan(self, epoch: int, validation: bool = False) -> List[Tuple[np.ndarray, Optional[int]]]:
        """``(tile indices, dropout seed)`` of every step of epoch ``epoch``.  Training: the tiles in the order
        ``np.random.default_rng([seed, epoch]).permutation(len(train_store))``, cut into pieces of ``batch_size``; the dropout
        seed of step ``k`` is ``dropout_seed(seed, epoch * steps_per_epoch + k)`` and is written to ``model.dropout_seed``
        before the step's forward.  ``validation=True``: the validation store in its own order, seed None (no dropout in
        ``eval()``).  This method, with the stores' noise (a function of (seed, epoch, tile)), is the whole source of randomness
        of an epoch.

        With ``batch_nodes`` set the same order is cut greedily by cell count instead: a piece closes before the tile that would
        take its cells (``store.offsets`` differences) above ``batch_nodes``; a tile larger than that forms a piece alone.  Seeds
        are numbered by piece, as above.

        Under either rule a training piece whose tiles hold fewer than two nodes in total (``store.node_counts``: a refinement
        grid with one valid cell, a last piece of one such tile) cannot train -- ``train()`` needs two rows for BatchNorm's batch
        statistics -- and is joined to the piece before it, or, when it is the first, to the piece after it.  A joined piece may
        therefore pass ``batch_size`` by those tiles and ``batch_nodes`` by their cells; every other piece is as the rule cut it,
        and the seeds are numbered over the pieces that remain.  Validation plans are not joined (``eval()`` takes one node), and
        neither is the plan over a store that carries no node counts."""
        store = self.val_store if validation else self.train_store
        n = len(store)
        order = np.arange(n, dtype=np.int64) if validation else \
            np.random.default_rng([self.seed, int(epoch)]).permutation(n).astype(np.int64)
        pieces = self._pieces(store, order, trainable=not validation)
        if validation:
            return [(p, None) for p in pieces]
        return [(p, dropout_seed(self.seed, int(epoch) * len(pieces) + k)) for k, p in enumerate(pieces)]

    def augment_plan(self, epoch: int) -> np.ndarray:
        """The geometric op (``dihedral_ops``, int8) of every tile of the training store in epoch ``epoch``, as the settings'
        ``augment_rotations`` / ``augment_flips`` ask, drawn from ``np.random.default_rng([seed, epoch, 0xA6])``.  With
        ``augment_geometry`` on, the training step over the tiles ``indices`` passes ``ops[indices]`` to ``TileStore.batch``: the op
        of a tile is a function of (seed, epoch, tile) and does not depend on how the epoch is cut into steps.  Validation, the
        training statistics and the construction-time probe never turn a tile."""
        s = self.settings
        return dihedral_ops(len(self.train_store), bool(s.augment_rotations), bool(s.augment_flips),
                            np.random.default_rng([self.seed, int(epoch), 0xA6]))

    # ---- epochs ------------------------------------------------------------------------------------------------------------
    def _train_epoch(self) -> Dict[str, float]:
        """Run one training epoch."""
        self.model.train()
        metrics = self.train_metrics
        metrics.reset()
        ops = self.augment_plan(self.current_epoch) if getattr(self, "augment_geometry", False) else None
        for indices, drop_seed in self.step_plan(self.current_epoch):
            graph, targets = self.train_store.batch(indices, self.current_epoch, ops=None if ops is None else ops[indices])
            self.model.dropout_seed = drop_seed
            self.optimizer.zero_grad()
            outputs = self.model(graph)
            losses = self.criterion(outputs, targets)
            losses["total"].backward()
            self.optimizer.step()
            metrics.update(graph, losses, self.criterion)
        return metrics.result()

    def _validate_epoch(self) -> Dict[str, float]:
        """Run one validation epoch."""
        self.model.eval()
        metrics = self.val_metrics
        metrics.reset()
        with torch.no_grad():
            for indices, _ in self.step_plan(self.current_epoch, validation=True):
                graph, targets = self.val_store.batch(indices, self.current_epoch)
                outputs = self.model(graph)
                losses = self.criterion(outputs, targets)
                metrics.update(graph, losses, self.criterion)
        return metrics.result()

    def train(self) -> Dict[str, List[float]]:
        """Run the full training loop (trainer.py:662-728; after ``resume`` it continues at the epoch after the checkpoint's).
        Returns the history: ``train_loss``, ``val_loss``, ``train_acc``, ``val_acc``."""
        history = self.history
        epochs = int(self.settings.epochs)
        for epoch in range(self._next_epoch, epochs):
            self.current_epoch = epoch
            train_metrics = self._train_epoch()
            history["train_loss"].append(train_metrics["loss"])
            history["train_acc"].append(train_metrics["accuracy"])
            if self.val_store is not None:
                val_metrics = self._validate_epoch()
                history["val_loss"].append(val_metrics["loss"])
                history["val_acc"].append(val_metrics["accuracy"])
                if self.scheduler is not None:
                    if isinstance(self.scheduler, ReduceLROnPlateau):
                        self.scheduler.step(val_metrics["loss"])
                    else:
                        self.scheduler.step()
                improved, stop = self.stop_rule.update(val_metrics["loss"])
                if improved:
                    self._save_checkpoint("best_model.pt")
                elif stop:
                    logger.info(f"Early stopping at epoch {epoch}")
                    break
                logger.info(f"Epoch {epoch+1}/{epochs} - Train Loss: {train_metrics['loss']:.4f}, "
                            f"Val Loss: {val_metrics['loss']:.4f}, Val Acc: {val_metrics['accuracy']:.4f}")
            else:
                logger.info(f"Epoch {epoch+1}/{epochs} - Train Loss: {train_metrics['loss']:.4f}, "
                            f"Train Acc: {train_metrics['accuracy']:.4f}")
            if (epoch + 1) % 10 == 0:
                self._save_checkpoint(f"checkpoint_epoch_{epoch+1}.pt")
        self._next_epoch = self.current_epoch + 1
        self._save_checkpoint("final_model.pt")
        return history

    # ---- checkpoints -------------------------------------------------------------------------------------------------------
    def _config_dict(self):
        cfg = self.config
        if dataclasses.is_dataclass(cfg) and not isinstance(cfg, type):
            return dataclasses.asdict(cfg)
        return dict(cfg) if isinstance(cfg, dict) else {"training": dict(vars(self.settings))}

    def _save_checkpoint(self, filename: str):
        """The reference's checkpoint (trainer.py:811-825) from plain containers and tensors only, so that
        ``torch.load(weights_only=True)`` and ``BathymetricPipeline.load_model`` read it: ``config`` is a nested dict,
        ``model_config`` holds the model's own shape, ``edge_dim`` is the model's; ``patience_counter``, ``history`` and ``seed``
        let ``resume`` continue the run."""
        m = self.model
        checkpoint = {
            "epoch": int(self.current_epoch),
            "model_state_dict": {k: v.detach().clone() for k, v in m.state_dict().items()},
            "optimizer_state_dict": self.optimizer.state_dict(),
            "best_val_loss": float(self.best_val_loss),
            "config": self._config_dict(),
            "in_channels": int(m.feature_extractor.mlp[0].in_features),
            "edge_dim": m.edge_dim,
            "correction_norm_floor": CORRECTION_NORM_FLOOR,
            "correction_norm_cap": CORRECTION_NORM_CAP,
            "model_config": {"gnn_type": m.gnn_type, "gnn_hidden_channels": int(m.hidden_channels),
                             "gnn_num_layers": int(m.num_gnn_layers), "gnn_heads": int(m.heads),
                             "gnn_dropout": float(m.gnn.dropout), "num_classes": int(m.num_classes),
                             "predict_correction": bool(m.predict_correction)},
            "patience_counter": int(self.patience_counter),
            "history": {k: [float(v) for v in vs] for k, vs in self.history.items()},
            "seed": int(self.seed),
        }
        if self.scheduler is not None:
            checkpoint["scheduler_state_dict"] = self.scheduler.state_dict()
        path = self.output_dir / filename
        torch.save(checkpoint, path)
        logger.info(f"Saved checkpoint: {path}")

    def resume(self, path):
        """Restore model, optimizer, scheduler, epoch, best loss, patience counter and history from a checkpoint of this
        class; the next ``train()`` continues at the following epoch."""
        ckpt = torch.load(Path(path), map_location="cpu", weights_only=True)
        self.model.load_state_dict(ckpt["model_state_dict"])
        self.model.to(self.device)
        self.optimizer.load_state_dict(ckpt["optimizer_state_dict"])
        if self.scheduler is not None and "scheduler_state_dict" in ckpt:
            self.scheduler.load_state_dict(ckpt["scheduler_state_dict"])
        self.current_epoch = int(ckpt["epoch"])
        self._next_epoch = self.current_epoch + 1
        self.best_val_loss = float(ckpt["best_val_loss"])
        self.patience_counter = int(ckpt.get("patience_counter", 0))
        hist = ckpt.get("history") or {}
        self.history = {k: [float(v) for v in hist.get(k, [])] for k in ("train_loss", "val_loss", "train_acc", "val_acc")}
        return ckpt
