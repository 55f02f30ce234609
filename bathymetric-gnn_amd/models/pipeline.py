"""Tile-batch inference -- drop-in for the reference's ``models/pipeline.py``.

``TileBatchEngine`` is the MI355X-native core: a batch of tiles goes through ONE fused call
(``bgnn_infer_tiles``: graph build -> forward -> node-to-grid scatter + correction
de-normalisation) and comes back as three [h, w] grids per tile.  ``BathymetricPipeline`` keeps the
reference's class surface (``__init__``, ``load_model``, ``process``, ``_process_tile``,
``_apply_corrections``) on top of it; ``process_grid`` is the in-memory entry (file I/O needs GDAL,
which is outside the path).
"""
from __future__ import annotations

import ctypes as C
import logging
from pathlib import Path
from typing import Dict, List, Optional, Sequence, Tuple, Union

import numpy as np
import torch

from .. import runtime as rt
from ..config import Config
from ..config.constants import CORRECTION_NORM_FLOOR
from ..data import BathymetricGrid, GraphBuilder, TileManager, TileMerger
from .gnn import BathymetricGNN
from .sharding import (TILE_RESULT_CHANNELS, exchange_halo_tile_rows, exchange_tile_results,  # noqa: F401 -- re-exported
                       gather_bands_to_rank0, shard_info, survey_shard_plan)
from .survey import StreamResources, SurveySteps, SurveyTilePlan, survey_resident, survey_streamed

logger = logging.getLogger(__name__)


def check_node_planes(node_planes) -> Optional[Tuple[str, ...]]:
    """``node_planes`` of a checkpoint as a tuple: a sublist of ``rt.NODE_PLANES`` in that order (the column order), or None."""
    if node_planes is None:
        return None
    planes = tuple(str(p) for p in node_planes)
    if planes != tuple(p for p in rt.NODE_PLANES if p in planes) or len(set(planes)) != len(planes):
        raise ValueError(f"node_planes={list(planes)!r}: a sublist of {list(rt.NODE_PLANES)} in that order expected")
    return planes


class TileBatchEngine:
    """Fused per-batch inference on one GPU (one engine per worker / device)."""

    def __init__(self, model: BathymetricGNN, graph_builder: GraphBuilder, device=None,
                 auto_correct_threshold: float = 0.85, review_threshold: float = 0.6,
                 norm_floor: float = CORRECTION_NORM_FLOOR, ctx: Optional[rt.Context] = None,
                 node_planes: Optional[Sequence[str]] = None):
        self.model = model
        # the planes the model takes beside the computed node features (a sublist of rt.NODE_PLANES, from the checkpoint's
        # "node_planes"); None: not stated -- uncertainty is taken when the model's width asks for it, density when it is given
        self.node_planes = check_node_planes(node_planes)
        self.graph_builder = graph_builder
        # ``ctx``: an extra library context (``rt.new_context``) -- engines on different contexts overlap their batches
        self.ctx = ctx if ctx is not None else rt.get_context(device if device is not None else graph_builder._device)
        self.auto_correct_threshold = auto_correct_threshold
        self.review_threshold = review_threshold
        self.norm_floor = norm_floor

    def infer_device(self, hw: np.ndarray, res: np.ndarray, depth_t: torch.Tensor, mask_t: torch.Tensor,
                     unc_t: Optional[torch.Tensor], out=None,
                     n_nodes_out: Optional[torch.Tensor] = None, defer_end: bool = False, begin: bool = True,
                     density_t: Optional[torch.Tensor] = None):
        """Device-resident tiles in, device-resident grids out: returns float32 [3, cells]
        (classification, confidence, correction), same cell layout as ``depth_t``.  Asynchronous
        with respect to the host.  ``defer_end``: do not order the caller's torch stream behind this batch yet (the
        caller calls ``engine.ctx.end()`` before it reads ``out``): batches given to engines on different contexts
        then run concurrently.  ``begin=False``: do not order this batch behind the caller's current torch stream either (the
        inputs were produced on the engine's own stream, or behind an event it already waits for).  ``density_t``: the tiles' sounding
        density, laid out like ``depth_t``: one more node-feature column behind the others (``bgnn_infer_tiles_aux``)."""
        ctx = self.ctx
        cells = depth_t.numel()
        if out is None:
            out = torch.empty((3, cells), dtype=torch.float32, device=ctx.device)
        # `out`: a [3, cells] tensor, or three 1-D [cells] tensors (classification, confidence, correction)
        if not all(o.is_contiguous() and o.numel() == cells for o in (out[0], out[1], out[2])):
            raise RuntimeError(f"infer_device: out holds three contiguous arrays of {cells} cells each")
        tiles, keep = rt.make_tiles(hw, res, depth_t, mask_t, unc_t)
        model_h = self.model.native(ctx, int(self.graph_builder._opts.n_edge_features))
        n_aux, aux, _keep_aux = rt.make_aux_planes([density_t] if density_t is not None else None, cells)
        if begin:
            ctx.begin()
        if n_aux:
            rt.check(ctx.lib.bgnn_infer_tiles_aux(
                ctx.handle, model_h, C.byref(tiles), C.byref(self.graph_builder._opts), n_aux, aux,
                C.c_float(self.auto_correct_threshold), C.c_float(self.review_threshold), C.c_float(self.norm_floor),
                rt.ptr(out[0]), rt.ptr(out[1]), rt.ptr(out[2]), rt.ptr(n_nodes_out)))
        else:
            rt.check(ctx.lib.bgnn_infer_tiles(
                ctx.handle, model_h, C.byref(tiles), C.byref(self.graph_builder._opts),
                C.c_float(self.auto_correct_threshold), C.c_float(self.review_threshold), C.c_float(self.norm_floor),
                rt.ptr(out[0]), rt.ptr(out[1]), rt.ptr(out[2]), rt.ptr(n_nodes_out)))
        if not defer_end:
            ctx.end()
        return out

    def infer(self, depths: Sequence[np.ndarray], masks: Sequence[Optional[np.ndarray]],
              uncs: Optional[Sequence[Optional[np.ndarray]]], resolutions,
              densities: Optional[Sequence[Optional[np.ndarray]]] = None) -> List[Dict[str, np.ndarray]]:
        """Host grids in, per-tile dicts of host grids out.  ``densities``: the tiles' sounding density (all or none)."""
        if len(depths) == 0:
            return []
        have_unc = uncs is not None and any(u is not None for u in uncs)
        have_den = densities is not None and any(a is not None for a in densities)
        if self.node_planes is not None:                 # stated by the checkpoint: exactly those planes, each of them required
            for name, have in (("uncertainty", have_unc), ("sounding_density", have_den)):
                if name in self.node_planes and not have:
                    raise ValueError(f"the model takes the node plane {name!r} and the tiles carry none")
            use_unc = uncs if "uncertainty" in self.node_planes else None
            use_den = densities if "sounding_density" in self.node_planes else None
        else:
            # not stated.  Uncertainty as before: taken when the model is as wide as the builder's columns with it.  Density only
            # where the width asks for a column beyond those (a model as wide as 7 + uncertainty never reads density in its place)
            cols, width = self.graph_builder.n_node_columns, self.model.in_channels
            use_unc = uncs if have_unc and width in (cols(True), cols(True, 1)) else None
            use_den = densities if have_den and width != cols(True) and width == cols(use_unc is not None, 1) else None
        a = self.graph_builder.upload_density(use_den, depths)
        hw, res, d, m, u = self.graph_builder.upload_tiles(depths, masks, use_unc, resolutions)
        out = self.infer_device(hw, res, d, m, u, density_t=a[0] if a else None).cpu().numpy()
        results, off = [], 0
        for i in range(hw.shape[0]):
            h, w = int(hw[i, 0]), int(hw[i, 1])
            n = h * w
            results.append({"classification": out[0, off:off + n].reshape(h, w).copy(),
                            "confidence": out[1, off:off + n].reshape(h, w).copy(),
                            "correction": out[2, off:off + n].reshape(h, w).copy()})
            off += n
        return results


class HostTilePipeline:
    """Host tiles in, host grids out, with both PCIe crossings overlapped with compute.

    The reference's ``_process_tile`` hands host arrays across the boundary one tile at a time
    (models/pipeline.py:253-262 ``.to(device)``, :288-295 ``.cpu()``).  Here a batch of equally sized tiles
    is staged in pinned host memory, copied on a dedicated H2D stream, classified on the engine's stream and
    copied back on a D2H stream; ``depth`` slots (default 2) of pinned + device buffers let batch i+1 upload
    and batch i-1 download while batch i computes.  ``submit`` enqueues a batch and returns the result of the
    batch submitted ``depth`` calls earlier (or None); ``drain`` yields what is still in flight, in order.
    Result arrays are views of a pinned output buffer that stays untouched until the NEXT call of ``submit`` /
    ``drain`` step (there is one output buffer more than there are slots): use or copy them before that."""

    def __init__(self, engine: TileBatchEngine, n_tiles: int, h: int, w: int, with_uncertainty: bool = False,
                 resolution=(1.0, 1.0), depth: int = 2):
        self.eng, self.ctx = engine, engine.ctx
        dev = self.ctx.device
        self.n, self.h, self.w = int(n_tiles), int(h), int(w)
        self.cells = self.n * self.h * self.w
        self.hw = np.tile(np.array([[h, w]], np.int32), (self.n, 1))
        self.res = np.tile(np.array([[float(resolution[0]), float(resolution[1])]], np.float64), (self.n, 1))
        self.h2d, self.d2h = torch.cuda.Stream(dev), torch.cuda.Stream(dev)
        mk = lambda dt, shape=None: torch.empty(shape or self.cells, dtype=dt, device=dev)
        pin = lambda dt, shape=None: torch.empty(shape or self.cells, dtype=dt, pin_memory=True)
        self.slots = []
        for _ in range(depth):
            self.slots.append({
                "h_depth": pin(torch.float32), "h_mask": pin(torch.uint8), "h_unc": pin(torch.float32) if with_uncertainty else None,
                "d_depth": mk(torch.float32), "d_mask": mk(torch.uint8), "d_unc": mk(torch.float32) if with_uncertainty else None,
                "d_out": mk(torch.float32, (3, self.cells)), "h_out": None,
                "up": torch.cuda.Event(), "done": torch.cuda.Event(), "down": torch.cuda.Event(), "busy": False, "tag": None})
        self._free_out = [pin(torch.float32, (3, self.cells)) for _ in range(depth + 1)]
        self._lent = None            # the output buffer whose views the caller currently holds
        self.i = 0

    def _recycle(self):
        if self._lent is not None:
            self._free_out.append(self._lent)
            self._lent = None

    def _result(self, slot):
        slot["down"].synchronize()
        slot["busy"] = False
        self._lent, slot["h_out"] = slot["h_out"], None
        o = self._lent.numpy().reshape(3, self.n, self.h, self.w)
        return slot["tag"], {"classification": o[0], "confidence": o[1], "correction": o[2]}

    def submit(self, depth: np.ndarray, mask: np.ndarray, unc: Optional[np.ndarray] = None, tag=None):
        self._recycle()                                            # views handed out by the previous call expire now
        slot = self.slots[self.i % len(self.slots)]
        self.i += 1
        ready = self._result(slot) if slot["busy"] else None       # also: its device / pinned input buffers are free again
        slot["h_depth"].numpy()[:] = np.asarray(depth, np.float32).reshape(-1)
        slot["h_mask"].numpy()[:] = np.asarray(mask).reshape(-1).view(np.uint8)
        if slot["h_unc"] is not None:
            slot["h_unc"].numpy()[:] = np.asarray(unc, np.float32).reshape(-1)
        slot["h_out"] = self._free_out.pop()                       # never the buffer just lent to the caller
        with torch.cuda.stream(self.h2d):
            slot["d_depth"].copy_(slot["h_depth"], non_blocking=True)
            slot["d_mask"].copy_(slot["h_mask"], non_blocking=True)
            if slot["h_unc"] is not None:
                slot["d_unc"].copy_(slot["h_unc"], non_blocking=True)
            slot["up"].record(self.h2d)
        with torch.cuda.stream(self.ctx.stream):                   # the engine orders its work behind the current stream
            self.ctx.stream.wait_event(slot["up"])
            self.eng.infer_device(self.hw, self.res, slot["d_depth"], slot["d_mask"], slot["d_unc"], out=slot["d_out"])
            slot["done"].record(self.ctx.stream)
        with torch.cuda.stream(self.d2h):
            self.d2h.wait_event(slot["done"])
            slot["h_out"].copy_(slot["d_out"], non_blocking=True)
            slot["down"].record(self.d2h)
        slot["busy"], slot["tag"] = True, tag
        return ready

    def drain(self):
        for k in range(len(self.slots)):
            slot = self.slots[(self.i + k) % len(self.slots)]
            if slot["busy"]:
                self._recycle()
                yield self._result(slot)


class BathymetricPipeline:
    """Complete inference pipeline (reference ``BathymetricPipeline``, models/pipeline.py:36-382)."""

    def __init__(self, config: Config, vr_bag_mode: str = "resampled", tile_batch: int = 16):
        self.config = config
        self.vr_bag_mode = vr_bag_mode
        self.tile_batch = max(1, int(tile_batch))
        self.tile_manager = TileManager(tile_size=config.tile.tile_size, overlap=config.tile.overlap,
                                        min_valid_ratio=config.tile.min_valid_ratio)
        # like the reference (:64-67), include_self_loops is not forwarded
        self.graph_builder = GraphBuilder(connectivity=config.graph.connectivity,
                                          edge_features=config.graph.edge_features)
        self.model: Optional[BathymetricGNN] = None
        self.node_planes: Optional[Tuple[str, ...]] = None
        self._engine: Optional[TileBatchEngine] = None
        self.host_stitch = False      # True: numpy TileMerger on the host even on one GPU (the multi-rank path)
        if config.device != "cuda" or not torch.cuda.is_available():
            raise rt.BgnnError(f"config.device={config.device!r}: this pipeline runs on an MI355X only "
                               "(there is no CPU fallback)")
        self.device = torch.device("cuda", torch.cuda.current_device())
        logger.info(f"Pipeline initialized, device: {self.device}")

    # ---- model -----------------------------------------------------------------------------
    def set_model(self, model: BathymetricGNN, node_planes: Optional[Sequence[str]] = None):
        """``node_planes``: the planes the model takes beside the computed node features, as its checkpoint states them
        (``"node_planes"``: a sublist of ``["uncertainty", "sounding_density"]``).  The pipeline then passes exactly those; a grid
        that lacks one raises ``ValueError``.  None: not stated -- a model of 8 input channels takes uncertainty, as before."""
        self.node_planes = check_node_planes(node_planes)
        if self.node_planes is not None:
            want = self.graph_builder.n_node_columns("uncertainty" in self.node_planes, int("sounding_density" in self.node_planes))
            if want != model.in_channels:
                raise ValueError(f"node_planes={list(self.node_planes)} give {want} node columns, the model has in_channels="
                                 f"{model.in_channels}")
        self.model = model.to(self.device).eval()
        self.model.node_planes = self.node_planes        # (travels with the model: NativeVRProcessor reads it)
        self._engine = TileBatchEngine(self.model, self.graph_builder, self.device,
                                       self.config.inference.auto_correct_threshold,
                                       self.config.inference.review_threshold, node_planes=self.node_planes)

    def load_model(self, model_path: Union[str, Path], trust_pickle: bool = False):
        """Checkpoint -> model (reference :92-132).  Accepts the trainer's dict
        (``model_state_dict`` + ``in_channels`` / ``edge_dim`` / optional ``model_config`` or
        pickled ``config``) and a plain ``{state_dict, meta}`` form.  Loaded with
        ``weights_only=True``.  A checkpoint that pickles the reference's ``Config`` object
        (``training/trainer.py:809-829``) cannot be read that way: unpickling executes code from the file, so it
        is an explicit opt-in (``trust_pickle=True``; the reference does it unconditionally, :105) and needs the
        reference's ``config`` package importable."""
        model_path = Path(model_path)
        if not model_path.exists():
            raise FileNotFoundError(f"Model not found: {model_path}")
        try:
            ckpt = torch.load(model_path, map_location="cpu", weights_only=True)
        except Exception as e:
            if not trust_pickle:
                raise RuntimeError(
                    f"{model_path} cannot be loaded with weights_only=True ({type(e).__name__}: it holds pickled Python "
                    "objects, e.g. the trainer's Config). Unpickling executes code from the file: pass "
                    "load_model(path, trust_pickle=True) only for a checkpoint you trust, or re-save it as "
                    "{'model_state_dict', 'in_channels', 'edge_dim', 'model_config': dict}") from e
            ckpt = torch.load(model_path, map_location="cpu", weights_only=False)
        mc = ckpt.get("model_config", None)
        if mc is None and ckpt.get("config", None) is not None:
            mc = getattr(ckpt["config"], "model", None)
        if mc is None:
            mc = self.config.model
        get = (lambda k, dflt=None: mc.get(k, dflt)) if isinstance(mc, dict) else (lambda k, dflt=None: getattr(mc, k, dflt))
        sd = ckpt.get("model_state_dict", ckpt.get("state_dict"))
        model = BathymetricGNN(
            in_channels=ckpt.get("in_channels", 7), hidden_channels=get("gnn_hidden_channels", 64),
            num_gnn_layers=get("gnn_num_layers", 4), gnn_type=get("gnn_type", "GAT"), heads=get("gnn_heads", 4),
            num_classes=get("num_classes", 3), predict_correction=get("predict_correction", True), dropout=0.0,
            edge_dim=ckpt.get("edge_dim", 3))
        model.load_state_dict(sd)
        planes = ckpt.get("node_planes", None)
        if planes is None:
            self.set_model(model)                      # (no key: the in_channels == 8 rule, as before)
        else:
            self.set_model(model, node_planes=planes)
        logger.info(f"Model loaded from {model_path}")

    # ---- per tile ----------------------------------------------------------------------------
    def _tile_uncertainty(self, tile):
        # The reference passes tile.uncertainty unconditionally (:253), which makes x 8 columns wide
        # and fails for a 7-channel model; like NativeVRProcessor we drop the band when the model
        # does not take it.
        return tile.uncertainty if self._takes_uncertainty() else None

    # ---- which planes the model takes: stated by the checkpoint ("node_planes"), else the in_channels == 8 rule ----
    def _takes_uncertainty(self) -> bool:
        planes = getattr(self, "node_planes", None)
        return "uncertainty" in planes if planes is not None else self.model.in_channels == 8

    def _takes_density(self) -> bool:
        planes = getattr(self, "node_planes", None)
        return planes is not None and "sounding_density" in planes

    def _grid_planes(self, grid):
        """(uncertainty, density) of ``grid`` as the model takes them (None: not taken).  With stated ``node_planes`` a plane the
        grid lacks is a ``ValueError`` that names it."""
        unc = getattr(grid, "uncertainty", None)
        den = getattr(grid, "density", None)
        if getattr(self, "node_planes", None) is not None:
            for name, plane in (("uncertainty", unc), ("sounding_density", den)):
                if name in self.node_planes and plane is None:
                    raise ValueError(f"the model takes the node plane {name!r} and the grid has none")
        return (unc if self._takes_uncertainty() else None), (den if self._takes_density() else None)

    def _refuse_density(self, route: str):
        if self.model is not None and self._takes_density():
            raise NotImplementedError(f"{route} does not carry the sounding density plane yet: a model whose node_planes hold "
                                      "'sounding_density' runs through process_grid / process_survey_device on one GPU")

    def _process_tiles(self, tiles, grid: BathymetricGrid) -> List[Dict[str, np.ndarray]]:
        if self.model is None:
            raise RuntimeError("Model not loaded. Call load_model() first.")
        dens = None
        if self._takes_density():
            _, den = self._grid_planes(grid)
            dens = [den[t.row_start:t.row_end, t.col_start:t.col_end] for t in tiles]
        res = self._engine.infer([t.data for t in tiles], [t.valid_mask for t in tiles],
                                 [self._tile_uncertainty(t) for t in tiles], [grid.resolution] * len(tiles), dens)
        for r, t in zip(res, tiles):
            r["cleaned_depth"] = t.data       # original; corrections are applied after stitching (:310)
        return res

    def _process_tile(self, tile, grid: BathymetricGrid) -> Dict[str, np.ndarray]:
        """One tile -> {'cleaned_depth', 'classification', 'confidence', 'correction'} (reference :243-314)."""
        return self._process_tiles([tile], grid)[0]

    # ---- whole grid ----------------------------------------------------------------------------
    def process_survey_device(self, depth_t: torch.Tensor, valid_t: torch.Tensor, unc_t: Optional[torch.Tensor],
                              resolution, shard: Optional[Tuple[int, int]] = None,
                              survey_shape: Optional[Tuple[int, int]] = None, row_offset: int = 0,
                              density_t: Optional[torch.Tensor] = None):
        """Survey resident in HBM in, ``[4, H, W]`` float32 device tensor out (classification, confidence,
        correction, cleaned depth): tiles are cut (``bgnn_cut_tiles``), filtered by ``min_valid_ratio``
        (``bgnn_tile_valid_counts``), classified batch by batch into three long per-tile result arrays and
        stitched / post-processed by ``bgnn_stitch_tiles``.  Nothing crosses PCIe in between; sized for one
        GPU's 288 GB (a 60000 x 60000 survey @512/128 holds 14 GB of depth, 77 GB of per-tile results and
        58 GB of outputs).

        ``shard=(rank, world)`` (one process per GPU, ``torch.distributed`` initialised, every rank holding the
        survey): the rank classifies the tile rows ``survey_shard_plan`` gives it, receives the few earlier tile
        rows that reach into its band of survey rows (``exchange_halo_tile_rows``, the only inter-GPU traffic)
        and stitches that band; returns ``(row0, row1, [4, row1-row0, W])``.  Every cell sees the same tiles in
        the same ascending order as on one GPU, so the bands concatenate to the single-GPU result bit for bit.

        A rank does not need the whole survey: with ``survey_shape=(H, W)`` and ``row_offset``, ``depth_t`` / ``valid_t`` /
        ``unc_t`` hold only the survey rows ``[row_offset, row_offset + depth_t.shape[0])`` -- what the rank's own tile rows
        span (``survey_rows_of_rank``).

        ``density_t``: the survey's sounding density plane (``SoundingGrid.density_plane``), float32 of ``depth_t``'s shape, for
        a model that takes it: its tile windows are cut like the others and go in as one more node-feature column.  One GPU only."""
        if self.model is None:
            raise RuntimeError("Model not loaded. Call load_model() first.")
        if density_t is not None:
            if shard is not None and shard[1] > 1:
                raise NotImplementedError("the sharded survey path does not carry the sounding density plane yet")
            if density_t.dtype != torch.float32 or not density_t.is_contiguous() or density_t.shape != depth_t.shape:
                raise ValueError("density_t: a contiguous float32 plane of depth_t's shape expected")
        elif self._takes_density():
            raise ValueError("the model takes the node plane 'sounding_density' and density_t is None")
        LH, W = (int(v) for v in depth_t.shape)              # rows held locally
        H = int(survey_shape[0]) if survey_shape is not None else LH
        row_offset = int(row_offset)
        if survey_shape is not None and int(survey_shape[1]) != W:
            raise ValueError(f"survey_shape={tuple(survey_shape)}: the planes are {W} cells wide")
        if not (0 <= row_offset and row_offset + LH <= H):
            raise ValueError(f"row_offset={row_offset}: {LH} local rows do not lie within the survey's {H}")
        if depth_t.dtype != torch.float32 or not depth_t.is_contiguous():
            raise ValueError("depth_t: a contiguous float32 plane expected")
        if not valid_t.is_contiguous() or valid_t.shape != depth_t.shape:
            raise ValueError("valid_t: a contiguous plane of depth_t's shape expected")
        valid_u8 = valid_t.view(torch.uint8) if valid_t.dtype == torch.bool else valid_t
        steps = SurveySteps(self._engine, SurveyTilePlan(self.tile_manager, (H, W)), resolution, self.tile_batch,
                            self.config.inference.auto_correct_threshold)
        R0, R1, o, self.last_tile_counts = survey_resident(steps, self.tile_manager.min_valid_ratio, depth_t, valid_u8, unc_t, density_t,
                                                           shard if shard is not None else (0, 1), row_offset)
        logger.info(f"Processed {self.last_tile_counts[0]} tiles ({self.last_tile_counts[1]} skipped below min_valid_ratio)")
        return o if shard is None else (R0, R1, o)

    def survey_rows_of_rank(self, shape, rank: int, world: int):
        """Survey rows ``[lo, hi)`` rank ``rank`` of ``world`` must hold for a survey of ``shape``: the span of its own tile
        rows (its band of cell rows lies inside it).  (0, 0) for a rank without tile rows."""
        p = SurveyTilePlan(self.tile_manager, shape)
        plan = p.shard_plan(world)
        ta, tb = plan[rank]["tile_rows"]
        return (int(p.rs[ta]), int(p.re[tb - 1])) if tb > ta else (0, 0), plan

    # ---- host grid in, host grids out, streamed (one GPU) -----------------------------------------------------------
    STREAM_MIN_CELLS = 1 << 24        # surveys from 16 M cells on take the streamed form (below: one upload, one download)
    STREAM_BAND_TILE_ROWS = 2         # tile rows classified between two band stitches
    STREAM_UPLOAD_ROWS_BYTES = 128 << 20

    def process_grid_streamed(self, grid: BathymetricGrid, band_tile_rows: Optional[int] = None) -> Dict[str, np.ndarray]:
        """``process_grid_device`` for a survey that lives in HOST memory, with both PCIe crossings and the host-side copies under the
        kernels (reference :163-211 is host arrays in, host arrays out).  Same tiles, same kernels, same stitch as
        ``process_survey_device`` -- the results are bit-identical to it -- in three overlapped roles:

        * an UPLOAD thread copies the survey into pinned slabs and H2D's them chunk by chunk on its own stream; the valid mask is
          made on the device from the depth (``BathymetricGrid.valid_mask``: finite and not the nodata value; a foreign grid
          object's own mask is uploaded instead), and as soon as a tile row's rows are resident its tiles' valid counts are taken
          (``bgnn_tile_valid_counts``) -- the ``min_valid_ratio`` filter never makes the classifying stream wait for the host;
        * THIS thread cuts and classifies the kept tiles, tile row by tile row, into a ring of per-tile result slots that holds
          just the tile rows a stitch can still reach; after every ``band_tile_rows`` tile rows the survey rows NO later tile
          touches are final: they are stitched (``bgnn_stitch_tiles`` on a row band -- the stitch is a per-cell gather, so a band is
          the same arithmetic as the whole survey) together with the valid mask as float32, and queued for download;
        * a DOWNLOAD thread waits for a band's D2H (own stream, pinned slabs) and copies it into the five result arrays -- fresh
          pageable memory, whose first touch costs as much as the copy itself: that runs beside the kernels too."""
        if self.model is None:
            raise RuntimeError("Model not loaded. Call load_model() first.")
        self._refuse_density("process_grid_streamed")
        depth_h = np.ascontiguousarray(grid.depth, dtype=np.float32)
        plain_mask = type(grid) is BathymetricGrid
        valid_h = None if plain_mask else np.ascontiguousarray(grid.valid_mask).view(np.uint8)
        nodata = grid.nodata_value if plain_mask else None
        use_unc = self._grid_planes(grid)[0] is not None
        unc_h = np.ascontiguousarray(grid.uncertainty, dtype=np.float32) if use_unc else None
        steps = SurveySteps(self._engine, SurveyTilePlan(self.tile_manager, grid.shape), grid.resolution, self.tile_batch,
                            self.config.inference.auto_correct_threshold)
        if getattr(self, "_stream_resources", None) is None:      # (made on first use: pinned slabs and the upload context)
            self._stream_resources = StreamResources()
        out, self.last_tile_counts = survey_streamed(
            steps, self._stream_resources, self.tile_manager.min_valid_ratio, depth_h, valid_h, nodata, unc_h,
            max(1, int(band_tile_rows or self.STREAM_BAND_TILE_ROWS)), self.STREAM_UPLOAD_ROWS_BYTES)
        logger.info(f"Processed {self.last_tile_counts[0]} tiles ({self.last_tile_counts[1]} skipped below min_valid_ratio)")
        return out

    def process_grid_device(self, grid: BathymetricGrid) -> Optional[Dict[str, np.ndarray]]:
        """Survey path with everything between the two PCIe crossings on the device: the survey is uploaded once,
        processed by ``process_survey_device`` and the four result grids come back in one copy.  Same results as the host
        merge (``host_stitch = True``), bit for bit, for any number of GPUs.

        Under an initialised ``torch.distributed`` job the survey is row-band sharded: every rank uploads ONLY the rows its
        own tile rows span (not the whole survey), classifies and stitches its band, and the bands go to rank 0 as tensors
        (``gather_bands_to_rank0``).  Rank 0 returns the result dict; the other ranks return None."""
        if self.model is None:
            raise RuntimeError("Model not loaded. Call load_model() first.")
        dev = self._engine.ctx.device
        valid_np = grid.valid_mask
        unc_np, den_np = self._grid_planes(grid)
        use_unc = unc_np is not None
        up = lambda a, lo, hi, dt: torch.from_numpy(np.ascontiguousarray(a[lo:hi], dtype=dt)).to(dev)
        rank, world = shard_info()
        H, W = (int(v) for v in grid.shape)
        if world == 1 and H * W >= self.STREAM_MIN_CELLS and den_np is None:
            return self.process_grid_streamed(grid)
        if world == 1:
            depth_t = up(grid.depth, 0, H, np.float32)
            valid_t = torch.from_numpy(np.ascontiguousarray(valid_np).view(np.uint8)).to(dev)
            unc_t = up(grid.uncertainty, 0, H, np.float32) if use_unc else None
            den_t = up(den_np, 0, H, np.float32) if den_np is not None else None
            host = self.process_survey_device(depth_t, valid_t, unc_t, grid.resolution, density_t=den_t).cpu().numpy()
        else:               # row bands: each rank holds and stitches its own rows; the bands are gathered once at the end
            self._refuse_density("the sharded survey path")
            (lo, hi), plan = self.survey_rows_of_rank((H, W), rank, world)
            band = None
            if hi > lo:
                depth_t = up(grid.depth, lo, hi, np.float32)
                valid_t = torch.from_numpy(np.ascontiguousarray(valid_np[lo:hi]).view(np.uint8)).to(dev)
                unc_t = up(grid.uncertainty, lo, hi, np.float32) if use_unc else None
                _, _, band = self.process_survey_device(depth_t, valid_t, unc_t, grid.resolution, shard=(rank, world),
                                                        survey_shape=(H, W), row_offset=lo)
            host = gather_bands_to_rank0(plan, rank, band, W, device=dev)
            if host is None:
                return None
        return {"cleaned_depth": host[3], "classification": host[0], "confidence": host[1], "correction": host[2],
                "valid_mask": valid_np.astype(np.float32)}

    def process_grid(self, grid: BathymetricGrid) -> Dict[str, np.ndarray]:
        """The body of ``process`` between load and save (reference :163-211), tiles batched.

        Default: the device path (``process_grid_device``), on one GPU or row-band sharded over the ranks of an
        initialised ``torch.distributed`` job.  With ``host_stitch = True`` (or without a device engine) the
        reference-shaped host merge below runs instead: the tiles that pass the ``min_valid_ratio`` filter are
        dealt round-robin by index to the ranks, each rank classifies its share, the per-tile grids are
        exchanged once (``exchange_tile_results``: tensors, no pickling; tiles are independent, so there is no collective inside the
        data path) and EVERY rank stitches them in ascending spec order -- the float32 blend sums and the
        ``>`` tie rule of the discrete channel therefore do not depend on the number of GPUs."""
        if self.model is None:
            raise RuntimeError("Model not loaded. Call load_model() first.")
        if getattr(self, "_engine", None) is not None and not getattr(self, "host_stitch", False):
            return self.process_grid_device(grid)      # one GPU, or row bands over the ranks' GPUs
        _, _, specs = self.tile_manager.compute_tile_grid(grid.shape)
        by_pos = {(s.tile_row, s.tile_col): s for s in specs}
        tiles = list(self.tile_manager.iterate_tiles(grid, skip_empty=True))
        rank, world = shard_info()
        mine = list(range(rank, len(tiles), world))
        done = {}
        for i0 in range(0, len(mine), self.tile_batch):
            idx = mine[i0:i0 + self.tile_batch]
            for i, r in zip(idx, self._process_tiles([tiles[i] for i in idx], grid)):
                done[i] = r
        done = exchange_tile_results(done)
        merger = TileMerger(self.tile_manager)
        merger.initialize(grid_shape=grid.shape, channels=["cleaned_depth", "classification", "confidence", "correction"])
        for i in range(len(tiles)):                  # ascending spec order
            t = tiles[i]
            merger.add_tile(by_pos[(t.tile_row, t.tile_col)], done[i])
        num_tiles = len(tiles)
        logger.info(f"Processed {num_tiles} tiles ({len(specs) - num_tiles} skipped below min_valid_ratio)")
        results = merger.finalize()
        valid_mask = grid.valid_mask
        results["valid_mask"] = valid_mask.astype(np.float32)
        unprocessed = valid_mask & np.isnan(results["classification"])
        if np.any(unprocessed):                      # :198-207
            logger.info(f"Preserving {int(np.sum(unprocessed)):,} valid cells from unprocessed tiles")
            results["cleaned_depth"][unprocessed] = grid.depth[unprocessed]
            for ch in ("classification", "confidence", "correction"):
                results[ch][unprocessed] = 0.0
        results["cleaned_depth"] = self._apply_corrections(grid, results)
        return results

    def process(self, input_path, output_path, export_extras: bool = True) -> Dict[str, np.ndarray]:
        """File in, file out (reference :134-241).  Reading / writing BAG / GeoTIFF is the
        reference's GDAL code and is not part of this package."""
        if self.model is None:
            raise RuntimeError("Model not loaded. Call load_model() first.")
        raise ImportError("GDAL is required to read/write survey files; load the grid with the reference's "
                          "BathymetricLoader and call process_grid(grid) instead")

    def _apply_corrections(self, grid: BathymetricGrid, results: Dict[str, np.ndarray]) -> np.ndarray:
        """cleaned = depth - correction where class == NOISE, confidence > threshold, valid (:316-349)."""
        cleaned = grid.depth.copy()
        apply = ((results["classification"] == BathymetricGNN.CLASS_NOISE)
                 & (results["confidence"] > self.config.inference.auto_correct_threshold) & grid.valid_mask)
        cleaned[apply] = grid.depth[apply] - results["correction"][apply]
        nvalid = max(int(np.sum(grid.valid_mask)), 1)
        logger.info(f"Applied corrections to {int(np.sum(apply))} cells ({100 * np.sum(apply) / nvalid:.1f}% of valid)")
        return cleaned
