"""Ground truth at native resolution from a clean / noisy VR BAG pair: step 1.2 of the reference's ``docs/TRAINING_PLAN.md``
(``compute_ground_truth_native``), with both files' refinement records in HBM.

The plan walks the clean file's refinement grids in Python, looks each up in a dictionary of the noisy file's grids, and labels
the pair cell by cell.  Here ``vr_pair_table`` decides on the host, vectorised over the base grid, which noisy grid faces which
record range of the clean file; ``compute_ground_truth_native`` uploads the two record arrays as they are and runs everything per
cell as ``bgnn_vr_ground_truth`` (include/bgnn_vrtruth.h): labels, difference, mask, the copied-out noisy depth and uncertainty,
the per-grid counts, the statistics and the exact median of the noise magnitudes.  The outputs are flat, grid after grid in the
noisy file's iteration order (row-major over the base grid, cells of a zero dimension skipped): the record order of
``NativeVRProcessor.process_refinements(noisy, return_results=True)``, so a classified BAG is evaluated against them as it stands
(``NativeGroundTruth.evaluate``), and ``TileStore.from_refinement_pairs`` cuts its training grids out of them on the device.

GDAL's resampled view (``resampled_shape`` / ``resolution`` of the plan's statistics, the GeoTIFF) stays with the reference."""
from __future__ import annotations

import ctypes as C
import dataclasses
from typing import Any, Dict, Iterator, Optional, Tuple

import numpy as np
import torch

from .. import runtime as rt
from .vr_bag import SRBagHandler, refinement_table

PAIRED, UNPAIRED_MISSING, UNPAIRED_DIMENSIONS = 0, 1, 2
PAIR_REASONS = ("paired", "missing", "dimensions")


@dataclasses.dataclass
class VRPairTable:
    """What ``vr_pair_table`` returns.  One entry per refinement grid of the NOISY file, in its iteration order:
    ``rows`` (``runtime.VT_PAIR_DTYPE``: the table ``bgnn_vr_ground_truth`` takes), ``base_row`` / ``base_col``, ``hw`` (int32
    ``[G, 2]``: rows, columns), ``res`` (float64 ``[G, 2]``: x, y, the noisy file's), ``clean_res`` (the clean twin's, NaN without
    one), ``reason`` (int8: ``PAIRED``, ``UNPAIRED_MISSING`` -- the clean file has no grid there --, ``UNPAIRED_DIMENSIONS``);
    ``clean_only``: the grids that exist in the clean file alone; ``total``: the cells of all noisy grids."""
    rows: np.ndarray
    base_row: np.ndarray
    base_col: np.ndarray
    hw: np.ndarray
    res: np.ndarray
    clean_res: np.ndarray
    reason: np.ndarray
    clean_only: int
    total: int
    base_shape: Tuple[int, int]

    @property
    def paired(self) -> np.ndarray:
        return self.reason == PAIRED

    @property
    def offsets(self) -> np.ndarray:
        return np.concatenate([self.rows["out_offset"], [self.total]]).astype(np.int64)

    def unpaired(self) -> Dict[str, int]:
        """``{"missing": n, "dimensions": n, "clean_only": n}``."""
        return {"missing": int(np.count_nonzero(self.reason == UNPAIRED_MISSING)),
                "dimensions": int(np.count_nonzero(self.reason == UNPAIRED_DIMENSIONS)), "clean_only": int(self.clean_only)}


def _num_records(handler) -> int:
    return int(handler.varres_refinements.shape[-1])


def vr_pair_table(clean_handler, noisy_handler) -> VRPairTable:
    """Pair the refinement grids of a noisy VR BAG with those of its clean twin, on the host and without a loop over grids.

    The base shapes must agree (the plan's own check; ``ValueError`` with its message).  A noisy grid at base cell ``(r, c)`` is
    paired iff the clean metadata at ``(r, c)`` has non-zero dimensions equal to the noisy ones -- the plan's dictionary lookup
    and its ``dimensions`` comparison; the two files may lay their records out in different orders, each grid's ``index`` is its
    own file's.  A refined cell of either file whose record range leaves that file raises ``ValueError``."""
    cs, ns = tuple(clean_handler.base_shape), tuple(noisy_handler.base_shape)
    if cs != ns:
        raise ValueError(f"Base shape mismatch: clean {cs} vs noisy {ns}")
    cmd, nmd = np.asarray(clean_handler.varres_metadata), np.asarray(noisy_handler.varres_metadata)
    if cmd.shape != nmd.shape:
        raise ValueError(f"Base shape mismatch: clean {cmd.shape} vs noisy {nmd.shape}")
    tab = refinement_table(nmd)
    ctab = refinement_table(cmd)
    for name, t, n in (("noisy", tab, _num_records(noisy_handler)), ("clean", ctab, _num_records(clean_handler))):
        bad = np.nonzero(t["index"] + t["cells"] > n)[0]
        if bad.size:
            g = int(bad[0])
            raise ValueError(f"{name} file: the refinement grid at base cell ({int(t['base_row'][g])}, {int(t['base_col'][g])}) holds "
                             f"records {int(t['index'][g])} .. {int(t['index'][g] + t['cells'][g])} of {n}")
    r, c = tab["base_row"], tab["base_col"]
    twin = cmd[r, c]
    cdx, cdy = twin["dimensions_x"].astype(np.int64), twin["dimensions_y"].astype(np.int64)
    exists = (cdx != 0) & (cdy != 0)
    same = exists & (cdx == tab["dims_x"]) & (cdy == tab["dims_y"])
    reason = np.where(same, PAIRED, np.where(exists, UNPAIRED_DIMENSIONS, UNPAIRED_MISSING)).astype(np.int8)
    n = len(tab["cells"])
    rows = np.zeros(n, dtype=rt.VT_PAIR_DTYPE)
    rows["cells"] = tab["cells"]
    if n:
        np.cumsum(tab["cells"][:-1], out=rows["out_offset"][1:])
    rows["noisy_start"] = tab["index"]
    rows["clean_start"] = np.where(same, twin["index"].astype(np.int64), -1)
    ndx, ndy = nmd["dimensions_x"], nmd["dimensions_y"]
    clean_only = int(len(ctab["cells"]) - np.count_nonzero(exists))
    assert clean_only == int(np.count_nonzero((cmd["dimensions_x"] != 0) & (cmd["dimensions_y"] != 0) & ~((ndx != 0) & (ndy != 0))))
    clean_res = np.stack([np.where(same, twin["resolution_x"], np.nan), np.where(same, twin["resolution_y"], np.nan)], 1)
    return VRPairTable(rows=rows, base_row=r.astype(np.int64), base_col=c.astype(np.int64),
                       hw=np.stack([tab["dims_y"], tab["dims_x"]], 1).astype(np.int32),
                       res=np.stack([tab["res_x"], tab["res_y"]], 1).astype(np.float64), clean_res=clean_res.astype(np.float64),
                       reason=reason, clean_only=clean_only, total=int(tab["cells"].sum()) if n else 0, base_shape=cs)


def _records_to_device(handler, device) -> torch.Tensor:
    """``varres_refinements`` as a float32 ``[N, 2]`` device tensor: uploaded as it is when the dtype is the plain 8-byte
    (depth, depth_uncrt) layout, otherwise converted once on the host."""
    ref = np.asarray(handler.varres_refinements).reshape(-1)
    f = ref.dtype.fields
    plain = (ref.dtype.itemsize == 8 and f["depth"][1] == 0 and f["depth_uncrt"][1] == 4 and f["depth"][0] == np.dtype("<f4")
             and f["depth_uncrt"][0] == np.dtype("<f4"))
    if plain:
        host = np.ascontiguousarray(ref).view(np.float32).reshape(-1, 2)
    else:
        host = np.empty((ref.shape[0], 2), np.float32)
        host[:, 0] = ref["depth"]; host[:, 1] = ref["depth_uncrt"]
    return torch.from_numpy(host).to(device)


def vr_ground_truth_build(noisy_rec: torch.Tensor, clean_rec: torch.Tensor, rows: np.ndarray, total: int,
                          noise_threshold: float = 0.15, nodata: float = 1.0e6, with_uncertainty: bool = True, ctx=None):
    """``bgnn_vr_ground_truth`` on float32 ``[N, 2]`` device record arrays and a ``runtime.VT_PAIR_DTYPE`` host table:
    ``(labels, difference, noisy_depth, uncertainty or None, mask, grid_counts, stats_block)``.  Asynchronous on the context's
    stream, ordered against the caller's current stream."""
    dev = noisy_rec.device
    ctx = ctx if ctx is not None else rt.get_context(dev)
    for name, t in (("noisy", noisy_rec), ("clean", clean_rec)):
        if t.dtype != torch.float32 or t.dim() != 2 or t.shape[1] != 2 or t.device != dev or not t.is_contiguous():
            raise TypeError(f"{name} records must be a contiguous float32 [N, 2] tensor on {dev}")
    rows = np.ascontiguousarray(rows, dtype=rt.VT_PAIR_DTYPE)
    n, total = len(rows), int(total)
    labels = torch.empty(total, dtype=torch.int32, device=dev)
    difference = torch.empty(total, dtype=torch.float32, device=dev)
    depth = torch.empty(total, dtype=torch.float32, device=dev)
    unc = torch.empty(total, dtype=torch.float32, device=dev) if with_uncertainty else None
    mask = torch.empty(total, dtype=torch.uint8, device=dev)
    counts = torch.zeros((n, rt.VT_COUNTS), dtype=torch.int64, device=dev)
    stats = torch.zeros(rt.VT_STATS_BYTES // 8, dtype=torch.int64, device=dev)
    if total == 0:
        stats.view(torch.float64)[4] = float("nan")           # the median of no magnitude
        return labels, difference, depth, unc, mask, counts, stats
    ws_bytes = int(ctx.lib.bgnn_vr_ground_truth_workspace_bytes(total, n))
    ws = torch.empty(ws_bytes // 8, dtype=torch.int64, device=dev)
    ctx.begin()
    rt.check(ctx.lib.bgnn_vr_ground_truth(ctx.handle, rt.ptr(noisy_rec), int(noisy_rec.shape[0]),
                                          rt.ptr(clean_rec) if clean_rec.shape[0] else None, int(clean_rec.shape[0]),
                                          C.c_void_p(rows.ctypes.data), n, total, float(nodata), float(noise_threshold), rt.ptr(ws),
                                          C.c_size_t(ws_bytes), rt.ptr(labels), rt.ptr(difference), rt.ptr(depth), rt.ptr(unc),
                                          rt.ptr(mask), rt.ptr(counts), rt.ptr(stats)))
    ctx.end()
    return labels, difference, depth, unc, mask, counts, stats


@dataclasses.dataclass
class NativeGroundTruth:
    """What ``compute_ground_truth_native`` leaves on the device.  Flat tensors of one entry per cell of the noisy file's
    refinement grids, grid after grid in iteration order: ``labels`` (int32: 0 seafloor, 2 noise, -1 no data or no twin),
    ``difference`` (float32, noisy - clean; NaN without a twin), ``noisy_depth``, ``uncertainty`` (float32, the noisy records as
    they are), ``mask`` (uint8: both depths valid).  Host tables, one row per grid: ``hw`` (int32 ``[G, 2]``), ``res`` (float64
    ``[G, 2]``), ``offsets`` (int64 ``[G + 1]``), ``paired`` (bool), ``base_row`` / ``base_col``.  ``grid_counts``: int64
    ``[G, 4]`` on the device (valid, class 0, class 1, class 2 per grid)."""
    labels: torch.Tensor
    difference: torch.Tensor
    noisy_depth: torch.Tensor
    uncertainty: Optional[torch.Tensor]
    mask: torch.Tensor
    grid_counts: torch.Tensor
    stats_block: torch.Tensor
    hw: np.ndarray
    res: np.ndarray
    offsets: np.ndarray
    paired: np.ndarray
    base_row: np.ndarray
    base_col: np.ndarray
    pairs: VRPairTable
    noise_threshold: float
    clean_survey: str = "None"
    noisy_survey: str = "None"
    _host_block: Any = None

    def __len__(self) -> int:
        return int(self.hw.shape[0])

    def block(self):
        """The statistics block on the host (``runtime.VT_STATS_DTYPE``).  The first call synchronises; later ones do not."""
        if self._host_block is None:
            raw = self.stats_block.cpu().numpy().tobytes()
            self._host_block = np.frombuffer(raw, dtype=np.dtype(rt.VT_STATS_DTYPE))[0]
        return self._host_block

    def stats(self) -> Dict[str, Any]:
        """The plan's ``*_ground_truth_stats.json`` dictionary without ``resampled_shape`` / ``resolution`` (GDAL's resampled view).
        ``mean_noise_magnitude`` is the float64 sum over the count; maximum and median are the plan's own values."""
        b = self.block()
        valid, noise, seafloor = int(b["valid"]), int(b["noise"]), int(b["seafloor"])
        out = {
            "clean_survey": str(self.clean_survey),
            "noisy_survey": str(self.noisy_survey),
            "noise_threshold": self.noise_threshold,
            "processing_mode": "native_vr",
            "base_shape": [int(v) for v in self.pairs.base_shape],
            "grids_processed": int(np.count_nonzero(self.paired)),
            "valid_cells": valid,
            "noise_cells": noise,
            "noise_percentage": float(100 * noise / max(1, valid)),
            "seafloor_cells": seafloor,
        }
        if noise > 0:
            out["mean_noise_magnitude"] = float(b["noise_abs_sum"]) / noise
            out["max_noise_magnitude"] = float(b["noise_abs_max"])
            out["median_noise_magnitude"] = float(b["noise_abs_median"])
        return out

    def labels_by_grid(self) -> Iterator[Tuple[Tuple[int, int], Dict[str, Any]]]:
        """``((base_row, base_col), {"labels", "difference", "resolution", "dimensions"})`` of every paired grid as host arrays,
        in the plan's order (row-major over the base grid, which both files share); ``resolution`` is the clean grid's, as there.
        One copy of the two planes to the host."""
        labels, diff = self.labels.cpu().numpy(), self.difference.cpu().numpy()
        for g in np.nonzero(self.paired)[0].tolist():
            a, b = int(self.offsets[g]), int(self.offsets[g + 1])
            shape = (int(self.hw[g, 0]), int(self.hw[g, 1]))
            yield (int(self.base_row[g]), int(self.base_col[g])), {
                "labels": labels[a:b].reshape(shape), "difference": diff[a:b].reshape(shape),
                "resolution": (float(self.pairs.clean_res[g, 0]), float(self.pairs.clean_res[g, 1])), "dimensions": shape}

    def evaluate(self, classification, confidence=None) -> Dict[str, Any]:
        """``compute_metrics``' dictionary of a classified noisy BAG against these labels.  ``classification`` / ``confidence``:
        host arrays or device tensors of one entry per record in this object's order -- rows 0 and 1 of what
        ``process_refinements(noisy_handler, return_results=True)`` returns."""
        from ..training.evaluation import Evaluator
        ev = Evaluator(self.labels.device)
        ev.add(self.labels, classification, confidence)
        return ev.metrics()


def compute_ground_truth_native(clean, noisy, noise_threshold: float = 0.15, device=None) -> NativeGroundTruth:
    """The plan's ``compute_ground_truth_native`` from two VR handlers (``VRBagHandler``, file- or array-backed), without the file
    I/O: ``vr_pair_table`` on the host, everything per cell on the device.  Nothing synchronises until ``stats()`` or a host
    accessor is called."""
    for name, h in (("clean", clean), ("noisy", noisy)):
        if isinstance(h, SRBagHandler) or not hasattr(h, "varres_metadata"):
            raise TypeError(f"{name}: compute_ground_truth_native takes VR BAG handlers; a single-resolution pair is a raster pair: "
                            "use compute_ground_truth")
    device = rt.resolve_device(device)
    pairs = vr_pair_table(clean, noisy)
    noisy_rec = _records_to_device(noisy, device)
    clean_rec = _records_to_device(clean, device)
    nodata = float(getattr(noisy, "NODATA", 1.0e6))
    labels, difference, depth, unc, mask, counts, stats = vr_ground_truth_build(noisy_rec, clean_rec, pairs.rows, pairs.total,
                                                                                noise_threshold, nodata)
    return NativeGroundTruth(labels, difference, depth, unc, mask, counts, stats, pairs.hw, pairs.res, pairs.offsets, pairs.paired,
                             pairs.base_row, pairs.base_col, pairs, noise_threshold,
                             str(getattr(clean, "path", None)), str(getattr(noisy, "path", None)))
