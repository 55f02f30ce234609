"""The survey routes of ``BathymetricPipeline``: one tile plan, one classify step, one stitch step.

``SurveyTilePlan`` is the geometry of a tiled survey as a host object (numpy only: no device, no library).  ``SurveySteps`` holds the
two device steps -- cut + classify a list of tiles into result slots, stitch a band of survey rows -- that both routes run:
``survey_resident`` (survey in HBM, one GPU or one rank's row band; ``BathymetricPipeline.process_survey_device``) and
``survey_streamed`` (host survey, upload / classify / stitch / download overlapped; ``BathymetricPipeline.process_grid_streamed``).
The streamed route is bit-identical to the resident one because it calls the same two steps with the same plan.
"""
from __future__ import annotations

import ctypes as C
import queue
import threading
from typing import Dict, List, Tuple

import numpy as np
import torch

from .. import runtime as rt
from .sharding import exchange_halo_tile_rows, pack_halo_tile_row, survey_shard_plan, unpack_halo_tile_row

RESULT_ORDER = ("classification", "confidence", "correction", "cleaned_depth", "valid_mask")


def keep_from_counts(counts, cells: int, min_valid_ratio: float) -> np.ndarray:
    """The ``min_valid_ratio`` rule from exact per-tile valid counts: True for a tile that is processed.  It is the float64 test of
    ``TileManager.iterate_tiles`` (``tile.valid_ratio < min_valid_ratio`` skips, with ``valid_ratio = sum / size``), negated the same
    way, so the device routes keep exactly the tiles the host merge keeps."""
    return ~((np.asarray(counts, np.int64) / cells) < min_valid_ratio)


class SurveyTilePlan:
    """Tile lattice of a survey of ``shape`` under ``tile_manager``: ``ntr x ntc`` tiles of one extent ``th x tw`` (``cells`` each),
    tile row t spanning survey rows ``[rs[t], re[t])``, tile column j spanning ``[cs[j], ce[j])`` (int64), ``origins`` the int32
    ``[ntr * ntc, 2]`` table of (row, column) starts in spec order, ``pitch`` the row length of the blend tables."""

    def __init__(self, tile_manager, shape):
        self.H, self.W = (int(v) for v in shape)
        self.ntr, self.ntc, specs = tile_manager.compute_tile_grid((self.H, self.W))
        sa = np.array([[s.row_start, s.col_start, s.row_end, s.col_end] for s in specs], np.int64)
        self.th, self.tw = int(sa[0, 2] - sa[0, 0]), int(sa[0, 3] - sa[0, 1])
        if np.any(sa[:, 2] - sa[:, 0] != self.th) or np.any(sa[:, 3] - sa[:, 1] != self.tw):     # (the shift-back rule gives one extent)
            raise ValueError(f"the tiles of a {self.H} x {self.W} survey differ in extent: the survey routes take one tile shape")
        self.cells = self.th * self.tw
        self.pitch = max(self.th, self.tw)
        ntc = self.ntc
        self.rs, self.re = sa[::ntc, 0].copy(), sa[::ntc, 2].copy()
        self.cs, self.ce = sa[:ntc, 1].copy(), sa[:ntc, 3].copy()
        self.origins = np.ascontiguousarray(sa[:, :2], dtype=np.int32)
        self._blend = tile_manager._create_1d_blend

    def _padded(self, size: int, n: int) -> np.ndarray:
        w = np.zeros((n, self.pitch), np.float32)
        w[:, :size] = self._blend(size)
        return w

    @property
    def col_weights(self) -> np.ndarray:
        """``[ntc, pitch]``: ``TileManager._create_1d_blend`` of every tile column, zero beyond ``tw``."""
        return self._padded(self.tw, self.ntc)

    def row_weights(self, tile_rows) -> np.ndarray:
        """``[len(tile_rows), pitch]``: the same for the given tile rows."""
        return self._padded(self.th, len(tile_rows))

    def rows_touching(self, R0: int, R1: int) -> np.ndarray:
        """Tile rows (ascending) that cover some survey row of ``[R0, R1)``."""
        return np.nonzero((self.rs < R1) & (self.re > R0))[0]

    @property
    def reach(self) -> int:
        """The most earlier tile rows that end past the first survey row of any tile row."""
        return max(int(np.count_nonzero(self.re[:t] > self.rs[t])) for t in range(self.ntr))

    def ring_slots(self, band_tile_rows: int) -> int:
        """Tile rows whose results a band-wise stitch can still read: the band's own and those that reach into it."""
        return min(self.ntr, band_tile_rows + self.reach)

    def bands(self, band_tile_rows: int) -> List[Tuple[Tuple[int, int], Tuple[int, int]]]:
        """``[((ta, tb), (R0, R1)), ...]``: tile rows taken ``band_tile_rows`` at a time, each with the survey rows that are final
        once they are classified (no later tile row touches them).  The row ranges partition ``[0, H)`` in order."""
        out, R0 = [], 0
        for ta in range(0, self.ntr, band_tile_rows):
            tb = min(ta + band_tile_rows, self.ntr)
            R1 = max(int(self.rs[tb]) if tb < self.ntr else self.H, R0)
            out.append(((ta, tb), (R0, R1)))
            R0 = R1
        return out

    def stitch_tables(self, tile_rows, R0: int):
        """What one stitch of survey rows from ``R0`` on takes for ``tile_rows``: their int32 row starts and ends relative to
        ``R0``, and their blend weights."""
        tile_rows = np.asarray(tile_rows, np.int64)
        return (self.rs[tile_rows] - R0).astype(np.int32), (self.re[tile_rows] - R0).astype(np.int32), self.row_weights(tile_rows)

    def shard_plan(self, world: int):
        return survey_shard_plan(self.rs, self.re, self.H, world)


class TileScratch:
    """Cut tiles of one batch (flat device planes) and the per-tile shape / resolution tables that go with them."""

    def __init__(self, dev, n_tiles: int, plan: SurveyTilePlan, resol: np.ndarray, with_unc: bool, with_density: bool):
        mk = lambda dt: torch.empty(n_tiles * plan.cells, dtype=dt, device=dev)
        self.depth, self.mask = mk(torch.float32), mk(torch.uint8)
        self.unc = mk(torch.float32) if with_unc else None
        self.density = mk(torch.float32) if with_density else None
        self.hw = np.tile(np.array([[plan.th, plan.tw]], np.int32), (n_tiles, 1))
        self.res = np.tile(resol, (n_tiles, 1))


class SurveySteps:
    """The device steps both survey routes share, for one route call: ``classify`` and ``stitch`` on ``engine``'s context."""

    def __init__(self, engine, plan: SurveyTilePlan, resolution, tile_batch: int, threshold: float):
        self.eng, self.ctx, self.dev = engine, engine.ctx, engine.ctx.device
        self.plan, self.tile_batch, self.threshold = plan, tile_batch, threshold
        self.resol = np.array([[float(resolution[0]), float(resolution[1])]], np.float64)
        self._columns = None

    def to_device(self, a: np.ndarray) -> torch.Tensor:
        return torch.from_numpy(np.ascontiguousarray(a)).to(self.dev)

    def scratch(self, n_tiles: int, with_unc: bool, with_density: bool = False) -> TileScratch:
        return TileScratch(self.dev, n_tiles, self.plan, self.resol, with_unc, with_density)

    def column_tables(self):
        """(column starts, column ends, column blend weights) on the device; uploaded once per route call."""
        if self._columns is None:
            p = self.plan
            self._columns = (self.to_device(p.cs.astype(np.int32)), self.to_device(p.ce.astype(np.int32)), self.to_device(p.col_weights))
        return self._columns

    def classify(self, depth_t, valid_u8, unc_t, density_t, org_t, idx_t, results, slot0: int, s: TileScratch):
        """Cut the tiles ``org_t[idx_t]`` out of the planes (``depth_t.shape`` rows held, origins in those rows) and classify them,
        ``tile_batch`` at a time, into the slots ``slot0, slot0 + 1, ...`` of the three ``results`` arrays.  ``density_t``: a second
        cut with the plane in the uncertainty slot (depth and mask: the same values again) gives the density windows."""
        p, ctx = self.plan, self.ctx
        rows, W = (int(v) for v in depth_t.shape)
        for b0 in range(0, len(idx_t), self.tile_batch):
            nb = min(self.tile_batch, len(idx_t) - b0)
            o_b = org_t[idx_t[b0:b0 + nb]].contiguous()
            ctx.begin()
            rt.check(ctx.lib.bgnn_cut_tiles(ctx.handle, rows, W, rt.ptr(depth_t), rt.ptr(valid_u8), rt.ptr(unc_t), nb, rt.ptr(o_b),
                                            p.th, p.tw, rt.ptr(s.depth), rt.ptr(s.mask), rt.ptr(s.unc)))
            if density_t is not None:
                rt.check(ctx.lib.bgnn_cut_tiles(ctx.handle, rows, W, rt.ptr(depth_t), rt.ptr(valid_u8), rt.ptr(density_t), nb,
                                                rt.ptr(o_b), p.th, p.tw, rt.ptr(s.depth), rt.ptr(s.mask), rt.ptr(s.density)))
            ctx.end()
            lo = (slot0 + b0) * p.cells; hi = lo + nb * p.cells; n = nb * p.cells
            self.eng.infer_device(s.hw[:nb], s.res[:nb], s.depth[:n], s.mask[:n], s.unc[:n] if s.unc is not None else None,
                                  out=tuple(r[lo:hi] for r in results),
                                  density_t=s.density[:n] if density_t is not None else None)

    def stitch(self, tile_rows, tile_off, R0: int, R1: int, results, depth_rows, valid_rows, out):
        """Stitch survey rows ``[R0, R1)`` from ``tile_rows`` (ascending; ``tile_off``: their tiles' offsets into ``results``, -1 for
        a skipped tile) into ``out[0..3]`` (classification, confidence, correction, cleaned depth).  ``depth_rows`` / ``valid_rows``:
        those rows of the survey."""
        p, ctx = self.plan, self.ctx
        rs_b, re_b, roww = p.stitch_tables(tile_rows, R0)
        rs_t, re_t = self.to_device(rs_b), self.to_device(re_b)
        cs_t, ce_t, cw_t = self.column_tables()
        rw_t, off_t = self.to_device(roww), self.to_device(tile_off)
        ctx.begin()
        rt.check(ctx.lib.bgnn_stitch_tiles(
            ctx.handle, R1 - R0, p.W, len(tile_rows), p.ntc, rt.ptr(rs_t), rt.ptr(re_t), rt.ptr(cs_t), rt.ptr(ce_t), rt.ptr(rw_t),
            rt.ptr(cw_t), p.pitch, rt.ptr(off_t), rt.ptr(results[0]), rt.ptr(results[1]), rt.ptr(results[2]),
            rt.ptr(depth_rows), rt.ptr(valid_rows), C.c_float(self.threshold),
            rt.ptr(out[0]), rt.ptr(out[1]), rt.ptr(out[2]), rt.ptr(out[3])))
        ctx.end()


# ---- survey resident in HBM (one GPU, or one rank's row band) ---------------------------------------------------------------
def survey_resident(steps: SurveySteps, min_valid_ratio: float, depth_t, valid_u8, unc_t, density_t,
                    shard: Tuple[int, int], row_offset: int):
    """Body of ``process_survey_device`` (see there): the planes hold survey rows ``[row_offset, row_offset + depth_t.shape[0])``.
    Returns ``(R0, R1, [4, R1 - R0, W] tensor, (tiles processed, tiles skipped))``."""
    p, ctx, dev = steps.plan, steps.ctx, steps.dev
    ntc, cells = p.ntc, p.cells
    LH = int(depth_t.shape[0])
    rank, world = shard
    plan = p.shard_plan(world)
    me = plan[rank]
    ta, tb = me["tile_rows"]; R0, R1 = me["cell_rows"]
    own = np.arange(ta * ntc, tb * ntc)                              # my tiles, ascending spec order
    if len(own) and not (p.rs[ta] >= row_offset and p.re[tb - 1] <= row_offset + LH):
        raise ValueError("the local rows do not cover this rank's tile rows")
    if not (R0 == R1 or (R0 >= row_offset and R1 <= row_offset + LH)):
        raise ValueError("the local rows do not cover this rank's band of survey rows")
    # ---- min_valid_ratio filter, exact integer counts ----
    keep = np.zeros(0, bool)
    if len(own):
        org = p.origins[own].copy()
        org[:, 0] -= row_offset                                      # origins in local rows
        org_t = steps.to_device(org)
        cnt_t = torch.empty(len(own), dtype=torch.int64, device=dev)
        ctx.begin()
        rt.check(ctx.lib.bgnn_tile_valid_counts(ctx.handle, LH, p.W, rt.ptr(valid_u8), len(own), rt.ptr(org_t), p.th, p.tw, rt.ptr(cnt_t)))
        ctx.end()
        keep = keep_from_counts(cnt_t.cpu().numpy(), cells, min_valid_ratio)
    proc = np.nonzero(keep)[0]                                       # positions in `own`
    n_proc = len(proc)
    halo_rows = [t for _, t in me["need"]]
    total = max(n_proc + len(halo_rows) * ntc, 1) * cells
    results = tuple(torch.empty(total, dtype=torch.float32, device=dev) for _ in range(3))     # classification, confidence, correction
    if n_proc:
        scratch = steps.scratch(min(steps.tile_batch, n_proc), unc_t is not None, density_t is not None)
        steps.classify(depth_t, valid_u8, unc_t, density_t, org_t, steps.to_device(proc), results, 0, scratch)
        del scratch
    off_own = np.full(len(own), -1, np.int64)                        # result offsets of my own tiles, by (tile row, tile col)
    off_own[proc] = np.arange(n_proc, dtype=np.int64) * cells
    # ---- the only inter-GPU step: earlier tile rows that reach into my band ----
    off_halo = np.full((len(halo_rows), ntc), -1, np.int64)
    if world > 1:
        for q in plan:
            q["_halo_shape"], q["_halo_dtype"], q["_halo_device"] = (3 * ntc * cells + ntc,), torch.float32, dev
        wanted = sorted({t for q in plan for src, t in q["need"] if src == rank})
        local = {t: pack_halo_tile_row(results, off_own[(t - ta) * ntc:(t - ta + 1) * ntc], cells) for t in wanted}
        torch.cuda.synchronize(dev)
        got = exchange_halo_tile_rows(plan, rank, local)
        for j, t in enumerate(halo_rows):
            off_halo[j] = unpack_halo_tile_row(got[t], results, (n_proc + j * ntc) * cells, ntc, cells)
    # ---- stitch my band: tile rows involved = halo rows (earlier, ascending) then my own ----
    o = torch.empty((4, R1 - R0, p.W), dtype=torch.float32, device=dev)
    if R1 > R0:
        steps.stitch(np.array(halo_rows + list(range(ta, tb)), np.int64), np.concatenate([off_halo.reshape(-1), off_own]), R0, R1,
                     results, depth_t[R0 - row_offset:R1 - row_offset], valid_u8[R0 - row_offset:R1 - row_offset], o)
    return R0, R1, o, (n_proc, len(own) - n_proc)


# ---- host survey, streamed (one GPU) ----------------------------------------------------------------------------------------
class StreamResources:
    """What the streamed route keeps between calls: its pinned slabs (page-locking ~1 GB costs ~0.3 s), for surveys of one geometry
    -- another geometry starts afresh --, and the upload thread's library context (calls on one context are not re-entrant, so
    the thread has its own; its stream is the upload stream)."""

    def __init__(self):
        self.pins: Dict = {}
        self.sig = None
        self.ctx = None
        self._taken: Dict = {}

    def start_call(self, sig):
        if self.sig != sig:
            self.pins.clear()
            self.sig = sig
        self._taken = {}

    def pin(self, dt, *shape) -> torch.Tensor:
        lst = self.pins.setdefault((dt, shape), [])
        i = self._taken[(dt, shape)] = self._taken.get((dt, shape), -1) + 1
        while len(lst) <= i:
            lst.append(torch.empty(shape, dtype=dt, pin_memory=True))
        return lst[i]

    def upload_ctx(self, dev):
        if self.ctx is None or self.ctx.handle is None:
            self.ctx = rt.new_context(dev)
        return self.ctx


class TileRowState:
    """What the three roles of the streamed route share: per tile row, the keep flags of its tiles (published by the uploader) and
    the event behind which its survey rows and mask are resident; and the first error of a thread, for the caller's thread."""

    def __init__(self, ntr: int):
        self.cv = threading.Condition()
        self.keep_rows: Dict[int, np.ndarray] = {}
        self.row_ready = [torch.cuda.Event() for _ in range(ntr)]
        self.errors: List[BaseException] = []

    def publish(self, t0: int, t1: int, keep: np.ndarray, ntc: int):
        with self.cv:
            for t in range(t0, t1):
                self.keep_rows[t] = keep[(t - t0) * ntc:(t - t0 + 1) * ntc]
            self.cv.notify_all()

    def fail(self, e: BaseException):
        with self.cv:
            self.errors.append(e); self.cv.notify_all()

    def check(self):
        with self.cv:
            if self.errors:
                raise self.errors[0]

    def wait_for(self, ta: int, tb: int):
        """Until the keep flags of tile rows ``[ta, tb)`` are published; raises a thread's error instead."""
        with self.cv:
            while not self.errors and any(t not in self.keep_rows for t in range(ta, tb)):
                self.cv.wait(0.05)
            if self.errors:
                raise self.errors[0]


class SurveyUploader:
    """UPLOAD role: copies the host survey into pinned slabs and H2D's it chunk by chunk on the upload context's stream; makes the
    valid mask on the device (or uploads a foreign grid's own); and as soon as a tile row's rows are resident takes its tiles' valid
    counts and publishes the keep flags -- the ``min_valid_ratio`` filter never makes the classifying stream wait for the host."""

    def __init__(self, state: TileRowState, plan: SurveyTilePlan, up_ctx, min_valid_ratio: float, up_rows: int, host, device, slabs,
                 org_t):
        self.state, self.plan, self.up_ctx, self.min_valid_ratio, self.up_rows = state, plan, up_ctx, min_valid_ratio, up_rows
        self.depth_h, self.unc_h, self.valid_h, self.nodata = host
        self.depth_t, self.unc_t, self.valid_t = device
        self.pin_d, self.pin_u, self.pin_m = slabs                  # two pinned slabs each (None: plane not uploaded)
        self.org_t = org_t

    def run(self):
        try:
            self._upload()
        except BaseException as e:                                   # noqa: BLE001 -- handed to the caller's thread
            self.state.fail(e)

    def _upload(self):
        p, up_ctx, up_stream = self.plan, self.up_ctx, self.up_ctx.stream
        H, W, ntr, ntc = p.H, p.W, p.ntr, p.ntc
        depth_t, unc_t, valid_t, nodata = self.depth_t, self.unc_t, self.valid_t, self.nodata
        done_rows, next_t, slot_ev = 0, 0, [None, None]
        with torch.cuda.stream(up_stream):
            k = 0
            while done_rows < H:
                r0, r1 = done_rows, min(H, done_rows + self.up_rows)
                j = k % 2
                if slot_ev[j] is not None:
                    slot_ev[j].synchronize()               # the slab's previous H2D has left it
                n = r1 - r0
                np.copyto(self.pin_d[j].numpy()[:n], self.depth_h[r0:r1])
                depth_t[r0:r1].copy_(self.pin_d[j][:n], non_blocking=True)
                if self.unc_h is not None:
                    np.copyto(self.pin_u[j].numpy()[:n], self.unc_h[r0:r1])
                    unc_t[r0:r1].copy_(self.pin_u[j][:n], non_blocking=True)
                if self.valid_h is not None:
                    np.copyto(self.pin_m[j].numpy()[:n], self.valid_h[r0:r1])
                    valid_t[r0:r1].copy_(self.pin_m[j][:n], non_blocking=True)
                else:                                      # BathymetricGrid.valid_mask on the device
                    d = depth_t[r0:r1]
                    m = torch.isfinite(d)
                    if nodata is not None and not np.isnan(nodata):
                        m &= d != nodata
                    valid_t[r0:r1].copy_(m)
                slot_ev[j] = torch.cuda.Event(); slot_ev[j].record(up_stream)
                done_rows, k = r1, k + 1
                # tile rows whose rows are now all resident: valid counts -> min_valid_ratio filter
                t0 = next_t
                while next_t < ntr and p.re[next_t] <= done_rows:
                    next_t += 1
                if next_t > t0:
                    n_t = (next_t - t0) * ntc
                    cnt_t = torch.empty(n_t, dtype=torch.int64, device=depth_t.device)
                    rt.check(up_ctx.lib.bgnn_tile_valid_counts(up_ctx.handle, H, W, rt.ptr(valid_t), n_t,
                                                               rt.ptr(self.org_t[t0 * ntc:next_t * ntc]), p.th, p.tw, rt.ptr(cnt_t)))
                    for t in range(t0, next_t):
                        self.state.row_ready[t].record(up_stream)
                    keep = keep_from_counts(cnt_t.cpu().numpy(), p.cells, self.min_valid_ratio)      # (syncs the upload stream only)
                    self.state.publish(t0, next_t, keep, ntc)


class SurveyDownloader:
    """DOWNLOAD role: ``submit`` queues a stitched band's D2H into one of two pinned slabs on the download stream; the thread
    (``run``) waits for it and copies it into the five result arrays -- fresh pageable memory, whose first touch costs as much as the
    copy itself, so that runs beside the kernels too."""

    def __init__(self, state: TileRowState, dev, o_pin, out: Dict[str, np.ndarray]):
        self.state, self.dev, self.o_pin, self.out = state, dev, o_pin, out
        self.stream = torch.cuda.Stream(dev)
        self.q: "queue.Queue" = queue.Queue()
        self.slot_free = [threading.Event(), threading.Event()]
        for e in self.slot_free:
            e.set()
        self.band_done = [None, None]                                # D2H events of the band that last used each device / pinned slot

    def run(self):
        try:
            while True:
                item = self.q.get()
                if item is None:
                    return
                j, r0, r1, ev = item
                ev.synchronize()
                src = self.o_pin[j].numpy()
                for c, name in enumerate(RESULT_ORDER):
                    np.copyto(self.out[name][r0:r1], src[c, :r1 - r0])
                self.slot_free[j].set()
        except BaseException as e:                                   # noqa: BLE001
            self.state.fail(e)
            for e2 in self.slot_free:
                e2.set()

    def wait_device_slot(self, j: int):
        if self.band_done[j] is not None:
            torch.cuda.current_stream(self.dev).wait_event(self.band_done[j])      # the device slab's last download has left it

    def submit(self, j: int, o: torch.Tensor, R0: int, R1: int):
        """Queue the download of ``o[:, :R1 - R0]`` (written on the current stream) as survey rows ``[R0, R1)``."""
        n_r = R1 - R0
        stitched = torch.cuda.Event(); stitched.record(torch.cuda.current_stream(self.dev))
        self.slot_free[j].wait()                                     # the pinned slab's last band has been copied out
        self.state.check()
        self.slot_free[j].clear()
        with torch.cuda.stream(self.stream):
            self.stream.wait_event(stitched)
            for c in range(5):                                       # (contiguous blocks: a strided copy would go through a host-side temporary)
                self.o_pin[j][c, :n_r].copy_(o[c, :n_r], non_blocking=True)
            ev = torch.cuda.Event(); ev.record(self.stream)
        self.band_done[j] = ev
        self.q.put((j, R0, R1, ev))

    def finish(self):
        self.q.put(None)


def survey_streamed(steps: SurveySteps, res: StreamResources, min_valid_ratio: float, depth_h, valid_h, nodata, unc_h,
                    band_tile_rows: int, upload_rows_bytes: int):
    """Body of ``process_grid_streamed`` (see there).  ``valid_h`` None: the mask is made on the device from the depth and
    ``nodata``.  Returns ``(result dict of host arrays, (tiles processed, tiles skipped))``."""
    p, ctx, dev = steps.plan, steps.ctx, steps.dev
    H, W, ntr, ntc, cells = p.H, p.W, p.ntr, p.ntc, p.cells
    use_unc = unc_h is not None
    nb = band_tile_rows
    K = p.ring_slots(nb)                                           # ring slots (tile rows)
    bands = p.bands(nb)
    max_rows = max(r1 - r0 for _, (r0, r1) in bands)
    # ---- device / pinned buffers ----
    mk = lambda dt, *shape: torch.empty(shape, dtype=dt, device=dev)
    res.start_call((H, W, p.th, p.tw, nb, use_unc, valid_h is None))
    depth_t, valid_t = mk(torch.float32, H, W), mk(torch.uint8, H, W)
    unc_t = mk(torch.float32, H, W) if use_unc else None
    r_all = mk(torch.float32, 3, K * ntc * cells)                 # ring: [channel][slot][tile][cells]
    results = (r_all[0], r_all[1], r_all[2])
    o_dev = [mk(torch.float32, 5, max_rows, W) for _ in range(2)]
    o_pin = [res.pin(torch.float32, 5, max_rows, W) for _ in range(2)]
    up_rows = max(1, min(H, upload_rows_bytes // (4 * W)))
    up_pin = [res.pin(torch.float32, up_rows, W) for _ in range(2)]
    up_pin_u = [res.pin(torch.float32, up_rows, W) for _ in range(2)] if use_unc else None
    up_pin_m = [res.pin(torch.uint8, up_rows, W) for _ in range(2)] if valid_h is not None else None
    torch.cuda.synchronize(dev)                                   # (buffers made on this stream, used on three others)
    up_ctx = res.upload_ctx(dev)
    out = {k: np.empty((H, W), np.float32) for k in RESULT_ORDER}
    state = TileRowState(ntr)
    org_t = torch.from_numpy(p.origins).to(dev)
    up = SurveyUploader(state, p, up_ctx, min_valid_ratio, up_rows, (depth_h, unc_h, valid_h, nodata), (depth_t, unc_t, valid_t),
                        (up_pin, up_pin_u, up_pin_m), org_t)
    down = SurveyDownloader(state, dev, o_pin, out)
    t_up = threading.Thread(target=up.run, name="bgnn-survey-up", daemon=True)
    t_dn = threading.Thread(target=down.run, name="bgnn-survey-down", daemon=True)
    t_up.start(); t_dn.start()
    steps.column_tables()
    tile_off = np.full((ntr, ntc), -1, np.int64)
    scratch = steps.scratch(min(steps.tile_batch, ntc), use_unc)
    n_proc = 0
    try:
        for bi, ((ta, tb), (R0, R1)) in enumerate(bands):
            state.wait_for(ta, tb)
            for t in range(ta, tb):
                kept = np.nonzero(state.keep_rows[t])[0]
                slot = t % K
                tile_off[t, :] = -1
                tile_off[t, kept] = (slot * ntc + np.arange(len(kept), dtype=np.int64)) * cells
                if not len(kept):
                    continue
                n_proc += len(kept)
                ctx.stream.wait_event(state.row_ready[t])
                steps.classify(depth_t, valid_t, unc_t, None, org_t, steps.to_device(t * ntc + kept), results, slot * ntc, scratch)
            if R1 <= R0:
                continue
            # ---- stitch the rows that are final now, with the tile rows that reach into them ----
            inv = p.rows_touching(R0, R1)
            if not (inv.max() < tb and inv.min() > tb - 1 - K):
                raise RuntimeError("a stitch only reads tile rows still in the ring")
            j = bi % 2
            down.wait_device_slot(j)
            o = o_dev[j]
            steps.stitch(inv, tile_off[inv].reshape(-1), R0, R1, results, depth_t[R0:R1], valid_t[R0:R1], o)
            # (the four stitched grids are [n_r][W] blocks at the head of their [max_rows][W] planes; the mask as float32 beside them)
            o[4, :R1 - R0].copy_(valid_t[R0:R1])
            down.submit(j, o, R0, R1)
    finally:
        down.finish()
        t_up.join(); t_dn.join()
        torch.cuda.synchronize(dev)
    state.check()
    return out, (n_proc, ntr * ntc - n_proc)
