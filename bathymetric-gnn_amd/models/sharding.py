"""The ``torch.distributed`` side of the survey paths: who owns which tile rows, and the few tensors that cross GPUs.

The host-stitch path exchanges whole per-tile grids (``exchange_tile_results``); the device path shards the survey into row bands
(``survey_shard_plan``), hands the tile rows that straddle two bands over point to point (``exchange_halo_tile_rows``, with
``pack_halo_tile_row`` / ``unpack_halo_tile_row`` for the block that travels) and collects the stitched bands on rank 0
(``gather_bands_to_rank0``).  ``models.pipeline`` re-exports all of it.
"""
from __future__ import annotations

from typing import Dict, Optional

import numpy as np
import torch


def shard_info():
    """(rank, world_size) of the tile-parallel job: torch.distributed if initialised, else (0, 1)."""
    import torch.distributed as dist
    if dist.is_available() and dist.is_initialized():
        return dist.get_rank(), dist.get_world_size()
    return 0, 1


# Channel order of a packed tile-result block: ONE order on every rank, whether or not the rank holds tiles.
TILE_RESULT_CHANNELS = ("classification", "cleaned_depth", "confidence", "correction")


def exchange_tile_results(mine: dict) -> dict:
    """Union of every rank's {tile index: result dict} for the host-stitch path (every rank merges, so every rank needs
    every tile).  The grids travel as ONE float32 tensor per rank (``all_gather`` of [count, channels, h, w] blocks padded
    to the largest count; the tile indices as an int64 tensor) -- no pickling.  The data path itself (graph build,
    forward, scatter) has no collective.  For large surveys use the device path (row bands + halo rows), which moves
    ~0.5 GB per band boundary instead of every tile to every rank."""
    import torch.distributed as dist
    if not (dist.is_available() and dist.is_initialized()) or dist.get_world_size() == 1:
        return mine
    world = dist.get_world_size()
    dev = torch.device("cuda", torch.cuda.current_device()) if dist.get_backend() == "nccl" else torch.device("cpu")
    keys = []
    if mine:
        have = set(next(iter(mine.values())).keys())
        keys = [k for k in TILE_RESULT_CHANNELS if k in have] + sorted(have - set(TILE_RESULT_CHANNELS))
    shape = tuple(next(iter(mine.values()))[keys[0]].shape) if mine else (0, 0)
    # agree on (channel names are fixed by the caller) count, tile shape
    # (last entry: are this rank's channels the standard ones in the standard order?  A rank WITHOUT tiles can only unpack those.)
    std = int(keys == list(TILE_RESULT_CHANNELS)[:len(keys)])
    meta = torch.tensor([len(mine), len(keys), shape[0], shape[1], std], dtype=torch.int64, device=dev)
    metas = [torch.empty_like(meta) for _ in range(world)]
    dist.all_gather(metas, meta)
    metas = [m.cpu().numpy() for m in metas]
    nmax = int(max(m[0] for m in metas))
    nk, th, tw = (int(max(m[i] for m in metas)) for i in (1, 2, 3))
    if nmax == 0:
        return mine
    # Every check below reads only `metas`, which all ranks hold alike, and runs BEFORE the next collective: the ranks fail
    # together instead of one raising while the others wait in the block all_gather.
    if not all(m[0] == 0 or (m[1], m[2], m[3]) == (nk, th, tw) for m in metas):
        raise ValueError("exchange_tile_results: tiles of one survey share one shape and one channel count")
    if any(m[0] == 0 for m in metas) and (nk > len(TILE_RESULT_CHANNELS) or any(m[0] > 0 and m[4] == 0 for m in metas)):
        raise ValueError(f"exchange_tile_results: a rank without tiles can only unpack the standard channels {TILE_RESULT_CHANNELS} "
                         "in that order, and another rank packed something else")
    if not keys:                                           # this rank holds no tile: it still takes part in the collective,
        keys = list(TILE_RESULT_CHANNELS)[:nk]             # and unpacks in the same channel order the packing ranks used
    idx = torch.full((nmax,), -1, dtype=torch.int64)
    blk = torch.zeros((nmax, nk, th, tw), dtype=torch.float32)
    for j, (i, r) in enumerate(sorted(mine.items())):
        idx[j] = i
        for c, k in enumerate(keys):
            blk[j, c] = torch.from_numpy(np.ascontiguousarray(r[k], dtype=np.float32))
    idx, blk = idx.to(dev), blk.to(dev)
    idxs = [torch.empty_like(idx) for _ in range(world)]
    blks = [torch.empty_like(blk) for _ in range(world)]
    dist.all_gather(idxs, idx)
    dist.all_gather(blks, blk)
    out = {}
    for ii, bb in zip(idxs, blks):
        ii = ii.cpu().numpy(); bb = bb.cpu().numpy()
        for j, i in enumerate(ii):
            if i >= 0:
                out[int(i)] = {k: bb[j, c] for c, k in enumerate(keys)}
    return out


def gather_bands_to_rank0(plan, rank: int, band: Optional[torch.Tensor], width: int, channels: int = 4, device=None):
    """The sharded survey path's last step: every rank's stitched band [channels, rows, width] (float32) goes to rank 0 by
    point-to-point ``send`` / ``recv`` of the tensor itself (RCCL under ``nccl``; staged through the host under ``gloo``),
    one message per band -- not an all-gather of pickled arrays to everybody.  Rank 0 returns the assembled
    [channels, H, width] host array, the other ranks None."""
    import torch.distributed as dist
    via_host = dist.get_backend() == "gloo"
    H = max(p["cell_rows"][1] for p in plan)
    if rank != 0:
        R0, R1 = plan[rank]["cell_rows"]
        if R1 > R0:
            t = band.contiguous()
            dist.send(t.cpu() if via_host else t, dst=0)
        return None
    host = np.empty((channels, H, width), np.float32)
    R0, R1 = plan[0]["cell_rows"]
    if R1 > R0:
        host[:, R0:R1] = band.cpu().numpy()
    if via_host:
        recv_dev = torch.device("cpu")
    elif device is not None:
        recv_dev = torch.device(device)
    elif band is not None:
        recv_dev = band.device
    else:
        recv_dev = torch.device("cuda", torch.cuda.current_device())
    for k in range(1, len(plan)):
        R0, R1 = plan[k]["cell_rows"]
        if R1 == R0:
            continue
        buf = torch.empty((channels, R1 - R0, width), dtype=torch.float32, device=recv_dev)
        dist.recv(buf, src=k)
        host[:, R0:R1] = buf.cpu().numpy()
    return host


def survey_shard_plan(row_start, row_end, height: int, world: int):
    """Row-band ownership of a tiled survey over ``world`` GPUs (contiguous row bands localise the
    stitch).  Tile rows are split into contiguous blocks; rank k owns tile rows ``[a_k, b_k)`` and the survey cell
    rows ``[R_k, R_{k+1})`` with ``R_k = row_start[a_k]`` (``R_0 = 0``, ``R_world = height``).  The cells of a band
    are covered by the rank's own tile rows plus the earlier tile rows that reach into it (``row_end > R_k``):
    those are the only results that cross GPUs.  Returns a list of dicts
    ``{"tile_rows": (a, b), "cell_rows": (R0, R1), "need": [(src_rank, tile_row), ...]}``."""
    rs = np.asarray(row_start, np.int64); re = np.asarray(row_end, np.int64)
    ntr = len(rs)
    cuts = [int(x) for x in np.linspace(0, ntr, world + 1).round()]
    owner = np.empty(ntr, np.int64)
    for k in range(world):
        owner[cuts[k]:cuts[k + 1]] = k
    plan = []
    for k in range(world):
        a, b = cuts[k], cuts[k + 1]
        if a == b:                                     # more GPUs than tile rows: nothing to own
            plan.append({"tile_rows": (a, b), "cell_rows": (height, height), "need": []})
            continue
        R0 = 0 if a == 0 else int(rs[a])
        nxt = next((cuts[j] for j in range(k + 1, world) if cuts[j] < cuts[j + 1]), ntr)
        R1 = height if nxt >= ntr else int(rs[nxt])
        need = [(int(owner[t]), int(t)) for t in range(0, a) if re[t] > R0]
        plan.append({"tile_rows": (a, b), "cell_rows": (R0, R1), "need": need})
    return plan


def exchange_halo_tile_rows(plan, rank: int, local_rows: Dict[int, torch.Tensor]) -> Dict[int, torch.Tensor]:
    """Point-to-point exchange of the tile-row result blocks ``survey_shard_plan`` lists under ``need``: every rank
    sends each of its tile rows that a later band needs and receives the ones its own band needs.  ``local_rows``
    maps tile row -> tensor (all of one shape and dtype); returns {tile row: tensor} for the received rows.  This
    is the path's only inter-GPU traffic (RCCL send/recv over xGMI under the ``nccl`` backend; staged through the
    host under ``gloo``)."""
    import torch.distributed as dist
    if not plan[rank]["need"] and not any(src == rank for p in plan for src, _ in p["need"]):
        return {}
    via_host = dist.get_backend() == "gloo"
    ops, recv, keep = [], {}, []
    for dst, p in enumerate(plan):                       # same deterministic order on every rank
        for src, t in p["need"]:
            if src == rank and dst != rank:
                buf = local_rows[t].contiguous()
                buf = buf.cpu() if via_host else buf
                keep.append(buf)
                ops.append(dist.P2POp(dist.isend, buf, dst, tag=t))
            elif dst == rank and src != rank:
                shape, dtype, dev = plan[rank]["_halo_shape"], plan[rank]["_halo_dtype"], plan[rank]["_halo_device"]
                buf = torch.empty(shape, dtype=dtype, device="cpu" if via_host else dev)
                recv[t] = buf
                ops.append(dist.P2POp(dist.irecv, buf, src, tag=t))
    if ops:
        for w in dist.batch_isend_irecv(ops):
            w.wait()
    if via_host:
        recv = {t: b.to(plan[rank]["_halo_device"]) for t, b in recv.items()}
    return recv


def pack_halo_tile_row(results, row_off: np.ndarray, cells: int) -> torch.Tensor:
    """One tile row's results as the block that travels: ``[3][ntc][cells]`` (classification, confidence, correction; zeros for a
    skipped tile) followed by ``ntc`` keep flags.  ``row_off``: the row's offsets into the three ``results`` arrays, -1 for a skipped
    tile; the kept tiles of a row hold consecutive slots."""
    ntc = len(row_off)
    blk = 3 * ntc * cells
    kept = np.nonzero(row_off >= 0)[0]
    dev = results[0].device
    buf = torch.zeros(blk + ntc, dtype=torch.float32, device=dev)
    if len(kept):
        cols = torch.from_numpy(kept).to(dev)
        p0 = int(row_off[kept[0]]); p1 = p0 + len(kept) * cells
        for c, r in enumerate(results):
            buf[c * ntc * cells:(c + 1) * ntc * cells].view(ntc, cells)[cols] = r[p0:p1].view(len(kept), cells)
        buf[blk + cols] = 1.0
    return buf


def unpack_halo_tile_row(buf: torch.Tensor, results, base: int, ntc: int, cells: int) -> np.ndarray:
    """Inverse of ``pack_halo_tile_row``: the block's ``ntc`` tiles go into ``results`` from offset ``base`` on; returns the row's
    offsets (-1 where the sender had skipped the tile)."""
    blk = 3 * ntc * cells
    for c, r in enumerate(results):
        r[base:base + ntc * cells] = buf[c * ntc * cells:(c + 1) * ntc * cells]
    kp = buf[blk:].cpu().numpy() > 0
    row_off = np.full(ntc, -1, np.int64)
    row_off[kp] = base + np.nonzero(kp)[0].astype(np.int64) * cells
    return row_off
