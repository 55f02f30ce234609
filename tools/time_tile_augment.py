#!/usr/bin/env python3
"""The tile gather under the symmetries of the square (include/bgnn_augment.h) against torch's way to assemble a step's planes.

    python tools/time_tile_augment.py                 # both cases, 30 repetitions after 5 warm-up rounds
    python tools/time_tile_augment.py --what ragged --reps 50

Two seeded ground-truth stores (five planes: depth, uncertainty, labels, difference as 4-byte words, the mask as bytes):

  uniform   64 tiles of 512 x 512; a batch is four of them (every repetition takes the next four, so that the 285 MB store, not
            one batch kept in the Infinity Cache, is what is read)
  ragged    6000 tiles of 3 x 3 to 50 x 50 cells (refinement grids); a batch is 2000 of them (the next 2000 every repetition)

and per case

  call      ``bgnn_tile_gather`` alone into buffers allocated beforehand (the table's upload through the pinned staging included),
            with all-identity ops and with all-90-degree ops; from its bytes -- 2 x (4 x 4 + 1) per cell, read plus written, and 32
            per entry -- the rate and the share of the 8.0 TB/s HBM peak
  gather    ``TileStore.gather`` (the same call behind the allocation of the outputs and the workspace), identity and 90 degrees
  torch     the transform restated with torch: ``rot90`` of every tile's view, ``cat`` per plane (90 degrees)

Every figure: the median (and minimum) over ``--reps`` of HIP events on the caller's stream around one call, behind a matrix product
that keeps the device busy while the host enqueues, and the median of a host clock around the call and a device synchronise (which
is what a training step waits for when the host is the bottleneck).  The results of the two ways are compared as bits first.

The events around a call include the table's upload and the hand-over between the caller's stream and the context's.  For the
kernel alone, run ``--kernel-only OP --what CASE`` under ``rocprofv3 --kernel-trace --stats``: it launches the gather ``--reps``
times and prints the bytes of one launch, to set against the trace's average duration of ``tile_gather``."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_PEAK = 8.0e12
NAMES = ("depth", "unc", "labels", "difference", "mask")


def make_store(torch, hw, device, seed):
    import numpy as np
    from bathymetric_gnn_amd.training import TileStore
    g = torch.Generator(device=device).manual_seed(seed)
    cells = int((hw[:, 0].astype(np.int64) * hw[:, 1]).sum())
    labels = (torch.rand(cells, generator=g, device=device) * 4).to(torch.int32) - 1
    return TileStore("ground_truth", hw, np.ones((len(hw), 2)), -30 + 5 * torch.randn(cells, generator=g, device=device),
                     (labels >= 0).view(torch.uint8), torch.rand(cells, generator=g, device=device), labels=labels,
                     difference=torch.randn(cells, generator=g, device=device), device=device)


def measure(torch, fn, reps, warmup):
    """``fn(rep)`` timed ``reps`` times after ``warmup`` rounds: events on the current stream behind a busy device, and a host clock."""
    busy = torch.randn(4096, 4096, device="cuda")
    sink = torch.empty_like(busy)
    for r in range(warmup):
        fn(r)
    torch.cuda.synchronize()
    ev, wall = [], []
    for r in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.mm(busy, busy, out=sink)
        a.record()
        fn(warmup + r)
        b.record()
        b.synchronize()
        ev.append(a.elapsed_time(b) * 1e3)
    for r in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn(warmup + r)
        torch.cuda.synchronize()
        wall.append((time.perf_counter() - t0) * 1e6)
    return {"device_us_median": round(statistics.median(ev), 2), "device_us_min": round(min(ev), 2),
            "host_us_median": round(statistics.median(wall), 1)}


def raw_call(rt, ctx, store, idx, ops, out, ws):
    import numpy as np
    table = np.zeros(len(idx), dtype=rt.TILE_ENTRY_DTYPE)
    cells = store.offsets[idx + 1] - store.offsets[idx]
    table["src"], table["dst"] = store.offsets[idx], np.cumsum(cells) - cells
    table["h"], table["w"], table["op"] = store.hw[idx, 0], store.hw[idx, 1], ops
    words = [store.depth, store.unc, store.labels, store.difference]
    src = (C.c_void_p * 4)(*[t.data_ptr() for t in words])
    dst = (C.c_void_p * 4)(*[out[k].data_ptr() for k in NAMES[:4]])
    ctx.begin()
    rt.check(ctx.lib.bgnn_tile_gather(ctx.handle, src, dst, 4, rt.ptr(store.mask), rt.ptr(out["mask"]), int(store.offsets[-1]),
                                      int(cells.sum()), C.c_void_p(table.ctypes.data), len(idx), rt.ptr(ws), C.c_size_t(ws.numel() * 8)))
    ctx.end()


def torch_turn(torch, store, idx, ops):
    planes = {k: getattr(store, k) for k in NAMES}
    out = {k: [] for k in NAMES}
    for i, op in zip(idx.tolist(), ops.tolist()):
        a, b, (h, w) = int(store.offsets[i]), int(store.offsets[i + 1]), store.hw[i]
        for k, p in planes.items():
            t = p[a:b].view(int(h), int(w))
            out[k].append(torch.rot90(torch.flip(t, (1,)) if op >> 2 else t, op & 3).reshape(-1))
    return {k: torch.cat(v) for k, v in out.items()}


def same(torch, a, b):
    return all(torch.equal(a[k].view(torch.int32) if a[k].dtype == torch.float32 else a[k],
                           b[k].view(torch.int32) if b[k].dtype == torch.float32 else b[k]) for k in NAMES)


def run_case(args, what):
    import numpy as np
    import torch
    from bathymetric_gnn_amd import runtime as rt
    dev = torch.device("cuda:0")
    ctx = rt.get_context(dev)
    rng = np.random.default_rng(5)
    if what == "uniform":
        hw, batch = np.full((64, 2), 512, np.int32), 4
    else:
        hw, batch = rng.integers(3, 51, size=(6000, 2)).astype(np.int32), 2000
    store = make_store(torch, hw, dev, 11)
    order = rng.permutation(len(store)).astype(np.int64)
    pick = lambda r: order[(r * batch) % len(store):(r * batch) % len(store) + batch]
    ident, quarter = np.zeros(batch, np.int32), np.ones(batch, np.int32)
    out = {"case": what, "build": rt.build_id(), "tiles": len(store), "batch": batch, "reps": args.reps,
           "store_mbytes": round(int(store.offsets[-1]) * 17 / 1e6, 1)}
    if args.kernel_only is not None:
        # for a kernel trace: nothing but `reps` launches of one op on the rotating batches, and the bytes of one of them
        bufs = {k: torch.empty(int(store.offsets[-1]), dtype=getattr(store, k).dtype, device=dev) for k in NAMES}
        ws = torch.empty(int(ctx.lib.bgnn_tile_gather_workspace_bytes(batch)) // 8, dtype=torch.int64, device=dev)
        for r in range(args.reps):
            raw_call(rt, ctx, store, pick(r), np.full(batch, args.kernel_only, np.int32), bufs, ws)
        torch.cuda.synchronize()
        cells = statistics.mean(int((store.offsets[pick(r) + 1] - store.offsets[pick(r)]).sum()) for r in range(len(store) // batch))
        out.update(op=args.kernel_only, batch_bytes=int(2 * 17 * cells + 32 * batch))
        print(json.dumps(out), flush=True)
        return 0
    # the two ways agree first
    idx = pick(0)
    mixed = (np.arange(batch) % 8).astype(np.int32)
    out["equal_bits"] = all(same(torch, store.gather(idx, ops)[2], torch_turn(torch, store, idx, ops)) for ops in (mixed, ident))
    if not out["equal_bits"]:
        print(json.dumps(out), flush=True)
        return 1
    max_cells = max(int((store.offsets[pick(r) + 1] - store.offsets[pick(r)]).sum()) for r in range(len(store) // batch))
    bufs = {k: torch.empty(max_cells, dtype=getattr(store, k).dtype, device=dev) for k in NAMES}
    ws = torch.empty(int(ctx.lib.bgnn_tile_gather_workspace_bytes(batch)) // 8, dtype=torch.int64, device=dev)
    cells = statistics.mean(int((store.offsets[pick(r) + 1] - store.offsets[pick(r)]).sum()) for r in range(len(store) // batch))
    nbytes = 2 * 17 * cells + 32 * batch
    out["batch_mbytes"] = round(nbytes / 1e6, 2)
    for name, ops in (("identity", ident), ("quarter_turn", quarter)):
        m = measure(torch, lambda r: raw_call(rt, ctx, store, pick(r), ops, bufs, ws), args.reps, args.warmup)
        m["gbytes_per_s"] = round(nbytes / m["device_us_median"] / 1e3, 1)
        m["share_of_hbm_peak"] = round(nbytes / (m["device_us_median"] * 1e-6) / HBM_PEAK, 3)
        out[f"call_{name}"] = m
        out[f"gather_{name}"] = measure(torch, lambda r: store.gather(pick(r), ops), args.reps, args.warmup)
    out["torch_quarter_turn"] = measure(torch, lambda r: torch_turn(torch, store, pick(r), quarter), max(args.reps // 3, 3), 2)
    print(json.dumps(out), flush=True)
    return 0


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--what", nargs="+", default=["uniform", "ragged"], choices=["uniform", "ragged"])
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--kernel-only", type=int, choices=range(8), metavar="OP",
                    help="launch bgnn_tile_gather --reps times with this op and nothing else (to run under a kernel trace)")
    args = ap.parse_args()
    if args.reps < 1:
        ap.error("--reps must be at least 1")
    for what in args.what:
        rc = run_case(args, what)
        if rc:
            return rc
    return 0


if __name__ == "__main__":
    sys.exit(main())
