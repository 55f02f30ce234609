#!/usr/bin/env python3
"""A tile store from planes in HBM: the device scan and gather against the host-planned path, on the same machine.

    python tools/time_tile_store.py                          # 4096^2 and 20000^2 ground truth, 4096^2 survey
    python tools/time_tile_store.py --sizes 4096 --reps 7

Every measurement is a step of its own: a child process (``--step``) under a time limit (``--limit`` seconds), one JSON line each;
the first step that fails or runs out of time ends the run.  The planes are seeded synthetic ones, no file is read.  A step

  truth   builds the four planes of an S x S ground truth in HBM (labels 0 / 1 / 2 with -1 in blocks, so that tiles are dropped;
          difference, depth, uncertainty) and builds the store twice per repetition, alternating the two ways in one process:
          ``TileStore.from_ground_truth`` on the device tensors (the label plane goes to the host, ``plan_ground_truth_tiles`` runs
          there, ``torch.cat`` cuts) and ``TileStore.from_ground_truths`` (scan, 32 bytes per box to the host, gather).  Tile 512,
          overlap 64.  A host clock around a device synchronise, after a warm-up of either; median, minimum and maximum of
          ``--reps`` repetitions.  The two stores are compared as bits.
          ``scan`` / ``cut``: HIP events on the context's stream around ``bgnn_tile_scan`` / ``bgnn_tile_cut`` alone (table upload
          included), with the bytes each moves worked out from the box list -- scan: 4 B read per cell of every candidate box;
          cut: 8 B per cell and plane of every kept box (read + write) and 1 B of mask -- and the bandwidth that gives.
  survey  ``TileStore.from_grid`` on host arrays against ``TileStore.from_survey`` on the same planes in HBM, S x S, the same way.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

TILE, OVERLAP = 512, 64


def make_truth(torch, size, device, seed=7):
    g = torch.Generator(device=device).manual_seed(seed)
    shape = (size, size)
    labels = (torch.rand(shape, generator=g, device=device) * 20).to(torch.int32).clamp_(max=2)       # 0: 5 %, 1: 5 %, 2: 90 % ...
    labels = 2 - labels                                                                            # ... 0: 90 %, 1: 5 %, 2: 5 %
    block = max(size // 16, 1)
    holes = torch.rand((16, 16), generator=g, device=device) < 0.3                                   # blocks without data
    holes = holes.repeat_interleave(block, 0).repeat_interleave(block, 1)
    labels[:holes.shape[0], :holes.shape[1]][holes[:size, :size]] = -1
    del holes
    labels[torch.rand(shape, generator=g, device=device) < 0.02] = -1
    difference = torch.randn(shape, generator=g, device=device) * 0.05
    difference[labels < 0] = float("nan")
    depth = -30 + 5 * torch.randn(shape, generator=g, device=device)
    unc = torch.rand(shape, generator=g, device=device)
    return labels, difference, depth, unc


def wall(torch, fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def spread(ms):
    return {"median_ms": round(statistics.median(ms), 3), "min_ms": round(min(ms), 3), "max_ms": round(max(ms), 3)}


def alternate(torch, old, new, reps):
    """Warm-up of either, then ``reps`` rounds of old, new; the last results and the two lists of wall times."""
    a, b = old(), new()
    torch.cuda.synchronize()
    t_old, t_new = [], []
    for _ in range(reps):
        del a, b
        ms, a = wall(torch, old)
        t_old.append(ms)
        ms, b = wall(torch, new)
        t_new.append(ms)
    return a, b, t_old, t_new


def same_bits(torch, a, b):
    for k in ("depth", "mask", "unc", "labels", "difference"):
        x, y = getattr(a, k), getattr(b, k)
        if (x is None) != (y is None):
            return False
        if x is not None and not torch.equal(x.view(torch.int32) if x.dtype == torch.float32 else x,
                                             y.view(torch.int32) if y.dtype == torch.float32 else y):
            return False
    return bool((a.hw == b.hw).all() and (a.res == b.res).all() and (a.offsets == b.offsets).all())


def events(torch, ctx, fn, reps):
    """Median / minimum of HIP events on the context's stream around ``fn`` (which works on that stream and does not wait for the
    host).  A matrix product queued in front keeps the stream busy while the host enqueues ``fn``, so the events bracket device
    time and not the host's enqueueing."""
    fn()
    busy = torch.randn(4096, 4096, device=ctx.device)
    sink = torch.empty_like(busy)
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        with torch.cuda.stream(ctx.stream):
            torch.mm(busy, busy, out=sink)
        a.record(ctx.stream)
        fn()
        b.record(ctx.stream)
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return statistics.median(ms), min(ms)


def step_truth(args):
    import numpy as np
    import torch
    from bathymetric_gnn_amd import runtime as rt
    from bathymetric_gnn_amd.training import TileStore, cut_tile_boxes, plan_tile_boxes, scan_tile_boxes
    dev = torch.device("cuda:0")
    ctx = rt.get_context(dev)
    labels, difference, depth, unc = make_truth(torch, args.size, dev)
    kw = dict(tile_size=TILE, overlap=OVERLAP, min_valid_ratio=0.1, device=dev)
    old = lambda: TileStore.from_ground_truth(labels, difference, depth, unc, **kw)
    new = lambda: TileStore.from_ground_truths([(labels, difference, depth, unc, (1.0, 1.0))], **kw)
    a, b, t_old, t_new = alternate(torch, old, new, args.reps)
    out = {"step": "truth", "size": args.size, "build": rt.build_id(), "reps": args.reps, "tiles": len(b),
           "from_ground_truth": spread(t_old), "from_ground_truths": spread(t_new),
           "speedup": round(statistics.median(t_old) / statistics.median(t_new), 2),
           "equal_bits": same_bits(torch, a, b) and a.boxes == b.boxes and a._class_counts == b._class_counts}
    kept = b.boxes
    del a, b
    candidates = plan_tile_boxes(args.size, args.size, TILE, OVERLAP)
    out["candidates"] = len(candidates)
    scan_bytes = 4 * TILE * TILE * len(candidates) + 32 * len(candidates)
    med, best = events(torch, ctx, lambda: scan_tile_boxes(labels, candidates, ctx=ctx), args.reps)
    out["scan"] = {"median_ms": round(med, 4), "min_ms": round(best, 4), "mbytes": round(scan_bytes / 1e6, 1),
                   "gbytes_per_s": round(scan_bytes / med / 1e6, 1)}
    cells = TILE * TILE * len(kept)
    stores = [torch.empty(cells, dtype=p.dtype, device=dev) for p in (labels, difference, depth, unc)]
    mask = torch.empty(cells, dtype=torch.uint8, device=dev)
    offsets = np.arange(len(kept), dtype=np.int64) * (TILE * TILE)
    cut_bytes = cells * (4 * 8 + 1)
    med, best = events(torch, ctx, lambda: cut_tile_boxes([labels, difference, depth, unc], stores, kept, offsets, mask=mask, ctx=ctx),
                       args.reps)
    out["cut"] = {"median_ms": round(med, 4), "min_ms": round(best, 4), "mbytes": round(cut_bytes / 1e6, 1),
                  "gbytes_per_s": round(cut_bytes / med / 1e6, 1)}
    print(json.dumps(out), flush=True)


def step_survey(args):
    import torch
    from bathymetric_gnn_amd import runtime as rt
    from bathymetric_gnn_amd.data import BathymetricGrid, TileManager
    from bathymetric_gnn_amd.training import TileStore
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(11)
    shape = (args.size, args.size)
    depth = -30 + 5 * torch.randn(shape, generator=g, device=dev)
    depth[torch.rand(shape, generator=g, device=dev) < 0.02] = 1.0e6
    depth[: args.size // 3, : args.size // 2] = float("nan")
    unc = torch.rand(shape, generator=g, device=dev)
    grid = BathymetricGrid(depth.cpu().numpy(), unc.cpu().numpy(), 1.0e6, resolution=(1.0, 1.0))
    tm = TileManager(TILE, OVERLAP, min_valid_ratio=0.1)
    old = lambda: TileStore.from_grid(grid, tm, device=dev)
    new = lambda: TileStore.from_survey(depth, tm, unc, nodata_value=1.0e6, device=dev)
    a, b, t_old, t_new = alternate(torch, old, new, args.reps)
    out = {"step": "survey", "size": args.size, "build": rt.build_id(), "reps": args.reps, "tiles": len(b), "from_grid": spread(t_old),
           "from_survey": spread(t_new), "speedup": round(statistics.median(t_old) / statistics.median(t_new), 2),
           "equal_bits": same_bits(torch, a, b)}
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--sizes", type=int, nargs="+", default=[4096, 20000])
    ap.add_argument("--survey-size", type=int, default=4096)
    ap.add_argument("--what", nargs="+", default=["truth", "survey"], choices=["truth", "survey"])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--limit", type=int, default=240, help="seconds per step")
    ap.add_argument("--step", choices=["truth", "survey"], help="run one step in this process")
    ap.add_argument("--size", type=int, default=4096)
    args = ap.parse_args()
    if args.reps < 1:
        ap.error("--reps must be at least 1")
    if args.step:
        return (step_truth if args.step == "truth" else step_survey)(args)
    steps = [("truth", s) for s in args.sizes if "truth" in args.what]
    steps += [("survey", args.survey_size)] if "survey" in args.what else []
    for what, size in steps:
        cmd = [sys.executable, os.path.abspath(__file__), "--step", what, "--size", str(size), "--reps", str(args.reps)]
        try:
            r = subprocess.run(cmd, timeout=args.limit)
        except subprocess.TimeoutExpired:
            print(json.dumps({"step": what, "size": size, "error": f"no result within {args.limit} s"}), flush=True)
            return 1
        if r.returncode != 0:
            print(json.dumps({"step": what, "size": size, "error": f"exit status {r.returncode}"}), flush=True)
            return 1
    return 0


if __name__ == "__main__":
    sys.exit(main())
