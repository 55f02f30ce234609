#!/usr/bin/env python3
"""Slope-based feature labels: the device call at survey size, the review-region export of a plane of the same size as a yardstick,
and the reference's arithmetic on the same machine.

    python tools/time_slope_features.py                      # device and numpy / scipy restatement at 20000^2, the literal loop at 1000^2
    python tools/time_slope_features.py --device-size 4096 --host-size 4096 --loop-size 512

Every measurement is a step of its own: a child process (``--step``) under a time limit (``--limit`` seconds), one JSON line
each; the first step that fails or runs out of time ends the run.  A step

  device     builds an S x S relief in HBM (plane waves and bumps in multiples of 3/64 m, 1.0e6 holes, 0.3 % NaN cells), times
             ``slope_features_build`` from the HBM plane to labels, mask and counts (HIP events, median of ``--reps``), then
             ``add_feature_labels`` with ``--wrecks`` wrecks of radius 50 (HIP events around the whole call: the slope step, the host
             plan of the discs and ``rasterize_features``), and once on the wall clock to ``stats()``
  yardstick  ``review_regions_build`` on tools/time_review_regions.py's field of the same size: the same labelling scheme with
             more aggregates and an ordered compaction
  host       the restatement of the reference's script -- ``np.gradient``, the float32 slope, ``ndimage.label``, ``np.bincount`` for
             the sizes -- on the same relief at ``--host-size``, on the wall clock
  loop       the script's size filter as it stands -- ``labeled == i`` over the whole raster once per cluster -- at ``--loop-size``
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
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
THRESHOLD, MIN_SIZE, RADIUS, NODATA, Q = 15.0, 100, 50, 1.0e6, 3.0 / 64.0


def make_relief(torch, size, device, seed=23):
    """Structures of 30 .. 300 cells whatever the size; slopes on both sides of 15 degrees."""
    g = torch.Generator(device="cpu").manual_seed(seed)
    r = torch.arange(size, dtype=torch.float32, device=device)
    z = torch.full((size, size), 30.0, dtype=torch.float32, device=device)
    for _ in range(6):
        f = (0.003 + 0.027 * torch.rand(2, generator=g)) * (2 * torch.randint(0, 2, (2,), generator=g) - 1)
        amp, phase = 0.02 / f.abs().max().item() * (0.5 + torch.rand(1, generator=g).item()), 6.2831853 * torch.rand(1, generator=g).item()
        z += amp * torch.sin(6.2831853 * (f[0].item() * r[:, None] + f[1].item() * r[None, :]) + phase)
    gd = torch.Generator(device=device).manual_seed(seed)
    z += 3.0 * (torch.rand((size, size), generator=gd, device=device) < 0.0005)
    z = torch.round(z / Q) * Q
    for k in range(max(1, size // 500)):                        # holes of 40 x 60 cells
        r0, c0 = (torch.randint(0, max(1, size - 60), (2,), generator=g)).tolist()
        z[r0:r0 + 40, c0:c0 + 60] = NODATA
    z[torch.rand((size, size), generator=gd, device=device) < 0.003] = float("nan")
    return z


def device_ms(torch, fn, reps):
    fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    torch.cuda.synchronize()
    return ms


def step_device(args):
    import numpy as np
    import torch
    from bathymetric_gnn_amd import runtime as rt
    from bathymetric_gnn_amd.data import add_feature_labels, slope_cut
    from bathymetric_gnn_amd.data.slope_features import slope_features_build, slope_stats
    dev = torch.device("cuda:0")
    depth = make_relief(torch, args.size, dev)
    cut = slope_cut(THRESHOLD)
    ms = device_ms(torch, lambda: slope_features_build(depth, cut, MIN_SIZE), args.reps)
    stats = slope_stats(slope_features_build(depth, cut, MIN_SIZE)[2])
    rng = np.random.default_rng(5)
    gt = (0.0, 1.0, 0.0, 0.0, 0.0, -1.0)
    wrecks = [{"x": float(x), "y": -float(y)} for x, y in rng.uniform(0, args.size, (args.wrecks, 2))]
    ms_w = device_ms(torch, lambda: add_feature_labels(depth, wrecks, THRESHOLD, RADIUS, MIN_SIZE, transform=gt), args.reps)
    t0 = time.perf_counter()
    result = add_feature_labels(depth, wrecks, THRESHOLD, RADIUS, MIN_SIZE, transform=gt)
    final = result.stats()
    wall = (time.perf_counter() - t0) * 1e3
    print(json.dumps({"step": "device", "size": args.size, "cells": depth.numel(), "build": rt.build_id(),
                      "slope_ms": round(statistics.median(ms), 3), "slope_ms_min": round(min(ms), 3),
                      "with_wrecks_ms": round(statistics.median(ms_w), 3), "with_wrecks_ms_min": round(min(ms_w), 3),
                      "with_wrecks_wall_ms": round(wall, 3), "wrecks": args.wrecks,
                      "workspace_gib": round(rt.load_library().bgnn_slope_features_workspace_bytes(args.size, args.size) / 2 ** 30, 2),
                      **stats, "feature_cells": final["feature_cells"]}), flush=True)


def step_yardstick(args):
    import numpy as np
    import torch
    from bathymetric_gnn_amd.data.review_regions import review_regions_build
    from time_review_regions import make_field
    conf = make_field(torch, args.size, torch.device("cuda:0"))
    mask = torch.empty_like(conf)
    capacity = min(conf.numel() // 100, 1 << 16)
    ms = device_ms(torch, lambda: review_regions_build(conf, np.float32(0.4), np.float32(0.7), 100, capacity, mask), args.reps)
    print(json.dumps({"step": "yardstick", "size": args.size, "cells": conf.numel(), "review_regions_ms": round(statistics.median(ms), 3),
                      "review_regions_ms_min": round(min(ms), 3)}), flush=True)


def steep_cells(np, depth):
    with np.errstate(all="ignore"):
        gy, gx = np.gradient(depth)
        return np.degrees(np.arctan(np.sqrt(gx ** 2 + gy ** 2))) > THRESHOLD


def step_host(args):
    import numpy as np
    import torch
    from scipy import ndimage
    depth = make_relief(torch, args.size, torch.device("cpu")).numpy()
    t0 = time.perf_counter()
    steep = steep_cells(np, depth)
    t1 = time.perf_counter()
    labeled, n = ndimage.label(steep)
    t2 = time.perf_counter()
    keep = np.bincount(labeled.ravel(), minlength=n + 1) >= MIN_SIZE
    keep[0] = False
    mask = keep[labeled]
    valid = (depth != np.float32(NODATA)) & np.isfinite(depth)
    labels = np.zeros(depth.shape, np.int32)
    labels[~valid] = -1
    labels[mask & valid] = 1
    t3 = time.perf_counter()
    print(json.dumps({"step": "host", "size": args.size, "cells": int(depth.size), "host_s": round(t3 - t0, 3), "slope_s": round(t1 - t0, 3),
                      "label_s": round(t2 - t1, 3), "clusters": int(n), "kept_clusters": int(keep.sum()), "kept_cells": int(mask.sum()),
                      "slope_feature_cells": int((labels == 1).sum())}), flush=True)


def step_loop(args):
    import numpy as np
    import torch
    from scipy import ndimage
    depth = make_relief(torch, args.size, torch.device("cpu")).numpy()
    t0 = time.perf_counter()
    mask = steep_cells(np, depth)
    labeled, n = ndimage.label(mask)
    for i in range(1, n + 1):
        if np.sum(labeled == i) < MIN_SIZE:
            mask[labeled == i] = False
    t1 = time.perf_counter()
    print(json.dumps({"step": "loop", "size": args.size, "cells": int(depth.size), "loop_s": round(t1 - t0, 3), "clusters": int(n),
                      "kept_cells": int(mask.sum())}), flush=True)


STEPS = {"device": step_device, "yardstick": step_yardstick, "host": step_host, "loop": step_loop}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--device-size", type=int, default=20000)
    ap.add_argument("--host-size", type=int, default=20000)
    ap.add_argument("--loop-size", type=int, default=1000)
    ap.add_argument("--wrecks", type=int, default=1000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--limit", type=int, default=300, help="seconds per step")
    ap.add_argument("--step", choices=sorted(STEPS), help="run one step in this process")
    ap.add_argument("--size", type=int, default=1024)
    args = ap.parse_args()
    if args.step:
        return STEPS[args.step](args)
    for what, size in (("device", args.device_size), ("yardstick", args.device_size), ("loop", args.loop_size), ("host", args.host_size)):
        if size <= 0:
            continue
        cmd = [sys.executable, os.path.abspath(__file__), "--step", what, "--size", str(size), "--reps", str(args.reps),
               "--wrecks", str(args.wrecks)]
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
