#!/usr/bin/env python3
"""Feature labels: the device call at survey size, and the reference's loop on the same machine at a size where it ends.

    python tools/feature_labels_time.py                      # the three device cases and the numpy loop
    python tools/feature_labels_time.py --cases 4096:1000    # one device case: SIZE:FEATURES

Every measurement is a step of its own: a child process (``--step``) under a time limit (``--limit`` seconds), one JSON line
each; the first step that fails or runs out of time ends the run.  A step

  device  builds an S x S depth plane in HBM (2 % nodata) and F features with uniformly drawn centres and the reference's default
          radii at 1 m cells (50 / 25 / 30 pixels, drawn evenly), times the host plan on the wall clock (size query and fill, median
          of ``--reps``) and ``bgnn_feature_labels`` with that plan from the HBM plane to the label plane and the counts (HIP events
          around the call: the upload of plan and table through the context's staging and the one kernel; warm-up, then the median,
          minimum and maximum of ``--reps``).  ``gb_per_s`` is the 8 bytes per cell the job has to move (one read of the depth, one
          write of the labels) over the median.
  host    the reference's loop restated in numpy (``np.ogrid`` over the whole plane, a float64 distance plane and a boolean mask
          per feature) at ``--host-size`` with ``--host-features`` features, on the wall clock; ``ns_per_feature_cell`` is that
          time over features x cells.  The loop's cost is linear in features x cells, so the ``extrapolated_s`` entries are that
          figure times each device case's features x cells: EXTRAPOLATED, not measured.
"""
import argparse
import ctypes as C
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

DEFAULT_CASES = "4096:1000,20000:1000,20000:100000"
RADII = (50, 25, 30)                                  # WRECKS, UWTROC, OBSTRN at 1 m


def make_table(np, size, features, seed=7):
    rng = np.random.default_rng(seed)
    return np.stack([rng.integers(0, size, features), rng.integers(0, size, features), rng.choice(RADII, features),
                     np.ones(features, np.int64)], 1).astype(np.int32)


def step_device(args):
    import numpy as np
    import torch
    from bathymetric_gnn_amd import runtime as rt
    from bathymetric_gnn_amd.data.feature_labels import _plan_buffer
    dev = torch.device("cuda:0")
    size, n = args.size, args.features
    g = torch.Generator(device=dev).manual_seed(11)
    depth = -30 + 5 * torch.randn((size, size), generator=g, device=dev)
    depth[torch.rand((size, size), generator=g, device=dev) < 0.02] = 1.0e6
    table = make_table(np, size, n)
    plan_ms = []
    for _ in range(args.reps):
        t0 = time.perf_counter()
        raw, bins = _plan_buffer(table, (size, size))
        plan_ms.append((time.perf_counter() - t0) * 1e3)
    ctx = rt.get_context(dev)
    lib = ctx.lib
    ws = torch.empty((int(lib.bgnn_feature_labels_workspace_bytes(n, C.c_size_t(raw.nbytes))) + 7) // 8, dtype=torch.int64, device=dev)
    labels = torch.empty((size, size), dtype=torch.int32, device=dev)
    stats = torch.zeros(3, dtype=torch.int64, device=dev)

    def call():
        ctx.begin()
        rt.check(lib.bgnn_feature_labels(ctx.handle, rt.ptr(depth), None, size, size, 1.0e6, table.ctypes.data_as(C.c_void_p), n,
                                         raw.ctypes.data_as(C.c_void_p), C.c_size_t(raw.nbytes), rt.ptr(ws), C.c_size_t(ws.numel() * 8),
                                         rt.ptr(labels), rt.ptr(stats)))
        ctx.end()

    for _ in range(2):
        call()
    torch.cuda.synchronize()
    ms = []
    for _ in range(args.reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        call()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    med = statistics.median(ms)
    cells = size * size
    print(json.dumps({"step": "device", "size": size, "features": n, "cells": cells, "build": rt.build_id(),
                      "plan_ms": round(statistics.median(plan_ms), 3), "plan_entries": int(raw[bins]), "plan_bytes": int(raw.nbytes),
                      "device_ms": round(med, 3), "device_ms_min": round(min(ms), 3), "device_ms_max": round(max(ms), 3),
                      "gb_per_s": round(8 * cells / (med * 1e-3) / 1e9, 1), "reps": args.reps,
                      "valid_cells": int(stats[0].item()), "feature_cells": int(stats[1].item())}), flush=True)


def step_host(args):
    import numpy as np
    size, n = args.size, args.features
    rng = np.random.default_rng(11)
    depth = (-30 + 5 * rng.standard_normal((size, size))).astype(np.float32)
    depth[rng.random((size, size)) < 0.02] = 1.0e6
    table = make_table(np, size, n)
    shape = depth.shape
    t0 = time.perf_counter()
    valid = (depth != 1.0e6) & np.isfinite(depth)
    labels = np.zeros(shape, dtype=np.int32)
    labels[~valid] = -1
    for row, col, radius_px, label_value in table:
        yy, xx = np.ogrid[:shape[0], :shape[1]]
        dist = np.sqrt((xx - col) ** 2 + (yy - row) ** 2)
        feature_mask = dist <= radius_px
        labels[feature_mask & valid] = label_value
    s = time.perf_counter() - t0
    per = s / (n * size * size)
    out = {"step": "host", "size": size, "features": n, "host_s": round(s, 3), "ns_per_feature_cell": round(per * 1e9, 3),
           "feature_cells": int((labels == 1).sum()), "extrapolated_s": {}}
    for case in args.cases.split(","):
        cs, cf = (int(v) for v in case.split(":"))
        out["extrapolated_s"][case] = round(per * cf * cs * cs, 1)
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--cases", default=DEFAULT_CASES, help="device cases, SIZE:FEATURES separated by commas")
    ap.add_argument("--host-size", type=int, default=4096)
    ap.add_argument("--host-features", type=int, default=20)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--limit", type=int, default=240, help="seconds per step")
    ap.add_argument("--step", choices=["device", "host"], help="run one step in this process")
    ap.add_argument("--size", type=int, default=1024)
    ap.add_argument("--features", type=int, default=100)
    args = ap.parse_args()
    if args.step:
        return (step_device if args.step == "device" else step_host)(args)
    steps = [("host", args.host_size, args.host_features)] if args.host_size > 0 else []
    steps += [("device",) + tuple(int(v) for v in case.split(":")) for case in args.cases.split(",") if case]
    for what, size, features in steps:
        cmd = [sys.executable, os.path.abspath(__file__), "--step", what, "--size", str(size), "--features", str(features),
               "--reps", str(args.reps), "--cases", args.cases]
        try:
            r = subprocess.run(cmd, timeout=args.limit)
        except subprocess.TimeoutExpired:
            print(json.dumps({"step": what, "size": size, "features": features, "error": f"no result within {args.limit} s"}), flush=True)
            return 1
        if r.returncode != 0:
            print(json.dumps({"step": what, "size": size, "features": features, "error": f"exit status {r.returncode}"}), flush=True)
            return 1
    return 0


if __name__ == "__main__":
    sys.exit(main())
