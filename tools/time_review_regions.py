#!/usr/bin/env python3
"""Review-region export: the device call at survey size, the noise analysis of planes of the same size as a yardstick, and the
reference's arithmetic on the same machine.

    python tools/time_review_regions.py                      # device and scipy restatement at 20000^2, the literal loop at 4096^2
    python tools/time_review_regions.py --device-size 4096 --host-size 4096 --loop-size 512

Every measurement is a step of its own: a child process (``--step``) under a time limit (``--limit`` seconds), one JSON line
each; the first step that fails or runs out of time ends the run.  A step

  device     builds an S x S smooth confidence field in HBM (a few plane waves through a sigmoid, 0.5 % NaN cells), times
             ``review_regions_build`` from the HBM plane to the counts, the record table and the mask (HIP events, median of
             ``--reps``), and once ``export_review_regions`` from the HBM plane to the list of regions on the wall clock (the one read
             of the table included)
  yardstick  ``noise_analysis_build`` on four planes of the same size (tools/time_noise_analysis.py's): the same labelling
             structure, with the analysis' selections and roughness on top
  host       the fast restatement of the reference's script -- ``ndimage.label``, ``np.bincount``, ``ndimage.find_objects``, a
             float64 mean per kept region -- on the same field at ``--host-size``, on the wall clock
  loop       the reference's loop as it stands -- ``labeled == i`` over the whole raster once per region -- at ``--loop-size``
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
LOW, HIGH, MIN_SIZE = 0.4, 0.7, 100


def make_field(torch, size, device, seed=17):
    """A smooth confidence field in (0, 1): structures of 30 .. 300 cells, whatever the size."""
    g = torch.Generator(device="cpu").manual_seed(seed)
    r = torch.arange(size, dtype=torch.float32, device=device)
    z = torch.zeros((size, size), dtype=torch.float32, device=device)
    for _ in range(6):
        f = (0.003 + 0.027 * torch.rand(2, generator=g)) * (2 * torch.randint(0, 2, (2,), generator=g) - 1)
        amp, phase = 0.5 + torch.rand(1, generator=g).item(), 6.2831853 * torch.rand(1, generator=g).item()
        z += amp * torch.sin(6.2831853 * (f[0].item() * r[:, None] + f[1].item() * r[None, :]) + phase)
    conf = torch.sigmoid(z)
    del z
    gd = torch.Generator(device=device).manual_seed(seed)
    conf[torch.rand((size, size), generator=gd, device=device) < 0.005] = float("nan")
    return conf


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
    from bathymetric_gnn_amd.data.review_regions import export_review_regions, review_regions_build
    dev = torch.device("cuda:0")
    conf = make_field(torch, args.size, dev)
    mask = torch.empty_like(conf)
    capacity = min(conf.numel() // MIN_SIZE, 1 << 16)
    ms = device_ms(torch, lambda: review_regions_build(conf, np.float32(LOW), np.float32(HIGH), MIN_SIZE, capacity, mask), args.reps)
    del mask
    t0 = time.perf_counter()
    result = export_review_regions(None, conf, LOW, HIGH, MIN_SIZE)
    wall = (time.perf_counter() - t0) * 1e3
    print(json.dumps({"step": "device", "size": args.size, "cells": conf.numel(), "build": rt.build_id(),
                      "device_ms": round(statistics.median(ms), 3), "device_ms_min": round(min(ms), 3), "export_wall_ms": round(wall, 3),
                      "workspace_gib": round(rt.load_library().bgnn_review_workspace_bytes(args.size, args.size) / 2 ** 30, 2),
                      **result.counts}), flush=True)


def step_yardstick(args):
    import torch
    from bathymetric_gnn_amd.data.noise_analysis import noise_analysis_build
    from time_noise_analysis import make_planes
    planes = make_planes(torch, args.size, torch.device("cuda:0"))
    ms = device_ms(torch, lambda: noise_analysis_build(*planes), args.reps)
    print(json.dumps({"step": "yardstick", "size": args.size, "cells": planes[0].numel(), "noise_analysis_ms": round(statistics.median(ms), 3),
                      "noise_analysis_ms_min": round(min(ms), 3)}), flush=True)


def step_host(args):
    import numpy as np
    import torch
    from scipy import ndimage
    conf = make_field(torch, args.size, torch.device("cpu")).numpy()
    t0 = time.perf_counter()
    with np.errstate(invalid="ignore"):
        unc = (conf >= np.float32(LOW)) & (conf <= np.float32(HIGH))
    unc &= np.isfinite(conf)
    labeled, n = ndimage.label(unc)
    t1 = time.perf_counter()
    sizes = np.bincount(labeled.ravel(), minlength=n + 1)
    boxes = ndimage.find_objects(labeled)
    kept = np.flatnonzero(sizes[1:] >= MIN_SIZE) + 1
    keep = np.zeros(n + 1, bool)
    keep[kept] = True
    mask = keep[labeled].astype(np.float32)
    regions = []
    for i in kept:
        sl = boxes[i - 1]
        cells = conf[sl][labeled[sl] == i].astype(np.float64)
        regions.append((int(sizes[i]), float(cells.sum() / cells.size), sl))
    t2 = time.perf_counter()
    print(json.dumps({"step": "host", "size": args.size, "cells": int(conf.size), "host_s": round(t2 - t0, 3), "label_s": round(t1 - t0, 3),
                      "regions": int(n), "kept_regions": len(regions), "kept_cells": int(mask.sum())}), flush=True)


def step_loop(args):
    import numpy as np
    import torch
    from scipy import ndimage
    confidence = make_field(torch, args.size, torch.device("cpu")).numpy()
    t0 = time.perf_counter()
    with np.errstate(invalid="ignore"):
        uncertain = (confidence >= LOW) & (confidence <= HIGH)
    uncertain &= np.isfinite(confidence)
    labeled, num_regions = ndimage.label(uncertain)
    review_mask = np.zeros_like(uncertain)
    regions = []
    for i in range(1, num_regions + 1):
        region_mask = labeled == i
        if np.sum(region_mask) >= MIN_SIZE:
            review_mask |= region_mask
            rows, cols = np.where(region_mask)
            regions.append((int(np.sum(region_mask)), float(np.mean(confidence[region_mask])), int(rows.min()), int(rows.max()),
                            int(cols.min()), int(cols.max())))
    t1 = time.perf_counter()
    print(json.dumps({"step": "loop", "size": args.size, "cells": int(confidence.size), "loop_s": round(t1 - t0, 3), "regions": int(num_regions),
                      "kept_regions": len(regions)}), flush=True)


STEPS = {"device": step_device, "yardstick": step_yardstick, "host": step_host, "loop": step_loop}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--device-size", type=int, default=20000)
    ap.add_argument("--host-size", type=int, default=20000)
    ap.add_argument("--loop-size", type=int, default=4096)
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
