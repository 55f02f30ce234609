#!/usr/bin/env python3
"""Noise pattern analysis: the device call at survey size, and the reference's arithmetic on the same machine at a size where it ends.

    python tools/time_noise_analysis.py                      # device at 20000^2, numpy / scipy at 1024^2
    python tools/time_noise_analysis.py --device-size 4096 --host-size 256

Every measurement is a step of its own: a child process (``--step``) under a time limit (``--limit`` seconds), one JSON line
each; the first step that fails or runs out of time ends the run.  A step

  device  builds S x S planes in HBM (8 % scattered noise cells and a stripe every 512 rows, 2 % invalid cells), times
          ``noise_analysis_build`` from the HBM planes to the result block (HIP events, median of ``--reps``), and once
          ``analyze_noise_patterns`` from the HBM planes to the dictionary on the wall clock (the one read of the block included).
  host    the reference's ``analyze_ground_truth`` arithmetic as the reference states it -- ``scipy.ndimage.generic_filter`` with
          ``np.nanstd`` as a Python callback per cell, ``ndimage.label``, ``np.median`` / ``np.percentile`` / ``np.nanmedian`` -- on
          planes of the same kind at ``--host-size``, on the wall clock, with the share of the filter alone.
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


def make_planes(torch, size, device, seed=11):
    g = torch.Generator(device=device).manual_seed(seed)
    shape = (size, size)
    clean = -30 + 5 * torch.randn(shape, generator=g, device=device)
    labels = torch.where(torch.rand(shape, generator=g, device=device) < 0.08, 2, 0).to(torch.int32)
    labels[::512, :] = 2
    labels[torch.rand(shape, generator=g, device=device) < 0.02] = -1
    difference = 0.05 * torch.randn(shape, generator=g, device=device)
    spike = (0.2 + torch.rand(shape, generator=g, device=device)) * torch.where(torch.rand(shape, generator=g, device=device) < 0.6, 1.0, -1.0)
    difference = torch.where(labels == 2, spike, difference)
    del spike
    difference[labels < 0] = float("nan")
    noisy = clean + torch.nan_to_num(difference)
    return labels, difference, noisy, clean


def step_device(args):
    import torch
    from bathymetric_gnn_amd import runtime as rt
    from bathymetric_gnn_amd.data.noise_analysis import analyze_noise_patterns, noise_analysis_build
    dev = torch.device("cuda:0")
    planes = make_planes(torch, args.size, dev)
    noise_analysis_build(*planes)
    torch.cuda.synchronize()
    ms = []
    for _ in range(args.reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        noise_analysis_build(*planes)
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    analysis = analyze_noise_patterns(planes, device=dev)
    wall = (time.perf_counter() - t0) * 1e3
    cells = planes[0].numel()
    print(json.dumps({"step": "device", "size": args.size, "cells": cells, "build": rt.build_id(), "device_ms": round(statistics.median(ms), 3),
                      "device_ms_min": round(min(ms), 3), "analyze_wall_ms": round(wall, 3),
                      "workspace_gib": round(rt.load_library().bgnn_noise_analysis_workspace_bytes(args.size, args.size) / 2 ** 30, 2),
                      "num_clusters": analysis["clustering"]["num_clusters"]}), flush=True)


def step_host(args):
    import warnings
    import numpy as np
    import torch
    from scipy import ndimage
    labels, difference, noisy, clean = (p.numpy() for p in make_planes(torch, args.size, torch.device("cpu")))
    warnings.simplefilter("ignore")
    t0 = time.perf_counter()
    valid, noise = labels >= 0, labels == 2
    mag = np.abs(difference[noise & valid])
    out = [np.mean(mag), np.std(mag), np.median(mag), np.percentile(mag, 90), np.percentile(mag, 99), np.max(mag)]
    d = difference[noise & valid]
    out += [np.mean(d > 0), np.mean(d < 0), np.mean(d[d > 0]), np.mean(d[d < 0])]
    edges = [0, 10, 20, 50, 100, 200, 500, 1000, 10000]
    for lo, hi in zip(edges, edges[1:]):
        in_range = (-noisy >= lo) & (-noisy < hi) & noise & valid
        out.append((np.sum(in_range), np.sum((-noisy >= lo) & (-noisy < hi) & valid), np.mean(np.abs(difference[in_range])) if in_range.any() else 0))
    labeled, k = ndimage.label(noise)
    sizes = ndimage.sum(noise, labeled, range(1, k + 1))
    out += [np.mean(sizes), np.median(sizes), np.max(sizes), np.sum(sizes == 1)]
    out.append(np.sum(noise, axis=0) / np.maximum(np.sum(valid, axis=0), 1))
    t1 = time.perf_counter()
    rough = ndimage.generic_filter(clean.astype(np.float64), lambda x: np.nanstd(x), size=5, mode="constant", cval=np.nan)
    t2 = time.perf_counter()
    out += [np.nanmean(rough[noise & valid]), np.nanmedian(rough[noise & valid]), np.nanmean(rough[(labels == 0) & valid]),
            np.nanmedian(rough[(labels == 0) & valid])]
    t3 = time.perf_counter()
    print(json.dumps({"step": "host", "size": args.size, "cells": int(labels.size), "host_s": round(t3 - t0, 3),
                      "generic_filter_s": round(t2 - t1, 3), "num_clusters": int(k)}), flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--device-size", type=int, default=20000)
    ap.add_argument("--host-size", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--limit", type=int, default=300, help="seconds per step")
    ap.add_argument("--step", choices=["device", "host"], help="run one step in this process")
    ap.add_argument("--size", type=int, default=1024)
    args = ap.parse_args()
    if args.step:
        return (step_device if args.step == "device" else step_host)(args)
    for what, size in (("host", args.host_size), ("device", args.device_size)):
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
