#!/usr/bin/env python3
"""Ground truth from a survey pair and model evaluation, device against numpy on the same machine.

    python tools/time_ground_truth.py                        # 4096^2 and 20000^2, uniform and clustered, truth and evaluation
    python tools/time_ground_truth.py --sizes 4096 --no-numpy

Every measurement is a step of its own: a child process (``--step``) under a time limit (``--limit`` seconds), one JSON line
each; the first step that fails or runs out of time ends the run.  A step

  truth  builds an S x S clean / noisy pair in HBM (``uniform``: differences spread evenly over +-1 m; ``clustered``: sigma = 1 cm
         around a 37 cm offset with 1 % outliers -- nearly every cell falls into two bins of the first histogram), times
         ``ground_truth_build`` from the HBM planes to labels (HIP events, median of ``--reps``), and, unless ``--no-numpy``,
         the same arithmetic in numpy on the planes copied to the host, and compares offset and labels.
         ``gbytes_per_s`` is the call's compulsory traffic over its time: 8 B read + 4 B written per cell by the first pass, 4 B
         read by each of the two refining passes, 4 B read + 8 B written by the labelling pass (+ 8 B with an uncertainty plane)
  eval   times ``Evaluator.add`` + ``metrics()`` on S x S device planes (12 B per cell) against the reference's formula in numpy.

For the time of each kernel, run one step under ``rocprofv3 --kernel-trace --stats -- python tools/time_ground_truth.py --step ...``.
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


def make_pair(torch, size, dist, device, seed=3):
    g = torch.Generator(device=device).manual_seed(seed)
    shape = (size, size)
    clean = -30 + 5 * torch.randn(shape, generator=g, device=device)
    if dist == "uniform":
        d = 2 * torch.rand(shape, generator=g, device=device) - 1
    else:
        d = 0.37 + 0.01 * torch.randn(shape, generator=g, device=device)
        out = torch.rand(shape, generator=g, device=device) < 0.01
        d = torch.where(out, d + (torch.rand(shape, generator=g, device=device) * 5 - 2.5), d)
    noisy = clean + d
    del d
    noisy[torch.rand(shape, generator=g, device=device) < 0.02] = float("nan")
    clean[torch.rand(shape, generator=g, device=device) < 0.02] = 1.0e6
    unc = torch.rand(shape, generator=g, device=device)
    return clean, noisy, unc


def timed(torch, fn, reps):
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
    return statistics.median(ms), min(ms)


def step_truth(args):
    import numpy as np
    import torch
    from bathymetric_gnn_amd import runtime as rt
    from bathymetric_gnn_amd.data.ground_truth import ground_truth_build
    dev = torch.device("cuda:0")
    clean, noisy, unc = make_pair(torch, args.size, args.dist, dev)
    cells = clean.numel()
    out = {"step": "truth", "size": args.size, "dist": args.dist, "cells": cells, "build": rt.build_id()}
    for label, u, per_cell in (("", None, 32), ("_with_uncertainty", unc, 40)):
        med, best = timed(torch, lambda: ground_truth_build(clean, noisy, u, 0.15), args.reps)
        out["device_ms" + label], out["device_ms_min" + label] = round(med, 3), round(best, 3)
        out["gbytes_per_s" + label] = round(per_cell * cells / med / 1e6, 1)
    labels, diff, _, stats = ground_truth_build(clean, noisy, None, 0.15)
    block = np.frombuffer(stats.cpu().numpy().tobytes(), np.dtype(rt.GT_STATS_DTYPE))[0]
    out["offset"], out["valid"], out["noise"] = float(block["offset"]), int(block["valid"]), int(block["noise"])
    if not args.no_numpy:
        c, z = clean.cpu().numpy(), noisy.cpu().numpy()
        t0 = time.perf_counter()
        raw = z - c
        valid = (c != 1.0e6) & np.isfinite(c) & (z != 1.0e6) & np.isfinite(z)
        t1 = time.perf_counter()
        offset = np.median(raw[valid])
        t2 = time.perf_counter()
        d = raw - offset
        lab = np.full(c.shape, 0, dtype=np.int32)
        with np.errstate(invalid="ignore"):
            lab[(np.abs(d) > 0.15) & valid] = 2
        lab[~valid] = -1
        d[~valid] = np.nan
        t3 = time.perf_counter()
        out["numpy_ms"], out["numpy_median_ms"] = round((t3 - t0) * 1e3, 1), round((t2 - t1) * 1e3, 1)
        out["speedup"] = round(out["numpy_ms"] / out["device_ms"], 1)
        out["offset_equal"] = bool(np.float32(block["offset"]) == offset)
        out["labels_equal"] = bool(np.array_equal(labels.cpu().numpy(), lab))
    print(json.dumps(out), flush=True)


def numpy_metrics(y_true, y_pred, confidence):
    """The reference's compute_metrics arithmetic (per-class masks, a 3 x 3 matrix of mask sums, confidence statistics)."""
    import numpy as np
    valid = (y_true >= 0) & (y_pred >= 0) & np.isfinite(y_pred)
    y_true, y_pred, confidence = y_true[valid].astype(np.int32), y_pred[valid].astype(np.int32), confidence[valid]
    m = {"total_samples": int(len(y_true)), "overall_accuracy": float(np.mean(y_true == y_pred))}
    for k in range(3):
        tp = np.sum((y_true == k) & (y_pred == k)); fp = np.sum((y_true != k) & (y_pred == k)); fn = np.sum((y_true == k) & (y_pred != k))
        m[k] = (int(tp), int(fp), int(fn), int(np.sum(y_true == k)))
    m["confusion_matrix"] = [[int(np.sum((y_true == i) & (y_pred == j))) for j in range(3)] for i in range(3)]
    correct = y_true == y_pred
    m["confidence"] = [float(np.mean(confidence)), float(np.std(confidence)), float(np.mean(confidence[correct])),
                       float(np.mean(confidence[~correct]))]
    for t in (0.5, 0.6, 0.7, 0.8, 0.9):
        mask = confidence >= t
        if np.sum(mask) > 0:
            m["confidence"] += [float(np.mean(y_true[mask] == y_pred[mask])), float(np.mean(mask))]
    return m


def step_eval(args):
    import torch
    from bathymetric_gnn_amd import runtime as rt
    from bathymetric_gnn_amd.training import Evaluator
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(5)
    shape = (args.size, args.size)
    labels = torch.randint(-1, 3, shape, generator=g, device=dev, dtype=torch.int32)
    pred = torch.where(torch.rand(shape, generator=g, device=dev) < 0.85, labels.clamp(min=0),
                       torch.randint(0, 3, shape, generator=g, device=dev, dtype=torch.int32)).to(torch.float32)
    pred[torch.rand(shape, generator=g, device=dev) < 0.03] = float("nan")
    conf = torch.rand(shape, generator=g, device=dev)
    ev = Evaluator(dev)
    result = {}

    def run():
        ev.reset()
        ev.add(labels, pred, conf)
        result["m"] = ev.metrics()
    run()
    wall = []
    for _ in range(args.reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        run()
        wall.append((time.perf_counter() - t0) * 1e3)
    add_ms, _ = timed(torch, lambda: ev.add(labels, pred, conf), args.reps)
    cells = labels.numel()
    out = {"step": "eval", "size": args.size, "cells": cells, "build": rt.build_id(), "add_device_ms": round(add_ms, 3),
           "gbytes_per_s": round(12 * cells / add_ms / 1e6, 1), "add_and_metrics_wall_ms": round(statistics.median(wall), 3),
           "total_samples": result["m"]["total_samples"]}
    if not args.no_numpy:
        y, p, c = labels.cpu().numpy(), pred.cpu().numpy(), conf.cpu().numpy()
        t0 = time.perf_counter()
        import numpy as np
        with np.errstate(invalid="ignore"):
            ref = numpy_metrics(y, p, c)
        out["numpy_ms"] = round((time.perf_counter() - t0) * 1e3, 1)
        out["speedup"] = round(out["numpy_ms"] / out["add_and_metrics_wall_ms"], 1)
        out["integers_equal"] = bool(ref["total_samples"] == result["m"]["total_samples"] and
                                     ref["confusion_matrix"] == result["m"]["confusion_matrix"] and
                                     ref["overall_accuracy"] == result["m"]["overall_accuracy"])
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--sizes", type=int, nargs="+", default=[4096, 20000])
    ap.add_argument("--dists", nargs="+", default=["uniform", "clustered"], choices=["uniform", "clustered"])
    ap.add_argument("--what", nargs="+", default=["truth", "eval"], choices=["truth", "eval"])
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--limit", type=int, default=240, help="seconds per step")
    ap.add_argument("--no-numpy", action="store_true")
    ap.add_argument("--step", choices=["truth", "eval"], help="run one step in this process")
    ap.add_argument("--size", type=int, default=4096)
    ap.add_argument("--dist", default="clustered", choices=["uniform", "clustered"])
    args = ap.parse_args()
    if args.step:
        return (step_truth if args.step == "truth" else step_eval)(args)
    steps = [("truth", s, d) for s in args.sizes for d in args.dists if "truth" in args.what]
    steps += [("eval", s, "clustered") for s in args.sizes if "eval" in args.what]
    for what, size, dist in steps:
        cmd = [sys.executable, os.path.abspath(__file__), "--step", what, "--size", str(size), "--dist", dist, "--reps", str(args.reps)]
        cmd += ["--no-numpy"] if args.no_numpy else []
        try:
            r = subprocess.run(cmd, timeout=args.limit)
        except subprocess.TimeoutExpired:
            print(json.dumps({"step": what, "size": size, "dist": dist, "error": f"no result within {args.limit} s"}), flush=True)
            return 1
        if r.returncode != 0:
            print(json.dumps({"step": what, "size": size, "dist": dist, "error": f"exit status {r.returncode}"}), flush=True)
            return 1
    return 0


if __name__ == "__main__":
    sys.exit(main())
