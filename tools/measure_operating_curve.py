#!/usr/bin/env python3
"""Operating curves on the device: the time of one pass over survey-sized planes, beside the evaluation pass on the same planes.

    python tools/measure_operating_curve.py                  # 20000 x 20000, 101 thresholds
    python tools/measure_operating_curve.py --size 4096 --reps 10

Builds an S x S synthetic ground truth (labels, difference) and prediction (classification, confidence, correction) in HBM and
times, in one process and alternating between them (HIP events around each call, median / min / max of ``--reps``):

  curve          ``OperatingCurve.add`` with the residual planes (20 B per cell), confidences spread evenly over [0, 1)
  evaluator      ``Evaluator.add`` on the same labels, classification and confidence (12 B per cell)
  curve_equal    ``OperatingCurve.add`` with every confidence on one value (0.99): every lane of a wave on one histogram entry
  curve_cluster  ``OperatingCurve.add`` with nine confidences in ten on 0.99 and the rest spread (what a trained model gives)
  curve_bare     ``OperatingCurve.add`` without the residual planes (12 B per cell)

``gbytes_per_s`` is the call's compulsory traffic over its median time.  The expectation the figures are read against:
curve / evaluator near 20 / 12, up to 1.5 x that for LDS-atomic conflicts; curve_equal within 3 x curve.  The script reports the
ratios and does not judge them.  It also checks that two runs leave equal bits and that the curve's totals are the evaluator's.
One JSON line.  For the time of the kernel alone, run it under ``rocprofv3 --kernel-trace --stats -- python tools/...``.
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--size", type=int, default=20000)
    ap.add_argument("--thresholds", type=int, default=101)
    ap.add_argument("--reps", type=int, default=20)
    args = ap.parse_args()
    import numpy as np
    import torch
    from bathymetric_gnn_amd import runtime as rt
    from bathymetric_gnn_amd.training import Evaluator, OperatingCurve
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: this script measures on the device only")
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(7)
    shape = (args.size, args.size)
    labels = torch.randint(-1, 3, shape, generator=g, device=dev, dtype=torch.int32)
    pred = torch.where(torch.rand(shape, generator=g, device=dev) < 0.85, labels.clamp(min=0),
                       torch.randint(0, 3, shape, generator=g, device=dev, dtype=torch.int32)).to(torch.float32)
    pred[torch.rand(shape, generator=g, device=dev) < 0.03] = float("nan")
    conf = torch.rand(shape, generator=g, device=dev)
    diff = 0.4 * torch.randn(shape, generator=g, device=dev)
    diff[labels < 0] = float("nan")
    corr = (diff * torch.rand(shape, generator=g, device=dev)).nan_to_num_(0.0)
    conf_equal = torch.full(shape, 0.99, device=dev)
    conf_cluster = torch.where(torch.rand(shape, generator=g, device=dev) < 0.9, conf_equal, conf)
    thr = np.linspace(0, 1, args.thresholds).astype(np.float32)
    oc, ev = OperatingCurve(thr, dev), Evaluator(dev)
    calls = {
        "curve": (lambda: oc.add(labels, pred, conf, diff, corr), 20),
        "evaluator": (lambda: ev.add(labels, pred, conf), 12),
        "curve_equal": (lambda: oc.add(labels, pred, conf_equal, diff, corr), 20),
        "curve_cluster": (lambda: oc.add(labels, pred, conf_cluster, diff, corr), 20),
        "curve_bare": (lambda: oc.add(labels, pred, conf), 12),
    }
    for fn, _ in calls.values():                                # warm every shape the timed window uses
        fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in calls}
    for _ in range(args.reps):                                  # alternating: a drift of the machine touches every call alike
        for name, (fn, _) in calls.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            ms[name].append(a.elapsed_time(b))
    cells = labels.numel()
    out = {"tool": "measure_operating_curve", "size": args.size, "cells": cells, "thresholds": int(thr.size), "reps": args.reps,
           "build": rt.build_id(), "device": torch.cuda.get_device_name(0)}
    for name, (_, per_cell) in calls.items():
        med = statistics.median(ms[name])
        out[name] = {"ms": round(med, 3), "ms_min": round(min(ms[name]), 3), "ms_max": round(max(ms[name]), 3),
                     "gbytes_per_s": round(per_cell * cells / med / 1e6, 1)}
    out["curve_over_evaluator"] = round(out["curve"]["ms"] / out["evaluator"]["ms"], 3)
    out["equal_over_curve"] = round(out["curve_equal"]["ms"] / out["curve"]["ms"], 3)
    out["cluster_over_curve"] = round(out["curve_cluster"]["ms"] / out["curve"]["ms"], 3)
    # results: equal bits from two runs, and the totals of the evaluation
    blocks = []
    for _ in range(2):
        oc.reset()
        oc.add(labels, pred, conf, diff, corr)
        blocks.append(oc._block.clone())
    ev.reset()
    ev.add(labels, pred, conf)
    curve, eb = oc.curve(), ev.block()
    out["equal_bits"] = bool(torch.equal(blocks[0], blocks[1]))
    out["totals_equal_evaluator"] = bool(curve["total"] == int(eb["total"]) and
                                         np.array_equal(np.array(curve["confusion_matrix"]), eb["confusion"]))
    out["total"], out["mae_before"], out["mae_after_at_0.5"] = curve["total"], curve["residual"]["mae_before"], \
        curve["residual"]["mae_after"][int(np.argmin(np.abs(thr - 0.5)))]
    print(json.dumps(out), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
