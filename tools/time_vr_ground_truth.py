#!/usr/bin/env python3
"""Native-resolution ground truth from a VR BAG pair: ``bgnn_vr_ground_truth`` against the numpy restatement, on the same machine.

    python tools/time_vr_ground_truth.py                     # about 2.5e7 records
    python tools/time_vr_ground_truth.py --base 40 --copies 4 --reps 5

The pair: ``synthetic_vr_bag(base, base)`` stacked ``--copies`` times along the base grid's rows (each copy's records behind the
one before), as the clean file with the copies' records in reverse order; the noisy file is the same grids in iteration order with
spikes of 0.3 .. 2 m on 3 % of the records and jitter of 0.05 m on 20 %.  One JSON line:

  device      HIP events on the context's stream around ``vr_ground_truth_build`` (table upload, the label pass, the two refinement
              passes of the median, the finishing kernels), records already in HBM: median / minimum / maximum of ``--reps`` runs
              after a warm-up, the 33 B per cell the label pass must move (16 read: an 8-byte noisy record and the 8-byte sector
              share of the clean depth; 17 written) over the median, and the same with the 16 B per cell the two selection passes
              re-read
  upload      host clock around the upload of both record arrays
  numpy_flat  the restatement at its best on the host: one gather of the clean depths into noisy order, then whole-array numpy
              (difference, masks, labels, mean / max / median of the magnitudes), median of three runs
  plan_loop   the plan's own loop over the grids (``iterate_refinements`` of both handlers, a dictionary, per-grid numpy), once
and whether the device's labels and statistics equal the flat restatement's."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def make_pair(np, base, copies, seed=1000):
    from bathymetric_gnn_amd import synthetic
    from bathymetric_gnn_amd.data import VRBagHandler
    md0, ref0 = synthetic.synthetic_vr_bag(base, base, seed=seed)
    n0 = ref0.shape[1]
    refined = md0["dimensions_x"] > 0
    noisy_md, clean_md = [], []
    for r in range(copies):
        a, b = md0.copy(), md0.copy()
        a["index"][refined] += r * n0
        b["index"][refined] += (copies - 1 - r) * n0
        noisy_md.append(a); clean_md.append(b)
    clean_ref = np.tile(ref0, (1, copies))
    noisy_ref = clean_ref.copy()
    rng = np.random.default_rng(seed)
    depth = noisy_ref["depth"][0]
    valid = np.isfinite(depth) & (depth != np.float32(1.0e6))
    u = rng.random(depth.shape[0], dtype=np.float32)
    spike, jitter = valid & (u < 0.03), valid & (u >= 0.03) & (u < 0.23)
    depth[spike] += (rng.choice(np.array([-1, 1], np.float32), int(spike.sum())) * rng.uniform(0.3, 2.0, int(spike.sum()))).astype(np.float32)
    depth[jitter] += rng.uniform(-0.05, 0.05, int(jitter.sum())).astype(np.float32)
    noisy_ref["depth"][0] = depth
    return (VRBagHandler.from_arrays(np.concatenate(clean_md), clean_ref), VRBagHandler.from_arrays(np.concatenate(noisy_md), noisy_ref))


def numpy_flat(np, clean, noisy, pairs, threshold=0.15):
    rows = pairs.rows
    paired = rows["clean_start"] >= 0
    run0 = rows["out_offset"]
    src = np.repeat(np.where(paired, rows["clean_start"], 0) - run0, rows["cells"]) + np.arange(pairs.total, dtype=np.int64)
    cell_paired = np.repeat(paired, rows["cells"])
    nd = noisy.varres_refinements["depth"][0]
    cd = clean.varres_refinements["depth"][0][src]
    nodata = np.float32(1.0e6)
    with np.errstate(invalid="ignore"):
        difference = np.where(cell_paired, nd - cd, np.float32(np.nan))
        valid = cell_paired & np.isfinite(nd) & (nd != nodata) & np.isfinite(cd) & (cd != nodata)
        noise = valid & (np.abs(difference) > threshold)
    labels = np.where(valid, np.where(noise, 2, 0), -1).astype(np.int32)
    mags = np.abs(difference[noise]).astype(np.float64)
    stats = {"valid": int(valid.sum()), "noise": int(noise.sum())}
    if mags.size:
        stats.update(mean=float(np.mean(mags)), max=float(np.max(mags)), median=float(np.median(mags)))
    return labels, stats


def plan_loop(np, clean, noisy, threshold=0.15):
    noisy_grids = {(g.base_row, g.base_col): g for g in noisy.iterate_refinements(min_valid_ratio=0.0)}
    valid_cells = noise_cells = 0
    magnitudes = []
    for cg in clean.iterate_refinements(min_valid_ratio=0.0):
        ng = noisy_grids.get((cg.base_row, cg.base_col))
        if ng is None or cg.dimensions != ng.dimensions:
            continue
        difference = ng.depth - cg.depth
        valid = cg.valid_mask & ng.valid_mask
        labels = np.full(cg.depth.shape, 0, dtype=np.int32)
        noise_mask = np.abs(difference) > threshold
        labels[noise_mask & valid] = 2
        labels[~valid] = -1
        valid_cells += int(np.sum(valid)); noise_cells += int(np.sum(labels == 2))
        if np.any(noise_mask & valid):
            magnitudes.extend(np.abs(difference[noise_mask & valid]).tolist())
    m = np.array(magnitudes)
    return {"valid": valid_cells, "noise": noise_cells, "mean": float(np.mean(m)), "max": float(np.max(m)), "median": float(np.median(m))}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--base", type=int, default=60, help="side of the base grid of one copy")
    ap.add_argument("--copies", type=int, default=12)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--no-plan-loop", action="store_true")
    args = ap.parse_args()
    import numpy as np
    import torch
    from bathymetric_gnn_amd import runtime as rt
    from bathymetric_gnn_amd.data import vr_pair_table
    from bathymetric_gnn_amd.data.vr_ground_truth import _records_to_device, vr_ground_truth_build
    dev = torch.device("cuda:0")
    ctx = rt.get_context(dev)
    clean, noisy = make_pair(np, args.base, args.copies)
    t0 = time.perf_counter()
    pairs = vr_pair_table(clean, noisy)
    t_table = (time.perf_counter() - t0) * 1e3
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    noisy_rec, clean_rec = _records_to_device(noisy, dev), _records_to_device(clean, dev)
    torch.cuda.synchronize()
    t_upload = (time.perf_counter() - t0) * 1e3
    build = lambda: vr_ground_truth_build(noisy_rec, clean_rec, pairs.rows, pairs.total, 0.15, 1.0e6, ctx=ctx)
    out = build()
    busy = torch.randn(4096, 4096, device=dev)
    sink = torch.empty_like(busy)
    torch.cuda.synchronize()
    ms = []
    for _ in range(args.reps):           # (a matrix product in front keeps the stream busy while the host enqueues the call)
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        with torch.cuda.stream(ctx.stream):
            torch.mm(busy, busy, out=sink)
        a.record(ctx.stream)
        out = build()
        b.record(ctx.stream)
        b.synchronize()
        ms.append(a.elapsed_time(b))
    torch.cuda.synchronize()
    med = statistics.median(ms)
    cells = pairs.total
    block = np.frombuffer(out[6].cpu().numpy().tobytes(), dtype=np.dtype(rt.VT_STATS_DTYPE))[0]
    flat_ms = []
    for _ in range(3):
        t0 = time.perf_counter()
        labels, stats = numpy_flat(np, clean, noisy, pairs)
        flat_ms.append((time.perf_counter() - t0) * 1e3)
    equal = bool(np.array_equal(out[0].cpu().numpy(), labels)) and int(block["valid"]) == stats["valid"] and \
        int(block["noise"]) == stats["noise"] and float(block["noise_abs_median"]) == stats.get("median") and \
        float(block["noise_abs_max"]) == stats.get("max")
    res = {"build": rt.build_id(), "records": int(noisy_rec.shape[0]), "cells": cells, "grids": int(len(pairs.rows)),
           "paired_grids": int(pairs.paired.sum()), "noise_cells": stats["noise"], "reps": args.reps,
           "pair_table_ms": round(t_table, 2), "upload_ms": round(t_upload, 2),
           "device": {"median_ms": round(med, 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4),
                      "label_pass_mbytes": round(33 * cells / 1e6, 1), "gbytes_per_s_33B": round(33 * cells / med / 1e6, 1),
                      "gbytes_per_s_49B": round(49 * cells / med / 1e6, 1)},
           "numpy_flat": {"median_ms": round(statistics.median(flat_ms), 1), "min_ms": round(min(flat_ms), 1)},
           "equal": equal}
    if not args.no_plan_loop:
        t0 = time.perf_counter()
        loop = plan_loop(np, clean, noisy)
        res["plan_loop"] = {"ms": round((time.perf_counter() - t0) * 1e3, 1),
                            "equal": loop["valid"] == stats["valid"] and loop["noise"] == stats["noise"] and
                            loop["median"] == stats["median"] and loop["max"] == stats["max"]}
    print(json.dumps(res), flush=True)
    return 0 if equal else 1


if __name__ == "__main__":
    sys.exit(main())
