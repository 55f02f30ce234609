#!/usr/bin/env python3
"""BASELINE config 4 through the drop-in API on HOST arrays: a synthetic varres_metadata / varres_refinements pair (refinement
grids 3x3 .. 50x50) through
  * NativeVRProcessor.process_refinements (records resident in HBM, chunks in flight on two contexts) at several chunk sizes,
  * run_refinements: synchronous (the reference's control flow), the pipelined grid loop (coalesced submissions), and its default
    for a VRBagHandler (routed to process_refinements), with and without a results sink,
  * with ``--sidecar-res R [R ...]`` (raster pixel sizes in metres; a base cell is 64 m): the routed run painting a SidecarBuilder on
    the device, the routed run feeding a host SidecarBuilder as results sink, and the device run plus the download of the four
    planes (``planes()``).  ``--only-sidecar`` skips every other line except "run_refinements default (routed)", the baseline.
Wall clock includes H2D of the records and D2H of the corrected records; the output writer is opened before the clock."""
import argparse, json, os, sys, time
import numpy as np, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from bathymetric_gnn_amd import synthetic
from bathymetric_gnn_amd.data import GraphBuilder, SidecarBuilder, VRBagHandler
from bathymetric_gnn_amd.models import BathymetricGNN
from bathymetric_gnn_amd.scripts.inference_native import NativeVRProcessor, run_refinements

ap = argparse.ArgumentParser()
ap.add_argument("--base", type=int, nargs="+", default=[28, 70], help="base grid is base x base cells (28 -> 676 grids, 70 -> ~4 100)")
ap.add_argument("--chunks", type=int, nargs="+", default=[0, 64 << 10, 128 << 10, 256 << 10, 512 << 10, 1 << 20, 8 << 20],
                help="cell budgets of process_refinements to sweep (0 = its automatic choice)")
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--sidecar-res", type=float, nargs="*", default=[], help="raster pixel sizes (m) of the sidecar lines; a base cell is 64 m")
ap.add_argument("--only-sidecar", action="store_true", help="only the routed baseline and the sidecar lines")
args = ap.parse_args()
sd = synthetic.synthetic_state_dict(in_channels=8, seed=1234)
m = BathymetricGNN(in_channels=8, edge_dim=3, dropout=0.0); m.load_state_dict({k: torch.as_tensor(v) for k, v in sd.items()})
proc = NativeVRProcessor(m.to("cuda:0").eval(), GraphBuilder(), torch.device("cuda:0"))


def timed(fn, h, prep=None):
    walls, st = [], None
    for _ in range(args.reps + 1):                    # (the first repetition grows the pinned staging buffers)
        w = h.copy_and_open_for_writing()
        extra = () if prep is None else (prep(),)     # (a fresh sidecar builder: made before the clock, like the writer)
        torch.cuda.synchronize(); t0 = time.perf_counter()
        st = fn(h, w, *extra)
        torch.cuda.synchronize(); walls.append(time.perf_counter() - t0)
    best = min(walls[1:])
    return {"best_ms": 1e3 * best, "median_ms": 1e3 * float(np.median(walls[1:])), "max_ms": 1e3 * max(walls[1:]),
            "all_ms": [round(1e3 * t, 3) for t in walls[1:]], "M_nodes_per_s": st["cells_processed"] / best / 1e6}, w


BASE_CELL_M = 64.0


def sidecar_lines(out, h, base):
    """Three lines per raster resolution.  The planes of the device run and of the host builder are compared once, outside the clock."""
    for res in args.sidecar_res:
        px = int(BASE_CELL_M / res)
        shape, gt = (base * px, base * px), (0.0, res, 0.0, base * BASE_CELL_M, 0.0, -res)
        mk = lambda: SidecarBuilder.from_georef(h, shape, gt)
        key = f"sidecar res={res:g}"
        out[f"{key}: routed + device sidecar"], _ = timed(lambda h, w, sb: run_refinements(proc, h, w, 0.0, sidecar=sb), h, mk)
        out[f"{key}: routed + host builder as sink"], _ = timed(
            lambda h, w, sb: run_refinements(proc, h, w, 0.0, results_sink=sb.add_refinement_results), h, mk)

        def dev_and_download(h, w, sb):
            st = run_refinements(proc, h, w, 0.0, sidecar=sb)
            sb.planes()
            return st
        out[f"{key}: device sidecar + planes() download"], _ = timed(dev_and_download, h, mk)
        a, b = mk(), mk()
        run_refinements(proc, h, h.copy_and_open_for_writing(), 0.0, sidecar=a)
        run_refinements(proc, h, h.copy_and_open_for_writing(), 0.0, results_sink=b.add_refinement_results)
        pa, pb = a.planes(), b.planes()
        tab = h.refinement_table()
        row0, col0, scale = a.placement(tab)
        r_lo, r_hi = np.clip(row0, 0, shape[0]), np.clip(row0 + tab["dims_y"] * scale, 0, shape[0])
        c_lo, c_hi = np.clip(col0, 0, shape[1]), np.clip(col0 + tab["dims_x"] * scale, 0, shape[1])
        out[f"{key}: raster"] = {"shape": list(shape), "raster_pixels": shape[0] * shape[1],
                                 "footprint_pixels": int(((r_hi - r_lo) * (c_hi - c_lo)).sum()),
                                 "painted_pixels": int((~np.isnan(pa[0])).sum()),
                                 "device_equals_host": bool(np.array_equal(pa.view(np.uint32), pb.view(np.uint32)))}


for base in args.base:
    md, ref = synthetic.synthetic_vr_bag(base, base, seed=4242)
    h = VRBagHandler.from_arrays(md, ref)
    out = {"base": base, "grids": h.num_refinement_cells, "cells": h.total_refinement_nodes}
    if args.only_sidecar:
        out["run_refinements default (routed)"], _ = timed(lambda h, w: run_refinements(proc, h, w, 0.0), h)
        sidecar_lines(out, h, base)
        print(json.dumps(out), flush=True)
        continue
    for c in args.chunks:
        out[f"process_refinements chunk={c or 'auto'}"], w_dev = timed(lambda h, w: proc.process_refinements(h, w, 0.0, cell_budget=c or None), h)
    out["run_refinements synchronous"], w_sync = timed(lambda h, w: run_refinements(proc, h, w, 0.0, pipelined=False), h)
    out["run_refinements pipelined loop"], w_loop = timed(lambda h, w: run_refinements(proc, h, w, 0.0, records_resident=False), h)
    out["run_refinements default (routed)"], w_def = timed(lambda h, w: run_refinements(proc, h, w, 0.0), h)
    n_sink = [0]
    def sink(g, a, b, c):
        n_sink[0] += 1
    out["run_refinements default + sink"], _ = timed(lambda h, w: run_refinements(proc, h, w, 0.0, results_sink=sink), h)
    out["run_refinements loop + sink"], _ = timed(lambda h, w: run_refinements(proc, h, w, 0.0, results_sink=sink, records_resident=False), h)
    out["records_equal"] = bool(np.array_equal(w_dev.refinements.view(np.uint32), w_sync.refinements.view(np.uint32)) and
                                np.array_equal(w_loop.refinements.view(np.uint32), w_sync.refinements.view(np.uint32)) and
                                np.array_equal(w_def.refinements.view(np.uint32), w_sync.refinements.view(np.uint32)))
    sidecar_lines(out, h, base)
    print(json.dumps(out), flush=True)
