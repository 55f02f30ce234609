#!/usr/bin/env python3
"""The locale guide on the device: the time of ``data.locale_guide_planes`` beside ``RobustSoundingGrid.hypotheses(rule="count")``
of a grid of the same shape, in the same process.

    python tools/measure_locale_guide.py --size 20000      # 4e8 cells, a scattered cloud of 2e8 soundings for the count build
    python tools/measure_locale_guide.py --size 5000

One size per process (each step of a measurement run under a time limit of its own).  The planes of the guide are made in HBM:
``center2`` a sloping seabed with 0.2 m of noise in units of 2^-17 m, and for every ``--shares`` value a pair ``n_hyp`` / ``chosen``
with that share of the cells witnesses.  The count build runs on a ``RobustSoundingGridder`` result of ``--size`` x ``--size``
cells at 0.5 m filled with ``size^2 / 2`` scattered soundings, as in tools/measure_sounding_hypotheses.py.  For every radius and
share the guide and the count build (without records) alternate, HIP events around each call, median / min / max of ``--reps``
after one warm-up call each.

The bytes model, from shapes: the guide reads 16 B per cell and writes 8 B, the halo re-read left out (it stays in L2);
``gbytes_per_s`` is that over the measured time.  ``--full-range`` draws ``center2`` uniformly from +-(2^32 - 1) instead: every
window then spans nearly the whole range and the bisection takes its 33 steps, which is what a bisection that did not start from
the window's min .. max would take on any plane.  It also checks that two runs leave equal bits.  One JSON line."""
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
    ap.add_argument("--radii", type=int, nargs="+", default=[1, 2, 4, 8])
    ap.add_argument("--shares", type=float, nargs="+", default=[0.1, 0.9, 1.0])
    ap.add_argument("--gap", type=float, default=0.5)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--full-range", action="store_true")
    args = ap.parse_args()
    import torch
    from bathymetric_gnn_amd import runtime as rt
    from bathymetric_gnn_amd.data import RobustSoundingGridder, locale_guide_planes
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: this script measures on the device only")
    dev = torch.device("cuda:0")
    S, res = args.size, 0.5
    n = S * S // 2
    x0, y0 = 500000.0, 4000000.0 + S * res
    g = torch.Generator(device=dev).manual_seed(7)
    u = lambda: torch.rand(n, generator=g, device=dev, dtype=torch.float64)
    x, y = x0 + u() * (S * res), y0 - u() * (S * res)
    z = (-30.0 + 2.0 * torch.randn(n, generator=g, device=dev)).contiguous()
    robust = RobustSoundingGridder((S, S), (x0, y0), res, n, device=dev)
    robust.add(x, y, z)
    del x, y, z
    grid = robust.finalize()
    del robust

    rows = torch.arange(S, device=dev, dtype=torch.float32)
    depth = -20.0 - 0.01 * rows[:, None] - 0.004 * rows[None, :] + 0.2 * torch.randn((S, S), generator=g, device=dev)
    center2 = torch.round(depth.double() * 131072.0).to(torch.int64)
    del depth
    if args.full_range:
        center2 = torch.randint(-(2 ** 32 - 1), 2 ** 32, (S, S), generator=g, device=dev, dtype=torch.int64)
    masks = {}
    for share in args.shares:
        w = torch.rand((S, S), generator=g, device=dev) < share
        masks[share] = (torch.where(w, 1, 2).to(torch.int32), torch.zeros((S, S), dtype=torch.int32, device=dev))
        del w

    def timed(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b)

    stat = lambda v: {"ms": round(statistics.median(v), 3), "ms_min": round(min(v), 3), "ms_max": round(max(v), 3), "runs": len(v)}
    count_build = lambda: grid.hypotheses(args.gap, records=False)
    timed(count_build)
    out = {"tool": "measure_locale_guide", "size": S, "cells": S * S, "soundings": n, "gap_m": args.gap, "reps": args.reps, "full_range": args.full_range,
           "build": rt.build_id(), "device": torch.cuda.get_device_name(0), "cases": [], "equal_bits": True}
    count_ms = []
    model = 24 * S * S
    for radius in args.radii:
        for share in args.shares:
            n_hyp, chosen = masks[share]
            min_support = min(3, (2 * radius + 1) ** 2 - 1)
            guide = lambda: locale_guide_planes(n_hyp, chosen, center2, radius, min_support)
            timed(guide)
            ms, beside = [], []
            for _ in range(args.reps):                           # alternating: a drift of the machine touches both alike
                ms.append(timed(guide))
                beside.append(timed(count_build))
            count_ms += beside
            a, b = guide(), guide()
            same = bool(torch.equal(a[0].view(torch.int32), b[0].view(torch.int32))) and bool(torch.equal(a[1], b[1]))
            out["equal_bits"] = out["equal_bits"] and same
            case = {"radius": radius, "share": share, "min_support": min_support, **stat(ms), "count_build_ms": stat(beside)["ms"]}
            case["over_count_build"] = round(case["ms"] / case["count_build_ms"], 3)
            case["gbytes_per_s"] = round(model / case["ms"] / 1e6, 1)
            case["ns_per_cell"] = round(case["ms"] * 1e6 / (S * S), 4)
            case["with_guide"] = int((a[1] >= min_support).sum())
            case["mean_support"] = round(float(a[1].double().mean()), 3)
            del a, b
            out["cases"].append(case)
    out["count_build"] = stat(count_ms)
    print(json.dumps(out), flush=True)
    return 0 if out["equal_bits"] else 1


if __name__ == "__main__":
    sys.exit(main())
