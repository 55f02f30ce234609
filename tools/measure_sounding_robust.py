#!/usr/bin/env python3
"""Robust gridding of soundings on the device: the time of ``RobustSoundingGridder.add`` + ``finalize`` and of the flag pass at
survey size, beside ``SoundingGridder.add`` + ``finalize`` on the same cloud and a plain read of the bytes the robust path must
move at least.

    python tools/measure_sounding_robust.py --case scattered --size 20000      # 2e8 soundings on 20000 x 20000 cells
    python tools/measure_sounding_robust.py --case swath --size 5000           # 8 per cell, in swath order
    python tools/measure_sounding_robust.py --case one_cell --n 16777216       # the single-workgroup radix path
    python tools/measure_sounding_robust.py --case flag --size 5000            # the flag pass over the cloud that was gridded

One case per process (each step of a measurement run under a time limit of its own).  The cloud of ``--n`` soundings is built in
HBM over a ``--size`` x ``--size`` grid at 0.5 m:

  scattered   every sounding in a cell drawn uniformly
  swath       raster order, ``n / cells`` consecutive soundings per cell (at least 4; four at half a sounding per cell, as in
              tools/measure_sounding_grid.py)
  one_cell    every sounding in one cell of an 8 x 8 grid: one workgroup sorts it all
  flag        the scattered cloud gridded once (not timed), then ``flag`` over all of it

HIP events around each call, median / min / max of ``--reps`` after one warm-up round, the calls alternating.  ``read_floor`` is
``x.sum() + y.sum() + z.sum()`` over the cloud (20 B per sounding) plus, for add + finalize, a sum over a ``2 n`` int32 tensor and a
copy of an ``n`` int32 tensor (the 8 B the stage is read back with, and 4 + 4 B of the sort); the flag pass's floor is the 20 B read
alone.  The memory the robust path moves at least: 20 B read and 8 B written in add, 8 + 4 in the scatter, 4 + 4 in the sort,
per sounding; 4 B per cell three times over in the scan and 49 B per cell of planes and ``start`` written.  It also checks that two
runs leave equal bits and that ``count`` equals the first gridder's.  One JSON line."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--case", choices=("scattered", "swath", "one_cell", "flag"), required=True)
    ap.add_argument("--n", type=int, default=200_000_000)
    ap.add_argument("--size", type=int, default=20000)
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    import torch
    from bathymetric_gnn_amd import runtime as rt
    from bathymetric_gnn_amd.data import RobustSoundingGridder, SoundingGridder
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: this script measures on the device only")
    dev = torch.device("cuda:0")
    n, res = args.n, 0.5
    S = 8 if args.case == "one_cell" else args.size
    x0, y0 = 500000.0, 4000000.0 + S * res
    g = torch.Generator(device=dev).manual_seed(7)
    u = lambda: torch.rand(n, generator=g, device=dev, dtype=torch.float64)
    z = (-30.0 + 2.0 * torch.randn(n, generator=g, device=dev)).contiguous()
    if args.case in ("scattered", "flag"):
        x, y = x0 + u() * (S * res), y0 - u() * (S * res)
    elif args.case == "swath":
        run = max(4, n // (S * S))
        cell = torch.arange(n, device=dev, dtype=torch.int64) // run % (S * S)
        x, y = x0 + ((cell % S).double() + 0.05 + 0.9 * u()) * res, y0 - ((cell // S).double() + 0.05 + 0.9 * u()) * res
        del cell
    else:
        x, y = x0 + (S // 2 + 0.05 + 0.9 * u()) * res, y0 - (S // 3 + 0.05 + 0.9 * u()) * res
    robust = RobustSoundingGridder((S, S), (x0, y0), res, n, device=dev)
    first = SoundingGridder((S, S), (x0, y0), res, device=dev)

    def timed(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b)

    def robust_add():
        robust.reset()
        return timed(lambda: robust.add(x, y, z))

    def first_add():
        first.reset()
        return timed(lambda: first.add(x, y, z))

    pairs = torch.zeros(2 * n, dtype=torch.int32, device=dev)
    words, words_out = torch.zeros(n, dtype=torch.int32, device=dev), torch.empty(n, dtype=torch.int32, device=dev)
    read20 = lambda: float(x.sum() + y.sum() + z.sum())
    floor_all = lambda: (read20(), int(pairs.sum()), words_out.copy_(words))
    out = {"tool": "measure_sounding_robust", "case": args.case, "n": n, "size": S, "soundings_per_cell": round(n / (S * S), 3),
           "resolution": res, "reps": args.reps, "build": rt.build_id(), "device": torch.cuda.get_device_name(0),
           "wave_max": rt.ROBUST_WAVE_MAX, "lds_max": rt.ROBUST_LDS_MAX, "stage_gbytes": round(8 * n / 1e9, 2)}
    stat = lambda v: {"ms": round(statistics.median(v), 3), "ms_min": round(min(v), 3), "ms_max": round(max(v), 3), "runs": len(v)}
    if args.case == "flag":
        robust.add(x, y, z)
        grid = robust.finalize()
        robust.flag(x, y, z, grid)
        read20()
        ms = {"flag": [], "read_floor": []}
        for _ in range(args.reps):
            ms["flag"].append(timed(lambda: robust.flag(x, y, z, grid)))
            ms["read_floor"].append(timed(read20))
        out.update({k: stat(v) for k, v in ms.items()})
        out["flag"]["gbytes_per_s"] = round(21 * n / out["flag"]["ms"] / 1e6, 1)
        out["flag_over_floor"] = round(out["flag"]["ms"] / out["read_floor"]["ms"], 2)
        flags = robust.flag(x, y, z, grid)
        out["flag_counts"] = [int((flags == v).sum()) for v in (0, 1, 2)]
        out["flags_add_up"] = out["flag_counts"][1] == int((grid.count - grid.kept).sum(dtype=torch.int64))
        print(json.dumps(out), flush=True)
        return 0
    reps = args.reps
    robust_add(); first_add(); floor_all()                      # warm every shape the timed window uses
    warm = timed(robust.finalize)
    first.finalize()
    if args.case == "one_cell" and warm > 5000.0:
        reps = 1                                                 # (the single-workgroup path: one timed run is enough beside the warm one)
    out["robust_finalize_warm_ms"] = round(warm, 3)
    ms = {k: [] for k in ("robust_add", "robust_finalize", "first_add", "first_finalize", "read_floor")}
    for _ in range(reps):                                        # alternating: a drift of the machine touches every call alike
        ms["robust_add"].append(robust_add())
        ms["robust_finalize"].append(timed(robust.finalize))
        ms["first_add"].append(first_add())
        ms["first_finalize"].append(timed(first.finalize))
        ms["read_floor"].append(timed(floor_all))
    out.update({k: stat(v) for k, v in ms.items()})
    out["robust_add_plus_finalize_ms"] = round(out["robust_add"]["ms"] + out["robust_finalize"]["ms"], 3)
    out["first_add_plus_finalize_ms"] = round(out["first_add"]["ms"] + out["first_finalize"]["ms"], 3)
    out["robust_over_first"] = round(out["robust_add_plus_finalize_ms"] / out["first_add_plus_finalize_ms"], 2)
    out["robust_over_floor"] = round(out["robust_add_plus_finalize_ms"] / out["read_floor"]["ms"], 2)
    out["robust_add"]["gbytes_per_s"] = round(28 * n / out["robust_add"]["ms"] / 1e6, 1)
    a, b = robust.finalize(), robust.finalize()
    keys = ("count", "kept", "median", "mad", "kept_mean", "kept_std", "kept_min", "kept_max", "valid", "center2", "limit", "start")
    accepted = a.counters["accepted"]
    out["equal_bits"] = all(bool(torch.equal(getattr(a, k), getattr(b, k))) for k in keys) and \
        bool(torch.equal(a.sorted_q[:accepted], b.sorted_q[:accepted]))
    out["count_equals_first"] = bool(torch.equal(a.count, first.finalize().count))
    out["counters"] = a.counters
    out["rejected"] = int((a.count - a.kept).sum(dtype=torch.int64))
    out["cells_over_wave_max"] = int((a.count > rt.ROBUST_WAVE_MAX).sum())
    print(json.dumps(out), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
