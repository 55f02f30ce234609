#!/usr/bin/env python3
"""Depth hypotheses per cell on the device: the time of ``RobustSoundingGrid.hypotheses`` beside ``RobustSoundingGridder.finalize``
of the same gridder, in the same process, on the clouds of tools/measure_sounding_robust.py.

    python tools/measure_sounding_hypotheses.py --case scattered --size 20000      # 2e8 soundings on 20000 x 20000 cells
    python tools/measure_sounding_hypotheses.py --case swath --size 5000           # 8 per cell, in swath order
    python tools/measure_sounding_hypotheses.py --case one_cell --n 16777216       # one cell: one workgroup walks it all

One case per process (each step of a measurement run under a time limit of its own).  The cloud of ``--n`` soundings is built in
HBM over a ``--size`` x ``--size`` grid at 0.5 m as there (scattered, swath, one_cell), added once (not timed) and finalized;
then ``finalize`` and the four forms of ``hypotheses(--gap)`` -- by count and by guide (the guide: the grid's own ``median``), with
and without records -- alternate, HIP events around each call, median / min / max of ``--reps`` after one warm-up round.

The bytes model, from shapes: the pass reads 4 B per accepted sounding and 8 B per cell (``start`` twice over), 4 B per cell more
with a guide, and writes 57 B per cell of planes and 8 B per hypothesis of records.  ``gbytes_per_s`` is that over the measured
time, ``of_copy`` its fraction of a plain device copy's rate (read + write) measured in the same process.  It also checks that two
runs leave equal bits, that the planes are the same with and without records, and that every sounding lies in one hypothesis.
One JSON line."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PLANES = ("n_hyp", "chosen", "kept", "depth", "std", "min", "max", "share", "valid", "center2", "limit")


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--case", choices=("scattered", "swath", "one_cell"), required=True)
    ap.add_argument("--n", type=int, default=200_000_000)
    ap.add_argument("--size", type=int, default=20000)
    ap.add_argument("--gap", type=float, default=0.5)
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    import torch
    from bathymetric_gnn_amd import runtime as rt
    from bathymetric_gnn_amd.data import RobustSoundingGridder
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: this script measures on the device only")
    dev = torch.device("cuda:0")
    n, res = args.n, 0.5
    S = 8 if args.case == "one_cell" else args.size
    x0, y0 = 500000.0, 4000000.0 + S * res
    g = torch.Generator(device=dev).manual_seed(7)
    u = lambda: torch.rand(n, generator=g, device=dev, dtype=torch.float64)
    z = (-30.0 + 2.0 * torch.randn(n, generator=g, device=dev)).contiguous()
    if args.case == "scattered":
        x, y = x0 + u() * (S * res), y0 - u() * (S * res)
    elif args.case == "swath":
        run = max(4, n // (S * S))
        cell = torch.arange(n, device=dev, dtype=torch.int64) // run % (S * S)
        x, y = x0 + ((cell % S).double() + 0.05 + 0.9 * u()) * res, y0 - ((cell // S).double() + 0.05 + 0.9 * u()) * res
        del cell
    else:
        x, y = x0 + (S // 2 + 0.05 + 0.9 * u()) * res, y0 - (S // 3 + 0.05 + 0.9 * u()) * res
    robust = RobustSoundingGridder((S, S), (x0, y0), res, n, device=dev)
    robust.add(x, y, z)
    del x, y, z

    def timed(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b)

    warm = timed(robust.finalize)
    grid = robust.finalize()
    guide = grid.median
    forms = {"count": dict(records=False), "count_records": dict(records=True),
             "guide": dict(rule="guide", guide=guide, records=False), "guide_records": dict(rule="guide", guide=guide, records=True)}
    for kw in forms.values():
        grid.hypotheses(args.gap, **kw)
    words = 1 << 28                                              # a 1 GiB copy: 2 GiB moved
    src, dst = torch.zeros(words, dtype=torch.int32, device=dev), torch.empty(words, dtype=torch.int32, device=dev)
    dst.copy_(src)
    reps = 1 if args.case == "one_cell" and warm > 5000.0 else args.reps
    ms = {k: [] for k in ["finalize", "copy"] + list(forms)}
    for _ in range(reps):                                        # alternating: a drift of the machine touches every call alike
        ms["finalize"].append(timed(robust.finalize))
        for name, kw in forms.items():
            ms[name].append(timed(lambda: grid.hypotheses(args.gap, **kw)))
        ms["copy"].append(timed(lambda: dst.copy_(src)))
    del src, dst
    stat = lambda v: {"ms": round(statistics.median(v), 3), "ms_min": round(min(v), 3), "ms_max": round(max(v), 3), "runs": len(v)}
    out = {"tool": "measure_sounding_hypotheses", "case": args.case, "n": n, "size": S, "soundings_per_cell": round(n / (S * S), 3),
           "resolution": res, "gap_m": args.gap, "reps": reps, "build": rt.build_id(), "device": torch.cuda.get_device_name(0),
           "wave_max": rt.ROBUST_WAVE_MAX, "finalize_warm_ms": round(warm, 3)}
    out.update({k: stat(v) for k, v in ms.items()})
    copy_rate = 8 * words / out["copy"]["ms"] / 1e6
    out["copy"]["gbytes_per_s"] = round(copy_rate, 1)
    a, b = grid.hypotheses(args.gap), grid.hypotheses(args.gap)
    bare = grid.hypotheses(args.gap, records=False)
    accepted, cells = grid.counters["accepted"], S * S
    total = int(a.hyp_start[-1]) & 0xFFFFFFFF
    for name in forms:
        model = 4 * accepted + 8 * cells + (4 * cells if name.startswith("guide") else 0) + 57 * cells + \
            (8 * total if name.endswith("records") else 0)
        rate = model / out[name]["ms"] / 1e6
        out[name].update(model_gbytes=round(model / 1e9, 3), gbytes_per_s=round(rate, 1), of_copy=round(rate / copy_rate, 3),
                         over_finalize=round(out[name]["ms"] / out["finalize"]["ms"], 3))
    out["equal_bits"] = all(bool(torch.equal(getattr(a, k), getattr(b, k))) for k in PLANES + ("hyp_start",)) and \
        bool(torch.equal(a.hyp_first[:total], b.hyp_first[:total])) and bool(torch.equal(a.hyp_count[:total], b.hyp_count[:total]))
    out["planes_equal_without_records"] = all(bool(torch.equal(getattr(a, k), getattr(bare, k))) for k in PLANES)
    out["hypotheses"] = total
    out["every_sounding_in_one"] = int(a.hyp_count[:total].sum(dtype=torch.int64)) == accepted and \
        int(a.n_hyp.sum(dtype=torch.int64)) == total
    out["accepted"] = accepted
    out["cells_over_wave_max"] = int((grid.count > rt.ROBUST_WAVE_MAX).sum())
    out["cells_with_two_or_more"] = int((a.n_hyp >= 2).sum())
    out["max_hypotheses_in_a_cell"] = int(a.n_hyp.max())
    print(json.dumps(out), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
