#!/usr/bin/env python3
"""Gridding soundings on the device: the time of ``SoundingGridder.add`` + ``finalize`` at survey size, beside a plain read of the
same bytes and the numpy restatement on the host.

    python tools/measure_sounding_grid.py                    # 2e8 soundings on 20000 x 20000 cells
    python tools/measure_sounding_grid.py --n 2000000 --size 2000 --reps 3

Builds three clouds of ``--n`` soundings in HBM over a ``--size`` x ``--size`` grid at 0.5 m and times, in one process and alternating
between them (HIP events around each call, median / min / max of ``--reps``; one warm-up round first):

  scattered   every sounding in a cell drawn uniformly: no two neighbours in the input share a cell
  swath       raster order, four consecutive soundings per cell: consecutive soundings in the same or the neighbouring cell
  one_cell    every sounding in one cell: the worst contention.  Timed at ``--n`` / 10 first; where that projects to more than
              ``--one-cell-budget`` seconds the full size is timed once.
  read_floor  ``x.sum() + y.sum() + z.sum()``: a plain read of the same 20 B per sounding, the floor of any add
  finalize    ``SoundingGridder.finalize`` on the scattered state (40 B read and 21 B written per cell)

and on the host ``numpy_restatement``: cell index, ``bincount`` on the cell for the count and with q and q * q as weights, at
``--host-n`` soundings scattered over a grid with half a sounding per cell, in ns per sounding.  The state is reset (not timed) before every add.  It also checks that two adds of one
cloud leave equal bits in every plane, and that the counters add up.  One JSON line."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--n", type=int, default=200_000_000)
    ap.add_argument("--size", type=int, default=20000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--host-n", type=int, default=10_000_000)
    ap.add_argument("--one-cell-budget", type=float, default=10.0)
    args = ap.parse_args()
    import numpy as np
    import torch
    from bathymetric_gnn_amd import runtime as rt
    from bathymetric_gnn_amd.data import SoundingGridder
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: this script measures on the device only")
    dev = torch.device("cuda:0")
    n, S, res = args.n, args.size, 0.5
    x0, y0 = 500000.0, 4000000.0 + S * res
    g = torch.Generator(device=dev).manual_seed(7)
    u = lambda: torch.rand(n, generator=g, device=dev, dtype=torch.float64)
    z = (-30.0 + 2.0 * torch.randn(n, generator=g, device=dev)).contiguous()
    clouds = {"scattered": (x0 + u() * (S * res), y0 - u() * (S * res), z)}
    cell = torch.arange(n, device=dev, dtype=torch.int64) // 4 % (S * S)
    clouds["swath"] = (x0 + ((cell % S).double() + 0.05 + 0.9 * u()) * res, y0 - ((cell // S).double() + 0.05 + 0.9 * u()) * res, z)
    del cell
    clouds["one_cell"] = (x0 + (S // 2 + 0.05 + 0.9 * u()) * res, y0 - (S // 3 + 0.05 + 0.9 * u()) * res, z)
    gr = SoundingGridder((S, S), (x0, y0), res, device=dev)

    def timed(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b)

    def add(name, m=None):
        x, y, zz = clouds[name]
        gr.reset()
        return timed(lambda: gr.add(x[:m], y[:m], zz[:m])) if m else timed(lambda: gr.add(x, y, zz))

    out = {"tool": "measure_sounding_grid", "n": n, "size": S, "resolution": res, "reps": args.reps, "build": rt.build_id(),
           "device": torch.cuda.get_device_name(0), "state_bytes_per_cell": rt.SOUNDINGS_CELL_BYTES,
           "state_gbytes": round(gr._state.numel() * 8 / 1e9, 2)}
    small = max(1, n // 10)
    add("one_cell", small)                                       # warm-up of the one-cell case, at the small size
    tenth = [add("one_cell", small) for _ in range(3)]
    out["one_cell_tenth"] = {"n": small, "ms": round(statistics.median(tenth), 3), "ms_min": round(min(tenth), 3), "ms_max": round(max(tenth), 3)}
    one_cell_reps = args.reps if statistics.median(tenth) * 10 / 1e3 <= args.one_cell_budget else 1
    floor = lambda: float(clouds["scattered"][0].sum() + clouds["scattered"][1].sum() + clouds["scattered"][2].sum())
    for name in ("scattered", "swath"):                          # warm every shape the timed window uses
        add(name)
    floor()
    gr.finalize()
    ms = {k: [] for k in ("scattered", "swath", "one_cell", "read_floor", "finalize")}
    for rep in range(args.reps):                                 # alternating: a drift of the machine touches every call alike
        ms["swath"].append(add("swath"))
        if rep < one_cell_reps:
            ms["one_cell"].append(add("one_cell"))
        ms["read_floor"].append(timed(floor))
        ms["scattered"].append(add("scattered"))
        ms["finalize"].append(timed(gr.finalize))
    for name, v in ms.items():
        med = statistics.median(v)
        out[name] = {"ms": round(med, 3), "ms_min": round(min(v), 3), "ms_max": round(max(v), 3), "runs": len(v)}
        if name != "finalize":
            out[name]["ns_per_sounding"] = round(med * 1e6 / n, 4)
            out[name]["gbytes_per_s"] = round(20 * n / med / 1e6, 1)
    out["finalize"]["gbytes_per_s"] = round(61 * S * S / out["finalize"]["ms"] / 1e6, 1)
    for name in ("scattered", "swath"):
        out[name + "_add_plus_finalize_ms"] = round(out[name]["ms"] + out["finalize"]["ms"], 3)
        out[name + "_over_floor"] = round(out[name]["ms"] / out["read_floor"]["ms"], 2)
    # results: equal bits from two runs, and counters that add up
    planes = []
    for _ in range(2):
        add("swath")
        f = gr.finalize()
        planes.append([getattr(f, k).clone() for k in ("count", "mean", "std", "min", "max", "valid")])
    out["equal_bits"] = all(bool(torch.equal(a.view(torch.uint8), b.view(torch.uint8))) for a, b in zip(*planes))
    c = gr.counters()
    out["counters"] = c
    out["counters_add_up"] = sum(c.values()) == n and c["accepted"] == int(planes[0][0].sum(dtype=torch.int64))
    # the numpy restatement on the host
    hn = args.host_n
    hs = max(1, int((2 * hn) ** 0.5))                            # a grid with the device run's half a sounding per cell
    rng = np.random.default_rng(7)
    hx, hy = x0 + rng.random(hn) * (hs * res), y0 - rng.random(hn) * (hs * res)
    hz = (-30.0 + 2.0 * rng.standard_normal(hn)).astype(np.float32)
    t0 = time.perf_counter()
    col, row = np.floor((hx - x0) / res), np.floor((y0 - hy) / res)
    ok = (col >= 0) & (col < hs) & (row >= 0) & (row < hs) & np.isfinite(hz) & (np.abs(hz) < 32768)
    hc = (row[ok].astype(np.int64) * hs + col[ok].astype(np.int64))
    q = np.rint(hz[ok].astype(np.float64) * 65536.0)
    count = np.bincount(hc, minlength=hs * hs)
    s1 = np.bincount(hc, weights=q, minlength=hs * hs)
    s2 = np.bincount(hc, weights=q * q, minlength=hs * hs)
    host_s = time.perf_counter() - t0
    out["numpy_restatement"] = {"n": hn, "grid": hs, "ns_per_sounding": round(host_s * 1e9 / hn, 1),
                                "note": "scattered; count, S1 and S2 by bincount (float64 weights); no extremes"}
    assert int(count.sum()) == int(ok.sum()) and s1.size == s2.size
    print(json.dumps(out), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
