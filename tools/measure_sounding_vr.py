#!/usr/bin/env python3
"""Gridding soundings at variable resolution on the device: the time of ``add`` + ``finalize`` of both VR gridders, of the density
pass and of the plan at survey size, beside the uniform gridders on the same cloud at the same number of cells, and the state of a
planned layout beside the uniform grid at the ladder's finest resolution.

    python tools/measure_sounding_vr.py                      # 2e8 soundings, 1250 x 1250 base cells of 8 m at 16 x 16
    python tools/measure_sounding_vr.py --n 2000000 --base 125 --reps 3

The timed layout is uniform (every base cell ``--dim`` x ``--dim``), so that ``SoundingGridder`` / ``RobustSoundingGridder`` on a
``base * dim`` square grid at ``8 / dim`` metres have the same cells; its table is built like any other and the kernels do not know.
Two clouds of ``--n`` soundings in HBM, timed in one process, alternating (HIP events around each call, median / min / max of
``--reps``; one warm-up round first; states reset before every add and the reset not timed):

  scattered   every sounding in a record drawn uniformly: no two neighbours in the input share a record
  swath       record order, four consecutive soundings per record

  vr_add, vr_finalize                ``VRSoundingGridder``          uniform_add, uniform_finalize              ``SoundingGridder``
  vr_stage, vr_robust_finalize       ``RobustVRSoundingGridder``    uniform_robust_add, uniform_robust_finalize ``RobustSoundingGridder``
  density, plan                      ``VRLayoutPlanner.add`` and ``.plan`` (the plan with its copy of the table to the host)
  read_floor                         ``x.sum() + y.sum() + z.sum()``: a plain read of the same 20 B per sounding

It checks that the VR planes equal the uniform ones after flipud and regrouping (the clouds keep 0.05 cell away from every
border), and that the counters add up.  ``planned``: a cloud of ``--n`` / 10 soundings whose density varies by 100 x from west to
east, planned with the default ladder: records and state bytes beside the uniform grid at the finest rung.  One JSON line."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--n", type=int, default=200_000_000)
    ap.add_argument("--base", type=int, default=1250, help="base cells each way")
    ap.add_argument("--dim", type=int, default=16, help="records each way per base cell of the timed layout")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--target-count", type=int, default=4)
    args = ap.parse_args()
    import numpy as np
    import torch
    from bathymetric_gnn_amd import runtime as rt
    from bathymetric_gnn_amd.data import (RobustSoundingGridder, RobustVRSoundingGridder, SoundingGridder, VRLayout, VRLayoutPlanner,
                                          VRSoundingGridder)
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: this script measures on the device only")
    dev = torch.device("cuda:0")
    n, S, d, B = args.n, args.base, args.dim, 8.0
    x0, y0 = 500000.0, 4000000.0
    total, side, res = S * S * d * d, S * d, B / d
    g = torch.Generator(device=dev).manual_seed(7)
    u = lambda m=n: torch.rand(m, generator=g, device=dev, dtype=torch.float64)
    z = (-30.0 + 2.0 * torch.randn(n, generator=g, device=dev)).contiguous()

    def at_records(rec):
        """Soundings inside the given records of the uniform layout, 0.05 cell away from the borders."""
        b, s = rec // (d * d), rec % (d * d)
        x = x0 + ((b % S) * d + s % d).double() * res + (0.05 + 0.9 * u(rec.numel())) * res
        y = y0 + ((b // S) * d + s // d).double() * res + (0.05 + 0.9 * u(rec.numel())) * res
        return x, y

    clouds = {"scattered": at_records(torch.randint(0, total, (n,), generator=g, device=dev)) + (z,),
              "swath": at_records(torch.arange(n, device=dev, dtype=torch.int64) // 4 % total) + (z,)}
    index = (np.arange(S * S, dtype=np.int64) * (d * d)).reshape(S, S)
    dims = np.full((S, S), d, np.int32)
    layout = VRLayout((S, S), (x0, y0), B, index, dims, dims, total, device=dev)

    def timed(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b)

    out = {"tool": "measure_sounding_vr", "n": n, "base": S, "dim": d, "base_resolution": B, "records": total, "reps": args.reps,
           "build": rt.build_id(), "device": torch.cuda.get_device_name(0), "table_mbytes": round(layout.table.numel() * 8 / 1e6, 2),
           "state_gbytes": round(layout.state_bytes / 1e9, 2)}
    floor = lambda: float(clouds["scattered"][0].sum() + clouds["scattered"][1].sum() + clouds["scattered"][2].sum())
    keys = ("count", "mean", "std", "min", "max", "valid")

    def regroup(plane):                                          # the north-up uniform plane in the order of the records
        return plane.flip(0).reshape(S, d, S, d).permute(0, 2, 1, 3).reshape(-1)

    def measure(pairs, names):
        """``pairs``: (VR gridder, uniform gridder); the four timings per cloud, alternating."""
        vr, un = pairs
        ms = {f"{c}_{k}": [] for c in clouds for k in names}
        for rep in range(args.reps + 1):                         # (round 0 warms every shape and is dropped)
            for c, cloud in clouds.items():
                vr.reset(); un.reset()
                t = [timed(lambda: vr.add(*cloud)), timed(lambda: un.add(*cloud)), timed(vr.finalize), timed(un.finalize)]
                if rep:
                    for k, v in zip(names, t):
                        ms[f"{c}_{k}"].append(v)
        return ms

    def summary(ms):
        for name, v in ms.items():
            out[name] = {"ms": round(statistics.median(v), 3), "ms_min": round(min(v), 3), "ms_max": round(max(v), 3), "runs": len(v)}

    # ---- the streaming gridders -------------------------------------------------------------------------------------------------
    vr, un = VRSoundingGridder(layout), SoundingGridder((side, side), (x0, y0 + S * B), res, device=dev)
    summary(measure((vr, un), ("vr_add", "uniform_add", "vr_finalize", "uniform_finalize")))
    fv, fu = vr.finalize(), un.finalize()                        # (the swath cloud, added last)
    out["equal_to_uniform"] = all(bool(torch.equal(getattr(fv, k).view(torch.uint8), regroup(getattr(fu, k)).view(torch.uint8))) for k in keys)
    c = vr.counters()
    out["counters"] = c
    out["counters_add_up"] = sum(c.values()) == n and c["accepted"] == int(fv.count.sum(dtype=torch.int64)) == n
    del vr, un, fv, fu
    torch.cuda.empty_cache()
    # ---- the robust gridders ----------------------------------------------------------------------------------------------------
    vr, un = RobustVRSoundingGridder(layout, n), RobustSoundingGridder((side, side), (x0, y0 + S * B), res, n, device=dev)
    summary(measure((vr, un), ("vr_stage", "uniform_robust_add", "vr_robust_finalize", "uniform_robust_finalize")))
    fv, fu = vr.finalize(), un.finalize()
    out["robust_equal_to_uniform"] = all(bool(torch.equal(getattr(fv, k).view(torch.uint8), regroup(getattr(fu, k)).view(torch.uint8)))
                                         for k in ("count", "kept", "median", "mad", "kept_mean", "kept_std", "valid", "center2", "limit"))
    flag_ms = [timed(lambda: vr.flag(*clouds["scattered"], fv)) for _ in range(args.reps + 1)][1:]
    summary({"scattered_vr_flag": flag_ms})
    del vr, un, fv, fu
    torch.cuda.empty_cache()
    # ---- density, plan, the plain read ------------------------------------------------------------------------------------------
    ms = {"scattered_density": [], "swath_density": [], "plan": [], "read_floor": []}
    for rep in range(args.reps + 1):
        for cname, cloud in clouds.items():
            planner = VRLayoutPlanner((S, S), (x0, y0), B, device=dev)
            t = timed(lambda: planner.add(*cloud))
            if rep:
                ms[f"{cname}_density"].append(t)
        t_plan, t_floor = timed(lambda: planner.plan(args.target_count)), timed(floor)
        if rep:
            ms["plan"].append(t_plan); ms["read_floor"].append(t_floor)
    summary(ms)
    planned = planner.plan(args.target_count)
    out["plan_of_timed_cloud"] = {"records": planned.total, "dims": sorted(set(np.unique(planned.dx).tolist()))}
    for cname in clouds:
        for kind, parts in (("vr", ("vr_add", "vr_finalize")), ("uniform", ("uniform_add", "uniform_finalize")),
                            ("vr_robust", ("vr_stage", "vr_robust_finalize")),
                            ("uniform_robust", ("uniform_robust_add", "uniform_robust_finalize"))):
            out[f"{cname}_{kind}_add_plus_finalize_ms"] = round(sum(out[f"{cname}_{p}"]["ms"] for p in parts), 3)
    # ---- a cloud whose density varies by 100 x: the planned state beside the uniform grid at the finest rung -----------------------
    m = max(1, n // 10)
    w = u(m)
    px = x0 + (torch.log1p(99.0 * w) / float(np.log(100.0))) * (S * B) * (1 - 1e-12)      # density proportional to 100^(x / extent)
    py = y0 + u(m) * (S * B) * (1 - 1e-12)
    planner = VRLayoutPlanner((S, S), (x0, y0), B, device=dev)
    planner.add(px, py, z[:m].contiguous())
    lay = planner.plan(args.target_count)
    counts = planner.counts()
    finest = 64
    out["planned"] = {"n": m, "target_count": args.target_count, "density_ratio_east_over_west":
                      round(float(counts[:, -S // 20:].sum()) / max(1.0, float(counts[:, :S // 20].sum())), 1),
                      "records": lay.total, "state_gbytes": round(lay.state_bytes / 1e9, 3),
                      "dims": {int(k): int(v) for k, v in zip(*np.unique(lay.dx, return_counts=True))},
                      "uniform_at_finest_records": S * S * finest * finest,
                      "uniform_at_finest_state_gbytes": round((32 + 40 * S * S * finest * finest) / 1e9, 3),
                      "uniform_at_planned_finest_state_gbytes": round((32 + 40 * S * S * int(lay.dx.max()) ** 2) / 1e9, 3)}
    print(json.dumps(out), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
