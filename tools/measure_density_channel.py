#!/usr/bin/env python3
"""What the ninth input channel costs: the headline batch with and without the sounding density plane, in one process.

    python tools/measure_density_channel.py                  # 128 tiles of 256 x 256, 8-connected, exact float32
    python tools/measure_density_channel.py --tiles 16 --reps 10

Two models of the default shape (4 layers, hidden 64, 4 heads) over one seeded batch that carries an uncertainty plane:

  8 channels   seven computed features + uncertainty: ``bgnn_infer_tiles`` -- the extractor runs inside the lin_0 GEMM (fused front)
  9 channels   the same + sounding density: ``bgnn_infer_tiles_aux`` -- the wide node table is filled (node_aux.hip), the extractor
               keeps a launch of its own (K = 16), h0 is written and read once more

Every figure is the median (and minimum) over ``--reps`` of HIP events around one ``TileBatchEngine.infer_device`` call, the two
models ALTERNATING call by call after ``--warmup`` rounds of both, so that a drift of the machine falls on both alike.  The wide
table's fill is timed by the library's own per-kernel events (``Context.profile(["features"])``: the feature kernel with and without
the fill behind it, in ``GraphBuilder.build_from_device``, alternating build by build; the median of the differences), and set
against its bytes: 32 read + 64 written + 4 per plane per node.
One JSON line at the end."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tiles", type=int, default=128)
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()
    import numpy as np
    import torch
    from bathymetric_gnn_amd import runtime as rt, synthetic
    from bathymetric_gnn_amd.data import GraphBuilder
    from bathymetric_gnn_amd.models import BathymetricGNN
    from bathymetric_gnn_amd.models.pipeline import TileBatchEngine
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: this tool measures on the device only")
    dev = torch.device("cuda:0")
    B, n = args.tiles, args.size
    depth, mask, unc = synthetic.synthetic_tile_batch(B, n, n, 100, "V1", True)
    rng = np.random.default_rng(1)
    den = (np.float32(1) / rng.integers(1, 12, depth.shape).astype(np.float32)).astype(np.float32)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev).reshape(-1)
    d_t, m_t, u_t, a_t = up(depth), up(mask.view(np.uint8)), up(unc), up(den)
    hw = np.tile(np.array([[n, n]], np.int32), (B, 1)); res = np.full((B, 2), 0.5)
    gb = GraphBuilder()
    ctx = rt.get_context(dev)
    assert ctx.get_option("matrix_path") == 0 and ctx.get_option("fused_front") == 1

    def engine(in_channels):
        sd = synthetic.synthetic_state_dict(in_channels=in_channels, seed=1234)
        m = BathymetricGNN(in_channels=in_channels, edge_dim=3, dropout=0.0)
        m.load_state_dict({k: torch.as_tensor(v) for k, v in sd.items()})
        return TileBatchEngine(m.to(dev).eval(), gb, dev)
    e8, e9 = engine(8), engine(9)
    out = torch.empty((3, d_t.numel()), dtype=torch.float32, device=dev)
    calls = {"8": lambda: e8.infer_device(hw, res, d_t, m_t, u_t, out=out),
             "9": lambda: e9.infer_device(hw, res, d_t, m_t, u_t, out=out, density_t=a_t)}
    for _ in range(args.warmup):
        for f in calls.values():
            f()
    torch.cuda.synchronize()
    ms = {k: [] for k in calls}
    for _ in range(args.reps):
        for k, f in calls.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(); f(); b.record()
            b.synchronize()
            ms[k].append(a.elapsed_time(b))
    nodes = int(mask.sum())
    # the wide table's fill by the library's own events: the "features" scope with and without it
    builds = (("plain", None), ("aux", [a_t]))
    for _ in range(2):
        for _, aux in builds:
            gb.build_from_device(hw, res, d_t, m_t, u_t, aux_t=aux)
    ctx.synchronize()
    ctx.profile(["features"]); ctx.profile_read()
    per = {"plain": [], "aux": []}
    for _ in range(args.reps):                              # alternating: a drift of the machine falls on both alike
        for name, aux in builds:
            gb.build_from_device(hw, res, d_t, m_t, u_t, aux_t=aux)
            per[name].append(ctx.profile_read()["features"]["ms"])
    ctx.profile([])
    feat = {k: statistics.median(v) for k, v in per.items()}
    fill_ms = statistics.median([a - p for a, p in zip(per["aux"], per["plain"])])
    fill_bytes = nodes * (32 + 64 + 4)
    med = {k: statistics.median(v) for k, v in ms.items()}
    result = {"tiles": B, "size": n, "nodes": nodes, "reps": args.reps,
              "ms_8_channels": {"median": med["8"], "min": min(ms["8"])}, "ms_9_channels": {"median": med["9"], "min": min(ms["9"])},
              "nodes_per_s_8": nodes / med["8"] * 1e3, "nodes_per_s_9": nodes / med["9"] * 1e3, "ratio_9_over_8": med["9"] / med["8"],
              "features_ms_plain": feat["plain"], "features_ms_with_fill": feat["aux"], "x16_fill_ms": fill_ms,
              "x16_fill_bytes": fill_bytes, "x16_fill_TB_per_s": fill_bytes / max(fill_ms, 1e-9) * 1e-9}
    print(json.dumps(result))


if __name__ == "__main__":
    main()
