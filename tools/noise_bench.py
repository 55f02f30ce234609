"""Synthetic training samples on the GPU, timed: SyntheticNoiseGenerator.generate_batch on clean tiles resident in HBM, for the
two batch shapes of the training path (16 tiles of 256 x 256 and 4 tiles of 512 x 512, V1 tiles: about 11 % holes), and the same
followed by GraphBuilder.build_from_device and training_targets (what stands in front of a training step).  A batch is timed
from the call to a device synchronise, host work included (the scalar draws, the plan tables); medians over --steps batches after
--warmup, every batch with fresh sample indices; the device time of the generator's own launches comes from the library's event
scopes in ten further batches.  Prints one JSON line, milliseconds per batch.

    python tools/noise_bench.py [--steps 50] [--warmup 5]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    a = ap.parse_args()
    from bathymetric_gnn_amd import runtime as rt
    from bathymetric_gnn_amd import synthetic
    from bathymetric_gnn_amd.data import GraphBuilder, NoiseAugmentor, SyntheticNoiseGenerator, training_targets
    if not torch.cuda.is_available():
        raise SystemExit("noise_bench needs a GPU")
    dev = torch.device("cuda:0")
    gb = GraphBuilder()
    res = {"metric": "noise_batch_ms", "steps": a.steps}
    for n, side in ((16, 256), (4, 512)):
        tiles = [synthetic.synthetic_tile(side, side, s, "V1") for s in range(n)]
        hw = np.array([[side, side]] * n, np.int32)
        rs = np.full((n, 2), 0.5, np.float64)
        clean_t = torch.from_numpy(np.concatenate([t[0].ravel() for t in tiles])).to(dev)
        mask_t = torch.from_numpy(np.concatenate([t[1].ravel() for t in tiles]).view(np.uint8)).to(dev)
        aug = NoiseAugmentor(SyntheticNoiseGenerator(seed=1), seed=2)

        def sample():
            return aug.augment_batch(hw, clean_t, mask_t)

        def sample_graph_targets():
            b = aug.augment_batch(hw, clean_t, mask_t)
            g = gb.build_from_device(hw, rs, b.noisy_depth, mask_t, None)
            return training_targets(g, clean_t, b.noisy_depth, b.classification, b.noise_mask)

        for name, fn in (("generate", sample), ("generate_graph_targets", sample_graph_targets)):
            ms = []
            for it in range(a.warmup + a.steps):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn()
                torch.cuda.synchronize()
                if it >= a.warmup:
                    ms.append((time.perf_counter() - t0) * 1e3)
            res[f"{name}_{n}x{side}"] = round(float(np.median(ms)), 3)
            res[f"{name}_{n}x{side}_p90"] = round(float(np.percentile(ms, 90)), 3)
        # device time of the generator's launches alone, by the library's event scopes: "stats" holds the two statistics passes,
        # the windowed filter and the finalise launch, "scatter" the per-cell apply kernel
        ctx = rt.get_context(dev)
        ctx.profile(["stats", "scatter"])
        for _ in range(10):
            sample()
        pr = ctx.profile_read()
        ctx.profile([])
        res[f"device_stats_and_filter_{n}x{side}"] = round(pr["stats"]["ms"] / 10, 3)
        res[f"device_apply_{n}x{side}"] = round(pr["scatter"]["ms"] / 10, 3)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
