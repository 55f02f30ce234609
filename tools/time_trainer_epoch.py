#!/usr/bin/env python3
"""One training epoch and one validation epoch of ``Trainer``, wall time, in one process; one JSON line.

    python tools/time_trainer_epoch.py --case uniform
    python tools/time_trainer_epoch.py --case ragged --reps 5
    python tools/time_trainer_epoch.py --case uniform --root /path/to/another/checkout     # the same workload on that checkout's package

uniform  a synthetic store (``from_tiles``) of 64 tiles of 512 x 512 (8 distinct seeded V1 tiles, repeated), validation 16 tiles,
         ``batch_size`` 2: the model and settings of tests/test_gpu_trainer.py (``_model("GAT")``, ``_config()``), 32 + 8 steps
ragged   a ground-truth store of 6000 tiles of 3 x 3 to 50 x 50 cells (the seeded store of tools/time_tile_augment.py's ragged
         case: the sizes of refinement grids), validation 2000 such tiles, ``batch_nodes`` 200000: 22 + 8 steps

After one warm-up epoch, ``--reps`` epochs (training then validation) under a host clock between two device synchronises.  The
line also carries the epochs' losses: two checkouts that compute the same thing print the same floats.  To compare two checkouts,
alternate their processes and set the medians against the spread of either."""
import argparse
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--case", required=True, choices=["uniform", "ragged"])
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--root", default=ROOT, help="the checkout whose package is timed (default: this one)")
    args = ap.parse_args()
    if args.reps < 1:
        ap.error("--reps must be at least 1")
    sys.path.insert(0, args.root)
    import numpy as np
    import torch
    from bathymetric_gnn_amd import runtime as rt
    from bathymetric_gnn_amd import synthetic
    from bathymetric_gnn_amd.config import Config
    from bathymetric_gnn_amd.models import BathymetricGNN
    from bathymetric_gnn_amd.training import TileStore, Trainer
    dev = torch.device("cuda:0")

    sd = synthetic.synthetic_state_dict(in_channels=7, num_layers=2, seed=1, gnn_type="GAT")
    model = BathymetricGNN(in_channels=7, hidden_channels=64, num_gnn_layers=2, gnn_type="GAT", heads=4, dropout=0.1, edge_dim=3)
    model.load_state_dict({k: torch.as_tensor(v) for k, v in sd.items()})
    cfg = Config()
    cfg.training = {"batch_size": 2, "epochs": 2, "scheduler": "cosine"}
    kw = {}
    if args.case == "uniform":
        base = [synthetic.synthetic_tile(512, 512, 40 + i, "V1", False) for i in range(8)]
        tr = [base[i % 8] for i in range(64)]
        va = [base[(i + 3) % 8] for i in range(16)]
        train = TileStore.from_tiles([t[0] for t in tr], [t[1] for t in tr], None, [(0.5, 0.5)] * len(tr), seed=0)
        val = TileStore.from_tiles([t[0] for t in va], [t[1] for t in va], None, [(0.5, 0.5)] * len(va), seed=1)
    else:
        def make(n, seed):
            hw = np.random.default_rng(seed).integers(3, 51, size=(n, 2)).astype(np.int32)
            g = torch.Generator(device=dev).manual_seed(seed)
            cells = int((hw[:, 0].astype(np.int64) * hw[:, 1]).sum())
            labels = (torch.rand(cells, generator=g, device=dev) * 4).to(torch.int32) - 1
            return TileStore("ground_truth", hw, np.ones((n, 2)), -30 + 5 * torch.randn(cells, generator=g, device=dev),
                             (labels >= 0).view(torch.uint8), None, labels=labels,
                             difference=0.3 * torch.randn(cells, generator=g, device=dev), device=dev)
        train, val = make(6000, 5), make(2000, 6)
        kw["batch_nodes"] = 200000
    with tempfile.TemporaryDirectory() as out_dir:
        t = Trainer(cfg, model.cuda(), train, val, output_dir=out_dir, seed=4, **kw)
        steps = (len(t.step_plan(0)), len(t.step_plan(0, validation=True)))

        def epoch(e):
            t.current_epoch = e
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            a = t._train_epoch()
            b = t._validate_epoch()
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) * 1e3, a["loss"], b["loss"]

        epoch(0)                                             # warm-up: the allocator, the plans
        runs = [epoch(e) for e in range(1, 1 + args.reps)]
    print(json.dumps({"case": args.case, "root": args.root, "build": rt.build_id(), "steps_train_val": steps,
                      "epoch_ms": [round(r[0], 2) for r in runs], "losses": [r[1:] for r in runs]}), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
