"""One training step of BathymetricGNN (default shape: GAT, hidden 64, heads 4, 4 layers, edge_dim 3, dropout 0.1; --gnn-type picks
GraphSAGE or GIN instead) on a batch of 16 synthetic 256 x 256 V0 tiles, timed by phase on the GPU: the taped training forward, backward (bgnn_backward), weight repack +
optimizer step (the repack timed on its own: host packing and upload of the blob), and the
untaped training forward for comparison.  --loss fused|torch replaces the fixed linear form of the outputs by BathymetricGNNLoss on random
labels (90 / 2 / 8 % class mix, mask = label 2), through the fused kernels or as separate torch operations (``forward_torch``); its
forward is timed on its own ("loss") and its backward is part of "backward".  Prints one JSON line (milliseconds, medians over --steps) with the tape's bytes per node.
--optimizer fused runs training.FusedAdamW (clip_grad_norm_ 1.0 + AdamW + the in-place refresh of the packed model) instead of torch's
SGD and the host repack: "step" is the optimizer step with its refresh, "step_and_forward_share" adds what the following training forward
pays because the weights changed (its time minus that of the same forward run once more), "pack_weights_calls" counts the host repacks
of the timed iterations (0: the step never went through the host).
--targets torch|fused adds the per-node training targets of the batch to the step (synthetic noise generated once, outside the timed
loop): ``data.training_targets`` (about ten torch launches over the graph's exported batch / valid_rows / valid_cols / local_std) or
the one launch of ``bgnn_training_targets``.  "targets" is that call per step; for torch, "targets_fresh_export" is the same call with
the graph's exported tensors dropped first, which is what a training loop pays (every step builds a new graph), and for fused
"targets_kernel_us" / "targets_gb_per_s" are 50 back-to-back launches between two device events (launch overhead included) over the
bytes the kernel moves.  --bookkeeping item|device (with --loss fused) adds the step's bookkeeping: the reference's two ``.item()``
round trips, or ``EpochMetrics.update`` (``bgnn_epoch_accumulate``; no host wait, the figure ends in a device synchronise).

    python tools/train_step_bench.py [--gnn-type GAT|GraphSAGE|GIN] [--tiles 16] [--size 256] [--steps 10] [--warmup 3] [--loss fused|torch]
                                     [--optimizer torch|fused] [--targets torch|fused] [--bookkeeping item|device]
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
    ap.add_argument("--gnn-type", default="GAT", choices=["GAT", "GraphSAGE", "GIN"])
    ap.add_argument("--tiles", type=int, default=16)
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--loss", default=None, choices=["fused", "torch"])
    ap.add_argument("--optimizer", default="torch", choices=["torch", "fused"])
    ap.add_argument("--targets", default=None, choices=["torch", "fused"])
    ap.add_argument("--bookkeeping", default=None, choices=["item", "device"])
    a = ap.parse_args()
    if a.bookkeeping and a.loss != "fused":
        ap.error("--bookkeeping needs --loss fused (the device form reads the fused loss pass's terms and counts)")
    from bathymetric_gnn_amd import synthetic
    from bathymetric_gnn_amd.data import GraphBuilder
    from bathymetric_gnn_amd.models import BathymetricGNN
    from bathymetric_gnn_amd import runtime as rt
    dev = torch.device("cuda:0")
    tiles = [synthetic.synthetic_tile(a.size, a.size, s, "V0") for s in range(a.tiles)]
    g = GraphBuilder().build_graphs([t[0] for t in tiles], [t[1] for t in tiles], None, [(0.5, 0.5)] * a.tiles)
    sd = synthetic.synthetic_state_dict(in_channels=7, seed=1234, gnn_type=a.gnn_type)
    m = BathymetricGNN(in_channels=7, edge_dim=3, dropout=0.1, gnn_type=a.gnn_type)
    m.load_state_dict({k: torch.as_tensor(v) for k, v in sd.items()})
    m.to(dev).train()
    fused = a.optimizer == "fused"
    if fused:
        from bathymetric_gnn_amd.training import FusedAdamW
        opt = FusedAdamW(m, lr=1e-6, max_grad_norm=1.0)
        packs = []
        real_pack = BathymetricGNN.pack_weights
        BathymetricGNN.pack_weights = lambda self, *x, **k: (packs.append(1), real_pack(self, *x, **k))[1]
    else:
        opt = torch.optim.SGD(m.parameters(), lr=1e-6)
    N = g.num_nodes
    w = torch.randn(N, 3, device=dev)
    if a.loss:
        from bathymetric_gnn_amd.training import BathymetricGNNLoss, compute_class_weights
        rng = np.random.default_rng(0)
        labels = torch.from_numpy(rng.choice(3, size=N, p=(0.90, 0.02, 0.08))).to(dev)
        targets = {"class_labels": labels, "noise_mask": labels == 2,
                   "correction_targets": torch.from_numpy(rng.standard_normal(N).astype(np.float32)).to(dev)}
        crit = BathymetricGNNLoss(class_weights=compute_class_weights(labels), label_smoothing=0.1)
        loss_fn = crit if a.loss == "fused" else crit.forward_torch

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = fn()
        torch.cuda.synchronize()
        return r, (time.perf_counter() - t0) * 1e3

    rec = {"taped_forward": [], "backward": [], "repack_and_step": [], "untaped_forward": []}
    if fused:
        rec = {"taped_forward": [], "backward": [], "step": [], "step_and_forward_share": [], "untaped_forward": []}
    if a.loss:
        rec["loss"] = []
    if a.targets:
        from bathymetric_gnn_amd.data import SyntheticNoiseGenerator, training_targets
        from bathymetric_gnn_amd.training.tile_store import training_targets_fused
        gb = GraphBuilder()
        hw, res_, clean_t, mask_t, _ = gb.upload_tiles([t[0] for t in tiles], [t[1] for t in tiles], None, [(0.5, 0.5)] * a.tiles)
        nb = SyntheticNoiseGenerator(seed=0).generate_batch(hw, clean_t, mask_t, sample_indices=list(range(a.tiles)))
        g = gb.build_from_device(hw, res_, nb.noisy_depth, mask_t, None)        # the step's graph: built from the noisy depth
        N = g.num_nodes
        w = torch.randn(N, 3, device=dev)
        rec["targets"] = []
        if a.targets == "torch":
            rec["targets_fresh_export"] = []
            make_targets = lambda: training_targets(g, clean_t, nb.noisy_depth, nb.classification, nb.noise_mask)
        else:
            make_targets = lambda: training_targets_fused(g, 0, nb.noisy_depth, clean_t, nb.classification, nb.noise_mask)
    if a.bookkeeping:
        from bathymetric_gnn_amd.training import EpochMetrics
        rec["bookkeeping"] = []
        metrics = EpochMetrics(dev)
        metrics.reset()
        book = {"loss": 0.0, "correct": 0, "nodes": 0}
    for it in range(a.warmup + a.steps):
        m.dropout_seed = it
        opt.zero_grad(set_to_none=True)
        out, t_fwd = timed(lambda: m(g))
        if a.targets:
            _, t_tgt = timed(make_targets)
            if a.targets == "torch":
                for k in ("batch", "valid_rows", "valid_cols", "local_std"):
                    g._cache.pop(k, None)
                _, t_tgt_fresh = timed(make_targets)
        if a.loss:
            losses, t_loss = timed(lambda: loss_fn(out, targets))
            loss = losses["total"]
        else:
            loss = (out["class_logits"] * w).sum() + out["confidence"].sum() + out["correction"].sum()
        _, t_bwd = timed(loss.backward)
        _, t_opt = timed(opt.step)
        if a.bookkeeping == "item":
            def host_bookkeeping():                    # training/trainer.py:764-767 of the reference
                book["loss"] += losses["total"].item() * N
                book["correct"] += (out["predicted_class"] == targets["class_labels"]).sum().item()
                book["nodes"] += N
            _, t_book = timed(host_bookkeeping)
        elif a.bookkeeping == "device":
            _, t_book = timed(lambda: metrics.update(g, losses, crit))
        with torch.no_grad():
            _, t_plain = timed(lambda: m(g))           # untaped training forward (repacks like every training forward)
        ctx = rt.get_context(dev)
        if fused:
            with torch.no_grad():
                _, t_again = timed(lambda: m(g))       # the same forward once more: nothing changed but the running statistics
            if it + 1 == a.warmup:
                del packs[:]
            if it >= a.warmup:
                rec["step"].append(t_opt)
                rec["step_and_forward_share"].append(t_opt + max(0.0, t_plain - t_again))
        else:
            t0 = time.perf_counter()
            m.invalidate_native()                      # the repack on its own: host packing + upload of the blob
            m.native(ctx, 3)
            torch.cuda.synchronize()
            t_pack = (time.perf_counter() - t0) * 1e3
            if it >= a.warmup:
                rec["repack_and_step"].append(t_opt + t_pack)
        if it >= a.warmup:
            rec["taped_forward"].append(t_fwd)
            rec["backward"].append(t_bwd)
            rec["untaped_forward"].append(t_plain)
            if a.loss:
                rec["loss"].append(t_loss)
            if a.targets:
                rec["targets"].append(t_tgt)
                if a.targets == "torch":
                    rec["targets_fresh_export"].append(t_tgt_fresh)
            if a.bookkeeping:
                rec["bookkeeping"].append(t_book)
    extra = {}
    if a.targets == "fused":
        reps = 50
        ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        ev0.record()
        for _ in range(reps):
            make_targets()
        ev1.record()
        torch.cuda.synchronize()
        us = ev0.elapsed_time(ev1) * 1e3 / reps
        cells = int(nb.noisy_depth.numel())
        moved = 4 * cells + N * (4 + 4 + 8 + 1 + 4) + N * (8 + 4 + 1)      # node ids; noisy, clean, label, mask, local_std; y, target, mask
        extra = {"targets_kernel_us": round(us, 2), "targets_bytes": moved, "targets_gb_per_s": round(moved / us / 1e3, 1)}
    if a.bookkeeping == "device":
        r = metrics.result()
        extra["bookkeeping_steps"] = r["steps"]
    tape_bytes = int(ctx.lib.bgnn_tape_bytes(m.native(ctx, 3), g._handle))
    res = {"metric": "train_step_ms", "gnn_type": a.gnn_type, "nodes": N, "tiles": a.tiles, "size": a.size,
           **({"loss_path": a.loss} if a.loss else {}),
           **({"optimizer": "fused", "pack_weights_calls": len(packs)} if fused else {}),
           **({"targets_path": a.targets} if a.targets else {}), **({"bookkeeping_path": a.bookkeeping} if a.bookkeeping else {}),
           **extra,
           **{k: round(float(np.median(v)), 3) for k, v in rec.items()},
           "tape_bytes_per_node": round(tape_bytes / N, 1), "tape_gb": round(tape_bytes / 1e9, 3)}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
