"""The multi-task training loss on the GPU, timed: BathymetricGNNLoss forward + ``total.backward()`` on 1 048 576 nodes of random
inputs of the default shape (3 classes, correction head, noise mask), (a) through the fused kernels and (b) as the same formulas
composed from the component modules as separate torch operations on the same GPU (``forward_torch``: what there was to run before
the kernels existed).  A repetition is timed from the call to a device synchronise, host work included; medians over --steps
repetitions after --warmup.  Prints one JSON line, milliseconds.

    python tools/loss_bench.py [--nodes 1048576] [--steps 50] [--warmup 5]
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
    ap.add_argument("--nodes", type=int, default=1 << 20)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    a = ap.parse_args()
    from bathymetric_gnn_amd.training import BathymetricGNNLoss, compute_class_weights
    if not torch.cuda.is_available():
        raise SystemExit("loss_bench needs a GPU")
    dev = torch.device("cuda:0")
    n = a.nodes
    rng = np.random.default_rng(0)
    labels = torch.from_numpy(rng.choice(3, size=n, p=(0.90, 0.02, 0.08))).to(dev)
    logits = torch.from_numpy((2.0 * rng.standard_normal((n, 3))).astype(np.float32)).to(dev).requires_grad_(True)
    outputs = {"class_logits": logits, "predicted_class": logits.detach().argmax(-1),
               "confidence": torch.sigmoid(torch.from_numpy(rng.standard_normal(n).astype(np.float32)).to(dev)).requires_grad_(True),
               "correction": torch.from_numpy(rng.standard_normal(n).astype(np.float32)).to(dev).requires_grad_(True)}
    targets = {"class_labels": labels, "correction_targets": torch.from_numpy(rng.standard_normal(n).astype(np.float32)).to(dev),
               "noise_mask": labels == 2}
    crit = BathymetricGNNLoss(class_weights=compute_class_weights(labels), label_smoothing=0.1)

    def run(fn, backward=True):
        ms = []
        for it in range(a.warmup + a.steps):
            for k in ("class_logits", "confidence", "correction"):
                outputs[k].grad = None
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            losses = fn(outputs, targets)
            if backward:
                losses["total"].backward()
            torch.cuda.synchronize()
            if it >= a.warmup:
                ms.append((time.perf_counter() - t0) * 1e3)
        return round(float(np.median(ms)), 3), round(float(np.percentile(ms, 90)), 3), float(losses["total"].detach())

    res = {"metric": "loss_forward_backward_ms", "nodes": n, "steps": a.steps}
    res["fused"], res["fused_p90"], total_fused = run(crit)
    res["torch_ops"], res["torch_ops_p90"], total_torch = run(crit.forward_torch)
    res["fused_forward_only"] = run(crit, backward=False)[0]
    res["torch_ops_forward_only"] = run(crit.forward_torch, backward=False)[0]
    res["speedup"] = round(res["torch_ops"] / res["fused"], 2)
    res["total_fused"], res["total_torch_ops"] = total_fused, total_torch
    print(json.dumps(res))


if __name__ == "__main__":
    main()
