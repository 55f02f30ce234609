#!/usr/bin/env python3
"""Error percentiles on the device (include/bgnn_quantile.h, training/huber_delta.py): what the adaptive Huber delta costs.

    python tools/measure_error_quantile.py                    # every section, each in a child process under its own time limit
    python tools/measure_error_quantile.py --section add      # one section in this process

Sections (HIP events around each call, alternating between the variants of a section, median / min / max of ``--reps``):

  add     ``CorrectionErrorTracker.add`` at ``--rows`` rows (1 M) with 20 % of them masked, beside ``torch.clone`` of the same 9 bytes
          per row (two float32 planes and the mask) in the same process; ``add_equal``: every error equal and every row masked, the
          worst contention on one bin of the top-digit histogram; ``add_all``: every row masked, errors spread; ``back_to_back``:
          50 adds (and 50 x 3 clones) between two events, per call -- a single call of 9 MB is mostly launch latency
  step    one training step of the default GAT on 16 x 256^2 tiles (1 M nodes: taped forward, fused loss, backward, FusedAdamW,
          EpochMetrics) with ``tracker.add`` after the loss and without it, alternating
  select  ``CorrectionErrorTracker.percentiles`` over 10^7 and 10^8 staged keys for one and for three percentiles (the read-back
          included), beside ``numpy.percentile`` on the host for the same errors (one run) and checked against it

The parent stops at the first section that fails or runs into its limit and starts nothing after it.  One JSON line.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
LIMITS = {"add": 120, "step": 240, "select": 360}             # seconds per section


def _events(fn):
    import torch
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def _alternate(calls, reps):
    import torch
    for fn in calls.values():                                    # warm every shape the timed window uses
        fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in calls}
    for _ in range(reps):
        for name, fn in calls.items():
            ms[name].append(_events(fn))
    return {k: {"ms": round(statistics.median(v), 4), "ms_min": round(min(v), 4), "ms_max": round(max(v), 4)} for k, v in ms.items()}


def section_add(args):
    import torch
    from bathymetric_gnn_amd.training import CorrectionErrorTracker
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(3)
    n = args.rows
    c, t = torch.randn(n, generator=g, device=dev), torch.randn(n, generator=g, device=dev)
    mask = (torch.rand(n, generator=g, device=dev) < 0.2)
    ones = torch.ones(n, dtype=torch.bool, device=dev)
    c_equal = t + 1.25
    tracker = CorrectionErrorTracker(n, dev)

    def add(cc, mm):
        tracker.reset()                                          # (a memset of 8 KiB: inside the figure, as a step never pays it)
        tracker.add(cc, t, mm)
    out = _alternate({"add": lambda: add(c, mask), "clone": lambda: (c.clone(), t.clone(), mask.clone()),
                      "add_all": lambda: add(c, ones), "add_equal": lambda: add(c_equal, ones),
                      "reset": tracker.reset}, args.reps)
    for k in ("add", "clone", "add_all", "add_equal"):
        out[k]["gbytes_per_s"] = round(9 * n / out[k]["ms"] / 1e6, 1)      # (clone also writes 9 B per row)
    out["add_over_clone"] = round(out["add"]["ms"] / out["clone"]["ms"], 3)
    # a single call at this size is mostly launch latency: 50 calls back to back between two events, per call
    roomy = CorrectionErrorTracker(12 * n, dev)                  # (50 adds of 20 % of the rows fit)

    def back_to_back(fn):
        def run():
            for _ in range(50):
                fn()
        return run
    roomy.reset()
    b2b = _alternate({"add": back_to_back(lambda: roomy.add(c, t, mask)), "clone": back_to_back(lambda: (c.clone(), t.clone(), mask.clone())),
                      "reset": roomy.reset}, 5)
    out["back_to_back"] = {k: {"us_per_call": round(b2b[k]["ms"] * 20, 2), "gbytes_per_s": round(9 * n / (b2b[k]["ms"] / 50) / 1e6, 1)}
                           for k in ("add", "clone")}
    out["back_to_back"]["add_over_clone"] = round(b2b["add"]["ms"] / b2b["clone"]["ms"], 3)
    out["equal_over_all"] = round(out["add_equal"]["ms"] / out["add_all"]["ms"], 3)
    out["rows"] = n
    return out


def section_step(args):
    import numpy as np
    import torch
    from bathymetric_gnn_amd import synthetic
    from bathymetric_gnn_amd.data import GraphBuilder
    from bathymetric_gnn_amd.models import BathymetricGNN
    from bathymetric_gnn_amd.training import (BathymetricGNNLoss, CorrectionErrorTracker, EpochMetrics, FusedAdamW,
                                              compute_class_weights)
    dev = torch.device("cuda:0")
    tiles = [synthetic.synthetic_tile(256, 256, s, "V0") for s in range(16)]
    graph = GraphBuilder().build_graphs([t[0] for t in tiles], [t[1] for t in tiles], None, [(0.5, 0.5)] * 16)
    sd = synthetic.synthetic_state_dict(in_channels=7, seed=1234, gnn_type="GAT")
    m = BathymetricGNN(in_channels=7, edge_dim=3, dropout=0.1, gnn_type="GAT")
    m.load_state_dict({k: torch.as_tensor(v) for k, v in sd.items()})
    m.to(dev).train()
    opt = FusedAdamW(m, lr=1e-6, max_grad_norm=1.0)
    n = graph.num_nodes
    rng = np.random.default_rng(0)
    labels = torch.from_numpy(rng.choice(3, size=n, p=(0.90, 0.02, 0.08))).to(dev)
    targets = {"class_labels": labels, "noise_mask": labels == 2,
               "correction_targets": torch.from_numpy(rng.standard_normal(n).astype(np.float32)).to(dev)}
    crit = BathymetricGNNLoss(class_weights=compute_class_weights(labels))
    metrics, tracker = EpochMetrics(dev), CorrectionErrorTracker(8 * n, dev)      # (room for every timed step's 8 % of the rows)
    metrics.reset()
    tracker.reset()
    seed = [0]

    def step(track):
        seed[0] += 1
        m.dropout_seed = seed[0]
        opt.zero_grad()
        out = m(graph)
        losses = crit(out, targets)
        if track:
            tracker.add(out["correction"], targets["correction_targets"], targets["noise_mask"])
        losses["total"].backward()
        opt.step()
        metrics.update(graph, losses, crit)
    out = _alternate({"step_tracked": lambda: step(True), "step_plain": lambda: step(False)}, args.reps)
    out["nodes"] = n
    out["tracker_share_of_step"] = round((out["step_tracked"]["ms"] - out["step_plain"]["ms"]) / out["step_plain"]["ms"], 5)
    with torch.no_grad():
        corr = m(graph)["correction"].detach()
    out["add_alone"] = _alternate({"add": lambda: tracker.add(corr, targets["correction_targets"], targets["noise_mask"])}, args.reps)["add"]
    out["dropped"] = tracker.percentiles([95.0])["dropped"]      # 0: every timed add filed its rows
    return out


def section_select(args):
    import numpy as np
    import torch
    from bathymetric_gnn_amd.training import CorrectionErrorTracker
    dev = torch.device("cuda:0")
    out = {}
    for keys in (10 ** 7, 10 ** 8):
        g = torch.Generator(device=dev).manual_seed(keys % 1000 + 1)
        c = torch.randn(keys, generator=g, device=dev) * 3.0
        t = torch.zeros(keys, device=dev)
        tracker = CorrectionErrorTracker(keys, dev)
        tracker.reset()
        piece = keys // 8
        for k in range(0, keys, piece):                          # several adds, as an epoch makes them
            tracker.add(c[k:k + piece], t[k:k + piece], None)
        res = _alternate({"one": lambda: tracker.percentiles([95.0]), "three": lambda: tracker.percentiles([50.0, 95.0, 99.0])},
                         max(3, args.reps // 2))
        host = c.abs().cpu().numpy().astype(np.float64)
        t0 = time.perf_counter()
        want = [float(v) for v in np.percentile(host, [50.0, 95.0, 99.0])]     # (the cast and the copy to the host not counted)
        res["numpy_three_ms"] = round((time.perf_counter() - t0) * 1e3, 1)
        got = tracker.percentiles([50.0, 95.0, 99.0])
        res["equal_numpy"] = bool(got["values"] == want and got["count"] == keys)
        res["gkeys_per_s_one"] = round(keys / res["one"]["ms"] / 1e6, 2)
        out[f"keys_{keys}"] = res
        del tracker, c, t, host
    return out


SECTIONS = {"add": section_add, "step": section_step, "select": section_select}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--section", choices=sorted(SECTIONS), default=None)
    ap.add_argument("--rows", type=int, default=1 << 20)
    ap.add_argument("--reps", type=int, default=20)
    args = ap.parse_args()
    if args.section:
        import torch
        from bathymetric_gnn_amd import runtime as rt
        if not torch.cuda.is_available():
            raise SystemExit("no GPU: this script measures on the device only")
        out = {"section": args.section, "build": rt.build_id(), "device": torch.cuda.get_device_name(0), "reps": args.reps}
        out.update(SECTIONS[args.section](args))
        print(json.dumps(out), flush=True)
        return 0
    result = {"tool": "measure_error_quantile"}
    for name in ("add", "step", "select"):
        cmd = [sys.executable, os.path.abspath(__file__), "--section", name, "--rows", str(args.rows), "--reps", str(args.reps)]
        try:
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=LIMITS[name])
        except subprocess.TimeoutExpired:
            result[name] = {"error": f"no result within {LIMITS[name]} s"}
            print(json.dumps(result), flush=True)
            return 2                                             # nothing more is started on this GPU
        if r.returncode != 0:
            result[name] = {"error": f"exit status {r.returncode}", "stderr": r.stderr[-2000:]}
            print(json.dumps(result), flush=True)
            return 2
        result[name] = json.loads(r.stdout.strip().splitlines()[-1])
    print(json.dumps(result), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
