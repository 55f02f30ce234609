"""Trained-like inputs for the accuracy tests, and the rule that bounds a kernel's distance to the float64 forward.

Depth enters the model raw (the extractor sees ``depth`` and ``local_mean`` un-normalised), so ``h1`` and layer 0's
pre-BatchNorm activations carry a common mode that grows with depth.  A trained checkpoint's layer-0 ``running_mean`` tracks
that common mode, so its BatchNorm subtracts two large, nearly equal numbers and amplifies whatever rounding happened before
the subtraction.  ``deep_tile`` puts a synthetic tile at survey depths; ``fit_batchnorm`` gives a state dict the running
statistics a model trained on the given graphs would have.  At depth, float32 arithmetic itself sits far from the true
(float64) result -- 1e-3 and more on the logits at -4000 m -- so a fixed absolute bar against the float32 oracle no longer
separates a correct kernel from a wrong one: ``float64_bound`` compares against float64 instead, relative to what float32
arithmetic achieves on the same input.
"""
import numpy as np
import torch

from oracle import gat_cpu, graph_cpu

from _calibration import calibrate_heads

DEPTH_BANDS = (-20.0, -200.0, -1000.0, -4000.0, -10000.0)
OUTPUT_KEYS = ("class_logits", "confidence", "correction", "hidden")

# The acceptance factor of float64_bound, chosen once from the exact-f32 path's measured ratios (distance to float64 over the
# float32 oracle's distance to float64, per output, over every band, both BatchNorm fits and every route of
# tests/test_gpu_conditioning.py on an MI355X): at most 1.8 on predict() / the backbone output, 2.5 on the tile routes'
# de-normalised correction.  The kernels sum in other orders than torch's CPU ops and fold BatchNorm into float32 scale /
# shift vectors, so they are neither systematically closer nor farther than float32 arithmetic; the float32 oracle summing
# its edges in reverse order lands at 0.9 .. 1.0.  The deliberate defects of tests/test_oracle_conditioning.py (h1 stored as
# bf16, layer 0's BatchNorm shift held in bf16, one neighbour dropped) land at 10^2 .. 10^5.  4 keeps a 1.6 x margin over
# the worst measured ratio and stays two orders of magnitude below every defect.
BOUND_C = 4.0
BOUND_FLOOR = 1e-6


def deep_tile(h, w, seed, variant="V0", depth=-20.0, slope=0.0, with_uncertainty=False):
    """``synthetic.synthetic_tile`` with its valid cells shifted so that they sit around ``depth`` metres (the synthetic
    field is centred near -20 m).  ``slope > 0`` adds a plane ramp falling ``slope`` metres per cell along the columns and
    ``slope / 2`` along the rows (0.05: a 5 % grade on a 1 m grid), so gradients, ``depth_difference`` and ``slope`` edge
    features are large too.  Invalid cells keep the nodata value 1e6.  Returns (depth f32, valid bool, uncertainty f32 |
    None) like ``synthetic_tile``."""
    from bathymetric_gnn_amd import synthetic
    d, m, u = synthetic.synthetic_tile(h, w, seed, variant, with_uncertainty)
    r = np.arange(h, dtype=np.float64)[:, None]
    c = np.arange(w, dtype=np.float64)[None, :]
    shifted = d.astype(np.float64) + (float(depth) + 20.0) - slope * (c + 0.5 * r)
    d = np.where(m, shifted, synthetic.NODATA).astype(np.float32)
    return d, m, u


def oracle_batch(graphs):
    """Block-diagonal batch (x, edge_index, edge_attr) of oracle graphs."""
    x, ei, ea, _, _ = graph_cpu.batch_graphs(graphs)
    return x, ei, ea


def fit_batchnorm(sd, graphs, calibrate=True, stat_dtype=np.float32, **calib):
    """A copy of ``sd`` whose every ``gnn.norms.{l}.module.running_mean`` / ``running_var`` is the float64 per-channel mean /
    biased variance of layer l's pre-BatchNorm output over the block-diagonal batch of ``graphs``, layer l + 1 fitted on the
    output of layer l's FITTED norm -- what a model trained on these graphs carries.

    One float64 training-mode forward of the oracle does this for any backbone: training-mode BatchNorm normalises each
    layer with the batch mean / biased variance, which is what eval mode does with the fitted statistics, so every layer
    sees the input it sees under the fit.  The running statistics it returns are 0.9 * old + 0.1 * mean and
    0.9 * old + 0.1 * unbiased variance; with the old ones set to zero the batch statistics come back exactly (to float64
    rounding).  ``stat_dtype``: float32 is what a checkpoint holds (and what the library is given); float64 keeps the exact
    fit.  ``calibrate``: then ``calibrate_heads`` on the same batch, so that classes and actions are mixed."""
    sd = dict(sd)
    L = gat_cpu.num_layers_of(sd)
    x, ei, ea = oracle_batch(graphs)
    zeroed = dict(sd)
    for l in range(L):
        pre = f"gnn.norms.{l}.module."
        zeroed[pre + "running_mean"] = np.zeros_like(np.asarray(sd[pre + "running_mean"]), np.float64)
        zeroed[pre + "running_var"] = np.zeros_like(np.asarray(sd[pre + "running_var"]), np.float64)
    stats = {}
    M = x.shape[0]
    gat_cpu.forward(zeroed, x, ei, ea, dtype=torch.float64, train_stats=stats)
    for l in range(L):
        pre = f"gnn.norms.{l}.module."
        mean = stats[pre + "running_mean"].numpy() / 0.1
        var = stats[pre + "running_var"].numpy() / 0.1 * ((M - 1) / M)
        sd[pre + "running_mean"] = mean.astype(stat_dtype)
        sd[pre + "running_var"] = var.astype(stat_dtype)
    if calibrate:
        sd = calibrate_heads(sd, x, ei, ea, **calib)
    return sd


def distances(out, ref, keys=OUTPUT_KEYS):
    """max |out - ref| per output key present in both (``out``: GPU tensors or oracle outputs)."""
    d = {}
    for k in keys:
        if k in out and k in ref and out[k] is not None:
            a = out[k].detach().double().cpu().reshape(ref[k].shape)
            d[k] = float((a - ref[k].double()).abs().max()) if a.numel() else 0.0
    return d


def float64_bound(out, ref32, ref64, c=BOUND_C, floor=BOUND_FLOOR, keys=OUTPUT_KEYS):
    """The acceptance rule for a forward at any depth: for every output (logits, confidence, correction, hidden) the
    distance of ``out`` to the float64 forward ``ref64`` is at most ``c`` x the float32 oracle's (``ref32``) distance to
    it, plus ``floor``.  Predicted classes must equal float64's wherever float64's top-2 probability gap exceeds 10 x the
    logit bound.  Returns (ok, report) -- report holds the distances, the bounds and the disagreeing-class count, for the
    assertion message and the tables."""
    d_out, d_32 = distances(out, ref64, keys), distances(ref32, ref64, keys)
    report = {"ok": True}
    for k, e in d_out.items():
        b = c * d_32[k] + floor
        report[k] = {"dist": e, "float32_dist": d_32[k], "bound": b}
        if not e <= b:                                   # (NaN fails)
            report["ok"] = False
    # the logit bound decides which classes are sure -- from the references, so that outputs without logits (the tile
    # routes' class grids) are held to the same rule
    lb = c * distances(ref32, ref64, ("class_logits",))["class_logits"] + floor
    top2 = torch.topk(ref64["class_probs"], 2, dim=-1).values
    sure = (top2[:, 0] - top2[:, 1]) > 10 * lb
    pc = out["predicted_class"] if "predicted_class" in out else out["class_logits"].argmax(-1)
    bad = int((pc.detach().cpu().long()[sure] != ref64["predicted_class"][sure]).sum())
    report["class_mismatch_on_sure"] = bad
    report["sure_fraction"] = float(sure.double().mean()) if sure.numel() else 1.0
    if bad:
        report["ok"] = False
    return report["ok"], report
