#!/usr/bin/env python3
"""Golden vectors for the multi-task training loss, produced by the REFERENCE's own ``training/losses.py``:

    python tests/golden/make_golden_loss.py /path/to/reference

The module is loaded by file path (the reference's ``training/__init__`` pulls in the trainer with its PyG / GDAL / tqdm
imports).  Each fixture (``loss/<case>.npz``) holds the float32 inputs, the reference's six values and the gradients of ``total``
with respect to class_logits / confidence / correction on those inputs (``ref32_*`` / ``g32_*``) and on their float64 copies
(``ref64_*`` / ``g64_*``), and the integer counts behind the two count-derived terms.  For the float64 run the name ``F`` in the
reference module is replaced by a stand-in that forwards everything to ``torch.nn.functional`` and casts the target of
``binary_cross_entropy`` to the input's dtype (as written the reference raises "Found dtype Float but expected Double"); nothing
else is touched.  ``loss/helpers.npz`` holds ``compute_class_weights`` / ``compute_correction_delta`` cases and
``loss/signatures.json`` the signatures with their defaults.
"""
import importlib.util
import inspect
import json
import os
import sys

sys.dont_write_bytecode = True
import numpy as np
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
REF = sys.argv[1] if len(sys.argv) > 1 else os.environ.get("BGNN_REFERENCE", "")
spec = importlib.util.spec_from_file_location("ref_losses", os.path.join(REF, "training", "losses.py"))
L = importlib.util.module_from_spec(spec)
sys.modules["ref_losses"] = L
spec.loader.exec_module(L)
OUT = os.path.join(HERE, "loss")
TERMS = ("classification", "correction", "confidence", "feature_preservation", "shoal_safety", "total")


class _CastingF:
    """``torch.nn.functional`` with the 0/1 target of binary_cross_entropy cast to the input's dtype."""

    def __getattr__(self, name):
        return getattr(F, name)

    @staticmethod
    def binary_cross_entropy(input, target, *a, **k):
        return F.binary_cross_entropy(input, target.to(input.dtype), *a, **k)


def run(inp, dtype, class_weights, eps, delta):
    L.F = _CastingF() if dtype == torch.float64 else F
    try:
        w = None if class_weights is None else torch.from_numpy(class_weights).to(dtype)
        crit = L.BathymetricGNNLoss(class_weights=w, label_smoothing=eps, correction_delta=delta)
        outputs = {"predicted_class": torch.from_numpy(inp["predicted_class"])}
        leaves = {}
        for k in ("class_logits", "confidence", "correction"):
            if k in inp:
                leaves[k] = outputs[k] = torch.from_numpy(inp[k]).to(dtype).requires_grad_(True)
        targets = {"class_labels": torch.from_numpy(inp["class_labels"])}
        if "correction_targets" in inp:
            targets["correction_targets"] = torch.from_numpy(inp["correction_targets"]).to(dtype)
        if "noise_mask" in inp:
            targets["noise_mask"] = torch.from_numpy(inp["noise_mask"])
        losses = crit(outputs, targets)
        assert tuple(losses) == TERMS
        losses["total"].backward()
        vals = {k: losses[k].detach().numpy().copy() for k in TERMS}
        grads = {k: v.grad.numpy().copy() for k, v in leaves.items() if v.grad is not None}
        return vals, grads
    finally:
        L.F = F


def inputs(n, c=3, seed=0, mix=(0.7, 0.1, 0.2)):
    rng = np.random.default_rng(7000 + seed)
    mix = np.asarray(mix, np.float64)
    labels = rng.choice(len(mix), size=n, p=mix / mix.sum()).astype(np.int64)
    logits = (2.0 * rng.standard_normal((n, c))).astype(np.float32)
    agree = rng.random(n) < 0.6                       # the model is right on most rows, so both BCE branches are populated
    logits[np.arange(n)[agree], labels[agree]] += np.float32(3.0)
    pred = logits.argmax(axis=1).astype(np.int64)
    conf = (1.0 / (1.0 + np.exp(-2.0 * rng.standard_normal(n)))).astype(np.float32)
    corr = (1.5 * rng.standard_normal(n)).astype(np.float32)
    tgt = (1.5 * rng.standard_normal(n)).astype(np.float32)
    return dict(class_logits=logits, confidence=conf, correction=corr, predicted_class=pred, class_labels=labels,
                correction_targets=tgt, noise_mask=labels == 2)


def make(name, inp, class_weights=None, eps=0.0, delta=1.0):
    cw = None if class_weights is None else np.asarray(class_weights, np.float32)
    v32, g32 = run(inp, torch.float32, cw, eps, delta)
    v64, g64 = run(inp, torch.float64, cw, eps, delta)
    y, q = inp["class_labels"], inp["predicted_class"]
    fp = (y == 0) & (q == 2)
    tgt = inp.get("correction_targets")
    fx = dict(inp, label_smoothing=np.float64(eps), delta=np.float64(delta), n=np.int64(len(y)),
              n_feature_as_noise=np.int64(((y == 1) & (q == 2)).sum()), n_false_positives=np.int64(fp.sum()),
              n_shoal=np.int64((fp & (tgt < 0)).sum() if tgt is not None else 0),
              n_deep=np.int64((fp & ~(tgt < 0)).sum() if tgt is not None else 0))
    if cw is not None:
        fx["class_weights"] = cw
    for k in TERMS:
        assert v32[k].dtype == np.float32 and v32[k].shape == (), (name, k, v32[k].dtype)
        fx["ref32_" + k], fx["ref64_" + k] = v32[k], v64[k]
    assert set(g32) == set(g64)
    for k in g32:
        assert g32[k].dtype == np.float32 and g64[k].dtype == np.float64
        fx["g32_" + k], fx["g64_" + k] = g32[k], g64[k]
    path = os.path.join(OUT, name + ".npz")
    np.savez_compressed(path, **fx)
    assert os.path.getsize(path) <= 200_000, (name, os.path.getsize(path))
    print(f"{name}: n={len(y)} " + " ".join(f"{k}={float(v64[k]):.6g}" for k in TERMS) + f" grads={sorted(g32)} bytes={os.path.getsize(path)}")
    return fx


def drop(inp, *keys):
    return {k: v for k, v in inp.items() if k not in keys}


def main():
    os.makedirs(OUT, exist_ok=True)
    make("n1", inputs(1, seed=1, mix=(0, 0, 1)))
    make("n2", inputs(2, seed=2))
    make("n257_weighted_smoothed", inputs(257, seed=3), class_weights=(0.4, 1.7, 0.9), eps=0.1)
    fx = make("n2049_plain", inputs(2049, seed=4))
    assert fx["n_false_positives"] and fx["n_shoal"] and fx["n_deep"] and fx["n_feature_as_noise"]
    make("c5", inputs(300, c=5, seed=5, mix=(0.5, 0.1, 0.2, 0.1, 0.1)), class_weights=(1.0, 2.0, 0.5, 1.5, 0.75), eps=0.05, delta=0.8)
    i = inputs(200, seed=6)
    i["noise_mask"] = np.zeros(200, bool)
    fx = make("no_masked_row", i)
    assert float(fx["ref64_correction"]) == 0.0 and "g64_correction" not in fx
    make("no_noise_mask", drop(inputs(200, seed=7), "noise_mask"), delta=1.25)
    i = inputs(200, seed=8)
    i["class_logits"][i["class_labels"] == 0, 2] = -30.0
    i["predicted_class"] = i["class_logits"].argmax(axis=1).astype(np.int64)
    fx = make("no_false_positive", i)
    assert fx["n_false_positives"] == 0 and float(fx["ref64_shoal_safety"]) == 0.0
    make("no_correction", drop(inputs(200, seed=9), "correction"), eps=0.1)
    fx = make("no_correction_targets", drop(inputs(200, seed=10), "correction_targets"))
    assert float(fx["ref64_shoal_safety"]) == 0.0 and float(fx["ref64_correction"]) == 0.0
    i = inputs(120, seed=11)
    i["class_labels"][[0, 17, 50, 51, 119]] = -100
    make("ignored5", i, class_weights=(0.4, 1.7, 0.9), eps=0.1)
    # saturated: confidences exactly 0, 1 and 1 - 2^-24 on both sides of t, and a row whose softmax rounds to (1, 0, 0)
    i = inputs(8, seed=12)
    i["class_logits"][0] = i["class_logits"][1] = (40.0, -40.0, 0.0)
    i["predicted_class"] = i["class_logits"].argmax(axis=1).astype(np.int64)
    i["class_labels"] = i["predicted_class"].copy()
    i["class_labels"][1::2] = (i["class_labels"][1::2] + 1) % 3                      # t = 1, 0, 1, 0, ...
    near_one = np.float32(1.0) - np.float32(2.0 ** -24)
    assert near_one < 1.0
    i["confidence"] = np.array([0.0, 0.0, 1.0, 1.0, near_one, near_one, 0.5, 0.3], np.float32)
    i["noise_mask"] = np.array([1, 0, 1, 0, 1, 1, 0, 1], bool)
    fx = make("saturated", i, eps=0.1)
    assert all(np.isfinite(fx["ref64_" + k]) for k in TERMS) and np.isfinite(fx["g64_confidence"]).all()
    fx = make("n0", inputs(0, seed=13))
    assert np.isnan(fx["ref64_total"]) and float(fx["ref64_correction"]) == 0.0 and float(fx["ref64_shoal_safety"]) == 0.0

    # the two helpers
    h = {}
    for j, (cnt, nc, sm) in enumerate((((900, 20, 80), 3, 0.1), ((5, 0, 5), 3, 0.1), ((1, 2, 3, 4, 5), 5, 0.05))):
        lab = np.random.default_rng(j).permutation(np.repeat(np.arange(len(cnt)), cnt)).astype(np.int64)
        h[f"cw{j}_labels"], h[f"cw{j}_args"] = lab, np.array([nc, sm], np.float64)
        h[f"cw{j}_weights"] = L.compute_class_weights(torch.from_numpy(lab), num_classes=nc, smoothing=sm).numpy()
    rng = np.random.default_rng(99)
    for j, (arr, pct, md) in enumerate(((2.0 * rng.standard_normal(1000), 95.0, 1.0), (0.2 * rng.standard_normal(64).astype(np.float32), 90.0, 0.5),
                                       (np.zeros(0), 95.0, 1.0))):
        h[f"cd{j}_corrections"], h[f"cd{j}_args"] = arr, np.array([pct, md], np.float64)
        h[f"cd{j}_delta"] = np.float64(L.compute_correction_delta(arr, percentile=pct, min_delta=md))
    np.savez_compressed(os.path.join(OUT, "helpers.npz"), **h)

    def params(fn):
        return [[n, None if p.default is inspect.Parameter.empty else p.default] for n, p in inspect.signature(fn).parameters.items()
                if n != "self"]
    sig = {}
    for cls in (L.BathymetricGNNLoss, L.ClassificationLoss, L.CorrectionLoss, L.ConfidenceCalibrationLoss, L.FeaturePreservationLoss,
                L.ShoalSafetyLoss):
        sig[cls.__name__] = {"__init__": params(cls.__init__), "forward": params(cls.forward)}
    for fn in (L.compute_class_weights, L.compute_correction_delta):
        sig[fn.__name__] = params(fn)
    crit = L.BathymetricGNNLoss()
    sig["attributes"] = sorted(k for k in list(vars(crit)) + list(crit._modules) if not k.startswith("_") and k != "training")
    json.dump(sig, open(os.path.join(OUT, "signatures.json"), "w"), indent=1)


if __name__ == "__main__":
    main()
