#!/usr/bin/env python3
"""Golden vectors for model evaluation, produced by the REFERENCE's own ``scripts/evaluate_model.py::compute_metrics``:

    BGNN_REFERENCE=<reference checkout> python tests/golden/make_golden_eval.py

The script is loaded with a stand-in for GDAL (_reference_scripts.py).  ``eval/<case>.npz`` holds the inputs (``labels`` int32,
``classification`` float32, ``confidence`` float32 unless the case has none), ``eval/<case>.json`` the dictionary the reference
returned (NaN written as JSON's ``NaN``).  Every assert looks at the reference's output alone.
"""
import json
import os
import sys
import warnings

sys.dont_write_bytecode = True
import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from _reference_scripts import load_reference_script, save_npz  # noqa: E402

ref, _ = load_reference_script("evaluate_model")
OUT = os.path.join(HERE, "eval")
F32 = np.float32
THRESHOLDS = [0.5, 0.6, 0.7, 0.8, 0.9]


def run(name, labels, classification, confidence=None):
    labels = np.ascontiguousarray(labels, np.int32)
    classification = np.ascontiguousarray(classification, F32)
    arrays = {"labels": labels, "classification": classification}
    if confidence is not None:
        confidence = np.ascontiguousarray(confidence, F32)
        arrays["confidence"] = confidence
    assert labels.shape == classification.shape and labels.ndim == 2 and labels.size <= 64 * 64
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")                      # the mean of an empty selection, comparisons with NaN
        m = ref.compute_metrics(labels, classification, confidence)
    size = save_npz(os.path.join(OUT, name + ".npz"), arrays)
    with open(os.path.join(OUT, name + ".json"), "w") as f:
        json.dump(m, f, indent=2, sort_keys=True)
        f.write("\n")
    print(f"{name:20s} {labels.shape[0]:2d} x {labels.shape[1]:2d}  total = {m['total_samples']:5d}  accuracy = {m['overall_accuracy']:.4f}  {size} bytes")
    return m


def random_planes(rng, h, w, classes=(0, 1, 2), accuracy=0.8):
    labels = rng.choice(classes, (h, w)).astype(np.int32)
    pred = np.where(rng.random((h, w)) < accuracy, labels, rng.choice(classes, (h, w))).astype(F32)
    conf = rng.random((h, w)).astype(F32)
    return labels, pred, conf


def main():
    os.makedirs(OUT, exist_ok=True)
    rng = np.random.default_rng(20240612)

    # random planes with labels -1 and NaN / negative predictions
    labels, pred, conf = random_planes(rng, 48, 40)
    labels[rng.random(labels.shape) < 0.1] = -1
    pred[rng.random(pred.shape) < 0.05] = np.nan
    pred[rng.random(pred.shape) < 0.05] = -1.0
    pred[3, 4], pred[5, 6] = np.inf, -np.inf
    m = run("random", labels, pred, conf)
    dropped = (labels < 0) | ~(pred >= 0) | ~np.isfinite(pred)
    assert m["total_samples"] == int((~dropped).sum()) < labels.size - 250 and (labels[np.isnan(pred)] >= 0).any()
    assert all(f"accuracy_at_{t}" in m["confidence"] for t in THRESHOLDS) and 0.7 < m["overall_accuracy"] < 0.95
    assert all(m[c]["false_positives"] > 0 and m[c]["false_negatives"] > 0 for c in ("seafloor", "feature", "noise"))

    # labels and predictions of 3 and 5: outside the three classes, yet counted, and correct when equal
    labels, pred, conf = random_planes(rng, 32, 32, classes=(0, 1, 2, 3, 5), accuracy=0.6)
    m = run("high_classes", labels, pred, conf)
    in3 = sum(sum(r) for r in m["confusion_matrix"])
    trace = sum(m["confusion_matrix"][i][i] for i in range(3))
    assert m["total_samples"] == 32 * 32 > in3 and round(m["overall_accuracy"] * 1024) > trace, "equal labels above 2 count as correct"
    assert m["noise"]["support"] > sum(m["confusion_matrix"][2]), "a prediction above 2 is a false negative outside the matrix"
    assert m["noise"]["false_positives"] > m["confusion_matrix"][0][2] + m["confusion_matrix"][1][2]

    # non-integer predictions: 0.5 -> 0, 1.7 -> 1
    labels, pred, conf = random_planes(rng, 24, 24)
    frac = rng.random(pred.shape)
    pred = np.where(frac < 0.3, F32(0.5), np.where(frac < 0.6, F32(1.7), pred)).astype(F32)
    m = run("fractional", labels, pred, conf)
    assert m["seafloor"]["true_positives"] >= int(((pred == F32(0.5)) & (labels == 0)).sum()) > 10
    assert m["feature"]["true_positives"] >= int(((pred == F32(1.7)) & (labels == 1)).sum()) > 10

    # confidences exactly at float32(t) and at both float32 neighbours, for all five thresholds; half the cells correct
    edges = []
    for t in THRESHOLDS:
        e = F32(t)
        edges += [np.nextafter(e, F32(0)), e, np.nextafter(e, F32(1))]
    conf = np.tile(np.array(edges, F32), 16).reshape(16, 15)
    labels = np.zeros((16, 15), np.int32)
    pred = (np.arange(16 * 15).reshape(16, 15) // 15 % 2).astype(F32)       # rows alternate correct / incorrect
    m = run("threshold_edges", labels, pred, conf)
    for t in THRESHOLDS:
        covered = int((conf >= F32(t)).sum())                 # float32 comparison: the edge itself is covered
        assert round(m["confidence"][f"coverage_at_{t}"] * 240) == covered, t
        assert (float(F32(t)) < t) == (t in (0.7, 0.9)) or t == 0.5
    assert (conf == F32(0.7)).sum() == 16 and float(F32(0.7)) < 0.7, "float32(0.7) < 0.7 and yet covered"
    assert round(m["confidence"]["coverage_at_0.7"] * 240) == int((conf.astype(np.float64) >= 0.7).sum()) + 16

    # nothing covered at 0.9: the keys are missing
    labels, pred, conf = random_planes(rng, 16, 16)
    conf = (conf * F32(0.85)).astype(F32)
    m = run("no_cover_09", labels, pred, conf)
    assert "accuracy_at_0.9" not in m["confidence"] and "coverage_at_0.9" not in m["confidence"] and "accuracy_at_0.8" in m["confidence"]

    # all correct, all incorrect: the integer fall-backs
    labels, pred, conf = random_planes(rng, 16, 20, accuracy=1.1)
    m = run("all_correct", labels, pred, conf)
    assert m["overall_accuracy"] == 1.0 and m["confidence"]["mean_incorrect"] == 0 and isinstance(m["confidence"]["mean_incorrect"], int)
    m = run("all_incorrect", labels, ((labels + 1) % 3).astype(F32), conf)
    assert m["overall_accuracy"] == 0.0 and m["confidence"]["mean_correct"] == 0 and isinstance(m["confidence"]["mean_correct"], int)
    assert all(m[c]["precision"] == 0 and m[c]["f1"] == 0 for c in ("seafloor", "feature", "noise"))

    # no counted cell
    labels, pred, conf = random_planes(rng, 8, 8)
    m = run("no_counted", np.full_like(labels, -1), pred, conf)
    assert m["total_samples"] == 0 and np.isnan(m["overall_accuracy"]) and "confidence" not in m

    # confidence=None
    labels, pred, _ = random_planes(rng, 20, 12)
    m = run("no_confidence", labels, pred, None)
    assert "confidence" not in m and m["total_samples"] == 240

    # a NaN confidence on a counted cell poisons the sums; an uncounted NaN does not matter
    labels, pred, conf = random_planes(rng, 12, 12)
    labels[0, 0] = -1
    conf[0, 0] = np.nan
    conf[1, 1] = np.nan
    pred[1, 1] = labels[1, 1]
    m = run("nan_confidence", labels, pred, conf)
    assert np.isnan(m["confidence"]["mean"]) and np.isnan(m["confidence"]["std"]) and np.isnan(m["confidence"]["mean_correct"])
    assert not np.isnan(m["confidence"]["mean_incorrect"]) and "coverage_at_0.5" in m["confidence"]

    # a constant confidence plane: the variance is zero
    labels, pred, _ = random_planes(rng, 30, 30)
    m = run("constant_confidence", labels, pred, np.full((30, 30), 0.8, F32))
    assert m["confidence"]["std"] < 1e-6 and abs(m["confidence"]["mean"] - float(F32(0.8))) < 1e-6


if __name__ == "__main__":
    main()
