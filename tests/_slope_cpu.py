"""CPU oracle of the slope-based feature labels (include/bgnn_slope.h, data/slope_features.py): the reference's
``scripts/prepare_feature_labels.py`` restated on numpy / scipy, the fixture the reference's own code wrote
(tests/golden/make_golden_slope.py), and the helpers the device tests share.

The restatement keeps the script's arithmetic -- ``np.gradient`` on the raw float32 plane, ``degrees(arctan(sqrt(gx**2 + gy**2)))``
in float32, ``>`` against the threshold, ``ndimage.label`` with its default structure -- and replaces only the loop
``for i in range(1, n + 1): np.sum(labeled == i)`` by one ``np.bincount``."""
import json
import os

import numpy as np
from scipy import ndimage

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURE = os.path.join(HERE, "golden", "slope", "slope_features.npz")
NODATA = 1.0e6
STATS_NAMES = ("valid_cells", "steep_cells", "clusters", "kept_clusters", "kept_cells", "slope_feature_cells")
ULP_GUARD = 64


def squared_gradient(depth):
    """``gx**2 + gy**2`` as the script forms it (float32, NaN where the stencil holds one)."""
    depth = np.asarray(depth, np.float32)
    with np.errstate(all="ignore"):
        gy, gx = np.gradient(depth)
        return gx ** 2 + gy ** 2


def steep_mask(depth, slope_threshold=15.0):
    with np.errstate(all="ignore"):
        slope = np.degrees(np.arctan(np.sqrt(squared_gradient(depth))))
        return slope > float(slope_threshold)


def feature_mask(depth, slope_threshold=15.0, min_cluster_size=100):
    """``(mask, counts)``: the script's ``create_feature_mask_from_slope`` and the steep cells, clusters, kept clusters and kept
    cells on the way."""
    steep = steep_mask(depth, slope_threshold)
    labeled, n = ndimage.label(steep)
    sizes = np.bincount(labeled.ravel(), minlength=n + 1)
    keep = sizes >= min_cluster_size
    keep[0] = False
    mask = keep[labeled]
    return mask, {"steep_cells": int(steep.sum()), "clusters": int(n), "kept_clusters": int(keep.sum()), "kept_cells": int(mask.sum())}


def valid_cells(depth):
    depth = np.asarray(depth, np.float32)
    return (depth != np.float32(NODATA)) & np.isfinite(depth)


def wreck_pixels(wrecks, gt, shape):
    """The script's centre arithmetic: the (row, col) of the wrecks on the grid, in order."""
    out = []
    for x, y in wrecks:
        col = int((x - gt[0]) / gt[1])
        row = int((y - gt[3]) / gt[5])
        if 0 <= row < shape[0] and 0 <= col < shape[1]:
            out.append((row, col))
    return out


def add_feature_labels(depth, slope_threshold=15.0, min_cluster_size=100, wrecks=None, gt=None, wreck_radius=50):
    """``(labels, mask, stats, wreck count)``: the script's ``add_feature_labels`` on an array (int32 labels), with the six
    counts of the device's slope statistics block."""
    depth = np.asarray(depth, np.float32)
    valid = valid_cells(depth)
    mask, counts = feature_mask(depth, slope_threshold, min_cluster_size)
    labels = np.zeros(depth.shape, np.int32)
    labels[~valid] = -1
    labels[mask & valid] = 1
    stats = dict(counts, valid_cells=int(valid.sum()), slope_feature_cells=int((mask & valid).sum()))
    pixels = wreck_pixels(wrecks, gt, depth.shape) if wrecks else []
    yy, xx = np.ogrid[:depth.shape[0], :depth.shape[1]]
    for row, col in pixels:
        dist = np.sqrt((xx - col) ** 2 + (yy - row) ** 2)
        labels[(dist <= wreck_radius) & valid] = 1
    return labels, mask, stats, len(pixels)


def overlay(base_labels, depth, slope_threshold=15.0, min_cluster_size=100):
    """Overlay mode: ``(labels, stats)``; only cells labelled 0 may become 1, every other value passes through."""
    base = np.asarray(base_labels, np.int32)
    mask, counts = feature_mask(depth, slope_threshold, min_cluster_size)
    paint = mask & (base == 0)
    labels = np.where(paint, 1, base).astype(np.int32)
    return labels, dict(counts, valid_cells=int((base >= 0).sum()), slope_feature_cells=int(paint.sum()))


def stats_list(stats):
    return [stats[k] for k in STATS_NAMES]


def ulps_from_cut(depth, cut):
    """The smallest distance, in float32 steps, between a cell's ``s`` and ``cut`` (non-negative floats order as their bit
    patterns); a large number for a NaN cut or a plane without a non-NaN ``s``."""
    s = squared_gradient(depth)
    if np.isnan(cut):
        return 2 ** 31
    bits = s[~np.isnan(s)].view(np.uint32).astype(np.int64)
    return int(np.abs(bits - int(np.float32(cut).view(np.uint32))).min()) if bits.size else 2 ** 31


def load_fixture():
    """``(cases, cuts)``: name -> dict(depth, threshold, min_cluster_size, mask, labels or None, transform, wrecks, radius,
    wreck_count) and threshold -> the maker's cut bits."""
    z = np.load(FIXTURE)
    meta = json.loads(str(z["cases"]))
    cases = {}
    for name, m in meta.items():
        cases[name] = {"depth": z[m["plane"]], "threshold": m["threshold"], "min_cluster_size": m["min_cluster_size"],
                       "mask": z[name + "_mask"].astype(bool), "labels": z[name + "_labels"].astype(np.int32) if m["has_labels"] else None,
                       "transform": None if m["transform"] is None else tuple(m["transform"]),
                       "wrecks": None if m["wrecks"] is None else [tuple(p) for p in m["wrecks"]], "radius": m["radius"],
                       "wreck_count": m["wreck_count"]}
    cuts = {float(t): int(b) for t, b in zip(z["cut_thresholds"], z["cut_bits"])}
    return cases, cuts
