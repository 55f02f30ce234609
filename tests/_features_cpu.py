"""CPU oracle of the feature labels: the loop of the reference's ``create_feature_labels`` (scripts/extract_s57_features.py:824-862)
on a table of applied features ``(row, col, radius_px, label)``, with the painting confined to each disc's clamped bounding box so
that large cases stay cheap.  tests/test_host_features.py checks it bit for bit against the reference's own output on every golden
case; that is what licenses its use as the oracle where the labels are not the stock ones.  Also the golden loader, and the
resolution of a host plan (bin lists) on the CPU."""
import glob
import json
import os
from types import SimpleNamespace

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "features")
NODATA = 1.0e6
BIN = 64


def valid_mask(depth, nodata=NODATA):
    depth = np.asarray(depth)
    return (depth != nodata) & np.isfinite(depth)


def paint(table, paintable, labels):
    """Paints ``table`` in list order into ``labels`` (in place) on the cells of ``paintable``; returns the painted mask."""
    rows, cols = labels.shape
    painted = np.zeros(labels.shape, bool)
    for row, col, radius_px, label in np.asarray(table, dtype=np.int64).reshape(-1, 4):
        if radius_px < 0:
            continue
        r0, r1 = max(row - radius_px, 0), min(row + radius_px, rows - 1) + 1
        c0, c1 = max(col - radius_px, 0), min(col + radius_px, cols - 1) + 1
        yy, xx = np.ogrid[r0:r1, c0:c1]
        dist = np.sqrt((xx - col) ** 2 + (yy - row) ** 2)
        mask = (dist <= radius_px) & paintable[r0:r1, c0:c1]
        labels[r0:r1, c0:c1][mask] = label
        painted[r0:r1, c0:c1] |= mask
    return painted


def counts(labels, valid, painted):
    return {"valid_cells": int(valid.sum()), "feature_cells": int((labels == 1).sum()), "painted_cells": int(painted.sum())}


def feature_labels(table, depth, nodata=NODATA):
    """Depth mode: ``(labels int32, counts)``."""
    valid = valid_mask(depth, nodata)
    labels = np.where(valid, 0, -1).astype(np.int32)
    painted = paint(table, valid, labels)
    return labels, counts(labels, valid, painted)


def overlay_labels(table, base):
    """Overlay mode: only the zeros of ``base`` are painted."""
    base = np.asarray(base, dtype=np.int32)
    labels = base.copy()
    painted = paint(table, base == 0, labels)
    return labels, counts(labels, base >= 0, painted)


def resolve_plan(table, bin_ptr, bin_feat, paintable, labels):
    """What the kernel does with a plan: every paintable cell takes the label of the first feature of its bin's list that holds
    it (integer test).  ``labels`` is changed in place."""
    table = np.asarray(table, dtype=np.int64).reshape(-1, 4)
    rows, cols = labels.shape
    bins_c = -(-cols // BIN)
    for b in range(len(bin_ptr) - 1):
        r0, c0 = (b // bins_c) * BIN, (b % bins_c) * BIN
        sub, can = labels[r0:r0 + BIN, c0:c0 + BIN], paintable[r0:r0 + BIN, c0:c0 + BIN].copy()
        yy, xx = np.ogrid[r0:r0 + sub.shape[0], c0:c0 + sub.shape[1]]
        for k in bin_feat[bin_ptr[b]:bin_ptr[b + 1]]:
            row, col, radius_px, label = table[k]
            hit = can & ((xx - col) ** 2 + (yy - row) ** 2 <= radius_px * radius_px) & (radius_px >= 0)
            sub[hit] = label
            can &= ~hit
    return labels


def load_cases():
    """Every golden case: name, depth, labels, geotransform, features (objects with object_class / x / y), feature_radius and the
    recorded counts."""
    out = []
    for path in sorted(glob.glob(os.path.join(GOLDEN, "*.json"))):
        meta = json.load(open(path))
        z = np.load(path[:-5] + ".npz")
        out.append(SimpleNamespace(name=os.path.basename(path)[:-5], depth=z["depth"], labels=z["labels"], band_depth=z["band_depth"],
                                   transform=tuple(meta["geotransform"]), features=[SimpleNamespace(**f) for f in meta["features"]],
                                   feature_radius=meta["feature_radius"], meta=meta))
    return out
