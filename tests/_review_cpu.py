"""CPU oracle of the review-region export (include/bgnn_review.h, data/review_regions.py): the reference's
``scripts/export_for_review.py`` restated twice on numpy / scipy, the fixture the reference's own code wrote, and the comparison the
device tests share.

``fast_regions``   ``ndimage.label`` once, ``np.bincount`` for the sizes, ``ndimage.find_objects`` for the boxes, a float64 mean per
                   kept region (numpy's pairwise sum over the region's cells: its error is a few 2^-53, far below the tolerances)
``slow_regions``   the script's loop as it stands: ``labeled == i`` over the whole raster once per region, ``np.mean`` of the
                   float32 cells -- for small inputs
"""
import json
import os

import numpy as np
from scipy import ndimage

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURE = os.path.join(HERE, "golden", "review", "review_regions.npz")
COUNT_NAMES = ("uncertain_cells", "regions", "kept_regions", "kept_cells")
# |device mean - float64 mean|: every cell enters as llrint(c * 2^32), at most 2^-33 off; the mean of n such errors is at most
# 2^-33; the one division and the oracle's float64 sum add a few 2^-53.  2^-32 covers them with a factor of two.
MEAN_ATOL = 2.0 ** -32


def uncertain_mask(confidence, low, high):
    """The script's mask.  numpy compares a float32 array with a Python float in float32: the bounds are rounded first (made
    explicit here, so that the result does not depend on numpy's promotion rules)."""
    confidence = np.asarray(confidence, np.float32)
    with np.errstate(invalid="ignore"):
        unc = (confidence >= np.float32(low)) & (confidence <= np.float32(high))
    return unc & np.isfinite(confidence)


def fast_regions(confidence, low=0.4, high=0.7, min_region_size=100):
    """``(regions, review_mask, counts)``: the reference's list of dictionaries (``mean_confidence`` a float64 mean), its boolean
    review mask, and the four counts of the device call."""
    confidence = np.asarray(confidence, np.float32)
    unc = uncertain_mask(confidence, low, high)
    labeled, n = ndimage.label(unc)
    sizes = np.bincount(labeled.ravel(), minlength=n + 1)
    boxes = ndimage.find_objects(labeled)
    kept = np.flatnonzero(sizes[1:] >= min_region_size) + 1
    keep_label = np.zeros(n + 1, bool)
    keep_label[kept] = True
    regions = []
    for i in kept:
        sl = boxes[i - 1]
        cells = confidence[sl][labeled[sl] == i].astype(np.float64)
        regions.append({"id": len(regions) + 1,
                        "size": int(sizes[i]),
                        "mean_confidence": float(np.sum(cells) / cells.size),
                        "bounds": {"min_row": int(sl[0].start), "max_row": int(sl[0].stop - 1),
                                   "min_col": int(sl[1].start), "max_col": int(sl[1].stop - 1)}})
    counts = dict(zip(COUNT_NAMES, (int(unc.sum()), int(n), int(kept.size), int(sizes[kept].sum()))))
    return regions, keep_label[labeled], counts


def slow_regions(confidence, low=0.4, high=0.7, min_region_size=100):
    """``(regions, review_mask)`` by the script's own loop (its statements, on arrays instead of a file)."""
    confidence = np.asarray(confidence, np.float32)
    uncertain = uncertain_mask(confidence, low, high)
    labeled, num_regions = ndimage.label(uncertain)
    review_mask = np.zeros_like(uncertain)
    regions = []
    for i in range(1, num_regions + 1):
        region_mask = labeled == i
        if np.sum(region_mask) >= min_region_size:
            review_mask |= region_mask
            rows, cols = np.where(region_mask)
            regions.append({"id": len(regions) + 1,
                            "size": int(np.sum(region_mask)),
                            "mean_confidence": float(np.mean(confidence[region_mask])),
                            "bounds": {"min_row": int(rows.min()), "max_row": int(rows.max()),
                                       "min_col": int(cols.min()), "max_col": int(cols.max())}})
    return regions, review_mask


def same_regions(got, want):
    """Count, order, ``id``, ``size`` and ``bounds`` equal, with the reference's keys, nesting and Python types."""
    assert len(got) == len(want), (len(got), len(want))
    for g, w in zip(got, want):
        assert list(g) == ["id", "size", "mean_confidence", "bounds"] and list(g["bounds"]) == ["min_row", "max_row", "min_col", "max_col"]
        assert type(g["id"]) is int and type(g["size"]) is int and type(g["mean_confidence"]) is float
        assert all(type(v) is int for v in g["bounds"].values())
        assert (g["id"], g["size"], g["bounds"]) == (w["id"], w["size"], w["bounds"]), (g, w)


def float32_mean_bound(size, mean):
    """|float32 np.mean - true mean| for ``size`` positive terms: any order of the ``size - 1`` float32 additions, and the division,
    each within 2^-24 relative."""
    return ((size - 1) + 1) * 2.0 ** -24 * mean


def check_device_result(result, confidence, low, high, min_region_size):
    """A ``ReviewRegions`` against ``fast_regions`` of the same planes: regions, means within ``MEAN_ATOL``, mask cell for cell,
    counts.  Returns the oracle's triple."""
    want, want_mask, want_counts = fast_regions(confidence, low, high, min_region_size)
    same_regions(result.regions, want)
    for g, w in zip(result.regions, want):
        assert abs(g["mean_confidence"] - w["mean_confidence"]) <= MEAN_ATOL, (g, w)
    mask = result.review_mask.cpu().numpy()
    assert mask.dtype == np.float32 and mask.shape == want_mask.shape
    assert np.array_equal(mask, want_mask.astype(np.float32))
    assert result.counts == want_counts, (result.counts, want_counts)
    return want, want_mask, want_counts


def load_fixture():
    """The cases of the fixture: ``name -> {confidence, classification, low, high, min_region_size, review_mask, regions}`` with
    the mask the reference wrote to band 1 and the list it dumped as JSON."""
    z = np.load(FIXTURE, allow_pickle=False)
    cases = {}
    for name in json.loads(str(z["names"])):
        low, high, min_size = (z[name + "_params"][k] for k in range(3))
        cases[name] = {"confidence": z[name + "_confidence"], "classification": z[name + "_classification"],
                       "low": float(low), "high": float(high), "min_region_size": int(min_size),
                       "review_mask": z[name + "_review_mask"], "regions": json.loads(str(z[name + "_regions"]))}
    return cases
