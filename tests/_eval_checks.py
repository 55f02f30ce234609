"""Shared by the ground-truth / evaluation tests (host and GPU): the fixtures under tests/golden/truth and tests/golden/eval, a
numpy construction of the two device blocks from their definitions in include/bgnn_eval.h, and the comparison of a metrics /
statistics dictionary with the reference's.

Float tolerances.  Integers, and ratios of integers, are compared with ``==``.  The float sums (``mean_noise_magnitude``; the
confidence ``mean``, ``mean_correct``, ``mean_incorrect``, ``std``) are formed by the reference in float32 pairwise arithmetic, so
its values are not the yardstick: the same formula is evaluated here in float64.  A float64 sum of n values in [0, 1] carries at
most n * 2^-53 relative error (each of the n - 1 additions rounds once, relative 2^-53, and the terms share a sign or are bounded
by 1); the device forms the sum in another order and divides once more, so 4 * n * 2^-53 is allowed: relative on the means,
absolute on std^2 (a variance of values in [0, 1] is a difference of two such means, both at most 1; a constant plane must
therefore give std^2 <= that bound).  In addition the value under test may be no farther from the float64 value than the
fixture's float32 value is."""
import glob
import json
import math
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
TRUTH_CASES = sorted(os.path.basename(p)[:-4] for p in glob.glob(os.path.join(GOLDEN, "truth", "*.npz")))
EVAL_CASES = sorted(os.path.basename(p)[:-4] for p in glob.glob(os.path.join(GOLDEN, "eval", "*.npz")))
THRESHOLDS = (0.5, 0.6, 0.7, 0.8, 0.9)
CLASS_NAMES = ("seafloor", "feature", "noise")
_cache = {}


def sum_tolerance(n):
    return 4.0 * max(int(n), 1) * 2.0 ** -53


def load_case(kind, name):
    """The arrays of ``golden/<kind>/<name>.npz`` and the dictionary of its ``.json`` (loaded once; do not modify)."""
    if (kind, name) not in _cache:
        z = np.load(os.path.join(GOLDEN, kind, name + ".npz"), allow_pickle=False)
        arrays = {k: z[k] for k in z.files}
        for a in arrays.values():
            a.setflags(write=False)
        _cache[(kind, name)] = (arrays, json.load(open(os.path.join(GOLDEN, kind, name + ".json"))))
    return _cache[(kind, name)]


def truth_bands(g):
    """Bands 1-5 of a truth fixture (bands 3 / 4 of an uncropped pair are stored once, as the input depths)."""
    return [g["band1"], g["band2"], g.get("band3", g["noisy_depth"]), g.get("band4", g["clean_depth"]), g["band5"]]


def grids_of(g):
    """The fixture's two surveys as this package's ``BathymetricGrid`` (writable copies of the planes)."""
    from bathymetric_gnn_amd.data import BathymetricGrid
    out = []
    for side in ("clean", "noisy"):
        unc = g.get(side + "_uncertainty")
        out.append(BathymetricGrid(depth=g[side + "_depth"].copy(), uncertainty=None if unc is None else unc.copy(),
                                   transform=tuple(float(v) for v in g[side + "_transform"]), crs="EPSG:32619",
                                   resolution=tuple(float(v) for v in g[side + "_resolution"]),
                                   bounds=tuple(float(v) for v in g[side + "_bounds"]), source_path=None))
    return out


# ---- ground-truth statistics ------------------------------------------------------------------------------------------
def numpy_stats_block(labels, difference_band, offset):
    """The statistics block (runtime.GT_STATS_DTYPE) from label and masked difference planes, by its definition."""
    from bathymetric_gnn_amd import runtime
    b = np.zeros((), np.dtype(runtime.GT_STATS_DTYPE))
    noise, sea = labels == 2, labels == 0
    mag = np.abs(difference_band[noise])
    b["valid"], b["noise"], b["seafloor"] = int((labels >= 0).sum()), int(noise.sum()), int(sea.sum())
    b["noise_abs_sum"] = mag.astype(np.float64).sum()
    b["seafloor_sum"] = difference_band[sea].astype(np.float64).sum()
    b["offset"] = offset
    b["noise_abs_max"] = mag.max() if mag.size else 0.0
    return b


def check_stats(got, want, labels, difference_band):
    """``got``: the stats dictionary under test; ``want``: the reference's JSON; the planes: the reference's, for the float64 mean."""
    assert sorted(got) == sorted(want)
    for k in ("noise_threshold", "grid_shape", "valid_cells", "noise_cells", "noise_percentage", "seafloor_cells"):
        assert got[k] == want[k] and type(got[k]) is type(want[k]), k
    if "max_noise_magnitude" in want:
        assert got["max_noise_magnitude"] == want["max_noise_magnitude"]
        mag = np.abs(difference_band[labels == 2]).astype(np.float64)
        exact = mag.sum() / mag.size
        # (magnitudes above 1 m exist: the bound scales with the values, so it is taken relative, as for the means)
        err = abs(got["mean_noise_magnitude"] - exact)
        assert err <= sum_tolerance(mag.size) * exact, (err, exact)
        assert err <= abs(want["mean_noise_magnitude"] - exact)


# ---- evaluation -------------------------------------------------------------------------------------------------------
def counted_cells(labels, pred):
    with np.errstate(invalid="ignore"):
        valid = (labels >= 0) & (pred >= 0) & np.isfinite(pred)
    return valid, labels[valid].astype(np.int64), np.trunc(pred[valid].astype(np.float64)).astype(np.int64)


def numpy_eval_block(labels, pred, conf=None):
    """The accumulator block (runtime.EVAL_ACC_DTYPE) of one call, by its definition in the header."""
    from bathymetric_gnn_amd import runtime
    b = np.zeros((), np.dtype(runtime.EVAL_ACC_DTYPE))
    valid, yt, yp = counted_cells(labels, pred)
    correct = yt == yp
    b["total"], b["correct"] = yt.size, int(correct.sum())
    m = np.zeros((4, 4), np.int64)
    np.add.at(m, (np.minimum(yt, 3), np.minimum(yp, 3)), 1)
    b["confusion"] = m
    if conf is not None:
        c = conf[valid]
        e = c.astype(np.float64) - 0.5
        with np.errstate(invalid="ignore"):
            for j, t in enumerate(THRESHOLDS):
                cov = c >= np.float32(t)
                b["covered"][j], b["covered_correct"][j] = int(cov.sum()), int((cov & correct).sum())
        b["conf_sum"], b["conf_sq"] = e.sum(), (e * e).sum()
        b["conf_correct_sum"], b["conf_incorrect_sum"] = e[correct].sum(), e[~correct].sum()
        b["conf_cells"] = yt.size
    return b


def reference_formula_float64(labels, pred, conf):
    """The reference's confidence statistics evaluated in float64 on the same planes."""
    valid, yt, yp = counted_cells(labels, pred)
    c = conf[valid].astype(np.float64)
    correct = yt == yp
    out = {"n": c.size, "mean": c.mean() if c.size else math.nan, "var": c.var() if c.size else math.nan}
    out["mean_correct"] = (c[correct].mean(), int(correct.sum())) if correct.any() else (0, 0)
    out["mean_incorrect"] = (c[~correct].mean(), int((~correct).sum())) if (~correct).any() else (0, 0)
    return out


def _same(a, b):
    """Equal values of equal type (NaN equals NaN)."""
    if isinstance(a, float) and isinstance(b, float) and math.isnan(a) and math.isnan(b):
        return True
    return a == b and type(a) is type(b)


def check_metrics(got, want, labels, pred, conf=None, fixture=True):
    """``got``: the dictionary under test; ``want``: the reference's JSON for the same planes (``fixture=False``: a float64 replay
    in numpy instead, whose float sums are no float32 values to be closer than)."""
    assert sorted(got) == sorted(want)
    assert _same(got["total_samples"], want["total_samples"])
    assert _same(got["overall_accuracy"], want["overall_accuracy"]), (got["overall_accuracy"], want["overall_accuracy"])
    for name in CLASS_NAMES:
        assert sorted(got[name]) == sorted(want[name])
        for k, v in want[name].items():
            assert _same(got[name][k], v), (name, k, got[name][k], v)
    assert got["confusion_matrix"] == want["confusion_matrix"]
    assert all(type(v) is int for row in got["confusion_matrix"] for v in row)
    if "confidence" not in want:
        return
    gc, wc = got["confidence"], want["confidence"]
    assert sorted(gc) == sorted(wc)
    for k, v in wc.items():
        if k.startswith(("accuracy_at_", "coverage_at_")):
            assert _same(gc[k], v), (k, gc[k], v)
    ref = reference_formula_float64(labels, pred, conf)
    tol = sum_tolerance(ref["n"])
    for k in ("mean", "mean_correct", "mean_incorrect"):
        exact, n = (ref[k], ref["n"]) if k == "mean" else ref[k]
        if n == 0:                                            # the reference's integer 0
            assert _same(gc[k], wc[k]) and gc[k] == 0, k
        elif math.isnan(exact):
            assert math.isnan(gc[k]) and math.isnan(wc[k]), k
        else:
            err = abs(gc[k] - exact)
            assert err <= sum_tolerance(n) * abs(exact), (k, gc[k], exact)
            assert not fixture or err <= abs(wc[k] - exact), (k, gc[k], wc[k], exact)
    if math.isnan(ref["var"]):
        assert math.isnan(gc["std"]) and math.isnan(wc["std"])
    else:
        assert abs(gc["std"] ** 2 - ref["var"]) <= tol, (gc["std"], ref["var"])
        assert not fixture or abs(gc["std"] - math.sqrt(ref["var"])) <= abs(wc["std"] - math.sqrt(ref["var"])), (gc["std"], wc["std"], ref["var"])
