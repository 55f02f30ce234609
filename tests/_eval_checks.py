"""Shared by the ground-truth / evaluation tests (host and GPU): the fixtures under tests/golden/truth and tests/golden/eval, a
numpy construction of the two device blocks from their definitions in include/bgnn_eval.h, and the comparison of a metrics /
statistics dictionary with the reference's.  Further down: the order-preserving key of a float32 and its inverse, the median rule
and the whole ground truth in numpy (``truth_oracle``), and the inputs test_gpu_truth_eval_edges.py constructs from seeded
generators (test_host_ground_truth.py checks them without a GPU).

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
import types

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
    # (a prediction beyond int64 is clamped to 2^62 before the cast: an int32 label never equals it, and it is ">= 3" either way)
    return valid, labels[valid].astype(np.int64), np.minimum(np.trunc(pred[valid].astype(np.float64)), 2.0 ** 62).astype(np.int64)


def numpy_eval_block(labels, pred, conf=None):
    """The accumulator block (runtime.EVAL_ACC_DTYPE) of one call, by its definition in the header."""
    from bathymetric_gnn_amd import runtime
    b = np.zeros((), np.dtype(runtime.EVAL_ACC_DTYPE))
    valid, yt, yp = counted_cells(labels, pred)
    correct = yt == yp
    b["total"], b["correct"] = yt.size, int(correct.sum())
    b["confusion"] = np.bincount(np.minimum(yt, 3) * 4 + np.minimum(yp, 3), minlength=16).reshape(4, 4)
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


# ---- ground truth: the numpy oracle -------------------------------------------------------------------------------------
F32 = np.float32
NODATA = 1.0e6
# two full trips of the largest grid a streaming pass launches, three more tiles and three cells: every workgroup walks its
# grid-stride loop at least twice, some three times, the last tile is ragged and the last thread's 4-cell load is partial.  (The
# tests establish "past the largest grid" through the workspace sizes, which stop growing there.)
PAST_ONE_GRID_CELLS = 2 * 2048 * 1024 + 3 * 1024 + 3


def order_key(v):
    """The order-preserving uint32 image of float32 values: key(a) < key(b) exactly when a < b, with -0.0 one below +0.0."""
    u = np.asarray(v, F32).view(np.uint32)
    return np.where(u >> 31 != 0, ~u, u | np.uint32(0x80000000)).astype(np.uint32)


def key_value(k):
    """The inverse of ``order_key``."""
    k = np.asarray(k, np.uint32)
    return np.where(k >> 31 != 0, k & np.uint32(0x7FFFFFFF), ~k).astype(np.uint32).view(F32)


def key_digits(k):
    """The three digits (11, 11 and 10 bits, from the top) the selection narrows a key by."""
    k = int(k)
    return k >> 21, (k >> 10) & 0x7FF, k & 0x3FF


def median_rule(values):
    """The offset by the rule make_golden_truth.py checks against the reference: the middle element of the sorted values, or
    the float32 sum of the two middle ones halved in float32 (NaN without a value)."""
    s = np.sort(np.asarray(values, F32))
    n = s.size
    if n == 0:
        return F32(np.nan)
    return s[(n - 1) // 2] if n % 2 else F32(s[n // 2 - 1] + s[n // 2]) / F32(2)


def truth_oracle(clean, noisy, threshold=0.15, nodata=NODATA, unc=None):
    """Ground truth of a float32 pair in numpy: validity, raw difference, the offset by ``median_rule``, difference, labels, the
    masked uncertainty and the statistics block (float sums in float64)."""
    assert clean.dtype == F32 and noisy.dtype == F32
    with np.errstate(over="ignore", invalid="ignore"):
        valid = np.isfinite(clean) & np.isfinite(noisy) & (clean != F32(nodata)) & (noisy != F32(nodata))
        raw = noisy - clean
        offset = median_rule(raw[valid])
        difference = np.where(valid, raw - offset, F32(np.nan)).astype(F32)
        labels = np.where(valid, np.where(np.abs(difference) > F32(threshold), 2, 0), -1).astype(np.int32)
    masked = None if unc is None else np.where(valid, unc, F32(np.nan)).astype(F32)
    return types.SimpleNamespace(valid=valid, raw=raw, offset=offset, difference=difference, labels=labels, uncertainty=masked,
                                 block=numpy_stats_block(labels, difference, offset))


def same_values(a, b):
    """Equal in value, NaN in the same places (signed zeros compare equal)."""
    return np.array_equal(a, b, equal_nan=True)


def check_truth(labels, difference, uncertainty, block, want, sums=True):
    """Host copies of what ``ground_truth_build`` returned (``block``: a record of runtime.GT_STATS_DTYPE) against a
    ``truth_oracle``: labels and counts with ``==``, planes, offset and maximum by value, the two float64 sums within
    ``sum_tolerance(n)`` relative to the sum of the terms' magnitudes (the oracle's own pairwise float64 sum errs by about
    log2(n) * 2^-53 of that, far inside the bound)."""
    assert labels.dtype == np.int32 and np.array_equal(labels, want.labels)
    assert difference.dtype == F32 and same_values(difference, want.difference)
    if want.uncertainty is None:
        assert uncertainty is None
    else:
        assert uncertainty.dtype == F32 and same_values(uncertainty, want.uncertainty)
    for k in ("valid", "noise", "seafloor"):
        assert int(block[k]) == int(want.block[k]), (k, int(block[k]), int(want.block[k]))
    assert same_values(F32(block["offset"]), want.offset), (block["offset"], want.offset)
    assert F32(block["noise_abs_max"]) == want.block["noise_abs_max"], (block["noise_abs_max"], want.block["noise_abs_max"])
    if sums:
        for k, terms in (("noise_abs_sum", np.abs(want.difference[want.labels == 2])), ("seafloor_sum", want.difference[want.labels == 0])):
            terms = terms.astype(np.float64)
            err, bound = abs(float(block[k]) - terms.sum()), sum_tolerance(terms.size) * np.abs(terms).sum()
            print(f"{k}: {float(block[k])!r} against {terms.sum()!r}, error {err:.3e}, bound {bound:.3e}")
            assert err <= bound, (k, err, bound)


# ---- ground truth: constructed inputs -----------------------------------------------------------------------------------
def _frozen(*arrays):
    for a in arrays:
        if a is not None:
            a.setflags(write=False)
    return arrays


def past_one_grid_pair():
    """``(clean, noisy, unc)`` of PAST_ONE_GRID_CELLS cells as one flat plane: depth -40 +- 10 m, difference 0.3 sigma - 0.05,
    2 % nodata in clean, 2 % NaN in noisy, uniform uncertainty (built once; do not modify)."""
    if "pair" not in _cache:
        rng = np.random.default_rng(20240701)
        n = PAST_ONE_GRID_CELLS
        clean = (-40 + 10 * rng.standard_normal(n)).astype(F32)
        noisy = (clean + (0.3 * rng.standard_normal(n) - 0.05).astype(F32)).astype(F32)
        clean[rng.random(n) < 0.02] = NODATA
        noisy[rng.random(n) < 0.02] = np.nan
        _cache["pair"] = _frozen(clean, noisy, rng.random(n, dtype=F32))
    return _cache["pair"]


def past_one_grid_truth(start=0):
    """The oracle of ``past_one_grid_pair()[start:]`` at the default threshold (computed once per ``start``)."""
    if ("pair_truth", start) not in _cache:
        clean, noisy, unc = past_one_grid_pair()
        _cache[("pair_truth", start)] = truth_oracle(clean[start:], noisy[start:], 0.15, unc=unc[start:])
    return _cache[("pair_truth", start)]


def exact_pair(values, rng, invalid=7, nodata=NODATA, extra=None):
    """A flat pair whose valid raw differences are exactly ``values`` (clean depth 0, as ``exact()`` of make_golden_truth.py),
    shuffled, with ``invalid`` invalid cells of four kinds mixed in.  ``extra``: ``(clean, noisy)`` cells appended as they are."""
    values = np.asarray(values, F32)
    bad_clean = np.array([nodata, 0, 0, 0, np.nan, -np.inf, 0], F32)
    bad_noisy = np.array([1, np.nan, np.inf, nodata, 1, 1, -np.inf], F32)
    pick = np.arange(invalid) % bad_clean.size
    clean = np.concatenate([np.zeros(values.size, F32), bad_clean[pick]] + ([] if extra is None else [np.asarray(extra[0], F32)]))
    noisy = np.concatenate([values, bad_noisy[pick]] + ([] if extra is None else [np.asarray(extra[1], F32)]))
    perm = rng.permutation(clean.size)
    unc = (0.2 + 0.1 * rng.random(clean.size)).astype(F32)
    return clean[perm], noisy[perm], unc


def _uniform_values(rng, n):
    v = rng.integers(0, 2 ** 32, 2 * n, dtype=np.uint64).astype(np.uint32).view(F32)
    with np.errstate(invalid="ignore"):
        v = v[np.isfinite(v) & (np.abs(v) < F32(1e38))]     # (the float32 sum of the middle pair cannot overflow)
    assert v.size >= n
    return v[:n]


def _around(rng, lo, hi, below, above, copies):
    """``below`` values under ``lo``, ``copies`` each of ``lo`` and ``hi``, ``above`` values over ``hi`` (all within 0.3 .. 1.6,
    so both neighbours' top-level bins hold other keys too)."""
    assert 0.31 < lo <= hi < 1.59
    return np.concatenate([rng.uniform(0.3, float(lo) - 0.0005, below), np.full(copies, lo), np.full(copies, hi),
                           rng.uniform(float(hi) + 0.0005, 1.6, above)]).astype(F32)


STRADDLE_KEYS = {                                             # the lower and the upper middle key
    "straddle_level1": ((0x5FA << 21) | 0x1FFFFF, 0x5FB << 21),                                    # 0.87499994 | 0.875
    "straddle_level2": (((((0x5FA << 11) | 0x3FF) << 10) | 0x3FF), ((0x5FA << 11) | 0x400) << 10),   # 0.81249994 | 0.8125
}
BIN_OWNER_KEYS = {"first_bin_owner": 0x5FA << 21, "last_bin_owner": (0x5FA << 21) | 0x1FFFFF}           # 0.75 | 0.87499994
ADVERSARIAL_CASES = ("uniform_keys_4098", "uniform_keys_4099", "straddle_level1", "straddle_level2", "first_bin_owner",
                     "last_bin_owner", "denormals", "signed_zeros", "overflow_tails", "other_nodata")
DENORMAL_LIMIT = F32(2.0 ** -127)                             # values below it differ by less than the smallest normal number


def adversarial_case(name):
    """One constructed pair for the selection (built once; do not modify): ``clean``, ``noisy``, ``unc`` (flat float32),
    ``threshold``, ``nodata``, ``sums`` (whether the float sums are finite and checked), and ``values``, the raw differences
    that were put in (None where the planes were not built from values)."""
    if ("case", name) in _cache:
        return _cache[("case", name)]
    rng = np.random.default_rng([20240702, ADVERSARIAL_CASES.index(name)])
    nodata, sums, extra = NODATA, True, None
    if name.startswith("uniform_keys_"):
        values = _uniform_values(rng, int(name.rsplit("_", 1)[1]))
    elif name in STRADDLE_KEYS:                               # even: the middle pair is the last copy of lo and the first of hi
        lo, hi = (key_value(k) for k in STRADDLE_KEYS[name])
        values = _around(rng, lo, hi, 700, 700, 300)
    elif name == "first_bin_owner":                           # odd; the median is the first of 200 copies: n = 2 * 900 + 1
        v = key_value(BIN_OWNER_KEYS[name])
        values = _around(rng, v, v, 900, 701, 100)
    elif name == "last_bin_owner":                            # odd; the median is the last of 200 copies: n = 2 * (900 + 199) + 1
        v = key_value(BIN_OWNER_KEYS[name])
        values = _around(rng, v, v, 900, 1099, 100)
    elif name == "denormals":
        bits = rng.integers(1, 0x400000, 1001).astype(np.uint32) | (rng.integers(0, 2, 1001).astype(np.uint32) << 31)
        values = bits.view(F32)
    elif name == "signed_zeros":                              # 600 of 1000 are zeros; the middle pair is (-0.0, +0.0)
        values = np.concatenate([rng.uniform(-0.5, -0.01, 200), np.full(300, -0.0), np.full(300, 0.0), rng.uniform(0.01, 0.5, 200)]).astype(F32)
    elif name == "overflow_tails":                            # finite operands whose float32 difference is +-inf: valid cells
        values = (0.3 * rng.standard_normal(2001) - 0.05).astype(F32)
        extra = (np.array([-3e38] * 3 + [3e38] * 4, F32), np.array([3e38] * 3 + [-3e38] * 4, F32))
        sums = False
    elif name == "other_nodata":                              # -9999 is the nodata; 1.0e6 is a depth like any other
        n, nodata, values = 3001, -9999.0, None
        clean = (-40 + 10 * rng.standard_normal(n)).astype(F32)
        noisy = (clean + (0.3 * rng.standard_normal(n) - 0.05).astype(F32)).astype(F32)
        for plane, value, share in ((clean, -9999.0, 0.03), (noisy, -9999.0, 0.03), (clean, 1.0e6, 0.01), (noisy, 1.0e6, 0.01), (noisy, np.nan, 0.02)):
            plane[rng.random(n) < share] = value
        unc = rng.random(n, dtype=F32)
    else:
        raise KeyError(name)
    if values is not None:
        clean, noisy, unc = exact_pair(values, rng, invalid=6 if name == "denormals" else 7, extra=extra)
        values = _frozen(np.asarray(values, F32))[0]
    clean, noisy, unc = _frozen(clean, noisy, unc)
    _cache[("case", name)] = types.SimpleNamespace(name=name, clean=clean, noisy=noisy, unc=unc, threshold=0.15, nodata=nodata,
                                                   sums=sums, values=values)
    return _cache[("case", name)]


def adversarial_truth(name):
    """The oracle of ``adversarial_case(name)`` (computed once)."""
    if ("case_truth", name) not in _cache:
        c = adversarial_case(name)
        _cache[("case_truth", name)] = truth_oracle(c.clean, c.noisy, c.threshold, c.nodata, c.unc)
    return _cache[("case_truth", name)]


# ---- evaluation: constructed inputs -------------------------------------------------------------------------------------
def past_one_grid_eval():
    """``(labels, pred, conf)`` of PAST_ONE_GRID_CELLS cells as flat planes: labels from {-1, 0, 1, 2, 4}, predictions 85 % right
    and 3 % NaN, uniform confidence (built once; do not modify)."""
    if "eval" not in _cache:
        rng = np.random.default_rng(20240703)
        n = PAST_ONE_GRID_CELLS
        labels = rng.choice(np.array([-1, 0, 1, 2, 4], np.int32), n, p=[.1, .5, .1, .25, .05])
        pred = np.where(rng.random(n) < 0.85, labels, rng.integers(0, 4, n)).astype(F32)
        pred[rng.random(n) < 0.03] = np.nan
        _cache["eval"] = _frozen(labels, pred, rng.random(n, dtype=F32))
    return _cache["eval"]


ODD_PREDICTIONS = (-0.0, 2.9999998, 3.0, 1e30, np.inf, -np.inf, -0.5, 0.0, 1.0, 2.0)
ODD_LABELS = (0, 1, 2, 3, 2 ** 31 - 1, -2 ** 31, -1)


def odd_eval_planes():
    """``(labels, pred, conf)`` of 351 cells: every pair of ODD_LABELS x ODD_PREDICTIONS five times over, each time with another
    of 21 confidences -- ``float32(t)`` and both float32 neighbours for each threshold, values below 0 and above 1 -- shuffled.
    The confidences lie in [-0.25, 1.5]: ``abs(c - 0.5) <= 1``, so the terms of the sums are bounded by 1 as the tolerance assumes."""
    if "odd_eval" not in _cache:
        rng = np.random.default_rng(20240704)
        edges = [f(F32(t)) for t in THRESHOLDS for f in (lambda e: np.nextafter(e, F32(0)), lambda e: e, lambda e: np.nextafter(e, F32(1)))]
        confs = np.array(edges + [-0.25, -1e-3, 0.0, 1.0, 1.0000001, 1.5], F32)
        pairs = [(l, p) for l in ODD_LABELS for p in ODD_PREDICTIONS]
        cells = 5 * len(pairs) + 1
        idx = np.arange(cells)
        labels = np.array([pairs[i % len(pairs)][0] for i in idx], np.int32)
        pred = np.array([pairs[i % len(pairs)][1] for i in idx], F32)
        conf = confs[idx % confs.size]
        perm = rng.permutation(cells)
        _cache["odd_eval"] = _frozen(labels[perm], pred[perm], conf[perm])
    return _cache["odd_eval"]
