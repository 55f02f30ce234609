"""Shared by the noise pattern analysis tests (host and GPU): the fixtures under tests/golden/analysis, a numpy / scipy restatement
of the reference's ``analyze_ground_truth`` that returns the result block of include/bgnn_analysis.h plus the two column arrays
(``numpy_analysis_block``), and the comparison of an analysis dictionary with the reference's (``check_analysis``).

The restatement follows the definitions in the header: counts and the label statistics with ``ndimage.label`` (default
structure: 4-connectivity), the order statistics by a full sort, float sums in float64, and the roughness vectorised -- the 25
shifted copies of the NaN-padded float64 clean depth with ``np.nanstd`` over the stack, which is what ``generic_filter`` with
``mode='constant', cval=nan`` hands its callback window by window.

Comparison rules.  ``==`` with the same type: shape, every count, ratios of counts, the whole clustering part, the swath rates,
the maximum, the median.  p90 / p99 equal the reference's float32 value; one float32 ulp is allowed where the interpolation's
rounding may differ, none for the ``percentile_ranks_*`` and ``ties`` cases.  Means and the standard deviation of float32 data:
the reference sums in float32, so the yardstick is the float64 value formed here from the fixture's planes, within
``_eval_checks.sum_tolerance(n)`` relative; the reference's own number is held to its float32 distance from that value
(``F32_SUM``: numpy's pairwise float32 sum carries at most (24 + log2 n) * 2^-24 relative -- blocks of 128 terms in 8 accumulators,
then a tree -- on terms of one sign; the float32 standard deviation inherits that relative to std + mean, the mean's error entering
through the deviations).  Roughness means and medians: relative 1e-9 (fewer than 2^18 cells: a float64 sum in any order is within
n * 2^-53 < 3e-11, the window statistic adds a few 25 * 2^-53, one decade of margin; an order statistic moves by no more than the
largest change of an element), NaN must match NaN."""
import glob
import json
import math
import os
import warnings

import numpy as np
from scipy import ndimage

from _eval_checks import GOLDEN, sum_tolerance

F32 = np.float32
ANALYSIS_CASES = sorted(os.path.basename(p)[:-4] for p in glob.glob(os.path.join(GOLDEN, "analysis", "*.npz")))
STRICT_CASES = tuple(n for n in ANALYSIS_CASES if n.startswith(("percentile_ranks", "ties")))
PLANES = ("labels", "difference", "noisy_depth", "clean_depth")
ROUGH_RTOL = 1e-9
_cache = {}


def load_analysis_case(name):
    """``(planes, analysis, report)`` of ``golden/analysis/<name>``: the four planes in PLANES order (read-only), the reference's
    dictionary and the text its ``print_analysis`` wrote (loaded once)."""
    if name not in _cache:
        z = np.load(os.path.join(GOLDEN, "analysis", name + ".npz"), allow_pickle=False)
        planes = tuple(z[k] for k in PLANES)
        for a in planes:
            a.setflags(write=False)
        j = json.load(open(os.path.join(GOLDEN, "analysis", name + ".json")))
        _cache[name] = (planes, j["analysis"], j["report"])
    return _cache[name]


def roughness(clean):
    """``ndimage.generic_filter(clean.astype(float64), nanstd, size=5, mode='constant', cval=nan)``, vectorised."""
    h, w = clean.shape
    padded = np.full((h + 4, w + 4), np.nan)
    padded[2:-2, 2:-2] = clean.astype(np.float64)
    stack = np.stack([padded[a:a + h, b:b + w] for a in range(5) for b in range(5)])
    with warnings.catch_warnings(), np.errstate(invalid="ignore"):
        warnings.simplefilter("ignore", RuntimeWarning)
        return np.nanstd(stack, axis=0)


def cluster_sizes(noise_mask):
    labeled, k = ndimage.label(noise_mask)
    return np.bincount(labeled.reshape(-1), minlength=k + 1)[1:].astype(np.int64)


def numpy_analysis_block(labels, difference, noisy, clean, with_roughness=True):
    """``(block, col_noise, col_valid)`` by the definitions of include/bgnn_analysis.h (``block``: a record of runtime.NA_DTYPE).
    ``with_roughness=False`` leaves the three roughness entries zero (the 25-plane stack is the costly part on a large grid)."""
    from bathymetric_gnn_amd import runtime
    from bathymetric_gnn_amd.data.noise_analysis import magnitude_ranks
    labels = np.asarray(labels).astype(np.int32)
    b = np.zeros((), np.dtype(runtime.NA_DTYPE))
    valid, noise, sea = labels >= 0, labels == 2, labels == 0
    d = difference[noise]
    fin = np.isfinite(d)
    b["valid"], b["noise"], b["seafloor"] = int(valid.sum()), int(noise.sum()), int(sea.sum())
    b["nonfinite"] = int((~fin).sum())
    d64 = d[fin].astype(np.float64)
    mag = np.abs(d[fin])
    mag64 = mag.astype(np.float64)
    b["positive"], b["negative"] = int((d64 > 0).sum()), int((d64 < 0).sum())
    with np.errstate(invalid="ignore"):
        x = -noisy
        for i in range(8):
            inb = (x >= F32(runtime.NA_DEPTH_EDGES[i])) & (x < F32(runtime.NA_DEPTH_EDGES[i + 1]))
            b["bin_noise"][i], b["bin_valid"][i] = int((inb & noise).sum()), int((inb & valid).sum())
            sel = difference[inb & noise]
            b["bin_abs_sum"][i] = np.abs(sel[np.isfinite(sel)]).astype(np.float64).sum()
    n = mag.size
    b["abs_sum"], b["sq_sum"] = mag64.sum(), (d64 * d64).sum()
    b["dev_sq_sum"] = ((mag64 - mag64.sum() / n) ** 2).sum() if n else 0.0
    b["pos_sum"], b["neg_sum"] = d64[d64 > 0].sum(), d64[d64 < 0].sum()
    b["abs_max"] = mag.max() if n else 0.0
    if n:
        ranks, _, _ = magnitude_ranks(n)
        b["mag_rank"], b["mag_value"] = ranks, np.sort(mag)[ranks]
    else:
        b["mag_rank"], b["mag_value"] = -1, np.nan
    sizes = np.sort(cluster_sizes(noise))
    k = sizes.size
    b["num_clusters"], b["cluster_cells"] = k, int(sizes.sum())
    b["max_cluster"], b["isolated"] = (int(sizes[-1]) if k else 0), int((sizes == 1).sum())
    for i in range(7):
        b["size_bins"][i] = int(((sizes >= runtime.NA_SIZE_EDGES[i]) & (sizes < runtime.NA_SIZE_EDGES[i + 1])).sum())
    b["size_mid"] = [sizes[(k - 1) // 2], sizes[k // 2]] if k else 0
    rough = roughness(clean) if with_roughness else None
    for j, cls in enumerate((noise, sea) if with_roughness else ()):
        r = np.sort(rough[cls][~np.isnan(rough[cls])])
        m = r.size
        b["rough_count"][j], b["rough_sum"][j] = m, r.sum()
        b["rough_mid"][2 * j:2 * j + 2] = [r[(m - 1) // 2], r[m // 2]] if m else np.nan
    return b, noise.sum(axis=0).astype(np.int32), valid.sum(axis=0).astype(np.int32)


def numpy_analysis(labels, difference, noisy, clean, file="None"):
    """The reference's dictionary from the restatement, assembled by the package's own host code."""
    from bathymetric_gnn_amd.data.noise_analysis import analysis_from_block
    block, col_noise, col_valid = numpy_analysis_block(labels, difference, noisy, clean)
    return analysis_from_block(block, col_noise, col_valid, np.asarray(labels).shape, file)


# the ground truth's constructed keys (_eval_checks.adversarial_case) whose magnitudes the six-rank selection is held to
MAGNITUDE_KEY_CASES = ("uniform_keys_4098", "uniform_keys_4099", "straddle_level1", "straddle_level2", "first_bin_owner",
                       "last_bin_owner", "denormals")


def magnitude_key_case(name):
    """``(planes, block, col_noise, col_valid)``: a 1 x n grid whose ``difference`` is ``|values|`` of
    ``adversarial_case(name)``, every label 2, both depths 0, and the restatement's result (built once; read-only)."""
    if ("keys", name) not in _cache:
        from _eval_checks import adversarial_case
        difference = np.abs(adversarial_case(name).values).reshape(1, -1)
        assert difference.dtype == F32 and np.isfinite(difference).all()
        zero = np.zeros_like(difference)
        planes = (np.full(difference.shape, 2, np.int32), difference, zero, zero)
        for a in planes:
            a.setflags(write=False)
        _cache[("keys", name)] = (planes,) + numpy_analysis_block(*planes)
    return _cache[("keys", name)]


def ulps_apart(a, b):
    """The distance of two float32 values of one sign in units of the last place."""
    return abs(int(F32(a).view(np.int32)) - int(F32(b).view(np.int32)))


def _same(a, b):
    """Equal values of equal type (NaN equals NaN)."""
    if isinstance(a, float) and isinstance(b, float) and math.isnan(a) and math.isnan(b):
        return True
    return a == b and type(a) is type(b)


def f32_sum_bound(n):
    return (24 + math.log2(max(n, 1))) * 2.0 ** -24


def _check_mean(key, got, want, terms, fixture):
    """``terms``: the float32 values the reference averaged; of one sign."""
    n = terms.size
    if n == 0:
        assert _same(got, want) and got == 0, key               # the reference's integer 0
        return
    exact = terms.astype(np.float64).sum() / n
    err = abs(got - exact)
    print(f"{key}: {got!r} against {exact!r} (reference {want!r}), error {err:.3e}, bound {sum_tolerance(n) * abs(exact):.3e}")
    assert type(got) is float and err <= sum_tolerance(n) * abs(exact), (key, got, exact)
    if fixture:
        assert abs(want - exact) <= f32_sum_bound(n) * abs(exact), (key, want, exact)


def check_analysis(got, want, planes, strict=False, fixture=True):
    """``got``: the dictionary under test; ``want``: the reference's JSON for the same planes (``fixture=False``: the restatement's
    dictionary instead, whose float sums are float64 already); ``planes``: (labels, difference, noisy_depth, clean_depth)."""
    labels, difference, noisy, _ = planes
    labels = np.asarray(labels).astype(np.int32)
    assert list(got) == list(want)
    assert _same(got["file"], want["file"]) and _same(got["shape"], want["shape"]) and all(type(v) is int for v in got["shape"])
    if "magnitude" not in want:
        return
    noise = labels == 2
    d = difference[noise]
    mag = np.abs(d)
    n = mag.size

    gm, wm = got["magnitude"], want["magnitude"]
    assert list(gm) == list(wm) and all(type(v) is float for v in gm.values())
    assert gm["max"] == wm["max"] and gm["median"] == wm["median"], (gm, wm)
    for k in ("p90", "p99"):
        ulps = abs(int(F32(gm[k]).view(np.int32)) - int(F32(wm[k]).view(np.int32)))
        assert float(F32(gm[k])) == gm[k] and ulps <= (0 if strict else 1), (k, gm[k], wm[k])
    _check_mean("magnitude.mean", gm["mean"], wm["mean"], mag, fixture)
    mag64 = mag.astype(np.float64)
    exact_mean = mag64.sum() / n
    exact_std = math.sqrt(((mag64 - exact_mean) ** 2).sum() / n)
    err = abs(gm["std"] - exact_std)
    print(f"magnitude.std: {gm['std']!r} against {exact_std!r} (reference {wm['std']!r}), error {err:.3e}, bound {sum_tolerance(n) * exact_std:.3e}")
    assert err <= sum_tolerance(n) * exact_std, (gm["std"], exact_std)
    if fixture:
        assert abs(wm["std"] - exact_std) <= f32_sum_bound(n) * (exact_std + exact_mean), (wm["std"], exact_std)

    gs, ws = got["sign"], want["sign"]
    assert list(gs) == list(ws)
    assert _same(gs["positive_ratio"], ws["positive_ratio"]) and _same(gs["negative_ratio"], ws["negative_ratio"]), (gs, ws)
    _check_mean("sign.mean_positive", gs["mean_positive"], ws["mean_positive"], d[d > 0], fixture)
    _check_mean("sign.mean_negative", gs["mean_negative"], ws["mean_negative"], d[d < 0], fixture)

    gd, wd = got["depth_dependent"], want["depth_dependent"]
    assert list(gd) == list(wd)
    for key in wd:
        assert list(gd[key]) == list(wd[key]) and _same(gd[key]["count"], wd[key]["count"]), key
        assert _same(gd[key]["noise_rate"], wd[key]["noise_rate"]), (key, gd[key], wd[key])
        lo, hi = (F32(v) for v in key[:-1].split("-"))
        with np.errstate(invalid="ignore"):
            inb = (-noisy >= lo) & (-noisy < hi) & noise
        _check_mean(f"depth_dependent.{key}.mean_magnitude", gd[key]["mean_magnitude"], wd[key]["mean_magnitude"], np.abs(difference[inb]), fixture)

    assert ("clustering" in got) == ("clustering" in want)
    if "clustering" in want:
        gc, wc = got["clustering"], want["clustering"]
        assert list(gc) == list(wc)
        for k, v in wc.items():
            if k == "size_distribution":
                assert list(gc[k]) == list(v) and all(_same(gc[k][b], v[b]) for b in v), (gc[k], v)
            else:
                assert _same(gc[k], v), (k, gc[k], v)

    assert list(got["swath_pattern"]) == list(want["swath_pattern"])
    for k, v in want["swath_pattern"].items():
        assert _same(got["swath_pattern"][k], v), (k, got["swath_pattern"][k], v)

    gr, wr = got["roughness_context"], want["roughness_context"]
    assert list(gr) == list(wr)
    for k, v in wr.items():
        assert type(gr[k]) is float, k
        if math.isnan(v):
            assert math.isnan(gr[k]), (k, gr[k])
        else:
            print(f"roughness_context.{k}: {gr[k]!r} against {v!r}, relative error {abs(gr[k] - v) / max(abs(v), 1e-300):.3e}")
            assert abs(gr[k] - v) <= ROUGH_RTOL * abs(v), (k, gr[k], v)
