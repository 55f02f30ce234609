"""Noise pattern analysis of a ground truth: the reference's ``scripts/analyze_noise_patterns.py`` with the planes in HBM.

``analyze_noise_patterns`` runs everything per cell -- counts, depth bins, float64 sums, the order statistics of ``|difference|``,
the 4-connected clusters of the noise mask with their sizes, the per-column counts and the 5 x 5 roughness of the clean depth with
its class means and medians -- as ``bgnn_noise_analysis`` (include/bgnn_analysis.h): radix selections and a union-find labelling
on the device, no sort, no Python callback per cell, and one read of a 528-byte result block plus two ``[cols]`` count arrays.
``analysis_from_block`` is the host half: the reference's dictionary from that block, with numpy's own median / percentile rules.
``print_analysis`` writes the reference's report.  Reading the GeoTIFF (GDAL) stays with the reference."""
from __future__ import annotations

import ctypes as C
import math
import warnings
from pathlib import Path
from typing import Any, Dict, Tuple

import numpy as np
import torch

from .. import runtime as rt

F32 = np.float32
_SWATH_KEYS = ("left_quarter_noise_rate", "center_left_noise_rate", "center_right_noise_rate", "right_quarter_noise_rate")


def percentile_ranks(n: int, p: float) -> Tuple[int, int, np.float32]:
    """The two ranks ``np.percentile(a, p)`` reads on a float32 array of ``n`` values and its interpolation weight: numpy forms
    the virtual index in the array's dtype, ``(n - 1) * q`` with ``q = p / float32(100)``."""
    q = F32(p) / F32(100)
    v = F32(F32(n - 1) * q)
    f = np.floor(v)
    lo, hi = int(f), int(F32(f + F32(1)))
    gamma = F32(v - f)
    if v >= F32(n - 1):
        lo = hi = n - 1
    if v < 0:
        lo = hi = 0
    return lo, hi, gamma


def _lerp(a: np.float32, b: np.float32, t: np.float32) -> np.float32:
    """numpy's ``_lerp`` on float32 scalars: ``a + (b - a) * t``, and ``b - (b - a) * (1 - t)`` from ``t >= 0.5``."""
    diff = F32(b - a)
    if t >= 0.5:
        return F32(b - F32(diff * F32(F32(1) - t)))
    return F32(a + F32(diff * t))


def magnitude_ranks(n: int):
    """The six ranks of the result block's ``mag_rank`` for ``n`` noise cells, and the two percentile weights."""
    l90, h90, g90 = percentile_ranks(n, 90)
    l99, h99, g99 = percentile_ranks(n, 99)
    return [(n - 1) // 2, n // 2, l90, h90, l99, h99], g90, g99


def analysis_from_block(block, col_noise, col_valid, shape, file="None") -> Dict[str, Any]:
    """The reference's ``analyze_ground_truth`` dictionary from a result block on the host (a record of ``runtime.NA_DTYPE``)
    and the per-column noise / valid counts.  Counts, ratios of counts, the clustering part, the swath rates, the maximum and
    the selected order statistics are the reference's own values; the means and the standard deviation are float64 sums over
    the count where the reference sums in float32.  Raises ``ValueError`` when a noise cell's difference is not finite."""
    analysis: Dict[str, Any] = {"file": str(file), "shape": [int(v) for v in shape]}
    n = int(block["noise"])
    if n == 0:
        return analysis
    if int(block["nonfinite"]) > 0:
        raise ValueError(f"{int(block['nonfinite'])} noise cells have a difference that is not finite")

    ranks, g90, g99 = magnitude_ranks(n)
    if ranks != [int(v) for v in block["mag_rank"]]:
        raise rt.BgnnError(f"the device selected ranks {[int(v) for v in block['mag_rank']]} of {n} values, numpy reads {ranks}")
    v = [F32(x) for x in block["mag_value"]]
    analysis["magnitude"] = {
        "mean": float(block["abs_sum"]) / n,
        "std": math.sqrt(float(block["dev_sq_sum"]) / n),
        "median": float(v[0] if n % 2 else F32(v[0] + v[1]) / F32(2)),
        "p90": float(_lerp(v[2], v[3], g90)),
        "p99": float(_lerp(v[4], v[5], g99)),
        "max": float(block["abs_max"]),
    }

    pos, neg = int(block["positive"]), int(block["negative"])
    analysis["sign"] = {
        "positive_ratio": pos / n,
        "negative_ratio": neg / n,
        "mean_positive": float(block["pos_sum"]) / pos if pos > 0 else 0,
        "mean_negative": float(block["neg_sum"]) / neg if neg > 0 else 0,
    }

    depth_noise = {}
    for i in range(len(rt.NA_DEPTH_EDGES) - 1):
        count, total = int(block["bin_noise"][i]), int(block["bin_valid"][i])
        if count > 100 and total > 0:
            depth_noise[f"{rt.NA_DEPTH_EDGES[i]}-{rt.NA_DEPTH_EDGES[i + 1]}m"] = {
                "count": count,
                "mean_magnitude": float(block["bin_abs_sum"][i]) / count,
                "noise_rate": count / total,
            }
    analysis["depth_dependent"] = depth_noise

    k = int(block["num_clusters"])
    if k > 0:
        lo, hi = (int(s) for s in block["size_mid"])
        analysis["clustering"] = {
            "num_clusters": k,
            "mean_cluster_size": int(block["cluster_cells"]) / k,
            "median_cluster_size": float(lo) if k % 2 else (float(lo) + float(hi)) / 2,
            "max_cluster_size": int(block["max_cluster"]),
            "isolated_noise_ratio": int(block["isolated"]) / k,
            "size_distribution": {f"{rt.NA_SIZE_EDGES[i]}-{rt.NA_SIZE_EDGES[i + 1]}": int(block["size_bins"][i])
                                  for i in range(len(rt.NA_SIZE_EDGES) - 1)},
        }

    # numpy itself on the integer counts: the four rates are the reference's bits
    valid_by_col = np.maximum(np.asarray(col_valid, np.int64), 1)
    noise_by_col = np.asarray(col_noise, np.int64) / valid_by_col
    quarters = np.array_split(noise_by_col, 4)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)       # (fewer than four columns: the mean of an empty quarter is NaN)
        analysis["swath_pattern"] = {key: float(np.mean(q)) for key, q in zip(_SWATH_KEYS, quarters)}

    def mean_median(j):
        m = int(block["rough_count"][j])
        if m == 0:
            return math.nan, math.nan
        a, b = float(block["rough_mid"][2 * j]), float(block["rough_mid"][2 * j + 1])
        return float(block["rough_sum"][j]) / m, (a if m % 2 else (a + b) / 2)
    noise_mean, noise_median = mean_median(0)
    sea_mean, sea_median = mean_median(1)
    analysis["roughness_context"] = {
        "noise_mean_roughness": noise_mean,
        "noise_median_roughness": noise_median,
        "seafloor_mean_roughness": sea_mean,
        "seafloor_median_roughness": sea_median,
    }
    return analysis


def split_result(host: np.ndarray, cols: int):
    """``(block, col_noise, col_valid)`` from the host copy of what ``noise_analysis_build`` returned."""
    words = rt.NA_BYTES // 4
    block = np.frombuffer(host[:words].tobytes(), dtype=np.dtype(rt.NA_DTYPE))[0]
    return block, host[words:words + cols], host[words + cols:words + 2 * cols]


def noise_analysis_build(labels: torch.Tensor, difference: torch.Tensor, noisy_depth: torch.Tensor, clean_depth: torch.Tensor,
                         ctx=None) -> torch.Tensor:
    """``bgnn_noise_analysis`` on device planes of one ``[rows, cols]`` shape (``labels`` int32, the rest float32, contiguous):
    an int32 device tensor holding the result block, then ``col_noise [cols]``, then ``col_valid [cols]`` (``split_result``).
    Asynchronous on the context's stream, ordered against the caller's current stream."""
    dev = labels.device
    ctx = ctx if ctx is not None else rt.get_context(dev)
    for name, t, dtype in (("labels", labels, torch.int32), ("difference", difference, torch.float32),
                           ("noisy_depth", noisy_depth, torch.float32), ("clean_depth", clean_depth, torch.float32)):
        if t.dtype != dtype or t.device != dev or not t.is_contiguous():
            raise TypeError(f"{name} must be a contiguous {dtype} tensor on {dev}")
        if t.dim() != 2 or t.shape != labels.shape:
            raise ValueError(f"{name} has shape {tuple(t.shape)}, labels {tuple(labels.shape)}")
    rows, cols = (int(v) for v in labels.shape)
    if rows < 1 or cols < 1:
        raise ValueError(f"a grid of {rows} x {cols}")
    if rows * cols > rt.NA_MAX_CELLS:
        raise NotImplementedError(f"{rows} x {cols} cells exceed the limit of {rt.NA_MAX_CELLS} (int32 cluster labels)")
    ws_bytes = int(ctx.lib.bgnn_noise_analysis_workspace_bytes(rows, cols))
    ws = torch.empty((ws_bytes + 7) // 8, dtype=torch.int64, device=dev)
    words = rt.NA_BYTES // 4
    out = torch.empty(words + 2 * cols, dtype=torch.int32, device=dev)
    base = out.data_ptr()
    ctx.begin()
    rt.check(ctx.lib.bgnn_noise_analysis(ctx.handle, rt.ptr(labels), rt.ptr(difference), rt.ptr(noisy_depth), rt.ptr(clean_depth),
                                         rows, cols, rt.ptr(ws), C.c_size_t(ws.numel() * 8), C.c_void_p(base),
                                         C.c_void_p(base + 4 * words), C.c_void_p(base + 4 * (words + cols))))
    ctx.end()
    return out


def _to_device(plane, device, labels=False) -> torch.Tensor:
    if isinstance(plane, torch.Tensor):
        t = plane.to(device)
        return t.to(torch.int32 if labels else torch.float32).contiguous()
    # (a copy: the caller's array may be read-only; labels as the reference reads the band, ``astype(int32)``)
    return torch.from_numpy(np.array(plane, dtype=np.int32 if labels else np.float32, order="C")).to(device)


def analyze_noise_patterns(gt, file="None", device=None) -> Dict[str, Any]:
    """The reference's ``analyze_ground_truth`` (analyze_noise_patterns.py) of a ``GroundTruth`` or of the four planes ``(labels,
    difference, noisy_depth, clean_depth)``: device tensors or host arrays, ``labels`` int32 or the float32 band the reference's
    writer produces (read as the reference reads it, ``astype(int32)``).  Everything per cell runs on the device; nothing
    synchronises until the one read of the result."""
    planes = (gt.labels, gt.difference, gt.noisy_depth, gt.clean_depth) if hasattr(gt, "noisy_depth") else tuple(gt)
    if len(planes) != 4:
        raise ValueError("four planes expected: labels, difference, noisy_depth, clean_depth")
    if device is None and isinstance(planes[0], torch.Tensor) and planes[0].is_cuda:
        device = planes[0].device
    device = rt.resolve_device(device)
    shape = tuple(int(v) for v in planes[0].shape)
    if len(shape) != 2:
        raise ValueError(f"labels has shape {shape}: a [rows, cols] plane expected")
    if shape[0] * shape[1] == 0:
        return {"file": str(file), "shape": list(shape)}
    labels, difference, noisy, clean = (_to_device(p, device, labels=(i == 0)) for i, p in enumerate(planes))
    out = noise_analysis_build(labels, difference, noisy, clean)
    block, col_noise, col_valid = split_result(out.cpu().numpy(), shape[1])
    return analysis_from_block(block, col_noise, col_valid, shape, file)


def format_analysis(analysis: Dict[str, Any]) -> str:
    """The text of the reference's ``print_analysis``."""
    rule = "=" * 60
    lines = ["", rule, f"NOISE PATTERN ANALYSIS: {Path(analysis['file']).name}", rule, "",
             f"Grid shape: {analysis['shape']}"]
    if "magnitude" not in analysis:
        return "\n".join(lines + ["No noise found in this file."])
    m, s = analysis["magnitude"], analysis["sign"]
    lines += ["", "1. Noise Magnitude:",
              f"   Mean: {m['mean']:.3f}m, Std: {m['std']:.3f}m",
              f"   Median: {m['median']:.3f}m, 90th percentile: {m['p90']:.3f}m",
              f"   Max: {m['max']:.3f}m",
              "", "2. Noise Direction:",
              f"   Deepening (positive): {100 * s['positive_ratio']:.1f}% (mean: {s['mean_positive']:.3f}m)",
              f"   Shoaling (negative): {100 * s['negative_ratio']:.1f}% (mean: {s['mean_negative']:.3f}m)",
              "", "3. Depth-dependent noise rate:"]
    for depth_range, stats in analysis.get("depth_dependent", {}).items():
        lines.append(f"   {depth_range}: {100 * stats['noise_rate']:.2f}% noise rate, {stats['mean_magnitude']:.3f}m mean magnitude")
    if "clustering" in analysis:
        c = analysis["clustering"]
        lines += ["", "4. Spatial Clustering:",
                  f"   Number of clusters: {c['num_clusters']:,}",
                  f"   Mean cluster size: {c['mean_cluster_size']:.1f} cells",
                  f"   Isolated points: {100 * c['isolated_noise_ratio']:.1f}%"]
    sp, r = analysis["swath_pattern"], analysis["roughness_context"]
    lines += ["", "5. Swath Pattern (noise rate by column quartile):",
              f"   Left (outer): {100 * sp['left_quarter_noise_rate']:.2f}%",
              f"   Center-left: {100 * sp['center_left_noise_rate']:.2f}%",
              f"   Center-right: {100 * sp['center_right_noise_rate']:.2f}%",
              f"   Right (outer): {100 * sp['right_quarter_noise_rate']:.2f}%",
              "", "6. Roughness Context:",
              f"   Noise in areas with roughness: {r['noise_mean_roughness']:.4f} (mean)",
              f"   Seafloor in areas with roughness: {r['seafloor_mean_roughness']:.4f} (mean)"]
    if r["seafloor_mean_roughness"] > 0:
        lines.append(f"   Ratio: {r['noise_mean_roughness'] / r['seafloor_mean_roughness']:.2f}x (>1 means noise in rougher areas)")
    return "\n".join(lines)


def print_analysis(analysis: Dict[str, Any]) -> None:
    """The reference's report of an analysis dictionary, line for line (host formatting only)."""
    print(format_analysis(analysis))
