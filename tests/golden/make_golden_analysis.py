#!/usr/bin/env python3
"""Golden vectors for the noise pattern analysis, produced by the REFERENCE's own
``scripts/analyze_noise_patterns.py::analyze_ground_truth`` and ``print_analysis``:

    BGNN_REFERENCE=<reference checkout> python tests/golden/make_golden_analysis.py

The script is loaded through _reference_scripts.py; its ``gdal.Open`` is replaced here by a stand-in that serves four arrays as
bands 1-4 (labels as the float32 band the reference's writer produces).  ``analysis/<case>.npz`` holds the four planes (``labels``
int32, ``difference``, ``noisy_depth``, ``clean_depth`` float32), ``analysis/<case>.json`` the dictionary the reference returned
(key order kept, NaN written as JSON's ``NaN``) and the text it printed.  Every assert looks at the reference's output alone.
"""
import contextlib
import io
import json
import os
import sys
import warnings
from pathlib import Path

sys.dont_write_bytecode = True
import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from _reference_scripts import load_reference_script, save_npz  # noqa: E402

ref, _ = load_reference_script("analyze_noise_patterns")
OUT = os.path.join(HERE, "analysis")
F32 = np.float32
NODATA = 1.0e6


class _Band:
    def __init__(self, array):
        self.array = array

    def ReadAsArray(self):
        return np.array(self.array, copy=True)


class _Dataset:
    def __init__(self, bands):
        self.bands = bands

    def GetRasterBand(self, i):
        return _Band(self.bands[i - 1])


def run(name, labels, difference, noisy, clean):
    labels = np.ascontiguousarray(labels, np.int32)
    planes = {"labels": labels, "difference": np.ascontiguousarray(difference, F32), "noisy_depth": np.ascontiguousarray(noisy, F32),
              "clean_depth": np.ascontiguousarray(clean, F32)}
    assert all(p.shape == labels.shape for p in planes.values()) and labels.ndim == 2 and labels.size <= 256 * 256
    assert np.isfinite(planes["difference"][labels == 2]).all(), "a noise cell's difference is finite"
    bands = [labels.astype(F32), planes["difference"], planes["noisy_depth"], planes["clean_depth"]]
    ref.gdal.Open = lambda _path: _Dataset(bands)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")                      # nanstd of an all-NaN window, the mean of an empty column quarter
        a = ref.analyze_ground_truth(Path(name + ".tif"))
        text = io.StringIO()
        with contextlib.redirect_stdout(text):
            ref.print_analysis(a)
    size = save_npz(os.path.join(OUT, name + ".npz"), planes)
    assert size <= 700 * 1024, (name, size)
    with open(os.path.join(OUT, name + ".json"), "w") as f:
        json.dump({"analysis": a, "report": text.getvalue()}, f, indent=1)
        f.write("\n")
    c = a.get("clustering", {})
    print(f"{name:24s} {labels.shape[0]:3d} x {labels.shape[1]:3d}  noise = {int((labels == 2).sum()):5d}  clusters = {c.get('num_clusters', 0):5d}  {size} bytes")
    return a


def planes_for(rng, labels, depth=-30.0, magnitude=None):
    """Planes around a label plane: a gently sloping clean depth with ripples, a noisy depth, and a difference that is small on
    the seafloor, +-(0.2 + exponential) on noise cells (``magnitude``: those magnitudes instead) and NaN on invalid cells."""
    h, w = labels.shape
    rr, cc = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    clean = (depth + 0.02 * rr + 0.01 * cc + 0.05 * rng.standard_normal((h, w))).astype(F32)
    noise = labels == 2
    if magnitude is None:
        magnitude = 0.2 + rng.exponential(0.3, int(noise.sum()))
    difference = (0.05 * rng.standard_normal((h, w))).astype(F32)
    difference[noise] = (np.asarray(magnitude) * rng.choice([-1.0, 1.0], int(noise.sum()), p=[0.35, 0.65])).astype(F32)
    difference[labels < 0] = np.nan
    noisy = (clean + np.nan_to_num(difference)).astype(F32)
    return difference, noisy, clean


def main():
    os.makedirs(OUT, exist_ok=True)
    rng = np.random.default_rng(20240815)

    # ragged size; scattered noise and a stripe; a nodata block in clean, a NaN block in noisy; three populated depth bins
    h, w = 97, 203
    labels = np.where(rng.random((h, w)) < 0.08, 2, 0)
    labels[rng.random((h, w)) < 0.04] = -1
    labels[20:60, 100:104] = 2
    difference, noisy, clean = planes_for(rng, labels)
    for c0, c1, d in ((0, 68, -5.0), (68, 136, -15.0), (136, 203, -35.0)):
        noisy[:, c0:c1] = (d + 0.5 * rng.standard_normal((h, c1 - c0))).astype(F32)
    clean[70:80, 10:30] = NODATA
    labels[72:78, 12:28] = -1                                 # (the rim of the block keeps valid cells: their windows see 1e6)
    noisy[40:50, 150:170] = np.nan
    labels[40:50, 150:170] = -1
    difference[labels < 0] = np.nan
    a = run("mixed_97x203", labels, difference, noisy, clean)
    assert list(a["depth_dependent"]) == ["0-10m", "10-20m", "20-50m"] and a["clustering"]["max_cluster_size"] >= 160
    assert a["roughness_context"]["seafloor_mean_roughness"] > 100 and list(a) == [
        "file", "shape", "magnitude", "sign", "depth_dependent", "clustering", "swath_pattern", "roughness_context"]

    # one 4-connected snake through every tile: full even rows, joined alternately at the right and the left end
    labels = np.zeros((128, 128), np.int64)
    labels[0::2, :] = 2
    labels[1::4, 127] = 2
    labels[3::4, 0] = 2
    a = run("serpentine_128", labels, *planes_for(rng, labels))
    assert a["clustering"]["num_clusters"] == 1 and a["clustering"]["max_cluster_size"] == int((labels == 2).sum()) == 64 * 128 + 64

    # comb teeth that join only in the last row
    labels = np.zeros((130, 67), np.int64)
    labels[:, 0::2] = 2
    labels[129, :] = 2
    a = run("comb_130x67", labels, *planes_for(rng, labels))
    assert a["clustering"]["num_clusters"] == 1 and a["clustering"]["size_distribution"]["1000-10000"] == 1

    # diagonal contact only: 4-connectivity makes every noise cell its own cluster
    rr, cc = np.meshgrid(np.arange(64), np.arange(64), indexing="ij")
    labels = np.where((rr + cc) % 2 == 0, 2, 0)
    a = run("checkerboard_64", labels, *planes_for(rng, labels))
    assert a["clustering"]["num_clusters"] == 2048 and a["clustering"]["isolated_noise_ratio"] == 1.0 and a["clustering"]["median_cluster_size"] == 1.0

    # a single cluster of 16384 cells: in no size bin
    labels = np.full((128, 128), 2)
    a = run("all_noise_128", labels, *planes_for(rng, labels))
    assert a["clustering"]["num_clusters"] == 1 and a["clustering"]["max_cluster_size"] == 16384
    assert sum(a["clustering"]["size_distribution"].values()) == 0 and np.isnan(a["roughness_context"]["seafloor_mean_roughness"])

    # two clusters of 3 and 4 cells: the median size is 3.5
    labels = np.zeros((16, 16), np.int64)
    labels[2, 3:6] = 2
    labels[9:11, 8:10] = 2
    a = run("two_clusters_even", labels, *planes_for(rng, labels))
    assert a["clustering"]["num_clusters"] == 2 and a["clustering"]["median_cluster_size"] == 3.5 and a["clustering"]["mean_cluster_size"] == 3.5

    # no noise cell: file and shape only
    labels = np.where(rng.random((20, 30)) < 0.1, -1, 0)
    a = run("no_noise", labels, *planes_for(rng, labels))
    assert list(a) == ["file", "shape"] and a["shape"] == [20, 30]

    # noise and invalid cells only
    labels = np.where(rng.random((40, 40)) < 0.3, 2, -1)
    a = run("no_seafloor", labels, *planes_for(rng, labels))
    assert np.isnan(a["roughness_context"]["seafloor_mean_roughness"]) and np.isnan(a["roughness_context"]["seafloor_median_roughness"])
    assert not np.isnan(a["roughness_context"]["noise_median_roughness"])

    # exactly 100 noise cells in 0-10 m (absent), 101 in 10-20 m (present), 50 in 20-50 m; depths exactly on 10.0 and 20.0
    labels = np.zeros((32, 32), np.int64)
    labels.reshape(-1)[rng.choice(320, 100, replace=False)] = 2
    labels.reshape(-1)[320 + rng.choice(320, 101, replace=False)] = 2
    labels.reshape(-1)[640 + rng.choice(384, 50, replace=False)] = 2
    difference, noisy, clean = planes_for(rng, labels)
    noisy[0:10, :] = (-5.0 + rng.random((10, 32))).astype(F32)
    noisy[10:20, :] = (-15.0 + rng.random((10, 32))).astype(F32)
    noisy[10:20, 0:16] = -10.0
    noisy[20:32, :] = -20.0
    a = run("bin_edges", labels, difference, noisy, clean)
    assert list(a["depth_dependent"]) == ["10-20m"] and a["depth_dependent"]["10-20m"]["count"] == 101
    assert int(((labels == 2) & (noisy == F32(-10.0))).sum()) > 10 and a["depth_dependent"]["10-20m"]["noise_rate"] == 101 / 320

    # +-inf and NaN in clean beside valid cells
    labels = np.where(rng.random((24, 24)) < 0.25, 2, 0)
    difference, noisy, clean = planes_for(rng, labels)
    clean[3, 3], clean[10, 12], clean[10, 13], clean[20, 5] = np.inf, -np.inf, np.inf, np.nan
    clean[15:18, 15:18] = np.nan
    a = run("inf_neighbour", labels, difference, noisy, clean)
    assert all(np.isfinite(v) for v in a["roughness_context"].values())

    # degenerate shapes
    labels = np.where(rng.random((1, 300)) < 0.4, 2, 0)
    a = run("one_row_1x300", labels, *planes_for(rng, labels))
    assert a["clustering"]["num_clusters"] > 20
    labels = np.where(rng.random((300, 1)) < 0.4, 2, 0)
    a = run("one_col_300x1", labels, *planes_for(rng, labels))
    assert np.isnan(a["swath_pattern"]["right_quarter_noise_rate"]) and a["clustering"]["num_clusters"] > 20
    labels = np.full((1, 1), 2)
    a = run("one_cell", labels, *planes_for(rng, labels))
    assert a["clustering"]["num_clusters"] == 1 and a["magnitude"]["median"] == a["magnitude"]["max"] == a["magnitude"]["p99"]

    # noise counts for which (n - 1) * 0.9 and (n - 1) * 0.99 are integral (101, 1001) and one for which they are not (157)
    for n in (101, 1001, 157):
        labels = np.zeros((40, 40), np.int64)
        labels.reshape(-1)[rng.choice(1600, n, replace=False)] = 2
        a = run(f"percentile_ranks_{n}", labels, *planes_for(rng, labels))
        assert a["magnitude"]["median"] < a["magnitude"]["p90"] < a["magnitude"]["p99"] < a["magnitude"]["max"]

    # many equal magnitudes around the selected ranks: 1000 noise cells, runs of equal values across the median, p90 and p99
    labels = np.zeros((40, 40), np.int64)
    labels.reshape(-1)[rng.choice(1600, 1000, replace=False)] = 2
    mags = np.concatenate([rng.uniform(0.2, 0.3, 400), np.full(200, 0.5), rng.uniform(0.6, 0.7, 250), np.full(100, 0.75),
                           rng.uniform(0.8, 0.9, 30), np.full(15, 1.25), rng.uniform(1.3, 1.4, 5)])
    a = run("ties", labels, *planes_for(rng, labels, magnitude=rng.permutation(mags)))
    assert a["magnitude"]["median"] == 0.5 and a["magnitude"]["p90"] == 0.75 and a["magnitude"]["p99"] == 1.25


if __name__ == "__main__":
    main()
