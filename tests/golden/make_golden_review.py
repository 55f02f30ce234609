#!/usr/bin/env python3
"""Golden vectors for the review-region export, produced by the REFERENCE's own ``scripts/export_for_review.py``:

    BGNN_REFERENCE=<reference checkout> python tests/golden/make_golden_review.py

That script exists in the reference as a fenced Python block of ``docs/TRAINING_PLAN.md`` (step 5.1).  This maker reads the one
block that names ``scripts/export_for_review.py`` at run time and executes it as a module -- no text of it is kept here -- with a
stand-in ``osgeo.gdal``: ``Open`` serves the classification and confidence arrays as bands 1 and 2, ``GetDriverByName`` hands out the
``RecordingDriver`` of _reference_scripts.py, which keeps what the script writes.  ``review/review_regions.npz`` holds, per case, the
two input planes, the parameters, the review mask the script wrote to band 1 and the region list it dumped as JSON.  (A
subdirectory, as for the analysis fixtures: every ``*.npz`` directly under tests/golden is a graph case of conftest's
``golden_names``.)  Every assert looks at the reference's output alone.
"""
import contextlib
import io
import json
import os
import re
import sys
import tempfile
import types
from pathlib import Path

sys.dont_write_bytecode = True
import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from _reference_scripts import RecordingDriver, reference_root, save_npz  # noqa: E402

OUT = os.path.join(HERE, "review")
F32 = np.float32


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

    def GetGeoTransform(self):
        return (0.0, 1.0, 0.0, 0.0, 0.0, -1.0)

    def GetProjection(self):
        return ""


def load_reference_block():
    """The reference's export script as a module, and the recording driver its ``gdal.GetDriverByName`` hands out."""
    text = open(os.path.join(reference_root(), "docs", "TRAINING_PLAN.md"), encoding="utf-8").read()
    blocks = [b for b in re.findall(r"```python\n(.*?)```", text, flags=re.S) if "scripts/export_for_review.py" in b]
    assert len(blocks) == 1, f"{len(blocks)} fenced Python blocks name scripts/export_for_review.py"
    driver = RecordingDriver()
    gdal = types.ModuleType("osgeo.gdal")
    gdal.GDT_Float32 = 6
    gdal.GetDriverByName = lambda _name: driver
    osgeo = types.ModuleType("osgeo")
    osgeo.gdal = gdal
    sys.modules.update({"osgeo": osgeo, "osgeo.gdal": gdal})
    mod = types.ModuleType("reference_export_for_review")
    exec(compile(blocks[0], "export_for_review.py", "exec"), mod.__dict__)
    return mod, driver


ref, driver = load_reference_block()


def run(arrays, name, classification, confidence, low, high, min_region_size):
    classification = np.ascontiguousarray(classification, F32)
    confidence = np.ascontiguousarray(confidence, F32)
    assert classification.shape == confidence.shape and confidence.ndim == 2
    ref.gdal.Open = lambda _path: _Dataset([classification, confidence])
    with tempfile.TemporaryDirectory() as tmp:
        out = Path(tmp) / (name + ".tif")
        with contextlib.redirect_stdout(io.StringIO()):
            ref.export_review_regions(Path(name + "_gnn_outputs.tif"), out, low, high, min_region_size)
        regions = json.load(open(out.with_suffix(".json")))
    ds = driver.datasets[-1]
    assert (ds.width, ds.height, len(ds.bands)) == (confidence.shape[1], confidence.shape[0], 3)
    assert [b.description for b in ds.bands] == ["review_mask", "confidence", "classification"]
    mask = ds.bands[0].array
    assert mask.dtype == F32 and set(np.unique(mask)) <= {0.0, 1.0} and int(mask.sum()) == sum(r["size"] for r in regions)
    assert np.array_equal(ds.bands[1].array, confidence, equal_nan=True) and np.array_equal(ds.bands[2].array, classification, equal_nan=True)
    arrays.update({name + "_classification": classification, name + "_confidence": confidence,
                   name + "_params": np.array([low, high, min_region_size], np.float64), name + "_review_mask": mask.astype(np.uint8),
                   name + "_regions": np.array(json.dumps(regions))})
    sizes = [r["size"] for r in regions]
    print(f"{name:16s} {confidence.shape[0]:3d} x {confidence.shape[1]:3d}  regions = {len(regions):3d}  sizes {min(sizes, default=0)} .. {max(sizes, default=0)}")
    return regions


def smooth_field(rng, h, w, waves=3):
    """A smooth confidence field in (0, 1): a few random plane waves through a sigmoid, rounded to multiples of 2^-12 (the
    fixture compresses to a fraction of its size)."""
    rr, cc = np.meshgrid(np.arange(h, dtype=np.float64), np.arange(w, dtype=np.float64), indexing="ij")
    z = np.zeros((h, w))
    for _ in range(waves):
        fr, fc = rng.uniform(0.01, 0.06, 2) * rng.choice([-1, 1], 2)
        z += rng.uniform(0.5, 1.5) * np.sin(2 * np.pi * (fr * rr + fc * cc) + rng.uniform(0, 2 * np.pi))
    return (np.round(4096.0 / (1.0 + np.exp(-z))) / 4096.0).astype(F32)


def main():
    os.makedirs(OUT, exist_ok=True)
    rng = np.random.default_rng(20240901)
    arrays, names = {}, []

    # the reference's defaults but for the size: a ragged smooth field with NaNs, cells exactly on both bounds (float32(0.4) and
    # float32(0.7): what the comparison with the Python floats 0.4 / 0.7 rounds to), regions on both sides of min_region_size
    h, w = 150, 333
    conf = smooth_field(rng, h, w)
    conf[rng.random((h, w)) < 0.01] = np.nan
    conf[40:44, 100:140] = F32(0.4)
    conf[90:93, 200:260] = F32(0.7)
    conf[10, 10:29] = F32(0.5); conf[9, 9:30] = 0.9; conf[11, 9:30] = 0.9; conf[10, 9] = 0.9; conf[10, 29] = 0.9      # 19 cells: dropped
    conf[20, 10:30] = F32(0.5); conf[19, 9:31] = 0.9; conf[21, 9:31] = 0.9; conf[20, 9] = 0.9; conf[20, 30] = 0.9     # 20 cells: kept
    cls = ((np.arange(h)[:, None] // 16 + np.arange(w)[None, :] // 16) % 3).astype(F32)
    cls[np.isnan(conf)] = np.nan
    regions = run(arrays, "smooth_150x333", cls, conf, 0.4, 0.7, 20)
    names.append("smooth_150x333")
    assert len(regions) >= 5 and any(r["size"] == 20 for r in regions) and not any(r["size"] == 19 for r in regions)
    assert [r["id"] for r in regions] == list(range(1, len(regions) + 1))

    # other bounds, +-inf beside NaN, a 300-cell-high ragged strip; every region of at least one cell is kept
    h, w = 301, 67
    conf = smooth_field(rng, h, w, waves=4)
    conf[rng.random((h, w)) < 0.02] = np.nan
    conf[5, 5], conf[200, 60] = np.inf, -np.inf
    regions = run(arrays, "strip_301x67", np.zeros((h, w), F32), conf, 0.25, 0.3, 1)
    names.append("strip_301x67")
    assert len(regions) >= 3 and min(r["size"] for r in regions) < 5

    # nothing to review
    regions = run(arrays, "none_40x50", np.ones((40, 50), F32), np.full((40, 50), 0.95, F32), 0.4, 0.7, 100)
    names.append("none_40x50")
    assert regions == []

    arrays["names"] = np.array(json.dumps(names))
    size = save_npz(os.path.join(OUT, "review_regions.npz"), arrays)
    assert size <= 200 * 1024, size
    print(f"review/review_regions.npz: {size} bytes")


if __name__ == "__main__":
    main()
