#!/usr/bin/env python3
"""Golden vectors for the feature labels, produced by the REFERENCE's own
``scripts/extract_s57_features.py::create_feature_labels``:

    BGNN_REFERENCE=<reference checkout> python tests/golden/make_golden_features.py

The script is loaded through _reference_scripts.py; its stand-in ``gdal`` module gets three more attributes here
(``UseExceptions``, ``OF_RASTER`` and an ``OpenEx`` that serves a depth array, a geotransform, a projection and the raster sizes).
The labels band the recording driver captures is the expected output.  ``features/<case>.npz`` holds the input ``depth`` (float32)
and the two captured bands (``labels`` as int32, ``band_depth``); ``features/<case>.json`` the geotransform, the feature list as
plain records, the radius overrides, the number the reference logged as applied and the counts taken from the captured band.
Every assert looks at the reference's output alone.  Nothing here opens a network connection: the reference's ``query_*``
functions are neither imported by name nor called.
"""
import json
import logging
import os
import re
import sys
import tempfile
from pathlib import Path

sys.dont_write_bytecode = True
import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from _reference_scripts import load_reference_script, save_npz  # noqa: E402

ref, driver = load_reference_script("extract_s57_features")
gdal = sys.modules["osgeo"].gdal
OUT = os.path.join(HERE, "features")
F32 = np.float32
NODATA = 1.0e6


class _Band:
    def __init__(self, array):
        self.array = array

    def ReadAsArray(self):
        return np.array(self.array, copy=True)


class _Survey:
    def __init__(self, depth, gt):
        self.depth, self.gt = depth, tuple(gt)
        self.RasterYSize, self.RasterXSize = depth.shape

    def GetRasterBand(self, i):
        assert i == 1
        return _Band(self.depth)

    def GetGeoTransform(self):
        return self.gt

    def GetProjection(self):
        return "LOCAL_CS[\"golden\"]"


class _Log(logging.Handler):
    def __init__(self):
        super().__init__(logging.INFO)
        self.lines = []

    def emit(self, record):
        self.lines.append(record.getMessage())


gdal.UseExceptions = lambda: None
gdal.OF_RASTER = 2
logging.disable(logging.NOTSET)                  # (the loader silences logging; the applied count is only logged)
ref.logger.handlers = []
ref.logger.propagate = False
ref.logger.setLevel(logging.INFO)
LOG = _Log()
ref.logger.addHandler(LOG)


def feat(object_class, x, y):
    return ref.S57Feature(object_class=object_class, geometry_type="Point", x=float(x), y=float(y))


def run(name, depth, gt, features, feature_radius=None):
    depth = np.ascontiguousarray(depth, F32)
    assert depth.ndim == 2 and depth.shape[0] <= 300 and depth.shape[1] <= 300 and depth.size <= 256 * 256
    gdal.OpenEx = lambda _path, _flags, open_options=None: _Survey(depth, gt)
    del driver.datasets[:]
    del LOG.lines[:]
    with tempfile.TemporaryDirectory() as tmp:
        ref.create_feature_labels(features, Path(name + ".bag"), Path(tmp) / "out" / (name + ".tif"), feature_radius)
    (ds,) = driver.datasets
    band = ds.bands[0].array
    assert band.dtype == F32 and band.shape == depth.shape and ds.bands[0].nodata == -1 and ds.geotransform == tuple(gt)
    labels = band.astype(np.int32)
    assert np.array_equal(labels.astype(F32), band)
    (applied,) = [int(m.group(1)) for m in (re.match(r"Applied (\d+) feature labels", line) for line in LOG.lines) if m]
    arrays = {"depth": depth, "labels": labels, "band_depth": np.asarray(ds.bands[1].array)}
    size = save_npz(os.path.join(OUT, name + ".npz"), arrays)
    assert size <= 700 * 1024, (name, size)
    counts = {"feature_cells": int((labels == 1).sum()), "valid_cells": int((labels >= 0).sum()), "painted_cells": int((labels > 0).sum())}
    with open(os.path.join(OUT, name + ".json"), "w") as f:
        json.dump({"shape": list(depth.shape), "geotransform": list(gt),
                   "features": [{"object_class": q.object_class, "geometry_type": q.geometry_type, "x": q.x, "y": q.y} for q in features],
                   "feature_radius": feature_radius, "applied_features": applied, **counts}, f, indent=1)
        f.write("\n")
    print(f"{name:28s} {depth.shape[0]:3d} x {depth.shape[1]:3d}  features = {len(features):4d}  applied = {applied:4d}  "
          f"feature cells = {counts['feature_cells']:6d}  {size} bytes")
    return labels, applied


def seabed(rng, h, w, depth=-30.0):
    rr, cc = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    return (depth + 0.02 * rr + 0.01 * cc + 0.05 * rng.standard_normal((h, w))).astype(F32)


def extent(labels, row=None, col=None):
    """The painted cells of one row or one column: (first, last)."""
    line = labels[row] if row is not None else labels[:, col]
    at = np.flatnonzero(line == 1)
    return int(at[0]), int(at[-1])


def main():
    os.makedirs(OUT, exist_ok=True)
    rng = np.random.default_rng(20240917)
    unit = (1000.0, 1.0, 0.0, 5000.0, 0.0, -1.0)          # 1 m cells, north up: x = 1000 + col, y = 5000 - row

    # ragged size; nodata, NaN and +-inf holes; discs that cross them
    h, w = 97, 203
    depth = seabed(rng, h, w)
    depth[10:30, 40:60] = NODATA
    depth[50:70, 100:130] = np.nan
    depth[80, 150:170] = np.inf
    depth[81, 150:170] = -np.inf
    depth[rng.random((h, w)) < 0.03] = NODATA
    features = [feat("WRECKS", 1050, 5000 - 25), feat("UWTROC", 1110, 5000 - 60), feat("OBSTRN", 1160, 5000 - 80),
                feat("UWTROC", 1020.7, 5000 - 90.2), feat("WRECKS", 1199.9, 5000 - 3.5)]
    labels, applied = run("ragged_holes_97x203", depth, unit, features)
    assert applied == 5 and (labels[10:30, 40:60] == -1).all() and (labels[50:70, 100:130] == -1).all()
    assert (labels[80:82, 150:170] == -1).all() and labels[25, 61] == 1 and labels[60, 99] == 1 and labels[79, 160] == 1

    # centres on all four edges and corners
    h, w = 64, 80
    depth = seabed(rng, h, w)
    features = [feat("UWTROC", 1000 + c + 0.5, 5000 - r - 0.5) for r, c in
                ((0, 0), (0, w - 1), (h - 1, 0), (h - 1, w - 1), (0, 40), (h - 1, 40), (32, 0), (32, w - 1))]
    labels, applied = run("edges_corners", depth, unit, features, {"UWTROC": 6})
    assert applied == 8 and labels[0, 0] == labels[0, w - 1] == labels[h - 1, 0] == labels[h - 1, w - 1] == 1
    assert extent(labels, row=0)[0] == 0 and extent(labels, row=32) == (0, w - 1) and labels[32, 7] == 0 and labels[6, 0] == 1 and labels[7, 0] == 0

    # centres just outside each side.  int() truncates towards zero: x half a pixel left of the origin is column 0, y half a pixel
    # above it is row 0 -- both in bounds; a pixel and a half out, or on the far edges, is out
    h, w = 40, 50
    depth = seabed(rng, h, w)
    features = [feat("UWTROC", 1000 - 0.5, 5000 - 20.5),          # column 0
                feat("UWTROC", 1025.5, 5000 + 0.5),               # row 0
                feat("UWTROC", 1000 - 1.5, 5000 - 10.5),          # column -1: out
                feat("UWTROC", 1010.5, 5000 + 1.5),               # row -1: out
                feat("UWTROC", 1000 + w, 5000 - 10.5),            # column w: out
                feat("UWTROC", 1010.5, 5000 - h)]                 # row h: out
    labels, applied = run("just_outside", depth, unit, features, {"UWTROC": 3})
    assert applied == 2 and extent(labels, row=20) == (0, 3) and extent(labels, col=0) == (17, 23)
    assert extent(labels, col=25) == (0, 3) and extent(labels, row=0) == (22, 28) and int((labels == 1).sum()) == 2 * 18
    features = [feat("UWTROC", 1000 - 0.999, 5000 + 0.999)]       # still (0, 0)
    labels, applied = run("just_outside_corner", depth, unit, features, {"UWTROC": 2})
    assert applied == 1 and extent(labels, row=0) == (0, 2) and extent(labels, col=0) == (0, 2) and int((labels == 1).sum()) == 6

    # a UTM-sized origin, 2 m cells
    h, w = 90, 120
    depth = seabed(rng, h, w)
    utm = (500000.0, 2.0, 0.0, 4.1e6, 0.0, -2.0)
    features = [feat("WRECKS", 500000 + 2 * 60.3, 4.1e6 - 2 * 45.8), feat("OBSTRN", 500000 + 2 * 10.99, 4.1e6 - 2 * 80.01)]
    labels, applied = run("utm_origin", depth, utm, features)
    assert applied == 2 and extent(labels, row=45) == (35, 85) and extent(labels, col=60) == (20, 70)     # 50 m / 2 m = 25
    assert extent(labels, row=80) == (0, 25) and extent(labels, col=10) == (65, 89)                        # 30 m / 2 m = 15

    # 0.3 m cells: 25 / 0.3 = 83.33 -> 84; 2.1 / 0.3 = 7.000000000000001 in float64 -> 8; 0.9 / 0.3 = 3.0 -> 3
    h, w = 180, 180
    depth = seabed(rng, h, w)
    fine = (0.0, 0.3, 0.0, 0.0, 0.0, -0.3)
    labels, applied = run("resolution_0p3_rock", depth, fine, [feat("UWTROC", 0.3 * 90.5, -0.3 * 90.5)])
    assert applied == 1 and extent(labels, row=90) == (6, 174) and extent(labels, col=90) == (6, 174)
    features = [feat("OBSTRN", 0.3 * 40.5, -0.3 * 40.5), feat("WRECKS", 0.3 * 120.5, -0.3 * 100.5)]
    labels, applied = run("resolution_0p3_ceil", depth, fine, features, {"OBSTRN": 2.1, "WRECKS": 0.9})
    assert applied == 2 and extent(labels, row=40) == (32, 48) and extent(labels, col=40) == (32, 48)
    assert extent(labels, row=100) == (117, 123) and extent(labels, col=120) == (97, 103)

    # non-square pixels: the radius in pixels comes from gt[1] alone, the disc is round in pixels
    h, w = 120, 70
    depth = seabed(rng, h, w)
    oblong = (200.0, 2.0, 0.0, 900.0, 0.0, -0.5)
    labels, applied = run("nonsquare_pixels", depth, oblong, [feat("OBSTRN", 200 + 2 * 35.5, 900 - 0.5 * 60.5)])
    assert applied == 1 and extent(labels, row=60) == (20, 50) and extent(labels, col=35) == (45, 75)

    # radius 0: the centre cell alone; an override dict; a negative override: counted, paints nothing
    h, w = 48, 56
    depth = seabed(rng, h, w)
    features = [feat("UWTROC", 1020.5, 5000 - 10.5), feat("WRECKS", 1040.5, 5000 - 30.5)]
    labels, applied = run("radius_zero", depth, unit, features, {"UWTROC": 0, "WRECKS": 0})
    assert applied == 2 and int((labels == 1).sum()) == 2 and labels[10, 20] == 1 and labels[30, 40] == 1
    features = [feat("UWTROC", 1020.5, 5000 - 10.5), feat("WRECKS", 1040.5, 5000 - 30.5), feat("OBSTRN", 1010.5, 5000 - 40.5)]
    labels, applied = run("radius_override", depth, unit, features, {"UWTROC": 4.2, "WRECKS": 7})
    assert applied == 3 and list(labels[10, 14:27]) == [0] + [1] * 11 + [0] and list(labels[22:24, 40]) == [0, 1]      # ceil(4.2) = 5; 7
    assert extent(labels, row=40) == (0, 40)
    labels, applied = run("negative_override", depth, unit, features, {"UWTROC": -5, "WRECKS": -0.5, "OBSTRN": 2})
    assert applied == 3 and labels[30, 40] == 1 and int((labels == 1).sum()) == 1 + 13      # ceil(-0.5) = -0 -> radius 0; OBSTRN radius 2

    # a radius larger than the grid
    depth = seabed(rng, 40, 50)
    depth[5:9, 5:9] = NODATA
    labels, applied = run("radius_larger_than_grid", depth, unit, [feat("UWTROC", 1001.5, 5000 - 1.5)], {"UWTROC": 1000})
    assert applied == 1 and int((labels == 1).sum()) == 40 * 50 - 16 and int((labels == -1).sum()) == 16

    # SBDARE / SOUNDG are not counted; an unknown class gets label 1 and radius 30
    depth = seabed(rng, 80, 90)
    features = [feat("SBDARE", 1040.5, 5000 - 40.5), feat("SOUNDG", 1020.5, 5000 - 20.5), feat("UWTROC", 1070.5, 5000 - 60.5)]
    labels, applied = run("context_classes", depth, unit, features, {"SBDARE": 10, "UWTROC": 5})
    assert applied == 1 and labels[40, 40] == 0 and labels[20, 20] == 0 and extent(labels, row=60) == (65, 75)
    labels, applied = run("unknown_class", depth, unit, [feat("PILPNT", 1045.5, 5000 - 40.5)])
    assert applied == 1 and extent(labels, row=40) == (15, 75) and extent(labels, col=45) == (10, 70)

    # all features out of bounds
    features = [feat("WRECKS", 900, 5000 - 10), feat("UWTROC", 1500, 5000 - 10), feat("OBSTRN", 1010, 5100), feat("WRECKS", 1010, 4000)]
    labels, applied = run("all_out_of_bounds", depth, unit, features)
    assert applied == 0 and int((labels == 0).sum()) == labels.size

    # degenerate shapes
    depth = seabed(rng, 1, 300)
    depth[0, 100:110] = np.nan
    labels, applied = run("one_row_1x300", depth, unit, [feat("UWTROC", 1095.5, 4999.5), feat("OBSTRN", 1250.5, 4999.5)])
    assert applied == 2 and extent(labels, row=0) == (70, 280) and int((labels == 1).sum()) == 51 - 10 + 61
    depth = seabed(rng, 300, 1)
    labels, applied = run("one_col_300x1", depth, unit, [feat("WRECKS", 1000.5, 5000 - 20.5), feat("UWTROC", 1000.5, 5000 - 299.5)])
    assert applied == 2 and extent(labels, col=0) == (0, 299) and int((labels == 1).sum()) == 71 + 26
    labels, applied = run("one_cell", seabed(rng, 1, 1), unit, [feat("UWTROC", 1000.5, 4999.5)])
    assert applied == 1 and labels[0, 0] == 1
    labels, applied = run("one_cell_nodata", np.full((1, 1), NODATA, F32), unit, [feat("UWTROC", 1000.5, 4999.5)])
    assert applied == 1 and labels[0, 0] == -1

    # heavily overlapping discs
    h, w = 150, 170
    depth = seabed(rng, h, w)
    depth[rng.random((h, w)) < 0.05] = np.nan
    classes = ["WRECKS", "UWTROC", "OBSTRN", "SBDARE", "PILPNT"]
    features = [feat(classes[int(rng.integers(5))], 1000 + rng.uniform(50, 120), 5000 - rng.uniform(40, 110)) for _ in range(200)]
    labels, applied = run("heavy_overlap", depth, unit, features, {"WRECKS": 12, "PILPNT": 3.5})
    assert applied == sum(q.object_class != "SBDARE" for q in features) and int((labels == 1).sum()) > 5000


if __name__ == "__main__":
    main()
