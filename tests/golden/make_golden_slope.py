#!/usr/bin/env python3
"""Golden vectors for the slope-based feature labels, produced by the REFERENCE's own ``scripts/prepare_feature_labels.py``:

    BGNN_REFERENCE=<reference checkout> python tests/golden/make_golden_slope.py

That script exists in the reference as a fenced Python block of ``docs/TRAINING_PLAN.md`` (phase 3).  This maker reads the one block
that names ``scripts/prepare_feature_labels.py`` at run time and executes it as a module with ``__file__`` set -- no text of it is
kept here -- with stand-ins: ``osgeo.gdal`` (``OpenEx`` serves the depth plane, ``GetDriverByName`` hands out the ``RecordingDriver``
of _reference_scripts.py), ``osgeo.ogr`` (``Open`` serves a point layer), ``osgeo.osr`` and an empty ``data.vr_bag``.  The script's
``add_feature_labels`` never passes ``min_cluster_size``: it is run for the default of 100, and ``create_feature_mask_from_slope`` is
called directly for the other values.  ``slope/slope_features.npz`` holds the depth planes, and per case its parameters, the mask
``create_feature_mask_from_slope`` returned, the labels the script wrote to band 1 and the wreck count it logged.

Depths are multiples of 3/64 m: ``s = gx**2 + gy**2`` then lies on the lattice ``9 (a^2 + b^2) / 16384``, which misses 1.0 (the cut
of 45 degrees) and every other cut used here by far more than the 64 ulp the maker asserts for every cell -- numpy's float32
``arctan`` may differ by a few ulp between SIMD paths, which moves a cut by about a dozen ulp of ``s`` at most, so the fixture holds
on any machine.  Every assert looks at the inputs and the reference's output alone.
"""
import contextlib
import io
import json
import logging
import os
import re
import sys
import tempfile
import types
from pathlib import Path

sys.dont_write_bytecode = True
import numpy as np
from scipy import ndimage

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from _reference_scripts import RecordingDriver, reference_root, save_npz  # noqa: E402

OUT = os.path.join(HERE, "slope")
F32 = np.float32
Q = 3.0 / 64.0
NODATA = 1.0e6
ULP_GUARD = 64


class _Band:
    def __init__(self, array):
        self.array = array

    def ReadAsArray(self):
        return np.array(self.array, copy=True)


class _Dataset:
    def __init__(self, depth, transform):
        self.depth, self.transform = depth, transform
        self.RasterYSize, self.RasterXSize = depth.shape

    def GetRasterBand(self, i):
        assert i == 1
        return _Band(self.depth)

    def GetGeoTransform(self):
        return self.transform

    def GetProjection(self):
        return ""


class _Point:
    def __init__(self, x, y):
        self.x, self.y = x, y

    def GetX(self):
        return self.x

    def GetY(self):
        return self.y


class _Feature:
    def __init__(self, x, y):
        self.point = _Point(x, y)

    def GetGeometryRef(self):
        return self.point

    def GetField(self, _name):
        return None


class _Layer:
    def __init__(self, points):
        self.points = points

    def GetLayer(self):
        return [_Feature(x, y) for x, y in self.points]


class _Capture(logging.Handler):
    def __init__(self):
        super().__init__()
        self.lines = []

    def emit(self, record):
        self.lines.append(record.getMessage())


def load_reference_block():
    """The reference's script as a module, the recording driver its ``gdal.GetDriverByName`` hands out, and the list that
    receives every mask its ``create_feature_mask_from_slope`` returns."""
    root = reference_root()
    text = open(os.path.join(root, "docs", "TRAINING_PLAN.md"), encoding="utf-8").read()
    blocks = [b for b in re.findall(r"```python\n(.*?)```", text, flags=re.S) if "scripts/prepare_feature_labels.py" in b]
    assert len(blocks) == 1, f"{len(blocks)} fenced Python blocks name scripts/prepare_feature_labels.py"
    driver = RecordingDriver()
    gdal = types.ModuleType("osgeo.gdal")
    gdal.GDT_Float32 = 6
    gdal.OF_RASTER = 2
    gdal.UseExceptions = lambda: None
    gdal.GetDriverByName = lambda _name: driver
    ogr, osr = types.ModuleType("osgeo.ogr"), types.ModuleType("osgeo.osr")
    osgeo = types.ModuleType("osgeo")
    osgeo.gdal, osgeo.ogr, osgeo.osr = gdal, ogr, osr
    data, vr_bag = types.ModuleType("data"), types.ModuleType("data.vr_bag")
    vr_bag.VRBagHandler = object
    data.vr_bag = vr_bag
    sys.modules.update({"osgeo": osgeo, "osgeo.gdal": gdal, "osgeo.ogr": ogr, "osgeo.osr": osr, "data": data, "data.vr_bag": vr_bag})
    mod = types.ModuleType("reference_prepare_feature_labels")
    mod.__file__ = os.path.join(root, "scripts", "prepare_feature_labels.py")
    path_before = list(sys.path)
    exec(compile(blocks[0], "prepare_feature_labels.py", "exec"), mod.__dict__)
    sys.path[:] = path_before                                   # (the script puts its checkout first)
    masks = []
    inner = mod.create_feature_mask_from_slope

    def recording(*a, **kw):
        masks.append(np.array(inner(*a, **kw), copy=True))
        return masks[-1].copy()

    mod.create_feature_mask_from_slope = recording
    mod.unwrapped_mask = inner
    return mod, driver, masks


ref, driver, recorded_masks = load_reference_block()
capture = _Capture()
ref.logger.addHandler(capture)
ref.logger.setLevel(logging.INFO)
ref.logger.propagate = False


def cut_bits(threshold):
    """The smallest non-negative float32 ``s`` (its bits) whose slope, as the script computes it, exceeds ``threshold``; -1 when
    there is none.  The maker's own bisection, stored beside the cases."""
    def exceeds(bits):
        s = np.array([bits], np.uint32).view(F32)
        with np.errstate(all="ignore"):
            return bool((np.degrees(np.arctan(np.sqrt(s))) > threshold)[0])
    if not exceeds(0x7F800000):
        return -1
    if exceeds(0):
        return 0
    lo, hi = 0, 0x7F800000
    while hi - lo > 1:
        mid = (lo + hi) // 2
        lo, hi = (lo, mid) if exceeds(mid) else (mid, hi)
    return hi


def assert_clear_of_cut(depth, bits):
    """No cell's ``s`` within ULP_GUARD float32 steps of the cut (non-negative floats order as their bit patterns)."""
    with np.errstate(all="ignore"):
        gy, gx = np.gradient(depth)
        s = gx ** 2 + gy ** 2
    sb = s[~np.isnan(s)].view(np.uint32).astype(np.int64)
    near = np.abs(sb - bits) <= ULP_GUARD
    assert not near.any(), f"{int(near.sum())} cells within {ULP_GUARD} ulp of the cut"


def run_script(depth, transform, threshold, wrecks=None, radius=50):
    """The script's ``add_feature_labels``: ``(mask, labels, wreck count)``."""
    ref.gdal.OpenEx = lambda _path, _flags=0, open_options=None: _Dataset(depth, transform)
    ref.ogr.Open = lambda _path: _Layer(wrecks)
    del recorded_masks[:], capture.lines[:]
    with tempfile.TemporaryDirectory() as tmp:
        shp = None
        if wrecks is not None:
            shp = Path(tmp) / "wrecks.shp"
            shp.write_bytes(b"")
        with contextlib.redirect_stdout(io.StringIO()), np.errstate(all="ignore"):
            ref.add_feature_labels(Path("survey.bag"), Path(tmp) / "out" / "labels.tif", shp, threshold, radius)
    ds = driver.datasets[-1]
    assert (ds.width, ds.height, len(ds.bands)) == (depth.shape[1], depth.shape[0], 2) and ds.geotransform == tuple(transform)
    assert [b.description for b in ds.bands] == ["labels", "depth"] and ds.bands[0].nodata == -1
    assert np.array_equal(ds.bands[1].array, depth, equal_nan=True)
    labels = ds.bands[0].array
    assert labels.dtype == F32 and set(np.unique(labels)) <= {-1.0, 0.0, 1.0}
    assert len(recorded_masks) == 1
    added = [re.fullmatch(r"Added (\d+) wrecks from database", line) for line in capture.lines]
    added = [int(m.group(1)) for m in added if m]
    assert len(added) == (0 if wrecks is None else 1)
    return recorded_masks[0], labels.astype(np.int8), (added[0] if added else 0)


def relief(rng, h, w):
    """A ragged relief in multiples of Q: plane waves whose slopes straddle 5 .. 45 degrees, sparse bumps (small clusters), 1.0e6
    holes, NaNs and an inf, and a flat shelf that carries the planted clusters."""
    rr, cc = np.meshgrid(np.arange(h, dtype=np.float64), np.arange(w, dtype=np.float64), indexing="ij")
    z = np.full((h, w), 30.0)
    for _ in range(4):
        fr, fc = rng.uniform(0.01, 0.04, 2) * rng.choice([-1, 1], 2)
        z += rng.uniform(0.4, 1.6) * np.sin(2 * np.pi * (fr * rr + fc * cc) + rng.uniform(0, 2 * np.pi))
    bumps = rng.random((h, w)) < 0.004
    z[bumps] += rng.uniform(0.5, 4.0, int(bumps.sum()))
    d = (np.round(z / Q) * Q).astype(F32)
    for _ in range(5):                                          # holes
        r, c, a, b = rng.integers(0, h - 12), rng.integers(0, w - 12), rng.integers(2, 12), rng.integers(2, 12)
        d[r:r + a, c:c + b] = NODATA
    d[rng.random((h, w)) < 0.003] = np.nan
    return d


def plant_segment(d, r, c0, length, nan_above=None):
    """A flat shelf of 21.0 with one row segment raised by 9.0: the rows above and below (``length`` cells each) and four cells at
    the ends are steep at 5, 15 and 45 degrees alike (gradients of 4.5 and 9): one cluster of ``2 * length + 4`` cells.  A NaN two
    rows above takes one cell out of the upper row (a NaN in the stencil is never steep) without splitting the cluster."""
    d[r - 6:r + 7, c0 - 6:c0 + length + 6] = 21.0
    d[r, c0:c0 + length] = 30.0
    if nan_above is not None:
        d[r - 2, nan_above] = np.nan


def main():
    os.makedirs(OUT, exist_ok=True)
    rng = np.random.default_rng(20241019)
    arrays, cases = {}, {}
    bits = {t: cut_bits(t) for t in (5.0, 15.0, 45.0)}
    arrays["cut_thresholds"] = np.array(sorted(bits), np.float64)
    arrays["cut_bits"] = np.array([bits[t] for t in sorted(bits)], np.int64)

    def case(name, plane, threshold, min_cluster_size, mask, labels=None, transform=None, wrecks=None, radius=None, count=None):
        cases[name] = {"plane": plane, "threshold": threshold, "min_cluster_size": min_cluster_size, "transform": transform,
                       "wrecks": wrecks, "radius": radius, "wreck_count": count, "has_labels": labels is not None}
        arrays[name + "_mask"] = mask.astype(np.uint8)
        if labels is not None:
            arrays[name + "_labels"] = labels
        print(f"{name:24s} {plane:16s} steep kept = {int(mask.sum()):6d}  features = {-1 if labels is None else int((labels == 1).sum()):6d}")

    # the ragged relief: 300 x 301, a north-up transform with non-square pixels
    h, w = 300, 301
    gt = (500000.0, 2.0, 0.0, 4100000.0, 0.0, -1.5)
    d = relief(rng, h, w)
    plant_segment(d, 40, 60, 48)                                # 100 cells
    plant_segment(d, 80, 200, 48, nan_above=220)                # 99 cells
    d[150, 150] = np.inf
    arrays["relief_300x301"] = d
    for t in sorted(bits):
        assert_clear_of_cut(d, bits[t])
    for t in sorted(bits):
        mask, labels, _ = run_script(d, gt, t)
        case(f"relief_t{int(t)}", "relief_300x301", t, 100, mask, labels, gt)
    all_mask = ref.unwrapped_mask(d.copy(), 15.0, 1)
    case("relief_t15_min1", "relief_300x301", 15.0, 1, all_mask)
    case("relief_t15_min37", "relief_300x301", 15.0, 37, ref.unwrapped_mask(d.copy(), 15.0, 37))
    lab, n = ndimage.label(all_mask)
    sizes = np.bincount(lab.ravel())[1:]
    kept = arrays["relief_t15_mask"].astype(bool)
    assert 99 in sizes and 100 in sizes and lab[39, 70] and sizes[lab[39, 70] - 1] == 100 and sizes[lab[79, 210] - 1] == 99
    assert kept[39, 70] and not kept[79, 210] and all_mask[79, 210]
    assert (sizes < 37).any() and (sizes >= 100).sum() >= 3 and kept.sum() == sizes[sizes >= 100].sum()
    assert np.isnan(d).any() and np.isinf(d).any() and (d == F32(NODATA)).any()
    valid = (d != F32(NODATA)) & np.isfinite(d)
    assert (kept & ~valid).any(), "hole border cells are steep and counted into the clusters"

    # wrecks on the relief: a corner, half a pixel and one and a half pixels outside each edge (int() truncates towards zero: the
    # first lands in row / column 0, the second is skipped), on a hole, overlapping the planted 100-cell cluster, on the shelf
    def at(row, col):                                           # the centre of a pixel, geo
        return (gt[0] + (col + 0.5) * gt[1], gt[3] + (row + 0.5) * gt[5])
    hole = np.argwhere(d == F32(NODATA))[0]
    wrecks = [at(0, 0), at(h - 1, w - 1), at(-1, 150), at(-2, 150), at(150, -1), at(150, -2), at(h, 100), at(100, w),
              at(hole[0], hole[1]), at(40, 70), at(200, 120)]
    radius = 7
    mask, labels, count = run_script(d, gt, 15.0, wrecks, radius)
    case("relief_t15_wrecks", "relief_300x301", 15.0, 100, mask, labels, gt, [list(p) for p in wrecks], radius, count)
    assert count == 7 and np.array_equal(mask, kept), count          # (4 of the 11 lie off the grid)
    plain = arrays["relief_t15_labels"]
    assert (labels == 1).sum() > (plain == 1).sum() and labels[hole[0], hole[1]] == -1 and np.array_equal(labels == -1, plain == -1)
    for r, c in ((0, 0), (h - 1, w - 1), (0, 150), (150, 0), (40, 70), (200, 120)):
        assert valid[r, c] and labels[r, c] == 1, (r, c)
    assert (plain[200 - radius:200 + radius + 1, 120 - radius:120 + radius + 1] == 0).any() and kept[39, 70]

    # a 2 x 2 plane: every difference is one-sided
    d2 = np.array([[0.0, 3.0], [6.0, 30.0]], F32)
    arrays["tiny_2x2"] = d2
    for t in sorted(bits):
        assert_clear_of_cut(d2, bits[t])
    mask, labels, _ = run_script(d2, gt, 15.0)
    case("tiny_t15", "tiny_2x2", 15.0, 100, mask, labels, gt)
    assert not mask.any()
    m1 = ref.unwrapped_mask(d2.copy(), 15.0, 1)
    case("tiny_t15_min1", "tiny_2x2", 15.0, 1, m1)
    assert m1.all()

    # nothing steep: a gentle ramp (1.7 degrees)
    dn = (np.round((20.0 + 0.03 * np.arange(50, dtype=np.float64)[None, :] + np.zeros((40, 1))) / Q) * Q).astype(F32)
    arrays["gentle_40x50"] = dn
    assert_clear_of_cut(dn, bits[5.0])
    mask, labels, _ = run_script(dn, gt, 5.0)
    case("gentle_t5", "gentle_40x50", 5.0, 100, mask, labels, gt)
    assert not mask.any() and not labels.any()

    arrays["cases"] = np.array(json.dumps(cases))
    size = save_npz(os.path.join(OUT, "slope_features.npz"), arrays)
    assert size <= 200 * 1024, size
    print(f"slope/slope_features.npz: {size} bytes; cut bits {bits}")


if __name__ == "__main__":
    main()
