#!/usr/bin/env python3
"""Golden vectors for ground truth from survey pairs, produced by the REFERENCE's own ``scripts/prepare_ground_truth.py``:

    BGNN_REFERENCE=<reference checkout> python tests/golden/make_golden_truth.py

The script is loaded with stand-ins for GDAL and for the reference's ``data`` package (_reference_scripts.py); its ``load_survey``
is replaced by a function that returns prepared grids, and the GDAL driver records the five bands it writes.  Each
``truth/<case>.npz`` holds the two input grids and the reference's outputs (returned labels / difference, the recorded bands and
geotransform, the median it removed; bands 3 / 4 only where the pair was cropped, else they are the input depths); ``truth/<case>.json`` is its statistics file; ``truth/errors.json`` holds the messages of
its two refusals.

Every assert below looks at the reference's output alone: a case must exercise what its name claims whatever implementation is
later tested against it.  Where a case needs the raw difference to be an exact value, the clean depth is 0 (or -32 with steps of
2^-18), so that float32 ``noisy - clean`` returns the value that was put in.
"""
import json
import os
import sys
import tempfile
import types
import warnings
from pathlib import Path

sys.dont_write_bytecode = True
import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from _reference_scripts import load_reference_script, save_npz  # noqa: E402

ref, driver = load_reference_script("prepare_ground_truth")
OUT = os.path.join(HERE, "truth")
F32 = np.float32
NODATA = F32(1.0e6)


def grid(depth, unc=None, origin=(0.0, None), res=1.0):
    """A loaded survey as the reference's loader returns it: north-up, ``origin`` = (west edge, north edge)."""
    h, w = depth.shape
    x0 = origin[0]
    y0 = origin[1] if origin[1] is not None else h * res
    return types.SimpleNamespace(depth=depth, uncertainty=unc, transform=(x0, res, 0.0, y0, 0.0, -res), crs="EPSG:32619",
                                 resolution=(res, res), bounds=(x0, y0 - h * res, x0 + w * res, y0), nodata_value=1.0e6)


def key(v):
    u = np.asarray(v, F32).view(np.uint32).astype(np.uint64)
    return np.where(u >> 31, ~u & 0xFFFFFFFF, u | 0x80000000).astype(np.uint32)


def run(name, clean, noisy, threshold=0.15):
    """One call of the reference's compute_ground_truth; returns what it computed, and writes the fixture."""
    surveys = {f"{name}_clean.bag": clean, f"{name}_noisy.bag": noisy}
    ref.load_survey = lambda path, mode="resampled": surveys[Path(path).name]
    driver.datasets.clear()
    with tempfile.TemporaryDirectory() as tmp, warnings.catch_warnings():
        warnings.simplefilter("ignore")                      # the median and the percentages of an empty selection
        labels, difference = ref.compute_ground_truth(Path(f"{name}_clean.bag"), Path(f"{name}_noisy.bag"), Path(tmp), threshold)
        stats = json.load(open(os.path.join(tmp, f"{name}_ground_truth_stats.json")))
    ds, = driver.datasets
    bands = [b.array for b in ds.bands]
    assert [b.description for b in ds.bands] == ["labels", "difference", "noisy_depth", "clean_depth", "uncertainty"]
    assert all(b.dtype == np.float32 and b.shape == labels.shape for b in bands) and labels.dtype == np.int32
    assert np.array_equal(bands[0], labels.astype(F32))
    valid = labels >= 0
    raw = bands[2] - bands[3]                                 # the reference's own crops: noisy - clean
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        offset = np.median(raw[valid])                        # (the reference's line 171 on its own arrays)
    assert offset.dtype == np.float32
    # the rule the device code follows, checked against what the reference wrote
    s = np.sort(raw[valid])
    n = s.size
    if n:
        rule = s[(n - 1) // 2] if n % 2 else F32(s[n // 2 - 1] + s[n // 2]) / F32(2)
        assert rule == offset and np.array_equal(bands[1][valid], raw[valid] - offset)
    else:
        assert np.isnan(offset)
    assert np.isnan(bands[1][~valid]).all() and stats["valid_cells"] == n
    out = {"clean_depth": clean.depth, "noisy_depth": noisy.depth, "clean_transform": np.array(clean.transform, np.float64),
           "noisy_transform": np.array(noisy.transform, np.float64), "clean_bounds": np.array(clean.bounds, np.float64),
           "noisy_bounds": np.array(noisy.bounds, np.float64), "clean_resolution": np.array(clean.resolution, np.float64),
           "noisy_resolution": np.array(noisy.resolution, np.float64), "threshold": np.float64(threshold),
           "labels": labels, "difference": difference, "offset": offset, "geotransform": np.array(ds.geotransform, np.float64)}
    same = {3: noisy.depth, 4: clean.depth}              # bands 3 / 4 of an uncropped pair are the inputs: kept once
    for i, b in enumerate(bands):
        if i + 1 in same and b.shape == same[i + 1].shape:
            assert np.array_equal(b.view(np.uint32), same[i + 1].view(np.uint32))
            continue
        out[f"band{i + 1}"] = b
    if clean.uncertainty is not None:
        out["clean_uncertainty"] = clean.uncertainty
    if noisy.uncertainty is not None:
        out["noisy_uncertainty"] = noisy.uncertainty
    size = save_npz(os.path.join(OUT, name + ".npz"), out)
    assert size < (1 << 20), (name, size)
    with open(os.path.join(OUT, name + ".json"), "w") as f:
        json.dump(stats, f, indent=2, sort_keys=True)
        f.write("\n")
    print(f"{name:18s} {labels.shape[0]:3d} x {labels.shape[1]:3d}  n = {n:6d}  offset = {float(offset)!r:24s} noise = {stats['noise_cells']:5d}  {size} bytes")
    return types.SimpleNamespace(labels=labels, difference=difference, bands=bands, stats=stats, sorted=s, n=n, offset=offset, valid=valid)


def realistic(rng, h, w, sigma=0.1, shift=0.2, holes=0.05, unc=True):
    clean = (-30 + 5 * rng.standard_normal((h, w))).astype(F32)
    noisy = (clean + (shift + sigma * rng.standard_normal((h, w))).astype(F32)).astype(F32)
    clean[rng.random((h, w)) < holes] = NODATA
    noisy[rng.random((h, w)) < holes] = np.nan
    cu = (0.1 + 0.05 * rng.random((h, w))).astype(F32) if unc else None
    nu = (0.2 + 0.1 * rng.random((h, w))).astype(F32) if unc else None
    return clean, noisy, cu, nu


def exact(values, shape, rng, invalid_fill=True):
    """A pair whose valid raw differences are exactly ``values`` (clean depth 0), shuffled over ``shape``; the remaining cells
    are invalid."""
    values = np.asarray(values, F32)
    cells = shape[0] * shape[1]
    assert values.size <= cells
    noisy = np.full(cells, np.nan, F32)
    noisy[:values.size] = values
    clean = np.zeros(cells, F32)
    clean[values.size:] = NODATA if invalid_fill else 0
    perm = rng.permutation(cells)
    unc = (0.2 + 0.1 * rng.random(cells)).astype(F32)
    return clean[perm].reshape(shape), noisy[perm].reshape(shape), unc.reshape(shape)


def main():
    os.makedirs(OUT, exist_ok=True)
    rng = np.random.default_rng(20240611)

    # odd and even valid counts
    c, z, cu, nu = realistic(rng, 33, 31)
    if ((c != NODATA) & np.isfinite(z)).sum() % 2 == 0:
        c[np.argwhere((c != NODATA) & np.isfinite(z))[0][0], np.argwhere((c != NODATA) & np.isfinite(z))[0][1]] = NODATA
    r = run("odd_count", grid(c, cu), grid(z, nu))
    assert r.n % 2 == 1 and r.n > 900 and 0 < r.stats["noise_cells"] < r.n
    c, z, cu, nu = realistic(rng, 40, 37)
    if ((c != NODATA) & np.isfinite(z)).sum() % 2 == 1:
        i, j = np.argwhere((c != NODATA) & np.isfinite(z))[0]
        c[i, j] = NODATA
    r = run("even_count", grid(c, cu), grid(z, nu))
    assert r.n % 2 == 0 and r.n > 1200 and r.sorted[r.n // 2 - 1] != r.sorted[r.n // 2]

    # an even count whose middle elements differ in the sign bit
    vals = np.concatenate([-(0.01 * np.arange(1, 201)), 0.01 * np.arange(1, 201)]).astype(F32)
    c, z, u = exact(vals, (24, 20), rng)
    r = run("even_sign", grid(c, u), grid(z, u))
    a, b = r.sorted[r.n // 2 - 1], r.sorted[r.n // 2]
    assert r.n == 400 and np.signbit(a) and not np.signbit(b) and a == -b and r.offset == 0

    # an even count whose middle elements differ only in the low 10 mantissa bits: equal through both 11-bit levels
    base = F32(0.37)
    lo = base
    hi = (base.view(np.uint32) + np.uint32(5)).view(F32)
    assert (base.view(np.uint32) & 0x3FF) + 5 < 1024
    vals = np.concatenate([np.linspace(0.2, 0.36, 149), [lo, hi], np.linspace(0.38, 0.6, 149)]).astype(F32)
    c, z, u = exact(vals, (20, 16), rng)
    r = run("even_low_bits", grid(c, u), grid(z, u))
    a, b = r.sorted[r.n // 2 - 1], r.sorted[r.n // 2]
    assert r.n == 300 and a == lo and b == hi and 0 < (int(key(a)) ^ int(key(b))) < 1024

    # long runs of duplicates across the median
    vals = np.concatenate([np.full(250, 0.125), np.full(1000, 0.25), np.full(350, 0.5)]).astype(F32)
    c, z, u = exact(vals, (40, 40), rng, invalid_fill=False)
    r = run("duplicates", grid(c, u), grid(z, u))
    assert r.n == 1600 and r.sorted[r.n // 2 - 1] == r.sorted[r.n // 2] == F32(0.25) and (r.sorted == F32(0.25)).sum() == 1000
    assert r.stats["noise_cells"] == 350                     # 0.5 - 0.25 > 0.15 > 0.25 - 0.125

    # all differences equal (clean -32, noisy -31.875)
    c = np.full((17, 19), -32.0, F32)
    z = np.full((17, 19), -31.875, F32)
    u = (0.2 + 0.1 * rng.random((17, 19))).astype(F32)
    r = run("all_equal", grid(c, u), grid(z, u))
    assert r.n == 17 * 19 and r.sorted[0] == r.sorted[-1] == F32(0.125) and r.stats["noise_cells"] == 0
    assert "mean_noise_magnitude" not in r.stats and not r.bands[1].any()

    # n = 1, n = 2 and n = 0 valid cells
    for n_valid, vals in ((1, [0.75]), (2, [0.25, -1.5]), (0, [])):
        c, z, u = exact(vals, (8, 8), rng)
        r = run(f"n{n_valid}", grid(c, u), grid(z, u))
        assert r.n == n_valid and (r.labels >= 0).sum() == n_valid
        if n_valid == 2:
            assert r.offset == F32(-0.625) and r.stats["noise_cells"] == 2
        if n_valid == 0:
            assert r.stats["noise_percentage"] == 0 and np.isnan(r.bands[1]).all() and np.isnan(r.bands[4]).all()

    # NaN, +-inf and nodata holes in either plane
    c, z, cu, nu = realistic(rng, 32, 32, holes=0.0)
    specials = [np.nan, np.inf, -np.inf, NODATA]
    spots = rng.permutation(32 * 32)[:80].reshape(2, 4, 10)
    for plane, arr in enumerate((c, z)):
        for k, v in enumerate(specials):
            arr.reshape(-1)[spots[plane, k]] = v
    r = run("holes", grid(c, cu), grid(z, nu))
    bad = np.zeros(32 * 32, bool)
    bad[spots.reshape(-1)] = True
    assert np.array_equal(r.labels.reshape(-1) < 0, bad) and r.n == 32 * 32 - 80
    assert np.isnan(r.bands[4].reshape(-1)[bad]).all() and not np.isnan(r.bands[4].reshape(-1)[~bad]).any()

    # tightly clustered: sigma = 1 cm around a 37 cm offset, 1 % outliers
    c = (-30 + 5 * rng.standard_normal((64, 64))).astype(F32)
    d = 0.37 + 0.01 * rng.standard_normal((64, 64))
    out = rng.random((64, 64)) < 0.01
    d[out] += rng.choice([-1.0, 1.0], int(out.sum())) * rng.uniform(0.5, 3.0, int(out.sum()))
    z = (c + d.astype(F32)).astype(F32)
    u = (0.2 + 0.1 * rng.random((64, 64))).astype(F32)
    r = run("clustered", grid(c, u), grid(z, u))
    top = key(r.sorted) >> 21
    assert abs(float(r.offset) - 0.37) < 0.002 and np.bincount(top.astype(np.int64)).max() > 0.45 * r.n, "most keys share a top-level bin"
    assert 20 <= r.stats["noise_cells"] <= 70

    # |difference| exactly float32(threshold) and its two float32 neighbours (median exactly 0: the zeros outnumber the rest)
    for thr in (0.15, 0.5):
        t = F32(thr)
        below, above = np.nextafter(t, F32(0)), np.nextafter(t, F32(1))
        edge = np.array([below, t, above], F32)
        vals = np.concatenate([np.zeros(200, F32), np.repeat(edge, 4), -np.repeat(edge, 4), [F32(2 * thr), F32(-2 * thr)]])
        c, z, u = exact(vals, (16, 16), rng)
        name = f"threshold_{int(round(thr * 100)):03d}"
        r = run(name, grid(c, u), grid(z, u), threshold=thr)
        assert r.offset == 0 and r.n == 226
        mag = np.abs(r.bands[1])
        for v, lab in ((below, 0), (t, 0), (above, 2)):      # the comparison is float32's: float(t) > thr does not make t noise
            assert (mag == v).sum() == 8 and (r.labels[mag == v] == lab).all(), (name, v, lab)
        assert (float(t) > thr) == (thr == 0.15), "float32(0.15) > 0.15, float32(0.5) == 0.5"
        assert r.stats["noise_cells"] == 8 + 2 and r.stats["max_noise_magnitude"] == float(F32(2 * thr))

    # without an uncertainty plane
    c, z, _, _ = realistic(rng, 21, 27, unc=False)
    r = run("no_uncertainty", grid(c), grid(z))
    assert np.isnan(r.bands[4]).all() and r.n > 400

    # different extents, fractional-pixel offsets (half-metre cells; the noisy survey lies 3.2 m east and 1.3 m south)
    c, _, cu, _ = realistic(rng, 40, 50, holes=0.03)
    _, z, _, nu = realistic(rng, 45, 48, holes=0.03)
    clean = grid(c, cu, origin=(100.0, 200.0), res=0.5)
    noisy = grid(z, nu, origin=(103.2, 198.7), res=0.5)
    r = run("extents", clean, noisy)
    assert r.labels.shape == (37, 44) and r.labels.shape != c.shape and r.labels.shape != z.shape
    assert np.array_equal(r.bands[3], c[3:40, 6:50], equal_nan=True) and np.array_equal(r.bands[2], z[0:37, 0:44], equal_nan=True)

    # the one larger case: more than one workgroup's worth of cells, a row length that is no multiple of anything.  Values on
    # coarse binary grids keep the file small.
    h, w = 300, 257
    c = (np.round((-30 + 5 * rng.standard_normal((h, w))) * 16) / 16).astype(F32)
    d = (np.round((0.21 + 0.08 * rng.standard_normal((h, w))) * 256) / 256).astype(F32)
    z = (c + d).astype(F32)
    c[rng.random((h, w)) < 0.04] = NODATA
    z[rng.random((h, w)) < 0.04] = np.nan
    u = (np.round((0.2 + 0.1 * rng.random((h, w))) * 64) / 64).astype(F32)
    r = run("large", grid(c, u), grid(z, u))
    assert r.n > 70000 and 0 < r.stats["noise_cells"] < r.n // 4

    # the two refusals of the alignment
    errors = {}
    c, z, _, _ = realistic(rng, 8, 8, unc=False)
    for name, clean, noisy in (("no_overlap", grid(c, origin=(0.0, 8.0)), grid(z, origin=(8.0, 8.0))),
                               ("resolution", grid(c, res=1.0), grid(z, res=1.02))):
        surveys = {"a": clean, "b": noisy}
        ref.load_survey = lambda path, mode="resampled": surveys[Path(path).name]
        try:
            ref.compute_ground_truth(Path("a"), Path("b"), Path("unused"))
            raise AssertionError(name)
        except ValueError as e:
            errors[name] = {"message": str(e), "clean_bounds": list(clean.bounds), "noisy_bounds": list(noisy.bounds),
                            "clean_resolution": list(clean.resolution), "noisy_resolution": list(noisy.resolution),
                            "clean_transform": list(clean.transform), "noisy_transform": list(noisy.transform)}
    assert "overlap" in errors["no_overlap"]["message"] and "Resolution mismatch" in errors["resolution"]["message"]
    with open(os.path.join(OUT, "errors.json"), "w") as f:
        json.dump(errors, f, indent=2, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
