"""Slope-based feature labels without a GPU: the CPU oracle against the fixture the reference's own
``scripts/prepare_feature_labels.py`` wrote (tests/golden/make_golden_slope.py), ``slope_cut``, ``wreck_pixel_table`` and the Python
layer's refusals."""
import os

import numpy as np
import pytest

import _slope_cpu as cpu
from bathymetric_gnn_amd.data import add_feature_labels, create_feature_mask_from_slope, slope_cut, wreck_pixel_table

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES, CUTS = cpu.load_fixture()


def _predicate(bits, threshold):
    s = np.array([bits], np.uint32).view(np.float32)
    with np.errstate(all="ignore"):
        return bool((np.degrees(np.arctan(np.sqrt(s))) > threshold)[0])


@pytest.mark.parametrize("name", sorted(CASES))
def test_restatement_reproduces_the_reference(name):
    c = CASES[name]
    labels, mask, stats, count = cpu.add_feature_labels(c["depth"], c["threshold"], c["min_cluster_size"], c["wrecks"], c["transform"],
                                                        c["radius"] if c["radius"] is not None else 50)
    assert np.array_equal(mask, c["mask"])
    assert stats["kept_cells"] == int(c["mask"].sum())
    if c["labels"] is not None:
        assert np.array_equal(labels, c["labels"])
    if c["wreck_count"] is not None:
        assert count == c["wreck_count"]


def test_fixture_covers_its_cases():
    c = CASES["relief_t15_min1"]
    d = c["depth"]
    assert d.shape == (300, 301) and np.isnan(d).any() and np.isinf(d).any() and (d == np.float32(cpu.NODATA)).any()
    from scipy import ndimage
    lab, n = ndimage.label(c["mask"])
    sizes = np.bincount(lab.ravel())[1:]
    kept = CASES["relief_t15"]["mask"]
    assert 99 in sizes and 100 in sizes and kept.sum() == sizes[sizes >= 100].sum() and (kept & ~cpu.valid_cells(d)).any()
    assert {CASES[k]["threshold"] for k in CASES} == {5.0, 15.0, 45.0} == set(CUTS)
    assert CASES["tiny_t15_min1"]["depth"].shape == (2, 2) and CASES["tiny_t15_min1"]["mask"].all()
    assert not CASES["gentle_t5"]["mask"].any()
    w = CASES["relief_t15_wrecks"]
    assert w["wreck_count"] == 7 < len(w["wrecks"]) and w["transform"][1] != -w["transform"][5]
    for name, case in CASES.items():                            # the maker's condition, with the maker's cuts
        cut = np.array([CUTS[case["threshold"]]], np.uint32).view(np.float32)[0]
        assert cpu.ulps_from_cut(case["depth"], cut) > cpu.ULP_GUARD, name
    assert os.path.getsize(cpu.FIXTURE) <= 200 * 1024


@pytest.mark.parametrize("threshold", [5.0, 15.0, 45.0, 0.001, 89.9])
def test_slope_cut_is_the_first_float_over_the_threshold(threshold):
    cut = slope_cut(threshold)
    assert cut.dtype == np.float32 and cut > 0
    bits = int(cut.view(np.uint32))
    assert _predicate(bits, threshold) and not _predicate(bits - 1, threshold)
    if threshold in CUTS:
        assert abs(bits - CUTS[threshold]) <= cpu.ULP_GUARD


def test_slope_cut_edges():
    for t in (90.0, 1000.0, float("nan")):
        assert np.isnan(slope_cut(t)), t
    assert slope_cut(-1.0) == 0.0 and slope_cut(-1.0).dtype == np.float32
    assert np.sqrt(slope_cut(15.0)) == pytest.approx(np.tan(np.radians(15.0)), rel=1e-6)


def test_wreck_pixel_table_against_the_fixture():
    c = CASES["relief_t15_wrecks"]
    wrecks = [{"x": x, "y": y, "name": "Unknown"} for x, y in c["wrecks"]]
    table, count = wreck_pixel_table(wrecks, c["transform"], c["depth"].shape, c["radius"])
    assert count == c["wreck_count"] == len(table) and table.dtype == np.int32 and table.shape == (count, 4)
    assert [tuple(r[:2]) for r in table.tolist()] == cpu.wreck_pixels(c["wrecks"], c["transform"], c["depth"].shape)
    assert (table[:, 2] == c["radius"]).all() and (table[:, 3] == 1).all()
    # int() truncates towards zero: half a pixel outside lands in row / column 0, one and a half pixels outside is skipped
    assert (0, 150) in [tuple(r[:2]) for r in table.tolist()] and (150, 0) in [tuple(r[:2]) for r in table.tolist()]

    class P:
        def __init__(self, x, y):
            self.x, self.y = x, y
    table2, count2 = wreck_pixel_table([P(x, y) for x, y in c["wrecks"]], c["transform"], c["depth"].shape, c["radius"])
    assert count2 == count and np.array_equal(table2, table)
    empty, zero = wreck_pixel_table([], c["transform"], (5, 5))
    assert zero == 0 and empty.shape == (0, 4) and empty.dtype == np.int32
    big, _ = wreck_pixel_table(wrecks[:1], c["transform"], (300, 301), 10 ** 12)
    assert big[0, 2] == 601


def test_refusals_without_a_gpu():
    for shape in ((1, 7), (7, 1), (1, 1)):
        with pytest.raises(ValueError, match="gradient"):
            create_feature_mask_from_slope(np.zeros(shape, np.float32))
        with pytest.raises(ValueError, match="gradient"):
            add_feature_labels(np.zeros(shape, np.float32))
        with pytest.raises(ValueError):
            np.gradient(np.zeros(shape, np.float32))            # (what the reference meets)
    with pytest.raises(ValueError):
        create_feature_mask_from_slope(np.zeros((3, 4, 5), np.float32))
    gt = (0.0, 1.0, 0.0, 0.0, 0.0, -1.0)
    with pytest.raises(TypeError):
        wreck_pixel_table([{"x": 1.0, "y": -1.0}], gt, (4, 4), 2.5)
    with pytest.raises(TypeError):
        add_feature_labels(np.zeros((4, 4), np.float32), [{"x": 1.0, "y": -1.0}], wreck_radius=50.0, transform=gt)
    with pytest.raises(ValueError, match="transform"):
        add_feature_labels(np.zeros((4, 4), np.float32), [{"x": 1.0, "y": -1.0}])
