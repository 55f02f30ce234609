"""Feature labels, the parts that need no GPU: ``feature_pixel_table`` (the reference's float64 geo arithmetic) against the fixtures
the reference's own ``create_feature_labels`` produced (tests/golden/make_golden_features.py), the CPU oracle of _features_cpu bit
for bit against the same fixtures, and the host plan (``bgnn_feature_labels_plan`` through the C ABI, no device): descending lists,
cut at the first disc that holds a whole bin, empty where no disc reaches, sized as the query says, and resolving to the oracle's
labels."""
import logging

import numpy as np
import pytest

import _features_cpu as fc

CASES = fc.load_cases()
IDS = [c.name for c in CASES]
EXPECTED_CASES = {"ragged_holes_97x203", "edges_corners", "just_outside", "just_outside_corner", "utm_origin", "resolution_0p3_rock",
                  "resolution_0p3_ceil", "nonsquare_pixels", "radius_zero", "radius_override", "negative_override",
                  "radius_larger_than_grid", "context_classes", "unknown_class", "all_out_of_bounds", "one_row_1x300", "one_col_300x1",
                  "one_cell", "one_cell_nodata", "heavy_overlap"}


def _table(case):
    from bathymetric_gnn_amd.data import feature_pixel_table
    return feature_pixel_table(case.features, case.transform, case.depth.shape, case.feature_radius)


def test_every_case_is_there():
    assert set(IDS) == EXPECTED_CASES
    for c in CASES:
        assert c.depth.dtype == np.float32 and c.labels.dtype == np.int32 and c.labels.shape == c.depth.shape == tuple(c.meta["shape"])
        assert np.array_equal(c.band_depth, c.depth, equal_nan=True)
        assert c.meta["feature_cells"] == int((c.labels == 1).sum()) and c.meta["valid_cells"] == int((c.labels >= 0).sum())


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_pixel_table_and_oracle_reproduce_the_reference(case):
    """The table has one row per feature the reference logged as applied, and painting it gives the reference's band bit for bit
    (which checks centre, radius and label of every feature that shows, and the order)."""
    table, applied = _table(case)
    assert table.dtype == np.int32 and table.shape == (applied, 4) and table.flags.c_contiguous
    assert applied == case.meta["applied_features"]
    labels, counts = fc.feature_labels(table, case.depth)
    assert labels.dtype == np.int32 and np.array_equal(labels, case.labels)
    assert counts == {k: case.meta[k] for k in ("valid_cells", "feature_cells", "painted_cells")}


def test_pixel_table_entries():
    """The entries the fixtures pin, each asserted from the reference's output in the generator: truncation towards zero, ceil,
    skipped and uncounted features, the clamp, a negative radius."""
    by = {c.name: c for c in CASES}
    t = lambda name: _table(by[name])[0].tolist()
    assert t("just_outside") == [[20, 0, 3, 1], [0, 25, 3, 1]]              # x = origin - 0.5 -> column 0; y = origin + 0.5 -> row 0
    assert t("just_outside_corner") == [[0, 0, 2, 1]]
    assert t("utm_origin") == [[45, 60, 25, 1], [80, 10, 15, 1]]
    assert t("resolution_0p3_rock") == [[90, 90, 84, 1]]                    # 25 / 0.3 = 83.3
    assert t("resolution_0p3_ceil") == [[40, 40, 8, 1], [100, 120, 3, 1]]   # 2.1 / 0.3 = 7.000000000000001; 0.9 / 0.3 = 3.0
    assert t("nonsquare_pixels") == [[60, 35, 15, 1]]                       # 30 m / gt[1] = 2 m, whatever gt[5]
    assert t("radius_zero") == [[10, 20, 0, 1], [30, 40, 0, 1]]
    assert t("radius_override") == [[10, 20, 5, 1], [30, 40, 7, 1], [40, 10, 30, 1]]
    assert t("negative_override") == [[10, 20, -5, 1], [30, 40, 0, 1], [40, 10, 2, 1]]     # ceil(-0.5) = -0.0
    assert t("radius_larger_than_grid") == [[1, 1, 90, 1]]                  # 1000 clamped to 40 + 50
    assert t("context_classes") == [[60, 70, 5, 1]]                         # SBDARE and SOUNDG: label None, not counted
    assert t("unknown_class") == [[40, 45, 30, 1]]
    assert t("all_out_of_bounds") == [] and _table(by["all_out_of_bounds"])[0].shape == (0, 4)


def test_local_class_table_and_records():
    from bathymetric_gnn_amd.data import FEATURE_CLASSES, S57Feature, feature_pixel_table
    assert list(FEATURE_CLASSES) == ["WRECKS", "UWTROC", "OBSTRN", "SBDARE", "SOUNDG"]
    assert [v["label"] for v in FEATURE_CLASSES.values()] == [1, 1, 1, None, None]
    assert [v["default_radius"] for v in FEATURE_CLASSES.values()] == [50, 25, 30, 0, 0]
    f = S57Feature("WRECKS", "Point", 3.5, -2.5, depth=12.0)
    assert f.to_dict() == {"object_class": "WRECKS", "geometry_type": "Point", "x": 3.5, "y": -2.5, "depth": 12.0, "attributes": None,
                           "wkt": None}
    local = {"A": {"label": 3, "default_radius": 2}, "B": {"label": 4, "default_radius": 1}, "C": {"label": None, "default_radius": 9}}
    feats = [S57Feature("A", "Point", 3.5, -2.5), S57Feature("C", "Point", 1, -1), S57Feature("B", "Point", 5.5, -6.5),
             S57Feature("Z", "Point", 0.5, -0.5)]
    table, applied = feature_pixel_table(feats, (0, 1, 0, 0, 0, -1), (10, 10), feature_classes=local)
    assert applied == 3 and table.tolist() == [[2, 3, 2, 3], [6, 5, 1, 4], [0, 0, 20, 1]]   # unknown: label 1, radius 30 clamped to 10 + 10


def test_empty_list_returns_none_with_the_reference_warning(caplog):
    from bathymetric_gnn_amd.data import create_feature_labels
    with caplog.at_level(logging.WARNING):
        assert create_feature_labels([], np.zeros((4, 4), np.float32), transform=(0, 1, 0, 0, 0, -1)) is None
    assert "No features to label" in caplog.text


# ---- the host plan ---------------------------------------------------------------------------------------------------------------
def _plan(table, shape):
    from bathymetric_gnn_amd.data import feature_plan
    return feature_plan(np.ascontiguousarray(table, dtype=np.int32).reshape(-1, 4), shape)


def _check_plan(table, shape, bin_ptr, bin_feat):
    """The properties every plan has: sizes, descending lists, no feature after one that holds the whole bin, and no feature
    whose bounding box misses the bin."""
    rows, cols = shape
    bins_r, bins_c = -(-rows // 64), -(-cols // 64)
    table = np.asarray(table, dtype=np.int64).reshape(-1, 4)
    assert bin_ptr.dtype == np.int64 and bin_feat.dtype == np.int32
    assert len(bin_ptr) == bins_r * bins_c + 1 and bin_ptr[0] == 0 and (np.diff(bin_ptr) >= 0).all() and bin_ptr[-1] == len(bin_feat)
    for b in range(bins_r * bins_c):
        lst = bin_feat[bin_ptr[b]:bin_ptr[b + 1]].astype(np.int64)
        assert (np.diff(lst) < 0).all(), "descending"
        r0, c0 = (b // bins_c) * 64, (b % bins_c) * 64
        r1, c1 = min(r0 + 64, rows) - 1, min(c0 + 64, cols) - 1
        row, col, rad = table[:, 0], table[:, 1], table[:, 2]
        meets = (rad >= 0) & (row + rad >= r0) & (row - rad <= r1) & (col + rad >= c0) & (col - rad <= c1)
        assert meets[lst].all(), "only features whose bounding box meets the bin"
        far = np.maximum(np.abs(row - r0), np.abs(row - r1)) ** 2 + np.maximum(np.abs(col - c0), np.abs(col - c1)) ** 2
        holds = (rad >= 0) & (far <= rad * rad)                          # the disc holds the bin's four corner cells
        assert not holds[lst[:-1]].any(), "cut at the first disc that holds the bin"
        if holds.any():
            top = int(np.flatnonzero(holds)[-1])
            assert len(lst) and lst[-1] == top, "the cut is the highest such feature"
        # nothing that could show is missing: every feature above the cut whose disc has a cell in the bin is listed
        near = np.clip(row, r0, r1), np.clip(col, c0, c1)
        touches = (rad >= 0) & ((row - near[0]) ** 2 + (col - near[1]) ** 2 <= rad * rad)
        floor = lst[-1] if len(lst) and holds[lst[-1]] else -1
        assert set(np.flatnonzero(touches & (np.arange(len(table)) >= floor))) <= set(lst.tolist())


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_plan_resolves_to_the_reference(case):
    from bathymetric_gnn_amd import runtime
    table, _ = _table(case)
    bin_ptr, bin_feat = _plan(table, case.depth.shape)
    _check_plan(table, case.depth.shape, bin_ptr, bin_feat)
    lib = runtime.load_library()
    tp = table.ctypes.data if len(table) else None
    assert lib.bgnn_feature_labels_plan_bytes(tp, len(table), *case.depth.shape) == 8 * len(bin_ptr) + 4 * len(bin_feat)
    valid = fc.valid_mask(case.depth)
    labels = fc.resolve_plan(table, bin_ptr, bin_feat, valid, np.where(valid, 0, -1).astype(np.int32))
    assert np.array_equal(labels, case.labels)


def test_plan_of_a_survey_sized_disc():
    """513 x 700 with a radius-200 disc, small discs under and over it in list order: the bins inside the big disc hold it alone
    or it and what lies above it; a bin no bounding box meets is empty."""
    rng = np.random.default_rng(5)
    shape = (513, 700)
    under = [[int(rng.integers(513)), int(rng.integers(700)), int(rng.integers(0, 12)), 3] for _ in range(150)]
    over = [[int(rng.integers(513)), int(rng.integers(700)), int(rng.integers(0, 12)), 4] for _ in range(150)]
    big = len(under)
    table = np.array(under + [[256, 300, 200, 1]] + over, dtype=np.int32)
    bin_ptr, bin_feat = _plan(table, shape)
    _check_plan(table, shape, bin_ptr, bin_feat)
    bins_c = 11
    inside = [r * bins_c + c for r in (3, 4) for c in (3, 4, 5)]                  # rows 192-319, columns 192-383: well inside
    for b in inside:
        lst = bin_feat[bin_ptr[b]:bin_ptr[b + 1]]
        assert lst[-1] == big and (lst[:-1] > big).all()
    only_big = np.array([[256, 300, 200, 1]], dtype=np.int32)
    bp, bf = _plan(only_big, shape)
    assert all(bp[b + 1] - bp[b] == 1 for b in inside) and bp[10 + 1] - bp[10] == 0 and bp[8 * bins_c + 1] - bp[8 * bins_c] == 0
    valid = np.ones(shape, bool)
    valid[100:140, 250:330] = False
    want = np.where(valid, 0, -1).astype(np.int32)
    fc.paint(table, valid, want)
    got = fc.resolve_plan(table, bin_ptr, bin_feat, valid, np.where(valid, 0, -1).astype(np.int32))
    assert np.array_equal(got, want) and {1, 3, 4} <= set(np.unique(want).tolist())


def test_plan_stays_small():
    """Near sum(bounding-box area) / bin area, never features x bins: 2000 discs of radius 0-40 on 1024 x 1024 (256 bins), and 300
    survey-sized discs, which close every bin they hold."""
    rng = np.random.default_rng(6)
    table = np.stack([rng.integers(0, 1024, 2000), rng.integers(0, 1024, 2000), rng.integers(0, 41, 2000), np.ones(2000)], 1).astype(np.int32)
    bin_ptr, bin_feat = _plan(table, (1024, 1024))
    _check_plan(table, (1024, 1024), bin_ptr, bin_feat)
    assert 2000 <= len(bin_feat) <= 4 * 2000
    table = np.stack([rng.integers(0, 1024, 300), rng.integers(0, 1024, 300), np.full(300, 2048), np.ones(300)], 1).astype(np.int32)
    bin_ptr, bin_feat = _plan(table, (1024, 1024))
    assert len(bin_feat) == 256 and (bin_feat == 299).all()
