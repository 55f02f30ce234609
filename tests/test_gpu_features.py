"""Feature labels on the device (bgnn_feature_labels, data/feature_labels.py) against the fixtures the reference's own
``create_feature_labels`` produced (tests/golden/features, make_golden_features.py): labels bit for bit and the three counts; list
order, long bin lists, truncated lists and ragged grids against the CPU oracle of _features_cpu (which test_host_features.py ties
to the same fixtures); overlay mode; and ``GroundTruth.with_features`` through ``TileStore`` into one training epoch."""
import logging
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import _features_cpu as fc

pytestmark = pytest.mark.gpu

CASES = fc.load_cases()
IDS = [c.name for c in CASES]
UNIT = (0.0, 1.0, 0.0, 0.0, 0.0, -1.0)                # 1 m cells: x = col, y = -row
LOCAL = {"A": {"label": 1, "default_radius": 6}, "B": {"label": 3, "default_radius": 9}, "C": {"label": 4, "default_radius": 4}}


def _stats(block):
    from bathymetric_gnn_amd import runtime
    b = np.frombuffer(block.cpu().numpy().tobytes(), dtype=np.dtype(runtime.FL_STATS_DTYPE))[0]
    return {"valid_cells": int(b["valid"]), "feature_cells": int(b["feature"]), "painted_cells": int(b["painted"])}


def _depth(rng, shape, holes=0.05):
    d = (-30.0 + rng.standard_normal(shape)).astype(np.float32)
    d[rng.random(shape) < holes] = np.float32(1.0e6)
    d[rng.random(shape) < holes / 2] = np.nan
    return d


def _run_depth(table, depth, dev):
    from bathymetric_gnn_amd.data import rasterize_features
    labels, block = rasterize_features(np.ascontiguousarray(table, dtype=np.int32).reshape(-1, 4), depth=torch.from_numpy(depth).to(dev))
    return labels.cpu().numpy(), _stats(block)


def _check_depth(table, depth, dev):
    got, stats = _run_depth(table, depth, dev)
    want, counts = fc.feature_labels(table, depth)
    assert got.dtype == np.int32 and np.array_equal(got, want)
    assert stats == counts
    return want


@pytest.mark.parametrize("on_device", [False, True], ids=["host_array", "device_tensor"])
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_fixture(case, on_device, gpu_device):
    from bathymetric_gnn_amd.data import BathymetricGrid, create_feature_labels
    depth = torch.from_numpy(case.depth).to(gpu_device) if on_device else case.depth
    grid = BathymetricGrid(depth=depth, transform=case.transform, crs="EPSG:32619")
    fl = create_feature_labels(case.features, grid, feature_radius=case.feature_radius, device=gpu_device)
    assert fl.labels.dtype == torch.int32 and fl.labels.device == gpu_device and tuple(fl.labels.shape) == case.depth.shape
    assert np.array_equal(fl.labels.cpu().numpy(), case.labels)
    assert fl.stats() == {k: case.meta[k] for k in ("applied_features", "feature_cells", "valid_cells", "painted_cells")}
    assert fl.applied_features == case.meta["applied_features"] and fl.transform == case.transform and fl.crs == "EPSG:32619"
    if on_device:
        assert fl.depth.data_ptr() == depth.data_ptr(), "a plane already on the device is not copied"
    bands = fl.bands()
    assert [b.dtype for b in bands] == [np.float32, np.float32]
    assert np.array_equal(bands[0], case.labels.astype(np.float32)) and np.array_equal(bands[1], case.band_depth, equal_nan=True)


def test_survey_forms_and_empty_list(gpu_device, caplog):
    """A host array and a device tensor with ``transform=`` give what the grid gives; an empty list returns None with the
    reference's warning."""
    from bathymetric_gnn_amd.data import create_feature_labels
    case = next(c for c in CASES if c.name == "heavy_overlap")
    a = create_feature_labels(case.features, case.depth, transform=case.transform, feature_radius=case.feature_radius, device=gpu_device)
    t = torch.from_numpy(case.depth).to(gpu_device)
    b = create_feature_labels(case.features, t, transform=case.transform, feature_radius=case.feature_radius)
    assert np.array_equal(a.labels.cpu().numpy(), case.labels) and torch.equal(a.labels, b.labels) and a.stats() == b.stats()
    assert b.depth.data_ptr() == t.data_ptr() and a.crs is None
    with pytest.raises(ValueError):
        create_feature_labels(case.features, case.depth, device=gpu_device)
    with caplog.at_level(logging.WARNING):
        assert create_feature_labels([], t, transform=case.transform) is None
    assert "No features to label" in caplog.text


def test_list_order_decides(gpu_device):
    """Overlapping discs of labels 1, 3 and 4 (a local class table): the later feature wins; the reversed list gives the other
    answer, and both are the oracle's."""
    from bathymetric_gnn_amd.data import feature_pixel_table
    rng = np.random.default_rng(11)
    shape = (70, 90)
    depth = _depth(rng, shape)
    feats = [SimpleNamespace(object_class="ABC"[k % 3], x=30 + 3.0 * k + 0.5, y=-(30 + 1.0 * k + 0.5)) for k in range(9)]
    table, applied = feature_pixel_table(feats, UNIT, shape, feature_classes=LOCAL)
    assert applied == 9 and sorted(set(table[:, 3].tolist())) == [1, 3, 4]
    fwd = _check_depth(table, depth, gpu_device)
    rev = _check_depth(table[::-1], depth, gpu_device)
    assert not np.array_equal(fwd, rev) and {1, 3, 4} <= set(np.unique(fwd).tolist())
    assert np.array_equal(fwd > 0, rev > 0)                      # the same cells are painted, with other labels


def test_a_bin_list_longer_than_one_chunk(gpu_device):
    """3000 features with centres inside a 40 x 40 patch of a 257 x 300 grid: the bins around the patch have lists of far more
    than the 256 entries the kernel stages at once."""
    from bathymetric_gnn_amd.data import feature_plan
    rng = np.random.default_rng(12)
    shape = (257, 300)
    n = 3000
    table = np.stack([rng.integers(50, 90, n), rng.integers(100, 140, n), rng.integers(0, 7, n), rng.choice([1, 3, 4], n)], 1).astype(np.int32)
    bin_ptr, _ = feature_plan(table, shape)
    assert np.diff(bin_ptr).max() > 4 * 256
    _check_depth(table, _depth(rng, shape), gpu_device)
    # ... and a list that is long because nothing decides early: every disc of radius 0 on its own cell of one bin
    rr, cc = np.meshgrid(np.arange(64, 104), np.arange(128, 168), indexing="ij")
    table = np.stack([rr.ravel(), cc.ravel(), np.zeros(1600), 1 + np.arange(1600) % 5], 1).astype(np.int32)
    want = _check_depth(table, np.full(shape, -20.0, np.float32), gpu_device)
    assert int((want > 0).sum()) == 1600


def test_random_discs_1024(gpu_device):
    """2000 random features, radii 0 to 40, on 1024 x 1024 (the 16-byte path: the width is a multiple of four)."""
    rng = np.random.default_rng(13)
    n = 2000
    table = np.stack([rng.integers(0, 1024, n), rng.integers(0, 1024, n), rng.integers(0, 41, n), rng.choice([1, 3, 4], n)], 1).astype(np.int32)
    _check_depth(table, _depth(rng, (1024, 1024)), gpu_device)


def test_truncated_lists_under_a_survey_sized_disc(gpu_device):
    """513 x 700 with a radius-200 disc and small discs under and over it in list order: inside the big disc the plan drops what
    lies under it, and the result must not notice."""
    rng = np.random.default_rng(14)
    shape = (513, 700)
    small = lambda n, label: [[int(rng.integers(513)), int(rng.integers(700)), int(rng.integers(0, 15)), label] for _ in range(n)]
    table = np.array(small(200, 3) + [[256, 300, 200, 1]] + small(200, 4), dtype=np.int32)
    want = _check_depth(table, _depth(rng, shape), gpu_device)
    assert {1, 3, 4} <= set(np.unique(want).tolist()) and not (want[200:300, 250:350] == 3).any()


@pytest.mark.parametrize("shape", [(63, 65), (64, 64), (65, 127), (130, 67), (1, 129), (129, 1), (128, 132)], ids=str)
def test_ragged_grids_and_bin_corners(shape, gpu_device):
    """Grids that are no multiple of the bin in either direction (and widths that are / are not multiples of four: both load
    paths), with discs centred on the bins' corner cells and on the grid's last row and column."""
    rng = np.random.default_rng(15)
    rows, cols = shape
    centres = [(r, c) for r in (0, 63, 64, 127, 128, rows - 1) for c in (0, 63, 64, 127, 128, cols - 1) if r < rows and c < cols]
    table = np.array([[r, c, int(rng.integers(0, 9)), int(rng.choice([1, 3, 4]))] for r, c in centres]
                     + [[rows // 2, cols // 2, rows + cols, 1]] + [[r, c, 2, 4] for r, c in centres[::3]], dtype=np.int32)
    _check_depth(table, _depth(rng, shape), gpu_device)
    _check_depth(table[:len(centres)], _depth(rng, shape, holes=0.0), gpu_device)
    _check_depth(np.zeros((0, 4), np.int32), _depth(rng, shape), gpu_device)          # no feature: validity alone


@pytest.mark.parametrize("cols", [280000, 280001])
def test_more_bins_than_workgroups(cols, gpu_device):
    """3 x 280000: 4375 bins, more than the 16 workgroups per CU of a launch (4096 on 256 CUs), so workgroups take a second bin
    and carry their counts across bins; discs in first and second bins alike, one across the whole width."""
    rng = np.random.default_rng(20)
    n = 600
    table = np.stack([rng.integers(0, 3, n), rng.integers(0, cols, n), rng.integers(0, 200, n), rng.choice([1, 3, 4], n)], 1).astype(np.int32)
    table[0] = (1, cols // 2, cols + 3, 3)
    table[-1] = (2, cols - 1, 70, 1)
    want = _check_depth(table, _depth(rng, (3, cols)), gpu_device)
    assert (want[:, 4096 * 64:] == 1).any() and (want[:, :4096 * 64] == 4).any()


def test_negative_radius_and_full_cover(gpu_device):
    depth = _depth(np.random.default_rng(16), (100, 140))
    table = np.array([[50, 70, -3, 3], [10, 10, 240, 4], [50, 70, -1, 1]], dtype=np.int32)
    want = _check_depth(table, depth, gpu_device)
    assert set(np.unique(want).tolist()) == {-1, 4}


def test_overlay_mode(gpu_device):
    """The base plane holds -1, 0 and 2: only zeros change, and the result equals the depth-mode labels wherever the base label
    is 0 (and the cell is valid there)."""
    from bathymetric_gnn_amd.data import rasterize_features
    rng = np.random.default_rng(17)
    shape = (150, 203)
    depth = _depth(rng, shape)
    valid = fc.valid_mask(depth)
    base = np.where(valid, np.where(rng.random(shape) < 0.15, 2, 0), -1).astype(np.int32)
    n = 120
    table = np.stack([rng.integers(0, 150, n), rng.integers(0, 203, n), rng.integers(0, 25, n), rng.choice([1, 3], n)], 1).astype(np.int32)
    t = torch.from_numpy(base).to(gpu_device)
    labels, block = rasterize_features(table, base_labels=t)
    got = labels.cpu().numpy()
    want, counts = fc.overlay_labels(table, base)
    assert np.array_equal(got, want) and _stats(block) == counts
    assert np.array_equal(got[base != 0], base[base != 0]) and torch.equal(t.cpu(), torch.from_numpy(base))
    by_depth, _ = _run_depth(table, depth, gpu_device)
    assert np.array_equal(got[base == 0], by_depth[base == 0]) and (got[base == 0] > 0).any() and (by_depth[base == 2] > 0).any()
    assert counts["valid_cells"] == int(valid.sum()) and counts["painted_cells"] < int((by_depth > 0).sum())
    with pytest.raises(ValueError):
        rasterize_features(table, depth=torch.from_numpy(depth).to(gpu_device), base_labels=t)
    with pytest.raises(ValueError):
        rasterize_features(table)
    with pytest.raises(TypeError):
        rasterize_features(table, depth=t)                                            # int32 where float32 is needed
    with pytest.raises(TypeError):
        rasterize_features(table, depth=torch.from_numpy(depth).to(gpu_device).t())   # not contiguous
    with pytest.raises(TypeError):
        rasterize_features(table.astype(np.int64), base_labels=t)


def test_two_calls_give_equal_bits(gpu_device):
    from bathymetric_gnn_amd.data import rasterize_features
    rng = np.random.default_rng(18)
    n = 1500
    table = np.stack([rng.integers(0, 300, n), rng.integers(0, 500, n), rng.integers(0, 30, n), rng.choice([1, 3, 4], n)], 1).astype(np.int32)
    depth = torch.from_numpy(_depth(rng, (300, 500))).to(gpu_device)
    runs = [rasterize_features(table, depth=depth) for _ in range(2)]
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1]) and runs[0][1][2].item() > 0


def test_an_empty_plane_launches_nothing(gpu_device):
    from bathymetric_gnn_amd.data import rasterize_features
    table = np.array([[0, 0, 3, 1]], dtype=np.int32)              # (not even looked at: it would be outside any 0-cell grid)
    for shape in ((0, 17), (5, 0), (0, 0)):
        labels, block = rasterize_features(table, depth=torch.empty(shape, dtype=torch.float32, device=gpu_device))
        assert tuple(labels.shape) == shape and labels.dtype == torch.int32 and block.tolist() == [0, 0, 0]


def test_ground_truth_with_features_reaches_the_loss(tmp_path, gpu_device):
    """A ground truth from a small synthetic pair, three discs over it, through ``TileStore.from_ground_truth``: the targets of
    ``batch`` hold class 1 exactly as often as the label plane does over the same boxes, and one epoch of a ``Trainer`` on the
    store gives finite losses."""
    from bathymetric_gnn_amd import synthetic
    from bathymetric_gnn_amd.config import Config
    from bathymetric_gnn_amd.data import BathymetricGrid, S57Feature, compute_ground_truth
    from bathymetric_gnn_amd.models import BathymetricGNN
    from bathymetric_gnn_amd.training import TileStore, Trainer
    rng = np.random.default_rng(19)
    h, w = 96, 128
    rr, cc = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    clean = (-25.0 + 0.03 * rr + 0.02 * cc + 0.02 * rng.standard_normal((h, w))).astype(np.float32)
    noisy = clean + (0.02 * rng.standard_normal((h, w))).astype(np.float32)
    spikes = rng.random((h, w)) < 0.04
    noisy[spikes] += rng.choice([-1.0, 1.0], int(spikes.sum())).astype(np.float32)
    noisy[10:14, 100:110] = np.float32(1.0e6)
    transform = (400000.0, 0.5, 0.0, 4.2e6, 0.0, -0.5)
    bounds = (400000.0, 4.2e6 - 0.5 * h, 400000.0 + 0.5 * w, 4.2e6)
    grids = [BathymetricGrid(depth=d, transform=transform, crs="EPSG:32619", resolution=(0.5, 0.5), bounds=bounds) for d in (clean, noisy)]
    gt = compute_ground_truth(*grids, 0.15, device=gpu_device)
    feats = [S57Feature("UWTROC", "Point", 400000.0 + 0.5 * 30.5, 4.2e6 - 0.5 * 40.5), S57Feature("WRECKS", "Point", 400000.0 + 0.5 * 100.5, 4.2e6 - 0.5 * 20.5),
             S57Feature("OBSTRN", "Point", 400000.0 + 0.5 * 70.5, 4.2e6 - 0.5 * 90.5), S57Feature("SOUNDG", "Point", 400000.0 + 5, 4.2e6 - 5)]
    gtf = gt.with_features(feats, {"UWTROC": 6, "WRECKS": 9, "OBSTRN": 5})
    base, labels = gt.labels.cpu().numpy(), gtf.labels.cpu().numpy()
    table = np.array([[40, 30, 12, 1], [20, 100, 18, 1], [90, 70, 10, 1]], dtype=np.int32)
    want, counts = fc.overlay_labels(table, base)
    assert np.array_equal(labels, want) and np.array_equal(labels[base != 0], base[base != 0]) and (base == 2).sum() > 100
    assert gtf.feature_stats() == dict(counts, applied_features=3) and counts["feature_cells"] > 500
    assert gtf.stats() == gt.stats() and "feature_cells" not in gtf.stats()
    for k in ("difference", "noisy_depth", "clean_depth"):
        assert getattr(gtf, k).data_ptr() == getattr(gt, k).data_ptr(), k
    assert gtf.labels.data_ptr() != gt.labels.data_ptr() and not (base == 1).any()
    with pytest.raises(ValueError):
        gt.feature_stats()

    store = TileStore.from_ground_truth(*gtf.training_planes(), resolution=(0.5, 0.5), tile_size=32, overlap=8, min_valid_ratio=0.1,
                                        device=gpu_device)
    count = sum(int((labels[r0:r1, c0:c1] == 1).sum()) for r0, c0, r1, c1 in store.boxes)
    assert count > 500 and store._class_counts[1] == count
    _, targets = store.batch(range(len(store)))
    y = targets["class_labels"]
    assert int((y == 1).sum().item()) == count and int((y == 2).sum().item()) == store._class_counts[2]

    sd = synthetic.synthetic_state_dict(in_channels=7, num_layers=2, seed=1, gnn_type="GAT")
    model = BathymetricGNN(in_channels=7, hidden_channels=64, num_gnn_layers=2, gnn_type="GAT", heads=4, dropout=0.1, edge_dim=3)
    model.load_state_dict({k: torch.as_tensor(v) for k, v in sd.items()})
    cfg = Config()
    cfg.training = {"batch_size": len(store), "epochs": 1, "scheduler": "cosine"}
    hist = Trainer(cfg, model.cuda(), store, None, output_dir=tmp_path, seed=3).train()
    assert len(hist["train_loss"]) == 1 and np.isfinite(hist["train_loss"][0]) and np.isfinite(hist["train_acc"][0])
