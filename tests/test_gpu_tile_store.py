"""Training tiles cut from planes in HBM (include/bgnn_tilestore.h, ``TileStore.from_ground_truths`` / ``from_survey``) against the
paths the package already has: numpy counts, ``plan_ground_truth_tiles``, ``TileStore.from_ground_truth`` on host arrays and
``TileStore.from_grid``.  Everything here is an equality of integers or of bits; no tolerance appears.  Tiles are 32 x 32 with an
overlap of 8 unless a test says otherwise."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

TILE, OVERLAP = 32, 8
PLANES = ("depth", "mask", "unc", "labels", "difference")


# ---- inputs -----------------------------------------------------------------------------------------------------------------
def _labels(rng, shape, low=-1, holes=5):
    lab = rng.integers(low, 4, size=shape).astype(np.int32)
    for _ in range(holes):
        r, c = rng.integers(0, shape[0]), rng.integers(0, shape[1])
        lab[r:r + rng.integers(10, 70), c:c + rng.integers(10, 70)] = -1
    return lab


def _raster(seed, shape, unc=False, res=(1.0, 1.0)):
    """Host planes of a ground-truth raster: labels -1 .. 3 with rectangles of no data, a difference plane that is NaN (with
    several payloads and both signs) where there is no label, a depth plane, an uncertainty plane or None."""
    rng = np.random.default_rng(seed)
    lab = _labels(rng, shape)
    diff = rng.standard_normal(shape).astype(np.float32)
    bits = diff.view(np.uint32)
    bits[lab < 0] = rng.choice(np.array([0x7FC00000, 0x7FC12345, 0xFFC00001, 0x7F800001], np.uint32), int((lab < 0).sum()))
    depth = (-30 + 3 * rng.standard_normal(shape)).astype(np.float32)
    depth[lab < 0] = np.float32(1.0e6)
    u = rng.random(shape).astype(np.float32) if unc else None
    return lab, diff, depth, u, res


def _on_device(raster, dev):
    return tuple(torch.from_numpy(p).to(dev) if isinstance(p, np.ndarray) else p for p in raster)


def _host_store(raster, dev, ratio=0.1, tile=TILE, overlap=OVERLAP):
    from bathymetric_gnn_amd.training import TileStore
    lab, diff, depth, u, res = raster
    return TileStore.from_ground_truth(lab, diff, depth, u, resolution=res, tile_size=tile, overlap=overlap, min_valid_ratio=ratio, device=dev)


def _bits(t):
    return t.view(torch.int32) if t.dtype == torch.float32 else t


def _assert_planes_equal(store, want):
    """``want``: per plane name, the list of flat tensors whose concatenation the store's plane must equal as bits."""
    for k in PLANES:
        got = getattr(store, k)
        if want[k][0] is None:
            assert got is None, k
            continue
        ref = torch.cat(want[k])
        assert got.dtype == ref.dtype and got.device == ref.device and got.shape == ref.shape, k
        assert torch.equal(_bits(got), _bits(ref)), k


def _assert_node_counts(store):
    """``node_counts``: the valid cells of every tile, as the store's own mask holds them; host int64."""
    csum = np.concatenate([[0], np.cumsum(store.mask.cpu().numpy().astype(np.int64))])
    assert isinstance(store.node_counts, np.ndarray) and store.node_counts.dtype == np.int64
    assert np.array_equal(store.node_counts, csum[store.offsets[1:]] - csum[store.offsets[:-1]])


def _assert_store_is(store, hosts):
    """``store`` is the concatenation of the host-built stores ``hosts``."""
    assert len(store) == sum(len(h) for h in hosts)
    for s in [store] + list(hosts):
        _assert_node_counts(s)
    assert np.array_equal(store.hw, np.concatenate([h.hw for h in hosts])) and store.hw.dtype == np.int32
    assert np.array_equal(store.res, np.concatenate([h.res for h in hosts])) and store.res.dtype == np.float64
    cells = np.concatenate([[0]] + [np.diff(h.offsets) for h in hosts]).cumsum()
    assert np.array_equal(store.offsets, cells)
    assert store.boxes == [b for h in hosts for b in h.boxes]
    assert store._class_counts == {c: sum(h._class_counts[c] for h in hosts) for c in (0, 1, 2)}
    assert store.uniform == all(h.uniform for h in hosts) and store.kind == "ground_truth"
    _assert_planes_equal(store, {k: [getattr(h, k) for h in hosts] for k in PLANES})


def _numpy_counts(lab, boxes):
    return np.array([[(lab[r0:r1, c0:c1] >= 0).sum()] + [(lab[r0:r1, c0:c1] == c).sum() for c in (0, 1, 2)] for r0, c0, r1, c1 in boxes],
                    dtype=np.int64).reshape(-1, 4)


# ---- 3. the scan ------------------------------------------------------------------------------------------------------------
def test_scan_counts_equal_numpy(gpu_device):
    from bathymetric_gnn_amd.training import plan_tile_boxes, scan_tile_boxes
    rng = np.random.default_rng(1)
    lab = _labels(rng, (150, 131), low=-2)
    assert set(np.unique(lab)) == {-2, -1, 0, 1, 2, 3}
    boxes = plan_tile_boxes(150, 131, TILE, OVERLAP)
    assert boxes[-1] == (118, 99, 150, 131) and len(boxes) == 26
    counts = scan_tile_boxes(torch.from_numpy(lab).to(gpu_device), boxes)
    assert counts.dtype == torch.int64 and counts.shape == (26, 4) and counts.device == gpu_device
    want = _numpy_counts(lab, boxes)
    assert np.array_equal(counts.cpu().numpy(), want)
    assert want[:, 0].min() < 512 < want[:, 0].max() and (want[:, 1:].sum(1) < want[:, 0]).any()    # class 3 is valid, of no class


def test_scan_depth_mode(gpu_device):
    from bathymetric_gnn_amd.training import plan_tile_boxes, scan_tile_boxes
    rng = np.random.default_rng(2)
    depth = (-20 + rng.standard_normal((150, 131))).astype(np.float32)
    for value in (np.nan, np.inf, -np.inf, 1.0e6, -0.0):
        depth[rng.random(depth.shape) < 0.07] = np.float32(value)
    depth[40:90, 30:100] = np.float32(1.0e6)
    depth[100:140, 0:50] = np.nan
    boxes = plan_tile_boxes(150, 131, TILE, OVERLAP)
    plane = torch.from_numpy(depth).to(gpu_device)
    for nodata, valid in ((1.0e6, np.isfinite(depth) & (depth != np.float32(1.0e6))), (float("nan"), np.isfinite(depth)),
                          (None, np.isfinite(depth)), (0.0, np.isfinite(depth) & (depth != 0))):      # (0.0 == -0.0)
        want = np.array([[valid[r0:r1, c0:c1].sum(), 0, 0, 0] for r0, c0, r1, c1 in boxes], np.int64)
        got = scan_tile_boxes(plane, boxes, nodata=nodata).cpu().numpy()
        assert np.array_equal(got, want), nodata
        assert want[:, 0].min() < 512 < want[:, 0].max()


@pytest.mark.parametrize("shape,boxes", [
    ((150, 131), [(3, 5, 150, 131), (0, 0, 150, 131), (149, 130, 150, 131), (7, 1, 40, 66), (31, 0, 96, 65), (0, 2, 33, 131)]),
    ((37, 1203), [(0, 0, 37, 1203), (1, 3, 36, 260), (5, 946, 6, 1203), (0, 500, 37, 757), (2, 1, 35, 1026)]),
])
def test_scan_and_cut_boxes_of_any_extent(gpu_device, shape, boxes):
    """Boxes of one row, of more than one band of 32 rows, narrower than a wave, wider than one step of 256 cells, at odd
    columns, overlapping, flush with the far edges: counts and cut tiles against numpy slices."""
    from bathymetric_gnn_amd.training import cut_tile_boxes, scan_tile_boxes
    rng = np.random.default_rng(4)
    lab = _labels(rng, shape)
    f = rng.standard_normal(shape).astype(np.float32)
    f[lab < 0] = np.nan
    d_lab, d_f = torch.from_numpy(lab).to(gpu_device), torch.from_numpy(f).to(gpu_device)
    assert np.array_equal(scan_tile_boxes(d_lab, boxes).cpu().numpy(), _numpy_counts(lab, boxes))
    sizes = [(r1 - r0) * (c1 - c0) for r0, c0, r1, c1 in boxes]
    offsets = np.concatenate([[0], np.cumsum(sizes)])
    cells = int(offsets[-1])
    guard = 64
    s_lab = torch.full((cells + guard,), -77, dtype=torch.int32, device=gpu_device)
    s_f = torch.full((cells + guard,), 5.0, dtype=torch.float32, device=gpu_device)
    mask = torch.full((cells + guard,), 9, dtype=torch.uint8, device=gpu_device)
    cut_tile_boxes([d_lab, None, d_f], [s_lab, None, s_f], boxes, offsets[:-1], mask=mask, mask_plane=0)
    want_lab = np.concatenate([lab[r0:r1, c0:c1].ravel() for r0, c0, r1, c1 in boxes])
    want_f = np.concatenate([f[r0:r1, c0:c1].ravel() for r0, c0, r1, c1 in boxes])
    assert np.array_equal(s_lab[:cells].cpu().numpy(), want_lab)
    assert np.array_equal(s_f[:cells].cpu().numpy().view(np.int32), want_f.view(np.int32))
    assert np.array_equal(mask[:cells].cpu().numpy(), (want_lab >= 0).astype(np.uint8))
    # nothing is written past the last tile
    assert (s_lab[cells:] == -77).all() and (s_f[cells:] == 5.0).all() and (mask[cells:] == 9).all()
    # the mask from the float plane, and no mask at all
    mask2 = torch.full((cells,), 9, dtype=torch.uint8, device=gpu_device)
    s_f2 = torch.empty(cells, dtype=torch.float32, device=gpu_device)
    cut_tile_boxes([d_f], [s_f2], boxes, offsets[:-1], mask=mask2, mask_plane=0, nodata=None)
    assert np.array_equal(mask2.cpu().numpy(), np.isfinite(want_f).astype(np.uint8)) and torch.equal(_bits(s_f2), _bits(s_f[:cells]))
    s_f3 = torch.empty(cells, dtype=torch.float32, device=gpu_device)
    cut_tile_boxes([d_f], [s_f3], boxes, offsets[:-1])
    assert torch.equal(_bits(s_f3), _bits(s_f2))


# ---- 4. the threshold edge --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ratio,kept,dropped", [(0.125, 128, 127), (0.1, 103, 102)])
def test_keep_rule_at_the_line(gpu_device, ratio, kept, dropped):
    """32 x 56 at tile 32 / stride 24: the tiles (0, 0) and (0, 24), which share the columns 24 .. 31.  The first holds ``kept``
    labelled cells in its own columns, the second ``dropped`` in its own; nothing else is labelled."""
    from bathymetric_gnn_amd.training import TileStore, plan_ground_truth_tiles
    lab = np.full((32, 56), -1, np.int32)
    own_a = [(r, c) for r in range(32) for c in range(20)][:kept]
    own_b = [(r, c) for r in range(32) for c in range(34, 56)][:dropped]
    for k, (r, c) in enumerate(own_a + own_b):
        lab[r, c] = (0, 2, 1)[k % 3]
    assert (lab[:, 0:32] >= 0).sum() == kept and (lab[:, 24:56] >= 0).sum() == dropped
    f = np.arange(lab.size, dtype=np.float32).reshape(lab.shape)
    want_boxes, want_counts = plan_ground_truth_tiles(lab, TILE, OVERLAP, ratio)
    assert want_boxes == [(0, 0, 32, 32)]
    store = TileStore.from_ground_truths([_on_device((lab, f, f, None, (1.0, 1.0)), gpu_device)], TILE, OVERLAP, ratio, device=gpu_device)
    assert store.boxes == want_boxes and store._class_counts == want_counts and len(store) == 1
    _assert_store_is(store, [_host_store((lab, f, f, None, (1.0, 1.0)), gpu_device, ratio)])


# ---- 5. one raster ----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def survey_pair():
    rng = np.random.default_rng(19)
    h, w = 96, 128
    rr, cc = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    clean = (-25.0 + 0.03 * rr + 0.02 * cc + 0.02 * rng.standard_normal((h, w))).astype(np.float32)
    noisy = clean + (0.02 * rng.standard_normal((h, w))).astype(np.float32)
    spikes = rng.random((h, w)) < 0.04
    noisy[spikes] += rng.choice([-1.0, 1.0], int(spikes.sum())).astype(np.float32)
    noisy[10:14, 100:110] = np.float32(1.0e6)
    noisy[50:96, 0:40] = np.nan                                # enough missing cells to drop tiles
    return clean, noisy, rng.random((h, w)).astype(np.float32)


@pytest.mark.parametrize("with_unc", [False, True])
def test_single_raster_equals_from_ground_truth(gpu_device, survey_pair, with_unc):
    from bathymetric_gnn_amd.data import BathymetricGrid, S57Feature, compute_ground_truth
    from bathymetric_gnn_amd.training import TileStore
    clean, noisy, unc = survey_pair
    h, w = clean.shape
    transform = (400000.0, 0.5, 0.0, 4.2e6, 0.0, -0.5)
    bounds = (400000.0, 4.2e6 - 0.5 * h, 400000.0 + 0.5 * w, 4.2e6)
    grids = [BathymetricGrid(depth=d, uncertainty=unc if with_unc else None, transform=transform, crs="EPSG:32619", resolution=(0.5, 0.5),
                             bounds=bounds) for d in (clean, noisy)]
    gt = compute_ground_truth(*grids, 0.15, device=gpu_device)
    feats = [S57Feature("UWTROC", "Point", 400000.0 + 0.5 * 30.5, 4.2e6 - 0.5 * 40.5), S57Feature("WRECKS", "Point", 400000.0 + 0.5 * 100.5, 4.2e6 - 0.5 * 20.5)]
    gtf = gt.with_features(feats, {"UWTROC": 6, "WRECKS": 9})
    for truth in (gt, gtf):
        assert (truth.uncertainty is not None) == with_unc
        store = TileStore.from_ground_truths([truth], TILE, OVERLAP, 0.1, device=gpu_device)
        host = TileStore.from_ground_truth(*(None if t is None else t.cpu().numpy() for t in truth.training_planes()), resolution=(0.5, 0.5),
                                           tile_size=TILE, overlap=OVERLAP, min_valid_ratio=0.1, device=gpu_device)
        _assert_store_is(store, [host])
        assert np.array_equal(store.res, np.full((len(store), 2), 0.5)) and np.array_equal(store.sources, np.zeros(len(store), np.int32))
        assert 5 < len(store) < 16 and (96 - 32, 128 - 32, 96, 128) in store.boxes         # (16 candidates: some are dropped)
        assert store.in_channels == host.in_channels and torch.isnan(store.difference).any()
    assert store._class_counts[1] > 100                                   # (the painted truth came last)
    # a truth without a transform is cut at (1.0, 1.0)
    import dataclasses
    plain = TileStore.from_ground_truths([dataclasses.replace(gt, transform=None)], TILE, OVERLAP, 0.1, device=gpu_device)
    assert np.array_equal(plain.res, np.ones((len(plain), 2)))


# ---- 6. several rasters -----------------------------------------------------------------------------------------------------
def test_three_rasters_in_one_store(gpu_device, caplog):
    from bathymetric_gnn_amd.training import TileStore
    rasters = [_raster(11, (150, 131), True, (0.5, 0.5)), _raster(12, (64, 200), True, (1.0, 2.0)), _raster(13, (40, 40), True, (1.0, 1.0))]
    empty = _raster(14, (90, 70), True, (3.0, 3.0))
    empty[0][:] = -1
    small = _raster(15, (20, 100), True, (4.0, 4.0))
    hosts = [_host_store(r, gpu_device) for r in rasters]
    for r in (empty, small):
        with pytest.raises(ValueError, match="yields no tile"):
            _host_store(r, gpu_device)
    with caplog.at_level("WARNING"):
        store = TileStore.from_ground_truths([_on_device(r, gpu_device) for r in rasters + [empty, small]], TILE, OVERLAP, 0.1, device=gpu_device)
    assert sum("yields no tile" in rec.getMessage() for rec in caplog.records) == 2
    _assert_store_is(store, hosts)
    n = [len(h) for h in hosts]
    assert n[0] > 10 and n[1] > 5 and n[2] == 2 and store.uniform
    assert store.sources.dtype == np.int32 and store.sources.tolist() == [0] * n[0] + [1] * n[1] + [2] * n[2]
    assert sorted(set(map(tuple, store.res.tolist()))) == [(0.5, 0.5), (1.0, 1.0), (1.0, 2.0)]
    # the same rasters with the skipped ones in between, as host arrays: the raster index counts them
    mixed = TileStore.from_ground_truths([rasters[0], empty, rasters[1], small, rasters[2]], TILE, OVERLAP, 0.1, device=gpu_device)
    _assert_store_is(mixed, hosts)
    assert mixed.sources.tolist() == [0] * n[0] + [2] * n[1] + [4] * n[2]

    # a batch across the rasters: the first tile, the last, one of the middle raster
    picks = [(0, 0), (2, n[2] - 1), (1, n[1] // 2)]
    index = [sum(n[:k]) + i for k, i in picks]
    graph, targets = store.batch(index)
    parts = [hosts[k].batch([i]) for k, i in picks]
    assert graph.num_nodes == sum(g.num_nodes for g, _ in parts) > 0
    assert torch.equal(graph.x, torch.cat([g.x for g, _ in parts]))
    assert torch.equal(graph.edge_attr, torch.cat([g.edge_attr for g, _ in parts]))
    for key in ("class_labels", "correction_targets", "noise_mask"):
        assert torch.equal(targets[key], torch.cat([t[key] for _, t in parts])), key


# ---- 7. a survey ------------------------------------------------------------------------------------------------------------
def _survey(shape, seed=5):
    rng = np.random.default_rng(seed)
    depth = (-40 + 2 * rng.standard_normal(shape)).astype(np.float32)
    for value in (np.nan, np.inf, -np.inf, 1.0e6):
        depth[rng.random(shape) < 0.02] = np.float32(value)
    return depth, rng.random(shape).astype(np.float32)


def _assert_survey_store_is(store, ref):
    assert store.kind == ref.kind == "synthetic" and len(store) == len(ref)
    assert np.array_equal(store.hw, ref.hw) and store.hw.dtype == ref.hw.dtype
    assert np.array_equal(store.res, ref.res) and np.array_equal(store.offsets, ref.offsets) and store.uniform == ref.uniform
    _assert_planes_equal(store, {k: [getattr(ref, k)] for k in PLANES})
    _assert_node_counts(store); _assert_node_counts(ref)


@pytest.mark.parametrize("with_unc", [False, True])
@pytest.mark.parametrize("nodata", [1.0e6, None])
@pytest.mark.parametrize("shape", [(70, 100), (20, 100)])
def test_from_survey_equals_from_grid(gpu_device, shape, nodata, with_unc):
    """``upload_tiles`` stores each tile's depth as it is (invalid cells keep their value: sentinel, NaN, infinities), the crop of
    the grid's valid mask, and the uncertainty as it is: so must ``from_survey``."""
    from bathymetric_gnn_amd.data import BathymetricGrid, TileManager
    from bathymetric_gnn_amd.training import TileStore
    depth, unc = _survey(shape)
    unc = unc if with_unc else None
    tm = TileManager(TILE, OVERLAP, min_valid_ratio=0.5)
    kw = dict(nodata_value=nodata, resolution=(0.5, 2.0), device=gpu_device)
    ref = TileStore.from_grid(BathymetricGrid(depth, unc, nodata, resolution=(0.5, 2.0)), tm, device=gpu_device)
    store = TileStore.from_survey(torch.from_numpy(depth).to(gpu_device), tm, None if unc is None else torch.from_numpy(unc).to(gpu_device), **kw)
    _assert_survey_store_is(store, ref)
    specs = tm.compute_tile_grid(shape)[2]
    assert len(store) == len(specs) and store.boxes == [(s.row_start, s.col_start, s.row_end, s.col_end) for s in specs]
    if shape == (70, 100):
        assert store.uniform and (38, 68, 70, 100) in store.boxes
    else:
        assert store.hw.tolist() == [[20, 32]] * 4 and store.boxes[-1] == (0, 68, 20, 100)
    host = TileStore.from_survey(depth, tm, unc, **kw)                         # host arrays are uploaded
    _assert_survey_store_is(host, ref)


@pytest.mark.parametrize("nodata", [1.0e6, None])
def test_from_survey_drops_tiles_at_the_strict_line(gpu_device, nodata):
    """70 x 100, tile 32 / overlap 8, min_valid_ratio 0.25.  A block without data leaves the tile (0, 0) exactly 256 valid cells
    of 1024 (0.25 is not < 0.25: kept), the tile (0, 24) 64 and the tile (0, 48) none (both dropped).  One more missing cell
    takes the first tile below the line."""
    from bathymetric_gnn_amd.data import BathymetricGrid, TileManager
    from bathymetric_gnn_amd.training import TileStore
    depth, unc = _survey((70, 100), seed=6)
    depth[:] = np.where(np.isfinite(depth) & (depth != np.float32(1.0e6)), depth, np.float32(-40.0))
    hole = np.float32(np.nan) if nodata is None else np.float32(nodata)
    depth[0:32, 0:80] = hole
    depth[0:8, 0:32] = np.float32(-41.5)
    tm = TileManager(TILE, OVERLAP, min_valid_ratio=0.25)
    for missing, first_kept in ((None, True), ((0, 0), False)):
        d = depth.copy()
        if missing is not None:
            d[missing] = hole
        grid = BathymetricGrid(d, unc, nodata, resolution=(1.0, 1.0))
        assert int(grid.valid_mask[0:32, 0:32].sum()) == (256 if first_kept else 255)
        ref = TileStore.from_grid(grid, tm, device=gpu_device)
        store = TileStore.from_survey(torch.from_numpy(d).to(gpu_device), tm, torch.from_numpy(unc).to(gpu_device), nodata_value=nodata,
                                      device=gpu_device)
        _assert_survey_store_is(store, ref)
        assert ((0, 0, 32, 32) in store.boxes) == first_kept
        assert (0, 24, 32, 56) not in store.boxes and (0, 48, 32, 80) not in store.boxes and (0, 68, 32, 100) in store.boxes
        assert len(store) == 12 - 2 - (0 if first_kept else 1)
    with pytest.raises(ValueError, match="at least one tile"):
        TileStore.from_survey(torch.full((70, 100), float("nan"), device=gpu_device), tm, device=gpu_device)


# ---- 8. refusals ------------------------------------------------------------------------------------------------------------
def test_constructor_refusals(gpu_device):
    from bathymetric_gnn_amd.training import TileStore
    a, b = _raster(21, (64, 64), True), _raster(22, (64, 64), False)
    with pytest.raises(ValueError, match="uncertainty"):
        TileStore.from_ground_truths([_on_device(a, gpu_device), _on_device(b, gpu_device)], TILE, OVERLAP, device=gpu_device)
    empty = _raster(23, (64, 64))
    empty[0][:] = -1
    with pytest.raises(ValueError, match="yield no tile"):
        TileStore.from_ground_truths([_on_device(empty, gpu_device), _on_device(_raster(24, (20, 100)), gpu_device)], TILE, OVERLAP, device=gpu_device)
    with pytest.raises(ValueError, match="yield no tile"):
        TileStore.from_ground_truths([], TILE, OVERLAP, device=gpu_device)
    lab, diff, depth, u, res = _on_device(b, gpu_device)
    with pytest.raises(ValueError, match="shape"):
        TileStore.from_ground_truths([(lab, diff[:, :60].contiguous(), depth, None, res)], TILE, OVERLAP, device=gpu_device)
    with pytest.raises(ValueError, match="shape"):
        TileStore.from_ground_truths([(lab, diff, depth, depth[:60].contiguous(), res)], TILE, OVERLAP, device=gpu_device)
    with pytest.raises(TypeError):
        TileStore.from_ground_truths([(lab, diff.cpu().numpy(), depth, None, res)], TILE, OVERLAP, device=gpu_device)
    with pytest.raises(ValueError, match="Tile size must be larger than overlap"):
        TileStore.from_ground_truths([(lab, diff, depth, None, res)], 32, 32, device=gpu_device)
    from bathymetric_gnn_amd.data import TileManager
    with pytest.raises(ValueError, match="shape"):
        TileStore.from_survey(depth, TileManager(TILE, OVERLAP), uncertainty=depth[:, :50].contiguous(), device=gpu_device)


def test_c_level_refusals_launch_nothing(gpu_device):
    from bathymetric_gnn_amd import runtime as rt
    ctx = rt.get_context(gpu_device)
    lib = ctx.lib
    plane = torch.zeros((10, 10), dtype=torch.int32, device=gpu_device)
    counts = torch.full((2, 4), -5, dtype=torch.int64, device=gpu_device)
    store = torch.full((64,), -5, dtype=torch.int32, device=gpu_device)
    mask = torch.full((64,), 7, dtype=torch.uint8, device=gpu_device)
    ws = torch.zeros(64, dtype=torch.int64, device=gpu_device)
    box = lambda *rows: np.array(list(rows), dtype=rt.TILE_BOX_DTYPE)
    ptr = lambda t: None if t is None else C.c_void_p(t.ctypes.data if isinstance(t, np.ndarray) else t.data_ptr())

    def scan(boxes, n, plane=plane, ws=ws, counts=counts, handle=ctx.handle):
        return lib.bgnn_tile_scan(handle, ptr(plane), 10, 10, rt.TILE_VALID_LABEL, 0.0, ptr(boxes), n, ptr(ws), 512, ptr(counts))

    def cut(boxes, n, planes=(plane,), dst=(store,), handle=ctx.handle, ws=ws):
        src = None if planes is None else (C.c_void_p * len(planes))(*[None if p is None else p.data_ptr() for p in planes])
        out = None if dst is None else (C.c_void_p * len(dst))(*[None if p is None else p.data_ptr() for p in dst])
        return lib.bgnn_tile_cut(handle, src, out, 1, 10, 10, ptr(mask), 0, rt.TILE_VALID_LABEL, 0.0, ptr(boxes), n, 64, ptr(ws), 512)

    good = box((0, 0, 4, 4, 0))
    ctx.begin()
    for kw in (dict(handle=None), dict(plane=None), dict(ws=None), dict(counts=None)):
        assert scan(good, 1, **kw) == rt.ERR_INVALID and b"NULL" in lib.bgnn_last_error(), kw
    assert scan(None, 1) == rt.ERR_INVALID and b"NULL" in lib.bgnn_last_error()
    for kw in (dict(handle=None), dict(planes=None), dict(dst=None), dict(ws=None)):
        assert cut(good, 1, **kw) == rt.ERR_INVALID and b"NULL" in lib.bgnn_last_error(), kw
    assert cut(None, 1) == rt.ERR_INVALID and b"NULL" in lib.bgnn_last_error()
    for bad, why in ((box((0, 0, 0, 4, 0)), b"is empty"), (box((8, 0, 4, 4, 0)), b"leaves the plane"), (box((0, 7, 4, 4, 0)), b"leaves the plane"),
                     (box((0, 0, 4, 4, 0), (0, 0, 11, 1, 16)), b"leaves the plane")):
        assert scan(bad, len(bad)) == rt.ERR_INVALID and why in lib.bgnn_last_error()
        assert cut(bad, len(bad)) == rt.ERR_INVALID and why in lib.bgnn_last_error()
    assert cut(box((0, 0, 8, 8, 1)), 1) == rt.ERR_INVALID and b"past the store" in lib.bgnn_last_error()
    assert cut(good, 1, dst=(plane,)) == rt.ERR_INVALID and b"overlaps" in lib.bgnn_last_error()
    with pytest.raises(ValueError, match="leaves the plane"):
        rt.check(scan(box((8, 0, 4, 4, 0)), 1))
    # no boxes: BGNN_OK, nothing written
    assert scan(good, 0) == 0 and scan(None, 0, ws=None, counts=None) == 0 and cut(good, 0) == 0 and cut(None, 0, ws=None) == 0
    ctx.end()
    torch.cuda.synchronize()
    assert (counts == -5).all() and (store == -5).all() and (mask == 7).all() and (ws == 0).all()
    # and the same calls with good arguments do write
    ctx.begin()
    assert scan(good, 1) == 0 and cut(good, 1) == 0
    ctx.end()
    torch.cuda.synchronize()
    assert counts[0].tolist() == [16, 16, 0, 0] and (counts[1] == -5).all()
    assert (store[:16] == 0).all() and (store[16:] == -5).all() and (mask[:16] == 1).all() and (mask[16:] == 7).all()
    from bathymetric_gnn_amd.training import scan_tile_boxes
    assert scan_tile_boxes(plane, []).shape == (0, 4)


# ---- 9. past 2^31 cells -----------------------------------------------------------------------------------------------------
def test_plane_past_two_to_the_31_cells(gpu_device):
    """46400 x 46400 = 2.153e9 cells: the far-corner patch lies past cell 2^31, where 32-bit cell arithmetic would wrap.  The
    plane is -1 except a 600 x 600 patch of zeros and twos in the far corner; one float plane with a ramp in that patch serves as
    difference and depth.  Reference: ``from_ground_truth`` on the host, on the crop from 45248 on (101 strides of 448: the
    crop's stride grid is the plane's)."""
    from bathymetric_gnn_amd.training import TileStore, plan_tile_boxes
    free, _ = torch.cuda.mem_get_info(gpu_device)
    if free < 24 * 10 ** 9:
        pytest.skip(f"two 46400 x 46400 planes take 17.2 GB; only {free / 1e9:.1f} GB of device memory are free (24 GB wanted)")
    side, patch, origin = 46400, 600, 45248
    assert origin % 448 == 0 and (side - 512) * side < 2 ** 31 < (side - 1) * side      # the corner tile straddles cell 2^31
    rng = np.random.default_rng(9)
    lab_patch = rng.choice(np.array([0, 2], np.int32), size=(patch, patch), p=(0.8, 0.2)).astype(np.int32)
    ramp = (np.arange(patch * patch, dtype=np.float32).reshape(patch, patch) * np.float32(0.25) - np.float32(7.0))
    labels = torch.full((side, side), -1, dtype=torch.int32, device=gpu_device)
    plane = torch.zeros((side, side), dtype=torch.float32, device=gpu_device)
    labels[side - patch:, side - patch:] = torch.from_numpy(lab_patch).to(gpu_device)
    plane[side - patch:, side - patch:] = torch.from_numpy(ramp).to(gpu_device)
    store = TileStore.from_ground_truths([(labels, plane, plane, None, (1.0, 1.0))], 512, 64, 0.1, device=gpu_device)
    crop_lab = labels[origin:, origin:].cpu().numpy()
    crop_f = plane[origin:, origin:].cpu().numpy()
    del labels, plane
    assert np.array_equal(crop_lab[-patch:, -patch:], lab_patch) and (crop_lab[:-patch] == -1).all() and (crop_lab[:, :-patch] == -1).all()
    host = TileStore.from_ground_truth(crop_lab, crop_f, crop_f, None, tile_size=512, overlap=64, min_valid_ratio=0.1, device=gpu_device)
    assert host.boxes == [(448, 448, 960, 960), (640, 640, 1152, 1152)]
    host.boxes = [(r0 + origin, c0 + origin, r1 + origin, c1 + origin) for r0, c0, r1, c1 in host.boxes]
    assert host.boxes[-1] == (side - 512, side - 512, side, side) and len(plan_tile_boxes(side, side, 512, 64)) == 103 * 103 + 1
    _assert_store_is(store, [host])
    assert store._class_counts[0] > 0 and store._class_counts[2] > 0 and store._class_counts[1] == 0


# ---- 10. determinism, stream order ------------------------------------------------------------------------------------------
def test_equal_bits_on_every_run_and_behind_pending_work(gpu_device):
    from bathymetric_gnn_amd.training import TileStore
    raster = _raster(31, (150, 131), True, (0.5, 0.5))
    dev = _on_device(raster, gpu_device)
    host = _host_store(raster, gpu_device)
    first = TileStore.from_ground_truths([dev], TILE, OVERLAP, 0.1, device=gpu_device)
    second = TileStore.from_ground_truths([dev], TILE, OVERLAP, 0.1, device=gpu_device)
    _assert_store_is(first, [host])
    _assert_store_is(second, [host])
    # the planes are the results of work that is still queued on the caller's stream when the store is built
    torch.cuda.synchronize()
    m = torch.randn(4096, 4096, device=gpu_device)
    for _ in range(20):
        m = torch.tanh(m @ m * 1e-3)
    zero = (m[0, 0] * 0).to(torch.int32)                       # (finite: tanh keeps the chain bounded)
    later = lambda t: (t.view(torch.int32) + zero).view(t.dtype)   # (an integer add: a float one would quieten the signalling NaNs)
    pending = (later(dev[0]), later(dev[1]), later(dev[2]), later(dev[3]), dev[4])
    third = TileStore.from_ground_truths([pending], TILE, OVERLAP, 0.1, device=gpu_device)
    _assert_store_is(third, [host])
