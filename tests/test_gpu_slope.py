"""Slope-based feature labels on the device (include/bgnn_slope.h, ``add_feature_labels`` / ``create_feature_mask_from_slope``)
against the numpy / scipy restatement of the reference's ``scripts/prepare_feature_labels.py`` (_slope_cpu) and against the fixture
the reference's own code wrote.  Every case: labels, filtered mask and the six counts equal cell for cell.  The tile of the labelling
is 16 x 64: the shapes sit on it, one short of it and one past it; the chains run through every tile.

The device compares ``s = gx**2 + gy**2`` with a cut found by bisection on a one-element array, the oracle runs numpy's ``arctan``
over the plane; the two may disagree only where ``s`` lies within a few float32 steps of the cut (SIMD and scalar paths of numpy).
Every input here keeps ``s`` more than 64 steps away (depths in multiples of 3/64 put ``s`` on a coarse lattice); ``run`` asserts it
from the input alone."""
import numpy as np
import pytest
import torch
from scipy import ndimage

import _slope_cpu as cpu
from bathymetric_gnn_amd.data import add_feature_labels, create_feature_mask_from_slope, slope_cut
from bathymetric_gnn_amd.data.slope_features import slope_features_build, slope_stats
from test_gpu_review import FLATTEN_MASKS, comb, flatten_chunks, serpentine, spiral

pytestmark = pytest.mark.gpu
F32 = np.float32
Q = 3.0 / 64.0
CASES, CUTS = cpu.load_fixture()
TILE_R, TILE_C = 16, 64


def guard(depth, threshold):
    cut = slope_cut(threshold)
    if cut == 0:                                                # a negative threshold: every slope that is not NaN exceeds it
        return
    assert cpu.ulps_from_cut(depth, cut) > cpu.ULP_GUARD, "the input has a cell within 64 ulp of the cut"


def run(depth, threshold, min_size, device, wrecks=None, gt=None, radius=50):
    """Both public calls against the oracle; returns the oracle's ``(labels, mask, stats)``."""
    guard(depth, threshold)
    want_labels, want_mask, want_stats, want_count = cpu.add_feature_labels(depth, threshold, min_size, wrecks, gt, radius)
    ws = None if wrecks is None else [{"x": x, "y": y} for x, y in wrecks]
    got = add_feature_labels(depth, ws, threshold, radius, min_size, transform=gt, device=device)
    mask = create_feature_mask_from_slope(depth, threshold, min_size, device=device)
    assert mask.dtype == torch.bool and np.array_equal(mask.cpu().numpy(), want_mask)
    assert got.labels.dtype == torch.int32 and np.array_equal(got.labels.cpu().numpy(), want_labels)
    assert got.slope_stats() == want_stats and got.applied_features == want_count
    s = got.stats()
    assert s["feature_cells"] == int((want_labels == 1).sum()) and s["valid_cells"] == want_stats["valid_cells"]
    assert s["applied_features"] == want_count
    return want_labels, want_mask, want_stats


def relief(rng, h, w, holes=3, nan_rate=0.003, bump_rate=0.004):
    """A ragged relief in multiples of Q whose slopes straddle 5 .. 45 degrees, with bumps, 1.0e6 holes and NaNs."""
    rr, cc = np.meshgrid(np.arange(h, dtype=np.float64), np.arange(w, dtype=np.float64), indexing="ij")
    z = np.full((h, w), 30.0)
    for _ in range(4):
        fr, fc = rng.uniform(0.01, 0.04, 2) * rng.choice([-1, 1], 2)
        z += rng.uniform(0.4, 1.6) * np.sin(2 * np.pi * (fr * rr + fc * cc) + rng.uniform(0, 2 * np.pi))
    bumps = rng.random((h, w)) < bump_rate
    z[bumps] += rng.uniform(0.5, 4.0, int(bumps.sum()))
    d = (np.round(z / Q) * Q).astype(F32)
    for _ in range(holes if h > 12 and w > 12 else 0):
        r, c, a, b = rng.integers(0, h - 6), rng.integers(0, w - 6), rng.integers(2, 6), rng.integers(2, 6)
        d[r:r + a, c:c + b] = cpu.NODATA
    d[rng.random((h, w)) < nan_rate] = np.nan
    return d


@pytest.mark.parametrize("name", sorted(CASES))
def test_golden_fixture(name, gpu_device):
    c = CASES[name]
    mask = create_feature_mask_from_slope(c["depth"], c["threshold"], c["min_cluster_size"], device=gpu_device)
    assert np.array_equal(mask.cpu().numpy(), c["mask"])
    if c["labels"] is None:
        return
    wrecks = None if c["wrecks"] is None else [{"x": x, "y": y} for x, y in c["wrecks"]]
    got = add_feature_labels(c["depth"], wrecks, c["threshold"], c["radius"] if c["radius"] is not None else 50, c["min_cluster_size"],
                             transform=c["transform"], device=gpu_device)
    assert np.array_equal(got.labels.cpu().numpy(), c["labels"])
    assert got.applied_features == (c["wreck_count"] or 0)
    valid = cpu.valid_cells(c["depth"])
    assert got.slope_stats()["slope_feature_cells"] == int((c["mask"] & valid).sum()) and got.slope_stats()["kept_cells"] == int(c["mask"].sum())
    labels, depth = got.bands()
    assert labels.dtype == F32 and np.array_equal(labels, c["labels"].astype(F32)) and np.array_equal(depth, c["depth"], equal_nan=True)


@pytest.mark.parametrize("shape", [(16, 64), (15, 63), (17, 65), (2, 2), (2, 200), (200, 2), (37, 150)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_shapes_around_the_tile(shape, gpu_device):
    rng = np.random.default_rng([20241020, *shape])
    d = relief(rng, *shape)
    for threshold, min_size in ((15.0, 1), (15.0, 6), (5.0, 100)):
        _, _, stats = run(d, threshold, min_size, gpu_device)
    steps = np.add.outer(np.arange(shape[0]), np.arange(shape[1])).astype(F32)      # every cell steep: one cluster over every border
    _, mask, stats = run(steps, 15.0, 1, gpu_device)
    assert mask.all() and stats["clusters"] == 1 and stats["kept_cells"] == shape[0] * shape[1]


@pytest.mark.parametrize("shift", [-1, 0, 1])
def test_steps_on_the_tile_borders(shift, gpu_device):
    """A depth step between a tile's last row and the next tile's first, and between the last and first column: the steep cells on
    both sides take their difference through the halo."""
    d = np.full((40, 150), 21.0, F32)
    d[TILE_R + shift:, :] += F32(9.0)
    d[:, TILE_C + shift:] += F32(9.0)
    _, mask, stats = run(d, 15.0, 1, gpu_device)
    assert mask[TILE_R + shift - 1:TILE_R + shift + 1].all() and mask[:, TILE_C + shift - 1:TILE_C + shift + 1].all()
    assert stats["kept_cells"] == 2 * 150 + 2 * 40 - 4 and stats["clusters"] == 1


def test_one_sided_differences_at_the_border(gpu_device):
    """A step of 0.375 into the first / last row and column: the one-sided difference (0.375: 20.6 degrees) is steep, the central
    one of the next row (0.1875: 10.6 degrees) is not, and neither would a clamped central difference in the border row be."""
    for where in ("top", "bottom", "left", "right", "all"):
        d = np.full((33, 130), 21.0, F32)
        if where in ("top", "all"):
            d[0, :] += F32(0.375)
        if where in ("bottom", "all"):
            d[-1, :] += F32(0.375)
        if where in ("left", "all"):
            d[:, 0] += F32(0.375)
        if where in ("right", "all"):
            d[:, -1] += F32(0.375)
        _, mask, stats = run(d, 15.0, 1, gpu_device)
        inner = mask[1:-1, 1:-1]
        assert not inner.any() and stats["kept_cells"] > 0
        if where == "top":
            assert mask[0].all() and mask.sum() == 130
        if where == "right":
            assert mask[:, -1].all() and mask.sum() == 33
        if where == "all":
            assert stats["clusters"] == 1                       # (the corner cells' two differences cancel to steep all the same)


@pytest.mark.parametrize("name,pattern", [("serpentine", serpentine(31, 98)), ("comb", comb(31, 98)), ("spiral", spiral(31, 98))],
                         ids=lambda v: v if isinstance(v, str) else "")
def test_long_union_chains(name, pattern, gpu_device):
    """A pattern one cell wide, scaled to corridors four cells wide and raised by 64: the steep cells are the two cells on either
    side of every edge of the pattern.  The empty ring around it keeps the pattern's outline closed: one component."""
    d = (np.kron(np.pad(pattern, 1), np.ones((4, 4))) * 64.0).astype(F32) + F32(21.0)
    assert d.shape == (132, 400)
    steep = cpu.steep_mask(d, 15.0)
    lab, n = ndimage.label(steep)
    sizes = np.bincount(lab.ravel())
    sizes[0] = 0
    big = lab == int(np.argmax(sizes))
    tiles = {(r // TILE_R, c // TILE_C) for r, c in np.argwhere(big)}
    assert len(tiles) == -(-132 // TILE_R) * -(-400 // TILE_C), "one component runs through every tile"
    _, mask, stats = run(d, 15.0, int(sizes.max()), gpu_device)
    assert np.array_equal(mask, big) and stats["kept_clusters"] == 1 and stats["kept_cells"] == int(sizes.max()) > 5000


def lines_relief(name):
    """A depth plane whose steep cells at 15 degrees are FLATTEN_MASKS[name]: the rows are constant, so gx = 0.  One line: row 0
    stands 0.375 above the rest (the one-sided difference 0.375 is steep, the central one of row 1, 0.1875, is not).  Six lines: the
    even rows at one depth (no central difference across an odd row), the odd rows 0.75 apart (0.375 across every even row), and
    1.5 from the first and the last odd row to the plane's border rows."""
    h, w = FLATTEN_MASKS[name][0].shape
    d = np.full((h, w), 21.0, F32)
    if name == "one_line":
        d[0] += F32(0.375)
    else:
        d[0::2] = F32(22.5)
        d[1::2] = (F32(21.0) + F32(0.75) * np.arange(h // 2, dtype=F32))[:, None]
    return d


@pytest.mark.parametrize("name", sorted(FLATTEN_MASKS))
def test_flatten_wave_groups(name, gpu_device):
    """The two masks test_gpu_review.py builds for the wave-grouped flatten, as the steep cells of a depth plane."""
    mask, components, chunks = FLATTEN_MASKS[name]
    d = lines_relief(name)
    steep = cpu.steep_mask(d, 15.0)
    assert np.array_equal(steep, mask) and flatten_chunks(steep) == (components, chunks)
    _, kept, stats = run(d, 15.0, mask.shape[1], gpu_device)
    assert np.array_equal(kept, mask) and (stats["clusters"], stats["kept_clusters"], stats["kept_cells"]) == (components, components, mask.sum())
    _, kept, stats = run(d, 15.0, mask.shape[1] + 1, gpu_device)
    assert not kept.any() and stats["clusters"] == components


def test_clusters_of_99_and_100_cells_across_a_tile_corner(gpu_device):
    d = np.full((48, 300), 21.0, F32)
    d[TILE_R, 40:88] = 30.0                                     # rows 15 .. 17, columns 39 .. 88: across the corner (16, 64)
    d[2 * TILE_R, 170:218] = 30.0                               # across the corner (32, 192) ...
    d[2 * TILE_R - 2, 180] = np.nan                             # ... with one cell of its upper row taken out
    sizes = np.bincount(ndimage.label(cpu.steep_mask(d, 15.0))[0].ravel())[1:]
    assert sorted(sizes) == [99, 100]
    _, mask, stats = run(d, 15.0, 100, gpu_device)
    assert mask[TILE_R - 1, 63] and mask[TILE_R + 1, 64] and not mask[2 * TILE_R - 1:2 * TILE_R + 2].any()
    assert (stats["clusters"], stats["kept_clusters"], stats["kept_cells"], stats["steep_cells"]) == (2, 1, 100, 199)
    _, mask, stats = run(d, 15.0, 99, gpu_device)
    assert stats["kept_cells"] == 199
    _, mask, stats = run(d, 15.0, 101, gpu_device)
    assert not mask.any() and stats["slope_feature_cells"] == 0


def test_planes_without_a_valid_cell(gpu_device):
    labels, mask, stats = run(np.full((20, 70), np.nan, F32), 15.0, 1, gpu_device)
    assert (labels == -1).all() and not mask.any() and cpu.stats_list(stats) == [0] * 6
    labels, mask, stats = run(np.full((20, 70), cpu.NODATA, F32), 15.0, 1, gpu_device)
    assert (labels == -1).all() and not mask.any() and cpu.stats_list(stats) == [0] * 6
    # a threshold nothing reaches, and one everything reaches
    d = relief(np.random.default_rng(20241021), 20, 70)
    labels, mask, stats = run(d, 90.0, 1, gpu_device)
    assert not mask.any() and stats["valid_cells"] > 0
    labels, mask, stats = run(d, -1.0, 1, gpu_device)
    assert stats["steep_cells"] == int((~np.isnan(cpu.squared_gradient(d))).sum())


@pytest.mark.parametrize("shape", [(2, 131073), (1030, 2049)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_past_one_grid(shape, gpu_device):
    """2 x 131073: 2049 tiles, one workgroup of the 2048 labels a second tile.  1030 x 2049: more than 2048 steps of 1024 cells in
    the last pass, more than 2048 tiles."""
    d = relief(np.random.default_rng([20241022, *shape]), *shape, holes=0)
    _, _, stats = run(d, 15.0, 1, gpu_device)
    assert stats["clusters"] > 100
    _, _, stats = run(d, 15.0, 100, gpu_device)
    assert stats["clusters"] > stats["kept_clusters"]


def test_overlay_mode(gpu_device):
    rng = np.random.default_rng(20241023)
    d = relief(rng, 90, 210)
    guard(d, 15.0)
    base = rng.choice(np.array([-1, 0, 0, 0, 1, 2], np.int32), d.shape)
    want, want_stats = cpu.overlay(base, d, 15.0, 20)
    t_base = torch.from_numpy(base).to(gpu_device)
    labels, mask, block = slope_features_build(torch.from_numpy(d).to(gpu_device), slope_cut(15.0), 20, base_labels=t_base)
    got = labels.cpu().numpy()
    assert np.array_equal(got, want) and slope_stats(block) == want_stats and torch.equal(t_base.cpu(), torch.from_numpy(base))
    kept = mask.cpu().numpy().astype(bool)
    assert np.array_equal(kept, cpu.feature_mask(d, 15.0, 20)[0])
    for v in (-1, 2):
        assert (got[base == v] == v).all() and (kept & (base == v)).any()          # untouched, though steep cells lie there
    assert (got[base == 1] == 1).all() and (got[(base == 0) & kept] == 1).all() and (got[(base == 0) & ~kept] == 0).all()
    assert want_stats["slope_feature_cells"] == int(((base == 0) & kept).sum()) > 0
    # in place
    inplace = t_base.clone()
    ctx_labels, _, _ = slope_features_build(torch.from_numpy(d).to(gpu_device), slope_cut(15.0), 20, base_labels=inplace, want_mask=False)
    assert torch.equal(ctx_labels, labels)


def test_wrecks_over_the_slope_labels(gpu_device):
    rng = np.random.default_rng(20241024)
    h, w = 120, 170
    d = relief(rng, h, w)
    gt = (1000.0, 0.5, 0.0, 9000.0, 0.0, -2.0)
    centres = zip(rng.uniform(-0.2 * h, 1.2 * h, 40), rng.uniform(-0.2 * w, 1.2 * w, 40))
    wrecks = [(gt[0] + gt[1] * c, gt[3] + gt[5] * r) for r, c in centres]
    wrecks += [(gt[0] - 0.5 * gt[1], gt[3] - 0.5 * gt[5]), (gt[0] - 1.5 * gt[1], gt[3] + 5 * gt[5]), (gt[0] + (w + 0.5) * gt[1], gt[3] + 5 * gt[5])]
    labels, _, _ = run(d, 15.0, 30, gpu_device, wrecks, gt, 9)
    plain, _, _, _ = cpu.add_feature_labels(d, 15.0, 30)
    assert (labels == 1).sum() > (plain == 1).sum() and 3 < len(cpu.wreck_pixels(wrecks, gt, d.shape)) < len(wrecks)
    run(d, 15.0, 30, gpu_device, wrecks[:5], gt, 0)             # a radius of 0: the centre cell alone
    run(d, 15.0, 30, gpu_device, wrecks, gt, 10 ** 6)           # a disc over the whole plane


def test_ground_truth_with_slope_features_feeds_the_tile_store(gpu_device):
    from bathymetric_gnn_amd.data import BathymetricGrid, compute_ground_truth
    from bathymetric_gnn_amd.training import TileStore
    rng = np.random.default_rng(20241025)
    h, w = 96, 128
    rr, cc = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    clean = (np.round((-25.0 + 0.03 * rr + 0.02 * cc) / Q) * Q).astype(F32)
    clean[30:60, 40:80] += F32(3.0)                             # a block: its rim is steep
    noisy = clean + (0.02 * rng.standard_normal((h, w))).astype(F32)
    spikes = rng.random((h, w)) < 0.04
    noisy[spikes] += rng.choice([-1.0, 1.0], int(spikes.sum())).astype(F32)
    noisy[10:14, 100:110] = F32(1.0e6)
    transform = (400000.0, 0.5, 0.0, 4.2e6, 0.0, -0.5)
    bounds = (400000.0, 4.2e6 - 0.5 * h, 400000.0 + 0.5 * w, 4.2e6)
    grids = [BathymetricGrid(depth=g, uncertainty=None, transform=transform, crs="EPSG:32619", resolution=(0.5, 0.5), bounds=bounds)
             for g in (clean, noisy)]
    gt = compute_ground_truth(*grids, 0.15, device=gpu_device)
    source = gt.clean_depth.cpu().numpy()
    guard(source, 15.0)
    gts = gt.with_slope_features(15.0, 20)
    base = gt.labels.cpu().numpy()
    want, want_stats = cpu.overlay(base, source, 15.0, 20)
    got = gts.labels.cpu().numpy()
    assert np.array_equal(got, want) and gts.slope_stats() == want_stats and want_stats["slope_feature_cells"] > 100
    assert (base == 2).any() and (got[base == 2] == 2).all() and (got[base == -1] == -1).all() and not (base == 1).any()
    for plane in ("difference", "noisy_depth", "clean_depth"):
        assert getattr(gts, plane).data_ptr() == getattr(gt, plane).data_ptr()
    assert gts.labels.data_ptr() != gt.labels.data_ptr() and gt.slope_block is None
    with pytest.raises(ValueError):
        gt.slope_stats()
    with pytest.raises(ValueError):
        gt.with_slope_features(source="difference")
    store = TileStore.from_ground_truth(*gts.training_planes(), resolution=(0.5, 0.5), tile_size=32, overlap=8, min_valid_ratio=0.1,
                                        device=gpu_device)
    plain = TileStore.from_ground_truth(*gt.training_planes(), resolution=(0.5, 0.5), tile_size=32, overlap=8, min_valid_ratio=0.1,
                                        device=gpu_device)
    assert plain._class_counts[1] == 0 and store._class_counts[1] >= want_stats["slope_feature_cells"]
    assert store._class_counts[2] == plain._class_counts[2]
    noisy_src = gt.with_slope_features(15.0, 20, source="noisy_depth")
    want_noisy, _ = cpu.overlay(base, gt.noisy_depth.cpu().numpy(), 15.0, 20)
    assert np.array_equal(noisy_src.labels.cpu().numpy(), want_noisy)


def test_host_arrays_and_device_tensors_agree(gpu_device):
    from bathymetric_gnn_amd.data import BathymetricGrid
    d = relief(np.random.default_rng(20241026), 90, 210)
    gt = (0.0, 1.0, 0.0, 0.0, 0.0, -1.0)
    wrecks = [{"x": 50.5, "y": -40.5}, {"x": 180.5, "y": -10.5}]
    t = torch.from_numpy(d).to(gpu_device)
    host = add_feature_labels(d, wrecks, 15.0, 6, 30, transform=gt, device=gpu_device)
    dev = add_feature_labels(t, wrecks, 15.0, 6, 30, transform=gt)
    assert dev.depth.data_ptr() == t.data_ptr()                 # used where it lies
    grid = add_feature_labels(BathymetricGrid(depth=d, uncertainty=None, transform=gt, crs="EPSG:32619", resolution=(1.0, 1.0),
                                              bounds=(0.0, -90.0, 210.0, 0.0)), wrecks, 15.0, 6, 30, device=gpu_device)
    assert grid.crs == "EPSG:32619" and grid.transform == gt
    for other in (dev, grid):
        assert torch.equal(other.labels, host.labels) and other.stats() == host.stats() and other.slope_stats() == host.slope_stats()
    assert host.applied_features == 2 and host.stats()["painted_cells"] > 0
    assert torch.equal(create_feature_mask_from_slope(t, 15.0, 30), create_feature_mask_from_slope(d, 15.0, 30, device=gpu_device))
    # the defaults are the reference's
    assert torch.equal(add_feature_labels(t).labels, add_feature_labels(t, None, 15.0, 50, 100).labels)


def test_two_calls_give_equal_bits(gpu_device):
    t = torch.from_numpy(relief(np.random.default_rng(20241027), 300, 517)).to(gpu_device)
    a, b = add_feature_labels(t, min_cluster_size=10), add_feature_labels(t, min_cluster_size=10)
    assert a.labels.data_ptr() != b.labels.data_ptr() and torch.equal(a.labels, b.labels)
    assert torch.equal(a.slope_block, b.slope_block) and torch.equal(a.stats_block, b.stats_block) and a.slope_stats()["kept_clusters"] > 3
