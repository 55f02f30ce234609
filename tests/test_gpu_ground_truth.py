"""Ground truth from survey pairs on the device (bgnn_ground_truth_build, data/ground_truth.py) against the fixtures the
reference's own ``scripts/prepare_ground_truth.py`` wrote (tests/golden/truth, make_golden_truth.py): labels, the difference and
uncertainty planes, the median and every count exactly; the one float sum within the float64 bound of _eval_checks.py."""
import ctypes as C

import numpy as np
import pytest
import torch

from _eval_checks import TRUTH_CASES, check_stats, grids_of, load_case, truth_bands

pytestmark = pytest.mark.gpu


def _same_values(a, b):
    """Equal in value, NaN in the same places (signed zeros compare equal)."""
    return np.array_equal(a, b, equal_nan=True)


@pytest.mark.parametrize("on_device", [False, True], ids=["host_arrays", "device_tensors"])
@pytest.mark.parametrize("name", TRUTH_CASES)
def test_fixture(name, on_device, gpu_device):
    from bathymetric_gnn_amd.data import compute_ground_truth
    g, want = load_case("truth", name)
    clean, noisy = grids_of(g)
    if on_device:
        for grid in (clean, noisy):
            grid.depth = torch.from_numpy(grid.depth).to(gpu_device)
            grid.uncertainty = None if grid.uncertainty is None else torch.from_numpy(grid.uncertainty).to(gpu_device)
    gt = compute_ground_truth(clean, noisy, float(g["threshold"]), device=gpu_device)
    bands = truth_bands(g)
    assert gt.labels.dtype == torch.int32 and gt.difference.dtype == torch.float32 and gt.labels.device == gpu_device
    assert np.array_equal(gt.labels.cpu().numpy(), g["labels"])
    assert _same_values(gt.difference.cpu().numpy(), bands[1])
    if "noisy_uncertainty" in g:
        assert _same_values(gt.uncertainty.cpu().numpy(), bands[4])
    else:
        assert gt.uncertainty is None
    block = gt.block()
    offset = np.float32(block["offset"])
    assert offset == g["offset"] or (np.isnan(offset) and np.isnan(g["offset"])), (offset, g["offset"])
    assert gt.systematic_offset == float(g["offset"]) or np.isnan(g["offset"])
    assert int(block["valid"]) == want["valid_cells"] and int(block["noise"]) == want["noise_cells"]
    assert int(block["seafloor"]) == want["seafloor_cells"]
    stats = gt.stats()
    stats["clean_survey"], stats["noisy_survey"] = want["clean_survey"], want["noisy_survey"]     # (the fixtures' surveys have no path)
    check_stats(stats, want, g["labels"], bands[1])
    sea = g["labels"] == 0
    if sea.any():
        exact = bands[1][sea].astype(np.float64).sum() / int(sea.sum())
        assert abs(gt.seafloor_mean_difference - exact) <= 4 * int(sea.sum()) * 2.0 ** -53 * np.abs(bands[1][sea]).astype(np.float64).max()
    for got, ref in zip(gt.bands(), bands):
        assert got.dtype == np.float32 and _same_values(got, ref)
    assert gt.transform == tuple(float(v) for v in g["geotransform"]) and gt.crs == "EPSG:32619"


@pytest.mark.parametrize("name", ["clustered", "large", "even_low_bits"])
def test_two_calls_give_equal_bits(name, gpu_device):
    from bathymetric_gnn_amd.data import compute_ground_truth
    g, _ = load_case("truth", name)
    runs = []
    for _ in range(2):
        gt = compute_ground_truth(*grids_of(g), float(g["threshold"]), device=gpu_device)
        runs.append((gt.labels.cpu().numpy(), gt.difference.cpu().numpy().view(np.uint32), gt.uncertainty.cpu().numpy().view(np.uint32),
                     gt.stats_block.cpu().numpy()))
    for a, b in zip(*runs):
        assert np.array_equal(a, b)


def _numpy_ground_truth(clean, noisy, threshold):
    """The issue's six steps in numpy, with ``np.median`` for the offset."""
    raw = noisy - clean
    valid = np.isfinite(clean) & np.isfinite(noisy) & (clean != np.float32(1.0e6)) & (noisy != np.float32(1.0e6))
    offset = np.median(raw[valid])
    difference = np.where(valid, raw - offset, np.float32(np.nan)).astype(np.float32)
    with np.errstate(invalid="ignore"):
        labels = np.where(valid, np.where(np.abs(difference) > np.float32(threshold), 2, 0), -1).astype(np.int32)
    return offset, difference, labels


@pytest.fixture(scope="module")
def random_pair():
    """1000 x 1003: no multiple of a workgroup's 1024 cells, nor of a thread's 4; more workgroups than one."""
    rng = np.random.default_rng(7)
    clean = (-40 + 10 * rng.standard_normal((1000, 1003))).astype(np.float32)
    noisy = (clean + (0.3 * rng.standard_normal(clean.shape) - 0.05).astype(np.float32)).astype(np.float32)
    clean[rng.random(clean.shape) < 0.02] = 1.0e6
    noisy[rng.random(clean.shape) < 0.02] = np.nan
    unc = rng.random(clean.shape).astype(np.float32)
    return clean, noisy, unc, _numpy_ground_truth(clean, noisy, 0.15)


def test_random_pair_matches_numpy_median(random_pair, gpu_device):
    from bathymetric_gnn_amd.data.ground_truth import ground_truth_build
    clean, noisy, unc, (offset, difference, labels) = random_pair
    c, z, u = (torch.from_numpy(a).to(gpu_device) for a in (clean, noisy, unc))
    lab, diff, unc_out, stats = ground_truth_build(c, z, u, 0.15)
    from bathymetric_gnn_amd import runtime
    block = np.frombuffer(stats.cpu().numpy().tobytes(), np.dtype(runtime.GT_STATS_DTYPE))[0]
    assert np.float32(block["offset"]) == offset
    assert np.array_equal(lab.cpu().numpy(), labels) and _same_values(diff.cpu().numpy(), difference)
    assert _same_values(unc_out.cpu().numpy(), np.where(labels >= 0, unc, np.float32(np.nan)))
    assert (int(block["valid"]), int(block["noise"]), int(block["seafloor"])) == (int((labels >= 0).sum()), int((labels == 2).sum()),
                                                                                   int((labels == 0).sum()))
    mag = np.abs(difference[labels == 2])
    assert np.float32(block["noise_abs_max"]) == mag.max()
    exact = mag.astype(np.float64).sum()
    assert abs(float(block["noise_abs_sum"]) - exact) <= 4 * mag.size * 2.0 ** -53 * exact


def test_unaligned_planes_take_the_scalar_path_to_the_same_result(random_pair, gpu_device):
    """Planes that do not start on a 16-byte boundary are read element by element."""
    from bathymetric_gnn_amd.data.ground_truth import ground_truth_build
    clean, noisy, unc, _ = random_pair
    n = 70001
    c, z, u = (torch.from_numpy(a.reshape(-1)[:n + 1].copy()).to(gpu_device)[1:] for a in (clean, noisy, unc))
    assert c.data_ptr() % 16 == 4 and c.is_contiguous()
    offset, difference, labels = _numpy_ground_truth(clean.reshape(-1)[1:n + 1], noisy.reshape(-1)[1:n + 1], 0.2)
    lab, diff, unc_out, stats = ground_truth_build(c, z, u, 0.2)
    assert np.array_equal(lab.cpu().numpy(), labels) and _same_values(diff.cpu().numpy(), difference)
    assert _same_values(unc_out.cpu().numpy(), np.where(labels >= 0, unc.reshape(-1)[1:n + 1], np.float32(np.nan)))
    assert stats.view(torch.float32)[10].item() == offset
    # and the aligned copy of the same cells gives the same block, bit for bit
    lab2, diff2, _, stats2 = ground_truth_build(c.clone(), z.clone(), u.clone(), 0.2)
    assert torch.equal(stats, stats2) and torch.equal(lab, lab2) and torch.equal(diff.view(torch.int32), diff2.view(torch.int32))


def test_no_cells(gpu_device):
    from bathymetric_gnn_amd.data.ground_truth import ground_truth_build
    e = torch.empty((0, 5), dtype=torch.float32, device=gpu_device)
    lab, diff, unc, stats = ground_truth_build(e, e.clone())
    assert lab.shape == (0, 5) and unc is None and stats[:3].tolist() == [0, 0, 0] and np.isnan(stats.view(torch.float32)[10].item())


def test_refusals(gpu_device):
    from bathymetric_gnn_amd import runtime as rt
    ctx = rt.get_context(gpu_device)
    lib = ctx.lib
    n = 100
    f = [torch.zeros(n + 4, dtype=torch.float32, device=gpu_device) for _ in range(5)]
    lab = torch.zeros(n, dtype=torch.int32, device=gpu_device)
    need = lib.bgnn_ground_truth_workspace_bytes(n)
    ws = torch.zeros(need // 8 + 2, dtype=torch.int64, device=gpu_device)
    stats = torch.full((8,), 77, dtype=torch.int64, device=gpu_device)
    p = rt.ptr

    def call(clean=p(f[0]), noisy=p(f[1]), unc=p(f[2]), cells=n, ws_p=p(ws), ws_bytes=need, labels=p(lab), diff=p(f[3]), unc_out=p(f[4]),
             st=p(stats)):
        return lib.bgnn_ground_truth_build(ctx.handle, clean, noisy, unc, cells, 1.0e6, 0.15, ws_p, C.c_size_t(ws_bytes), labels, diff,
                                           unc_out, st)

    def refused(word, **kw):
        assert call(**kw) == rt.ERR_INVALID
        assert word in lib.bgnn_last_error().decode(), lib.bgnn_last_error()

    for k in ("clean", "noisy", "ws_p", "labels", "diff", "st"):
        refused("NULL", **{k: None})
    refused("unc_out without", unc=None)
    refused("-1 cells", cells=-1)
    refused("workspace of", ws_bytes=need - 8)
    refused("workspace is not 8-byte aligned", ws_p=C.c_void_p(ws.data_ptr() + 4))
    refused("statistics block is not 8-byte aligned", st=C.c_void_p(stats.data_ptr() + 4))
    refused("aliases", diff=p(f[0]))
    ctx.synchronize()
    assert stats.tolist() == [77] * 8 and not lab.any()      # nothing was launched
    assert call(cells=0) == 0
    ctx.synchronize()
    assert stats.tolist() == [77] * 8
    assert call(unc=None, unc_out=None) == 0              # (and the accepted call runs)
    ctx.synchronize()
    assert stats[0].item() == n


def test_tile_store_from_device_planes_equals_the_host_store(gpu_device):
    """``TileStore.from_ground_truth`` on the device planes of a GroundTruth against the same planes as host arrays: every plane,
    box and count."""
    from bathymetric_gnn_amd.data import compute_ground_truth
    from bathymetric_gnn_amd.training import TileStore
    g, _ = load_case("truth", "large")
    gt = compute_ground_truth(*grids_of(g), float(g["threshold"]), device=gpu_device)
    kw = dict(resolution=(0.5, 0.5), tile_size=64, overlap=16, min_valid_ratio=0.1, device=gpu_device)
    dev = TileStore.from_ground_truth(*gt.training_planes(), **kw)
    host = TileStore.from_ground_truth(*(t.cpu().numpy() for t in gt.training_planes()), **kw)
    assert len(dev) == len(host) > 20 and dev.boxes == host.boxes and dev._class_counts == host._class_counts
    assert (300 - 64, 257 - 64, 300, 257) in dev.boxes        # the far-corner edge tile
    assert np.array_equal(dev.hw, host.hw) and np.array_equal(dev.res, host.res) and np.array_equal(dev.offsets, host.offsets)
    for k in ("depth", "mask", "unc", "labels", "difference"):
        a, b = getattr(dev, k), getattr(host, k)
        assert a.dtype == b.dtype and a.device == b.device and a.shape == b.shape, k
        if a.dtype == torch.float32:
            a, b = a.view(torch.int32), b.view(torch.int32)
        assert torch.equal(a, b), k
    with pytest.raises(TypeError):
        TileStore.from_ground_truth(gt.labels, gt.difference.cpu().numpy(), gt.noisy_depth, **kw)
