"""Gridding soundings on the device (bgnn_soundings_*, data/sounding_grid.py) against the numpy / Python-integer restatement of
_soundings_cpu.py (test_host_soundings.py guards the restatement itself).  ``count``, ``min``, ``max``, ``mean``, ``valid`` and the
counters are compared for equal bits, and so is ``std``: the bound set for it was 1 float32 ulp, in case the device's float64 division
or square root were not correctly rounded; on the MI355X every cell of every case here came out with the restatement's bits, so
the check asks for that (the distance in ulps is still printed).  Any two device runs on the same soundings must leave equal bits."""
import numpy as np
import pytest
import torch

import _soundings_cpu as sc

pytestmark = pytest.mark.gpu

PLANES = ("count", "mean", "std", "min", "max", "valid")


def _ulps(a, b):
    def lin(v):
        i = np.ascontiguousarray(v, np.float32).view(np.int32).astype(np.int64)
        return np.where(i < 0, np.int64(-2 ** 31) - i, i)
    return np.abs(lin(a) - lin(b))


def _dev(device, *arrays):
    return [torch.from_numpy(np.array(a)).to(device) for a in arrays]           # (a copy: the shared clouds are read-only)


def _host(grid):
    return {k: getattr(grid, k).cpu().numpy() for k in PLANES}


def _check(grid, want, shape):
    got = _host(grid)
    assert grid.counters == want["counters"]
    for k in PLANES:
        assert got[k].shape == tuple(shape) and got[k].dtype == want[k].dtype, k
    for k in ("count", "valid"):
        assert np.array_equal(got[k], want[k]), k
    for k in ("mean", "min", "max"):
        assert np.array_equal(got[k].view(np.uint32), want[k].view(np.uint32)), k
    worst = int(_ulps(got["std"], want["std"]).max())
    print(f"std: {worst} ulp at most from the restatement, {int((got['std'].view(np.uint32) != want['std'].view(np.uint32)).sum())} "
          f"of {got['std'].size} cells differ")
    assert worst == 0                                            # (measured: the float64 division and square root round as the host's)
    return got


def _same_bits(a, b):
    for k in PLANES:
        assert a[k].tobytes() == b[k].tobytes(), k


@pytest.mark.parametrize("min_count", [1, 3])
def test_mixed_cloud(min_count, gpu_device):
    """20 000 soundings on 16 x 16 cells at res 0.3, origin (500000, 4000000): one in ten beyond a border, NaN in each of x, y, z,
    +-inf, z = 40000, z = -32768 (both out of range), z = +-32767.99 (accepted), soundings on the borders."""
    from bathymetric_gnn_amd.data import SoundingGridder
    x, y, z = sc.mixed_cloud()
    want = sc.mixed_want(min_count)
    g = SoundingGridder(sc.MIXED_SHAPE, sc.MIXED_ORIGIN, sc.MIXED_RES, device=gpu_device, min_count=min_count)
    g.add(*_dev(gpu_device, x, y, z))
    assert g.counters() == want["counters"] and g.offered == 20000
    grid = g.finalize()
    _check(grid, want, sc.MIXED_SHAPE)
    c = want["counters"]
    assert c["nonfinite"] == 7 and c["out_of_range"] == 2 and c["outside"] > 1500 and c["accepted"] > 17000
    assert grid.transform == (500000.0, 0.3, 0.0, 4000000.0, 0.0, -0.3) and grid.resolution == (0.3, 0.3)
    # host arrays go the same way (uploaded in chunks), and so does the one-call form
    from bathymetric_gnn_amd.data import grid_soundings
    g2 = grid_soundings(np.array(x), np.array(y), np.array(z), sc.MIXED_RES, shape=sc.MIXED_SHAPE, origin=sc.MIXED_ORIGIN,
                        device=gpu_device, min_count=min_count)
    _same_bits(_host(g2), _host(grid))
    assert g2.counters == c


def test_refusals_before_any_launch(gpu_device):
    from bathymetric_gnn_amd.data import SoundingGridder
    g = SoundingGridder((4, 4), (0.0, 4.0), 1.0, device=gpu_device)
    x, y, z = _dev(gpu_device, np.array([0.5]), np.array([3.5]), np.array([-1.0], np.float32))
    with pytest.raises(TypeError, match="float64"):
        g.add(x.float(), y, z)
    with pytest.raises(TypeError, match="float32"):
        g.add(x, y, z.double())
    with pytest.raises(ValueError, match="number of soundings"):
        g.add(x, y, torch.cat([z, z]))
    g.offered = 2 ** 31 - 1
    with pytest.raises(ValueError, match="a total above 2147483647"):
        g.add(x, y, z)
    g.offered = 0
    assert g.counters() == dict(accepted=0, nonfinite=0, outside=0, out_of_range=0)
    for bad in (dict(shape=(0, 4)), dict(resolution=0.0), dict(resolution=float("nan")), dict(min_count=0), dict(origin=(0.0, float("inf")))):
        kw = dict(shape=(4, 4), origin=(0.0, 4.0), resolution=1.0, device=gpu_device)
        kw.update(bad)
        with pytest.raises(ValueError):
            SoundingGridder(**kw)


@pytest.mark.parametrize("res", [0.7, 1.1])
@pytest.mark.parametrize("along", ["x", "y"])
def test_borders_decide_the_arithmetic(along, res, gpu_device):
    """Origin (0, 0), a 1 x 4096 and a 4096 x 1 grid, soundings at k * res for every k and one float64 step on either side: the
    cells must be numpy's floor(t / res) -- a multiply by the reciprocal, or an approximate division, files hundreds elsewhere."""
    from bathymetric_gnn_amd.data import SoundingGridder
    t, z = sc.border_cloud(res)
    on, k = t[:4096], np.arange(4096)
    want_cell = np.floor(on / np.float64(res))
    assert int((want_cell == k - 1).sum()) >= 100                # the input decides: the restatement itself files these in k - 1
    other = np.full(t.size, 0.5 * res)
    shape = (1, 4096) if along == "x" else (4096, 1)
    x, y = (t, -other) if along == "x" else (other, -t)
    want = sc.grid(x, y, z, shape, (0.0, 0.0), res)
    cell = np.floor(t / np.float64(res))
    inside = (cell >= 0) & (cell < 4096)
    assert np.array_equal(want["count"].reshape(-1), np.bincount(cell[inside].astype(np.int64), minlength=4096))
    g = SoundingGridder(shape, (0.0, 0.0), res, device=gpu_device)
    g.add(*_dev(gpu_device, x, y, z))
    _check(g.finalize(), want, shape)


def test_order_chunks_repeats(gpu_device):
    """The mixed cloud in one call, in seven ragged chunks (one empty, one of a single sounding), permuted, and twice over into
    fresh states: equal bits in every plane, std included, and equal counters.  finalize, add, finalize equals adding it all first."""
    from bathymetric_gnn_amd.data import SoundingGridder
    x, y, z = sc.mixed_cloud()
    new = lambda: SoundingGridder(sc.MIXED_SHAPE, sc.MIXED_ORIGIN, sc.MIXED_RES, device=gpu_device)
    dx, dy, dz = _dev(gpu_device, x, y, z)
    runs = []
    for _ in range(2):                                           # twice over into fresh states
        g = new(); g.add(dx, dy, dz); runs.append(g.finalize())
    cuts = [0, 1, 1, 4097, 4352, 9999, 16000, 20000]             # chunks of 1, 0, 4096, 255, 5647, 6001, 4000
    g = new()
    for lo, hi in zip(cuts[:-1], cuts[1:]):
        g.add(dx[lo:hi], dy[lo:hi], dz[lo:hi])
    assert g.offered == 20000
    runs.append(g.finalize())
    perm = torch.from_numpy(np.random.default_rng(9).permutation(z.size)).to(gpu_device)
    g = new(); g.add(dx[perm], dy[perm], dz[perm]); runs.append(g.finalize())
    g = new(); g.add(dx[:7001], dy[:7001], dz[:7001])
    first = g.finalize()
    g.add(dx[7001:], dy[7001:], dz[7001:])
    runs.append(g.finalize())
    ref = _host(runs[0])
    for r in runs[1:]:
        _same_bits(_host(r), ref)
        assert r.counters == runs[0].counters
    _check(runs[0], sc.mixed_want(1), sc.MIXED_SHAPE)
    want_first = sc.grid(x[:7001], y[:7001], z[:7001], sc.MIXED_SHAPE, sc.MIXED_ORIGIN, sc.MIXED_RES)
    _check(first, want_first, sc.MIXED_SHAPE)                    # (and the planes of the first finalize were its own)
    g.reset()
    assert g.offered == 0 and g.counters()["accepted"] == 0 and int(g.finalize().count.sum()) == 0


def test_contention_and_runs(gpu_device):
    """200 000 soundings in one cell of an 8 x 8 grid, and equal-cell runs of lengths 1 .. 130 laid end to end (runs straddle wave
    and workgroup boundaries): exact."""
    from bathymetric_gnn_amd.data import SoundingGridder
    rng = np.random.default_rng(4)
    n = 200000
    x = 3.0 + rng.uniform(0.0, 1.0, n)
    y = 8.0 - (5.0 + rng.uniform(0.001, 1.0, n))
    z = (-120.0 + 30.0 * rng.standard_normal(n)).astype(np.float32)
    want = sc.grid(x, y, z, (8, 8), (0.0, 8.0), 1.0)
    assert want["count"][5, 3] == n == want["counters"]["accepted"]
    g = SoundingGridder((8, 8), (0.0, 8.0), 1.0, device=gpu_device)
    g.add(*_dev(gpu_device, x, y, z))
    _check(g.finalize(), want, (8, 8))

    x, y, z = sc.runs_cloud()
    assert z.size == 130 * 131 // 2
    want = sc.grid(x, y, z, (8, 8), (0.0, 8.0), 1.0)
    assert want["counters"]["accepted"] == z.size and int((want["count"] > 0).sum()) == 64
    g = SoundingGridder((8, 8), (0.0, 8.0), 1.0, device=gpu_device)
    g.add(*_dev(gpu_device, x, y, z))
    _check(g.finalize(), want, (8, 8))


def test_far_corner_of_a_large_grid(gpu_device):
    """10400 x 10400 cells: a state of 4.3 GB, so the far cells lie past byte 2^32 of it (and past cell 2^26 of the planes).  A
    few soundings in the first cell, in the last one and in the first cell whose bytes start past 2^32 must land there and nowhere
    else.  (A cell ADDRESS past 2^31 needs an 86 GB state; the cell-index function is checked there on the host.)"""
    from bathymetric_gnn_amd.data import SoundingGridder
    H = W = 10400
    past = (2 ** 32) // 40 + 1                                   # the first cell that lies wholly past byte 2^32 of the state
    groups = {(0, 0): [-5.25, -7.5], (past // W, past % W): [-11.125], (H - 1, W - 1): [-3.0, -4.5, -9.75]}
    assert 32 + 40 * past >= 2 ** 32 and past < H * W
    xs, ys, zs = [], [], []
    for (r, c), depths in groups.items():
        for j, d in enumerate(depths):
            xs.append(c + 0.25 + 0.25 * j); ys.append(H - r - 0.5); zs.append(d)
    x, y, z = np.array(xs, np.float64), np.array(ys, np.float64), np.array(zs, np.float32)
    g = SoundingGridder((H, W), (0.0, float(H)), 1.0, device=gpu_device)
    g.add(*_dev(gpu_device, x, y, z))
    grid = g.finalize()
    assert grid.counters == dict(accepted=6, nonfinite=0, outside=0, out_of_range=0)
    assert int(grid.count.sum(dtype=torch.int64)) == 6 and int(grid.valid.sum(dtype=torch.int64)) == 3
    for (r, c), depths in groups.items():
        sel = np.array([(xi, yi, zi) for xi, yi, zi in zip(xs, ys, zs) if int(xi) == c and int(H - yi) == r])
        want = sc.grid(sel[:, 0], sel[:, 1], sel[:, 2].astype(np.float32), (1, 1), (float(c), float(H - r)), 1.0)
        assert want["count"][0, 0] == len(depths)
        for k in PLANES:
            got = getattr(grid, k)[r, c].cpu().numpy()
            assert got.tobytes() == want[k][0, 0].tobytes(), (r, c, k)


@pytest.mark.parametrize("n", [1, 255, 256, 257, 100003])
def test_extent_and_planning(n, gpu_device):
    """min and max of the finite coordinates, bit-equal to numpy's; the planned grid leaves no sounding outside."""
    from bathymetric_gnn_amd.data import SoundingGridder, plan_sounding_grid, sounding_extent
    rng = np.random.default_rng(n)
    x = 500000.0 + rng.uniform(-70, 90, n)
    y = 4000000.0 + rng.uniform(-40, 30, n)
    z = (-30.0 + rng.standard_normal(n)).astype(np.float32)
    if n > 1:
        for a, v in ((x, np.nan), (x, np.inf), (y, -np.inf), (y, np.nan), (x, -np.inf)):
            a[rng.integers(0, n, max(1, n // 50))] = v
        x[n // 2], y[n // 2] = 500123.25, 3999876.5              # (at least one sounding with both coordinates finite)
    dx, dy, dz = _dev(gpu_device, x, y, z)
    e = sounding_extent(dx, dy)
    fx, fy = x[np.isfinite(x)], y[np.isfinite(y)]
    assert (e["finite_x"], e["finite_y"]) == (fx.size, fy.size)
    for name, v in (("min_x", fx.min()), ("max_x", fx.max()), ("min_y", fy.min()), ("max_y", fy.max())):
        assert np.float64(e[name]).tobytes() == np.float64(v).tobytes(), name
    res = 0.7
    shape, origin = plan_sounding_grid(dx, dy, res)
    assert (shape, origin) == plan_sounding_grid(x, y, res)      # the device plan is the numpy plan
    g = SoundingGridder(shape, origin, res, device=gpu_device)
    g.add(dx, dy, dz)
    c = g.counters()
    both = np.isfinite(x) & np.isfinite(y)
    assert c["outside"] == 0 and c["accepted"] == int(both.sum()) and c["nonfinite"] == n - int(both.sum())
    _check(g.finalize(), sc.grid(x, y, z, shape, origin, res), shape)


def test_all_nan_cloud_is_refused(gpu_device):
    from bathymetric_gnn_amd.data import plan_sounding_grid, sounding_extent
    dx, dy = _dev(gpu_device, np.full(300, np.nan), np.linspace(0.0, 1.0, 300))
    e = sounding_extent(dx, dy)
    assert e["finite_x"] == 0 and e["min_x"] == np.inf and e["max_x"] == -np.inf and e["finite_y"] == 300
    with pytest.raises(ValueError, match="no finite coordinate"):
        plan_sounding_grid(dx, dy, 0.5)
    with pytest.raises(ValueError, match="no finite coordinate"):
        plan_sounding_grid(dx[:0], dy[:0], 0.5)


def test_hand_over_to_the_pipeline(gpu_device):
    """survey_tensors() goes straight into process_survey_device (64 / 16 tiles, an 8-channel model, so std is used as the
    uncertainty band); the result equals to_grid() sent through process_grid_device bit for bit; depth = "min" / "max" hand over
    those planes."""
    from bathymetric_gnn_amd import synthetic
    from bathymetric_gnn_amd.config import Config
    from bathymetric_gnn_amd.data import grid_soundings
    from bathymetric_gnn_amd.models import BathymetricGNN, BathymetricPipeline
    H, W, res = 150, 131, 0.5
    x0, y0 = 500000.0, 4000000.0
    rng = np.random.default_rng(6)
    n = 6 * H * W
    x = x0 + rng.uniform(0, W * res, n)
    y = y0 - rng.uniform(0, H * res, n)
    hole = (x < x0 + 20.0) & (y > y0 - 25.0)                     # a corner without soundings: invalid cells, skipped tiles
    x, y = x[~hole], y[~hole]
    z = (-30.0 - 0.05 * (x - x0) + 2.0 * np.sin((y0 - y) / 7.0) + 0.1 * rng.standard_normal(x.size)).astype(np.float32)
    grid = grid_soundings(*_dev(gpu_device, x, y, z), res, shape=(H, W), origin=(x0, y0), min_count=2)
    valid = grid.valid.cpu().numpy()
    assert 0.5 < valid.mean() < 0.95 and grid.counters["outside"] == 0
    cfg = Config(); cfg.tile.tile_size, cfg.tile.overlap = 64, 16
    pipe = BathymetricPipeline(cfg, tile_batch=7)
    sd = synthetic.synthetic_state_dict(in_channels=8, seed=1234)
    m = BathymetricGNN(in_channels=8, edge_dim=3, dropout=0.0); m.load_state_dict({k: torch.as_tensor(v) for k, v in sd.items()})
    pipe.set_model(m.to(gpu_device).eval())
    outs = {}
    for depth in ("mean", "min", "max"):
        depth_t, valid_t, unc_t = grid.survey_tensors(depth)
        assert depth_t is getattr(grid, depth) and valid_t is grid.valid and unc_t is grid.std
        out = pipe.process_survey_device(depth_t, valid_t, unc_t, grid.resolution).cpu().numpy()
        host = grid.to_grid(depth)
        assert np.array_equal(host.depth, depth_t.cpu().numpy()) and np.array_equal(host.uncertainty, grid.std.cpu().numpy())
        assert np.array_equal(host.valid_mask, valid.astype(bool)) and host.nodata_value == 1.0e6
        assert host.transform == (x0, res, 0.0, y0, 0.0, -res) and host.resolution == (res, res)
        assert host.bounds == (x0, y0 - H * res, x0 + W * res, y0)
        via_host = pipe.process_grid_device(host)
        for k, name in enumerate(("classification", "confidence", "correction", "cleaned_depth")):
            assert np.array_equal(via_host[name].view(np.uint32), out[k].view(np.uint32)), (depth, name)
        outs[depth] = out
    lo, mid, hi = grid.min.cpu().numpy(), grid.mean.cpu().numpy(), grid.max.cpu().numpy()
    v = valid.astype(bool)
    q = np.float32(2.0 ** -16)                                   # (the mean is formed from depths rounded to 2^-16 m)
    assert (lo[v] - q <= mid[v]).all() and (mid[v] <= hi[v] + q).all() and (lo[v] < hi[v]).any()
    assert not np.array_equal(outs["min"][3], outs["max"][3])    # (cleaned depth follows the surface that was handed over)
    with pytest.raises(ValueError):
        grid.survey_tensors("median")
