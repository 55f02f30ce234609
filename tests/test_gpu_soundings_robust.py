"""Robust gridding of soundings on the device (bgnn_soundings_robust_*, data/sounding_robust.py) against the numpy / Python-integer
restatement of _robust_cpu.py (test_host_soundings_robust.py guards the restatement itself).  Every plane, ``sorted_q``, ``start``,
the counters and the flags are compared for equal bits; any two device runs on the same soundings, in any order and any split over
``add`` calls, must leave equal bits."""
import functools

import numpy as np
import pytest
import torch

import _robust_cpu as rc
import _soundings_cpu as sc

pytestmark = pytest.mark.gpu

FLOATS = ("median", "mad", "kept_mean", "kept_std", "kept_min", "kept_max")


def _dev(device, *arrays):
    return [torch.from_numpy(np.array(a)).to(device) for a in arrays]           # (a copy: the shared clouds are read-only)


def _host(grid):
    """Everything a finalize returns, as host arrays; sorted_q cut to the accepted soundings (the rest of the capacity is unused)."""
    out = {k: getattr(grid, k).cpu().numpy() for k in rc.PLANES}
    out["start"] = grid.start.cpu().numpy().view(np.uint32).astype(np.int64)
    out["sorted_q"] = grid.sorted_q.cpu().numpy()[:int(out["start"][-1])]
    return out


def _check(grid, want, shape):
    got = _host(grid)
    assert grid.counters == want["counters"]
    for k in rc.PLANES:
        assert got[k].shape == tuple(shape) and got[k].dtype == want[k].dtype, k
    for k in ("count", "kept", "valid", "center2", "limit", "start", "sorted_q"):
        assert np.array_equal(got[k], want[k]), k
    for k in FLOATS:
        differ = got[k].view(np.uint32) != want[k].view(np.uint32)
        assert not differ.any(), (k, int(differ.sum()), got[k][differ][:4], want[k][differ][:4])
    return got


def _same_bits(a, b):
    for k in list(rc.PLANES) + ["start", "sorted_q"]:
        assert a[k].tobytes() == b[k].tobytes(), k


def _gridder(device, shape, origin, res, capacity, **kw):
    from bathymetric_gnn_amd.data import RobustSoundingGridder
    return RobustSoundingGridder(shape, origin, res, capacity, device=device, **kw)


@pytest.mark.parametrize("k,floor_m,min_count", [(3 * 1.4826, 0.0, 1), (1.0, 0.0, 3), (4.4478, 0.05, 1)])
def test_mixed_cloud(k, floor_m, min_count, gpu_device):
    """20 000 soundings on 16 x 16 cells (44 to 98 per cell: the wave class and the first of the LDS class), one in ten beyond a
    border, NaN, +-inf, out-of-range and border soundings planted; the flags of the cloud itself."""
    x, y, z = sc.mixed_cloud()
    want = rc.mixed_want(k, floor_m, min_count)
    g = _gridder(gpu_device, sc.MIXED_SHAPE, sc.MIXED_ORIGIN, sc.MIXED_RES, 20000, k=k, floor_m=floor_m, min_count=min_count)
    dx, dy, dz = _dev(gpu_device, x, y, z)
    g.add(dx, dy, dz)
    assert g.counters() == want["counters"] and g.offered == 20000
    grid = g.finalize()
    _check(grid, want, sc.MIXED_SHAPE)
    flags = g.flag(dx, dy, dz, grid).cpu().numpy()
    assert flags.dtype == np.uint8 and np.array_equal(flags, want["flags"])
    assert int((flags == 1).sum()) == int((want["count"].astype(np.int64) - want["kept"]).sum()) > 0
    assert grid.transform == (500000.0, 0.3, 0.0, 4000000.0, 0.0, -0.3) and grid.resolution == (0.3, 0.3)
    # a cell's sounding list in metres; host arrays go the same way (uploaded in chunks), and so does the one-call form
    cell = 5 * 16 + 7
    lo, hi = want["start"][cell], want["start"][cell + 1]
    assert np.array_equal(grid.cell_soundings(5, 7).cpu().numpy(), want["sorted_q"][lo:hi].astype(np.float64) / 65536.0)
    from bathymetric_gnn_amd.data import grid_soundings_robust
    g2 = grid_soundings_robust(np.array(x), np.array(y), np.array(z), sc.MIXED_RES, shape=sc.MIXED_SHAPE, origin=sc.MIXED_ORIGIN,
                               device=gpu_device, k=k, floor_m=floor_m, min_count=min_count)
    _same_bits(_host(g2), _host(grid))
    assert g2.counters == want["counters"]


BOUNDARY_SHAPE = (4, 8)


@functools.lru_cache(maxsize=None)
def _boundary_cloud():
    """One cell each with n = 0, 1, 2, 3, every class boundary - 1, exact, + 1 and one large segment, then cells whose depths hit:
    all-equal values (MAD 0, limit 0, all kept) in each class, two-valued cells in the wave and the radix class, mixed signs with
    -0.0, |z| just under 32768 of one sign (m2 near +-2^32) and of both signs through every radix digit, an even n with differing
    middles (a half-integer median).  Shuffled; a few soundings that are not accepted ride along."""
    from bathymetric_gnn_amd import runtime as rt
    wave, lds = rt.ROBUST_WAVE_MAX, rt.ROBUST_LDS_MAX
    rng = np.random.default_rng(17)
    normal = lambda n, mean=-35.0, sd=2.0: (mean + sd * rng.standard_normal(n)).astype(np.float32)
    big = np.float32(32767.998)
    near = lambda n, sign: (sign * (32767.0 + rng.uniform(0.0, 0.99, n))).astype(np.float32)
    cells = [np.zeros(0, np.float32), normal(1), np.array([-12.00001, -12.00003], np.float32), normal(3)]
    cells += [normal(n) for n in (wave - 1, wave, wave + 1, lds - 1, lds, lds + 1, 10000)]
    cells += [np.full(50, -17.25, np.float32), np.full(wave + 136, -17.25, np.float32), np.full(lds + 5, 3.5, np.float32)]
    cells += [rng.choice(np.array([-20.0, -20.5], np.float32), wave), rng.choice(np.array([-20.0, 70.125], np.float32), lds + 904)]
    cells += [np.concatenate([normal(38, 0.0, 0.001), np.array([-0.0, 0.0], np.float32)])]
    cells += [np.concatenate([near(5, 1), [big]]).astype(np.float32), near(wave + 1, -1),
              np.concatenate([near(lds // 2 + 1, 1), near(lds // 2, -1), [big, -big]]).astype(np.float32)]
    cells += [np.array([-9.5, -9.5], np.float32), np.array([-30.0, -30.00002, -30.00004, 55.0], np.float32)]
    assert len(cells) <= BOUNDARY_SHAPE[0] * BOUNDARY_SHAPE[1]
    xs, ys, zs = [], [], []
    for i, depths in enumerate(cells):
        r, c = divmod(i, BOUNDARY_SHAPE[1])
        xs.append(c + rng.uniform(0.05, 0.95, depths.size)); ys.append(BOUNDARY_SHAPE[0] - (r + rng.uniform(0.05, 0.95, depths.size)))
        zs.append(depths)
    xs.append(np.array([-0.5, 2.5, np.nan, 3.5])); ys.append(np.array([1.5, 1.5, 1.5, 9.0])); zs.append(np.array([-5, 40000, -5, -5], np.float32))
    x, y, z = np.concatenate(xs), np.concatenate(ys), np.concatenate(zs).astype(np.float32)
    p = rng.permutation(z.size)
    return sc._frozen(x[p].astype(np.float64), y[p].astype(np.float64), z[p]) + (tuple(c.size for c in cells),)


@functools.lru_cache(maxsize=None)
def _boundary_want():
    x, y, z, _ = _boundary_cloud()
    return rc.grid(x, y, z, BOUNDARY_SHAPE, (0.0, float(BOUNDARY_SHAPE[0])), 1.0)


def test_class_boundaries(gpu_device):
    from bathymetric_gnn_amd import runtime as rt
    x, y, z, sizes = _boundary_cloud()
    want = _boundary_want()
    n = want["count"].reshape(-1)
    assert tuple(n[:len(sizes)]) == sizes and want["counters"] == dict(accepted=sum(sizes), nonfinite=1, outside=2, out_of_range=1)
    for edge in (rt.ROBUST_WAVE_MAX, rt.ROBUST_LDS_MAX):
        assert {edge - 1, edge, edge + 1} <= set(n.tolist())
    assert {0, 1, 2, 3, 10000} <= set(n.tolist())
    c2, lim, kept = want["center2"].reshape(-1), want["limit"].reshape(-1), want["kept"].reshape(-1)
    assert (c2 % 2 != 0).any()                                   # a half-integer median
    assert ((lim == 0) & (kept == n) & (n >= 50)).sum() == 3     # the all-equal cells, one per class
    assert c2.max() > 2 ** 32 - 2 ** 18 and c2.min() < -(2 ** 32 - 2 ** 18)
    assert (kept < n).any() and 25000 < z.size < 45000
    g = _gridder(gpu_device, BOUNDARY_SHAPE, (0.0, float(BOUNDARY_SHAPE[0])), 1.0, z.size + 3)
    dx, dy, dz = _dev(gpu_device, x, y, z)
    g.add(dx, dy, dz)
    grid = g.finalize()
    _check(grid, want, BOUNDARY_SHAPE)
    assert np.array_equal(g.flag(dx, dy, dz, grid).cpu().numpy(), want["flags"])


def test_one_cell_and_runs(gpu_device):
    """200 000 soundings in one cell of an 8 x 8 grid, added in three chunks (the radix path, 782 tiles a pass), and equal-cell
    runs of lengths 1 .. 130 laid end to end (the stage is positional: runs cost nothing and change nothing)."""
    rng = np.random.default_rng(4)
    n = 200000
    x = 3.0 + rng.uniform(0.0, 1.0, n)
    y = 8.0 - (5.0 + rng.uniform(0.001, 1.0, n))
    z = (-120.0 + 30.0 * rng.standard_normal(n)).astype(np.float32)
    z[rng.integers(0, n, 300)] += np.float32(900.0)
    want = rc.grid(x, y, z, (8, 8), (0.0, 8.0), 1.0)
    assert want["count"][5, 3] == n == want["counters"]["accepted"] and n // 2 < want["kept"][5, 3] < n
    g = _gridder(gpu_device, (8, 8), (0.0, 8.0), 1.0, n)
    dx, dy, dz = _dev(gpu_device, x, y, z)
    for lo, hi in ((0, 70001), (70001, 70002), (70002, n)):
        g.add(dx[lo:hi], dy[lo:hi], dz[lo:hi])
    grid = g.finalize()
    _check(grid, want, (8, 8))
    assert np.array_equal(g.flag(dx, dy, dz, grid).cpu().numpy(), want["flags"])

    x, y, z = sc.runs_cloud()
    want = rc.grid(x, y, z, (8, 8), (0.0, 8.0), 1.0, k=2.0, min_count=2)
    assert want["counters"]["accepted"] == z.size and int((want["count"] > 0).sum()) == 64
    g = _gridder(gpu_device, (8, 8), (0.0, 8.0), 1.0, z.size, k=2.0, min_count=2)
    g.add(*_dev(gpu_device, x, y, z))
    _check(g.finalize(), want, (8, 8))


def test_order_chunks_repeats(gpu_device):
    """The mixed cloud in one call, in seven ragged chunks (one empty, one of a single sounding), permuted, and twice over into
    fresh stages: equal bits in everything finalize returns, and equal counters.  finalize, add, finalize equals adding it all
    first; the flags of a permuted cloud are the permuted flags."""
    x, y, z = sc.mixed_cloud()
    new = lambda: _gridder(gpu_device, sc.MIXED_SHAPE, sc.MIXED_ORIGIN, sc.MIXED_RES, 20000)
    dx, dy, dz = _dev(gpu_device, x, y, z)
    runs = []
    for _ in range(2):                                           # twice over into fresh stages
        g = new(); g.add(dx, dy, dz); runs.append(g.finalize())
    cuts = [0, 1, 1, 4097, 4352, 9999, 16000, 20000]             # chunks of 1, 0, 4096, 255, 5647, 6001, 4000
    g = new()
    for lo, hi in zip(cuts[:-1], cuts[1:]):
        g.add(dx[lo:hi], dy[lo:hi], dz[lo:hi])
    assert g.offered == 20000
    runs.append(g.finalize())
    perm = torch.from_numpy(np.random.default_rng(9).permutation(z.size)).to(gpu_device)
    g = new(); g.add(dx[perm], dy[perm], dz[perm]); runs.append(g.finalize())
    flags = g.flag(dx, dy, dz, runs[0])
    assert torch.equal(g.flag(dx[perm], dy[perm], dz[perm], runs[-1]), flags[perm])
    assert np.array_equal(flags.cpu().numpy(), rc.mixed_want()["flags"])
    g = new(); g.add(dx[:7001], dy[:7001], dz[:7001])
    first = g.finalize()
    first_host = _host(first)                                    # (taken before the second finalize: each returns tensors of its own)
    g.add(dx[7001:], dy[7001:], dz[7001:])
    runs.append(g.finalize())
    ref = _host(runs[0])
    for r in runs[1:]:
        _same_bits(_host(r), ref)
        assert r.counters == runs[0].counters
    _check(runs[0], rc.mixed_want(), sc.MIXED_SHAPE)
    want_first = rc.grid(x[:7001], y[:7001], z[:7001], sc.MIXED_SHAPE, sc.MIXED_ORIGIN, sc.MIXED_RES)
    _check(first, want_first, sc.MIXED_SHAPE)                    # (and the planes of the first finalize were, and stay, its own)
    _same_bits(_host(first), first_host)
    g.reset()
    assert g.offered == 0 and g.counters()["accepted"] == 0 and int(g.finalize().count.sum()) == 0


def test_against_the_first_gridder(gpu_device):
    """count equals SoundingGridder's on the same cloud; with floor_m = 65536 every sounding is kept and kept_mean, kept_std
    equal its mean and std bit for bit."""
    from bathymetric_gnn_amd.data import SoundingGridder
    x, y, z = sc.mixed_cloud()
    dx, dy, dz = _dev(gpu_device, x, y, z)
    for min_count in (1, 3):
        first = SoundingGridder(sc.MIXED_SHAPE, sc.MIXED_ORIGIN, sc.MIXED_RES, device=gpu_device, min_count=min_count)
        first.add(dx, dy, dz)
        a = first.finalize()
        g = _gridder(gpu_device, sc.MIXED_SHAPE, sc.MIXED_ORIGIN, sc.MIXED_RES, 20000, floor_m=65536.0, min_count=min_count)
        g.add(dx, dy, dz)
        b = g.finalize()
        assert a.counters == b.counters
        assert torch.equal(a.count, b.count) and torch.equal(b.kept, b.count) and torch.equal(a.valid, b.valid)
        assert torch.equal(a.mean.view(torch.int32), b.kept_mean.view(torch.int32))
        assert torch.equal(a.std.view(torch.int32), b.kept_std.view(torch.int32))
        assert int((g.flag(dx, dy, dz, b) == 1).sum()) == 0
        tight = _gridder(gpu_device, sc.MIXED_SHAPE, sc.MIXED_ORIGIN, sc.MIXED_RES, 20000, min_count=min_count)
        tight.add(dx, dy, dz)
        assert torch.equal(tight.finalize().count, a.count)


def test_flags_of_soundings_the_grid_never_saw(gpu_device):
    """The flag pass is stateless: soundings that were never added are judged by the rule of their cell -- 1 in a cell that
    finalize saw empty, 2 where they are not accepted, 0 / 1 by the limit elsewhere."""
    g = _gridder(gpu_device, (2, 3), (0.0, 2.0), 1.0, 16)
    x = np.array([0.5, 0.6, 0.7, 0.4, 0.3, 2.5], np.float64)
    y = np.array([1.5, 1.5, 1.5, 1.5, 1.5, 0.5], np.float64)
    z = np.array([-10.0, -10.5, -11.0, -10.25, -10.75, -3.0], np.float32)        # five in cell (0, 0), one in cell (1, 2)
    g.add(*_dev(gpu_device, x, y, z))
    grid = g.finalize()
    want = rc.grid(x, y, z, (2, 3), (0.0, 2.0), 1.0)
    _check(grid, want, (2, 3))
    assert want["limit"].reshape(-1).tolist() == [int(3 * 1.4826 * 0.25 * 131072), -1, -1, -1, -1, 0]
    nx = np.array([0.1, 0.2, 0.9, 1.5, 2.5, 2.5, 7.0, 0.5, np.nan, 0.5], np.float64)
    ny = np.array([1.9, 1.1, 1.5, 1.5, 0.5, 0.5, 0.5, -0.1, 0.5, 1.5], np.float64)
    nz = np.array([-10.5, -12.0, -9.0, -10.5, -3.0, -3.00002, -3.0, -3.0, -3.0, np.inf], np.float32)
    got = g.flag(*_dev(gpu_device, nx, ny, nz), grid).cpu().numpy()
    assert got.tolist() == [0, 1, 1, 1, 0, 1, 2, 2, 2, 2]
    assert np.array_equal(got, rc.flags(nx, ny, nz, (2, 3), (0.0, 2.0), 1.0, want["center2"], want["limit"]))
    assert g.flag(*_dev(gpu_device, nx[:0], ny[:0], nz[:0]), grid).numel() == 0
    other = _gridder(gpu_device, (2, 4), (0.0, 2.0), 1.0, 16)
    with pytest.raises(ValueError, match="geometry"):
        other.flag(*_dev(gpu_device, nx, ny, nz), grid)


def test_refusals_before_any_launch(gpu_device):
    g = _gridder(gpu_device, (4, 4), (0.0, 4.0), 1.0, 3)
    x, y, z = _dev(gpu_device, np.array([0.5, 1.5]), np.array([3.5, 3.5]), np.array([-1.0, -2.0], np.float32))
    with pytest.raises(TypeError, match="float64"):
        g.add(x.float(), y, z)
    with pytest.raises(TypeError, match="float32"):
        g.add(x, y, z.double())
    g.add(x, y, z)
    with pytest.raises(ValueError, match="more than the capacity of 3"):
        g.add(x, y, z)
    assert g.offered == 2 and g.counters() == dict(accepted=2, nonfinite=0, outside=0, out_of_range=0)
    g.add(x[:1], y[:1], z[:1])
    assert int(g.finalize().count.sum()) == 3
    for bad in (dict(shape=(0, 4)), dict(resolution=0.0), dict(min_count=0), dict(origin=(0.0, float("inf"))), dict(capacity=0),
                dict(k=0.99), dict(k=float("nan")), dict(floor_m=-1.0), dict(floor_m=float("inf")), dict(capacity=2 ** 31)):
        kw = dict(shape=(4, 4), origin=(0.0, 4.0), resolution=1.0, capacity=8, device=gpu_device)
        kw.update(bad)
        with pytest.raises(ValueError):
            from bathymetric_gnn_amd.data import RobustSoundingGridder
            RobustSoundingGridder(**kw)
    with pytest.raises(NotImplementedError):
        _gridder(gpu_device, (2 ** 16, 2 ** 15), (0.0, 0.0), 1.0, 8)


def test_far_corner_of_a_large_grid(gpu_device):
    """10400 x 10400 cells: start and the planes are addressed past cell 2^26 (and the int64 planes past byte 2^29).  A few
    soundings in the first cell, in one past cell 2^26 and in the last one must land there and nowhere else."""
    H = W = 10400
    past = 2 ** 26 + 12345
    groups = {(0, 0): [-5.25, -7.5], (past // W, past % W): [-11.125], (H - 1, W - 1): [-3.0, -4.5, -9.75, -80.0]}
    assert past < H * W
    xs, ys, zs = [], [], []
    for (r, c), depths in groups.items():
        for j, d in enumerate(depths):
            xs.append(c + 0.2 + 0.2 * j); ys.append(H - r - 0.5); zs.append(d)
    x, y, z = np.array(xs, np.float64), np.array(ys, np.float64), np.array(zs, np.float32)
    g = _gridder(gpu_device, (H, W), (0.0, float(H)), 1.0, 16)
    dx, dy, dz = _dev(gpu_device, x, y, z)
    g.add(dx, dy, dz)
    grid = g.finalize()
    assert grid.counters == dict(accepted=7, nonfinite=0, outside=0, out_of_range=0)
    assert int(grid.count.sum(dtype=torch.int64)) == 7 and int(grid.valid.sum(dtype=torch.int64)) == 3
    assert int(grid.kept.sum(dtype=torch.int64)) == 6 and int((grid.limit >= 0).sum()) == 3
    start = grid.start
    assert int(start[0]) == 0 and int(start[1]) == 2 == int(start[past]) and int(start[past + 1]) == 3 == int(start[H * W - 1])
    assert int(start[H * W]) == 7 and int((start[1:] - start[:-1]).sum(dtype=torch.int64)) == 7
    for (r, c), depths in groups.items():
        sel = [i for i in range(z.size) if int(x[i]) == c and int(H - y[i]) == r]
        want = rc.grid(x[sel], y[sel], z[sel], (1, 1), (float(c), float(H - r)), 1.0)
        assert want["count"][0, 0] == len(depths)
        for k in rc.PLANES:
            got = getattr(grid, k)[r, c].cpu().numpy()
            assert got.tobytes() == want[k][0, 0].tobytes(), (r, c, k)
        assert np.array_equal(grid.cell_soundings(r, c).cpu().numpy(), want["sorted_q"].astype(np.float64) / 65536.0)
    assert g.flag(dx, dy, dz, grid).cpu().numpy().tolist() == [0, 0, 0, 0, 0, 0, 1]


def test_hand_over_to_the_pipeline(gpu_device):
    """survey_tensors("median", "mad") goes straight into process_survey_device (64 / 16 tiles, an 8-channel model, so the MAD is
    used as the uncertainty band); the result equals to_grid("median", "mad") sent through process_grid_device bit for bit."""
    from bathymetric_gnn_amd import synthetic
    from bathymetric_gnn_amd.config import Config
    from bathymetric_gnn_amd.data import grid_soundings_robust
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
    z[rng.integers(0, z.size, z.size // 50)] += np.float32(4.0)  # fliers that the mean follows and the median does not
    grid = grid_soundings_robust(*_dev(gpu_device, x, y, z), res, shape=(H, W), origin=(x0, y0), min_count=2)
    valid = grid.valid.cpu().numpy()
    assert 0.5 < valid.mean() < 0.95 and grid.counters["outside"] == 0
    assert int((grid.count - grid.kept).sum()) > z.size // 100
    cfg = Config(); cfg.tile.tile_size, cfg.tile.overlap = 64, 16
    pipe = BathymetricPipeline(cfg, tile_batch=7)
    sd = synthetic.synthetic_state_dict(in_channels=8, seed=1234)
    m = BathymetricGNN(in_channels=8, edge_dim=3, dropout=0.0); m.load_state_dict({k: torch.as_tensor(v) for k, v in sd.items()})
    pipe.set_model(m.to(gpu_device).eval())
    depth_t, valid_t, unc_t = grid.survey_tensors("median", "mad")
    assert depth_t is grid.median and valid_t is grid.valid and unc_t is grid.mad
    out = pipe.process_survey_device(depth_t, valid_t, unc_t, grid.resolution).cpu().numpy()
    host = grid.to_grid("median", "mad")
    assert np.array_equal(host.depth, grid.median.cpu().numpy()) and np.array_equal(host.uncertainty, grid.mad.cpu().numpy())
    assert np.array_equal(host.valid_mask, valid.astype(bool)) and host.nodata_value == 1.0e6
    assert host.transform == (x0, res, 0.0, y0, 0.0, -res) and host.resolution == (res, res)
    assert host.bounds == (x0, y0 - H * res, x0 + W * res, y0)
    via_host = pipe.process_grid_device(host)
    for k, name in enumerate(("classification", "confidence", "correction", "cleaned_depth")):
        assert np.array_equal(via_host[name].view(np.uint32), out[k].view(np.uint32)), name
    assert grid.survey_tensors()[0] is grid.median and grid.survey_tensors()[2] is grid.kept_std
    for depth in ("kept_mean", "kept_min", "kept_max"):
        assert grid.survey_tensors(depth, "kept_std")[0] is getattr(grid, depth)
    v = valid.astype(bool)
    lo, mid, hi = (getattr(grid, k).cpu().numpy()[v] for k in ("kept_min", "median", "kept_max"))
    assert (lo <= mid).all() and (mid <= hi).all() and (lo < hi).any()
    with pytest.raises(ValueError):
        grid.survey_tensors("mean")
    with pytest.raises(ValueError):
        grid.survey_tensors("median", "std")
