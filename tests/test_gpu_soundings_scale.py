"""The sounding gridders past one launch grid (csrc/sounding_grid.hip, sounding_robust.hip, sounding_vr.hip) against the
restatements of _soundings_cpu.py, _robust_cpu.py and _vr_soundings_cpu.py, for equal bits.  The other sounding suites are careful
about values and make one trip through every grid-stride loop; here the sizes are chosen so that each loop makes a second trip:

  * one cloud of N = 2048 * 1024 + 3 * 1024 + 37 soundings in one call: workgroups 0 .. 3 of the six
    instantiations of sounding_pass (sounding_pass.h) and of vr_stage take two tiles (workgroup 3 a ragged one of 37), the other 2044 take one;
    robust_count and robust_scatter (256 slots a trip, 2048 workgroups) make five trips in workgroups 0 .. 12 and four in the rest;
  * its 2528 cells of more than 64 soundings: the 1024 walkers of robust_sort_long / robust_stats_long take two segments each and
    walkers 0 .. 479 a third, the radix class and the bitonic class in arrival order;
  * a dense grid of 1100 x 1000 cells: 269 scan tiles with non-zero counts, so scan_tile_sums carries over its first 256;
  * a three-call split whose first call is itself past one grid, so ``offered`` > 0 sits behind a strided call.

The restatement of the large cloud walks every sounding as a Python integer (seconds); it is computed once per module."""
import functools

import numpy as np
import pytest
import torch

import _robust_cpu as rc
import _soundings_cpu as sc
import _vr_soundings_cpu as vc

pytestmark = pytest.mark.gpu

# the device constants that the sizes follow from: a change of one of them makes the comment stale, and the size with it
TILE = 1024                    # SG_TILE, RB_TILE, VR_TILE: 4 soundings x 256 threads a trip (sounding_grid / _robust / _vr.hip)
MAX_GRID = 2048                # PLANE_MAX_GRID (plane_util.h): the grid cap of the kernels that stride
SLOT_TRIP = 256                # RB_THREADS: slots per workgroup and trip of robust_count and robust_scatter
LONG_GRID = 1024               # RB_LONG_GRID: the workgroups that walk the list of long segments
SCAN_TILE = 4096               # RB_SCAN_TILE: cells per tile of robust_tile_sums / robust_scan_cells
SCAN_SUMS_STEP = 256           # RB_THREADS: tiles per step of scan_tile_sums
WAVE_MAX, LDS_MAX = 64, 4096   # BGNN_ROBUST_WAVE_MAX, BGNN_ROBUST_LDS_MAX (checked against the runtime's below)

N = MAX_GRID * TILE + 3 * TILE + 37
SHAPE, ORIGIN, RES = (48, 64), (500000.0, 4000000.0), 0.5
MIN_COUNT = 3
BIG_CELLS, MID_CELLS = 128, 2400                                    # more than LDS_MAX soundings; 65 .. LDS_MAX
PLAIN = ("count", "mean", "std", "min", "max", "valid")


def _dev(device, *arrays):
    return [torch.from_numpy(np.array(a)).to(device) for a in arrays]           # (a copy: the shared clouds are read-only)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


def _differ(got, want):
    """The flat indices of the elements whose bits differ."""
    return np.flatnonzero((_bits(got).reshape(got.size, -1) != _bits(want).reshape(want.size, -1)).any(axis=1))


def _check_planes(got, want, names, shape):
    for k in names:
        assert got[k].shape == tuple(shape) and got[k].dtype == want[k].dtype, k
        d = _differ(got[k], want[k].reshape(shape))
        assert d.size == 0, (k, d.size, d[:4], got[k].reshape(-1)[d[:4]], want[k].reshape(-1)[d[:4]])


def _host_plain(grid):
    return {k: getattr(grid, k).cpu().numpy() for k in PLAIN}


def _host_robust(grid):
    out = {k: getattr(grid, k).cpu().numpy() for k in rc.PLANES}
    out["start"] = grid.start.cpu().numpy().view(np.uint32).astype(np.int64)
    out["sorted_q"] = grid.sorted_q.cpu().numpy()[:int(out["start"][-1])]
    return out


def _check_robust(grid, want, shape):
    got = _host_robust(grid)
    assert grid.counters == want["counters"]
    _check_planes(got, want, rc.PLANES, shape)
    for k in ("start", "sorted_q"):
        assert np.array_equal(got[k], want[k]), k
    return got


def _same_bits(a, b):
    assert a.keys() == b.keys()
    for k in a:
        assert a[k].tobytes() == b[k].tobytes(), k


def _busy(device):
    """Work left pending on the stream: what follows is queued behind it."""
    a = torch.ones(2048, 2048, device=device)
    for _ in range(8):
        a = (a @ a) * (1.0 / 2048.0)
    return a


# ---- the cloud past one grid ------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _cloud():
    """``(x, y, z)`` in swath order (sorted by cell, so that runs of one cell cross wave, tile and trip boundaries) and the planned
    soundings per cell.  128 cells of 4097 .. 4400, 2400 cells of 65 .. about 1200, 544 of 0 .. 64 (0, 1, 2, 63 and 64 among
    them), the classes scattered over the grid; every fiftieth sounding is planted outside, non-finite or out of range."""
    rng = np.random.default_rng(23)
    (H, W), (x0, y0) = SHAPE, ORIGIN
    cells = H * W
    bad_at = np.arange(7, N, 50)
    accepted = N - bad_at.size
    big = LDS_MAX + 1 + rng.integers(0, 304, BIG_CELLS)
    short = np.concatenate([[0, 1, 2, 63, 64], rng.integers(0, WAVE_MAX + 1, cells - BIG_CELLS - MID_CELLS - 5)])
    rest = accepted - int(big.sum()) - int(short.sum()) - (WAVE_MAX + 1) * MID_CELLS
    w = rng.uniform(0.0, 1.0, MID_CELLS)
    mid = WAVE_MAX + 1 + np.floor(w / w.sum() * rest).astype(np.int64)
    mid[:rest - int((mid - WAVE_MAX - 1).sum())] += 1
    assert mid.min() > WAVE_MAX and mid.max() <= LDS_MAX
    counts = np.concatenate([big, mid, short])[rng.permutation(cells)]
    assert counts.sum() == accepted
    cell = np.repeat(np.arange(cells), counts)
    ax = x0 + (cell % W + rng.uniform(0.05, 0.95, accepted)) * RES
    ay = y0 - (cell // W + rng.uniform(0.05, 0.95, accepted)) * RES
    az = (-20.0 - 0.01 * cell + 0.3 * rng.standard_normal(accepted)).astype(np.float32)
    fliers = rng.random(accepted) < 0.03
    az[fliers] += rng.uniform(3.0, 6.0, int(fliers.sum())).astype(np.float32)
    nb = bad_at.size
    bx = x0 + rng.uniform(0.05, W - 0.05, nb) * RES
    by = y0 - rng.uniform(0.05, H - 0.05, nb) * RES
    bz = (-20.0 + rng.standard_normal(nb)).astype(np.float32)
    kind = np.arange(nb) % 8
    bx[kind == 0] = x0 - 1.3
    by[kind == 1] = y0 - H * RES - 0.7
    bx[kind == 2] = np.nan
    bz[kind == 3] = np.inf
    bz[kind == 4] = 40000.0
    by[kind == 5] = -np.inf
    bz[kind == 6] = -32768.0
    bx[kind == 7] = x0 + W * RES + 0.2
    x, y, z = np.empty(N), np.empty(N), np.empty(N, np.float32)
    good = np.ones(N, bool)
    good[bad_at] = False
    x[good], y[good], z[good] = ax, ay, az
    x[bad_at], y[bad_at], z[bad_at] = bx, by, bz
    return sc._frozen(x, y, z) + (counts.reshape(H, W),)


@functools.lru_cache(maxsize=None)
def _perm():
    p = np.random.default_rng(29).permutation(N)
    p.setflags(write=False)
    return p


def _layout_of(name):
    x, y, z, _ = _cloud()
    if name == "swath":
        return x, y, z
    p = _perm()
    return x[p], y[p], z[p]


@functools.lru_cache(maxsize=None)
def _want_plain():
    x, y, z, _ = _cloud()
    return sc.grid(x, y, z, SHAPE, ORIGIN, RES, min_count=MIN_COUNT)


@functools.lru_cache(maxsize=None)
def _want_robust():
    """rc.grid of the whole cloud (swath order; the planes, ``start`` and ``sorted_q`` do not depend on the order), and the
    conditions the cloud was planned for, asserted before anything runs on the device."""
    from bathymetric_gnn_amd import runtime as rt
    assert (rt.ROBUST_WAVE_MAX, rt.ROBUST_LDS_MAX) == (WAVE_MAX, LDS_MAX)
    x, y, z, counts = _cloud()
    want = rc.grid(x, y, z, SHAPE, ORIGIN, RES, min_count=MIN_COUNT)
    n = want["count"].reshape(-1)
    assert z.size == N > MAX_GRID * TILE and np.array_equal(want["count"], counts)
    assert int((n > WAVE_MAX).sum()) > 2 * LONG_GRID                             # every walker: at least two segments, some three
    assert int((n > LDS_MAX).sum()) >= 128 and int(((n > WAVE_MAX) & (n <= LDS_MAX)).sum()) >= 1024
    assert {0, 1, 2, 63, 64} <= set(n.tolist())
    assert all(v > 0 for v in want["counters"].values()) and sum(want["counters"].values()) == N
    assert N - want["counters"]["accepted"] == len(range(7, N, 50))
    assert int((want["kept"] < want["count"]).sum()) > 1000 and (want["valid"] == 0).any()
    return want


def _plain_run(device, x, y, z, cuts=(0, N)):
    from bathymetric_gnn_amd.data import SoundingGridder
    g = SoundingGridder(SHAPE, ORIGIN, RES, device=device, min_count=MIN_COUNT)
    dx, dy, dz = _dev(device, x, y, z)
    for lo, hi in zip(cuts[:-1], cuts[1:]):
        g.add(dx[lo:hi], dy[lo:hi], dz[lo:hi])
    assert g.offered == N
    return g.finalize()


def _robust_run(device, x, y, z, cuts=(0, N)):
    """``(grid, flags)`` of the cloud added in the calls that ``cuts`` sets; the flags of the whole cloud in one call."""
    from bathymetric_gnn_amd.data import RobustSoundingGridder
    g = RobustSoundingGridder(SHAPE, ORIGIN, RES, N, device=device, min_count=MIN_COUNT)
    dx, dy, dz = _dev(device, x, y, z)
    for lo, hi in zip(cuts[:-1], cuts[1:]):
        g.add(dx[lo:hi], dy[lo:hi], dz[lo:hi])
    assert g.offered == N
    grid = g.finalize()
    return grid, g.flag(dx, dy, dz, grid).cpu().numpy()


@pytest.mark.parametrize("layout", ["swath", "permuted"])
def test_first_gridder_past_one_grid(layout, gpu_device):
    """sounding_pass<UniformAddress, FileSink>: 2051 tiles and the ragged 37 over 2048 workgroups, in one call; swath order is
    where file_sounding merges runs across the boundaries."""
    want = _want_plain()
    _want_robust()                                                               # (the conditions of the cloud)
    grid = _plain_run(gpu_device, *_layout_of(layout))
    assert grid.counters == want["counters"]
    _check_planes(_host_plain(grid), want, PLAIN, SHAPE)


def test_robust_gridder_past_one_grid(gpu_device):
    """sounding_pass with StageSink and FlagSink, robust_count and robust_scatter past one grid; 2528 listed cells over 1024 list
    walkers.  Swath order against rc.grid, the permuted cloud against it and against the swath run."""
    want = _want_robust()
    grid, flags = _robust_run(gpu_device, *_layout_of("swath"))
    a = _check_robust(grid, want, SHAPE)
    assert flags.dtype == np.uint8 and np.array_equal(flags, want["flags"])
    assert int((flags == 1).sum()) == int((want["count"].astype(np.int64) - want["kept"]).sum()) > 0
    grid_p, flags_p = _robust_run(gpu_device, *_layout_of("permuted"))
    _same_bits(_check_robust(grid_p, want, SHAPE), a)
    assert np.array_equal(flags_p, want["flags"][_perm()])


def test_three_calls_the_first_past_one_grid(gpu_device):
    """A first call of 2048 * 1024 + 1500 soundings (two trips in workgroups 0 and 1), one sounding, the rest: ``offered`` > 0
    behind a strided call.  Both gridders against the restatements, which is what the one-call form equals."""
    cuts = (0, MAX_GRID * TILE + 1500, MAX_GRID * TILE + 1501, N)
    x, y, z = _layout_of("permuted")
    grid = _plain_run(gpu_device, x, y, z, cuts)
    assert grid.counters == _want_plain()["counters"]
    _check_planes(_host_plain(grid), _want_plain(), PLAIN, SHAPE)
    want = _want_robust()
    grid_r, flags = _robust_run(gpu_device, x, y, z, cuts)
    _check_robust(grid_r, want, SHAPE)
    assert np.array_equal(flags, want["flags"][_perm()])


def test_behind_pending_work_and_twice_over(gpu_device):
    """Two runs into fresh state, each queued behind unfinished work on the stream: equal bits, and the restatement's."""
    x, y, z = _layout_of("swath")
    runs = []
    for _ in range(2):
        busy = _busy(gpu_device)
        plain = _plain_run(gpu_device, x, y, z)
        busy = busy + _busy(gpu_device)
        robust, flags = _robust_run(gpu_device, x, y, z)
        assert torch.isfinite(busy).all()
        runs.append((_host_plain(plain), _host_robust(robust), flags))
    _same_bits(runs[0][0], runs[1][0])
    _same_bits(runs[0][1], runs[1][1])
    assert np.array_equal(runs[0][2], runs[1][2]) and np.array_equal(runs[0][2], _want_robust()["flags"])
    _check_planes(runs[0][0], _want_plain(), PLAIN, SHAPE)
    _check_planes(runs[0][1], _want_robust(), rc.PLANES, SHAPE)


# ---- a dense grid past 256 scan tiles -----------------------------------------------------------------------------------------------

DENSE_SHAPE, DENSE_N = (1100, 1000), 2200000


def test_dense_grid_past_256_scan_tiles(gpu_device):
    """2.2 x 10^6 soundings spread over 1 100 000 cells (0 to about 12 a cell: the short class only): 269 scan tiles, every one
    with counts, 13 of them behind the first step of scan_tile_sums.  ``count``, all of ``start`` and ``sorted_q`` against
    bincount, cumsum and lexsort; the other planes against rc's rule on the cells around every tile border and every 53rd."""
    from bathymetric_gnn_amd.data import RobustSoundingGridder, SoundingGridder
    (H, W), (x0, y0), res = DENSE_SHAPE, ORIGIN, 0.5
    cells = H * W
    n_tiles = -(-cells // SCAN_TILE)
    assert cells > SCAN_TILE * SCAN_SUMS_STEP and n_tiles > SCAN_SUMS_STEP
    rng = np.random.default_rng(31)
    x = x0 + rng.uniform(0.0, W * res, DENSE_N)
    y = y0 - rng.uniform(0.0, H * res, DENSE_N)
    z = (-30.0 + 0.01 * (x - x0) + 0.2 * rng.standard_normal(DENSE_N)).astype(np.float32)
    z[rng.random(DENSE_N) < 0.05] += np.float32(4.0)
    x[::1000] = x0 - 0.25                                                        # a few that no cell takes
    z[500::1000] = np.nan
    cell, q, counters = rc.stage(x, y, z, DENSE_SHAPE, ORIGIN, res)
    acc = cell >= 0
    c, qa = cell[acc], q[acc]
    count = np.bincount(c, minlength=cells)
    start = np.concatenate([[0], np.cumsum(count)]).astype(np.int64)
    sorted_q = qa[np.lexsort((qa, c))].astype(np.int32)
    assert count.max() <= WAVE_MAX and counters["outside"] > 0 and counters["nonfinite"] > 0
    tile_sums = np.add.reduceat(count, np.arange(0, cells, SCAN_TILE))
    assert tile_sums.size == n_tiles and tile_sums.min() > 0                     # non-zero counts in every scan tile

    g = RobustSoundingGridder(DENSE_SHAPE, ORIGIN, res, DENSE_N, device=gpu_device)
    dx, dy, dz = _dev(gpu_device, x, y, z)
    g.add(dx, dy, dz)
    grid = g.finalize()
    got = _host_robust(grid)
    assert grid.counters == counters
    assert np.array_equal(got["count"].reshape(-1), count)
    assert got["start"].size == cells + 1 and np.array_equal(got["start"], start)
    assert np.array_equal(got["sorted_q"], sorted_q)

    near = lambda step: (np.arange(0, cells + step, step)[:, None] + np.arange(-2, 3)[None, :]).reshape(-1)
    subset = np.unique(np.concatenate([near(SCAN_TILE), near(SCAN_TILE * SCAN_SUMS_STEP), [0, cells - 1], np.arange(0, cells, 53)]))
    subset = subset[(subset >= 0) & (subset < cells)]
    assert subset.size >= 20000 and {0, cells - 1, SCAN_TILE * SCAN_SUMS_STEP - 1, SCAN_TILE * SCAN_SUMS_STEP} <= set(subset.tolist())
    # rc.grid on the soundings of those cells alone, each cell a unit cell of a 1 x K grid
    place = np.full(cells, -1, np.int64)
    place[subset] = np.arange(subset.size)
    sel = np.flatnonzero(acc & (place[np.maximum(cell, 0)] >= 0))
    want = rc.grid(place[cell[sel]] + 0.5, np.full(sel.size, 0.5), z[sel], (1, subset.size), (0.0, 1.0), 1.0)
    assert want["counters"]["accepted"] == sel.size and np.array_equal(want["count"].reshape(-1), count[subset])
    assert int((want["kept"] < want["count"]).sum()) > 100 and int((want["count"] == 0).sum()) > 100
    for k in rc.PLANES:
        d = _differ(got[k].reshape(-1)[subset], want[k].reshape(-1))
        assert d.size == 0, (k, d.size, subset[d[:4]])

    first = SoundingGridder(DENSE_SHAPE, ORIGIN, res, device=gpu_device)
    first.add(dx, dy, dz)
    a = first.finalize()
    assert a.counters == grid.counters and torch.equal(a.count, grid.count)


# ---- the variable-resolution passes past one grid -----------------------------------------------------------------------------------

VR_B = 4.0                                                                       # 8 x 8 cells of the uniform grid per base cell
VR_BASE = (SHAPE[0] // 8, SHAPE[1] // 8)
VR_ORIGIN = (ORIGIN[0], ORIGIN[1] - SHAPE[0] * RES)                              # the south-west corner
_VR_DIMS = (0, 3, 5, 8, 11, 16, 2, 7)


@functools.lru_cache(maxsize=None)
def _vr_layout():
    """6 x 8 base cells of dimensions 0, 2, 3, 5, 7, 8, 11 and 16, two of them 3 x 5 and 5 x 3: 3164 records, six cells unrefined."""
    r, c = np.meshgrid(np.arange(VR_BASE[0]), np.arange(VR_BASE[1]), indexing="ij")
    dx = np.array(_VR_DIMS)[(3 * r + c) % len(_VR_DIMS)]
    dy = dx.copy()
    dy[0, 1], dy[0, 2] = 5, 3
    lay = vc.make_layout(VR_BASE, VR_ORIGIN, VR_B, dx, dy)
    assert 3000 < lay["total"] < 4000 and int((dx == 0).sum()) == 6
    return lay


def _device_layout(device, lay):
    from bathymetric_gnn_amd.data import VRLayout
    return VRLayout(lay["base_shape"], lay["origin"], lay["B"], lay["index"], lay["dx"], lay["dy"], lay["total"], device=device)


def test_vr_density_and_plan_past_one_grid(gpu_device):
    """sounding_pass<VRBaseAddress, DensitySink> over the cloud in one call: the counts of the planner and the layout of
    ``plan_vr_layout`` against the restatement's density and plan."""
    from bathymetric_gnn_amd.data import VRLayoutPlanner, plan_vr_layout
    x, y, z = _layout_of("permuted")
    counts = vc.density(x, y, z, VR_ORIGIN, VR_B, VR_BASE)
    want = _want_robust()["counters"]
    assert int(counts.sum()) == want["accepted"]
    dev = _dev(gpu_device, x, y, z)
    planner = VRLayoutPlanner(VR_BASE, VR_ORIGIN, VR_B, device=gpu_device)
    planner.add(*dev)
    assert np.array_equal(planner.counts().cpu().numpy(), counts)
    target, ladder = 700, (1, 2, 4, 8, 16)                                       # 28 598 .. 60 020 a base cell: grids of 4 and of 8
    index, d, total = vc.plan(counts, target, ladder)
    assert set(d.reshape(-1).tolist()) == {4, 8}
    layout = plan_vr_layout(*dev, VR_B, target_count=target, ladder=ladder, base_shape=VR_BASE, origin=VR_ORIGIN)
    assert layout.total == total and np.array_equal(layout.dx, d) and np.array_equal(layout.dy, d)
    assert np.array_equal(layout.index, index)


@pytest.mark.parametrize("layout", ["swath", "permuted"])
def test_vr_gridder_past_one_grid(layout, gpu_device):
    """sounding_pass<VRAddress, FileSink> over the cloud in one call on the mixed layout: every plane and the five counters against
    the restatement."""
    from bathymetric_gnn_amd.data import VRSoundingGridder
    lay = _vr_layout()
    x, y, z = _layout_of(layout)
    want = vc.grid(x, y, z, lay, min_count=MIN_COUNT)
    assert all(v > 0 for v in want["counters"].values()) and sum(want["counters"].values()) == N
    g = VRSoundingGridder(_device_layout(gpu_device, lay), min_count=MIN_COUNT)
    g.add(*_dev(gpu_device, x, y, z))
    grid = g.finalize()
    assert grid.counters == want["counters"] and g.offered == N
    _check_planes(_host_plain(grid), want, PLAIN, (lay["total"],))


def test_robust_vr_gridder_past_one_grid(gpu_device):
    """vr_stage, finalize and sounding_pass<VRAddress, FlagSink> over the cloud in one call on the mixed
    layout, against the restatement directly."""
    from bathymetric_gnn_amd.data import RobustVRSoundingGridder
    lay = _vr_layout()
    x, y, z = _layout_of("permuted")
    want = vc.robust_grid(x, y, z, lay, min_count=MIN_COUNT)
    assert all(v > 0 for v in want["counters"].values()) and int((want["count"] > LDS_MAX).sum()) >= 16
    g = RobustVRSoundingGridder(_device_layout(gpu_device, lay), N, min_count=MIN_COUNT)
    dx, dy, dz = _dev(gpu_device, x, y, z)
    g.add(dx, dy, dz)
    grid = g.finalize()
    assert g.offered == N
    _check_robust(grid, want, (lay["total"],))
    flags = g.flag(dx, dy, dz, grid).cpu().numpy()
    assert flags.dtype == np.uint8 and np.array_equal(flags, want["flags"])
    assert int((flags == 2).sum()) == N - want["counters"]["accepted"] and (flags == 1).any()


def test_robust_vr_gridder_against_the_uniform_grid(gpu_device):
    """The same three passes on the uniform layout of 2 x 2 grids at B = 1, where every record is a cell of part 1: the records are
    the cells of the uniform robust grid at resolution B / 2 (flipud, regrouped), which test_robust_gridder_past_one_grid holds
    to rc.grid; the flags are that grid's flags."""
    from bathymetric_gnn_amd.data import RobustVRSoundingGridder
    want = _want_robust()
    d, base = 2, (SHAPE[0] // 2, SHAPE[1] // 2)
    lay = vc.make_layout(base, VR_ORIGIN, RES * d, np.full(base, d), np.full(base, d))
    assert lay["total"] == SHAPE[0] * SHAPE[1]
    x, y, z = _layout_of("permuted")
    g = RobustVRSoundingGridder(_device_layout(gpu_device, lay), N, min_count=MIN_COUNT)
    dx, dy, dz = _dev(gpu_device, x, y, z)
    g.add(dx, dy, dz)
    grid = g.finalize()
    assert grid.counters == dict(want["counters"], unrefined=0)
    for k in rc.PLANES:
        w = vc.uniform_to_records(want[k], base, d)
        got = getattr(grid, k).cpu().numpy()
        assert got.shape == w.shape and got.dtype == w.dtype and _differ(got, w).size == 0, k
    assert int(grid.start.cpu().numpy().view(np.uint32)[-1]) == want["counters"]["accepted"]
    flags = g.flag(dx, dy, dz, grid).cpu().numpy()
    assert np.array_equal(flags, want["flags"][_perm()])


# ---- host arrays in more than one upload ------------------------------------------------------------------------------------------

def test_host_arrays_in_many_uploads(gpu_device, monkeypatch):
    """The 20 000-sounding mixed cloud as host arrays with an upload chunk of 4097 (five uploads, the last of 3612) through both
    gridders and the one-call form: equal bits to the device-tensor route and to the restatements.  (``flag`` takes device
    tensors only; it judges the grid that the uploads built.)"""
    from bathymetric_gnn_amd.data import RobustSoundingGridder, SoundingGridder, grid_soundings_robust
    from bathymetric_gnn_amd.data import sounding_grid
    monkeypatch.setattr(sounding_grid, "UPLOAD_CHUNK", 4097)
    x, y, z = (np.array(a) for a in sc.mixed_cloud())
    shape, origin, res = sc.MIXED_SHAPE, sc.MIXED_ORIGIN, sc.MIXED_RES
    dx, dy, dz = _dev(gpu_device, x, y, z)
    calls = []
    plain = {}
    for name, args in (("host", (x, y, z)), ("device", (dx, dy, dz))):
        g = SoundingGridder(shape, origin, res, device=gpu_device)
        add_device = g._add_device
        g._add_device = lambda *a, f=add_device: (calls.append(int(a[0].shape[0])), f(*a))[1]
        g.add(*args)
        assert g.offered == 20000
        plain[name] = g.finalize()
    assert calls == [4097, 4097, 4097, 4097, 3612, 20000]
    assert plain["host"].counters == sc.mixed_want(1)["counters"]
    _check_planes(_host_plain(plain["host"]), sc.mixed_want(1), PLAIN, shape)
    _same_bits(_host_plain(plain["host"]), _host_plain(plain["device"]))
    want = rc.mixed_want()
    robust = {}
    for name, args in (("host", (x, y, z)), ("device", (dx, dy, dz))):
        g = RobustSoundingGridder(shape, origin, res, 20000, device=gpu_device)
        g.add(*args)
        assert g.offered == 20000
        grid = g.finalize()
        robust[name] = _check_robust(grid, want, shape)
        assert np.array_equal(g.flag(dx, dy, dz, grid).cpu().numpy(), want["flags"])
    _same_bits(robust["host"], robust["device"])
    one = grid_soundings_robust(x, y, z, res, shape=shape, origin=origin, device=gpu_device)
    _same_bits(_check_robust(one, want, shape), robust["device"])
