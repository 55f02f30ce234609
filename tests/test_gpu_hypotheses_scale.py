"""The depth hypotheses past one launch grid (csrc/sounding_hypotheses.hip) against the restatement of _hypotheses_cpu.py, for equal
bits.  test_gpu_hypotheses.py is careful about values and makes one trip through every grid-stride loop; here the sizes are chosen
so that each loop makes a second trip:

  * the cloud of test_gpu_soundings_scale.py (N = 2048 * 1024 + 3 * 1024 + 37 soundings on 48 x 64 cells) with its 2528 cells of
    more than 64 soundings: the 1024 walkers of hyp_count_long / hyp_choose_long take two cells each and walkers 0 .. 479 a third;
    128 of the cells have more than 4096 soundings, so a thread's share is 17 or 18 positions there and 1 .. 16 in the rest;
  * a dense grid of 1100 x 1000 cells: 4297 workgroups' worth of cells over the 2048 of hyp_count_short / hyp_choose_short (a
    third trip in workgroups 0 .. 200), and 269 scan tiles, so scan_tile_sums carries the hyp_start scan over its first 256.

The restatement of the large cloud walks every sounding as a Python integer (seconds); it is computed once per module."""
import functools

import numpy as np
import pytest
import torch

import _hypotheses_cpu as hc
import _robust_cpu as rc
import test_gpu_soundings_scale as ss

pytestmark = pytest.mark.gpu

# the device constants that the sizes follow from: a change of one of them makes the comment stale, and the size with it
MAX_GRID = 2048                # PLANE_MAX_GRID (plane_util.h): the grid cap of hyp_count_short, hyp_choose_short and the scan kernels
THREADS = 256                  # HY_THREADS: cells per workgroup and trip of the per-cell kernels; the shares of a long cell
LONG_GRID = 1024               # HY_LONG_GRID: the workgroups that walk the list of long cells
SCAN_TILE = 4096               # HY_SCAN_TILE: cells per tile of hyp_tile_sums / hyp_scan_cells
SCAN_SUMS_STEP = 256           # BLOCK_THREADS: tiles per step of scan_tile_sums
WAVE_MAX = 64                  # BGNN_ROBUST_WAVE_MAX: the longest cell that one thread walks

GAP_M = 0.05                   # 3 to 37 hypotheses in a long cell of the cloud, 5 and more in every cell of more than 4096


def _differ(got, want):
    return ss._differ(got, want)


def _host(hyp):
    out = {k: getattr(hyp, k).cpu().numpy() for k in hc.PLANES}
    out["ambiguity"] = hyp.ambiguity_plane().cpu().numpy()
    if hyp.hyp_start is not None:
        out["hyp_start"] = hyp.hyp_start.cpu().numpy().view(np.uint32).astype(np.int64)
        total = int(out["hyp_start"][-1])
        out["hyp_first"] = hyp.hyp_first.cpu().numpy().view(np.uint32).astype(np.int64)[:total]
        out["hyp_count"] = hyp.hyp_count.cpu().numpy()[:total]
    return out


def _check(got, want, records=True):
    for k in hc.PLANES + ("ambiguity",):
        assert got[k].shape == want[k].shape and got[k].dtype == want[k].dtype, k
        d = _differ(got[k], want[k])
        assert d.size == 0, (k, d.size, d[:4], got[k].reshape(-1)[d[:4]], want[k].reshape(-1)[d[:4]])
    if records:
        for k in hc.RECORDS:
            assert got[k].dtype == want[k].dtype and np.array_equal(got[k], want[k]), k


def _guide():
    """The robust median (nodata where a cell is not valid: the count key there), 4 m up in every third cell: at the fliers."""
    guide = ss._want_robust()["median"].copy()
    guide.reshape(-1)[::3] += np.float32(4.0)
    return guide


@functools.lru_cache(maxsize=None)
def _want(rule):
    robust = ss._want_robust()
    want = hc.grid(robust, GAP_M, rule, _guide() if rule == "guide" else None, ss.MIN_COUNT)
    n, n_hyp = robust["count"].reshape(-1), want["n_hyp"].reshape(-1)
    assert int((n > WAVE_MAX).sum()) > 2 * LONG_GRID and int((n > 16 * THREADS).sum()) >= 128
    assert int(n_hyp[n > WAVE_MAX].min()) >= 1 and int(n_hyp[n > WAVE_MAX].max()) > 8 and int((n_hyp[n > 16 * THREADS] > 4).sum()) > 64
    assert (want["valid"] == 0).any() and (want["chosen"] > 0).any() and int(want["hyp_start"][-1]) > 20000
    return want


def test_long_list_past_one_grid(gpu_device):
    """2528 listed cells over 1024 list walkers, by count and by guide, with and without records, and twice over: the list is
    rebuilt in another order every time, and nothing may depend on it."""
    from bathymetric_gnn_amd.data import RobustSoundingGridder
    want = _want("count")
    x, y, z = ss._layout_of("swath")
    g = RobustSoundingGridder(ss.SHAPE, ss.ORIGIN, ss.RES, ss.N, device=gpu_device, min_count=ss.MIN_COUNT)
    dx, dy, dz = ss._dev(gpu_device, x, y, z)
    g.add(dx, dy, dz)
    grid = g.finalize()
    hyp = grid.hypotheses(GAP_M)
    assert hyp.min_count == ss.MIN_COUNT
    a = _host(hyp)
    _check(a, want)
    again = _host(grid.hypotheses(GAP_M))
    assert a.keys() == again.keys() and all(a[k].tobytes() == again[k].tobytes() for k in a)
    bare = _host(grid.hypotheses(GAP_M, records=False))
    _check(bare, want, records=False)
    flags = g.flag(dx, dy, dz, hyp).cpu().numpy()
    assert np.array_equal(flags, rc.flags(x, y, z, ss.SHAPE, ss.ORIGIN, ss.RES, want["center2"], want["limit"]))
    wg = _want("guide")
    assert (wg["chosen"] != want["chosen"]).sum() > 100
    _check(_host(grid.hypotheses(GAP_M, rule="guide", guide=torch.from_numpy(_guide()).to(gpu_device))), wg)


def test_dense_grid_past_two_trips_and_256_scan_tiles(gpu_device):
    """2.2 x 10^6 soundings over 1 100 000 cells (the short class only).  ``n_hyp`` and all of the records against numpy on the
    sorted lists; the other planes against the restatement on the cells around every scan-tile border, around every trip
    border of the per-cell kernels, and every 53rd."""
    from bathymetric_gnn_amd.data import RobustSoundingGridder
    (H, W), (x0, y0), res, N = ss.DENSE_SHAPE, ss.ORIGIN, 0.5, ss.DENSE_N
    cells = H * W
    trip = MAX_GRID * THREADS
    assert cells > 2 * trip and -(-cells // SCAN_TILE) > SCAN_SUMS_STEP
    rng = np.random.default_rng(31)
    x = x0 + rng.uniform(0.0, W * res, N)
    y = y0 - rng.uniform(0.0, H * res, N)
    z = (-30.0 + 0.01 * (x - x0) + 0.2 * rng.standard_normal(N)).astype(np.float32)
    z[rng.random(N) < 0.05] += np.float32(4.0)
    cell, q, counters = rc.stage(x, y, z, ss.DENSE_SHAPE, ss.ORIGIN, res)
    acc = cell >= 0
    c, qa = cell[acc], q[acc]
    order = np.lexsort((qa, c))
    c, sorted_q = c[order], qa[order]
    count = np.bincount(c, minlength=cells)
    start = np.concatenate([[0], np.cumsum(count)]).astype(np.int64)
    assert count.max() <= WAVE_MAX
    # the runs of every cell at once: a run begins at the first sounding of a cell and after every break
    gap_q = hc.gap_q_of(GAP_M)
    begins = np.ones(c.size, bool)
    begins[1:] = (c[1:] != c[:-1]) | (sorted_q[1:] - sorted_q[:-1] > gap_q)
    first = np.flatnonzero(begins)
    n_hyp = np.bincount(c[first], minlength=cells)
    hyp_start = np.concatenate([[0], np.cumsum(n_hyp)]).astype(np.int64)
    hyp_count = np.diff(np.concatenate([first, [c.size]])).astype(np.int32)
    tile_sums = np.add.reduceat(n_hyp, np.arange(0, cells, SCAN_TILE))
    assert tile_sums.min() > 0 and n_hyp.max() >= 4 and first.size > cells       # hypotheses in every scan tile

    g = RobustSoundingGridder(ss.DENSE_SHAPE, ss.ORIGIN, res, N, device=gpu_device)
    g.add(*ss._dev(gpu_device, x, y, z))
    grid = g.finalize()
    assert grid.counters == counters
    hyp = grid.hypotheses(GAP_M)
    got = _host(hyp)
    assert np.array_equal(got["n_hyp"].reshape(-1), n_hyp)
    assert np.array_equal(got["hyp_start"], hyp_start) and np.array_equal(got["hyp_first"], first) and np.array_equal(got["hyp_count"], hyp_count)

    near = lambda step: (np.arange(0, cells + step, step)[:, None] + np.arange(-2, 3)[None, :]).reshape(-1)
    subset = np.unique(np.concatenate([near(SCAN_TILE), near(SCAN_TILE * SCAN_SUMS_STEP), near(trip), [0, cells - 1], np.arange(0, cells, 53)]))
    subset = subset[(subset >= 0) & (subset < cells)]
    assert subset.size >= 20000 and {trip - 1, trip, 2 * trip - 1, 2 * trip, cells - 1} <= set(subset.tolist())
    part = {"count": count[subset].astype(np.int32).reshape(1, -1),
            "start": np.concatenate([[0], np.cumsum(count[subset])]).astype(np.int64),
            "sorted_q": np.concatenate([sorted_q[start[i]:start[i + 1]] for i in subset]).astype(np.int32)}
    want = hc.grid(part, GAP_M)
    assert int((want["n_hyp"] > 1).sum()) > 1000 and int((want["n_hyp"] == 0).sum()) > 100
    for k in hc.PLANES + ("ambiguity",):
        d = _differ(got[k].reshape(-1)[subset], want[k].reshape(-1))
        assert d.size == 0, (k, d.size, subset[d[:4]])
    bare = _host(grid.hypotheses(GAP_M, records=False))
    assert all(bare[k].tobytes() == got[k].tobytes() for k in bare)
