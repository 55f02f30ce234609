"""Error percentiles past one launch grid (csrc/error_quantile.hip) against numpy, with the judges of test_gpu_error_quantile.py
(_quantile_cpu.py), for equal bits.  That suite's largest plane has 70 001 rows: one share per workgroup of qt_add, one chunk per
workgroup of the refine passes.  Here one ``add`` takes n = 2048 * 4096 + 3 * 4096 + 5 rows: 2052 shares over 2048 workgroups, so
workgroups 0 .. 3 take a second share (workgroup 3 a ragged one of 5 rows) through the loop-top barrier that keeps ``base`` and
``wave_total`` for the previous share's readers; with every row filed, the refine passes walk 8205 chunks of 1024 keys over 2048
workgroups, four or five trips each."""
import numpy as np
import pytest
import torch

from _quantile_cpu import PS, _check, _dev, _errors, _keys, _planes, _staged, _tracker

pytestmark = pytest.mark.gpu

# the device constants that the sizes follow from: a change of one of them makes the comment stale, and the size with it
WG_ROWS = 4096                 # BGNN_QUANTILE_WG_ROWS (bgnn_quantile.h): the rows of one share of qt_add
MAX_GRID = 2048                # BGNN_QUANTILE_MAX_GRID: the workgroups of a pass
REFINE_CHUNK = 1024            # QT_REFINE_CHUNK (error_quantile.hip): keys per workgroup and trip of a refine pass

N = MAX_GRID * WG_ROWS + 3 * WG_ROWS + 5


@pytest.fixture(scope="module")
def case_a():
    """Aligned planes, a one-in-five mask of arbitrary non-zero bytes, 300 non-finite rows among the masked ones; never modified."""
    rng, c, t = _planes(N, 41)
    mask = (rng.random(N) < 0.2).astype(np.uint8)
    mask[mask != 0] = rng.integers(1, 256, int((mask != 0).sum()))
    hit = rng.choice(np.flatnonzero(mask), 300, replace=False)
    c[hit[:100]], c[hit[100:200]], t[hit[200:]] = np.nan, np.inf, -np.inf
    e, nf = _errors(c, t, mask)
    assert nf == 300 and N // 6 < e.size < N // 4
    return c, t, mask, e, nf


def _busy(device):
    """Work left pending on the stream: what follows is queued behind it."""
    a = torch.ones(2048, 2048, device=device)
    for _ in range(8):
        a = (a @ a) * (1.0 / 2048.0)
    return a


def test_one_add_past_one_grid(case_a, gpu_device):
    """Case A: qt_add<vector loads, target, mask> with a second share in workgroups 0 .. 3; capacity n."""
    c, t, mask, e, nf = case_a
    assert N > MAX_GRID * WG_ROWS
    tr = _tracker(N, gpu_device)
    dc, dt, dm = _dev(c, gpu_device), _dev(t, gpu_device), _dev(mask, gpu_device)
    assert dc.data_ptr() % 16 == 0 and dt.data_ptr() % 16 == 0 and dm.data_ptr() % 4 == 0
    tr.add(dc, dt, dm)
    _check(tr, e, nf)


def test_unaligned_planes_every_row_filed(gpu_device):
    """Case B: planes that start one element into their allocations (the scalar loads), no mask and no target, so the values
    are filed sign and all and the refine passes stride over more than 2048 * 1024 keys."""
    rng, c, _ = _planes(N, 43)
    c[rng.choice(N, 50, replace=False)] = np.nan
    e, nf = _errors(c, None, None)
    assert nf == 50 and e.size > MAX_GRID * REFINE_CHUNK and (e < 0).any()
    tr = _tracker(N, gpu_device)
    dc = _dev(c, gpu_device, 1)
    assert dc.data_ptr() % 16 != 0
    tr.add(dc, None, None)
    _check(tr, e, nf)


def test_one_add_equals_three_uneven_adds(case_a, gpu_device):
    """The first of the three adds is itself past one grid (two shares in workgroups 0 and 1); then one row; then the rest."""
    c, t, mask, e, nf = case_a
    dc, dt, dm = _dev(c, gpu_device), _dev(t, gpu_device), _dev(mask, gpu_device)
    one = _tracker(N, gpu_device)
    one.add(dc, dt, dm)
    parts = _tracker(N, gpu_device)
    cuts = [0, MAX_GRID * WG_ROWS + WG_ROWS + 77, MAX_GRID * WG_ROWS + WG_ROWS + 78, N]
    assert cuts[1] > MAX_GRID * WG_ROWS
    for a, b in zip(cuts[:-1], cuts[1:]):
        parts.add(dc[a:b], dt[a:b], dm[a:b])
    assert np.array_equal(_staged(one, e.size), _staged(parts, e.size))
    assert one.state().tobytes() == parts.state().tobytes()
    assert one.select(PS).tobytes() == parts.select(PS).tobytes()
    assert one.percentiles(PS) == _check(parts, e, nf)


def test_behind_pending_work_and_twice_over(case_a, gpu_device):
    """Two runs into fresh state, each queued behind unfinished work on the stream: equal bits."""
    c, t, mask, e, nf = case_a
    blocks = []
    for _ in range(2):
        dc, dt, dm = _dev(c, gpu_device), _dev(t, gpu_device), _dev(mask, gpu_device)
        tr = _tracker(N, gpu_device)
        busy = _busy(gpu_device)
        tr.add(dc, dt, dm)
        busy = busy + _busy(gpu_device)
        block = tr.select(PS).tobytes()
        assert torch.isfinite(busy).all()
        blocks.append((block, tr.state().tobytes(), _staged(tr, e.size).tobytes()))
    assert blocks[0] == blocks[1]
    assert blocks[0][2] == np.sort(_keys(e)).tobytes()


def test_overflow_past_one_grid(gpu_device):
    """capacity 3 000 000 under 8.4 x 10^6 finite rows: the stage fills, the rest is counted, and nothing passes the stage."""
    from bathymetric_gnn_amd.training import CorrectionErrorTracker
    capacity, guard, front = 3000000, 4096, 32
    rng, c, t = _planes(N, 47)
    c[rng.choice(N, 40, replace=False)] = np.inf
    e, nf = _errors(c, t, None)
    m = e.size
    assert nf == 40 and m == N - 40
    pattern = np.arange(front + capacity + guard, dtype=np.int32) * 7 - 1000003
    buffer = torch.from_numpy(pattern.copy()).to(gpu_device)
    tr = CorrectionErrorTracker(capacity, device=gpu_device, stage=buffer[front:front + capacity])
    tr.reset()
    tr.add(_dev(c, gpu_device), _dev(t, gpu_device), None)
    got = tr.percentiles([95.0])
    assert got == {"count": capacity, "nonfinite": nf, "dropped": m - capacity, "values": [None]}
    st = tr.state()
    assert (int(st["rows"]), int(st["filed"]), int(st["nonfinite"]), int(st["dropped"]), int(st["cursor"])) == (N, capacity, nf, m - capacity, m)
    after = buffer.cpu().numpy()
    assert np.array_equal(after[:front], pattern[:front])
    assert np.array_equal(after[front + capacity:], pattern[front + capacity:])          # the guard region
    staged = after[front:front + capacity].view(np.uint32)
    assert np.array_equal(np.bincount(staged >> 21, minlength=2048), st["hist"])
    # a sub-multiset of the keys: no key more often than the input has it
    have, have_n = np.unique(_keys(e), return_counts=True)
    took, took_n = np.unique(staged, return_counts=True)
    at = np.minimum(np.searchsorted(have, took), have.size - 1)
    assert np.array_equal(have[at], took) and (took_n <= have_n[at]).all()
