"""The tail of the cloud pass (csrc/sounding_pass.h): what the lanes past ``n`` do is decided in one loop for six of the seven
passes -- ``sounding_pass`` under UniformAddress with FileSink, StageSink and FlagSink (``SoundingGridder.add``,
``RobustSoundingGridder.add`` and ``.flag``), under VRAddress with FileSink and FlagSink (``VRSoundingGridder.add``,
``RobustVRSoundingGridder.flag``) and under VRBaseAddress with DensitySink (``VRLayoutPlanner.add``) -- and in ``vr_stage``
(csrc/sounding_vr.hip, ``RobustVRSoundingGridder.add``), which the sizes and checks below cover alike.  FileSink and DensitySink shuffle across the wave, so the lanes
past ``n`` must reach them and must not be counted; StageSink and FlagSink store per sounding and must store nothing past ``n``.
(For FileSink the first half is a convention that no test can hold: a ``continue`` past ``n`` leaves its results as they are on this
chip, where a shuffle from a disabled lane reads as zero; DensitySink, which counts the lanes to the end of the wave, shows it.)

Every ``n`` is one lane, the wave edge (64), the workgroup edge (256) or the tile edge (1024) from either side, or four tiles and a
ragged 37.  The cloud is in swath order, three consecutive soundings per cell (or record), so a run straddles every one of those
edges and the last run ends in the final lane that is in range.  Everything is compared for equal bits with the restatements of
_soundings_cpu.py, _robust_cpu.py and _vr_soundings_cpu.py; the counters add up to ``n``; each flag output is a view of a larger
tensor with 64 bytes of a known pattern behind it, which must come back untouched."""
import contextlib

import numpy as np
import pytest
import torch

import _robust_cpu as rc
import _soundings_cpu as sc
import _vr_soundings_cpu as vc

pytestmark = pytest.mark.gpu

SIZES = (1, 63, 64, 65, 255, 257, 1023, 1024, 1025, 4133)
RUN = 3                                            # consecutive soundings per cell
SHAPE, ORIGIN, RES = (6, 5), (500000.0, 4000000.0), 0.5
BASE, BASE_ORIGIN, B, DIM = (2, 2), (5.0e5 + 0.3, 4.1e6), 3.0, 3
GUARD, PATTERN = 64, 0xA5
PLAIN = ("count", "mean", "std", "min", "max", "valid")


def _depths(n):
    """Depths of ``n`` soundings and, from 63 on, one of every kind that is not accepted, none of them in the last run."""
    rng = np.random.default_rng(n)
    z = (-30.0 + 2.0 * rng.standard_normal(n)).astype(np.float32)
    off = np.zeros(n, bool)                        # soundings to be moved off the grid
    if n >= 63:
        z[7], z[13], off[10] = np.nan, 40000.0, True
    return z, off, rng


def _uniform_cloud(n):
    z, off, rng = _depths(n)
    cell = np.arange(n) // RUN % (SHAPE[0] * SHAPE[1])
    x = ORIGIN[0] + (cell % SHAPE[1] + rng.uniform(0.05, 0.95, n)) * RES
    y = ORIGIN[1] - (cell // SHAPE[1] + rng.uniform(0.05, 0.95, n)) * RES
    x[off] = ORIGIN[0] - 1.0
    return x, y, z


def _vr_cloud(n):
    z, off, rng = _depths(n)
    record = np.arange(n) // RUN % (BASE[0] * BASE[1] * DIM * DIM)
    b, s = record // (DIM * DIM), record % (DIM * DIM)
    x = BASE_ORIGIN[0] + ((b % BASE[1]) * DIM + s % DIM + rng.uniform(0.05, 0.95, n)) * (B / DIM)
    y = BASE_ORIGIN[1] + ((b // BASE[1]) * DIM + s // DIM + rng.uniform(0.05, 0.95, n)) * (B / DIM)
    x[off] = BASE_ORIGIN[0] - 1.0
    return x, y, z


def _dev(device, *arrays):
    return [torch.from_numpy(a).to(device) for a in arrays]


def _same_bits(got, want, what):
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, what
    assert got.view(np.uint8).tobytes() == want.view(np.uint8).tobytes(), what


def _check_plain(grid, want, shape, what):
    for k in PLAIN:
        _same_bits(getattr(grid, k).cpu().numpy(), want[k].reshape(shape), (what, k))


def _check_robust(grid, want, shape, what):
    for k in rc.PLANES:
        _same_bits(getattr(grid, k).cpu().numpy(), want[k].reshape(shape), (what, k))
    start = grid.start.cpu().numpy().view(np.uint32)
    _same_bits(start, want["start"].astype(np.uint32), (what, "start"))
    _same_bits(grid.sorted_q.cpu().numpy()[:int(start[-1])], want["sorted_q"].astype(np.int32), (what, "sorted_q"))


@contextlib.contextmanager
def _guarded_flags(monkeypatch, n):
    """While it is open, ``torch.empty`` of ``n`` uint8 -- the flags that ``flag`` allocates -- is a view of a tensor of ``n + GUARD``
    bytes of PATTERN.  Yields the list of those tensors."""
    made, real = [], torch.empty

    def empty(*size, **kw):
        if size == (n,) and kw.get("dtype") is torch.uint8:
            made.append(torch.full((n + GUARD,), PATTERN, dtype=torch.uint8, device=kw["device"]))
            return made[-1][:n]
        return real(*size, **kw)

    with monkeypatch.context() as m:
        m.setattr(torch, "empty", empty)
        yield made


def _flags(monkeypatch, gridder, cloud, grid, want, what):
    n = int(cloud[0].shape[0])
    with _guarded_flags(monkeypatch, n) as made:
        flags = gridder.flag(*cloud, grid)
    assert len(made) == 1 and flags.data_ptr() == made[0].data_ptr() and tuple(flags.shape) == (n,), what
    whole = made[0].cpu().numpy()
    _same_bits(whole[:n], want, (what, "flags"))                                 # (0, 1 or 2: every flag was written)
    assert np.all(whole[n:] == PATTERN), (what, "guard", whole[n:])


@pytest.mark.parametrize("n", SIZES)
def test_uniform_passes(n, gpu_device, monkeypatch):
    """UniformAddress with FileSink, StageSink and FlagSink on a 6 x 5 grid."""
    from bathymetric_gnn_amd.data import RobustSoundingGridder, SoundingGridder
    x, y, z = _uniform_cloud(n)
    cloud = _dev(gpu_device, x, y, z)
    want = sc.grid(x, y, z, SHAPE, ORIGIN, RES)
    kinds = want["counters"]
    assert sum(kinds.values()) == n and (n < 63 or min(kinds.values()) >= 1)
    g = SoundingGridder(SHAPE, ORIGIN, RES, device=gpu_device)
    g.add(*cloud)
    assert g.counters() == kinds and g.offered == n
    _check_plain(g.finalize(), want, SHAPE, "SoundingGridder")
    want_r = rc.grid(x, y, z, SHAPE, ORIGIN, RES)
    r = RobustSoundingGridder(SHAPE, ORIGIN, RES, n, device=gpu_device)
    r.add(*cloud)
    assert r.counters() == kinds == want_r["counters"] and r.offered == n
    cell, q, _ = rc.stage(x, y, z, SHAPE, ORIGIN, RES)
    slots = r._stage[4:4 + n].cpu().numpy().view(np.int32).reshape(-1, 2)        # sounding by sounding, and nothing beyond
    assert np.array_equal(slots[:, 0], cell) and np.array_equal(slots[:, 1], q)
    grid = r.finalize()
    _check_robust(grid, want_r, SHAPE, "RobustSoundingGridder")
    _flags(monkeypatch, r, cloud, grid, want_r["flags"], "RobustSoundingGridder")


@pytest.mark.parametrize("n", SIZES)
def test_vr_passes(n, gpu_device, monkeypatch):
    """VRBaseAddress with DensitySink, VRAddress with FileSink and FlagSink, and vr_stage, on a 2 x 2 base grid, 3 x 3 in every cell."""
    from bathymetric_gnn_amd.data import RobustVRSoundingGridder, VRLayout, VRLayoutPlanner, VRSoundingGridder
    x, y, z = _vr_cloud(n)
    cloud = _dev(gpu_device, x, y, z)
    lay = vc.make_layout(BASE, BASE_ORIGIN, B, np.full(BASE, DIM), np.full(BASE, DIM))
    total = lay["total"]
    assert total == 36
    planner = VRLayoutPlanner(BASE, BASE_ORIGIN, B, device=gpu_device)
    planner.add(*cloud)
    counts = planner.counts().cpu().numpy()
    want = vc.grid(x, y, z, lay)
    kinds = want["counters"]
    assert sum(kinds.values()) == n and kinds["unrefined"] == 0 and (n < 63 or min(kinds[k] for k in sc.COUNTERS) >= 1)
    assert np.array_equal(counts, vc.density(x, y, z, BASE_ORIGIN, B, BASE)) and int(counts.sum()) == kinds["accepted"]
    assert planner.offered == n
    layout = VRLayout(BASE, BASE_ORIGIN, B, lay["index"], lay["dx"], lay["dy"], total, device=gpu_device)
    g = VRSoundingGridder(layout)
    g.add(*cloud)
    assert g.counters() == kinds and g.offered == n
    _check_plain(g.finalize(), want, (total,), "VRSoundingGridder")
    want_r = vc.robust_grid(x, y, z, lay)
    r = RobustVRSoundingGridder(layout, n)
    r.add(*cloud)
    assert r.counters() == kinds == want_r["counters"] and r.offered == n
    _, record = vc.classify(x, y, z, lay)
    q = np.where(record >= 0, np.rint(z.astype(np.float64) * sc.SCALE), 0.0).astype(np.int64)      # (an accepted z is finite)
    slots = r._stage[4:4 + n].cpu().numpy().view(np.int32).reshape(-1, 2)        # sounding by sounding, and nothing beyond
    assert np.array_equal(slots[:, 0], record) and np.array_equal(slots[:, 1], q)
    grid = r.finalize()
    _check_robust(grid, want_r, (total,), "RobustVRSoundingGridder")
    _flags(monkeypatch, r, cloud, grid, want_r["flags"], "RobustVRSoundingGridder")
