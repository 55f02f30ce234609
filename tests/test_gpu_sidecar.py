"""VR BAG sidecar raster on the device (include/bgnn_sidecar.h, csrc/vr_sidecar.hip) through the C ABI: the kernels on the inputs
of the reference-generated fixture (tests/golden/sidecar/sidecar_reference.npz) for any split into runs, any submission order and
two library contexts at once, and NativeVRProcessor.process_refinements(..., sidecar=builder) against the host builder fed grid by
grid by the reference-shaped loop.  Everything bit for bit: the rasterisation is integer work and copies."""
import ctypes as C

import numpy as np
import pytest
import torch

from test_gpu_vr_bag import _processor
from test_host_sidecar import fixture_case

pytestmark = pytest.mark.gpu

BASE_CELL = 60.0          # metres per base cell of the synthetic BAGs' rasters: grids of up to 50 cells x 4 m overlap their neighbours


@pytest.fixture(scope="module")
def golden():
    import os
    from test_host_sidecar import FIXTURE
    assert os.path.exists(FIXTURE)
    return np.load(FIXTURE)


@pytest.fixture(scope="module")
def processors():
    cache = {}

    def get(in_channels):
        if in_channels not in cache:
            cache[in_channels] = _processor(in_channels)
        return cache[in_channels]
    return get


def _table_of(items):
    col = lambda f, dt: np.array([f(g) for g, *_ in items], dt)
    return {"base_row": col(lambda g: g.base_row, np.int64), "base_col": col(lambda g: g.base_col, np.int64),
            "dims_y": col(lambda g: g.dimensions[0], np.int64), "dims_x": col(lambda g: g.dimensions[1], np.int64),
            "res_x": col(lambda g: g.resolution[0], np.float64), "res_y": col(lambda g: g.resolution[1], np.float64),
            "sw_x": col(lambda g: g.sw_corner[0], np.float64), "sw_y": col(lambda g: g.sw_corner[1], np.float64)}


class _Raster:
    """The device side of one sidecar raster, driven through the C ABI directly."""

    def __init__(self, ctx, sb, items):
        from bathymetric_gnn_amd import runtime as rt
        self.rt, self.ctx, self.items = rt, ctx, items
        self.h, self.w = sb.shape
        self.n = len(items)
        tab = _table_of(items)
        self.hw = np.ascontiguousarray(np.stack([tab["dims_y"], tab["dims_x"]], 1), dtype=np.int32)
        self.place = np.ascontiguousarray(np.stack(sb.placement(tab), 1), dtype=np.int64)
        self.pix_off = np.zeros(self.n + 1, np.int64)
        nbytes = ctx.lib.bgnn_sidecar_table_bytes(self.n)
        self.table = torch.empty(nbytes, dtype=torch.uint8, device=ctx.device)
        torch.cuda.synchronize()
        rt.check(ctx.lib.bgnn_sidecar_table(ctx.handle, self.h, self.w, self.n, self.hw.ctypes.data, self.place.ctypes.data,
                                            rt.ptr(self.table), nbytes, self.pix_off.ctypes.data))
        self.images = torch.zeros((3, self.h, self.w), dtype=torch.int64, device=ctx.device)
        self.planes = torch.empty((4, self.h, self.w), dtype=torch.float32, device=ctx.device)
        self.planes[3].zero_()
        self.cells = np.array([g.depth.size for g, *_ in items], np.int64)
        torch.cuda.synchronize()
        self.live = []

    def add(self, ctx, g0, g1, keep=None):
        """Upload the cells of grids [g0, g1) and paint them on ``ctx``'s stream (asynchronous)."""
        rt = self.rt
        cat = lambda k: torch.from_numpy(np.concatenate([np.asarray(it[k], np.float32).reshape(-1) for it in self.items[g0:g1]])).to(ctx.device)
        cls, conf, corr = cat(1), cat(2), cat(3)
        mask = torch.from_numpy(np.concatenate([g.valid_mask.reshape(-1) for g, *_ in self.items[g0:g1]]).astype(np.uint8)).to(ctx.device)
        keep_t = None if keep is None else torch.from_numpy(np.asarray(keep[g0:g1], np.uint8)).to(ctx.device)
        self.live.append((cls, conf, corr, mask, keep_t))
        torch.cuda.synchronize()                                  # (uploads on torch's stream; the kernels run on the contexts')
        rt.check(ctx.lib.bgnn_sidecar_add(ctx.handle, self.h, self.w, rt.ptr(self.images), rt.ptr(self.planes[3]), self.h * self.w,
                                          rt.ptr(self.table), self.n, g0, g1 - g0, int(self.pix_off[g1] - self.pix_off[g0]),
                                          rt.ptr(cls), rt.ptr(conf), rt.ptr(corr), rt.ptr(mask), int(self.cells[g0:g1].sum()),
                                          rt.ptr(keep_t)))

    def finish(self):
        torch.cuda.synchronize()
        self.rt.check(self.ctx.lib.bgnn_sidecar_finish(self.ctx.handle, self.h, self.w, self.rt.ptr(self.images), self.h * self.w,
                                                       self.rt.ptr(self.planes)))
        torch.cuda.synchronize()
        return self.planes.cpu().numpy()


def _same_bits(a, b):
    return a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32))


@pytest.mark.parametrize("name", ["main", "sr"])
def test_kernels_equal_the_reference_fixture(golden, name, gpu_device):
    """All grids in one add; one add per grid in REVERSED order; a random split into runs issued alternately on two contexts
    without any ordering between them.  Each equals the reference's planes bit for bit."""
    from bathymetric_gnn_amd import runtime as rt
    ctx, ctx2 = rt.get_context(gpu_device), rt.new_context(gpu_device)
    want = golden[f"{name}_planes"]
    sb, items = fixture_case(golden, name)
    n = len(items)
    try:
        r = _Raster(ctx, sb, items)
        assert r.pix_off[-1] > 0 and np.all(np.diff(r.pix_off) >= 0)
        r.add(ctx, 0, n)
        assert _same_bits(r.finish(), want)

        r = _Raster(ctx, sb, items)
        for g in reversed(range(n)):
            r.add(ctx, g, g + 1)
        assert _same_bits(r.finish(), want)

        rng = np.random.default_rng(8)
        for trial in range(3):
            cuts = np.sort(rng.choice(np.arange(1, n), size=min(4, n - 1), replace=False)) if n > 1 else np.array([], np.int64)
            bounds = [0] + cuts.tolist() + [n]
            runs = list(zip(bounds[:-1], bounds[1:]))
            r = _Raster(ctx, sb, items)
            for k, j in enumerate(rng.permutation(len(runs))):
                r.add(ctx if k % 2 == 0 else ctx2, *runs[j])
            assert _same_bits(r.finish(), want), (trial, runs)
    finally:
        torch.cuda.synchronize()
        ctx2.close()


def test_keep_flags_drop_grids(golden, gpu_device):
    """A grid whose keep flag is 0 (iterate_refinements skipped it) is not painted: equal to the host builder without it."""
    from bathymetric_gnn_amd import runtime as rt
    ctx = rt.get_context(gpu_device)
    sb, items = fixture_case(golden, "main")
    keep = np.ones(len(items), np.uint8); keep[[2, 8]] = 0
    for it, k in zip(items, keep):
        if k:
            sb.add_refinement_results(*it)
    fresh, _ = fixture_case(golden, "main")
    r = _Raster(ctx, fresh, items)
    r.add(ctx, 5, len(items), keep)
    r.add(ctx, 0, 5, keep)
    got = r.finish()
    assert _same_bits(got, sb.planes()) and not _same_bits(got, golden["main_planes"])


def _georef(handler, res):
    rows, cols = handler.base_shape
    px = BASE_CELL / res
    assert px == int(px)
    return (int(rows * px), int(cols * px)), (1000.0, res, 0.0, 5000.0, 0.0, -res)


def _non_contiguous(md, ref):
    """The record layout of test_process_refinements_non_contiguous_layout: grids stored in reverse order with gaps."""
    from bathymetric_gnn_amd.data.vr_bag import refinement_table
    t = refinement_table(md)
    md2, gap = md.copy(), 5
    total = int(t["cells"].sum()) + gap * len(t["cells"])
    ref2 = np.zeros((1, total), ref.dtype); ref2["depth"] = 1.0e6
    pos = total
    for r, c, i, n in zip(t["base_row"], t["base_col"], t["index"], t["cells"]):
        pos -= n + gap
        ref2[0, pos:pos + n] = ref[0, i:i + n]
        md2[r, c]["index"] = pos
    return md2, ref2


INT_STATS = ("grids_processed", "grids_skipped", "cells_processed", "cells_classified_noise", "cells_corrected")


@pytest.mark.parametrize("in_channels,ratio,budget,res,layout", [
    (8, 0.0, None, 0.5, "contiguous"),
    (8, 0.05, 1000, 0.75, "contiguous"),
    (7, 0.05, 1200, 2.0, "contiguous"),
    (8, 0.0, 1000, 0.75, "gaps"),
    (7, 0.0, None, 2.0, "gaps"),
])
def test_process_refinements_paints_the_host_builders_raster(processors, in_channels, ratio, budget, res, layout, gpu_device):
    """process_refinements(sidecar=) against a host builder fed by the reference-shaped synchronous loop; records and statistics
    against the same call without a sidecar.  (total_confidence is a float64 sum the apply kernel accumulates with one atomic add
    per workgroup, in arrival order: two runs of the SAME call may differ in its last bits, so it is compared to 1e-12 relative;
    every integer statistic and every record is compared exactly.)"""
    from bathymetric_gnn_amd import synthetic
    from bathymetric_gnn_amd.data import SidecarBuilder, VRBagHandler
    from bathymetric_gnn_amd.scripts.inference_native import run_refinements
    proc = processors(in_channels)
    md, ref = synthetic.synthetic_vr_bag(6, 7, seed=31 + in_channels, lo=3, hi=30, empty_fraction=0.08, sparse_fraction=0.08)
    if layout == "gaps":
        md, ref = _non_contiguous(md, ref)
    h = VRBagHandler.from_arrays(md, ref)
    assert h.refinement_table()["contiguous"] == (layout == "contiguous")
    shape, gt = _georef(h, res)
    if budget is not None:
        assert h.total_refinement_nodes / budget >= 6          # a chunk holds at most `budget` cells: both contexts, slot reuse
    host_sb = SidecarBuilder.from_georef(h, shape, gt)
    w_loop = h.copy_and_open_for_writing()
    proc.BATCH_NODE_BUDGET = 4000
    st_loop = run_refinements(proc, h, w_loop, ratio, pipelined=False, results_sink=host_sb.add_refinement_results)
    assert (st_loop["grids_processed"] < h.num_refinement_cells) == (ratio > 0)

    dev_sb = SidecarBuilder.from_georef(h, shape, gt)
    w_dev, w_plain = h.copy_and_open_for_writing(), h.copy_and_open_for_writing()
    st_dev = proc.process_refinements(h, w_dev, ratio, cell_budget=budget, sidecar=dev_sb)
    st_plain = proc.process_refinements(h, w_plain, ratio, cell_budget=budget)
    assert not dev_sb.fresh
    dev_t = dev_sb.planes_device()
    assert dev_t.is_cuda and tuple(dev_t.shape) == (4,) + shape
    assert _same_bits(dev_t.cpu().numpy(), host_sb.planes())
    assert _same_bits(dev_sb.planes(), host_sb.planes())
    assert _same_bits(dev_sb.classification, host_sb.classification) and _same_bits(dev_sb.valid_mask, host_sb.valid_mask)
    covered = ~np.isnan(host_sb.classification)
    assert covered.any() and not covered.all() and (host_sb.valid_mask[covered] == 0).any()
    # records and statistics: nothing of the run changes with the sidecar
    assert np.array_equal(w_dev.refinements.view(np.uint32), w_plain.refinements.view(np.uint32))
    assert np.array_equal(w_dev.refinements.view(np.uint32), w_loop.refinements.view(np.uint32))
    assert w_dev._corrections_applied == w_plain._corrections_applied
    assert set(st_dev) == set(st_plain)
    for k in INT_STATS:
        assert st_dev[k] == st_plain[k], k
    for k in ("total_confidence", "mean_confidence"):
        assert abs(st_dev[k] - st_plain[k]) <= 1e-12 * abs(st_plain[k]), k
    assert st_dev["cells_corrected"] > 0


def test_later_host_adds_act_as_later_writes(processors, golden, gpu_device):
    from bathymetric_gnn_amd import synthetic
    from bathymetric_gnn_amd.data import SidecarBuilder, VRBagHandler
    proc = processors(8)
    md, ref = synthetic.synthetic_vr_bag(3, 3, seed=5, lo=3, hi=12)
    h = VRBagHandler.from_arrays(md, ref)
    shape, gt = _georef(h, 2.0)
    a, b = SidecarBuilder.from_georef(h, shape, gt), SidecarBuilder.from_georef(h, shape, gt)
    proc.process_refinements(h, None, sidecar=a)
    proc.process_refinements(h, None, results_sink=b.add_refinement_results)
    g = next(h.iterate_refinements())
    extra = tuple(np.full(g.shape, v, np.float32) for v in (7.0, 8.0, 9.0))
    a.add_refinement_results(g, *extra); b.add_refinement_results(g, *extra)
    assert _same_bits(a.planes(), b.planes()) and (a.classification == 7.0).any()
    assert a.planes_device() is None                          # (the device tensor no longer holds the builder's state)


def test_scale_and_determinism(processors, gpu_device):
    """synthetic_vr_bag(64, 64) (~2.8 M cells, > 3 400 grids) on a 2 m raster: two device runs identical bit for bit and equal to
    the host builder fed with the same result planes."""
    from bathymetric_gnn_amd import synthetic
    from bathymetric_gnn_amd.data import SidecarBuilder, VRBagHandler
    proc = processors(8)
    md, ref = synthetic.synthetic_vr_bag(64, 64, seed=4000)
    h = VRBagHandler.from_arrays(md, ref)
    assert h.total_refinement_nodes > 2_000_000
    shape, gt = _georef(h, 2.0)
    runs = []
    for _ in range(2):
        sb = SidecarBuilder.from_georef(h, shape, gt)
        proc.process_refinements(h, None, 0.01, sidecar=sb)
        runs.append(sb.planes_device().cpu().numpy())
    assert _same_bits(runs[0], runs[1])
    host_sb = SidecarBuilder.from_georef(h, shape, gt)
    proc.process_refinements(h, None, 0.01, results_sink=host_sb.add_refinement_results)
    assert _same_bits(runs[0], host_sb.planes())
    assert (~np.isnan(runs[0][0])).mean() > 0.2


def test_refusals(processors, golden, gpu_device):
    from bathymetric_gnn_amd import runtime as rt
    from bathymetric_gnn_amd import synthetic
    from bathymetric_gnn_amd.data import VRBagHandler
    ctx = rt.get_context(gpu_device)
    lib = ctx.lib
    # a used builder
    sb, items = fixture_case(golden, "sr")
    sb.add_refinement_results(*items[0])
    md, ref = synthetic.synthetic_vr_bag(2, 2, seed=1, lo=3, hi=6)
    with pytest.raises(ValueError, match="fresh"):
        processors(8).process_refinements(VRBagHandler.from_arrays(md, ref), None, sidecar=sb)
    # the table
    hw = np.array([[4, 5], [3, 3]], np.int32); place = np.array([[0, 0, 2], [1, 1, 1]], np.int64)
    nbytes = lib.bgnn_sidecar_table_bytes(2)
    table = torch.empty(nbytes, dtype=torch.uint8, device=gpu_device)
    torch.cuda.synchronize()
    mk = lambda h, w, n, hw_, pl, nb: lib.bgnn_sidecar_table(ctx.handle, h, w, n, None if hw_ is None else hw_.ctypes.data,
                                                             None if pl is None else pl.ctypes.data, rt.ptr(table), nb, None)
    rt.check(mk(16, 16, 2, hw, place, nbytes))
    with pytest.raises(ValueError, match="BGNN_SIDECAR_MAX_PIXELS"):        # 20 000 x 20 000 = 4e8 pixels > 2^28
        rt.check(mk(20000, 20000, 2, hw, place, nbytes))
    with pytest.raises(ValueError, match="table_bytes"):
        rt.check(mk(16, 16, 2, hw, place, nbytes - 48))
    with pytest.raises(ValueError, match="NULL"):
        rt.check(mk(16, 16, 2, None, place, nbytes))
    bad = place.copy(); bad[1, 2] = 0
    with pytest.raises(ValueError, match="scale 0 < 1"):
        rt.check(mk(16, 16, 2, hw, bad, nbytes))
    # images that do not match the raster's shape, runs outside the table
    images = torch.zeros((3, 16, 16), dtype=torch.int64, device=gpu_device)
    planes = torch.zeros((4, 16, 16), dtype=torch.float32, device=gpu_device)
    vals = torch.zeros(29, dtype=torch.float32, device=gpu_device); mask = torch.ones(29, dtype=torch.uint8, device=gpu_device)
    torch.cuda.synchronize()
    add = lambda h, w, npix, tg, g0, ng: lib.bgnn_sidecar_add(ctx.handle, h, w, rt.ptr(images), rt.ptr(planes[3]), npix, rt.ptr(table), tg,
                                                              g0, ng, 49, rt.ptr(vals), rt.ptr(vals), rt.ptr(vals), rt.ptr(mask), 29, None)
    with pytest.raises(ValueError, match="images hold"):
        rt.check(add(16, 32, 256, 2, 0, 2))
    with pytest.raises(ValueError, match="outside the table"):
        rt.check(add(16, 16, 256, 2, 1, 2))
    with pytest.raises(ValueError, match="images hold"):
        rt.check(lib.bgnn_sidecar_finish(ctx.handle, 32, 16, rt.ptr(images), 256, rt.ptr(planes)))
    with pytest.raises(ValueError, match="BGNN_SIDECAR_MAX_PIXELS"):
        rt.check(lib.bgnn_sidecar_finish(ctx.handle, 20000, 20000, rt.ptr(images), 400000000, rt.ptr(planes)))
    torch.cuda.synchronize()
