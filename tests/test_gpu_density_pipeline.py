"""Sounding density from the gridder to the stitched survey: ``TileBatchEngine.infer`` with the plane against graph build +
``predict`` + ``graph_to_grid``; ``process_survey_device`` / ``process_grid`` against the host merge of per-tile results;
``TileStore`` with a density plane (crops, the eight ops, the batch's graph); a two-epoch ``Trainer`` run whose checkpoint states
its planes and loads into the pipeline; and the routes that refuse a model that takes density."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
RES = (0.5, 0.5)
PLANES = ["uncertainty", "sounding_density"]


def _survey(h, w, seed):
    """depth with a nodata corner and scattered holes, uncertainty, a per-cell sounding count (0 exactly on the invalid cells)."""
    rng = np.random.default_rng(seed)
    depth = (-30.0 + rng.standard_normal((h, w)).cumsum(0).cumsum(1) * 0.01).astype(np.float32)
    count = rng.integers(1, 12, (h, w)).astype(np.int32)
    count[rng.random((h, w)) < 0.1] = 0
    count[:40, :50] = 0
    depth[count == 0] = np.float32(1.0e6)
    unc = (0.05 + 0.1 * rng.random((h, w))).astype(np.float32)
    den = np.where(count >= 1, np.float32(1) / np.maximum(count, 1).astype(np.float32), np.float32(0)).astype(np.float32)
    return depth, unc, den, count


def _model(in_channels=9, seed=1234, layers=3):
    from bathymetric_gnn_amd import synthetic
    from bathymetric_gnn_amd.models import BathymetricGNN
    sd = synthetic.synthetic_state_dict(in_channels=in_channels, num_layers=layers, seed=seed)
    m = BathymetricGNN(in_channels=in_channels, num_gnn_layers=layers, edge_dim=3, dropout=0.0)
    m.load_state_dict({k: torch.as_tensor(v) for k, v in sd.items()})
    return m.to(torch.device("cuda:0")).eval()


def _pipe(model, node_planes=None, tile_batch=5):
    from bathymetric_gnn_amd.config import Config
    from bathymetric_gnn_amd.models import BathymetricPipeline
    cfg = Config(); cfg.tile.tile_size, cfg.tile.overlap = 64, 16
    pipe = BathymetricPipeline(cfg, tile_batch=tile_batch)
    pipe.set_model(model, node_planes=node_planes) if node_planes is not None else pipe.set_model(model)
    return pipe


def _same_bits(a, b):
    return np.array_equal(np.isnan(a), np.isnan(b)) and np.array_equal(np.nan_to_num(a).view(np.uint32), np.nan_to_num(b).view(np.uint32))


def test_engine_infer_with_density_is_build_predict_scatter(gpu_device):
    """The relation the engine tests assert at 8 channels: the grids of bgnn_infer_tiles(_aux) are predict on the batch's graph,
    scattered -- classes equal, confidence bit for bit, correction de-normalised with the node's local_std."""
    from bathymetric_gnn_amd.config.constants import CORRECTION_NORM_FLOOR
    from bathymetric_gnn_amd.data import GraphBuilder
    from bathymetric_gnn_amd.models.pipeline import TileBatchEngine
    d, u, a, count = _survey(150, 170, 5)
    boxes = [(0, 0, 64, 64), (40, 90, 104, 154), (86, 106, 150, 170), (10, 20, 43, 37), (100, 3, 105, 10)]     # ragged, one empty-ish
    crop = lambda p: [np.ascontiguousarray(p[r0:r1, c0:c1]) for r0, c0, r1, c1 in boxes]
    ds, us, As = crop(d), crop(u), crop(a)
    ms = [(t != 1.0e6) for t in ds]
    model, gb = _model(), GraphBuilder()
    eng = TileBatchEngine(model, gb, gpu_device, node_planes=PLANES)
    res = eng.infer(ds, ms, us, [RES] * len(ds), As)
    g = gb.build_graphs(ds, ms, us, [RES] * len(ds), densities=As)
    o = model.predict(g)
    ptr = g.ptr.numpy()
    for k, (r, mk) in enumerate(zip(res, ms)):
        n0, n1 = int(ptr[k]), int(ptr[k + 1])
        assert n1 - n0 == int(mk.sum())
        for name in ("classification", "confidence", "correction"):
            assert r[name].shape == mk.shape and not r[name][~mk].any(), name                      # invalid cells: exactly 0
        assert np.array_equal(r["classification"][mk], o["predicted_class"][n0:n1].float().cpu().numpy())
        assert np.array_equal(r["confidence"][mk].view(np.uint32), o["confidence"][n0:n1].cpu().numpy().view(np.uint32))
        scale = torch.clamp(g.local_std[n0:n1], min=CORRECTION_NORM_FLOOR)
        want = (o["correction"][n0:n1] * scale).cpu().numpy()
        assert np.allclose(r["correction"][mk], want, rtol=0, atol=1e-6 * max(1.0, float(np.abs(want).max())))
    # the uniform batch (the fused tail's own walk): three 64 x 64 tiles
    r3 = eng.infer(ds[:3], ms[:3], us[:3], [RES] * 3, As[:3])
    for k in range(3):
        for name in ("classification", "confidence", "correction"):
            assert _same_bits(r3[k][name], res[k][name]), name                                     # a tile's result: its own, in any batch
    # planes not stated: a 9-channel engine takes both when both are given; an 8-channel one keeps to uncertainty and never reads
    # density in its place
    r9 = TileBatchEngine(model, gb, gpu_device).infer(ds, ms, us, [RES] * len(ds), As)
    assert all(_same_bits(r9[k][n], res[k][n]) for k in range(len(ds)) for n in ("classification", "confidence", "correction"))
    e8 = TileBatchEngine(_model(in_channels=8), gb, gpu_device)
    both, only = e8.infer(ds, ms, us, [RES] * len(ds), As), e8.infer(ds, ms, us, [RES] * len(ds))
    assert all(_same_bits(both[k][n], only[k][n]) for k in range(len(ds)) for n in ("classification", "confidence", "correction"))
    with pytest.raises(ValueError, match="'sounding_density' and the tiles carry none"):
        eng.infer(ds, ms, us, [RES] * len(ds))
    with pytest.raises(ValueError, match="sounding density layer or none"):
        eng.infer(ds, ms, us, [RES] * len(ds), As[:-1] + [None])


def test_survey_with_density_equals_the_host_merge(gpu_device):
    """150 x 170 at tile 64 / overlap 16 (ragged footprint, nodata corner): the device route (cut, classify, stitch in HBM) against
    the host merge of per-tile results (``host_stitch``), bit for bit; the density plane moves the result."""
    from bathymetric_gnn_amd.data import BathymetricGrid
    d, u, a, _ = _survey(150, 170, 6)
    pipe = _pipe(_model(), PLANES)
    grid = BathymetricGrid(depth=d, uncertainty=u, nodata_value=1.0e6, resolution=RES, density=a)
    res = pipe.process_grid(grid)
    assert pipe.last_tile_counts[0] >= 9
    pipe.host_stitch = True
    host = pipe.process_grid(grid)
    pipe.host_stitch = False
    for k in host:
        assert _same_bits(res[k], host[k]), k
    t = lambda p: torch.from_numpy(p).to(gpu_device)
    valid = t(grid.valid_mask)
    dev = pipe.process_survey_device(t(d), valid, t(u), RES, density_t=t(a)).cpu().numpy()
    for i, k in enumerate(("classification", "confidence", "correction", "cleaned_depth")):
        assert _same_bits(dev[i], res[k]), k
    other = pipe.process_survey_device(t(d), valid, t(u), RES, density_t=t(np.ascontiguousarray(a[::-1, ::-1]))).cpu().numpy()
    assert not _same_bits(other[1], dev[1])
    with pytest.raises(ValueError, match="density_t is None"):
        pipe.process_survey_device(t(d), valid, t(u), RES)
    with pytest.raises(ValueError, match="'sounding_density' and the grid has none"):
        pipe.process_grid(BathymetricGrid(depth=d, uncertainty=u, nodata_value=1.0e6, resolution=RES))
    with pytest.raises(ValueError, match="density_t: a contiguous float32 plane"):
        pipe.process_survey_device(t(d), valid, t(u), RES, density_t=t(a)[:, :-1])


def test_an_8_channel_model_without_the_plane_runs_as_before(gpu_device):
    """density_t=None, no node_planes: the call with the new keyword equals the call without it, bit for bit; a grid that carries a
    density is processed without it."""
    from bathymetric_gnn_amd.data import BathymetricGrid
    d, u, a, _ = _survey(150, 170, 7)
    pipe = _pipe(_model(in_channels=8))
    t = lambda p: torch.from_numpy(p).to(gpu_device)
    valid = (t(d) != 1.0e6)
    base = pipe.process_survey_device(t(d), valid, t(u), RES)
    again = pipe.process_survey_device(t(d), valid, t(u), RES, density_t=None)
    assert torch.equal(base.view(torch.int32), again.view(torch.int32))
    with_den = pipe.process_grid(BathymetricGrid(depth=d, uncertainty=u, nodata_value=1.0e6, resolution=RES, density=a))
    for i, k in enumerate(("classification", "confidence", "correction", "cleaned_depth")):
        assert _same_bits(with_den[k], base[i].cpu().numpy()), k


def _rot(tile, op):
    return np.rot90(np.fliplr(tile) if op >= 4 else tile, op % 4)


def test_tile_store_carries_the_density_plane(gpu_device):
    from bathymetric_gnn_amd.data import TileManager
    from bathymetric_gnn_amd.training import TileStore
    d, u, a, _ = _survey(150, 170, 8)
    tm = TileManager(tile_size=64, overlap=16, min_valid_ratio=0.3)
    t = lambda p: torch.from_numpy(p).to(gpu_device)
    store = TileStore.from_survey(t(d), tm, uncertainty=t(u), nodata_value=1.0e6, resolution=RES, density=t(a), augment=False, seed=3)
    assert store.in_channels == 9 and store.node_planes == PLANES and len(store) >= 6
    plain = TileStore.from_survey(t(d), tm, uncertainty=t(u), nodata_value=1.0e6, resolution=RES, augment=False, seed=3)
    assert plain.in_channels == 8 and plain.density is None and plain.node_planes == ["uncertainty"]
    assert torch.equal(plain.depth.view(torch.int32), store.depth.view(torch.int32)) and torch.equal(plain.mask, store.mask)
    crops = [a[r0:r1, c0:c1] for r0, c0, r1, c1 in store.boxes]
    assert np.array_equal(store.density.cpu().numpy().view(np.uint32), np.concatenate([c.ravel() for c in crops]).view(np.uint32))
    idx = [2, 0, 5, 2, 1, 3, 4, 0]
    ops = np.arange(8)
    hw, res, p = store.gather(idx, ops)
    off = 0
    for k, (i, op) in enumerate(zip(idx, ops)):
        want = _rot(crops[i], int(op))
        assert tuple(hw[k]) == want.shape
        n = want.size
        got = p["density"][off:off + n].cpu().numpy().reshape(want.shape)
        assert np.array_equal(got.view(np.uint32), np.ascontiguousarray(want).view(np.uint32)), (i, op)
        off += n
    assert off == p["density"].numel() == p["depth"].numel()
    graph, targets = store.batch(idx, epoch=1, ops=ops)
    assert graph.num_features == 9 and targets["class_labels"].shape[0] == graph.num_nodes
    # (the synthetic noise moves the depth and leaves the plane: column 8 is the gathered density at the valid cells)
    assert torch.equal(graph.x[:, 8].view(torch.int32), p["density"][p["mask"].bool()].view(torch.int32))
    assert torch.equal(graph.x[:, 7].view(torch.int32), p["unc"][p["mask"].bool()].view(torch.int32))
    # ground-truth stores: the device constructor against the host one, with the plane as a sixth input
    rng = np.random.default_rng(4)
    lab = rng.integers(-1, 3, d.shape).astype(np.int32); lab[d == 1.0e6] = -1
    diff = rng.standard_normal(d.shape).astype(np.float32)
    kw = dict(tile_size=64, overlap=16, min_valid_ratio=0.1)
    host = TileStore.from_ground_truth(lab, diff, d, u, resolution=RES, density=a, device=gpu_device, **kw)
    dev = TileStore.from_ground_truths([(t(lab), t(diff), t(d), t(u), RES)], densities=[t(a)], device=gpu_device, **kw)
    assert host.in_channels == dev.in_channels == 9 and len(host) == len(dev) >= 4
    for name in ("depth", "unc", "labels", "difference", "density"):
        x, y = getattr(host, name), getattr(dev, name)
        assert torch.equal(x.view(torch.int32) if x.dtype == torch.float32 else x, y.view(torch.int32) if y.dtype == torch.float32 else y), name
    want = np.concatenate([a[r0:r1, c0:c1].ravel() for r0, c0, r1, c1 in dev.boxes])
    assert np.array_equal(dev.density.cpu().numpy().view(np.uint32), want.view(np.uint32))
    g2, _ = dev.batch([1, 0])
    _, _, p2 = dev.gather([1, 0])
    assert g2.num_features == 9 and torch.equal(g2.x[:, 8].view(torch.int32), p2["density"][p2["mask"].bool()].view(torch.int32))
    with pytest.raises(ValueError, match="for every raster or for none"):
        TileStore.from_ground_truths([(t(lab), t(diff), t(d), t(u), RES)] * 2, densities=[t(a), None], device=gpu_device, **kw)


def _gridded(gpu_device, seed=9, shape=(96, 112)):
    """A point cloud gridded on the device: the SoundingGrid and its host BathymetricGrid (density set by to_grid)."""
    from bathymetric_gnn_amd.data.sounding_grid import SoundingGridder
    rng = np.random.default_rng(seed)
    n = 60000
    x = rng.uniform(0.0, shape[1] * 0.5, n); y = rng.uniform(0.0, shape[0] * 0.5, n)
    z = (-20.0 + 0.02 * x + 0.03 * y + 0.05 * rng.standard_normal(n)).astype(np.float32)
    gr = SoundingGridder(shape, (0.0, shape[0] * 0.5), 0.5, device=gpu_device)
    gr.add(x, y, z)
    return gr.finalize()


def test_trainer_states_its_planes_and_the_pipeline_passes_them(tmp_path, gpu_device):
    from bathymetric_gnn_amd.config import Config
    from bathymetric_gnn_amd.models import BathymetricGNN, BathymetricPipeline
    from bathymetric_gnn_amd.training import TileStore, Trainer
    sg = _gridded(gpu_device)
    grid = sg.to_grid()
    assert grid.density is not None and grid.density.max() <= 1.0 and (grid.density[sg.count.cpu().numpy() == 1] == 1.0).all()
    rng = np.random.default_rng(2)

    def stores(seed):
        tiles = []
        for i in range(8):
            r0, c0 = int(rng.integers(0, 96 - 32)), int(rng.integers(0, 112 - 40))
            sl = (slice(r0, r0 + 32), slice(c0, c0 + 40))
            tiles.append((grid.depth[sl], grid.valid_mask[sl], grid.uncertainty[sl], grid.density[sl]))
        mk = lambda ts, s: TileStore.from_tiles([t[0] for t in ts], [t[1] for t in ts], [t[2] for t in ts], [RES] * len(ts),
                                                densities=[t[3] for t in ts], seed=s)
        return mk(tiles[:6], seed), mk(tiles[6:], seed + 1)
    state = rng.bit_generator.state
    runs = []
    for k in range(2):
        rng.bit_generator.state = state
        train, val = stores(0)
        assert len(train) == 6 and train.in_channels == 9 and train.node_planes == PLANES
        cfg = Config(); cfg.training = {"batch_size": 2, "epochs": 2, "scheduler": "cosine"}
        torch.manual_seed(11)
        model = BathymetricGNN(in_channels=9, num_gnn_layers=2, edge_dim=3)
        tr = Trainer(cfg, model, train, val, output_dir=tmp_path / f"run{k}", seed=4)
        hist = tr.train()
        assert all(len(v) == 2 and all(np.isfinite(v)) for v in hist.values())
        runs.append((hist, {n: v.detach().clone() for n, v in tr.model.state_dict().items()}))
    assert runs[0][0] == runs[1][0]
    for n in runs[0][1]:
        assert torch.equal(runs[0][1][n], runs[1][1][n]), n
    ck = torch.load(tmp_path / "run0" / "final_model.pt", map_location="cpu", weights_only=True)
    assert ck["in_channels"] == 9 and ck["node_planes"] == PLANES
    cfg = Config(); cfg.tile.tile_size, cfg.tile.overlap = 64, 16
    pipe = BathymetricPipeline(cfg, tile_batch=3)
    pipe.load_model(tmp_path / "run0" / "final_model.pt")
    assert pipe.node_planes == tuple(PLANES) and pipe.model.in_channels == 9
    res = pipe.process_grid(grid)
    vm = grid.valid_mask
    assert res["confidence"].shape == grid.shape and np.isfinite(res["confidence"][vm]).all() and set(np.unique(res["classification"][vm])) <= {0.0, 1.0, 2.0}
    depth_t, valid_t, unc_t, den_t = sg.survey_tensors(density=True)
    dev = pipe.process_survey_device(depth_t, valid_t, unc_t, RES, density_t=den_t).cpu().numpy()
    assert _same_bits(dev[1], res["confidence"])
    grid.density = None
    with pytest.raises(ValueError, match="'sounding_density' and the grid has none"):
        pipe.process_grid(grid)


def test_routes_that_refuse_a_model_with_density(gpu_device):
    from bathymetric_gnn_amd.data import BathymetricGrid, GraphBuilder
    from bathymetric_gnn_amd.scripts.inference_native import NativeVRProcessor, run_refinements
    from bathymetric_gnn_amd.training import TileStore
    d, u, a, _ = _survey(150, 170, 10)
    model = _model()
    pipe = _pipe(model, PLANES)
    grid = BathymetricGrid(depth=d, uncertainty=u, nodata_value=1.0e6, resolution=RES, density=a)
    with pytest.raises(NotImplementedError, match="process_grid_streamed does not carry the sounding density"):
        pipe.process_grid_streamed(grid)
    t = lambda p: torch.from_numpy(p).to(gpu_device)
    with pytest.raises(NotImplementedError, match="sharded survey path"):
        pipe.process_survey_device(t(d), t(grid.valid_mask), t(u), RES, shard=(0, 2), density_t=t(a))
    assert model.node_planes == tuple(PLANES)                                  # (set_model leaves the stated planes on the model)
    assert NativeVRProcessor(model, GraphBuilder(), device=gpu_device).node_planes == tuple(PLANES)
    wide = NativeVRProcessor(_model(), GraphBuilder(), device=gpu_device)      # nothing stated: 9 channels are wider than 7 + uncertainty
    with pytest.raises(NotImplementedError, match="process_refinements does not carry"):
        wide.process_refinements(None)
    proc = NativeVRProcessor(model, GraphBuilder(), device=gpu_device, node_planes=PLANES)
    with pytest.raises(NotImplementedError, match="process_refinements does not carry"):
        proc.process_refinements(None)
    with pytest.raises(NotImplementedError, match="run_refinements does not carry"):
        run_refinements(proc, None, None)
    with pytest.raises(NotImplementedError, match="from_refinement_pairs does not carry"):
        TileStore.from_refinement_pairs([], density=t(a))
