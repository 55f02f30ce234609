"""Operating curves on the device (bgnn_curve_accumulate, training/operating_curve.py) against the numpy restatement of
_curve_cpu.py: every comparison is exact equality of the int64 block (test_host_curve.py guards the restatement itself).  The planes
carry NaN, +-inf and huge values on purpose: the header promises a defined code and an in-range index for every bit pattern."""
import ctypes as C

import numpy as np
import pytest
import torch

import _curve_cpu as cc
from bathymetric_gnn_amd.training.operating_curve import WG_CELLS as WG      # the cells of one workgroup's share

pytestmark = pytest.mark.gpu

SIZES = [1, 63, 64, 65, 255, 257, WG - 1, WG, WG + 1, 3 * WG + 5, 1048583]
TABLES = [1, 2, 101, 128]


def _dev(planes, device, offset=0):
    """The planes on the device; ``offset`` > 0 puts every plane that many elements past its allocation's 256-byte base."""
    out = []
    for p in planes:
        if p is None:
            out.append(None)
            continue
        src = torch.from_numpy(np.array(p))                    # (a copy: the shared cases are read-only)
        t = torch.empty(p.size + offset, dtype=src.dtype, device=device)
        t[offset:] = src.to(device)
        out.append(t[offset:])
    return out


def _block_of(thr, planes, device, offset=0):
    from bathymetric_gnn_amd.training import OperatingCurve
    oc = OperatingCurve(thr, device)
    oc.add(*_dev(planes, device, offset))
    return oc.block()


def _same(got, want):
    assert got.dtype == want.dtype
    for f in want.dtype.names:
        assert np.array_equal(got[f], want[f]), f
    assert got.tobytes() == want.tobytes()


@pytest.mark.parametrize("n_thresholds", TABLES)
@pytest.mark.parametrize("cells", SIZES)
def test_adversarial_planes_equal_the_numpy_block(cells, n_thresholds, gpu_device):
    """Every size at which the kernel takes another path (a partial wave, a partial 16-byte vector, one workgroup's share +- 1,
    several workgroups, more shares than workgroups) times every table size, on the salted planes."""
    thr, planes, want = cc.adversarial_case(n_thresholds, cells)
    got = _block_of(thr, planes, gpu_device)
    _same(got, want)
    if cells >= WG - 1:                                         # (the salt is there: NaN confidences, skipped and summed residuals)
        assert int(want["counts"][-1].sum()) > 0 and int(want["res_skipped"]) > 0 and int(want["res_cells"].sum()) > 0


@pytest.mark.parametrize("n_thresholds", TABLES)
def test_planes_offset_by_one_element(n_thresholds, gpu_device):
    """Bases 4 bytes past a 16-byte boundary: the element-wise path; the same block as from aligned planes."""
    thr, planes, want = cc.adversarial_case(n_thresholds, 3 * WG + 5)
    dev = _dev(planes, gpu_device, offset=1)
    assert all(t.data_ptr() % 16 == 4 for t in dev)
    _same(_block_of(thr, planes, gpu_device, offset=1), want)
    # only one plane off the boundary is enough to leave the vector path
    from bathymetric_gnn_amd.training import OperatingCurve
    mixed = _dev(planes, gpu_device)
    mixed[3] = dev[3]
    oc = OperatingCurve(thr, gpu_device)
    oc.add(*mixed)
    _same(oc.block(), want)


@pytest.mark.parametrize("n_thresholds", TABLES)
@pytest.mark.parametrize("cells", [64, 3 * WG + 5, 200003])
def test_every_cell_on_one_value(cells, n_thresholds, gpu_device):
    """The worst contention: one confidence (a threshold itself, or its neighbour above), one label, one prediction."""
    thr = cc.thresholds_for(n_thresholds)
    for value in (thr[len(thr) // 2], np.nextafter(thr[-1], np.float32(np.inf))):
        planes = cc.one_value_planes(cells, value)
        want = cc.numpy_block(thr, *planes)
        assert np.count_nonzero(want["counts"]) == 1 and np.count_nonzero(want["res_cells"]) == 1
        _same(_block_of(thr, planes, gpu_device), want)


@pytest.mark.parametrize("n_thresholds", [1, 101])
def test_clustered_confidences(n_thresholds, gpu_device):
    """Nine cells in ten on one value, the rest spread: the peeled groups and the lanes that add for themselves, mixed."""
    thr = cc.thresholds_for(n_thresholds)
    n = 50021
    labels, pred, conf, diff, corr = cc.random_planes(n, 17)
    rng = np.random.default_rng(18)
    conf[rng.random(n) < 0.9] = np.float32(0.99)
    pred[rng.random(n) < 0.5] = 2.0
    planes = (labels, pred, conf, diff, corr)
    _same(_block_of(thr, planes, gpu_device), cc.numpy_block(thr, *planes))


def test_without_residual_planes(gpu_device):
    """difference and correction both absent: the residual entries are left alone (here: as reset left them)."""
    from bathymetric_gnn_amd.training import OperatingCurve, curve_from_block
    thr, planes, _ = cc.adversarial_case(101, 3 * WG + 5)
    want = cc.numpy_block(thr, *planes[:3])
    oc = OperatingCurve(thr, gpu_device)
    oc.add(*_dev(planes[:3], gpu_device))
    _same(oc.block(), want)
    assert "residual" not in oc.curve()
    cc.assert_curves_equal(oc.curve(), curve_from_block(want, thr))
    # a block whose residual entries hold something keeps it through such a call
    oc.reset()
    oc.add(*_dev(planes, gpu_device))
    oc.add(*_dev(planes[:3], gpu_device))
    _same(oc.block(), cc.add_blocks(cc.numpy_block(thr, *planes), want))
    with pytest.raises(ValueError, match="residual planes in every call"):
        curve_from_block(oc.block(), thr, with_residual=True)


@pytest.mark.parametrize("bands", [((0, 3), (3, 4), (4, 16)), ((0, 1), (1, 15), (15, 16))])
def test_three_row_bands_equal_one_call_and_reset_zeroes(bands, gpu_device):
    """Bands of a 16 x 203 plane start off a 16-byte boundary; they accumulate to the whole plane's block, reset zeroes it."""
    from bathymetric_gnn_amd.training import OperatingCurve
    thr = cc.thresholds_for(101)
    shape = (16, 203)
    planes = [p.reshape(shape) for p in cc.adversarial_planes(thr, shape[0] * shape[1], 23)]
    dev = [torch.from_numpy(p).to(gpu_device) for p in planes]
    whole = OperatingCurve(thr, gpu_device)
    whole.add(*dev)
    parts = OperatingCurve(thr, gpu_device)
    for a, b in bands:
        parts.add(*(t[a:b] for t in dev))
    assert any(dev[1][a:b].data_ptr() % 16 != 0 for a, b in bands)
    want = cc.numpy_block(thr, *planes)
    _same(whole.block(), want)
    _same(parts.block(), want)
    cc.assert_curves_equal(parts.curve(), cc.brute_curve(thr, *planes))
    parts.reset()
    assert not np.frombuffer(parts.block().tobytes(), np.uint8).any() and parts.curve()["total"] == 0
    parts.add(*planes)                                          # host arrays, after a reset
    _same(parts.block(), want)


def test_two_runs_give_equal_bits(gpu_device):
    from bathymetric_gnn_amd.training import OperatingCurve
    thr, planes, want = cc.adversarial_case(128, 1048583)
    dev = _dev(planes, gpu_device)
    blocks = []
    for _ in range(2):
        oc = OperatingCurve(thr, gpu_device)
        oc.add(*dev)
        blocks.append(oc._block.clone())
    assert torch.equal(blocks[0], blocks[1])
    assert blocks[0].cpu().numpy().tobytes() == want.tobytes()


def test_label_bands_as_floats_and_masking(gpu_device):
    """A float label band (band 1 of a ground-truth raster: NaN and negative values are no data) is masked as Evaluator masks it."""
    thr, planes, want = cc.adversarial_case(101, 3 * WG + 5)
    labels = planes[0].astype(np.float32)
    labels[planes[0] < 0] = np.where(np.arange((planes[0] < 0).sum()) % 2 == 0, np.nan, -9999.0)
    _same(_block_of(thr, (labels,) + planes[1:], gpu_device), want)


def test_consistent_with_evaluator(gpu_device):
    """With float32(0.5 .. 0.9) in the table, the totals, the confusion matrix, covered and covered_correct are the Evaluator
    block's on the same planes.  (Labels and predictions stay below 4 here: the block files classes above 2 as one, so its diagonal
    is Evaluator's ``correct`` only while that class holds one value.)"""
    from bathymetric_gnn_amd import runtime as rt
    from bathymetric_gnn_amd.training import Evaluator, OperatingCurve, curve_from_block
    rng = np.random.default_rng(31)
    n = 40009
    thr = np.unique(np.concatenate([cc.thresholds_for(101), np.array(rt.EVAL_THRESHOLDS, np.float32)]))
    special = np.concatenate([np.array(rt.EVAL_THRESHOLDS, np.float32), np.array([np.nan, np.inf, -1.0, 2.0], np.float32)])
    labels = rng.choice(np.array([-1, 0, 1, 2, 3], np.int32), n, p=[.1, .4, .1, .3, .1]).astype(np.int32)
    pred = rng.choice(np.array([np.nan, -1, 0.0, 1.0, 2.0, 2.9, 3.0, 3.5], np.float32), n).astype(np.float32)
    conf = rng.random(n).astype(np.float32)
    salt = rng.random(n) < 0.3
    conf[salt] = rng.choice(special, int(salt.sum()))
    dev = _dev((labels, pred, conf), gpu_device)
    ev = Evaluator(gpu_device)
    ev.add(*dev)
    oc = OperatingCurve(thr, gpu_device)
    oc.add(*dev)
    eb, blk = ev.block(), oc.block()
    counts = blk["counts"]
    assert int(counts.sum()) == int(eb["total"]) > 0
    assert np.array_equal(counts.sum(axis=0), eb["confusion"])
    assert int(np.trace(counts.sum(axis=0))) == int(eb["correct"])
    curve = curve_from_block(blk, thr)
    for j, t in enumerate(rt.EVAL_THRESHOLDS):
        k = int(np.flatnonzero(thr == np.float32(t))[0])
        covered = counts[2 * k + 1:2 * len(thr) + 1]
        assert int(covered.sum()) == int(eb["covered"][j]) > 0
        assert int(np.trace(covered.sum(axis=0))) == int(eb["covered_correct"][j])
        assert curve["coverage"]["coverage"][k] == int(eb["covered"][j]) / int(eb["total"])
        assert curve["coverage"]["accuracy"][k] == int(eb["covered_correct"][j]) / int(eb["covered"][j])
    m = ev.metrics()
    assert curve["total"] == m["total_samples"] and [r[:3] for r in curve["confusion_matrix"][:3]] == m["confusion_matrix"]
    assert curve["support"]["noise"] == m["noise"]["support"]


def test_end_to_end_survey_pair(gpu_device):
    """A synthetic survey pair through compute_ground_truth, process_survey_device (synthetic weights) and OperatingCurve with
    the device planes as they stand: equal to the host restatement on the downloaded planes; and at the pipeline's own
    auto_correct_threshold the auto-corrected cells are the cells whose cleaned depth differs from the input depth, plus the
    applied cells the correction leaves unchanged (a correction of exactly 0, or one below half an ulp of the depth)."""
    from bathymetric_gnn_amd import synthetic
    from bathymetric_gnn_amd.config import Config
    from bathymetric_gnn_amd.data import BathymetricGrid, compute_ground_truth
    from bathymetric_gnn_amd.models import BathymetricGNN, BathymetricPipeline
    from bathymetric_gnn_amd.training import OperatingCurve
    auto_thr = 0.541                                            # (the median confidence of this model's predicted noise)
    cfg = Config(); cfg.tile.tile_size, cfg.tile.overlap = 64, 16
    cfg.inference.auto_correct_threshold = auto_thr
    pipe = BathymetricPipeline(cfg, tile_batch=7)
    sd = synthetic.synthetic_state_dict(seed=2)                 # (weights that predict noise on a tenth of the cells)
    m = BathymetricGNN(in_channels=7, edge_dim=3, dropout=0.0); m.load_state_dict({k: torch.as_tensor(v) for k, v in sd.items()})
    pipe.set_model(m.to(gpu_device).eval())
    clean, _, _ = synthetic.synthetic_tile(160, 150, 21, "V1")
    rng = np.random.default_rng(6)
    noisy = clean + (0.02 * rng.standard_normal(clean.shape)).astype(np.float32)
    spikes = rng.random(clean.shape) < 0.05
    noisy[spikes] += rng.choice([-1.5, 1.5], int(spikes.sum())).astype(np.float32)
    for plane in (clean, noisy):                                # the same cells without data in both surveys
        plane[:70, :70] = 1.0e6
        plane[100:104, 20:90] = np.nan
    holes = ~np.isfinite(clean) | (clean == 1.0e6)             # (the synthetic tile's own)
    noisy[holes] = clean[holes]
    h, w = clean.shape
    transform = (400000.0, 0.5, 0.0, 4.2e6, 0.0, -0.5)
    bounds = (400000.0, 4.2e6 - 0.5 * h, 400000.0 + 0.5 * w, 4.2e6)
    grids = [BathymetricGrid(depth=d, uncertainty=None, transform=transform, crs="EPSG:32619", resolution=(0.5, 0.5), bounds=bounds)
             for d in (clean, noisy)]
    gt = compute_ground_truth(*grids, 0.15, device=gpu_device)
    assert tuple(gt.labels.shape) == (h, w)
    depth = gt.noisy_depth
    valid = (depth != 1.0e6) & torch.isfinite(depth)
    out = pipe.process_survey_device(depth, valid, None, (0.5, 0.5))
    thr = np.unique(np.concatenate([cc.thresholds_for(101), np.array([auto_thr], np.float32)]))
    oc = OperatingCurve(thr, gpu_device)
    oc.add(gt.labels, out[0], out[1], gt.difference, out[2])    # the device planes as they stand
    host = out.cpu().numpy()
    labels, difference = gt.labels.cpu().numpy(), gt.difference.cpu().numpy()
    want = cc.numpy_block(thr, labels, host[0], host[1], difference, host[2])
    _same(oc.block(), want)
    curve = oc.curve()
    cc.assert_curves_equal(curve, cc.brute_curve(thr, labels, host[0], host[1], difference, host[2]))
    # the cells the pipeline corrected
    d, ok = depth.cpu().numpy(), valid.cpu().numpy()
    applied = ok & (host[0] == 2.0) & (host[1] > np.float32(auto_thr))
    print("predicted classes on valid cells:", np.bincount(host[0][ok].astype(np.int64), minlength=3).tolist(), "confidence of predicted noise, quantiles 0 / 0.5 / 1:",
          np.quantile(host[1][ok & (host[0] == 2.0)], [0, 0.5, 1]).tolist() if (ok & (host[0] == 2.0)).any() else None, "applied:", int(applied.sum()))
    assert np.array_equal(ok, labels >= 0) and np.array_equal(ok, ~holes)
    changed = ok & (host[3] != d)
    unchanged = applied & (d - host[2] == d)
    assert int((applied & (host[2] == 0)).sum()) <= int(unchanged.sum())
    k = int(np.flatnonzero(thr == np.float32(auto_thr))[0])
    assert curve["auto_correct"]["cells"][k] == int(changed.sum()) + int(unchanged.sum()) > 0
    assert curve["residual"]["corrected_cells"][k] == curve["auto_correct"]["cells"][k]
    assert 0 < curve["auto_correct"]["cells"][k] < curve["total"] == int(ok.sum())


def test_refusals(gpu_device):
    from bathymetric_gnn_amd import runtime as rt
    from bathymetric_gnn_amd.training import OperatingCurve, curve_accumulate
    thr = cc.thresholds_for(2)
    n = 100
    lab = torch.zeros(n, dtype=torch.int32, device=gpu_device)
    f = torch.zeros(n, dtype=torch.float32, device=gpu_device)
    t_dev = torch.from_numpy(thr).to(gpu_device)
    block = torch.full((np.dtype(rt.curve_block_dtype(2)).itemsize // 8,), 77, dtype=torch.int64, device=gpu_device)
    oc = OperatingCurve(thr, gpu_device)
    # mismatched shapes
    with pytest.raises(ValueError, match="one shape"):
        oc.add(np.zeros((3, 3), np.int32), np.zeros((3, 4), np.float32), np.zeros((3, 3), np.float32))
    with pytest.raises(ValueError, match="one shape"):
        oc.add(np.zeros((3, 4), np.int32), np.zeros((3, 4), np.float32), np.zeros((3, 4), np.float32), np.zeros((4, 3), np.float32),
               np.zeros((3, 4), np.float32))
    with pytest.raises(ValueError, match="number of cells"):
        curve_accumulate(t_dev, lab, f[:50], f, None, None, block)
    # one residual plane without the other
    with pytest.raises(ValueError, match="both"):
        oc.add(lab, f, f, difference=f)
    with pytest.raises(ValueError, match="both"):
        oc.add(lab, f, f, correction=f)
    with pytest.raises(ValueError, match="both"):
        curve_accumulate(t_dev, lab, f, f, f, None, block)
    # thresholds on the wrong device or of the wrong dtype
    with pytest.raises(TypeError, match="thresholds"):
        curve_accumulate(torch.from_numpy(thr), lab, f, f, None, None, block)
    with pytest.raises(TypeError, match="thresholds"):
        curve_accumulate(t_dev.double(), lab, f, f, None, None, block)
    with pytest.raises(TypeError, match="labels"):
        curve_accumulate(t_dev, lab.long(), f, f, None, None, block)
    with pytest.raises(ValueError, match="block of"):
        curve_accumulate(t_dev, lab, f, f, None, None, block[:-1])
    assert oc.curve()["total"] == 0
    # the C entry itself, with a live context: refused before any launch, the block untouched
    ctx = rt.get_context(gpu_device)
    lib, p = ctx.lib, rt.ptr
    assert lib.bgnn_curve_accumulate(ctx.handle, p(t_dev), 2, p(lab), p(f), p(f), p(f), None, n, p(block)) == rt.ERR_INVALID
    assert lib.bgnn_curve_accumulate(ctx.handle, p(t_dev), 129, p(lab), p(f), p(f), None, None, n, p(block)) == rt.ERR_INVALID
    assert lib.bgnn_curve_accumulate(ctx.handle, p(t_dev), 2, p(lab), p(f), p(f), None, None, n,
                                     C.c_void_p(block.data_ptr() + 4)) == rt.ERR_INVALID
    assert lib.bgnn_curve_accumulate(ctx.handle, p(t_dev), 2, p(lab), p(f), p(f), None, None, 0, p(block)) == 0
    ctx.synchronize()
    assert block.tolist() == [77] * block.numel()
    assert lib.bgnn_curve_reset(ctx.handle, p(block), 2) == 0
    curve_accumulate(t_dev, lab, f, f, None, None, block)
    ctx.synchronize()
    assert int(block.sum()) == n and int(block[0]) == n        # label 0, prediction 0, confidence 0 below both thresholds: code 0
