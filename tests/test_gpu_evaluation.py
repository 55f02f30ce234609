"""Model evaluation on the device (bgnn_eval_accumulate, training/evaluation.py) against the dictionaries the reference's own
``compute_metrics`` returned (tests/golden/eval, make_golden_eval.py): keys and Python types, every integer and every ratio of
integers exactly, the float sums within the float64 bound of _eval_checks.py."""
import ctypes as C

import numpy as np
import pytest
import torch

from _eval_checks import EVAL_CASES, check_metrics, load_case, numpy_eval_block

pytestmark = pytest.mark.gpu
INT_FIELDS = ("total", "correct", "confusion", "covered", "covered_correct", "conf_cells")


@pytest.mark.parametrize("on_device", [False, True], ids=["host_arrays", "device_tensors"])
@pytest.mark.parametrize("name", EVAL_CASES)
def test_fixture(name, on_device, gpu_device):
    from bathymetric_gnn_amd.training import compute_metrics
    g, want = load_case("eval", name)
    planes = [g["labels"], g["classification"], g.get("confidence")]
    args = [None if p is None else (torch.from_numpy(p.copy()).to(gpu_device) if on_device else p.copy()) for p in planes]
    got = compute_metrics(*args, **({} if on_device else {"device": gpu_device}))
    check_metrics(got, want, *planes)


@pytest.mark.parametrize("name", EVAL_CASES)
def test_block_equals_the_numpy_count(name, gpu_device):
    """Every integer of the device block against the block counted in numpy by the header's definitions (this is also what pins
    the ">= 3" row and column, which the dictionary only shows through its sums)."""
    from bathymetric_gnn_amd.training import Evaluator
    g, _ = load_case("eval", name)
    conf = g.get("confidence")
    ev = Evaluator(gpu_device)
    ev.add(g["labels"].copy(), g["classification"].copy(), None if conf is None else conf.copy())
    got, want = ev.block(), numpy_eval_block(g["labels"], g["classification"], conf)
    for field in INT_FIELDS:
        assert np.array_equal(got[field], want[field]), field


@pytest.mark.parametrize("name,bands", [("threshold_edges", ((0, 3), (3, 4), (4, 16))), ("random", ((0, 5), (5, 31), (31, 48)))])
def test_three_uneven_row_bands_equal_one_call(name, bands, gpu_device):
    """Bands of a 15-column plane start off a 16-byte boundary (rows 3 and 4: byte 180 and 240): the element-wise path."""
    from bathymetric_gnn_amd.training import Evaluator
    g, want = load_case("eval", name)
    lab, pred, conf = (torch.from_numpy(g[k].copy()).to(gpu_device) for k in ("labels", "classification", "confidence"))
    whole = Evaluator(gpu_device)
    whole.add(lab, pred, conf)
    parts = Evaluator(gpu_device)
    for a, b in bands:
        parts.add(lab[a:b], pred[a:b], conf[a:b])
    if name == "threshold_edges":
        assert pred[3:4].data_ptr() % 16 != 0
    bw, bp = whole.block(), parts.block()
    for field in INT_FIELDS:
        assert np.array_equal(bw[field], bp[field]), field
    check_metrics(parts.metrics(), want, g["labels"], g["classification"], g["confidence"])
    parts.reset()
    assert not np.frombuffer(parts.block().tobytes(), np.uint8).any() and parts.metrics()["total_samples"] == 0


def test_more_than_one_workgroup_and_equal_bits(gpu_device):
    """301 x 1003 cells: many workgroups, a ragged tail; against the numpy count, and twice for equal bits."""
    from bathymetric_gnn_amd.training import Evaluator, metrics_from_block
    rng = np.random.default_rng(11)
    shape = (301, 1003)
    labels = rng.choice([-1, 0, 1, 2, 4], shape, p=[.1, .5, .1, .25, .05]).astype(np.int32)
    pred = np.where(rng.random(shape) < 0.85, labels, rng.choice([0, 1, 2, 3], shape)).astype(np.float32)
    pred[rng.random(shape) < 0.03] = np.nan
    conf = rng.random(shape).astype(np.float32)
    blocks = []
    for _ in range(2):
        ev = Evaluator(gpu_device)
        ev.add(labels, pred, conf)
        blocks.append(ev.block())
    assert blocks[0].tobytes() == blocks[1].tobytes()
    want = numpy_eval_block(labels, pred, conf)
    for field in INT_FIELDS:
        assert np.array_equal(blocks[0][field], want[field]), field
    check_metrics(metrics_from_block(blocks[0]), metrics_from_block(want), labels, pred, conf, fixture=False)


def test_evaluator_on_a_classified_survey(gpu_device):
    """Rows 0 / 1 of ``process_survey_device``'s output go in as they stand (NaN where no tile was classified); the result is the
    reference's formula replayed in numpy on the same planes."""
    from bathymetric_gnn_amd import synthetic
    from bathymetric_gnn_amd.config import Config
    from bathymetric_gnn_amd.models import BathymetricGNN, BathymetricPipeline
    from bathymetric_gnn_amd.training import Evaluator, metrics_from_block
    cfg = Config(); cfg.tile.tile_size, cfg.tile.overlap = 64, 16
    pipe = BathymetricPipeline(cfg, tile_batch=7)
    sd = synthetic.synthetic_state_dict(seed=1234)
    m = BathymetricGNN(in_channels=7, edge_dim=3, dropout=0.0); m.load_state_dict({k: torch.as_tensor(v) for k, v in sd.items()})
    pipe.set_model(m.to(gpu_device).eval())
    d, _, _ = synthetic.synthetic_tile(160, 150, 21, "V1")
    d[:70, :70] = 1.0e6
    depth = torch.from_numpy(d).to(gpu_device); valid = (depth != 1.0e6) & torch.isfinite(depth)
    out = pipe.process_survey_device(depth, valid, None, (0.5, 0.5))
    rng = np.random.default_rng(5)
    labels = rng.choice([-1, 0, 1, 2], d.shape, p=[.1, .5, .1, .3]).astype(np.int32)
    ev = Evaluator(gpu_device)
    ev.add(torch.from_numpy(labels).to(gpu_device), out[0], out[1])
    host = out.cpu().numpy()
    assert np.isnan(host[0]).any() and not np.isnan(host[0]).all()
    want_block = numpy_eval_block(labels, host[0], host[1])
    got_block = ev.block()
    assert 0 < int(want_block["total"]) < labels.size
    for field in INT_FIELDS:
        assert np.array_equal(got_block[field], want_block[field]), field
    check_metrics(ev.metrics(), metrics_from_block(want_block), labels, host[0], host[1], fixture=False)


def test_refusals(gpu_device):
    from bathymetric_gnn_amd import runtime as rt
    ctx = rt.get_context(gpu_device)
    lib = ctx.lib
    n = 100
    lab = torch.zeros(n + 4, dtype=torch.int32, device=gpu_device)
    pred = torch.zeros(n + 4, dtype=torch.float32, device=gpu_device)
    need = lib.bgnn_eval_workspace_bytes(n)
    ws = torch.zeros(need // 8 + 2, dtype=torch.int64, device=gpu_device)
    acc = torch.full((rt.EVAL_ACC_BYTES // 8 + 1,), 77, dtype=torch.int64, device=gpu_device)
    p = rt.ptr

    def call(labels=p(lab), pr=p(pred), conf=None, cells=n, ws_p=p(ws), ws_bytes=need, a=p(acc)):
        return lib.bgnn_eval_accumulate(ctx.handle, labels, pr, conf, cells, ws_p, C.c_size_t(ws_bytes), a)

    def refused(word, **kw):
        assert call(**kw) == rt.ERR_INVALID
        assert word in lib.bgnn_last_error().decode(), lib.bgnn_last_error()

    for k in ("labels", "pr", "ws_p", "a"):
        refused("NULL", **{k: None})
    refused("-5 cells", cells=-5)
    refused("workspace of", ws_bytes=need - 8)
    refused("workspace is not 8-byte aligned", ws_p=C.c_void_p(ws.data_ptr() + 4))
    refused("accumulator block is not 8-byte aligned", a=C.c_void_p(acc.data_ptr() + 4))
    assert lib.bgnn_eval_reset(ctx.handle, None) == rt.ERR_INVALID
    assert lib.bgnn_eval_reset(ctx.handle, C.c_void_p(acc.data_ptr() + 4)) == rt.ERR_INVALID
    assert call(cells=0) == 0
    ctx.synchronize()
    assert acc.tolist() == [77] * acc.numel()                 # nothing was launched
    assert lib.bgnn_eval_reset(ctx.handle, p(acc)) == 0 and call() == 0
    ctx.synchronize()
    assert acc[0].item() == n and acc[1].item() == n and acc[-1].item() == 77 and acc[-2].item() == 0      # no confidence: conf_cells stays 0
    with pytest.raises(ValueError):
        from bathymetric_gnn_amd.training import Evaluator
        Evaluator(gpu_device).add(np.zeros((3, 3), np.int32), np.zeros((3, 4), np.float32))
