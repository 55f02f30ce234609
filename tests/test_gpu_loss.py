"""The fused multi-task training loss on the GPU (include/bgnn_loss.h, bathymetric_gnn_amd.training).

Yardsticks: the reference's float64 run on the fixtures (tests/golden/loss/*.npz), and tests/_loss_cpu.py (pinned against that run
by tests/test_host_loss.py) at the sizes the fixtures do not reach.  Bounds, for every comparison with a float64 value:
  a term        |v - ref| <= 2^-23 |ref|: one float32 ulp, twice the half ulp of the single rounding; the rest covers summation
                order and libm differences in float64, below 1e-10 relative at a million rows
  a gradient    |g - g64| <= 2^-23 |g64| + 2^-40 max|g64| element-wise: the same, and the upstream weight the kernel receives as
                float32 (0.2 is 2^-26 relative from its float32); the floor is for elements that cancel (p - 1 on a saturated row)
NaN must appear exactly where the yardstick has NaN.  Through the model the parameter gradients are held to the rule of
tests/test_gpu_backward_training.py (``_accept``)."""
import glob
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import _loss_cpu as lc
import test_gpu_backward_plain as plain
from test_gpu_backward import _tiles_graph
from test_gpu_backward_training import _accept, _dropout, _oracle_for, _step, _tile
from test_gpu_backward_training import _net as _gat_net, _sd as _gat_sd

from bathymetric_gnn_amd.data import SyntheticNoiseGenerator, training_targets
from bathymetric_gnn_amd.training import BathymetricGNNLoss, compute_class_weights, compute_correction_delta, losses as L

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LOSS_DIR = os.path.join(ROOT, "tests", "golden", "loss")
FIXTURES = sorted(p for p in glob.glob(os.path.join(LOSS_DIR, "*.npz")) if not p.endswith("helpers.npz"))
NAMES = [os.path.basename(p)[:-4] for p in FIXTURES]
GRADS = ("class_logits", "confidence", "correction")
ULP, FLOOR = 2.0 ** -23, 2.0 ** -40
W3 = np.array([0.4, 1.7, 0.9], np.float32)       # class weights are float32 tensors: the yardstick takes the same values, widened
STATS = ("n_masked", "false_positives", "shoal_false_positives", "deep_false_positives", "n_ignored", "n_invalid")


# ---- helpers ------------------------------------------------------------------------------------------------------------------------
def make_inputs(n, c=3, seed=0, mix=(0.7, 0.1, 0.2)):
    """Seeded random inputs of the model's output shape: logits that agree with the label on most rows, predicted = argmax,
    confidence in (0, 1), corrections and targets of a few units, mask = (label 2)."""
    rng = np.random.default_rng(seed)
    labels = rng.choice(len(mix), size=n, p=np.asarray(mix, np.float64) / np.sum(mix)).astype(np.int64)
    logits = (2.0 * rng.standard_normal((n, c))).astype(np.float32)
    agree = rng.random(n) < 0.6
    logits[np.arange(n)[agree], labels[agree]] += np.float32(3.0)
    conf = (1.0 / (1.0 + np.exp(-2.0 * rng.standard_normal(n)))).astype(np.float32)
    return dict(class_logits=logits, confidence=conf, correction=(1.5 * rng.standard_normal(n)).astype(np.float32),
                predicted_class=logits.argmax(axis=1).astype(np.int64), class_labels=labels,
                correction_targets=(1.5 * rng.standard_normal(n)).astype(np.float32), noise_mask=labels == 2)


def criterion(cfg, dev):
    w = None if cfg["class_weights"] is None else torch.as_tensor(np.asarray(cfg["class_weights"], np.float32)).to(dev)
    return BathymetricGNNLoss(class_weights=w, label_smoothing=cfg["label_smoothing"], correction_delta=cfg["delta"])


def to_device(inp, dev, grad=True):
    outputs = {"predicted_class": torch.as_tensor(inp["predicted_class"]).to(dev)}
    for k in GRADS:
        if inp.get(k) is not None:
            outputs[k] = torch.as_tensor(inp[k]).to(dev).requires_grad_(grad)
    targets = {"class_labels": torch.as_tensor(inp["class_labels"]).to(dev)}
    for k in ("correction_targets", "noise_mask"):
        if inp.get(k) is not None:
            targets[k] = torch.as_tensor(inp[k]).to(dev)
    return outputs, targets


def run_gpu(inp, cfg, dev, combine=None):
    """(criterion, values, gradients) of one forward + backward on the device; ``combine(losses)`` is the scalar that is
    differentiated (default: total)."""
    crit = criterion(cfg, dev)
    outputs, targets = to_device(inp, dev)
    losses = crit(outputs, targets)
    assert tuple(losses) == lc.TERMS
    for k, v in losses.items():
        assert v.dtype == torch.float32 and v.dim() == 0 and v.device == dev, k
    (losses["total"] if combine is None else combine(losses)).backward()
    grads = {k: (None if outputs[k].grad is None else outputs[k].grad.detach().cpu().numpy()) for k in GRADS if k in outputs}
    return crit, {k: float(v.detach()) for k, v in losses.items()}, grads


def check_values(name, got, want):
    for k in lc.TERMS:
        v, r = float(got[k]), float(want[k])
        print(f"{name} {k}: gpu {v!r} ref {r!r}" + ("" if np.isnan(r) or r == 0 else f" ({abs(v - r) / abs(r) / ULP:.3f} ulp)"))
    for k in lc.TERMS:
        v, r = float(got[k]), float(want[k])
        if np.isnan(r):
            assert np.isnan(v), (name, k, v)
        else:
            assert abs(v - r) <= ULP * abs(r), (name, k, v, r)


def check_grads(name, got, want, ulps=1.0):
    """``want``: {input: float64 array, or None / absent when nothing flows}."""
    for k in GRADS:
        w = want.get(k)
        g = got.get(k)
        if w is None:
            assert g is None or not np.any(g), (name, k)
            continue
        assert g is not None and g.shape == w.shape and g.dtype == np.float32, (name, k)
        if not w.size:
            continue
        assert np.array_equal(np.isnan(g), np.isnan(w)), (name, k)
        ok = ~np.isnan(w)
        err = np.abs(g.astype(np.float64) - w)[ok]
        bound = (ulps * ULP * np.abs(w) + FLOOR * np.nanmax(np.abs(w)))[ok]
        worst = float((err[bound > 0] / bound[bound > 0]).max()) if (bound > 0).any() else 0.0      # (an all-zero gradient: bound 0)
        print(f"{name} d/d{k}: max|g64| {np.nanmax(np.abs(w)):.3e}, worst error / bound {worst:.3f}")
        assert (err <= bound).all(), (name, k, worst)


def check_stats(crit, inp, cfg):
    want = lc.counts(inp, cfg)
    st = crit.last_stats
    assert st["confusion"].dtype == torch.int64 and st["confusion"].is_cuda
    assert np.array_equal(st["confusion"].cpu().numpy(), want["confusion"])
    for k in STATS:
        assert int(st[k]) == want[k], (k, int(st[k]), want[k])
    assert int(st["confusion"].sum()) + want["n_ignored"] + want["n_invalid"] == len(inp["class_labels"])


def against_restatement(name, inp, cfg, dev):
    crit, vals, grads = run_gpu(inp, cfg, dev)
    check_values(name, vals, lc.loss(inp, cfg))
    check_grads(name, grads, lc.grads(inp, cfg))
    check_stats(crit, inp, cfg)
    return crit, vals, grads


# ---- parity with the reference on every fixture -------------------------------------------------------------------------------------
@pytest.mark.parametrize("path", FIXTURES, ids=NAMES)
def test_parity_with_the_reference(path, gpu_device):
    inp, cfg, z = lc.load_fixture(path)
    crit, vals, grads = run_gpu(inp, cfg, gpu_device)
    check_values(os.path.basename(path), vals, {k: z["ref64_" + k] for k in lc.TERMS})
    check_grads(os.path.basename(path), grads, {k: z["g64_" + k] for k in GRADS if "g64_" + k in z.files})
    if len(inp["class_labels"]):
        check_stats(crit, inp, cfg)
    else:
        assert crit.last_stats is None              # an empty batch launches nothing of the library


# ---- sizes around the launch geometry -----------------------------------------------------------------------------------------------
R, FW = L.ROWS_PER_WORKGROUP, L.FINISH_WIDTH
GEOMETRY = [R - 1, R, R + 1, 2 * R + 1, R * FW + 1]        # ..., three partials, one partial more than a finish pass reads


@pytest.mark.parametrize("n", GEOMETRY)
def test_sizes_around_the_launch_geometry(n, gpu_device):
    assert R > 1 and FW > 1
    inp = make_inputs(n, seed=300 + n % 97)
    against_restatement(f"n={n}", inp, lc.config(class_weights=W3, label_smoothing=0.1, delta=1.25), gpu_device)


def test_sixteen_classes_and_two(gpu_device):
    against_restatement("C=16", make_inputs(R + 3, c=16, seed=5, mix=(0.5, 0.2, 0.3)),
                        lc.config(class_weights=np.array([0.5 + 0.1 * i for i in range(16)], np.float32), label_smoothing=0.05), gpu_device)
    against_restatement("C=2", make_inputs(77, c=2, seed=6, mix=(0.6, 0.4)), lc.config(), gpu_device)


# ---- batch scale --------------------------------------------------------------------------------------------------------------------
def test_batch_scale_and_repeatability(gpu_device):
    n = 1 << 20
    inp = make_inputs(n, seed=2026, mix=(0.90, 0.02, 0.08))
    cfg = lc.config(class_weights=W3, label_smoothing=0.1)
    crit, vals, grads = against_restatement("1M", inp, cfg, gpu_device)
    crit2 = criterion(cfg, gpu_device)
    outputs, targets = to_device(inp, gpu_device)
    losses = crit2(outputs, targets)
    losses["total"].backward()
    for k in lc.TERMS:
        a, b = np.float32(vals[k]), losses[k].detach().cpu().numpy()
        assert a.tobytes() == b.tobytes(), k
    for k in GRADS:
        assert np.array_equal(grads[k].view(np.uint32), outputs[k].grad.cpu().numpy().view(np.uint32)), k
    assert torch.equal(crit.last_stats["confusion"], crit2.last_stats["confusion"])


# ---- autograd -----------------------------------------------------------------------------------------------------------------------
def test_backward_on_one_term_and_on_a_combination(gpu_device):
    inp = make_inputs(3 * R + 5, seed=41)
    cfg = lc.config(class_weights=W3, label_smoothing=0.1)
    _, _, g = run_gpu(inp, cfg, gpu_device, combine=lambda l: l["classification"])
    check_grads("classification alone", {"class_logits": g["class_logits"]}, {"class_logits": lc.grads(inp, cfg, (1.0, 0.0, 0.0))["class_logits"]})
    assert g["confidence"] is not None and not g["confidence"].any() and not g["correction"].any()
    # 2 total + confidence: upstream (2 w_cls, 2 w_conf + 1, 2 w_corr); the device forms it in float32 (two roundings, each half
    # an ulp) before the kernel's single rounding of the element: 2 ulp
    tw = cfg["term_weights"]
    _, _, g = run_gpu(inp, cfg, gpu_device, combine=lambda l: 2 * l["total"] + l["confidence"])
    check_grads("2 total + confidence", g, lc.grads(inp, cfg, (2 * tw[0], 2 * tw[2] + 1.0, 2 * tw[1])), ulps=2.0)
    # terms without a gradient
    crit = criterion(cfg, gpu_device)
    outputs, targets = to_device(inp, gpu_device)
    losses = crit(outputs, targets)
    assert not losses["feature_preservation"].requires_grad and not losses["shoal_safety"].requires_grad
    assert losses["total"].requires_grad and losses["correction"].requires_grad


def test_no_grad_gives_the_same_bits(gpu_device):
    inp = make_inputs(2 * R + 9, seed=43)
    cfg = lc.config(label_smoothing=0.1)
    crit = criterion(cfg, gpu_device)
    outputs, targets = to_device(inp, gpu_device)
    a = crit(outputs, targets)
    with torch.no_grad():
        b = crit(outputs, targets)
    for k in lc.TERMS:
        assert b[k].grad_fn is None and not b[k].requires_grad
        assert a[k].detach().cpu().numpy().tobytes() == b[k].cpu().numpy().tobytes(), k
    assert a["total"].grad_fn is not None


def test_bad_label_is_nan_not_an_assert(gpu_device):
    inp = make_inputs(R + 1, seed=47)
    inp["class_labels"][5] = 7
    inp["class_labels"][R] = -3
    cfg = lc.config()
    crit, vals, grads = run_gpu(inp, cfg, gpu_device)
    assert np.isnan(vals["classification"]) and np.isnan(vals["total"])
    want = lc.loss(inp, cfg)
    for k in ("correction", "confidence", "feature_preservation", "shoal_safety"):
        assert abs(vals[k] - float(want[k])) <= ULP * abs(float(want[k])), k
    assert int(crit.last_stats["n_invalid"]) == 2 and int(crit.last_stats["n_ignored"]) == 0
    check_grads("bad labels", grads, lc.grads(inp, cfg))
    torch.cuda.synchronize()                          # (the device is still alive: no assert fired)


def test_refusals(gpu_device):
    inp = make_inputs(10, c=17, seed=1, mix=(1, 1, 1))
    outputs, targets = to_device(inp, gpu_device)
    with pytest.raises(ValueError, match="classes"):
        BathymetricGNNLoss()(outputs, targets)
    inp = make_inputs(10, seed=1)
    outputs, targets = to_device(inp, gpu_device)
    with pytest.raises(ValueError, match="class_weights"):
        BathymetricGNNLoss(class_weights=torch.ones(4, device=gpu_device))(outputs, targets)
    targets["noise_mask"] = targets["noise_mask"].long()
    with pytest.raises(TypeError, match="noise_mask"):
        BathymetricGNNLoss()(outputs, targets)


def test_c_entry_points_refuse_bad_arguments(gpu_device):
    """The C ABI itself: refused calls name the reason, return BGNN_ERR_INVALID / UNSUPPORTED and launch nothing."""
    import ctypes as C
    from bathymetric_gnn_amd import runtime as rt
    ctx = rt.get_context(gpu_device)
    lib, n = ctx.lib, 100
    inp = make_inputs(n, seed=3)
    outputs, targets = to_device(inp, gpu_device, grad=False)
    li = rt.LossInputs(outputs["class_logits"].data_ptr(), outputs["confidence"].data_ptr(), outputs["correction"].data_ptr(),
                       outputs["predicted_class"].data_ptr(), targets["class_labels"].data_ptr(),
                       targets["correction_targets"].data_ptr(), targets["noise_mask"].view(torch.uint8).data_ptr())
    params = BathymetricGNNLoss()._params(3)
    nbytes = lib.bgnn_loss_workspace_bytes(n)
    ws = torch.zeros(nbytes, dtype=torch.uint8, device=gpu_device)
    terms = torch.full((6,), -1.0, device=gpu_device)
    counts = torch.full((16,), -1, dtype=torch.int64, device=gpu_device)

    def fwd(p=params, rows=n, ws_bytes=nbytes):
        return lib.bgnn_loss_forward(ctx.handle, C.byref(p), rows, C.byref(li), rt.ptr(ws), ws_bytes, rt.ptr(terms), rt.ptr(counts))
    assert fwd(rows=0) == rt.ERR_INVALID
    assert fwd(ws_bytes=nbytes - 256) == rt.ERR_INVALID and b"workspace" in lib.bgnn_last_error()
    assert fwd(rows=(1 << 30) + 1) == rt.ERR_UNSUPPORTED
    bad = BathymetricGNNLoss()._params(3)
    bad.num_classes = 17
    assert fwd(p=bad) == rt.ERR_INVALID and b"classes" in lib.bgnn_last_error()
    bad = BathymetricGNNLoss(correction_delta=0.0)._params(3)
    assert fwd(p=bad) == rt.ERR_INVALID and b"delta" in lib.bgnn_last_error()
    up = torch.ones(3, device=gpu_device)
    assert lib.bgnn_loss_backward(ctx.handle, C.byref(params), n, C.byref(li), None, rt.ptr(up), None, None, None) == rt.ERR_INVALID
    torch.cuda.synchronize()
    assert bool((terms == -1).all()) and bool((counts == -1).all()) and not bool(ws.any())       # nothing was launched
    assert fwd() == 0
    torch.cuda.synchronize()
    want = lc.loss(inp, lc.config())
    assert abs(float(terms[5]) - float(want["total"])) <= ULP * float(want["total"])


# ---- through the model --------------------------------------------------------------------------------------------------------------
class _ModelLoss:
    """``total`` of BathymetricGNNLoss on the device outputs; on the oracle's (CPU) outputs the same loss restated with torch
    operations in the outputs' dtype.  The predicted classes are data, not a function of the parameters: the ones the GPU step
    produced are held and used by both oracle runs, so that a near-tie that rounding flips cannot change the loss between them."""

    def __init__(self, y, target, nmask, dev):
        self.y, self.target, self.nmask = y, target, nmask
        self.class_w = compute_class_weights(y)
        self.delta = compute_correction_delta(target[nmask].cpu().numpy())
        self.crit = BathymetricGNNLoss(class_weights=self.class_w, label_smoothing=0.1, correction_delta=self.delta)
        self.pred = None

    def __call__(self, out):
        logits = out["class_logits"]
        if logits.is_cuda:
            self.pred = out["predicted_class"].cpu()
            return self.crit(out, {"class_labels": self.y, "correction_targets": self.target, "noise_mask": self.nmask})["total"]
        dt = logits.dtype
        y, q, tgt, mask = self.y.cpu(), self.pred, self.target.cpu().to(dt), self.nmask.cpu()
        c = self.crit
        cls = F.cross_entropy(logits, y, weight=self.class_w.cpu().to(dt), label_smoothing=0.1)
        corr = F.huber_loss(out["correction"][mask], tgt[mask], delta=self.delta)
        conf = F.binary_cross_entropy(out["confidence"], (q == y).to(dt))
        feat = 2.0 * ((y == 1) & (q == 2)).to(dt).mean()
        fp = (y == 0) & (q == 2)
        shoal = (3.0 * (fp & (tgt < 0)).sum() + 1.0 * (fp & ~(tgt < 0)).sum()).to(dt) / max(int(fp.sum()), 1)
        return (c.classification_weight * cls + c.correction_weight * corr + c.confidence_weight * conf +
                c.feature_preservation_weight * feat + c.shoal_safety_weight * shoal)


def _noisy_batch(tiles, dev, seed):
    """Two clean tiles -> the generator's noisy batch, the device graph and the oracle's graph of the NOISY tiles, and the
    per-node targets of ``training_targets``."""
    hw = np.array([t[0].shape for t in tiles], np.int32)
    clean_t = torch.from_numpy(np.concatenate([t[0].ravel() for t in tiles])).to(dev)
    mask_t = torch.from_numpy(np.concatenate([t[1].ravel() for t in tiles]).view(np.uint8)).to(dev)
    b = SyntheticNoiseGenerator(seed=seed).generate_batch(hw, clean_t, mask_t)
    noisy, off, noisy_tiles = b.noisy_depth.cpu().numpy(), 0, []
    for d, m, _ in tiles:
        noisy_tiles.append((noisy[off:off + d.size].reshape(d.shape), m, None))
        off += d.size
    g, x, ei, ea = _tiles_graph(noisy_tiles)
    y, target, nmask = training_targets(g, clean_t, b.noisy_depth, b.classification, b.noise_mask)
    assert int(nmask.sum()) > 0 and int((~nmask).sum()) > 0
    return g, x, ei, ea, y, target, nmask


@pytest.mark.parametrize("kind", ["GAT", "GraphSAGE", "GIN"])
def test_through_the_model(kind, gpu_device, monkeypatch):
    """Two unequal V1 tiles, 3 layers, dropout 0.1, targets from the noise generator: ``total.backward()`` fills every
    parameter's gradient, held to the rule of the backward tests against the oracle's float64 / float32 autograd."""
    g, x, ei, ea, y, target, nmask = _noisy_batch([_tile(37, 45, 3, "V1"), _tile(30, 40, 4, "V1")], gpu_device, seed=31)
    loss = _ModelLoss(y, target, nmask, gpu_device)
    if kind == "GAT":
        sd = _gat_sd(in_channels=7, num_layers=3, seed=141)
        m = _gat_net(sd, num_gnn_layers=3)
        drop = _dropout(m, 5, 0.1, 0.1)
    else:
        sd = plain._sd(kind, num_layers=3, seed=141)
        m = plain._net(sd, kind, num_gnn_layers=3)
        drop = plain._drop(m, 5, 0.1, 0.1)
    g_gpu, out = _step(m, g, loss, 5)
    assert all(p.grad is not None and bool(torch.isfinite(p.grad).all()) for p in m.parameters())
    assert loss.crit.last_stats is not None and int(loss.crit.last_stats["confusion"].sum()) == x.shape[0]
    if kind == "GAT":
        g64, g32 = _oracle_for(m, out, x.shape[0], sd, x, ei, ea, drop, loss, monkeypatch)
    else:
        g64, g32 = plain._oracle(m, out, x.shape[0], sd, x, ei, ea, drop, loss, monkeypatch)
    _accept("loss", f"{kind} through BathymetricGNNLoss", g_gpu, g64, g32)


# ---- a short trajectory -------------------------------------------------------------------------------------------------------------
def test_short_training_trajectory(gpu_device):
    """12 steps of AdamW with clip_grad_norm_(1.0) on one 32 x 40 tile under the fused loss: the parameters stay finite and the
    dropout-free total of the trained model is below the initial model's."""
    g, x, ei, ea, y, target, nmask = _noisy_batch([_tile(32, 40, 8, "V1")], gpu_device, seed=17)
    crit = BathymetricGNNLoss(class_weights=compute_class_weights(y), label_smoothing=0.1,
                              correction_delta=compute_correction_delta(target[nmask].cpu().numpy()))
    targets = {"class_labels": y, "correction_targets": target, "noise_mask": nmask}
    sd = _gat_sd(in_channels=7, num_layers=3, seed=125)

    def dropout_free_total(m):
        _dropout(m, 0, 0.0, 0.0)
        with torch.no_grad():
            m.train()
            return float(crit(m(g), targets)["total"])
    m = _gat_net(sd, num_gnn_layers=3)
    start = dropout_free_total(m)
    opt = torch.optim.AdamW(m.parameters(), lr=1e-3)
    seen = []
    for step in range(12):
        _dropout(m, step, 0.1, 0.1)
        m.train(); m.dropout_seed = step
        opt.zero_grad(set_to_none=True)
        total = crit(m(g), targets)["total"]
        total.backward()
        torch.nn.utils.clip_grad_norm_(m.parameters(), 1.0)
        opt.step()
        seen.append(total.detach())
    assert all(bool(torch.isfinite(p).all()) for p in m.parameters())
    end = dropout_free_total(m)
    print(f"totals {[round(float(v), 5) for v in seen]}; dropout-free total {start:.5f} -> {end:.5f}")
    assert end < start
