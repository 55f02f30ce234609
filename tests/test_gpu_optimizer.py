"""Fused gradient clipping + AdamW on the weight blob (``bgnn_adamw_step``), the in-place refresh of the packed model
(``bgnn_model_refresh`` / ``model_sync``) and ``training.FusedAdamW`` on top of them.

Acceptance rule of the step (the project's own, ``tests/_conditioning.py`` / ``test_gpu_backward_training._accept``): per parameter
max |p_gpu - p64| <= BOUND_C * max |p32 - p64| + FLOOR_REL * max |p64|, where p64 / p32 are ``clip_grad_norm_`` +
``torch.optim.AdamW`` on the CPU in float64 / float32 over the same per-parameter tensors; the same for ``exp_avg`` and
``exp_avg_sq``.  The refresh is held to bit identity with a fresh model that takes the host pack path."""
import copy
import ctypes as C
import math

import numpy as np
import pytest
import torch

from _conditioning import BOUND_C
from test_gpu_backward import FLOOR_REL, _loss, _loss_weights, _model, _set_dropout, _tiles_graph
from test_gpu_backward_training import _tile

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

LAYOUTS = {
    "gat-small": dict(gnn_type="GAT", in_channels=7, hidden=32, num_layers=1),            # a few thousand weights, odd count
    "gat-default": dict(gnn_type="GAT", in_channels=7),                                   # ~1/4 M weights: many reduction blocks
    "sage": dict(gnn_type="GraphSAGE", in_channels=7),
    "gin": dict(gnn_type="GIN", in_channels=7),
}


def _cpu_model(edge_dim=3, **kw):
    """(CPU BathymetricGNN holding synthetic weights, its state dict)"""
    from bathymetric_gnn_amd import synthetic
    from bathymetric_gnn_amd.models import BathymetricGNN
    sd = synthetic.synthetic_state_dict(seed=77, **kw)
    if edge_dim is None:
        sd = {k: v for k, v in sd.items() if "att_edge" not in k and "lin_edge" not in k}
    m = BathymetricGNN(in_channels=kw["in_channels"], hidden_channels=kw.get("hidden", 64), num_gnn_layers=kw.get("num_layers", 4),
                       gnn_type=kw["gnn_type"], edge_dim=edge_dim)
    m.load_state_dict({k: torch.as_tensor(v) for k, v in sd.items()})
    return m


def _graph():
    return _tiles_graph([_tile(37, 45, 3, "V1"), _tile(30, 40, 4, "V1")])


# ---- 1. the step against torch on the CPU -------------------------------------------------------------------------------------

def _grad_steps(slots, n, steps, target_norm, seed, zero=False):
    """``steps`` float32 gradient blobs: seeded normal values on the parameter slots, scaled to total norm ~ target_norm."""
    r = np.random.default_rng(seed)
    out = []
    for _ in range(steps):
        g = np.zeros(n, np.float32)
        if not zero:
            for name, off, cnt in slots:
                if name is not None:
                    g[off:off + cnt] = r.standard_normal(cnt)
            g *= np.float32(target_norm / np.sqrt(np.sum(g.astype(np.float64) ** 2)))
        out.append(g)
    return out


def _torch_reference(blob, slots, grads, skip, dtype, lr, wd, max_norm):
    """clip_grad_norm_ + AdamW on the CPU over per-parameter tensors; ``skip[(step, name)]``: that .grad is None.  Returns
    ({name: p}, {name: exp_avg}, {name: exp_avg_sq}, {name: steps taken}, [total norms])."""
    ps = {name: torch.tensor(blob[off:off + cnt], dtype=dtype, requires_grad=True) for name, off, cnt in slots if name is not None}
    opt = torch.optim.AdamW(list(ps.values()), lr=lr, weight_decay=wd, foreach=False)
    norms = []
    for s, g in enumerate(grads):
        for name, off, cnt in slots:
            if name is not None:
                ps[name].grad = None if (s, name) in skip else torch.tensor(g[off:off + cnt], dtype=dtype)
        live = [p for p in ps.values() if p.grad is not None]
        if max_norm is not None:
            norms.append(float(torch.nn.utils.clip_grad_norm_(live, max_norm, foreach=False)))
        else:
            norms.append(float(torch.sqrt(sum((p.grad.double() ** 2).sum() for p in live))))
        opt.step()
    st = {name: opt.state.get(p, {}) for name, p in ps.items()}
    zeros = lambda name: torch.zeros_like(ps[name])
    return ({k: v.detach() for k, v in ps.items()}, {k: st[k].get("exp_avg", zeros(k)) for k in ps},
            {k: st[k].get("exp_avg_sq", zeros(k)) for k in ps}, {k: int(st[k]["step"]) if st[k] else 0 for k in ps}, norms)


def _gpu_steps(blob, slots, grads, skip, lr, wd, max_norm, betas=(0.9, 0.999), eps=1e-8):
    """The same through bgnn_adamw_step on flat device blobs.  Returns (weights, exp_avg, exp_avg_sq) as CPU float32 arrays, the
    per-parameter step counts and the returned norms."""
    from bathymetric_gnn_amd import runtime as rt
    dev = torch.device(DEV)
    ctx = rt.get_context(dev)
    w = torch.from_numpy(blob.copy()).to(dev)
    m1, m2 = torch.zeros_like(w), torch.zeros_like(w)
    count = {name: 0 for name, _, _ in slots if name is not None}
    norms = []
    prm = rt.AdamWParams(lr, betas[0], betas[1], eps, wd, 0.0 if max_norm is None else max_norm)
    for s, g in enumerate(grads):
        gd = torch.from_numpy(g).to(dev)
        live = [(name, off, cnt) for name, off, cnt in slots if name is not None and (s, name) not in skip]
        tab = (rt.AdamWSlot * len(live))()
        for k, (name, off, cnt) in enumerate(live):
            count[name] += 1
            tab[k].offset, tab[k].count, tab[k].step = off, cnt, count[name]
        norm = torch.full((), -1.0, dtype=torch.float32, device=dev)
        ctx.begin()
        rt.check(ctx.lib.bgnn_adamw_step(ctx.handle, rt.ptr(w), rt.ptr(gd), rt.ptr(m1), rt.ptr(m2), w.numel(), tab, len(live),
                                         C.byref(prm), rt.ptr(norm)))
        ctx.end()
        norms.append(float(norm))
    return w.cpu().numpy(), m1.cpu().numpy(), m2.cpu().numpy(), count, norms


def _accept_step(what, gpu, slots, r64, r32):
    bad, worst = [], 0.0
    for name, off, cnt in slots:
        if name is None:
            continue
        v = torch.from_numpy(gpu[off:off + cnt]).double()
        d = (v - r64[name]).abs().max().item()
        d32 = (r32[name].double() - r64[name]).abs().max().item()
        bound = BOUND_C * d32 + FLOOR_REL * r64[name].abs().max().item()
        worst = max(worst, d / bound if bound > 0 else (0.0 if d == 0 else math.inf))
        if not d <= bound:
            bad.append(f"{what} {name}: gpu {d:.3e} f32 {d32:.3e} bound {bound:.3e}")
    print(f"  {what}: worst d / bound {worst:.3f}")
    assert not bad, "\n".join(bad)


def _check_step(layout, steps, target_norm, max_norm, wd, edge_dim=3, skip=(), zero=False, lr=1e-3):
    m = _cpu_model(edge_dim=edge_dim, **LAYOUTS[layout])
    slots = m.grad_slots(3)
    blob = m.pack_weights(3)
    n = blob.size
    grads = _grad_steps(slots, n, steps, target_norm, seed=steps * 100 + int(target_norm), zero=zero)
    skip = set(skip)
    p64, a64, b64, c64, n64 = _torch_reference(blob, slots, grads, skip, torch.float64, lr, wd, max_norm)
    p32, a32, b32, _, _ = _torch_reference(blob, slots, grads, skip, torch.float32, lr, wd, max_norm)
    w, m1, m2, count, norms = _gpu_steps(blob, slots, grads, skip, lr, wd, max_norm)
    print(f"{layout} n={n} steps={steps} norm~{target_norm} max_norm={max_norm} wd={wd}: norms gpu {norms} f64 {n64}")
    _accept_step("param", w, slots, p64, p32)
    _accept_step("exp_avg", m1, slots, a64, a32)
    _accept_step("exp_avg_sq", m2, slots, b64, b32)
    for a, b in zip(norms, n64):
        assert abs(a - b) <= 1e-6 * abs(b), (a, b)
    assert count == c64
    # what no slot lists is not touched at all: running statistics, the zero edge weights of an edge_dim=None model
    for name, off, cnt in slots:
        if name is None:
            assert np.array_equal(w[off:off + cnt].view(np.uint32), blob[off:off + cnt].view(np.uint32))
            assert not m1[off:off + cnt].any() and not m2[off:off + cnt].any()
    return m, slots, blob, w, m1, m2


@pytest.mark.parametrize("wd", [0.0, 1e-2])
@pytest.mark.parametrize("max_norm", [None, 1.0])
@pytest.mark.parametrize("target_norm", [0.3, 30.0])
@pytest.mark.parametrize("steps", [1, 5])
@pytest.mark.parametrize("layout", list(LAYOUTS))
def test_step_parity(layout, steps, target_norm, max_norm, wd, gpu_device):
    """max_norm None; 1.0 with the norm below it (the coefficient clamps to 1) and above it; weight decay off and on; 1 and 5 steps;
    every backbone's layout.  Running-statistics slots stay bit-unchanged."""
    m, slots, *_ = _check_step(layout, steps, target_norm, max_norm, wd)
    assert any(name is None for name, _, _ in slots)                  # (the running statistics are in the blob and not listed)
    assert sum(cnt for _, _, cnt in slots) % 2 == 1 or layout != "gat-small"


@pytest.mark.parametrize("layout", ["gat-small", "gat-default"])
def test_step_all_zero_gradient(layout, gpu_device):
    """g = 0: the norm is 0, the coefficient clamps to 1, the moments stay 0 and only the weight decay moves the weights."""
    _, slots, blob, w, m1, m2 = _check_step(layout, 2, 0.0, 1.0, 1e-2, zero=True)
    assert not m1.any() and not m2.any()
    name, off, cnt = next(s for s in slots if s[0] is not None)
    assert not np.array_equal(w[off:off + cnt], blob[off:off + cnt])


@pytest.mark.parametrize("layout", ["gat-small", "gat-default"])
def test_step_parameter_without_gradient(layout, gpu_device):
    """One parameter has ``.grad is None`` in step 2 of 5: torch skips it entirely there (no decay, no moment update, no step
    count) -- the slot is simply not listed, and its bias correction goes on from its own count."""
    m = _cpu_model(**LAYOUTS[layout])
    names = [n for n, _, _ in m.grad_slots(3) if n is not None]
    victim = names[len(names) // 2]
    _, slots, blob, w, m1, m2 = _check_step(layout, 5, 30.0, 1.0, 1e-2, skip=[(2, victim)])
    # and a single step in which it is skipped leaves it bit-unchanged
    grads = _grad_steps(slots, blob.size, 1, 30.0, seed=5)
    w1, a1, b1, count, _ = _gpu_steps(blob, slots, grads, {(0, victim)}, 1e-3, 1e-2, 1.0)
    off, cnt = next((o, c) for n, o, c in slots if n == victim)
    assert np.array_equal(w1[off:off + cnt].view(np.uint32), blob[off:off + cnt].view(np.uint32))
    assert not a1[off:off + cnt].any() and not b1[off:off + cnt].any() and count[victim] == 0


def test_step_edge_dim_none_filler_stays_zero(gpu_device):
    """An ``edge_dim=None`` GAT: the blob carries zeros where att_edge / lin_edge would be; no slot lists them, they stay exactly 0."""
    m, slots, blob, w, m1, m2 = _check_step("gat-default", 3, 30.0, 1.0, 1e-2, edge_dim=None)
    sd_keys = set(m.state_dict())
    filler = [(off, cnt) for name, off, cnt in slots if name is None and cnt > 0]
    stats = sum(1 for k in sd_keys if k.endswith(("running_mean", "running_var")))
    assert len(filler) == stats + 2 * m.num_gnn_layers                # (running statistics + two filler slots per layer)
    n_zero = 0
    for name, off, cnt in slots:
        if name is None and not blob[off:off + cnt].any():
            assert not w[off:off + cnt].view(np.uint32).any()
            n_zero += 1
    assert n_zero >= 2 * m.num_gnn_layers


def test_step_refuses_bad_tables(gpu_device):
    from bathymetric_gnn_amd import runtime as rt
    ctx = rt.get_context(torch.device(DEV))
    w = torch.zeros(100, device=DEV)
    prm = rt.AdamWParams(1e-3, 0.9, 0.999, 1e-8, 0.0, 0.0)
    for bad in ([(90, 20, 1)], [(0, 10, 0)], [(0, 10, 1), (5, 10, 1)]):
        tab = (rt.AdamWSlot * len(bad))(*[rt.AdamWSlot(*b) for b in bad])
        with pytest.raises(ValueError):
            rt.check(ctx.lib.bgnn_adamw_step(ctx.handle, rt.ptr(w), rt.ptr(w), rt.ptr(w), rt.ptr(w), 100, tab, len(bad), C.byref(prm), None))


# ---- 2. FusedAdamW ------------------------------------------------------------------------------------------------------------

def _gpu_model(kind="GAT", seed=125, dropout=0.1, **kw):
    from bathymetric_gnn_amd import synthetic
    sdkw = dict(in_channels=7, gnn_type=kind, seed=seed)
    mkw = dict(in_channels=7, gnn_type=kind, edge_dim=3, dropout=dropout)
    for a, b in (("hidden", "hidden_channels"), ("num_layers", "num_gnn_layers"), ("heads", "heads")):
        if a in kw:
            sdkw[a] = mkw[b] = kw[a]
    sd = synthetic.synthetic_state_dict(**sdkw)
    return _model(sd, torch.device(DEV), **mkw), mkw


def _fresh(m, mkw):
    """A new model holding ``m``'s weights: it takes the host pack path (pack_weights + bgnn_model_create)."""
    sd = {k: v.detach().cpu().clone() for k, v in m.state_dict().items()}
    f = _model(sd, torch.device(DEV), **mkw)
    _set_dropout(f, m.gnn.dropout)
    f.feature_extractor.mlp[2].p = m.feature_extractor.mlp[2].p
    return f


def _seeded_grads(m, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    for p in m.parameters():
        p.grad = (torch.randn(p.shape, generator=g) * scale).to(p.device)


def _equal_outputs(a, b, what):
    assert set(a) == set(b)
    for k in a:
        assert torch.equal(a[k], b[k]), f"{what}: {k} differs (max {(a[k].double() - b[k].double()).abs().max().item():.3e})"


def _train_forward(m, g, seed):
    m.train()
    m.dropout_seed = seed
    with torch.no_grad():
        return {k: v.clone() for k, v in m(g).items()}


def test_determinism(gpu_device):
    """Two optimizers over equal models and equal gradients: master, moments and norm are bit-identical after 3 steps."""
    from bathymetric_gnn_amd.training import FusedAdamW
    res = []
    for _ in range(2):
        m, _ = _gpu_model()
        opt = FusedAdamW(m, lr=1e-3, max_grad_norm=1.0)
        for s in range(3):
            _seeded_grads(m, 50 + s, 0.05)
            opt.step()
        res.append((m._flat_ok()["master"].clone(), opt._m1.clone(), opt._m2.clone(), opt.last_grad_norm.clone()))
    for a, b in zip(*res):
        assert torch.equal(a, b)
    assert res[0][3].dim() == 0 and res[0][3].is_cuda and float(res[0][3]) > 0


REFRESH_CASES = {
    "gat-default": dict(kind="GAT"),
    "gat-h32-heads8": dict(kind="GAT", hidden=32, heads=8),
    "gat-1-layer": dict(kind="GAT", num_layers=1),
    "sage": dict(kind="GraphSAGE"),
    "gin": dict(kind="GIN"),
}


@pytest.mark.parametrize("fold", [0, 1])
@pytest.mark.parametrize("case", list(REFRESH_CASES))
def test_refresh_identity(case, fold, gpu_device):
    """After each of 3 FusedAdamW steps on real gradients the training forward equals, bit for bit, that of a fresh model loaded
    from the trained model's state_dict(); then every eval entry point does (each one made stale again first: model_sync)."""
    from bathymetric_gnn_amd import runtime as rt
    from bathymetric_gnn_amd.data import GraphBuilder
    from bathymetric_gnn_amd.models.pipeline import TileBatchEngine
    from bathymetric_gnn_amd.training import FusedAdamW
    ctx = rt.get_context(torch.device(DEV))
    old = ctx.get_option("fold_extractor")
    ctx.set_option("fold_extractor", fold)
    try:
        kw = dict(REFRESH_CASES[case])
        m, mkw = _gpu_model(kw.pop("kind"), **kw)
        # (one case: a graph built with a non-default edge feature list -- the eval forward then takes the canonical-V tables)
        ef = ["slope", "distance", "depth_difference"] if case == "gat-default" and fold == 1 else None
        tiles = [_tile(37, 45, 3, "V1"), _tile(30, 40, 4, "V1")]
        g, x, _, _ = _tiles_graph(tiles, edge_features=ef)
        w = {k: v / x.shape[0] for k, v in _loss_weights(x.shape[0], 3, seed=9).items()}
        if ef is not None:
            m.eval()
            with torch.no_grad():
                m(g)                                                  # the table exists before the first refresh
        opt = FusedAdamW(m, lr=1e-3, max_grad_norm=1.0)
        for step in range(3):
            m.train(); m.dropout_seed = step
            opt.zero_grad()
            _loss(m(g), w).backward()
            opt.step()
            f = _fresh(m, mkw)
            _equal_outputs(_train_forward(m, g, 100 + step), _train_forward(f, g, 100 + step), f"training forward after step {step}")
        f = _fresh(m, mkw)
        stale = lambda: m._refresh_native(rt.REFRESH_ALL)              # (the packed model's eval images lag again)
        stale()
        with torch.no_grad():
            _equal_outputs(m.eval()(g), f.eval()(g), "eval forward")
        stale()
        _equal_outputs(m.predict(g), f.predict(g), "predict")
        xg = torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).to(DEV)
        stale()
        hm, hf = m.feature_extractor(xg), f.feature_extractor(xg)
        assert torch.equal(hm, hf), "feature_extractor"
        stale()
        assert torch.equal(m.classification_head(hm), f.classification_head(hf)), "classification_head"
        stale()
        gb = GraphBuilder(edge_features=ef)
        args = ([t[0] for t in tiles], [t[1] for t in tiles], None, [(0.5, 0.5)] * 2)
        rm, rf = TileBatchEngine(m, gb, gpu_device).infer(*args), TileBatchEngine(f, gb, gpu_device).infer(*args)
        for a, b in zip(rm, rf):
            for k in a:
                assert np.array_equal(a[k], b[k], equal_nan=True), f"TileBatchEngine.infer: {k}"
    finally:
        ctx.set_option("fold_extractor", old)


def _noisy_targets(n):
    r = np.random.default_rng(0)
    labels = torch.from_numpy(r.choice(3, size=n, p=(0.90, 0.02, 0.08))).to(DEV)
    return {"class_labels": labels, "noise_mask": labels == 2,
            "correction_targets": torch.from_numpy(r.standard_normal(n).astype(np.float32)).to(DEV)}


def test_no_repack(gpu_device, monkeypatch):
    """pack_weights is not called by forward / loss / backward / step on a flattened model, nor by an eval forward afterwards;
    replacing a parameter by hand or load_state_dict goes back to the host repack, and the next step() is still right."""
    from bathymetric_gnn_amd.models import BathymetricGNN
    from bathymetric_gnn_amd.training import BathymetricGNNLoss, FusedAdamW, compute_class_weights
    calls = []
    real = BathymetricGNN.pack_weights
    monkeypatch.setattr(BathymetricGNN, "pack_weights", lambda self, *a, **k: (calls.append(1), real(self, *a, **k))[1])
    m, mkw = _gpu_model()
    g, x, _, _ = _graph()
    targets = _noisy_targets(x.shape[0])
    crit = BathymetricGNNLoss(class_weights=compute_class_weights(targets["class_labels"]), label_smoothing=0.1)
    opt = FusedAdamW(m, lr=1e-3, max_grad_norm=1.0)
    n0 = len(calls)

    def iteration(seed):
        m.train(); m.dropout_seed = seed
        opt.zero_grad()
        crit(m(g), targets)["total"].backward()
        opt.step()

    for it in range(4):
        iteration(it)
    assert len(calls) == n0, "a training step repacked the weights through the host"
    with torch.no_grad():
        m.eval()(g)
    assert len(calls) == n0, "the eval forward repacked through pack_weights (model_sync should have completed the images)"
    # a parameter replaced by hand: the views are broken, the host repack takes over ...
    with torch.no_grad():
        m.classification_head.mlp[3].bias = torch.nn.Parameter(m.classification_head.mlp[3].bias.detach().clone() + 0.25)
    _train_forward(m, g, 7)
    assert len(calls) > n0
    # ... and the next step() flattens again and is right (the new parameter object is the one that moves)
    iteration(8)
    assert m._flat_ok() is not None
    _equal_outputs(_train_forward(m, g, 9), _train_forward(_fresh(m, mkw), g, 9), "after a replaced parameter")
    n1 = len(calls)
    iteration(10)
    assert len(calls) == n1
    # load_state_dict
    m.load_state_dict({k: v.detach().cpu().clone() * 1.0 for k, v in m.state_dict().items()})
    _train_forward(m, g, 11)
    assert len(calls) > n1
    iteration(12)
    _equal_outputs(_train_forward(m, g, 13), _train_forward(_fresh(m, mkw), g, 13), "after load_state_dict")
    n2 = len(calls)
    iteration(14)
    assert len(calls) == n2


def test_autograd_guard(gpu_device):
    from bathymetric_gnn_amd.training import FusedAdamW
    m, _ = _gpu_model()
    g, x, _, _ = _graph()
    w = {k: v / x.shape[0] for k, v in _loss_weights(x.shape[0], 3, seed=9).items()}
    opt = FusedAdamW(m)
    m.train(); m.dropout_seed = 1
    loss = _loss(m(g), w)
    loss.backward(retain_graph=True)
    opt.step()
    with pytest.raises(RuntimeError, match="modified by an inplace operation"):
        loss.backward()


def test_constructor_refusals(gpu_device):
    from bathymetric_gnn_amd.models import BathymetricGNN
    from bathymetric_gnn_amd.training import FusedAdamW
    m, _ = _gpu_model()
    m2, _ = _gpu_model()
    for bad, kw in ((m, dict(amsgrad=True)), (m, dict(maximize=True)), ([{"params": list(m.parameters())}, {"params": []}], {}),
                    ([m, m2], {}), (list(m.parameters()), {}), (BathymetricGNN(in_channels=7, edge_dim=3), {}),
                    (BathymetricGNN(in_channels=7, edge_dim=3).to(DEV).double(), {}),
                    (BathymetricGNN(in_channels=7, edge_dim=3, hidden_channels=48).to(DEV), {}),
                    (BathymetricGNN(in_channels=7, edge_dim=3, heads=3).to(DEV), {})):
        with pytest.raises(ValueError):
            FusedAdamW(bad, **kw)
    opt = FusedAdamW(m, lr=2e-3, weight_decay=0.0)
    assert len(opt.param_groups) == 1 and opt.param_groups[0]["lr"] == 2e-3 and opt.param_groups[0]["weight_decay"] == 0.0
    assert [id(p) for p in opt.param_groups[0]["params"]] == [id(p) for p in m.parameters()]
    _seeded_grads(m, 1)
    opt.zero_grad()
    assert all(p.grad is None for p in m.parameters())
    # .to() keeps working (the views break, the host repack takes over)
    m.to("cpu"); m.to(DEV)
    assert m._flat_ok() is None


def test_checkpoint_moves_between_optimizers(gpu_device):
    """FusedAdamW.state_dict() loads into torch.optim.AdamW over the same weights and back; one further step from the checkpoint
    passes the parity rule (torch's float32 step on the GPU is the float32 yardstick, a float64 CPU AdamW the reference)."""
    from bathymetric_gnn_amd.training import FusedAdamW
    m1, mkw = _gpu_model()
    f1 = FusedAdamW(m1, lr=1e-3, weight_decay=1e-2)
    for s in range(2):
        _seeded_grads(m1, 20 + s, 0.05)
        f1.step()
    ck = f1.state_dict()
    assert set(ck["state"]) == set(range(len(list(m1.parameters()))))
    assert all(set(v) == {"step", "exp_avg", "exp_avg_sq"} and float(v["step"]) == 2.0 for v in ck["state"].values())
    names = [n for n, _ in m1.named_parameters()]
    # into torch.optim.AdamW: float32 on the GPU, and float64 on the CPU
    m2 = _fresh(m1, mkw)
    t2 = torch.optim.AdamW(m2.parameters(), lr=1e-3, weight_decay=1e-2, foreach=False)
    t2.load_state_dict(copy.deepcopy(ck))           # (torch keeps the checkpoint's own `step` tensors: one copy per optimizer)
    p64 = [p.detach().cpu().double().requires_grad_() for p in m1.parameters()]
    t64 = torch.optim.AdamW(p64, lr=1e-3, weight_decay=1e-2, foreach=False)
    t64.load_state_dict(copy.deepcopy(ck))
    # ... and back, into a second FusedAdamW
    m3 = _fresh(m1, mkw)
    f3 = FusedAdamW(m3, lr=5e-4, weight_decay=0.0)
    f3.load_state_dict(t2.state_dict())
    assert f3.param_groups[0]["lr"] == 1e-3 and f3.param_groups[0]["weight_decay"] == 1e-2
    for m in (m1, m2, m3):
        _seeded_grads(m, 30, 0.05)
    for p, q in zip(p64, m1.parameters()):
        p.grad = q.grad.detach().cpu().double()
    f1.step(); t2.step(); t64.step(); f3.step()
    bad = []
    for n, a, b, c, r in zip(names, m1.parameters(), m2.parameters(), m3.parameters(), p64):
        assert torch.equal(a, c), f"{n}: the checkpoint loaded back does not continue bit-identically"
        d = (a.detach().cpu().double() - r.detach()).abs().max().item()
        d32 = (b.detach().cpu().double() - r.detach()).abs().max().item()
        bound = BOUND_C * d32 + FLOOR_REL * r.detach().abs().max().item()
        if not d <= bound:
            bad.append(f"{n}: fused {d:.3e} torch f32 {d32:.3e} bound {bound:.3e}")
    assert not bad, "\n".join(bad)
    s1, s2 = f1.state_dict()["state"], t2.state_dict()["state"]
    for i in s1:
        assert float(s1[i]["step"]) == float(s2[i]["step"]) == 3.0
        assert torch.allclose(s1[i]["exp_avg"], s2[i]["exp_avg"], rtol=1e-5, atol=1e-9)


@pytest.mark.parametrize("kind", ["GAT", "GraphSAGE", "GIN"])
def test_short_training_trajectory(kind, gpu_device):
    """12 steps with max_grad_norm=1.0, dropout on, under a CosineAnnealingWarmRestarts schedule: parameters stay finite, the
    dropout-free loss ends below the start, and the update follows the learning rate read back from param_groups.

    Update size: AdamW moves an element by lr * (m^ / (sqrt(v^) + eps) + wd * p).  In step 1, m^ / sqrt(v^) = sign(g) wherever
    |g| >> eps, so the median |dp| is lr itself (the decay term is 1e-5 of |p| ~ 0.1).  Later |m^| / sqrt(v^) <= 1 up to the
    bias-correction ratio, bounded by (1 - beta1) / sqrt(1 - beta2) = 3.17; and where the schedule restarts (lr x 6.8 from step 3
    to step 4 at T_0 = 4) the median update must grow with it."""
    from bathymetric_gnn_amd.training import FusedAdamW
    m, mkw = _gpu_model(kind, num_layers=3)
    g, x, _, _ = _tiles_graph([_tile(32, 40, 8, "V1")])
    w = {k: v / x.shape[0] for k, v in _loss_weights(x.shape[0], 3, seed=9).items()}

    def plain_loss(model):
        _set_dropout(model, 0.0)
        model.train()
        with torch.no_grad():
            return float(_loss(model(g), w))

    start = plain_loss(_fresh(m, mkw))
    opt = FusedAdamW(m, lr=1e-3, max_grad_norm=1.0)
    sched = torch.optim.lr_scheduler.CosineAnnealingWarmRestarts(opt, T_0=4)
    lrs, med, norms = [], [], []
    for step in range(12):
        _set_dropout(m, 0.1)
        m.train(); m.dropout_seed = step
        opt.zero_grad(set_to_none=True)
        _loss(m(g), w).backward()
        before = torch.cat([p.detach().reshape(-1).clone() for p in m.parameters()])
        lr = opt.param_groups[0]["lr"]
        assert abs(lr - 1e-3 * (1 + math.cos(math.pi * (step % 4) / 4)) / 2) < 1e-12
        opt.step()
        sched.step()
        after = torch.cat([p.detach().reshape(-1) for p in m.parameters()])
        assert torch.isfinite(after).all()
        lrs.append(lr); med.append(float((after - before).abs().median())); norms.append(float(opt.last_grad_norm))
    end = plain_loss(m)
    print(f"{kind}: lr {lrs}\n  median |dp| {med}\n  grad norms {norms}\n  dropout-free loss {start:.5f} -> {end:.5f}")
    assert end < start
    assert abs(med[0] / lrs[0] - 1.0) < 0.02
    assert all(0.01 * l <= d <= 3.17 * l for l, d in zip(lrs, med))
    assert med[4] > 2.0 * med[3] and med[8] > 2.0 * med[7]
