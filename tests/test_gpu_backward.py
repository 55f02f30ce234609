"""Backward pass of BathymetricGNN (GAT) on the GPU: ``loss.backward()`` after a training-mode forward fills every parameter's
``.grad`` from the HIP kernels (``bgnn_forward_train_tape`` + ``bgnn_backward``).

Reference gradients: the oracle's forward (``oracle.gat_cpu.backbone`` + the three heads through ``_mlp2``, head masks as
``gat_cpu.forward`` draws them) under torch autograd, in float64 (the truth) and float32 (what float32 arithmetic achieves), with
``gat_cpu._t`` replaced by a copy that does not detach, so that gradients reach the state-dict tensors, and with the very dropout
masks of the kernels (``CounterDropout``, same seed).  The acceptance rule is ``tests/_conditioning.py``'s: per parameter,
max |g_gpu - g64| <= BOUND_C * max |g32 - g64| + floor, the floor relative to the largest gradient of the model (the GAT bias
gradient is a sum that cancels to ~0 under batch-statistics BatchNorm and is judged on that absolute scale)."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from _conditioning import BOUND_C
from oracle import gat_cpu, graph_cpu

pytestmark = pytest.mark.gpu

FLOOR_REL = 1e-5           # floor of the bound, x the largest |gradient| of the model (float64)


def _t_keep_graph(v, dtype):
    if isinstance(v, torch.Tensor):
        return v.to("cpu", dtype)
    return torch.as_tensor(np.asarray(v)).to(dtype)


def _is_param(k):
    return not k.endswith(("running_mean", "running_var", "num_batches_tracked"))


def _loss_weights(N, nc, seed=7):
    r = np.random.default_rng(seed)
    return {"class_logits": r.standard_normal((N, nc)), "class_probs": r.standard_normal((N, nc)),
            "confidence": r.standard_normal(N), "correction": r.standard_normal(N)}


def _loss(out, w):
    """The fixed linear form of ``_loss_weights``, or ``w(out)`` when ``w`` is a loss callable."""
    if callable(w):
        return w(out)
    s = 0.0
    for k, v in w.items():
        if k in out:
            s = s + (out[k] * torch.as_tensor(v, dtype=out[k].dtype, device=out[k].device)).sum()
    return s


def oracle_grads(sd, x, ei, ea, dtype, drop, w, monkeypatch, outputs=None, functional=None):
    """{name: gradient} of the loss ``w`` (``_loss``) through the oracle's training-mode forward, and the loss value.  A parameter
    the loss does not reach is absent.  ``outputs``: a dict that receives the forward's outputs (detached) and predicted_class.
    ``functional``: stands in for ``torch.nn.functional`` inside the oracle (e.g. to give its ReLUs the kernels' patterns)."""
    monkeypatch.setattr(gat_cpu, "_t", _t_keep_graph)
    if functional is not None:
        monkeypatch.setattr(gat_cpu, "F", functional)
    P = {k: torch.tensor(np.asarray(v), dtype=dtype, requires_grad=_is_param(k)) for k, v in sd.items()
         if np.asarray(v).dtype.kind == "f"}
    x = torch.as_tensor(x).to(dtype); ea = torch.as_tensor(ea).to(dtype); ei = torch.as_tensor(ei).to(torch.int64)
    h = gat_cpu.backbone(x, ei, ea, P, dtype, train_stats={}, dropout=drop)
    hm = [None, None, None]
    if drop is not None and drop.p_heads > 0:          # (restates gat_cpu.forward: the heads' units side by side)
        hh = P["classification_head.mlp.0.weight"].shape[0]
        nh = 3 if "correction_head.mlp.0.weight" in P else 2
        m_all = drop.elementwise(torch.ones(h.shape[0], nh * hh, dtype=dtype), drop.p_heads, 2)
        hm = [m_all[:, i * hh:(i + 1) * hh] if i < nh else None for i in range(3)]
    logits = gat_cpu._mlp2(h, P, "classification_head.mlp.0", "classification_head.mlp.3", dtype, hm[0])
    out = {"class_logits": logits, "class_probs": F.softmax(logits, dim=-1),
           "confidence": torch.sigmoid(gat_cpu._mlp2(h, P, "confidence_head.mlp.0", "confidence_head.mlp.3", dtype, hm[1])).squeeze(-1)}
    if "correction_head.mlp.0.weight" in P:
        out["correction"] = gat_cpu._mlp2(h, P, "correction_head.mlp.0", "correction_head.mlp.3", dtype, hm[2]).squeeze(-1)
    if outputs is not None:
        outputs.update({k: v.detach() for k, v in out.items()}, predicted_class=out["class_probs"].detach().argmax(-1))
    loss = _loss(out, w)
    loss.backward()
    monkeypatch.undo()
    return {k: v.grad.detach().double() for k, v in P.items() if v.requires_grad and v.grad is not None}, float(loss.detach())


def _set_dropout(m, p):
    from bathymetric_gnn_amd.models.gnn import GATConv
    m.feature_extractor.mlp[2].p = p
    for c in m.gnn.convs:
        if isinstance(c, GATConv):
            c.dropout = p
    m.gnn.dropout = p
    for h in (m.classification_head, m.confidence_head, m.correction_head):
        if h is not None:
            h.mlp[2].p = p


def _model(sd, device, **kw):
    from bathymetric_gnn_amd.models import BathymetricGNN
    m = BathymetricGNN(**kw)
    m.load_state_dict({k: torch.as_tensor(v) for k, v in sd.items()}, strict=True)
    return m.to(device)


def _tiles_graph(tiles, conn="8-connected", edge_features=None):
    from bathymetric_gnn_amd.data import GraphBuilder
    gb = GraphBuilder(connectivity=conn, edge_features=edge_features)
    g = gb.build_graphs([t[0] for t in tiles], [t[1] for t in tiles], None, [(0.5, 0.5)] * len(tiles))
    ogs = [graph_cpu.build_graph(t[0], t[1], None, (0.5, 0.5), connectivity=conn, edge_feature_names=edge_features) for t in tiles]
    x, ei, ea, _, _ = graph_cpu.batch_graphs(ogs)
    return g, x, ei, ea


def _gpu_grads(m, data, w, seed):
    m.train()
    m.dropout_seed = seed
    m.zero_grad(set_to_none=True)
    out = m(data)
    _loss(out, w).backward()
    return {n: p.grad.detach().double().cpu() for n, p in m.named_parameters() if p.grad is not None}, out


def _check_parity(m, sd, data, x, ei, ea, p, seed, monkeypatch):
    nc = sd["classification_head.mlp.3.weight"].shape[0]
    w = _loss_weights(x.shape[0], nc)
    if not m.predict_correction:
        w.pop("correction")
    _set_dropout(m, p)
    g_gpu, _ = _gpu_grads(m, data, w, seed)
    drop = gat_cpu.CounterDropout(seed, p, p, p, p) if p > 0 else None
    g64, _ = oracle_grads(sd, x, ei, ea, torch.float64, drop, w, monkeypatch)
    g32, _ = oracle_grads(sd, x, ei, ea, torch.float32, drop, w, monkeypatch)
    assert set(g_gpu) == set(g64), set(g_gpu) ^ set(g64)
    gmax = max(v.abs().max().item() for v in g64.values())
    bad = []
    for k in g64:
        d_gpu = (g_gpu[k].reshape(g64[k].shape) - g64[k]).abs().max().item()
        d32 = (g32[k] - g64[k]).abs().max().item()
        if not d_gpu <= BOUND_C * d32 + FLOOR_REL * gmax:
            bad.append(f"{k}: gpu {d_gpu:.3e} vs f32 {d32:.3e} (floor {FLOOR_REL * gmax:.3e})")
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("p", [0.0, 0.1])
def test_gradient_parity_default_shape(p, gpu_device, monkeypatch):
    """4 layers, hidden 64, heads 4, edge_dim 3, two V1-masked tiles; dropout off and on (p = 0.1 at all four places)."""
    from bathymetric_gnn_amd import synthetic
    sd = synthetic.synthetic_state_dict(in_channels=7, num_layers=4, seed=41)
    m = _model(sd, gpu_device, in_channels=7, num_gnn_layers=4, edge_dim=3)
    tiles = [synthetic.synthetic_tile(37, 45, 3, "V1"), synthetic.synthetic_tile(30, 40, 4, "V1")]
    g, x, ei, ea = _tiles_graph(tiles)
    _check_parity(m, sd, g, x, ei, ea, p, 123, monkeypatch)


SWEEP = [  # (heads, hidden, layers, connectivity, edge_features, edge_dim)
    (1, 64, 3, "8-connected", None, 3),
    (2, 32, 1, "4-connected", ["slope"], 1),
    (2, 128, 3, "16-dilated", None, 3),
    (8, 32, 2, "8-connected", ["distance", "depth_difference", "slope", "depth_difference"], 4),
    (4, 64, 2, "8-connected", None, None),
]


@pytest.mark.parametrize("heads,hidden,layers,conn,efeat,edge_dim", SWEEP)
def test_gradient_parity_shapes_and_graphs(heads, hidden, layers, conn, efeat, edge_dim, gpu_device, monkeypatch):
    from bathymetric_gnn_amd import synthetic
    ed_sd = edge_dim if edge_dim is not None else 3
    sd = synthetic.synthetic_state_dict(in_channels=7, hidden=hidden, num_layers=layers, heads=heads, edge_dim=ed_sd, seed=43)
    if edge_dim is None:
        sd = {k: v for k, v in sd.items() if "att_edge" not in k and "lin_edge" not in k}
    m = _model(sd, gpu_device, in_channels=7, hidden_channels=hidden, num_gnn_layers=layers, heads=heads, edge_dim=edge_dim)
    tiles = [synthetic.synthetic_tile(29, 35, 5, "V1"), synthetic.synthetic_tile(24, 31, 6, "V0")]
    g, x, ei, ea = _tiles_graph(tiles, conn, efeat)
    _check_parity(m, sd, g, x, ei, ea, 0.1, 99, monkeypatch)


def _foreign_graph():
    rng = np.random.default_rng(3)
    N, E = 300, 1500
    pairs = rng.permutation((N - 10) * (N - 10))[:E]
    ei = np.stack([pairs // (N - 10), pairs % (N - 10)]).astype(np.int64)
    ei[1, :40] = 5; ei[0, :40] = np.arange(100, 140)                # hub: 40 in-edges (rows longer than 16)
    ei[:, 100:110] = np.arange(20, 30)[None, :]                     # explicit self loops
    ei = np.concatenate([ei, ei[:, 200:230]], axis=1)               # parallel edges
    x = rng.standard_normal((N, 7)).astype(np.float32)
    ea = rng.standard_normal((ei.shape[1], 3)).astype(np.float32)
    return x, ei, ea


def test_gradient_parity_foreign_graph(gpu_device, monkeypatch):
    """A Data built elsewhere: parallel edges, explicit self loops, a hub and isolated nodes (the transposed CSR index)."""
    from bathymetric_gnn_amd import synthetic
    from bathymetric_gnn_amd.data import Data
    sd = synthetic.synthetic_state_dict(in_channels=7, num_layers=3, seed=45)
    m = _model(sd, gpu_device, in_channels=7, num_gnn_layers=3, edge_dim=3)
    x, ei, ea = _foreign_graph()
    data = Data(x=torch.from_numpy(x).cuda(), edge_index=torch.from_numpy(ei).cuda(), edge_attr=torch.from_numpy(ea).cuda())
    _check_parity(m, sd, data, x, ei, ea, 0.1, 5, monkeypatch)


def test_backward_is_deterministic(gpu_device):
    """Two backward passes on the same tape give bit-identical gradients."""
    from bathymetric_gnn_amd import synthetic
    sd = synthetic.synthetic_state_dict(in_channels=7, num_layers=4, seed=47)
    m = _model(sd, gpu_device, in_channels=7, num_gnn_layers=4, edge_dim=3)
    _set_dropout(m, 0.1)
    g, x, _, _ = _tiles_graph([synthetic.synthetic_tile(64, 64, 7, "V1")])
    m.train(); m.dropout_seed = 3
    out = m(g)
    w = _loss_weights(x.shape[0], 3)
    loss = _loss(out, w)
    loss.backward(retain_graph=True)
    first = {n: p.grad.clone() for n, p in m.named_parameters()}
    m.zero_grad(set_to_none=True)
    loss.backward()
    for n, p in m.named_parameters():
        assert torch.equal(first[n], p.grad), n


def test_taped_forward_changes_nothing(gpu_device):
    """The taped forward's outputs and running statistics are bit-identical to the same forward under no_grad; an eval-mode
    forward returns tensors without grad_fn."""
    from bathymetric_gnn_amd import synthetic
    sd = synthetic.synthetic_state_dict(in_channels=7, num_layers=4, seed=49)
    tiles = [synthetic.synthetic_tile(37, 45, 3, "V1"), synthetic.synthetic_tile(20, 64, 4, "V0")]
    g, _, _, _ = _tiles_graph(tiles)
    res = []
    for taped in (False, True):
        m = _model(sd, gpu_device, in_channels=7, num_gnn_layers=4, edge_dim=3)
        _set_dropout(m, 0.1)
        m.train(); m.dropout_seed = 11
        with torch.set_grad_enabled(taped):
            out = m(g)
        assert (out["class_logits"].grad_fn is not None) == taped
        res.append(({k: v.detach().clone() for k, v in out.items()},
                    [(n.module.running_mean.clone(), n.module.running_var.clone()) for n in m.gnn.norms]))
    for k in res[0][0]:
        assert torch.equal(res[0][0][k], res[1][0][k]), k
    for a, b in zip(res[0][1], res[1][1]):
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    m.eval()
    out = m(g)
    assert all(v.grad_fn is None for v in out.values())


def test_short_training_trajectory(gpu_device, monkeypatch):
    """20 plain-SGD steps on one batch with dropout on (seed = step) against the float64 oracle stepped identically: the loss
    decreases, and every parameter stays as close to the float64 trajectory as the float32 oracle's own trajectory does (BOUND_C x
    its distance, plus 1e-5 of the parameter's size).  The bound is relative to float32 because the first extractor layer sees the
    raw depth (about -20 m here): batch-statistics BatchNorm removes the column means of the gradient, so that layer's weight
    gradient is a heavily cancelling sum, float32 arithmetic itself drifts ~1e-3 from float64 on it over 20 steps, and a fixed
    relative bar would measure that, not the kernels.  Then one AdamW step with clip_grad_norm_ runs."""
    from bathymetric_gnn_amd import synthetic
    sd = synthetic.synthetic_state_dict(in_channels=7, num_layers=3, seed=51)
    m = _model(sd, gpu_device, in_channels=7, num_gnn_layers=3, edge_dim=3)
    _set_dropout(m, 0.1)
    g, x, ei, ea = _tiles_graph([synthetic.synthetic_tile(32, 40, 8, "V1")])
    w = _loss_weights(x.shape[0], 3, seed=9)
    for k in w:
        w[k] = w[k] / x.shape[0]
    lr = 0.05
    opt = torch.optim.SGD(m.parameters(), lr=lr)
    ref = {k: np.asarray(v, dtype=np.float64).copy() for k, v in sd.items()}
    ref32 = {k: np.asarray(v).copy() for k, v in sd.items()}
    losses, ref_losses = [], []
    for step in range(20):
        m.train(); m.dropout_seed = step
        opt.zero_grad(set_to_none=True)
        loss = _loss(m(g), w)
        loss.backward()
        opt.step()
        losses.append(float(loss.detach()))
        g64, l64 = oracle_grads(ref, x, ei, ea, torch.float64, gat_cpu.CounterDropout(step, 0.1, 0.1, 0.1, 0.1), w, monkeypatch)
        ref_losses.append(l64)
        for k, gr in g64.items():
            ref[k] = ref[k] - lr * gr.numpy().reshape(ref[k].shape)
        g32, _ = oracle_grads(ref32, x, ei, ea, torch.float32, gat_cpu.CounterDropout(step, 0.1, 0.1, 0.1, 0.1), w, monkeypatch)
        for k, gr in g32.items():
            ref32[k] = (ref32[k] - np.float32(lr) * gr.numpy().astype(np.float32).reshape(ref32[k].shape)).astype(np.float32)
        # (the running statistics do not enter a training-mode forward; they are not compared here)
    assert losses[-1] < losses[0] and ref_losses[-1] < ref_losses[0]
    assert abs(losses[0] - ref_losses[0]) <= 1e-4 * (1 + abs(ref_losses[0]))
    for n, p in m.named_parameters():
        r = torch.as_tensor(ref[n]).reshape(p.shape)
        err = (p.detach().double().cpu() - r).abs().max().item()
        err32 = (torch.as_tensor(ref32[n]).double().reshape(p.shape) - r).abs().max().item()
        assert err <= BOUND_C * err32 + 1e-5 * r.abs().max().item(), (n, err, err32)
    opt2 = torch.optim.AdamW(m.parameters(), lr=1e-3)
    opt2.zero_grad()
    _loss(m(g), w).backward()
    torch.nn.utils.clip_grad_norm_(m.parameters(), 1.0)
    opt2.step()
    assert all(torch.isfinite(p).all() for p in m.parameters())


@pytest.mark.parametrize("what", ["GCN", "wide"])
def test_refusals(what, gpu_device):
    """No backward for GCN or for a 512-column layer: backward() raises NotImplementedError naming the limit, the forward values
    are those of the untaped forward."""
    from bathymetric_gnn_amd import synthetic
    if what == "GCN":
        kw = dict(in_channels=7, num_gnn_layers=2, gnn_type="GCN", edge_dim=3)
        sd = synthetic.synthetic_state_dict(in_channels=7, num_layers=2, gnn_type="GCN", seed=53)
        msg = "GAT"
    else:
        kw = dict(in_channels=7, num_gnn_layers=2, heads=8, edge_dim=3)
        sd = synthetic.synthetic_state_dict(in_channels=7, num_layers=2, heads=8, seed=53)
        msg = "256 columns"
    g, x, _, _ = _tiles_graph([synthetic.synthetic_tile(30, 30, 9, "V1")])
    m = _model(sd, gpu_device, **kw)
    m.train(); m.dropout_seed = 1
    with torch.no_grad():
        plain = m(g)["class_logits"].clone()
    m = _model(sd, gpu_device, **kw)
    m.train(); m.dropout_seed = 1
    out = m(g)
    assert torch.equal(out["class_logits"].detach(), plain)
    with pytest.raises(NotImplementedError, match=msg):
        _loss(out, _loss_weights(x.shape[0], 3)).backward()
