"""Training at 9 input channels (uncertainty and sounding density behind the computed features) on graphs built with the density
plane: the taped training forward, with batch statistics and dropout on, and ``backward()`` against the float64 restatement
that tests/test_gpu_backward_training.py (GAT) and tests/test_gpu_backward_plain.py (GraphSAGE) compare with -- their helpers,
their acceptance rule, unchanged; then one FusedAdamW step and the refresh of the packed model."""
import numpy as np
import pytest
import torch

from oracle import graph_cpu
from test_gpu_backward import _loss, _loss_weights, _model
from test_gpu_backward_plain import _parity as _parity_plain
from test_gpu_backward_training import _parity as _parity_gat

pytestmark = pytest.mark.gpu
RES = (0.5, 0.5)
W0 = "feature_extractor.mlp.0.weight"


def _tile(h, w, seed):
    rng = np.random.default_rng(seed)
    depth = (-25.0 + rng.standard_normal((h, w)).cumsum(0).cumsum(1) * 0.02).astype(np.float32)
    mask = rng.random((h, w)) < 0.85
    unc = (0.05 + 0.1 * rng.random((h, w))).astype(np.float32)
    den = (np.float32(1) / rng.integers(1, 9, (h, w)).astype(np.float32)).astype(np.float32)
    return depth, mask, unc, den


@pytest.fixture(scope="module")
def batch():
    """Two unequal tiles with holes: (tiles, oracle x [N, 9], edge_index, edge_attr), made once."""
    tiles = [_tile(37, 45, 3), _tile(30, 40, 4)]
    x, ei, ea, _, _ = graph_cpu.batch_graphs([graph_cpu.build_graph(d, m, u, RES) for d, m, u, _ in tiles])
    den = np.concatenate([a[m] for _, m, _, a in tiles])
    return tiles, np.concatenate([x, den[:, None]], axis=1).astype(np.float32), ei, ea


def _graph(tiles):
    from bathymetric_gnn_amd.data import GraphBuilder
    return GraphBuilder().build_graphs([t[0] for t in tiles], [t[1] for t in tiles], [t[2] for t in tiles], [RES] * len(tiles),
                                       densities=[t[3] for t in tiles])


def _sd(kind, seed):
    from bathymetric_gnn_amd import synthetic
    return synthetic.synthetic_state_dict(in_channels=9, num_layers=3, seed=seed, gnn_type=kind)


def _net(sd, kind):
    return _model(sd, torch.device("cuda:0"), in_channels=9, num_gnn_layers=3, gnn_type=kind, edge_dim=3)


def _ninth_column(m):
    """The gradient of the ninth weight column is not zero: every hidden unit either has a non-zero entry there or is dead in this
    batch (its ReLU never fires: the whole row of the gradient is exactly 0)."""
    g = m.feature_extractor.mlp[0].weight.grad
    assert g is not None and g.shape == (64, 9)
    alive = (g != 0).any(dim=1)
    assert alive.sum().item() >= 8 and bool((g[alive, 8] != 0).all())


@pytest.mark.parametrize("p", [0.0, 0.1])
def test_gat_training_step_against_float64(p, batch, gpu_device, monkeypatch):
    tiles, x, ei, ea = batch
    sd = _sd("GAT", 201)
    m = _net(sd, "GAT")
    g = _graph(tiles)
    assert g.num_features == 9 and g.num_nodes == x.shape[0]
    # (_parity: taped forward with batch statistics and every dropout at p, backward, float64 / float32 oracles with the kernels'
    #  ReLU patterns, the acceptance rule over EVERY parameter -- feature_extractor.mlp.0.weight with its ninth column among them)
    _parity_gat("density", f"GAT 9 channels p{p}", m, sd, g, x, ei, ea, monkeypatch, p=p, seed=23)
    _ninth_column(m)


@pytest.mark.parametrize("p", [0.0, 0.1])
def test_sage_training_step_against_float64(p, batch, gpu_device, monkeypatch):
    tiles, x, ei, ea = batch
    sd = _sd("GraphSAGE", 202)
    m = _net(sd, "GraphSAGE")
    _parity_plain("density", f"GraphSAGE 9 channels p{p}", m, sd, _graph(tiles), x, ei, ea, monkeypatch, p, seed=29)
    _ninth_column(m)


@pytest.mark.parametrize("kind", ["GAT", "GraphSAGE"])
def test_training_step_at_16_channels(kind, batch, gpu_device, monkeypatch):
    """The far end of the range: 8 auxiliary planes behind 7 features + uncertainty, in_channels 16 -- every column of the wide
    table and every row of the 16-row extractor weight, forward and backward, under the same rule (dropout on)."""
    from bathymetric_gnn_amd import synthetic
    from bathymetric_gnn_amd.data import GraphBuilder
    tiles, x, ei, ea = batch
    gb = GraphBuilder()
    hw, res, d, m, u = gb.upload_tiles([t[0] for t in tiles], [t[1] for t in tiles], [t[2] for t in tiles], [RES] * len(tiles))
    rng = np.random.default_rng(6)
    planes = [torch.from_numpy(rng.uniform(0.0, 1.0, d.numel()).astype(np.float32)).to(gpu_device) for _ in range(8)]
    g = gb.build_from_device(hw, res, d, m, u, aux_t=planes)
    x16 = np.concatenate([x[:, :8], torch.stack([p[m.bool()] for p in planes], dim=1).cpu().numpy()], axis=1).astype(np.float32)
    assert g.num_features == 16 and x16.shape == (g.num_nodes, 16)
    sd = synthetic.synthetic_state_dict(in_channels=16, num_layers=3, seed=205, gnn_type=kind)
    net = _model(sd, torch.device("cuda:0"), in_channels=16, num_gnn_layers=3, gnn_type=kind, edge_dim=3)
    if kind == "GAT":
        _parity_gat("density", "GAT 16 channels p0.1", net, sd, g, x16, ei, ea, monkeypatch, p=0.1, seed=31)
    else:
        _parity_plain("density", "GraphSAGE 16 channels p0.1", net, sd, g, x16, ei, ea, monkeypatch, 0.1, seed=31)
    grad = net.feature_extractor.mlp[0].weight.grad
    alive = (grad != 0).any(dim=1)
    assert grad.shape == (64, 16) and alive.sum().item() >= 8 and bool((grad[alive][:, 8:] != 0).all())


@pytest.mark.parametrize("kind", ["GAT", "GraphSAGE"])
def test_one_optimizer_step_moves_the_column_and_the_refresh_follows(kind, batch, gpu_device):
    from bathymetric_gnn_amd import runtime as rt
    from bathymetric_gnn_amd.models import BathymetricGNN
    from bathymetric_gnn_amd.training import FusedAdamW
    tiles, x, _, _ = batch
    m = _net(_sd(kind, 204), kind)
    g = _graph(tiles)
    before = m.feature_extractor.mlp[0].weight.detach().clone()
    lw = {k: v / x.shape[0] for k, v in _loss_weights(x.shape[0], 3, seed=9).items()}
    opt = FusedAdamW(m, lr=1e-3, max_grad_norm=1.0)
    m.train(); m.dropout_seed = 0
    opt.zero_grad()
    _loss(m(g), lw).backward()
    opt.step()
    after = m.feature_extractor.mlp[0].weight.detach()
    assert bool((after[:, 8] != before[:, 8]).any()) and bool(torch.isfinite(after).all())
    fresh = BathymetricGNN(in_channels=9, num_gnn_layers=3, gnn_type=kind, edge_dim=3)
    fresh.load_state_dict({k: v.detach().cpu().clone() for k, v in m.state_dict().items()})
    fresh = fresh.to(gpu_device)
    for name, run in (("training forward", lambda mod: _train_forward(mod, g)), ("predict", lambda mod: mod.eval().predict(g))):
        if name == "predict":
            m._refresh_native(rt.REFRESH_ALL)                     # (the eval images lag behind the blob again: model_sync repacks)
        a, b = run(m), run(fresh)
        for k in ("class_logits", "confidence", "correction"):
            assert torch.equal(a[k], b[k]), f"{name}: {k}"


def _train_forward(m, g, seed=100):
    m.train(); m.dropout_seed = seed
    with torch.no_grad():
        return {k: v.clone() for k, v in m(g).items()}
