"""The training step on what a VR store hands out (``compute_ground_truth_native`` -> ``TileStore.from_refinement_pairs`` ->
``batch``), held to the float64 oracle, and ``Trainer(batch_nodes=)`` on such a store against its own plan.

The other backward / loss / trainer tests feed two or three tiles of at least 24 x 31 cells at resolution (0.5, 0.5), mostly with 7
input channels.  A VR batch is a dozen grids of 2 x 2 .. 9 x 9 cells beside one large grid, every grid at its own, possibly
anisotropic, resolution (the expanded edge-attribute table has per-grid edge lengths only here), 8 input channels, an isolated
node (a grid with one valid cell), grids two cells wide (one-sided gradient features) and nodes with ``local_std == 0`` (the
mode-1 correction target on the floor and at both caps).  ``tests/_vr_truth_cpu.py: make_training_pair`` builds it.

Bars, all the project's own: graph tensors as ``test_gpu_graph`` (``_check_x`` / ``_check_ea``), parameter gradients by
``test_gpu_backward_training._accept`` (BOUND_C, FLOOR_REL), training-mode outputs within ``test_gpu_forward.TOL`` of the float32
oracle on the same dropout masks, BatchNorm's running statistics within 1e-5 of the oracle's, the loss terms within one float32 ulp
of ``_loss_cpu.loss`` (``test_gpu_loss.check_values``).  Every distance is printed before it is asserted."""
import copy

import numpy as np
import pytest
import torch

import _loss_cpu as lc
import test_gpu_backward_plain as plain
from _vr_truth_cpu import make_isolated_pair, make_training_pair, native_truth_cpu, store_batch_cpu
from conftest import ulp_diff_f32
from oracle import gat_cpu, graph_cpu
from test_gpu_backward_training import WORST, _accept, _dropout, _oracle_for, _step
from test_gpu_backward_training import _net as _gat_net, _sd as _gat_sd
from test_gpu_forward import TOL
from test_gpu_graph import _check_ea, _check_x
from test_gpu_loss import _ModelLoss, check_values
from test_gpu_trainer import _replay

pytestmark = pytest.mark.gpu

NODE_FEATURES = graph_cpu.DEFAULT_NODE_FEATURES + ["uncertainty"]
KINDS = ["GAT", "GraphSAGE", "GIN"]
OUTPUTS = ("class_logits", "confidence", "correction")
STAT_BAR = 1e-5                 # test_gpu_forward.py::test_layers_wider_than_256_columns


def _consts():
    from bathymetric_gnn_amd.config.constants import CORRECTION_NORM_CAP, CORRECTION_NORM_FLOOR
    return CORRECTION_NORM_FLOOR, CORRECTION_NORM_CAP


class _Case:
    """A pair, its restatement, its truth on the device and the store cut from it."""

    def __init__(self, clean, noisy, device):
        from bathymetric_gnn_amd.data import compute_ground_truth_native
        from bathymetric_gnn_amd.training import TileStore
        self.ref = native_truth_cpu(clean, noisy)
        self.truth = compute_ground_truth_native(clean, noisy, device=device)
        self.store = TileStore.from_refinement_pairs(self.truth, device=device)
        self.kept = self.store.grids[0]
        self._oracle = {}

    def oracle(self, indices):
        """``store_batch_cpu`` of ``indices``, computed once and left unchanged."""
        key = tuple(int(i) for i in indices)
        if key not in self._oracle:
            self._oracle[key] = store_batch_cpu(self.ref, self.kept, key, self.ref["res"][self.kept])
        return self._oracle[key]


@pytest.fixture(scope="module")
def vr(gpu_device):
    """The training pair's case, with the store tiles of its hand-set grids, and the two batches of test b."""
    clean, noisy, cases = make_training_pair(1)
    c = _Case(clean, noisy, gpu_device)
    place = {k: i for i, k in enumerate(c.ref["order"])}
    tile_of = {int(g): i for i, g in enumerate(c.kept)}
    c.tiles = {name: tile_of[place[k]] for name, k in cases.items() if place[k] in tile_of}
    assert set(cases) - set(c.tiles) == {"no_twin", "transposed"}                 # neither reached the store
    assert len(c.store) == len(c.ref["order"]) - 2 and c.store.in_channels == 8
    assert np.array_equal(c.store.node_counts, c.ref["grid_counts"][c.kept, 0]) and c.store.node_counts.dtype == np.int64
    order = np.random.default_rng(5).permutation(len(c.store))
    c.batches = {"whole store": [int(i) for i in order], "small grids": [int(i) for i in order if i != c.tiles["big"]]}
    return c


@pytest.fixture(scope="module")
def isolated(gpu_device):
    c = _Case(*make_isolated_pair(), gpu_device)
    assert len(c.store) == 2 and c.store.node_counts.tolist() == [1, 1]
    return c


@pytest.fixture(scope="module", autouse=True)
def _print_worst():
    yield
    for k, v in sorted(WORST.items()):
        if k.startswith("vr"):
            print(f"\n[{k}] worst d/f32 {v[0]:.3f}, worst d/bound {v[1]:.3f}")


def _store_statistics(store):
    """The class weights and the Huber delta ``Trainer._compute_training_stats`` takes from a ground-truth store: the scanned
    class counts, and the capped correction targets of its noise nodes (every tile, when the store holds at most 100)."""
    from bathymetric_gnn_amd.training import compute_class_weights, compute_correction_delta
    _, cap = _consts()
    assert len(store) <= 100
    counts = torch.tensor([int(store._class_counts.get(c, 0)) for c in range(3)], dtype=torch.long)
    weights = compute_class_weights(torch.arange(3).repeat_interleave(counts.clamp(min=1)), num_classes=3, smoothing=0.1)
    _, t = store.batch(range(len(store)))
    sel = t["correction_targets"][t["noise_mask"]]
    sel = sel[torch.isfinite(sel)].cpu().numpy()
    return weights, compute_correction_delta(np.clip(sel, -cap, cap), percentile=95.0, min_delta=1.0)


# ---- a. what store.batch hands out ----------------------------------------------------------------------------------------------
def test_a_batch_equals_the_oracle_batch(vr, gpu_device):
    floor, cap = _consts()
    indices = vr.batches["whole store"]
    assert indices != sorted(indices) and {vr.tiles[k] for k in ("big", "g22", "g29", "g92", "sparse", "flat")} <= set(indices)
    o = vr.oracle(indices)
    # from the input alone: an isolated node, the floor and both caps, three anisotropic resolutions
    ptr = np.concatenate([[0], np.cumsum(o["nodes"])])
    lone = [int(ptr[k]) for k in np.nonzero(o["nodes"] == 1)[0]]
    assert lone and not np.isin(lone, o["edge_index"]).any()
    assert vr.store.node_counts[vr.tiles["sparse"]] == 1
    q = o["difference"].astype(np.float64) / np.maximum(o["local_std"].astype(np.float64), floor)
    assert (o["local_std"] < floor).any() and (q > cap).any() and (q < -cap).any() and (np.abs(q) < cap).any()
    assert ((o["local_std"] == 0) & (o["difference"] != 0)).any()
    aniso = {tuple(r) for r in vr.store.res[indices].tolist() if r[0] != r[1]}
    assert len(aniso) >= 3, aniso
    assert (vr.store.hw[indices].min(axis=1) == 2).sum() >= 3                      # grids two cells wide
    assert o["x"].shape[0] <= 1200 and 100 <= vr.oracle(vr.batches["small grids"])["x"].shape[0] < 256

    g, t = vr.store.batch(indices)
    assert g.num_nodes == o["x"].shape[0] and g.num_edges == o["edge_index"].shape[1]
    assert np.array_equal(g.ptr.numpy(), ptr) and np.array_equal(g.batch.cpu().numpy(), o["batch"])
    assert np.array_equal(g.edge_index.cpu().numpy(), o["edge_index"])
    _check_x(g.x.cpu().numpy(), o["x"], NODE_FEATURES)
    _check_ea(g.edge_attr.cpu().numpy(), o["edge_attr"])
    assert np.array_equal(g.pos.cpu().numpy(), o["pos"])
    assert ulp_diff_f32(g.local_std.cpu().numpy(), o["local_std"]).max(initial=0) <= 1
    # per-grid edge lengths: the distances of the batch are not those of any single resolution
    assert len(np.unique(o["edge_attr"][:, 0])) > 6

    assert t["class_labels"].dtype == torch.int64 and t["noise_mask"].dtype == torch.bool
    assert np.array_equal(t["class_labels"].cpu().numpy(), o["labels"].astype(np.int64))
    assert np.array_equal(t["noise_mask"].cpu().numpy(), o["labels"] == 2)
    diff = torch.from_numpy(o["difference"]).to(gpu_device)
    want = torch.clamp(diff / torch.clamp(g.local_std, min=floor), min=-cap, max=cap)
    assert bool((want == cap).any()) and bool((want == -cap).any()) and bool((g.local_std < floor).any())
    assert torch.equal(t["correction_targets"].view(torch.int32), want.view(torch.int32))


# ---- b / c. one training step against float64 -------------------------------------------------------------------------------------
def _model_for(kind, seed):
    if kind == "GAT":
        sd = _gat_sd(in_channels=8, hidden=64, num_layers=3, heads=4, seed=seed)
        return sd, _gat_net(sd, in_channels=8, hidden_channels=64, num_gnn_layers=3, heads=4)
    sd = plain._sd(kind, in_channels=8, hidden=64, num_layers=3, seed=seed)
    return sd, plain._net(sd, kind, in_channels=8, hidden_channels=64, num_gnn_layers=3)


def _training_step(name, kind, case, indices, gpu_device, monkeypatch, seed=7):
    """One taped step of a 3-layer model (hidden 64, 4 heads, 8 input channels, dropout 0.1 at all four places) under
    ``BathymetricGNNLoss`` with the store's class weights, label smoothing 0.1 and the store's Huber delta, on the store's batch
    ``indices``: gradients, training-mode outputs, running statistics and loss terms against the oracle."""
    from bathymetric_gnn_amd.training import BathymetricGNNLoss
    o = case.oracle(indices)
    x, ei, ea = o["x"], o["edge_index"], o["edge_attr"]
    n = x.shape[0]
    g, t = case.store.batch(indices)
    assert g.num_nodes == n and x.shape[1] == 8
    y, target, nmask = t["class_labels"], t["correction_targets"], t["noise_mask"]
    assert int(nmask.sum()) > 0 and int((~nmask).sum()) > 0
    weights, delta = _store_statistics(case.store)
    loss = _ModelLoss(y, target, nmask, gpu_device)
    loss.class_w, loss.delta = weights.to(gpu_device), delta
    loss.crit = BathymetricGNNLoss(class_weights=loss.class_w, label_smoothing=0.1, correction_delta=delta)

    sd, m = _model_for(kind, 151)
    drop = _dropout(m, seed, 0.1, 0.1) if kind == "GAT" else plain._drop(m, seed, 0.1, 0.1)
    g_gpu, out = _step(m, g, loss, seed)
    assert all(p.grad is not None and bool(torch.isfinite(p.grad).all()) for p in m.parameters())
    group = f"vr {name}, {kind}"
    # the forward: float32 oracle on the same masks, and the running statistics it leaves
    stats = {}
    ref = gat_cpu.forward(sd, x, ei, ea, train_stats=stats, dropout=drop)
    dist = {k: (out[k].detach().cpu() - ref[k]).abs().max().item() for k in OUTPUTS}
    sdist = {}
    for l, norm in enumerate(m.gnn.norms):
        pre = f"gnn.norms.{l}.module."
        sdist[l] = ((norm.module.running_mean.cpu() - stats[pre + "running_mean"]).abs().max().item(),
                    (norm.module.running_var.cpu() - stats[pre + "running_var"]).abs().max().item())
    print(f"[{group}] {n} nodes, {ei.shape[1]} edges; forward distance to the float32 oracle "
          f"{ {k: float(f'{v:.3e}') for k, v in dist.items()} } (largest {max(dist.values()):.3e}, bar {TOL}); "
          f"running mean / var distance per layer { {l: (float(f'{a:.2e}'), float(f'{b:.2e}')) for l, (a, b) in sdist.items()} }")
    # the loss terms on the GPU's own outputs
    targets = {"class_labels": y, "correction_targets": target, "noise_mask": nmask}
    with torch.no_grad():
        terms = loss.crit({k: v.detach() for k, v in out.items()}, targets)
    inp = {k: out[k].detach().cpu().numpy() for k in OUTPUTS + ("predicted_class",)}
    inp.update({k: v.cpu().numpy() for k, v in targets.items()})
    cfg = lc.config(class_weights=weights.numpy(), label_smoothing=0.1, delta=delta)
    # the gradients
    if kind == "GAT":
        g64, g32 = _oracle_for(m, out, n, sd, x, ei, ea, drop, loss, monkeypatch)
    else:
        g64, g32 = plain._oracle(m, out, n, sd, x, ei, ea, drop, loss, monkeypatch)
    _accept(group, "BathymetricGNNLoss on the store's batch", g_gpu, g64, g32)
    # (_accept's d/f32 counts the parameters whose bound the float32 yardstick dominates; the plain ratio is over all of them)
    raw = max((g_gpu[k].reshape(g64[k].shape) - g64[k]).abs().max().item() / max((g32[k] - g64[k]).abs().max().item(), 1e-300)
              for k in g64)
    print(f"[{group}] worst d/bound {WORST[group][1]:.3f}, worst d/f32 {WORST[group][0]:.3f} where the yardstick dominates the "
          f"bound and {raw:.3f} over every parameter, largest forward distance {max(dist.values()):.3e}")
    for k, v in dist.items():
        assert v < TOL, (k, v)
    for l, (a, b) in sdist.items():
        assert a < STAT_BAR and b < STAT_BAR, (l, a, b)
    check_values(group, {k: float(v) for k, v in terms.items()}, lc.loss(inp, cfg))
    return g_gpu, out


@pytest.mark.parametrize("batch", ["whole store", "small grids"])
@pytest.mark.parametrize("kind", KINDS)
def test_b_training_step_against_float64(kind, batch, vr, gpu_device, monkeypatch):
    indices = vr.batches[batch]
    n = int(vr.store.node_counts[indices].sum())
    assert (vr.tiles["big"] in indices) == (batch == "whole store") and vr.tiles["sparse"] in indices
    if batch == "small grids":
        # one to two hundred rows under BatchNorm's batch statistics, the tape's row capacity (the cells) above them
        assert 100 <= n < 256 and int(np.diff(vr.store.offsets)[indices].sum()) > n
    _training_step(batch, kind, vr, indices, gpu_device, monkeypatch)


@pytest.mark.parametrize("kind", KINDS)
def test_c_two_isolated_nodes(kind, isolated, gpu_device, monkeypatch):
    """The smallest batch ``train()`` takes: two rows, no edge but the self loops the layers add."""
    o = isolated.oracle([1, 0])
    assert o["x"].shape[0] == 2 and o["edge_index"].shape[1] == 0 and o["nodes"].tolist() == [1, 1]
    res = isolated.store.res[[1, 0]]
    assert (res[:, 0] != res[:, 1]).all() and not np.array_equal(res[0], res[1])
    assert sorted(o["labels"].tolist()) == [0, 2]
    _training_step("two isolated nodes", kind, isolated, [1, 0], gpu_device, monkeypatch)


# ---- d. determinism --------------------------------------------------------------------------------------------------------------
def test_d_two_steps_give_equal_bits(vr, gpu_device):
    from bathymetric_gnn_amd.training import BathymetricGNNLoss
    indices = vr.batches["whole store"]
    weights, delta = _store_statistics(vr.store)
    crit = BathymetricGNNLoss(class_weights=weights.to(gpu_device), label_smoothing=0.1, correction_delta=delta)
    runs = []
    for _ in range(2):
        g, t = vr.store.batch(indices)
        sd, m = _model_for("GAT", 151)
        _dropout(m, 7, 0.1, 0.1)
        grads, out = _step(m, g, lambda o: crit(o, t)["total"], 7)
        runs.append((grads, {k: v.detach().cpu() for k, v in out.items()}, {k: v.detach().cpu() for k, v in m.state_dict().items()}))
    for part in range(3):
        a, b = runs[0][part], runs[1][part]
        assert list(a) == list(b)
        for k in a:
            assert torch.equal(a[k], b[k]), k


# ---- e. Trainer on the VR store equals its plan -----------------------------------------------------------------------------------
class _Cells:
    """A store as ``step_plan`` saw it before it knew node counts: its length and its cell offsets."""

    def __init__(self, offsets):
        self.offsets = offsets

    def __len__(self):
        return len(self.offsets) - 1


def _isolating_seed(store, one, batch_nodes):
    """The first seed below 64 whose epoch-0 cut by cell count alone leaves tile ``one`` in a piece of its own.  Host only."""
    from types import SimpleNamespace
    from bathymetric_gnn_amd.training import Trainer
    for s in range(64):
        t = Trainer.__new__(Trainer)
        t.seed, t.settings, t.batch_nodes = s, SimpleNamespace(batch_size=2), batch_nodes
        t.train_store = t.val_store = _Cells(store.offsets)
        if [one] in [p.tolist() for p, _ in t.step_plan(0)]:
            return s
    return None


def _trainer_model(kind, seed=1):
    from bathymetric_gnn_amd import synthetic
    from bathymetric_gnn_amd.models import BathymetricGNN
    sd = synthetic.synthetic_state_dict(in_channels=8, num_layers=2, seed=seed, gnn_type=kind)
    m = BathymetricGNN(in_channels=8, hidden_channels=64, num_gnn_layers=2, gnn_type=kind, heads=4, dropout=0.1, edge_dim=3)
    m.load_state_dict({k: torch.as_tensor(v) for k, v in sd.items()})
    return m.cuda()


@pytest.fixture(scope="module")
def val_store(gpu_device):
    return _Case(*make_training_pair(0)[:2], gpu_device).store


@pytest.mark.parametrize("kind", ["GAT", "GraphSAGE"])
def test_e_trainer_equals_its_plan(kind, vr, val_store, tmp_path, gpu_device):
    from bathymetric_gnn_amd.config import Config
    from bathymetric_gnn_amd.training import Trainer
    one = vr.tiles["sparse"]
    s = _isolating_seed(vr.store, one, 300)
    assert s is not None, "no seed below 64 isolates the one-node tile under the cut by cells alone"
    cfg = Config()
    cfg.training = {"batch_size": 2, "epochs": 1, "scheduler": "cosine"}
    t = Trainer(cfg, _trainer_model(kind), vr.store, val_store, output_dir=tmp_path / "a", seed=s, batch_nodes=300)
    plan = [p.tolist() for p, _ in t.step_plan(0)]
    cells, nodes = np.diff(vr.store.offsets), vr.store.node_counts
    print(f"{kind}: seed {s}, plan {plan}, nodes per step {[int(nodes[p].sum()) for p in plan]}")
    assert [one] not in plan and all(nodes[p].sum() >= 2 for p in plan) and len(plan) >= 2
    assert sorted(i for p in plan for i in p) == list(range(len(vr.store)))
    with_big = next(p for p in plan if vr.tiles["big"] in p)                      # 744 cells: alone, unless the lone tile joined it
    assert cells[vr.tiles["big"]] > 300 and set(with_big) <= {vr.tiles["big"], one}
    weights, delta = _store_statistics(vr.store)
    assert torch.equal(t.criterion.classification_loss.class_weights.cpu(), weights) and t.criterion.correction_loss.delta == delta
    history = copy.deepcopy(t.train())
    other = Trainer(cfg, _trainer_model(kind), vr.store, val_store, output_dir=tmp_path / "b", seed=s, batch_nodes=300)
    replayed = _replay(other, 1)
    print(f"{kind}: history {history}")
    assert history == replayed
    assert all(len(v) == 1 and all(np.isfinite(v)) for v in history.values())
    a, b = t.model.state_dict(), other.model.state_dict()
    assert list(a) == list(b)
    for k in a:
        assert torch.equal(a[k], b[k]), k
