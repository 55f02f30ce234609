"""Backward pass of the GraphSAGE and GIN backbones on the GPU (``bgnn_backward``, plain_backward.hip): ``loss.backward()``
after a training-mode forward fills every parameter's ``.grad``, as it does for GAT (``tests/test_gpu_backward.py``).

Reference gradients: the oracle's training-mode forward (``oracle.gat_cpu.sage_conv`` / ``gin_conv``) under torch autograd in
float64 and float32, with the kernels' dropout masks (``CounterDropout``, same seed) and the kernels' ReLU patterns (read from
the tape, laid out as train_api.hip ``TapeLayout`` documents; ``test_gpu_backward_training`` explains why).  Acceptance rule
as there: per parameter, max |g_gpu - g64| <= BOUND_C * max |g32 - g64| + FLOOR_REL * max |g64|, and a parameter the loss does
not reach gets exactly 0.

The backward of both aggregates sums over a node's OUT-edges (the transposed index); the foreign-graph tests use asymmetric
edge lists, where the forward's in-edge gather would give other sums."""
import numpy as np
import pytest
import torch

from _conditioning import BOUND_C
from oracle import gat_cpu, graph_cpu
from test_gpu_backward import _foreign_graph, _loss, _loss_weights, _model, _set_dropout, _tiles_graph, oracle_grads
from test_gpu_backward_training import _KernelReLU, _accept, _batch, _copies_identical, _masked, _sparse_tiles, _step, _tile, _tiled

pytestmark = pytest.mark.gpu
KINDS = ["GraphSAGE", "GIN"]
EPS32 = float(np.finfo(np.float32).eps)


def _sd(kind, **kw):
    from bathymetric_gnn_amd import synthetic
    kw.setdefault("in_channels", 7)
    return synthetic.synthetic_state_dict(gnn_type=kind, **kw)


def _net(sd, kind, **kw):
    kw.setdefault("in_channels", 7)
    kw.setdefault("edge_dim", 3)
    return _model(sd, torch.device("cuda:0"), gnn_type=kind, **kw)


def _drop(m, seed, p_ext, p):
    """Dropout p at the feature / head places and p_ext in the extractor; the oracle's CounterDropout with the same seed, or None."""
    _set_dropout(m, p)
    m.feature_extractor.mlp[2].p = p_ext
    return gat_cpu.CounterDropout(seed, p_ext, 0.0, p, p) if p_ext > 0 or p > 0 else None


def _plain_tape(m, out):
    """(tape, row capacity, head units HT, {table: byte offset}) of ``out``'s training step: a 256-byte header, then h0, h1, per
    layer the aggregate (SAGE mean | GIN s), GIN's u, z, hout, the float64 mean / rstd, then hbd -- [rows][width] float32 tables
    (hidden wide, hbd HT wide), each 256-byte aligned."""
    tape = out["class_logits"].grad_fn.info["tape"]
    hid, L, nh = m.hidden_channels, m.num_gnn_layers, 3 if m.predict_correction else 2
    gin = m.gnn_type == "GIN"

    def layout(rows, HT):
        off, t = 256, {}

        def take(key, nbytes):
            nonlocal off
            t[key] = off
            off += (nbytes + 255) & ~255
        take("h0", rows * hid * 4); take("h1", rows * hid * 4)
        for l in range(L):
            take(("agg", l), rows * hid * 4)
            if gin:
                take(("u", l), rows * hid * 4)
            take(("z", l), rows * hid * 4); take(("hout", l), rows * hid * 4)
            take(("mean", l), hid * 8); take(("rstd", l), hid * 8)
        take("hbd", rows * HT * 4)
        return off, t

    HT = -(-nh * (hid // 2) // 32) * 32                 # head_hidden_total: the heads' units padded to a multiple of 32
    per_row = 4 * (2 * hid + L * (4 if gin else 3) * hid + HT)
    est = (tape.numel() - 256) // per_row
    for rows in range(est, max(est - 64, -1), -1):      # (the total grows strictly with the row count: one match at most)
        total, t = layout(rows, HT)
        if total == tape.numel():
            return tape, rows, HT, t
    raise AssertionError("the tape's size fits no PlainTapeLayout of this model")


def _lin_pre(inp, sd, prefix):
    """A Linear's output v = W inp + b in float64 from the kernels' own input, and the bound on its float32 rounding in any
    summation order: (K + 1) eps (|W| |inp| + |b|)."""
    W = torch.as_tensor(np.asarray(sd[prefix + ".weight"]), dtype=torch.float64)
    b = torch.as_tensor(np.asarray(sd[prefix + ".bias"]), dtype=torch.float64)
    inp = inp.double()
    return inp @ W.T + b, (W.shape[1] + 1) * EPS32 * (inp.abs() @ W.abs().T + b.abs())


def _patterns(m, out, n, drop, sd, x):
    """The kernels' ReLU patterns over the first ``n`` rows, in the oracle's call order (extractor h0; per layer GIN's u, then the
    layer output but the last's; the heads' hidden units); for each the dropout mask that follows it (None: nothing dropped) and
    (pre, bound): the ReLU's input recomputed in float64 from the kernels' own tables on the tape (the Linear's input, or z and the
    batch statistics) and the bound on the float32 rounding of the kernel that made it."""
    tape, _, HT, t = _plain_tape(m, out)
    hid, L, nh = m.hidden_channels, m.num_gnn_layers, 3 if m.predict_correction else 2
    hh = hid // 2

    def table(off, w):
        return tape[off:off + n * w * 4].view(torch.float32).view(n, w).cpu()

    def keep(p, stream, w):
        if drop is None or p <= 0:
            return None
        return drop.elementwise(torch.ones(n, w, dtype=torch.float64), p, stream) != 0

    def stats(off):
        return tape[off:off + hid * 8].view(torch.float64).cpu()

    def bn_rounding(l):
        z = table(t[("z", l)], hid).double()
        pre = f"gnn.norms.{l}.module."
        scale = torch.as_tensor(np.asarray(sd[pre + "weight"]), dtype=torch.float64) * stats(t[("rstd", l)])
        shift = torch.as_tensor(np.asarray(sd[pre + "bias"]), dtype=torch.float64) - stats(t[("mean", l)]) * scale
        v = z * scale + shift                         # (bn_train.hip: float32 z * scale + shift)
        return v, 2 * EPS32 * ((z * scale).abs() + shift.abs() + v.abs())
    pats, keeps = [table(t["h0"], hid) > 0], [keep(drop.p_extractor if drop else 0, 1, hid)]
    allow = [_lin_pre(torch.as_tensor(np.asarray(x[:n])), sd, "feature_extractor.mlp.0")]
    for l in range(L):
        if m.gnn_type == "GIN":
            pats.append(table(t[("u", l)], hid) > 0); keeps.append(None)
            allow.append(_lin_pre(table(t[("agg", l)], hid), sd, f"gnn.convs.{l}.nn.0"))
        if l < L - 1:
            pats.append(table(t[("hout", l)], hid) > 0); keeps.append(keep(drop.p_features if drop else 0, 64 + l, hid))
            allow.append(bn_rounding(l))
    hb, h_last = table(t["hbd"], HT), table(t[("hout", L - 1)], hid)
    k_all = keep(drop.p_heads if drop else 0, 2, nh * hh)
    for k, head in enumerate(("classification_head", "confidence_head", "correction_head")[:nh]):
        pats.append(hb[:, k * hh:(k + 1) * hh] > 0)
        keeps.append(None if k_all is None else k_all[:, k * hh:(k + 1) * hh])
        allow.append(_lin_pre(h_last, sd, head + ".mlp.0"))
    return pats, keeps, allow


def _oracle(m, out, n, sd, x, ei, ea, drop, w, monkeypatch):
    """float64 / float32 oracle gradients with the kernels' ReLU patterns.  Every input where a pattern disagrees with float64's
    sign (and dropout keeps it) lies within BOUND_C x the float32 oracle's distance of 0 (the rule of test_gpu_backward_training),
    or the pattern is the sign of the kernels' own ReLU input recomputed from the tape, up to that kernel's float32 rounding.  The
    second case covers tiny batches: two rows give the float32 oracle's distance too few samples to be a yardstick, and the
    kernels' BatchNorm applies the statistics as z * scale + shift, whose rounding is relative to |z * scale|, not to |v|."""
    pats, keeps, allow = _patterns(m, out, n, drop, sd, x)
    f64, f32 = _KernelReLU(pats), _KernelReLU(pats)
    g64, _ = oracle_grads(sd, x, ei, ea, torch.float64, drop, w, monkeypatch, functional=f64)
    g32, _ = oracle_grads(sd, x, ei, ea, torch.float32, drop, w, monkeypatch, functional=f32)
    assert f64.i == f32.i == len(pats), (f64.i, f32.i, len(pats))
    n_bad, n_own, worst, bad = 0, 0, 0.0, []
    for i, (v64, v32, pat, kp, (pre, rnd)) in enumerate(zip(f64.seen, f32.seen, pats, keeps, allow)):
        off = pat != (v64 > 0)
        if kp is not None:
            off &= kp
        if off.any():
            r = v64[off].abs() / (BOUND_C * (v32.double() - v64).abs().max().item())
            own = (pat[off] == (pre[off] > 0)) | (pre[off].abs() <= rnd[off])
            n_bad += int(off.sum())
            n_own += int((own & (r > 1)).sum())
            worst = max(worst, r.max().item())
            if not bool((own | (r <= 1)).all()):
                bad.append(i)
    print(f"  ReLU inputs on the other side of 0 on the GPU: {n_bad} (largest |v| {worst:.3f} x the float32 bound; "
          f"{n_own} beyond it follow the kernels' own input)")
    assert not bad, f"ReLUs {bad}: a pattern differs from float64 beyond rounding and from the kernels' own input"
    return g64, g32


def _parity(group, name, m, sd, data, x, ei, ea, monkeypatch, p, seed, p_ext=None):
    drop = _drop(m, seed, p if p_ext is None else p_ext, p)
    w = _loss_weights(x.shape[0], m.num_classes)
    g_gpu, out = _step(m, data, w, seed)
    g64, g32 = _oracle(m, out, x.shape[0], sd, x, ei, ea, drop, w, monkeypatch)
    _accept(group, name, g_gpu, g64, g32)
    return g_gpu, out


# ---- 1. parity sweep over shapes and stencils ------------------------------------------------------------------------------------

SWEEP = [  # (layers, hidden, connectivity)
    (1, 32, "4-connected"),
    (2, 64, "16-dilated"),
    (4, 64, "8-connected"),
    (2, 128, "8-connected"),
    (4, 128, "4-connected"),
    (4, 32, "16-dilated"),
]


@pytest.mark.parametrize("p", [0.0, 0.1])
@pytest.mark.parametrize("layers,hidden,conn", SWEEP)
@pytest.mark.parametrize("kind", KINDS)
def test_parity_sweep(kind, layers, hidden, conn, p, gpu_device, monkeypatch):
    """Two unequal V1 tiles (holes) in one batch; every dropout at p (the extractor's too)."""
    sd = _sd(kind, hidden=hidden, num_layers=layers, seed=101 + layers)
    m = _net(sd, kind, hidden_channels=hidden, num_gnn_layers=layers)
    g, x, ei, ea = _tiles_graph([_tile(37, 45, 3, "V1"), _tile(30, 40, 4, "V1")], conn)
    _parity("sweep", f"{kind} L{layers} h{hidden} {conn} p{p}", m, sd, g, x, ei, ea, monkeypatch, p, seed=17)


@pytest.mark.parametrize("kind", KINDS)
def test_parity_stencil_self_loops(kind, gpu_device, monkeypatch):
    """GraphBuilder(include_self_loops=True): the self loop is an ordinary edge of SAGEConv's mean and GINConv's sum."""
    from bathymetric_gnn_amd.data import GraphBuilder
    tiles = [_tile(33, 41, 5, "V1"), _tile(25, 30, 6, "V1")]
    g = GraphBuilder(include_self_loops=True).build_graphs([t[0] for t in tiles], [t[1] for t in tiles], None, [(0.5, 0.5)] * 2)
    x, ei, ea, _, _ = graph_cpu.batch_graphs([graph_cpu.build_graph(d, v, None, (0.5, 0.5), include_self_loops=True)
                                               for d, v, _ in tiles])
    assert (ei[0] == ei[1]).sum() == x.shape[0]
    sd = _sd(kind, num_layers=3, seed=107)
    m = _net(sd, kind, num_gnn_layers=3)
    _parity("sweep", f"{kind} self loops", m, sd, g, x, ei, ea, monkeypatch, 0.1, seed=19)


# ---- 2. foreign graphs ----------------------------------------------------------------------------------------------------------

def _foreign_data():
    """_foreign_graph without its explicit self loops: asymmetric random edges, a 40-in-edge hub, 30 repeated edges and ten
    isolated nodes, as a Data (bgnn_graph_from_edges)."""
    from bathymetric_gnn_amd.data import Data
    x, ei, ea = _foreign_graph()
    keep = ei[0] != ei[1]
    ei, ea = np.ascontiguousarray(ei[:, keep]), np.ascontiguousarray(ea[keep])
    pairs = set(zip(ei[0].tolist(), ei[1].tolist()))
    assert sum((b, a) not in pairs for a, b in pairs) > 1000                  # mostly one-way
    assert len(pairs) < ei.shape[1]                                           # repeated edges
    assert len(set(range(x.shape[0])) - set(ei.ravel().tolist())) >= 10       # isolated nodes
    data = Data(x=torch.from_numpy(x).cuda(), edge_index=torch.from_numpy(ei).cuda(), edge_attr=torch.from_numpy(ea).cuda())
    return data, x, ei, ea


@pytest.mark.parametrize("p", [0.0, 0.1])
@pytest.mark.parametrize("kind", KINDS)
def test_parity_foreign_graph(kind, p, gpu_device, monkeypatch):
    data, x, ei, ea = _foreign_data()
    sd = _sd(kind, num_layers=3, seed=109)
    m = _net(sd, kind, num_gnn_layers=3)
    _parity("foreign", f"{kind} p{p}", m, sd, data, x, ei, ea, monkeypatch, p, seed=23)


# ---- 3. determinism and forward identity ----------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", KINDS)
def test_backward_is_deterministic(kind, gpu_device):
    """Two backward passes on the same tape give bit-identical gradients (dropout on)."""
    sd = _sd(kind, num_layers=4, seed=111)
    m = _net(sd, kind)
    _drop(m, 3, 0.1, 0.1)
    g, x, _, _ = _tiles_graph([_tile(64, 64, 7, "V1")])
    m.train(); m.dropout_seed = 3
    loss = _loss(m(g), _loss_weights(x.shape[0], 3))
    loss.backward(retain_graph=True)
    first = {n: p.grad.clone() for n, p in m.named_parameters()}
    assert torch.count_nonzero(first["gnn.convs.0." + ("lin_l.weight" if kind == "GraphSAGE" else "nn.0.weight")])
    m.zero_grad(set_to_none=True)
    loss.backward()
    for n, p in m.named_parameters():
        assert torch.equal(first[n], p.grad), n


@pytest.mark.parametrize("kind", KINDS)
def test_taped_forward_changes_nothing(kind, gpu_device):
    """The taped forward's outputs and running statistics are bit-identical to the same forward under no_grad."""
    sd = _sd(kind, num_layers=4, seed=113)
    g, _, _, _ = _tiles_graph([_tile(37, 45, 3, "V1"), _tile(20, 64, 4, "V0")])
    res = []
    for taped in (False, True):
        m = _net(sd, kind)
        _drop(m, 11, 0.1, 0.1)
        m.train(); m.dropout_seed = 11
        with torch.set_grad_enabled(taped):
            out = m(g)
        assert (out["class_logits"].grad_fn is not None) == taped
        if taped:
            assert out["class_logits"].grad_fn.info.get("tape") is not None and "refusal" not in out["class_logits"].grad_fn.info
        res.append(({k: v.detach().clone() for k, v in out.items()},
                    [(n.module.running_mean.clone(), n.module.running_var.clone()) for n in m.gnn.norms]))
    for k in res[0][0]:
        assert torch.equal(res[0][0][k], res[1][0][k]), k
    for a, b in zip(res[0][1], res[1][1]):
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


# ---- 4. batch scale ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", KINDS)
def test_million_nodes_by_replication(kind, gpu_device, monkeypatch):
    """16 copies of one 256 x 256 V0 tile (1 048 576 nodes), default shape, dropout 0, the linear loss's per-node weights tiled:
    every copy's outputs are bit-identical to copy 0's, a second backward on the tape is bit-identical, and gradient / 16 passes
    the acceptance rule against the tile's float64 / float32 gradients (ReLU patterns of copy 0 from the tape)."""
    B = 16
    sd = _sd(kind, num_layers=4, seed=117)
    m = _net(sd, kind)
    g, x, ei, ea = _batch([_tile(256, 256, 21, "V0")], copies=B)
    n1 = x.shape[0]
    assert n1 == 256 * 256 and g.num_nodes == B * n1 >= 1 << 20
    w = _loss_weights(n1, 3)
    _drop(m, 0, 0.0, 0.0)
    m.train(); m.zero_grad(set_to_none=True)
    out = m(g)
    assert _plain_tape(m, out)[1] >= B * n1
    _copies_identical(out, B, n1)
    loss = _loss(out, _tiled(w, B))
    loss.backward(retain_graph=True)
    first = {n: p.grad.detach().clone() for n, p in m.named_parameters()}
    m.zero_grad(set_to_none=True)
    loss.backward()
    for n, p in m.named_parameters():
        assert torch.equal(first[n], p.grad), n
    g64, g32 = _oracle(m, out, n1, sd, x, ei, ea, None, w, monkeypatch)
    _accept("scale", f"{kind} 1M nodes, {B} copies", {n: v.double().cpu() for n, v in first.items()}, g64, g32, scale=B)


# ---- 5. edges of the domain ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", KINDS)
def test_two_node_batch(kind, gpu_device, monkeypatch):
    """Two neighbouring cells, the smallest batch BatchNorm trains on.  Two rows normalise every column to about +-1, so the
    gradient through BatchNorm is a residual of that eps-level deviation: for most GraphSAGE weight draws the float32 oracle's own
    gradient error exceeds the gradient (no yardstick left).  The draw used here is one where float32 still resolves it."""
    valid = np.zeros((8, 8), bool)
    valid[3, 3:5] = True
    sd = _sd(kind, num_layers=4, seed=137)
    m = _net(sd, kind)
    g, x, ei, ea = _batch([_masked(8, 8, valid)])
    assert x.shape[0] == 2 == g.num_nodes
    _parity("edges", f"{kind} 2 nodes", m, sd, g, x, ei, ea, monkeypatch, 0.0, seed=29)


@pytest.mark.parametrize("kind", KINDS)
def test_capacity_far_above_nodes(kind, gpu_device, monkeypatch):
    """Four sparse 128 x 128 tiles: ~3 000 nodes in 65 536 rows of capacity."""
    sd = _sd(kind, num_layers=4, seed=121)
    m = _net(sd, kind)
    g, x, ei, ea = _batch(_sparse_tiles())
    assert x.shape[0] < 4000
    _, out = _parity("edges", f"{kind} sparse", m, sd, g, x, ei, ea, monkeypatch, 0.1, seed=31)
    assert _plain_tape(m, out)[1] >= 4 * 128 * 128


@pytest.mark.parametrize("kind", KINDS)
def test_empty_batch(kind, gpu_device):
    sd = _sd(kind, num_layers=4, seed=123)
    m = _net(sd, kind)
    _set_dropout(m, 0.1)
    g, x, _, _ = _batch([_masked(16, 16, np.zeros((16, 16), bool)), _masked(12, 20, np.zeros((12, 20), bool))])
    assert x.shape[0] == 0 == g.num_nodes
    m.train(); m.dropout_seed = 3
    out = m(g)
    assert all(v.shape[0] == 0 for v in out.values())
    _loss(out, _loss_weights(0, 3)).backward()
    for n, p in m.named_parameters():
        assert p.grad is not None and not torch.count_nonzero(p.grad), n


@pytest.mark.parametrize("kind", KINDS)
def test_short_training_trajectory(kind, gpu_device, monkeypatch):
    """AdamW with clip_grad_norm_(1.0) (the reference's training step) for 12 steps, dropout on: the parameters stay finite, the
    first step's loss is the float64 oracle's, and the dropout-free loss of the trained model is below the initial model's."""
    sd = _sd(kind, num_layers=3, seed=125)
    m = _net(sd, kind, num_gnn_layers=3)
    g, x, ei, ea = _tiles_graph([_tile(32, 40, 8, "V1")])
    w = {k: v / x.shape[0] for k, v in _loss_weights(x.shape[0], 3, seed=9).items()}
    opt = torch.optim.AdamW(m.parameters(), lr=1e-3)
    losses = []
    for step in range(12):
        drop = _drop(m, step, 0.1, 0.1)
        m.train(); m.dropout_seed = step
        opt.zero_grad(set_to_none=True)
        loss = _loss(m(g), w)
        if step == 0:
            _, l64 = oracle_grads(sd, x, ei, ea, torch.float64, drop, w, monkeypatch)
            assert abs(float(loss.detach()) - l64) <= 1e-4 * (1 + abs(l64))
        loss.backward()
        torch.nn.utils.clip_grad_norm_(m.parameters(), 1.0)
        opt.step()
        losses.append(float(loss.detach()))
        assert all(torch.isfinite(p).all() for p in m.parameters())
    _drop(m, 0, 0.0, 0.0)
    with torch.no_grad():
        m.train()
        end = float(_loss(m(g), w))
    m2 = _net(sd, kind, num_gnn_layers=3)
    _drop(m2, 0, 0.0, 0.0)
    with torch.no_grad():
        m2.train()
        start = float(_loss(m2(g), w))
    print(f"{kind}: losses {losses}; dropout-free loss {start:.5f} -> {end:.5f}")
    assert end < start


# ---- 6. refusals that stay ----------------------------------------------------------------------------------------------------

def test_gcn_still_refuses(gpu_device):
    """GCN keeps its refusal: backward() raises NotImplementedError naming the covered backbones; the forward values are those of
    the untaped forward."""
    sd = _sd("GCN", num_layers=2, seed=127)
    g, x, _, _ = _tiles_graph([_tile(30, 30, 9, "V1")])
    m = _net(sd, "GCN", num_gnn_layers=2)
    m.train(); m.dropout_seed = 1
    with torch.no_grad():
        plain = m(g)["class_logits"].clone()
    m = _net(sd, "GCN", num_gnn_layers=2)
    m.train(); m.dropout_seed = 1
    out = m(g)
    assert torch.equal(out["class_logits"].detach(), plain)
    with pytest.raises(NotImplementedError, match="GAT"):
        _loss(out, _loss_weights(x.shape[0], 3)).backward()


def test_padded_sage_still_refuses_training(gpu_device):
    """hidden 100 runs zero-padded: the training-mode forward refuses it (eval still runs)."""
    sd = _sd("GraphSAGE", hidden=100, num_layers=2, seed=129)
    g, _, _, _ = _tiles_graph([_tile(20, 20, 9, "V1")])
    m = _net(sd, "GraphSAGE", hidden_channels=100, num_gnn_layers=2)
    m.eval()
    assert torch.isfinite(m(g)["class_logits"]).all()
    m.train()
    with pytest.raises(NotImplementedError, match="zero-padded"):
        m(g)


@pytest.mark.parametrize("kind", KINDS)
def test_foreign_self_loops_still_refused(kind, gpu_device):
    """A foreign graph with explicit self loops: SAGEConv / GINConv would count them as edges, which the CSR does not hold."""
    from bathymetric_gnn_amd.data import Data
    x, ei, ea = _foreign_graph()
    assert (ei[0] == ei[1]).any()
    data = Data(x=torch.from_numpy(x).cuda(), edge_index=torch.from_numpy(ei).cuda(), edge_attr=torch.from_numpy(ea).cuda())
    m = _net(_sd(kind, num_layers=2, seed=131), kind, num_gnn_layers=2)
    m.train()
    with pytest.raises(NotImplementedError, match="self loops"):
        m(data)
