"""The GAT backward pass where training runs it: at batch scale, under the training loss, at survey depths, with several tapes in
flight and on edge graphs.  ``tests/test_gpu_backward.py`` holds the kernels to float64 on graphs of a few thousand nodes near
-20 m under a random linear loss; the branches below only run outside that envelope.

A. Batch scale by replication.  With every dropout at 0, B copies of one tile in one batch have that tile's BatchNorm batch
   statistics, every node computes what its twin in copy 0 computes, and the parameter gradient of the summed per-node loss is
   B x the single-tile gradient.  So a 1.1 M-node backward (row capacity >= 32 768: the W-resident GEMM form inside the backward,
   the taped fused-front branch, wgrad / colsum / BatchNorm reductions over up to 1 024 chunks) is held to the float64 oracle of
   one tile.
B. Row capacity far above the node count: sparse masks on large tiles, so the scale-only code paths run over mostly empty
   chunks, against the oracle directly.
C. The upstream training loss restated from its formulas, and losses that reach only some outputs (NULL output gradients).
D. Survey depths, -20 .. -10 000 m.
E. Two tapes in flight across a validation forward that repacks the model.
F. The smallest trainable batch, self-loop-only nodes and the empty batch.

Acceptance rule everywhere (``test_gpu_backward``): per parameter, max |g_gpu - g64| <= BOUND_C * max |g32 - g64| + FLOOR_REL *
max |g64|; a parameter the oracle's autograd does not reach must be exactly 0 on the GPU.  Every distance and its float32
yardstick is printed; the largest ratio per group is printed at the end of the module.

ReLU patterns.  ReLU's derivative jumps at 0.  An input within rounding of 0 (thousands of the ~1e6 ReLU inputs of these graphs
sit within BOUND_C x float32's distance of it) takes its side by the arithmetic's rounding, and one node on the other side moves
the gradients below it by that node's whole share -- ~1 / N of a sum, far above rounding.  The float32 oracle flips other inputs
than the kernels, so the float32 yardstick does not cover it: the kernels miss it by 10 .. 1000 x wherever they flip an input with
a large upstream gradient.  So the oracle runs with the kernels' ReLU patterns (from the tape: h0, the layer outputs, the heads'
hidden units, > 0), as it runs with their dropout masks, and ``_KernelReLU.check`` asserts that every input where the pattern
and float64 disagree is within BOUND_C x float32's distance of 0."""
import json

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from _conditioning import BOUND_C, DEPTH_BANDS, deep_tile, float64_bound
from oracle import gat_cpu, graph_cpu
from test_gpu_backward import FLOOR_REL, _foreign_graph, _loss, _loss_weights, _model, _set_dropout, oracle_grads

pytestmark = pytest.mark.gpu
RES = (0.5, 0.5)
WRES_MIN_ROWS = 32768           # launch_gemm_f32's W-resident form (K = 64) and the fused front from this row capacity on
WORST = {}                      # group -> (largest d_gpu / d32 where the yardstick term dominates the bound, largest d_gpu / bound)


@pytest.fixture(scope="module", autouse=True)
def _print_worst():
    yield
    if WORST:
        print("\nworst per group:", json.dumps({k: {"d_over_f32": v[0], "d_over_bound": v[1]} for k, v in sorted(WORST.items())}))


def _ctx():
    from bathymetric_gnn_amd import runtime as rt
    return rt.get_context(torch.device("cuda:0"))


def _sd(**kw):
    from bathymetric_gnn_amd import synthetic
    return synthetic.synthetic_state_dict(**kw)


def _net(sd, **kw):
    kw.setdefault("in_channels", 7)
    kw.setdefault("edge_dim", 3)
    return _model(sd, torch.device("cuda:0"), **kw)


def _tile(h, w, seed, variant="V1", unc=False):
    from bathymetric_gnn_amd import synthetic
    return synthetic.synthetic_tile(h, w, seed, variant, unc)


def _batch(tiles, conn="8-connected", copies=1):
    """The device batch of ``copies`` x ``tiles`` (tile order repeated) and the oracle's (x, edge_index, edge_attr) of ``tiles``
    once."""
    from bathymetric_gnn_amd.data import GraphBuilder
    ts = list(tiles) * copies
    unc = None if tiles[0][2] is None else [t[2] for t in ts]
    g = GraphBuilder(connectivity=conn).build_graphs([t[0] for t in ts], [t[1] for t in ts], unc, [RES] * len(ts))
    x, ei, ea, _, _ = graph_cpu.batch_graphs([graph_cpu.build_graph(d, m, u, RES, connectivity=conn) for d, m, u in tiles])
    return g, x, ei, ea


def _dropout(m, seed, p_ext, p):
    """Dropout p everywhere but the extractor (p_ext) on the model; the oracle's CounterDropout with the same seed, or None."""
    _set_dropout(m, p)
    m.feature_extractor.mlp[2].p = p_ext
    return gat_cpu.CounterDropout(seed, p_ext, p, p, p) if p_ext > 0 or p > 0 else None


def _tiled(w, copies):
    return {k: np.tile(v, (copies,) + (1,) * (v.ndim - 1)) for k, v in w.items()}


def _tape_rows_at_least(m, out, rows):
    """The tape of ``out``'s training step holds at least ``rows`` rows (the library sizes every table by the graph's row
    capacity: 4 bytes x (2 hidden + per layer heads x hidden + 2 heads + 2 width + the heads' hidden units) per row)."""
    info = out["class_logits"].grad_fn.info
    hid = m.hidden_channels
    per_row = 2 * hid + (3 if m.predict_correction else 2) * (hid // 2)
    for c in m.gnn.convs:
        width = c.heads * hid if c.concat else hid
        per_row += c.heads * hid + 2 * c.heads + 2 * width
    assert info["tape"].numel() >= 4 * per_row * rows, (info["tape"].numel(), per_row, rows)


class TrainingLoss:
    """The upstream multi-task training loss, restated from its formulas: class-weighted cross-entropy on class_logits with label
    smoothing 0.1 (weight 1), Huber on correction over the noise-labelled nodes (0.5), binary cross-entropy of confidence against
    ``argmax == label`` (0.2), and two penalties that depend on the argmax only (no gradient).  Labels, class weights, noise
    mask and correction targets come from a fixed seed.  ``terms`` picks the parts that carry a gradient; "probs" (not upstream)
    is a Brier score on class_probs, the one way to give class_probs a gradient of its own.

    The confidence target ``argmax == label`` is taken from the first outputs the loss sees -- the float64 oracle's -- and then
    held, so that a near-tie that float32 rounding flips cannot change the loss between the references and the GPU."""
    FULL = ("logits", "confidence", "correction")

    def __init__(self, N, nc, terms=FULL, seed=11):
        r = np.random.default_rng(seed)
        self.nc, self.terms = nc, terms
        self.labels = r.integers(0, nc, N)
        self.class_w = r.uniform(0.5, 2.0, nc)
        self.noise = r.random(N) < 0.3
        self.corr_t = r.normal(0.0, 0.5, N)
        self.correct = None

    def __call__(self, out):
        logits = out["class_logits"]
        dt, dev = logits.dtype, logits.device
        lab = torch.as_tensor(self.labels, device=dev)
        if self.correct is None:
            self.correct = logits.detach().argmax(-1).cpu().numpy() == self.labels
        loss = torch.zeros((), dtype=dt, device=dev)
        if "logits" in self.terms:
            loss = loss + F.cross_entropy(logits, lab, weight=torch.as_tensor(self.class_w, dtype=dt, device=dev), label_smoothing=0.1)
        if "probs" in self.terms:
            loss = loss + ((out["class_probs"] - F.one_hot(lab, self.nc).to(dt)) ** 2).sum(-1).mean()
        if "confidence" in self.terms:
            loss = loss + 0.2 * F.binary_cross_entropy(out["confidence"], torch.as_tensor(self.correct, dtype=dt, device=dev))
        if "correction" in self.terms and "correction" in out:
            noise = torch.as_tensor(self.noise, device=dev)
            loss = loss + 0.5 * F.huber_loss(out["correction"][noise], torch.as_tensor(self.corr_t, dtype=dt, device=dev)[noise])
        pred = logits.detach().argmax(-1)                 # argmax-only terms: values, no gradient
        loss = loss + 0.3 * ((lab == 1) & (pred == self.nc - 1)).to(dt).mean() + 0.5 * ((lab == 0) & (pred != 0)).to(dt).mean()
        return loss


def _accept(group, name, g_gpu, g64, g32, scale=1):
    """The acceptance rule over every parameter; ``g_gpu`` / ``scale`` is compared (B copies: scale = B, a power of two)."""
    gmax = max(v.abs().max().item() for v in g64.values())
    floor = FLOOR_REL * gmax
    bad, rows = [], []
    r_f32 = r_bound = 0.0
    assert set(g64) <= set(g_gpu), set(g64) - set(g_gpu)
    for k, v in g_gpu.items():
        if k not in g64:                                  # the loss does not reach it
            rows.append(f"{k}: unreached, max|g_gpu| {v.abs().max().item():.3e}")
            if torch.count_nonzero(v):
                bad.append(f"{k}: the loss does not reach it, yet the GPU gradient is not 0 ({v.abs().max().item():.3e})")
            continue
        d = (v.reshape(g64[k].shape) / scale - g64[k]).abs().max().item()
        d32 = (g32[k] - g64[k]).abs().max().item()
        bound = BOUND_C * d32 + floor
        rows.append(f"{k}: gpu {d:.3e} f32 {d32:.3e} bound {bound:.3e}")
        r_bound = max(r_bound, d / bound)
        if BOUND_C * d32 >= floor:
            r_f32 = max(r_f32, d / d32)
        if not d <= bound:
            bad.append(f"{k}: gpu {d:.3e} vs f32 {d32:.3e} (floor {floor:.3e})")
    print(f"[{group}] {name}: max|g64| {gmax:.3e}, worst d/f32 {r_f32:.3f}, worst d/bound {r_bound:.3f}\n  " + "\n  ".join(rows))
    w = WORST.get(group, (0.0, 0.0))
    WORST[group] = (max(w[0], r_f32), max(w[1], r_bound))
    assert not bad, "\n".join(bad)


def _tape_tables(m, out):
    """(tape, row capacity, head units HT, {table: byte offset}) of ``out``'s GAT training step (train_api.hip tape_layout: a
    256-byte header, then [row capacity][width] float32 tables, each 256-byte aligned)."""
    tape = out["class_logits"].grad_fn.info["tape"]
    hid, nh = m.hidden_channels, 3 if m.predict_correction else 2
    hh = hid // 2

    def layout(rows, HT):
        off, t = 256, {}

        def take(key, nbytes):
            nonlocal off
            t[key] = off
            off += (nbytes + 255) & ~255
        take("h0", rows * hid * 4); take("h1", rows * hid * 4)
        for l, c in enumerate(m.gnn.convs):
            HC = c.heads * hid
            W = HC if c.concat else hid
            take(("xw", l), rows * HC * 4); take(("asd", l), rows * 2 * c.heads * 4)
            take(("z", l), rows * W * 4); take(("hout", l, W), rows * W * 4)
            take(("mean", l), W * 8); take(("rstd", l), W * 8)
        take("hbd", rows * HT * 4)
        return off, t

    per_row = 4 * (2 * hid + sum(c.heads * hid + 2 * c.heads + 2 * (c.heads * hid if c.concat else hid) for c in m.gnn.convs))
    found = None
    for HT in (nh * hh, -(-nh * hh // 32) * 32):
        est = (tape.numel() - 256) // (per_row + 4 * HT)
        for rows in range(est, max(est - 64, -1), -1):
            total, t = layout(rows, HT)
            if total == tape.numel():
                found = (rows, HT, t)
                break
        if found:
            break
    assert found, "the tape's size fits no layout of this model"
    return (tape,) + found


def _tape_relu_patterns(m, out, n):
    """The kernels' ReLU patterns of ``out``'s training step, in the order the oracle applies its ReLUs: the extractor's h0, the
    output of every GAT layer but the last, then each head's hidden units -- every one ``> 0`` over the first ``n`` rows of the
    tape."""
    tape, rows, HT, t = _tape_tables(m, out)
    hid, nh = m.hidden_channels, 3 if m.predict_correction else 2
    hh = hid // 2

    def table(off, w):
        return tape[off:off + n * w * 4].view(torch.float32).view(n, w).cpu()
    pats = [table(t["h0"], hid) > 0]
    pats += [table(off, k[2]) > 0 for k, off in t.items() if isinstance(k, tuple) and k[0] == "hout" and k[1] < len(m.gnn.convs) - 1]
    hb = table(t["hbd"], HT)
    pats += [hb[:, k * hh:(k + 1) * hh] > 0 for k in range(nh)]
    return pats


class _KernelReLU:
    """``torch.nn.functional`` for the oracle, with its ReLUs (extractor, GAT layers, heads, in call order) taking the kernels'
    patterns: relu(v) = v * pattern.  Where the pattern and v's sign disagree, v is a dropped unit (the dropout mask that follows
    zeroes it either way) or an input within rounding of 0, whose forward value changes by |v|."""

    def __init__(self, patterns):
        self.patterns, self.seen, self.i = patterns, [], 0

    def __getattr__(self, name):
        return getattr(F, name)

    def relu(self, v):
        pat = self.patterns[self.i].to(v.dtype)
        self.i += 1
        self.seen.append(v.detach())
        return v * pat

    @staticmethod
    def check(f64, f32, drop, hid, nh):
        """Every input whose kernel pattern disagrees with float64's sign while dropout keeps it lies within BOUND_C x the float32
        oracle's distance to float64 of 0 (a rounding-level kink input, not a defect).  Returns (disagreements, largest |v| / bound)."""
        assert f64.i == f32.i == len(f64.patterns), (f64.i, f32.i, len(f64.patterns))
        L = len(f64.patterns) - 1 - nh
        n_bad, worst = 0, 0.0
        for i, (v64, v32, pat) in enumerate(zip(f64.seen, f32.seen, f64.patterns)):
            keep = torch.ones_like(pat)
            if drop is not None:
                if i == 0 and drop.p_extractor > 0:
                    keep = drop.elementwise(torch.ones(pat.shape, dtype=torch.float64), drop.p_extractor, 1) != 0
                elif 0 < i <= L and drop.p_features > 0:
                    keep = drop.elementwise(torch.ones(pat.shape, dtype=torch.float64), drop.p_features, 64 + i - 1) != 0
                elif i > L and drop.p_heads > 0:
                    k = i - L - 1
                    m_all = drop.elementwise(torch.ones(pat.shape[0], nh * pat.shape[1], dtype=torch.float64), drop.p_heads, 2)
                    keep = m_all[:, k * pat.shape[1]:(k + 1) * pat.shape[1]] != 0
            off = keep & (pat != (v64 > 0))
            if off.any():
                bound = BOUND_C * (v32.double() - v64).abs().max().item()
                n_bad += int(off.sum())
                worst = max(worst, v64[off].abs().max().item() / bound)
        assert worst <= 1.0, f"a ReLU input {worst:.2f} x the rounding bound away from 0 takes the other side on the GPU"
        return n_bad, worst


def _oracle(sd, x, ei, ea, drop, loss, monkeypatch, outputs=False, patterns=None, hid=64, nh=3):
    """float64 first (a TrainingLoss fixes its confidence target there), then float32; with ``patterns``, both run with the
    kernels' ReLU patterns (``_KernelReLU``), and the disagreements with float64's own signs are checked and printed."""
    o64, o32 = {}, {}
    f64 = _KernelReLU(patterns) if patterns is not None else None
    f32 = _KernelReLU(patterns) if patterns is not None else None
    g64, _ = oracle_grads(sd, x, ei, ea, torch.float64, drop, loss, monkeypatch, outputs=o64, functional=f64)
    g32, _ = oracle_grads(sd, x, ei, ea, torch.float32, drop, loss, monkeypatch, outputs=o32, functional=f32)
    if patterns is not None:
        n_bad, worst = _KernelReLU.check(f64, f32, drop, hid, nh)
        print(f"  ReLU inputs on the other side of 0 on the GPU: {n_bad} (largest |v| {worst:.3f} x the rounding bound)")
    return (g64, g32, o64, o32) if outputs else (g64, g32)


def _oracle_for(m, out, n, sd, x, ei, ea, drop, loss, monkeypatch, outputs=False):
    """``_oracle`` with the ReLU patterns of the GPU step that produced ``out``."""
    return _oracle(sd, x, ei, ea, drop, loss, monkeypatch, outputs, _tape_relu_patterns(m, out, n), m.hidden_channels,
                   3 if m.predict_correction else 2)


def _step(m, data, loss, seed):
    """One taped training forward + backward on the GPU: ({name: gradient, float64 on the host}, outputs)."""
    m.train()
    m.dropout_seed = seed
    m.zero_grad(set_to_none=True)
    out = m(data)
    _loss(out, loss).backward()
    return {n: p.grad.detach().double().cpu() for n, p in m.named_parameters()}, out


def _parity(group, name, m, sd, data, x, ei, ea, monkeypatch, p=0.1, p_ext=None, seed=5, loss=None):
    drop = _dropout(m, seed, p if p_ext is None else p_ext, p)
    if loss is None:
        loss = _loss_weights(x.shape[0], m.num_classes)
        if not m.predict_correction:
            loss.pop("correction")
    g_gpu, out = _step(m, data, loss, seed)
    if isinstance(loss, TrainingLoss):              # (its confidence target comes from the float64 outputs: fixed before the GPU's)
        loss.correct = None
    g64, g32 = _oracle_for(m, out, x.shape[0], sd, x, ei, ea, drop, loss, monkeypatch)
    if isinstance(loss, TrainingLoss):
        g_gpu, out = _step(m, data, loss, seed)
    _accept(group, name, g_gpu, g64, g32)
    return out


# ---- A. batch scale by replication -----------------------------------------------------------------------------------------------

def _copies_identical(out, B, n1):
    for k in ("class_logits", "confidence", "correction"):
        v = out[k].detach().reshape(B, n1, -1)
        same = (v == v[:1]).all(dim=2).all(dim=1)
        assert bool(same.all()), f"{k}: copies {torch.nonzero(~same).flatten()[:8].tolist()} differ from copy 0"


def test_a1_million_nodes_by_replication(gpu_device, monkeypatch):
    """Default shape, 128 copies of one 96 x 96 V1 tile (1.09 M nodes, row capacity 1 179 648), dropout 0, the linear loss's
    per-node weights tiled 128 times: (i) every copy's outputs are bit-identical to copy 0's, (ii) copy 0's are within
    float64_bound of the training-mode oracle on the tile, (iv) a second backward on the same tape is bit-identical, (iii)
    gradient / 128 passes the acceptance rule against the tile's float64 / float32 gradients."""
    B = 128
    sd = _sd(in_channels=7, num_layers=4, seed=61)
    m = _net(sd)
    g, x, ei, ea = _batch([_tile(96, 96, 17)], copies=B)
    n1 = x.shape[0]
    assert g.num_nodes == B * n1 and np.array_equal(g.ptr.numpy(), np.arange(B + 1) * n1)
    assert _ctx().get_option("fused_front") == 1
    w = _loss_weights(n1, 3)
    _dropout(m, 0, 0.0, 0.0)
    m.train(); m.zero_grad(set_to_none=True)
    out = m(g)
    _tape_rows_at_least(m, out, B * 96 * 96)
    _copies_identical(out, B, n1)
    g64, g32, o64, o32 = _oracle_for(m, out, n1, sd, x, ei, ea, None, w, monkeypatch, outputs=True)
    out0 = {k: out[k].detach()[:n1] for k in ("class_logits", "confidence", "correction", "predicted_class")}
    ok, rep = float64_bound(out0, o32, o64, keys=("class_logits", "confidence", "correction"))
    print("[A] copy 0 outputs vs float64:", json.dumps(rep))
    assert ok, rep
    loss = _loss(out, _tiled(w, B))
    loss.backward(retain_graph=True)
    first = {n: p.grad.detach().clone() for n, p in m.named_parameters()}
    m.zero_grad(set_to_none=True)
    loss.backward()
    for n, p in m.named_parameters():
        assert torch.equal(first[n], p.grad), n
    _accept("A", "1.1M nodes, 128 copies", {n: v.double().cpu() for n, v in first.items()}, g64, g32, scale=B)


def test_a2_front_boundary(gpu_device, monkeypatch):
    """8 copies of a 64 x 64 V0 tile: row capacity exactly 32 768, where the W-resident GEMM and the fused front begin.  The taped
    forward's fused-front branch (fused_front 1) and the plain one (0) give bit-identical outputs and gradients, and pass the
    acceptance rule against the tile's oracle."""
    B = 8
    sd = _sd(in_channels=7, num_layers=4, seed=63)
    g, x, ei, ea = _batch([_tile(64, 64, 19, "V0")], copies=B)
    assert x.shape[0] * B == B * 64 * 64 == WRES_MIN_ROWS
    w = _loss_weights(x.shape[0], 3)
    ctx = _ctx()
    assert ctx.get_option("fused_front") == 1 and ctx.get_option("fold_extractor") == 1
    res = {}
    for name, opts in (("front", {}), ("no front", {"fused_front": 0})):
        m = _net(sd)
        _dropout(m, 0, 0.0, 0.0)
        with ctx.options(**opts):
            gr, out = _step(m, g, _tiled(w, B), 0)
            _tape_rows_at_least(m, out, WRES_MIN_ROWS)
        res[name] = (gr, {k: v.detach().cpu() for k, v in out.items()})
        g64, g32 = _oracle_for(m, out, x.shape[0], sd, x, ei, ea, None, w, monkeypatch)
        _accept("A", f"32 768 rows, {name}", gr, g64, g32, scale=B)
    assert ctx.get_option("fused_front") == 1 and ctx.get_option("fold_extractor") == 1
    for k in res["front"][1]:
        assert torch.equal(res["front"][1][k], res["no front"][1][k]), k
    for k in res["front"][0]:
        assert torch.equal(res["front"][0][k], res["no front"][0][k]), k


def test_a2_unfolded_extractor(gpu_device, monkeypatch):
    """The same batch with fold_extractor 0 (the extractor's second Linear and lin_0 as separate GEMMs) passes the acceptance
    rule against the tile's oracle."""
    B = 8
    sd = _sd(in_channels=7, num_layers=4, seed=63)
    g, x, ei, ea = _batch([_tile(64, 64, 19, "V0")], copies=B)
    w = _loss_weights(x.shape[0], 3)
    m = _net(sd)
    _dropout(m, 0, 0.0, 0.0)
    with _ctx().options(fold_extractor=0):
        gr, out = _step(m, g, _tiled(w, B), 0)
        _tape_rows_at_least(m, out, WRES_MIN_ROWS)
    assert _ctx().get_option("fold_extractor") == 1
    g64, g32 = _oracle_for(m, out, x.shape[0], sd, x, ei, ea, None, w, monkeypatch)
    _accept("A", "32 768 rows, unfolded", gr, g64, g32, scale=B)


# ---- B. row capacity far above the node count --------------------------------------------------------------------------------

def _sparse_tiles():
    """Four 128 x 128 tiles (65 536 cells of row capacity) that keep a 24 x 24 window and ~1 % scattered cells: ~3 000 nodes."""
    from bathymetric_gnn_amd import synthetic
    tiles = []
    for i in range(4):
        d, _, _ = _tile(128, 128, 60 + i, "V0")
        valid = np.random.default_rng(70 + i).random((128, 128)) < 0.01
        r0, c0 = 8 + 28 * i, 96 - 24 * i
        valid[r0:r0 + 24, c0:c0 + 24] = True
        tiles.append((np.where(valid, d, synthetic.NODATA).astype(np.float32), valid, None))
    return tiles


SPARSE = {  # name: (state-dict / model keywords, dropout elsewhere, extractor dropout)
    "default, dropout 0": ({}, 0.0, 0.0),
    "default, front + dropout": ({}, 0.1, 0.0),
    "no correction, HT 64": ({"predict_correction": False}, 0.1, 0.1),
    "heads 1": ({"heads": 1}, 0.1, 0.1),
}


@pytest.mark.parametrize("name", list(SPARSE))
def test_b_capacity_far_above_nodes(name, gpu_device, monkeypatch):
    kw, p, p_ext = SPARSE[name]
    sd = _sd(in_channels=7, num_layers=4, seed=65, **kw)
    m = _net(sd, **kw)
    g, x, ei, ea = _batch(_sparse_tiles())
    assert x.shape[0] < 4000
    if p_ext == 0:
        assert _ctx().get_option("fused_front") == 1
    out = _parity("B", name, m, sd, g, x, ei, ea, monkeypatch, p=p, p_ext=p_ext, seed=21)
    _tape_rows_at_least(m, out, 4 * 128 * 128)


# ---- C. the training loss, and losses that reach only some outputs ------------------------------------------------------------

SUBSETS = {"logits": ("logits",), "probs": ("probs",), "confidence": ("confidence",), "correction": ("correction",),
           "full loss": TrainingLoss.FULL}


@pytest.mark.parametrize("subset", list(SUBSETS))
def test_c_output_gradient_subsets(subset, gpu_device, monkeypatch):
    """Only the outputs the loss uses get a gradient (torch passes None for the others, the library NULL); the heads it does not
    reach get exactly 0."""
    sd = _sd(in_channels=7, num_layers=4, seed=67)
    m = _net(sd)
    g, x, ei, ea = _batch([_tile(40, 44, 23), _tile(36, 30, 24)])
    loss = TrainingLoss(x.shape[0], 3, SUBSETS[subset])
    _parity("C", subset, m, sd, g, x, ei, ea, monkeypatch, seed=31, loss=loss)


HEAD_CONFIGS = {  # name: (keywords, uncertainty input)
    "1 class": ({"num_classes": 1}, False),
    "2 classes": ({"num_classes": 2}, False),
    "16 classes": ({"num_classes": 16}, False),
    "no correction": ({"predict_correction": False}, False),
    "in_channels 8": ({"in_channels": 8}, True),
    "hidden 32, no correction": ({"hidden": 32, "predict_correction": False}, False),
}


@pytest.mark.parametrize("name", list(HEAD_CONFIGS))
def test_c_head_configurations(name, gpu_device, monkeypatch):
    kw, unc = HEAD_CONFIGS[name]
    kw = dict(kw)
    ic = kw.pop("in_channels", 7)
    sd = _sd(in_channels=ic, num_layers=3, seed=69, **kw)
    if "hidden" in kw:
        kw["hidden_channels"] = kw.pop("hidden")
    m = _net(sd, in_channels=ic, num_gnn_layers=3, **kw)
    g, x, ei, ea = _batch([_tile(40, 44, 25, unc=unc), _tile(36, 30, 26, unc=unc)])
    assert x.shape[1] == ic
    loss = TrainingLoss(x.shape[0], m.num_classes)
    _parity("C", name, m, sd, g, x, ei, ea, monkeypatch, seed=33, loss=loss)


# ---- D. survey depths ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("band", DEPTH_BANDS)
def test_d_survey_depths(band, gpu_device, monkeypatch):
    """Two tiles at ``band`` metres, dropout 0.1, the training loss (batch statistics: no fitted BatchNorm needed)."""
    sd = _sd(in_channels=7, num_layers=4, seed=71)
    m = _net(sd)
    s = int(-band) % 89
    g, x, ei, ea = _batch([deep_tile(40, 40, s, "V1", band), deep_tile(32, 48, s + 1, "V1", band)])
    _parity("D", f"{band:g} m", m, sd, g, x, ei, ea, monkeypatch, seed=35, loss=TrainingLoss(x.shape[0], 3))


def test_d_sloped_tile_at_depth(gpu_device, monkeypatch):
    """A 5 % ramp at -4000 m: large depth differences and slopes on the edges as well."""
    sd = _sd(in_channels=7, num_layers=4, seed=73)
    m = _net(sd)
    g, x, ei, ea = _batch([deep_tile(48, 48, 9, "V1", -4000.0, slope=0.05)])
    _parity("D", "-4000 m, slope 0.05", m, sd, g, x, ei, ea, monkeypatch, seed=37, loss=TrainingLoss(x.shape[0], 3))


# ---- E. tapes in flight ---------------------------------------------------------------------------------------------------------

def test_e_two_tapes_across_a_validation_forward(gpu_device, monkeypatch):
    """Forward A (stencil batch), forward B (a foreign Data graph of another size), a no_grad eval forward on a third batch, then
    (loss_A + loss_B).backward().  The training forwards move the running statistics, so the model is repacked in between and
    both backward passes run on a freshly packed handle.  Every .grad is the float32 sum of A's and B's gradients computed
    alone on fresh models with the same seeds, bit for bit, and passes the acceptance rule against the oracle's sums."""
    from bathymetric_gnn_amd.data import Data
    sd = _sd(in_channels=7, num_layers=3, seed=75)
    gA, xA, eiA, eaA = _batch([_tile(40, 36, 27)])
    xB, eiB, eaB = _foreign_graph()
    dB = Data(x=torch.from_numpy(xB).cuda(), edge_index=torch.from_numpy(eiB).cuda(), edge_attr=torch.from_numpy(eaB).cuda())
    gC, _, _, _ = _batch([_tile(30, 30, 28)])
    wA, wB = _loss_weights(xA.shape[0], 3, seed=1), _loss_weights(xB.shape[0], 3, seed=2)
    sA, sB = 41, 42

    alone = []
    for data, w, s in ((gA, wA, sA), (dB, wB, sB)):
        m = _net(sd, num_gnn_layers=3)
        _dropout(m, s, 0.1, 0.1)
        alone.append(_step(m, data, w, s)[0])

    m = _net(sd, num_gnn_layers=3)
    _dropout(m, 0, 0.1, 0.1)
    m.train(); m.zero_grad(set_to_none=True)
    m.dropout_seed = sA
    outA = m(gA)
    m.dropout_seed = sB
    outB = m(dB)
    m.eval()
    with torch.no_grad():
        m(gC)
    m.train()
    for out in (outA, outB):
        info = out["class_logits"].grad_fn.info
        ent = (m._native or {}).get(info["key"])
        assert ent is None or ent[1] is not info["handle"], "the model was not repacked: the fallback handle is not exercised"
    (_loss(outA, wA) + _loss(outB, wB)).backward()
    for n, p in m.named_parameters():
        want = (alone[0][n].float() + alone[1][n].float())
        assert torch.equal(p.grad.cpu(), want), n

    oA = _oracle(sd, xA, eiA, eaA, gat_cpu.CounterDropout(sA, 0.1, 0.1, 0.1, 0.1), wA, monkeypatch)
    oB = _oracle(sd, xB, eiB, eaB, gat_cpu.CounterDropout(sB, 0.1, 0.1, 0.1, 0.1), wB, monkeypatch)
    g64 = {k: oA[0][k] + oB[0][k] for k in oA[0]}
    g32 = {k: oA[1][k] + oB[1][k] for k in oA[1]}
    _accept("E", "A + B across a repack", {n: p.grad.double().cpu() for n, p in m.named_parameters()}, g64, g32)


# ---- F. edge graphs -------------------------------------------------------------------------------------------------------------

def _masked(h, w, valid, seed=29):
    from bathymetric_gnn_amd import synthetic
    d, _, _ = _tile(h, w, seed, "V0")
    return np.where(valid, d, synthetic.NODATA).astype(np.float32), valid, None


def test_f_two_node_batch(gpu_device, monkeypatch):
    """The smallest batch BatchNorm trains on: two neighbouring cells."""
    valid = np.zeros((8, 8), bool)
    valid[3, 3:5] = True
    sd = _sd(in_channels=7, num_layers=4, seed=77)
    m = _net(sd)
    g, x, ei, ea = _batch([_masked(8, 8, valid)])
    assert x.shape[0] == 2 == g.num_nodes
    _parity("F", "2 nodes", m, sd, g, x, ei, ea, monkeypatch, p=0.0, seed=39)


def test_f_self_loops_only(gpu_device, monkeypatch):
    """A checkerboard under 4-connectivity: no node has a neighbour, every edge is a self loop (the target kernel's deg == 0
    self-attribute)."""
    r, c = np.indices((24, 24))
    valid = (r + c) % 2 == 0
    sd = _sd(in_channels=7, num_layers=4, seed=79)
    m = _net(sd)
    g, x, ei, ea = _batch([_masked(24, 24, valid)], conn="4-connected")
    assert x.shape[0] == 288 and (ei[0] == ei[1]).all()
    _parity("F", "self loops only", m, sd, g, x, ei, ea, monkeypatch, seed=43)


def test_f_empty_batch(gpu_device):
    """Tiles without a valid cell: the training forward returns empty outputs, and backward() raises nothing and leaves every
    gradient 0."""
    sd = _sd(in_channels=7, num_layers=4, seed=81)
    m = _net(sd)
    _set_dropout(m, 0.1)
    g, x, _, _ = _batch([_masked(16, 16, np.zeros((16, 16), bool)), _masked(12, 20, np.zeros((12, 20), bool))])
    assert x.shape[0] == 0 == g.num_nodes
    m.train(); m.dropout_seed = 3
    out = m(g)
    assert all(v.shape[0] == 0 for v in out.values())
    assert out["class_logits"].grad_fn is not None
    _loss(out, _loss_weights(0, 3)).backward()
    for n, p in m.named_parameters():
        assert p.grad is not None and not torch.count_nonzero(p.grad), n
