"""Foreign ``Data`` graphs (x / edge_index / edge_attr assembled elsewhere) at the sizes where their own route through the library
changes form, forward and backward against the float64 oracle.

The route: ``bgnn_graph_from_edges`` builds a CSR by target (graph_build.hip ``launch_generic_build``: degree count with integer
atomics, multi-block prefix scan into rowptr, atomic-cursor fill, per-row insertion sort by edge id, attribute gather); the
forward runs the CSR branches of ``gat_aggregate_kernel`` / ``neighbor_reduce_kernel``; the backward builds a transposed index
(gat_backward.hip ``ensure_transposed_index``: tr_count / tr_scan / tr_fill / tr_sort) and runs the CSR branches of
``gat_bwd_target_kernel`` / ``gat_bwd_source_kernel`` / ``plain_bwd_aggregate_kernel``.  No fused or tiled stencil kernel is on
it.  The other tests that reach it use N = 300, E ~ 1 500 and a 40-edge hub; the graphs here (``_foreign_graphs.foreign_graph``)
have rows of exactly 15 / 16 / 17 / 32 / 33 in-edges, a hub of 1 000 in-edges, a node of 1 000 out-edges, parallel edges, explicit
self loops, isolated nodes, and their edge array in random order.

S1  N = 2 049: the rowptr scan runs two SCAN_CHUNKs (scan_apply_rowptr_kernel adds a non-zero block offset, the spine sees two
    blocks); tr_scan_kernel runs with seg = 3 (threads 683 .. 1 023 have empty segments, thread 682 a clipped one).
S2  N = 33 025 (32 768 + 257), E ~ 8 N: row capacity above WRES_MIN_ROWS (the W-resident GEMM form, forward and backward), 17 scan
    chunks with rows of 16 / 17 / 33 edges at ids 2 047 / 2 048 / 2 049, wgrad / colsum / BatchNorm reductions over ~130 chunks.
S3  32 disjoint copies of the S2 graph, their edge lists interleaved at random (1 056 800 nodes, 8.5 M edges): more rows than
    256 x 16 x the multiprocessor count, so the grid-stride loops of tr_count / tr_fill / tr_sort take a second trip on their
    rowptr form, and the reductions run at their 1 024-chunk cap.
Rows of 15 / 16 (register array) and 17 / 32 / 33 / 1 000 edges (three-pass loop, AGG_MAXDEG = 16) are in every one of them, and
so are the 1 000-entry lists both one-thread insertion sorts order (generic_sort_rows_kernel by edge id, tr_sort_kernel by slot).

Acceptance rules, unchanged: forward ``_conditioning.float64_bound`` (BOUND_C = 4, BOUND_FLOOR = 1e-6); gradients
``test_gpu_backward_training._accept`` (BOUND_C, FLOOR_REL = 1e-5; a parameter the loss does not reach is exactly 0; the oracle runs
with the kernels' ReLU patterns, and every disagreement with float64's signs lies within BOUND_C x the float32 oracle's distance
of 0).  Every distance is printed, the largest ratios per group at the end of the module.

LeakyReLU sides.  The attention logit's LeakyReLU has ReLU's kink (slope 1 | 0.2), and an S2 graph has ~3 M logits: the S2 GAT step
(dropout seed 53) has one, edge 49 -> 29 255, head 0 of layer 1, at -4.8e-8 in float64 (0.003 x the rounding bound) that the kernels'
float32 sum puts on the positive side.  Against the oracle with float64's own side the step misses the rule (worst d / bound 4.5:
convs.1.att_src / att_dst off by 1.3e-2 where float32 is off by 9e-5, everything below layer 1 with them, layer 2 and the heads on
the yardstick); with the kernels' side it passes at 0.049.  So the GAT oracle here takes the kernels' LeakyReLU sides as it takes
their ReLU patterns (``_KernelSides``: recomputed from the attention dots on the tape), under the same rule: a side may differ from
float64's only within BOUND_C x the float32 oracle's distance of 0.  Nothing in the kernels was wrong.

Measured on an MI355X (worst d / float32 where the yardstick term dominates the bound | worst d / bound):
    gradients  S1 0 (the floor dominates everywhere) | 0.036   S2 0.18 | 0.049   S3 0.077 | 0.077   edges 0.99 | 0.22
    forward    S1 1.42 | 0.27   S2 2.65 (GCN) | 0.46   E = 0 1.13 | 0.16
    graph build / first backward (transposed index included), wall time:
               S2 GAT 29 ms / 71 ms, GraphSAGE 30 ms / 114 ms, GIN 23 ms / 57 ms;  S3 GAT 6.4 ms / 139 ms, GIN 5.6 ms / 98 ms
    (the 1 000-entry insertion sorts do not show: the module's 28 tests take 26 s, the float64 oracle most of it).
"""
import functools
import json
import time

import numpy as np
import pytest
import torch

from _calibration import calibrate_heads
from _conditioning import BOUND_C, BOUND_FLOOR, float64_bound
from _foreign_graphs import foreign_graph, in_degree, keep_target_order, pinned, replicate
from oracle import gat_cpu
from test_gpu_backward import _loss, _loss_weights, _model, oracle_grads
from test_gpu_backward_plain import EPS32
from test_gpu_backward_plain import _drop as _plain_dropout
from test_gpu_backward_plain import _oracle as _plain_oracle
from test_gpu_backward_plain import _parity as _plain_parity
from test_gpu_backward_plain import _plain_tape
from test_gpu_backward_training import WORST, WRES_MIN_ROWS, _accept, _copies_identical, _dropout, _KernelReLU, _step, _tape_relu_patterns, \
    _tape_rows_at_least, _tape_tables, _tiled

pytestmark = pytest.mark.gpu
S1_N = 2049
S2_N = WRES_MIN_ROWS + 257
S3_COPIES = 32
SIZES = {"S1": S1_N, "S2": S2_N}
FWD_WORST = {}                  # group -> (largest dist / float32's where the yardstick dominates, largest dist / bound)


@pytest.fixture(scope="module", autouse=True)
def _print_worst():
    yield
    grads = {k: {"d_over_f32": v[0], "d_over_bound": v[1]} for k, v in sorted(WORST.items()) if k.startswith("foreign")}
    fwd = {k: {"d_over_f32": v[0], "d_over_bound": v[1]} for k, v in sorted(FWD_WORST.items())}
    print("\nforeign graphs, worst per group: gradients", json.dumps(grads), "forward", json.dumps(fwd))


@functools.lru_cache(maxsize=None)
def _graph(N, loops, long_lists=1000):
    return foreign_graph(N, 8, seed=N % 97, self_loops=loops, long_lists=long_lists)


def _data(x, ei, ea):
    from bathymetric_gnn_amd.data import Data
    return Data(x=torch.from_numpy(x).cuda(), edge_index=torch.from_numpy(ei).cuda(), edge_attr=torch.from_numpy(ea).cuda())


def _sd(kind="GAT", **kw):
    from bathymetric_gnn_amd import synthetic
    kw.setdefault("num_layers", 3)
    return synthetic.synthetic_state_dict(in_channels=7, gnn_type=kind, **kw)


def _net(sd, kind="GAT", layers=3, **kw):
    return _model(sd, torch.device("cuda:0"), in_channels=7, edge_dim=3, gnn_type=kind, num_gnn_layers=layers, **kw)


def _sync():
    torch.cuda.synchronize()
    return time.perf_counter()


def _build_seconds(m, data):
    """Wall time of one ``bgnn_graph_from_edges`` on ``data`` (it returns after the build has finished on the device)."""
    from bathymetric_gnn_amd import runtime as rt
    t0 = _sync()
    g, keep = m._graph_of(data, rt.get_context(torch.device("cuda:0")))
    dt = _sync() - t0
    del g, keep
    return dt


def _eval_forward(group, name, m, data, sd, x, ei, ea, mixed=True):
    """An eval-mode forward (backbone output included) against the float32 and float64 oracle under float64_bound."""
    m.eval()
    with torch.no_grad():
        out = m._run(data, 0.85, 0.6, with_flags=False, want_hidden=True)
    assert all(torch.isfinite(v).all() for v in out.values() if v.is_floating_point())
    ref32 = gat_cpu.forward(sd, x, ei, ea)
    ref64 = gat_cpu.forward(sd, x, ei, ea, dtype=torch.float64)
    if mixed:
        assert torch.unique(ref64["predicted_class"]).numel() >= 2, "one class everywhere: the class comparison would be vacuous"
    ok, rep = float64_bound(out, ref32, ref64)
    r_f32 = max([v["dist"] / v["float32_dist"] for v in rep.values()
                 if isinstance(v, dict) and v["float32_dist"] > 0 and BOUND_C * v["float32_dist"] >= BOUND_FLOOR] + [0.0])
    r_bound = max(v["dist"] / v["bound"] for v in rep.values() if isinstance(v, dict))
    print(f"[{group}] {name}: worst d/f32 {r_f32:.3f}, worst d/bound {r_bound:.3f}", json.dumps(rep))
    w = FWD_WORST.get(group, (0.0, 0.0))
    FWD_WORST[group] = (max(w[0], r_f32), max(w[1], r_bound))
    assert ok, (name, rep)
    return out, ref32, ref64


class _KernelSides(_KernelReLU):
    """``_KernelReLU`` whose LeakyReLUs -- one per GAT layer, on the [edges + N self loops][heads] attention logits -- take the
    kernels' sides as its ReLUs take the kernels' patterns.  LeakyReLU's derivative jumps at 0 (1 | 0.2) as ReLU's does, and a graph
    of S2's size has ~3 M attention logits: now and then one lies within float32 rounding of 0, the kernels (which add the
    attention dots in their own order) take the other side than float64, and that edge's whole share of the gradient moves.
    ``sides``: per layer (side, known) -- the sign of the kernels' own logit, and where it is known beyond rounding; elsewhere the
    oracle keeps its own sign."""

    def __init__(self, patterns, sides):
        super().__init__(patterns)
        self.sides, self.logits, self.j = sides, [], 0

    def leaky_relu(self, v, slope):
        side, known = self.sides[self.j]
        self.j += 1
        self.logits.append(v.detach())
        return torch.where(torch.where(known, side, v > 0), v, slope * v)

    @staticmethod
    def check(f64, f32):
        """The rule of ``_KernelReLU.check`` for the logits: every logit whose kernel side disagrees with float64's sign lies within
        BOUND_C x the float32 oracle's distance to float64 (over that layer's logits) of 0.  Returns (disagreements, largest
        |v| / bound)."""
        assert f64.j == f32.j == len(f64.sides), (f64.j, f32.j, len(f64.sides))
        n_bad, worst = 0, 0.0
        for v64, v32, (side, known) in zip(f64.logits, f32.logits, f64.sides):
            off = known & (side != (v64 > 0))
            if off.any():
                bound = BOUND_C * (v32.double() - v64).abs().max().item()
                n_bad += int(off.sum())
                worst = max(worst, v64[off].abs().max().item() / bound)
        assert worst <= 1.0, f"an attention logit {worst:.2f} x the rounding bound away from 0 takes the other side on the GPU"
        return n_bad, worst


def _attention_sides(m, out, n, sd, ei, ea):
    """Per GAT layer, the sides of the kernels' attention logits in the oracle's edge order (the edges without explicit self loops,
    then the N added self loops): the logit recomputed in float64 from the kernels' own attention dots on the tape (asd: a_src |
    a_dst per node and head), the edge attributes and V = att_edge . lin_edge (float32, as the library packs it) -- and ``known``
    where it is further from 0 than the float32 rounding of the kernels' three additions and their edge dot product (for a self
    loop also that of the mean of up to 1 000 attributes)."""
    tape, _, _, t = _tape_tables(m, out)
    hid = m.hidden_channels
    src, dst = torch.as_tensor(ei[0]), torch.as_tensor(ei[1])
    keep = src != dst
    src, dst, e = src[keep], dst[keep], torch.as_tensor(ea).double()[keep]
    ED = e.shape[1]
    cnt = torch.zeros(n, dtype=torch.float64).index_add_(0, dst, torch.ones(dst.shape[0], dtype=torch.float64))
    loop = torch.zeros(n, ED, dtype=torch.float64).index_add_(0, dst, e) / cnt.clamp(min=1).unsqueeze(-1)
    loop_abs = torch.zeros(n, ED, dtype=torch.float64).index_add_(0, dst, e.abs()) / cnt.clamp(min=1).unsqueeze(-1)
    ar = torch.arange(n)
    src2, dst2, e2 = torch.cat([src, ar]), torch.cat([dst, ar]), torch.cat([e, loop])
    e2_abs = torch.cat([e.abs(), loop_abs * (cnt + 2).unsqueeze(-1)])
    sides = []
    for l, c in enumerate(m.gnn.convs):
        H = c.heads
        off = t[("asd", l)]
        asd = tape[off:off + n * 2 * H * 4].view(torch.float32).view(n, 2 * H).cpu().double()
        att_edge = torch.as_tensor(np.asarray(sd[f"gnn.convs.{l}.att_edge"]), dtype=torch.float64).reshape(H, hid, 1)
        W_e = torch.as_tensor(np.asarray(sd[f"gnn.convs.{l}.lin_edge.weight"]), dtype=torch.float64).reshape(H, hid, ED)
        V = (att_edge * W_e).sum(1).float().double()                     # [H][ED]
        a_s, a_d = asd[:, :H].index_select(0, src2), asd[:, H:].index_select(0, dst2)
        pre = a_s + a_d + e2 @ V.t()
        rnd = 4 * EPS32 * (a_s.abs() + a_d.abs() + e2_abs @ V.abs().t())
        side, known = pre > 0, pre.abs() > rnd
        e32, asd32, V32 = np.asarray(ea, np.float32)[keep.numpy()], asd.numpy().astype(np.float32), V.numpy().astype(np.float32)
        for k, h in torch.nonzero(~known).tolist()[:64]:     # (a handful at most: the kernels' float32 arithmetic redone for them)
            i, j = int(dst2[k]), int(src2[k])
            rows = np.flatnonzero(dst.numpy() == i) if k >= src.shape[0] else None
            lg = _kernel_logit(asd32[j, h], asd32[i, H + h], V32[h], e32[k] if rows is None else e32[rows], rows is not None)
            if lg is not None:
                side[k, h], known[k, h] = bool(lg > 0), True
        sides.append((side, known))
    return sides


def _kernel_logit(a_s, a_d, v, e, is_loop):
    """An attention logit as gat_aggregate_kernel / gat_bwd_target_kernel compute it, in float32 operation by operation:
    (a_src + a_dst) + dot, dot = sum_f e_f v_f accumulated from 0; for a node's added self loop (``e``: its row's attributes in
    edge-id order) e = (their running float32 sum) / count.  The compiler may contract the dot's multiply-adds into fused ones:
    both forms are computed, and None is returned where their signs differ or a logit is exactly 0 (the side stays the oracle's)."""
    f32, f64 = np.float32, np.float64
    if is_loop:
        tot = np.zeros(v.shape[0], f32)
        for row in e:
            tot = (tot + row).astype(f32)
        e = (tot / f32(max(len(e), 1))).astype(f32)
    base = f32(a_s + a_d)
    plain = fused = f32(0.0)
    for ef, vf in zip(e, v):
        plain = f32(plain + f32(ef * vf))
        fused = f32(f64(ef) * f64(vf) + f64(fused))
    lg = [f32(base + plain), f32(base + fused)]
    if lg[0] == 0 or lg[1] == 0 or (lg[0] > 0) != (lg[1] > 0):
        return None
    return lg[0]


def _gat_oracle(m, out, n, sd, x, ei, ea, drop, w, monkeypatch):
    """float64 / float32 oracle gradients of the GAT model with the kernels' ReLU patterns (``_tape_relu_patterns``) and the
    kernels' LeakyReLU sides (``_attention_sides``); both kinds of disagreement with float64's own signs are checked and printed."""
    pats, sides = _tape_relu_patterns(m, out, n), _attention_sides(m, out, n, sd, ei, ea)
    f64, f32 = _KernelSides(pats, sides), _KernelSides(pats, sides)
    g64, _ = oracle_grads(sd, x, ei, ea, torch.float64, drop, w, monkeypatch, functional=f64)
    g32, _ = oracle_grads(sd, x, ei, ea, torch.float32, drop, w, monkeypatch, functional=f32)
    n_relu, w_relu = _KernelReLU.check(f64, f32, drop, m.hidden_channels, 3 if m.predict_correction else 2)
    n_leaky, w_leaky = _KernelSides.check(f64, f32)
    unknown = sum(int((~k).sum()) for _, k in sides)
    print(f"  on the other side of 0 on the GPU: {n_relu} ReLU inputs (largest |v| {w_relu:.3f} x the rounding bound), {n_leaky} attention "
          f"logits (largest |v| {w_leaky:.3f} x the rounding bound; {unknown} logits within the kernels' own rounding of 0)")
    return g64, g32


def _gat_parity(group, name, m, sd, data, x, ei, ea, monkeypatch, p, seed):
    """``test_gpu_backward_training._parity`` with ``_gat_oracle``: one training step under the acceptance rule; returns the outputs."""
    drop = _dropout(m, seed, p, p)
    w = _loss_weights(x.shape[0], m.num_classes)
    g_gpu, out = _step(m, data, w, seed)
    g64, g32 = _gat_oracle(m, out, x.shape[0], sd, x, ei, ea, drop, w, monkeypatch)
    _accept(group, name, g_gpu, g64, g32)
    return out


def _assert_same(a, b, what):
    assert set(a) == set(b)
    for k in a:
        assert torch.equal(a[k], b[k]), f"{what}: {k} differs"


# ---- S1: two scan chunks, tr_scan with seg = 3 ---------------------------------------------------------------------------------

@pytest.mark.parametrize("p", [0.0, 0.1])
def test_s1_gat_training_step(p, gpu_device, monkeypatch):
    """N = 2 049, self loops included, 3 layers: the rowptr scan's second chunk and its spine over two blocks, tr_scan_kernel with
    seg = 3, rows of 15 / 16 | 17 / 32 / 33 / 1 000 in-edges on both sides of AGG_MAXDEG in the target kernel, the 1 000-entry
    out-list in the source kernel."""
    x, ei, ea = _graph(S1_N, True)
    assert -(-S1_N // 2048) == 2 and -(-S1_N // 1024) == 3
    sd = _sd(seed=201)
    m = _net(sd)
    _gat_parity("foreign S1", f"GAT p{p}", m, sd, _data(x, ei, ea), x, ei, ea, monkeypatch, p=p, seed=51)


@pytest.mark.parametrize("kind", ["GAT", "GCN", "GraphSAGE", "GIN"])
def test_s1_eval_forward(kind, gpu_device):
    """N = 2 049, the CSR branches of gat_aggregate_kernel (GAT) and neighbor_reduce_kernel (the others) over rows of 0 .. 1 000
    edges built by a two-chunk rowptr scan; heads calibrated so that classes mix.  GraphSAGE / GIN refuse explicit self loops."""
    x, ei, ea = _graph(S1_N, kind in ("GAT", "GCN"))
    sd = calibrate_heads(_sd(kind, seed=203), x, ei, ea)
    m = _net(sd, kind)
    _eval_forward("foreign S1", kind, m, _data(x, ei, ea), sd, x, ei, ea)


def test_s1_wide_gat_eval_forward(gpu_device):
    """heads 8 x hidden 64 = 512 columns on N = 2 049: the CSR aggregate runs as two 256-column launches, the second with
    hd0 = 4 (its heads' logits read at an offset into the layer's shared attention table), in layers 0 and 1 (the last layer has
    one head).  Eval forward only: the backward refuses more than 256 columns."""
    x, ei, ea = _graph(S1_N, True)
    sd = calibrate_heads(_sd(heads=8, hidden=64, seed=205), x, ei, ea)
    m = _net(sd, heads=8, hidden_channels=64)
    assert [c.heads * m.hidden_channels for c in m.gnn.convs] == [512, 512, 64]
    _eval_forward("foreign S1", "GAT 8 x 64", m, _data(x, ei, ea), sd, x, ei, ea)


# ---- S2: row capacity above the W-resident threshold -----------------------------------------------------------------------------

@pytest.mark.parametrize("kind", ["GAT", "GraphSAGE", "GIN"])
def test_s2_training_step(kind, gpu_device, monkeypatch):
    """N = 33 025, E ~ 266 000, dropout 0.1, 3 layers of the default widths: 33 025 rows of capacity (>= 32 768: the W-resident
    GEMM form in forward and backward), a 17-chunk rowptr scan with rows of 16 / 17 / 33 edges at ids 2 047 / 2 048 / 2 049,
    tr_scan_kernel with seg = 33, wgrad / colsum / BatchNorm reductions over ~130 chunks of 256 rows, both 1 000-entry lists.
    GraphSAGE / GIN: ``test_gpu_backward_plain``'s pattern-aware oracle, no self loops.  Prints the wall time of the graph build
    and of the first backward (which builds the transposed index)."""
    gat = kind == "GAT"
    x, ei, ea = _graph(S2_N, gat)
    assert x.shape[0] > WRES_MIN_ROWS and -(-S2_N // 2048) == 17 and {2047, 2048, 2049} <= set(pinned(S2_N))
    sd = _sd(kind, seed=207)
    m = _net(sd, kind)
    data = _data(x, ei, ea)
    if gat:
        out = _gat_parity("foreign S2", "GAT p0.1", m, sd, data, x, ei, ea, monkeypatch, p=0.1, seed=53)
        _tape_rows_at_least(m, out, S2_N)
    else:
        _, out = _plain_parity("foreign S2", f"{kind} p0.1", m, sd, data, x, ei, ea, monkeypatch, 0.1, seed=53)
        assert _plain_tape(m, out)[1] >= S2_N
    t_build = _build_seconds(m, data)
    m.zero_grad(set_to_none=True)
    loss = _loss(m(data), _loss_weights(S2_N, 3))
    t0 = _sync()
    loss.backward()
    print(f"[foreign S2] {kind}: graph build {t_build * 1e3:.1f} ms, first backward {(_sync() - t0) * 1e3:.1f} ms")


def test_s2_gcn_eval_forward(gpu_device):
    """GCN has no backward: its eval forward at N = 33 025 (neighbor_reduce_kernel's CSR branch over the 17-chunk rowptr, the
    W-resident GEMM form)."""
    x, ei, ea = _graph(S2_N, True)
    sd = calibrate_heads(_sd("GCN", seed=209), x, ei, ea)
    m = _net(sd, "GCN")
    _eval_forward("foreign S2", "GCN", m, _data(x, ei, ea), sd, x, ei, ea)


# ---- S3: a million rows by replication ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", ["GAT", "GIN"])
def test_s3_million_rows_by_replication(kind, gpu_device, monkeypatch):
    """32 disjoint copies of the S2 graph (no self loops) as ONE foreign graph of 1 056 800 nodes and 8.5 M edges, the copies' edge
    lists merged by a random interleave that keeps each copy's order, dropout 0, the per-node loss weights tiled.  Rows exceed
    256 x 16 x the multiprocessor count, so tr_count / tr_fill / tr_sort take a second grid-stride trip on their rowptr form; the
    rowptr scan runs 517 chunks; wgrad / colsum / BatchNorm run at their 1 024-chunk cap.  (i) every copy's outputs equal copy 0's
    bit for bit (each row sorted into copy 0's order whatever the atomics' arrival order), (ii) gradient / 32 passes the
    acceptance rule against ONE copy's float64 / float32 gradients, (iii) a second backward on the tape is bit-identical."""
    B = S3_COPIES
    x1, ei1, ea1 = _graph(S2_N, False)
    n1, rows = x1.shape[0], B * x1.shape[0]
    num_cus = torch.cuda.get_device_properties(0).multi_processor_count
    if rows <= 256 * 16 * num_cus:
        pytest.skip(f"{rows} rows fit one trip of a {16 * num_cus}-block grid: the grid-stride branch would not run on this device")
    free, _ = torch.cuda.mem_get_info()
    if free < 64 << 30:
        pytest.skip(f"{free >> 30} GiB of device memory free: the {rows}-row tape and its backward need more; the grid-stride "
                    "branch is not exercised")
    x, ei, ea = replicate(x1, ei1, ea1, B, seed=11)
    assert x.shape[0] == rows == 1056800 and ei.shape[1] == B * ei1.shape[1]
    data = _data(x, ei, ea)
    del x, ei, ea
    sd = _sd(kind, seed=211)
    m = _net(sd, kind)
    w = _loss_weights(n1, 3)
    (_dropout if kind == "GAT" else _plain_dropout)(m, 0, 0.0, 0.0)
    t_build = _build_seconds(m, data)
    m.train(); m.zero_grad(set_to_none=True)
    out = m(data)
    if kind == "GAT":
        _tape_rows_at_least(m, out, rows)
    else:
        assert _plain_tape(m, out)[1] >= rows
    _copies_identical(out, B, n1)
    loss = _loss(out, _tiled(w, B))
    t0 = _sync()
    loss.backward(retain_graph=True)
    t_bwd = _sync() - t0
    print(f"[foreign S3] {kind}: graph build {t_build * 1e3:.1f} ms, first backward {t_bwd * 1e3:.1f} ms")
    first = {n: p.grad.detach().clone() for n, p in m.named_parameters()}
    m.zero_grad(set_to_none=True)
    loss.backward()
    for n, p in m.named_parameters():
        assert torch.equal(first[n], p.grad), n
    if kind == "GAT":
        g64, g32 = _gat_oracle(m, out, n1, sd, x1, ei1, ea1, None, w, monkeypatch)
    else:
        g64, g32 = _plain_oracle(m, out, n1, sd, x1, ei1, ea1, None, w, monkeypatch)
    _accept("foreign S3", f"{kind} {rows} rows, {B} copies", {n: v.double().cpu() for n, v in first.items()}, g64, g32, scale=B)


# ---- properties that need no oracle ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", ["GAT", "GraphSAGE"])
@pytest.mark.parametrize("size", list(SIZES))
def test_determinism_under_contention(size, kind, gpu_device):
    """The same Data built twice: the degree count and the cursor fill run their atomics in another arrival order each time (1 000
    edges contend for the hub's cursor, their ids spread over the whole edge array), and the row sort by edge id removes it.  Two
    predictions are bit-identical; two training steps, each on a freshly built graph and transposed index (tr_fill's cursors,
    tr_sort), give bit-identical gradients."""
    x, ei, ea = _graph(SIZES[size], kind == "GAT")
    sd = _sd(kind, seed=213)
    m = _net(sd, kind)
    a, b = m.predict(_data(x, ei, ea)), m.predict(_data(x, ei, ea))
    _assert_same(a, b, "two predictions")
    (_dropout if kind == "GAT" else _plain_dropout)(m, 9, 0.1, 0.1)
    w = _loss_weights(x.shape[0], 3)
    g1, _ = _step(m, _data(x, ei, ea), w, 9)
    g2, _ = _step(m, _data(x, ei, ea), w, 9)
    assert torch.count_nonzero(g1["feature_extractor.mlp.0.weight"])
    _assert_same(g1, g2, "two training steps")


@pytest.mark.parametrize("kind", ["GAT", "GCN", "GIN"])
@pytest.mark.parametrize("size", list(SIZES))
def test_order_invariance_within_targets(size, kind, gpu_device):
    """The edge array re-ordered by a permutation that keeps the relative order of edges sharing a target: every CSR row, sorted by
    edge id, is the same list, so the eval outputs are bit-identical -- and, for GAT, so are a training step's gradients (the
    transposed index orders out-edges by CSR slot, which has not moved either)."""
    loops = kind in ("GAT", "GCN")
    x, ei, ea = _graph(SIZES[size], loops)
    perm = keep_target_order(ei, seed=5)
    ei2, ea2 = np.ascontiguousarray(ei[:, perm]), np.ascontiguousarray(ea[perm])
    m = _net(_sd(kind, seed=215), kind)
    _assert_same(m.predict(_data(x, ei, ea)), m.predict(_data(x, ei2, ea2)), "re-ordered edge array")
    if kind == "GAT":
        _dropout(m, 13, 0.1, 0.1)
        w = _loss_weights(x.shape[0], 3)
        g1, _ = _step(m, _data(x, ei, ea), w, 13)
        g2, _ = _step(m, _data(x, ei2, ea2), w, 13)
        _assert_same(g1, g2, "re-ordered edge array, gradients")


@pytest.mark.parametrize("size", list(SIZES))
def test_arbitrary_edge_order_stays_within_the_bound(size, gpu_device):
    """An arbitrary permutation of the edge array changes every row's summation order: the GAT eval forward stays within
    float64_bound of the oracle run on that order."""
    x, ei, ea = _graph(SIZES[size], True)
    perm = np.random.default_rng(7).permutation(ei.shape[1])
    ei2, ea2 = np.ascontiguousarray(ei[:, perm]), np.ascontiguousarray(ea[perm])
    assert np.array_equal(in_degree(ei2, x.shape[0]), in_degree(ei, x.shape[0]))
    sd = calibrate_heads(_sd(seed=217), x, ei2, ea2)
    m = _net(sd)
    _eval_forward(f"foreign {size}", "GAT, edges permuted", m, _data(x, ei2, ea2), sd, x, ei2, ea2)


# ---- edges of the route -----------------------------------------------------------------------------------------------------------

def test_no_edges(gpu_device, monkeypatch):
    """N = 50, E = 0: the build skips its edge kernels (rowptr all 0), every softmax is the self loop alone with a zero
    self-attribute, every out-list is empty.  Eval forward and a training step against the oracle."""
    rng = np.random.default_rng(21)
    x = rng.standard_normal((50, 7)).astype(np.float32)
    ei, ea = np.zeros((2, 0), np.int64), np.zeros((0, 3), np.float32)
    sd = _sd(seed=219)
    m = _net(sd)
    out, _, _ = _eval_forward("foreign edges", "E = 0", m, _data(x, ei, ea), sd, x, ei, ea, mixed=False)
    assert out["class_logits"].shape == (50, 3)
    _gat_parity("foreign edges", "E = 0", m, sd, _data(x, ei, ea), x, ei, ea, monkeypatch, p=0.1, seed=55)


def test_two_nodes_one_edge(gpu_device, monkeypatch):
    """N = 2, E = 1 (0 -> 1): the smallest batch BatchNorm trains on; node 0 has one out-edge and no in-edge, node 1 the reverse."""
    rng = np.random.default_rng(23)
    x = rng.standard_normal((2, 7)).astype(np.float32)
    ei, ea = np.array([[0], [1]], np.int64), rng.standard_normal((1, 3)).astype(np.float32)
    sd = _sd(seed=221)
    m = _net(sd)
    _gat_parity("foreign edges", "N = 2, E = 1", m, sd, _data(x, ei, ea), x, ei, ea, monkeypatch, p=0.0, seed=57)


def test_edge_index_views_and_host_tensors(gpu_device):
    """edge_index as a non-contiguous view (the transpose of an [E, 2] pair list, and every second column of a wider tensor) and
    as a CPU tensor next to device x / edge_attr: predictions and a training step's gradients equal those of the contiguous
    device tensor bit for bit."""
    from bathymetric_gnn_amd.data import Data
    x, ei, ea = _graph(300, True, 100)
    m = _net(_sd(seed=223))
    xd, ead = torch.from_numpy(x).cuda(), torch.from_numpy(ea).cuda()
    pairs = torch.from_numpy(np.ascontiguousarray(ei.T)).cuda()
    wide = torch.zeros((2, 2 * ei.shape[1]), dtype=torch.int64, device="cuda")
    wide[:, ::2] = torch.from_numpy(ei).cuda()
    forms = {"contiguous": torch.from_numpy(ei).cuda(), "transposed view": pairs.t(), "strided view": wide[:, ::2],
             "host tensor": torch.from_numpy(ei)}
    assert not forms["transposed view"].is_contiguous() and not forms["strided view"].is_contiguous()
    assert forms["host tensor"].device.type == "cpu"
    w = _loss_weights(300, 3)
    data = {name: Data(x=xd, edge_index=e, edge_attr=ead) for name, e in forms.items()}
    pred = {name: m.predict(d) for name, d in data.items()}      # (before any training step moves the running statistics)
    _dropout(m, 17, 0.1, 0.1)
    grads = {name: _step(m, d, w, 17)[0] for name, d in data.items()}
    for name in forms:
        _assert_same(pred["contiguous"], pred[name], name)
        _assert_same(grads["contiguous"], grads[name], name + ", gradients")
