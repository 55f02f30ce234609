"""Context option fused_light_form: the exact-f32 fused GAT launches with a narrow next stage in their light form (half-slab image,
head-pair coefficient table, four workgroups per CU) against the full-slab instances (option 0).  Same additions and the same k order per
accumulator: the grids must agree bit for bit; one case is held against the CPU oracle so that both forms cannot be wrong together."""
import numpy as np
import pytest
import torch

from oracle import gat_cpu, graph_cpu

gpu = pytest.mark.gpu
TOL = 1e-4


def _model(sd, in_channels=7, num_layers=4, heads=4, hidden=64, gnn_type="GAT"):
    from bathymetric_gnn_amd.models import BathymetricGNN
    m = BathymetricGNN(in_channels=in_channels, hidden_channels=hidden, num_gnn_layers=num_layers, heads=heads, gnn_type=gnn_type,
                       edge_dim=3, dropout=0.0)
    m.load_state_dict({k: torch.as_tensor(v) for k, v in sd.items()})
    return m.to(torch.device("cuda:0")).eval()


def _ctx(gpu_device):
    from bathymetric_gnn_amd import runtime as rt
    return rt.get_context(gpu_device)


@pytest.fixture(autouse=True)
def _restore_options():
    yield
    if not torch.cuda.is_available():
        return
    c = _ctx(torch.device("cuda:0"))
    c.set_option("fused_light_form", 1); c.set_option("matrix_path", "exact_f32"); c.set_option("ragged_atlas", 1)


def _both_forms(gpu_device, run):
    """run() -> (grids [3, cells], n_nodes) with the option at 1 and at 0"""
    c = _ctx(gpu_device)
    assert c.get_option("fused_light_form") == 1, "the light form is the default"
    out = {}
    for v in (1, 0):
        c.set_option("fused_light_form", v)
        out[v] = run()
    c.set_option("fused_light_form", 1)
    return out[1], out[0]


def _assert_same(a, b):
    assert int(a[1]) == int(b[1])
    for k in range(3):
        assert torch.equal(a[0][k], b[0][k]), ("classification", "confidence", "correction")[k]


def _runner(eng, gb, depth, mask, res=(0.5, 1.0), unc=None):
    hw, r, d, m, u = gb.upload_tiles(depth, mask, unc, [res] * len(depth))

    def run():
        nn = torch.zeros(1, dtype=torch.int64, device="cuda")
        o = eng.infer_device(hw, r, d, m, u, n_nodes_out=nn).clone()
        return o, int(nn.item())
    return run


def _uniform_holes():
    from bathymetric_gnn_amd import synthetic
    depth, mask, _ = synthetic.synthetic_tile_batch(3, 24, 40, 640, "V1")
    return list(depth), list(mask)


def _odd_sizes():
    from bathymetric_gnn_amd import synthetic
    t = [synthetic.synthetic_tile(h, w, 700 + i, "V1" if min(h, w) >= 20 else "V0") for i, (h, w) in enumerate([(13, 17), (9, 33)])]
    return [x[0] for x in t], [x[1] for x in t]


def _degenerate():
    from bathymetric_gnn_amd import synthetic
    d1, m1, _ = synthetic.synthetic_tile(11, 19, 811, "V0")
    m1 = np.zeros_like(m1); m1[5, 7] = True                                  # one valid node
    d2, m2, _ = synthetic.synthetic_tile(8, 16, 812, "V0")
    m2 = np.zeros_like(m2)                                                    # all invalid
    d3, m3, _ = synthetic.synthetic_tile(10, 20, 813, "V0")
    return [d1, d2, d3], [m1, m2, m3]


BATCHES = {"uniform_holes": _uniform_holes, "odd_sizes": _odd_sizes, "degenerate": _degenerate}


@gpu
@pytest.mark.parametrize("conn", ["8-connected", "4-connected"])
@pytest.mark.parametrize("batch", sorted(BATCHES))
def test_light_form_is_bit_identical_default_model(batch, conn, gpu_device):
    """The default model (4 layers, 4 heads: the 256 -> 64 launch and the heads launch) on a uniform batch with holes, on tiles whose
    sides are no multiples of the 8 x 16 block, and on a tile with one node next to a tile with none."""
    from bathymetric_gnn_amd import synthetic
    from bathymetric_gnn_amd.data import GraphBuilder
    from bathymetric_gnn_amd.models.pipeline import TileBatchEngine
    gb = GraphBuilder(device=gpu_device, connectivity=conn)
    eng = TileBatchEngine(_model(synthetic.synthetic_state_dict(seed=1234)), gb, gpu_device)
    depth, mask = BATCHES[batch]()
    a, b = _both_forms(gpu_device, _runner(eng, gb, depth, mask))
    _assert_same(a, b)
    assert a[1] == int(sum(int(m.sum()) for m in mask))
    if batch != "degenerate":
        assert float(a[0][1].max()) > 0.0 and bool(torch.isfinite(a[0]).all())


@gpu
@pytest.mark.parametrize("layers,heads", [(1, 4), (2, 4), (4, 4), (2, 1), (3, 2)])
def test_light_form_is_bit_identical_other_models(layers, heads, gpu_device):
    """L = 1 runs only the heads launch, L = 2 the 256 -> 64 launch right behind the front GEMM; 1 and 2 heads at hidden 64 run the
    64 -> 64 and 128 -> 64 instances, whose coefficient window is all heads."""
    from bathymetric_gnn_amd import synthetic
    from bathymetric_gnn_amd.data import GraphBuilder
    from bathymetric_gnn_amd.models.pipeline import TileBatchEngine
    gb = GraphBuilder(device=gpu_device)
    sd = synthetic.synthetic_state_dict(num_layers=layers, heads=heads, seed=77)
    eng = TileBatchEngine(_model(sd, num_layers=layers, heads=heads), gb, gpu_device)
    depth, mask = _uniform_holes()
    d2, m2 = _odd_sizes()
    a, b = _both_forms(gpu_device, _runner(eng, gb, depth + d2, mask + m2))
    _assert_same(a, b)
    assert float(a[0][1].max()) > 0.0


@gpu
@pytest.mark.parametrize("atlas", [1, 0])
def test_light_form_is_bit_identical_on_a_ragged_vr_batch(atlas, gpu_device):
    """About a dozen refinement grids between 3 x 3 and 50 x 50, walked through the packed canvas (cell_map / tile_of_cell, early exit
    of empty blocks) and grid by grid."""
    from bathymetric_gnn_amd import synthetic
    from bathymetric_gnn_amd.data import GraphBuilder
    from bathymetric_gnn_amd.models.pipeline import TileBatchEngine
    gb = GraphBuilder(device=gpu_device)
    eng = TileBatchEngine(_model(synthetic.synthetic_state_dict(in_channels=8, seed=1234), in_channels=8), gb, gpu_device)
    grids = synthetic.vr_grid_stream(12, seed0=1000)
    depth = [g[0] for g in grids]; unc = [g[1] for g in grids]
    mask = [np.isfinite(d) & (d < 1e5) for d in depth]
    run = _runner(eng, gb, depth, mask, res=(0.7, 0.9), unc=unc)
    c = _ctx(gpu_device)
    c.set_option("ragged_atlas", atlas)
    a, b = _both_forms(gpu_device, run)
    _assert_same(a, b)
    c.set_option("ragged_atlas", 1 - atlas)
    _assert_same(a, run())                               # and the other walk gives the same bits
    assert set(np.unique(a[0][0].cpu().numpy())) <= {0.0, 1.0, 2.0} and float(a[0][1].max()) > 0


@gpu
@pytest.mark.parametrize("case", ["bf16", "bf16x3", "k16", "GCN"])
def test_instances_without_a_light_form_ignore_the_option(case, gpu_device):
    from bathymetric_gnn_amd import synthetic
    from bathymetric_gnn_amd.data import GraphBuilder
    from bathymetric_gnn_amd.models.pipeline import TileBatchEngine
    gb = GraphBuilder(device=gpu_device, connectivity="16-dilated" if case == "k16" else "8-connected")
    kind = "GCN" if case == "GCN" else "GAT"
    eng = TileBatchEngine(_model(synthetic.synthetic_state_dict(seed=1234, gnn_type=kind), gnn_type=kind), gb, gpu_device)
    depth, mask = _uniform_holes()
    if case in ("bf16", "bf16x3"):
        _ctx(gpu_device).set_option("matrix_path", case)
    a, b = _both_forms(gpu_device, _runner(eng, gb, depth, mask))
    _assert_same(a, b)
    assert float(a[0][1].max()) > 0.0


@gpu
def test_light_form_against_the_cpu_oracle(gpu_device):
    """One tile, default model, option at its default: confidence and correction grids within 1e-4 of the float32 oracle."""
    from bathymetric_gnn_amd import synthetic
    from bathymetric_gnn_amd.data import GraphBuilder
    from bathymetric_gnn_amd.models.pipeline import TileBatchEngine
    sd = synthetic.synthetic_state_dict(seed=1234)
    gb = GraphBuilder(device=gpu_device)
    eng = TileBatchEngine(_model(sd), gb, gpu_device)
    d, m, _ = synthetic.synthetic_tile(24, 40, 640, "V1")
    assert _ctx(gpu_device).get_option("fused_light_form") == 1
    r = eng.infer([d], [m], None, [(0.5, 0.5)])[0]
    og = graph_cpu.build_graph(d, m, None, (0.5, 0.5))
    ref = gat_cpu.process_tile(sd, og)
    assert np.abs(r["confidence"] - ref["confidence"]).max() < TOL
    o = eng.model.predict(gb.build_graph(d, m, None, (0.5, 0.5)))
    rp = gat_cpu.predict(sd, og.x, og.edge_index, og.edge_attr)
    for k in ("class_logits", "confidence", "correction"):
        assert (o[k].cpu() - rp[k]).abs().max().item() < TOL, k
    assert np.array_equal(r["confidence"][m], o["confidence"].cpu().numpy())        # the grids hold predict()'s bits
    top2 = np.sort(gat_cpu.forward(sd, og.x, og.edge_index, og.edge_attr)["class_probs"].numpy(), axis=1)
    sure = graph_cpu.graph_to_grid(og, ((top2[:, -1] - top2[:, -2]) > TOL).astype(np.float32), 1.0).astype(bool)
    assert np.array_equal(r["classification"][sure], ref["classification"][sure])


def test_light_instances_fit_four_workgroups_per_cu():
    """No GPU needed: tools/kernel_resources.py (the compiler's own resource remarks, LDS from the launcher's FusedLds) for the light
    256 -> 64 and heads instances of both reference stencils: at most 128 VGPRs, no scratch (a spill reload would share vmcnt with the
    slab DMAs), at most 40 KB of LDS -- what four workgroups per CU need.  The form stands or falls by these numbers."""
    import os
    import re
    import subprocess
    import sys
    import __graft_entry__
    __graft_entry__.build()                              # no-op when up to date: the LDS figure comes from the built library
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, os.path.join(root, "tools", "kernel_resources.py"), "gat_layer_fused.hip", "0, 0, 1>"],
                       capture_output=True, text=True, check=True)
    rows = {}
    for line in r.stdout.splitlines():
        m = re.match(r"gat_layer_fused_kernel<([^>]*)>\s+VGPR\s+(\d+) AGPR\s+(\d+) scratch\s+(\d+) occ\s+(\d+) LDS\s+(\d+)", line)
        if m:
            rows[m.group(1)] = tuple(int(x) for x in m.groups()[1:])
    for inst in ("256, 64, 8, 2, 0, 0, 0, 1", "64, 64, 8, 3, 1, 0, 0, 1", "256, 64, 4, 2, 0, 0, 0, 1", "64, 64, 4, 3, 1, 0, 0, 1"):
        assert inst in rows, (inst, r.stdout, r.stderr[-500:])
        vgpr, agpr, scratch, occ, lds = rows[inst]
        print(inst, rows[inst])
        assert vgpr + agpr <= 128 and scratch == 0 and 0 < lds <= 40960 and occ >= 4, (inst, rows[inst])
