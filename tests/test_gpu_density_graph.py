"""Graphs built with auxiliary node planes (bgnn_graph_build_aux, node_aux.hip): every table of the plain build bit for bit, the
planes behind its columns as words, for uniform and ragged batches, holes, a one-cell tile and an empty one."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

SHAPES = [(2, 2), (5, 7), (17, 33), (64, 64)]
THREE = ["depth", "gradient_x", "curvature"]
PAYLOAD = np.uint32(0x7FC12345)                   # a quiet NaN with a payload


def _tiles(seed=3):
    """The four shapes twice: holes everywhere; the second 5 x 7 has one valid cell, the second 2 x 2 none."""
    rng = np.random.default_rng(seed)
    out = []
    for k, (h, w) in enumerate(SHAPES + SHAPES):
        depth = (-20.0 + rng.standard_normal((h, w)).cumsum(0).cumsum(1) * 0.05).astype(np.float32)
        mask = rng.random((h, w)) < 0.8
        if k == 4:
            mask[:] = False
        if k == 5:
            mask[:] = False
            mask[3, 4] = True
        unc = (0.05 + 0.1 * rng.random((h, w))).astype(np.float32)
        count = rng.integers(0, 9, (h, w))
        count[mask & (count == 0)] = 1
        den = np.where(count >= 1, np.float32(1) / np.maximum(count, 1).astype(np.float32), np.float32(0)).astype(np.float32)
        out.append((depth, mask, unc, den))
    flat = out[3][3].reshape(-1).view(np.uint32)
    flat[np.flatnonzero(out[3][1].reshape(-1))[7]] = PAYLOAD     # one valid cell of the first 64 x 64 carries the payload
    return out


def _words(t):
    return t.contiguous().cpu().numpy().view(np.uint32 if t.dtype == torch.float32 else np.int64)


@pytest.mark.parametrize("features", [None, THREE], ids=["seven", "three"])
@pytest.mark.parametrize("conn", ["4-connected", "8-connected"])
@pytest.mark.parametrize("with_unc", [False, True], ids=["plain", "unc"])
def test_density_column_behind_a_bit_identical_plain_build(with_unc, conn, features, gpu_device):
    from bathymetric_gnn_amd.data import GraphBuilder
    tiles = _tiles()
    gb = GraphBuilder(connectivity=conn, node_features=features)
    d, m, u, a = ([t[i] for t in tiles] for i in range(4))
    uncs = u if with_unc else None
    res = [(0.5, 0.25)] * len(tiles)
    plain = gb.build_graphs(d, m, uncs, res)
    wide = gb.build_graphs(d, m, uncs, res, densities=a)
    F0 = gb.n_node_columns(with_unc)
    assert F0 == (len(features) if features else 7) + int(with_unc)                 # the column lands in quarter 0, 1 or 2
    assert plain.num_features == F0 and wide.num_features == F0 + 1 == gb.n_node_columns(with_unc, 1)
    nf = __import__("ctypes").c_int32()
    from bathymetric_gnn_amd import runtime as rt
    rt.check(wide._ctx.lib.bgnn_graph_counts(wide._handle, None, None, nf, None, None, None))
    assert nf.value == F0 + 1
    assert wide.num_nodes == plain.num_nodes == sum(int(t[1].sum()) for t in tiles) and wide.num_edges == plain.num_edges
    assert np.array_equal(wide.ptr.numpy(), plain.ptr.numpy())
    assert wide.x.shape == (wide.num_nodes, F0 + 1)
    assert np.array_equal(_words(wide.x[:, :F0]), _words(plain.x))
    for name in ("edge_index", "edge_attr", "pos", "local_std", "valid_rows", "valid_cols", "batch"):
        assert np.array_equal(_words(getattr(wide, name)), _words(getattr(plain, name))), name
    want = np.concatenate([t[3][t[1]] for t in tiles]).view(np.uint32)              # batch order: tile by tile, row-major
    got = _words(wide.x[:, F0])
    assert np.array_equal(got, want) and (got == PAYLOAD).sum() == 1


@pytest.mark.parametrize("uniform", [False, True], ids=["ragged", "uniform"])
def test_two_planes_through_build_from_device(uniform, gpu_device):
    """aux_t=[a, b] gives columns F0 and F0 + 1; a uniform batch (the cached tile tables, the LDS-tiled feature kernel at 64 x 64) and
    the ragged one (the canvas form); the planes' invalid cells are never read into x."""
    from bathymetric_gnn_amd.data import GraphBuilder
    tiles = [t for t in _tiles(5) if not uniform or t[0].shape == (64, 64)]
    gb = GraphBuilder()
    hw, res, d, m, u = gb.upload_tiles([t[0] for t in tiles], [t[1] for t in tiles], [t[2] for t in tiles], [(1.0, 1.0)] * len(tiles))
    rng = np.random.default_rng(11)
    a = torch.from_numpy(rng.standard_normal(d.numel()).astype(np.float32)).to(gpu_device)
    b = torch.from_numpy(rng.integers(0, 2 ** 32, d.numel(), dtype=np.uint64).astype(np.uint32).view(np.float32)).to(gpu_device)
    plain = gb.build_from_device(hw, res, d, m, u)
    wide = gb.build_from_device(hw, res, d, m, u, aux_t=[a, b])
    assert wide.num_features == 10 and wide.x.shape[1] == 10
    valid = m.bool()
    assert np.array_equal(_words(wide.x[:, :8]), _words(plain.x))
    assert np.array_equal(_words(wide.x[:, 8]), _words(a[valid])) and np.array_equal(_words(wide.x[:, 9]), _words(b[valid]))
    assert np.array_equal(_words(wide.edge_attr), _words(plain.edge_attr))
    eight = gb.build_from_device(hw, res, d, m, u, aux_t=[a] * 8)                   # the wide table filled to its last column
    assert eight.x.shape[1] == 16 and np.array_equal(_words(eight.x[:, 15]), _words(a[valid]))
    assert np.array_equal(_words(eight.x[:, :8]), _words(plain.x))
    with pytest.raises(ValueError, match="plane 0 has"):
        gb.build_from_device(hw, res, d, m, u, aux_t=[a[:-1]])
    with pytest.raises(ValueError, match="at most 8"):
        gb.build_from_device(hw, res, d, m, u, aux_t=[a] * 9)


def test_empty_and_single_grids(gpu_device):
    """build_graph(density=...): one grid with no valid cell is the empty graph as before; one valid cell gives a 1 x (F0 + 1) table."""
    from bathymetric_gnn_amd.data import GraphBuilder
    gb = GraphBuilder()
    depth = np.full((5, 7), -3.0, np.float32)
    den = np.full((5, 7), 0.5, np.float32)
    empty = gb.build_graph(depth, np.zeros((5, 7), bool), None, (1.0, 1.0), density=den)
    assert empty.num_nodes == 0 and empty.x.shape[0] == 0
    mask = np.zeros((5, 7), bool); mask[2, 3] = True
    den[2, 3] = 0.125
    one = gb.build_graph(depth, mask, None, (1.0, 1.0), density=den)
    assert one.num_nodes == 1 and one.x.shape == (1, 8) and one.x[0, 7].item() == 0.125 and one.num_edges == 0


def test_density_plane_on_the_device_is_one_rounded_division(gpu_device):
    """density_from_count on the GPU against numpy word for word, every count up to 2^17 and large ones."""
    from bathymetric_gnn_amd.data.sounding_grid import density_from_count
    count = np.concatenate([np.arange(0, 1 << 17), [2 ** 24 - 1, 2 ** 24 + 1, 2 ** 31 - 1]]).astype(np.int32)
    want = np.where(count >= 1, np.float32(1) / np.maximum(count, 1).astype(np.float32), np.float32(0)).astype(np.float32)
    got = density_from_count(torch.from_numpy(count).to(gpu_device))
    assert got.dtype == torch.float32 and np.array_equal(_words(got), want.view(np.uint32))
