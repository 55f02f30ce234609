"""Sounding density as a node feature, the parts that need no GPU: the column count, the all-or-none rule of a batch, the
checkpoint key ``node_planes``, ``density_plane`` against numpy word for word, and the first extractor image of a model with more
than 8 input channels (tests/density_pack_check.cpp over csrc/model_images.h)."""
import json
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

from bathymetric_gnn_amd import runtime as rt
from bathymetric_gnn_amd.data import BathymetricGrid, GraphBuilder
from bathymetric_gnn_amd.data.sounding_grid import SoundingGrid, density_from_count
from bathymetric_gnn_amd.data.sounding_robust import RobustSoundingGrid
from bathymetric_gnn_amd.data.sounding_vr import RobustVRSoundingGrid, VRSoundingGrid
from bathymetric_gnn_amd.models.pipeline import BathymetricPipeline, check_node_planes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_n_node_columns():
    gb = GraphBuilder()
    assert gb.n_node_columns(False) == 7 and gb.n_node_columns(True) == 8                    # as before
    assert gb.n_node_columns(False, 1) == 8 and gb.n_node_columns(True, 1) == 9 and gb.n_node_columns(True, 8) == 16
    three = GraphBuilder(node_features=["depth", "uncertainty", "curvature"])
    assert three.n_node_columns(False) == 2 and three.n_node_columns(True) == 3 and three.n_node_columns(True, 1) == 4
    assert three.n_node_columns(False, 2) == 4


def test_mixed_batches_are_refused_before_the_device_is_asked_for():
    gb = GraphBuilder()
    d = [np.zeros((3, 4), np.float32), np.zeros((2, 2), np.float32)]
    with pytest.raises(ValueError, match="sounding density layer or none"):
        gb.upload_density([np.ones((3, 4), np.float32), None], d)
    with pytest.raises(ValueError, match="sounding density layer or none"):
        gb.build_graphs(d, densities=[None, np.ones((2, 2), np.float32)])
    with pytest.raises(ValueError, match="uncertainty layer or none"):                       # (the rule it mirrors)
        gb.upload_tiles(d, None, [np.ones((3, 4), np.float32), None], [(1.0, 1.0)] * 2)
    with pytest.raises(ValueError, match=r"density shape \(2, 2\) != depth shape \(3, 4\)"):
        gb.upload_density([np.ones((2, 2), np.float32), np.ones((2, 2), np.float32)], d)
    assert gb.upload_density(None, d) == [] and gb.upload_density([None, None], d) == []


def test_aux_plane_array():
    a, b = torch.arange(6, dtype=torch.float32), torch.ones(6)
    n, arr, keep = rt.make_aux_planes([a, b], 6)
    assert n == 2 and [arr[0], arr[1]] == [a.data_ptr(), b.data_ptr()]
    assert rt.make_aux_planes(None)[:2] == (0, None) and rt.make_aux_planes([])[:2] == (0, None)
    with pytest.raises(ValueError, match="at most 8"):
        rt.make_aux_planes([a] * 9)
    with pytest.raises(ValueError, match="plane 1 has 6 cells, the tile table has 7"):
        rt.make_aux_planes([torch.ones(7), b], 7)
    with pytest.raises(ValueError, match="float32"):
        rt.make_aux_planes([a.double()], 6)
    with pytest.raises(ValueError, match="plane 0 is None"):
        rt.make_aux_planes([None], 6)


def test_node_planes_key_round_trips_through_a_dict(tmp_path):
    assert check_node_planes(None) is None and check_node_planes([]) == ()
    assert check_node_planes(["uncertainty", "sounding_density"]) == ("uncertainty", "sounding_density")
    assert check_node_planes(("sounding_density",)) == ("sounding_density",)
    for bad in (["sounding_density", "uncertainty"], ["density"], ["uncertainty", "uncertainty"]):
        with pytest.raises(ValueError, match="a sublist of"):
            check_node_planes(bad)
    ck = {"in_channels": 9, "edge_dim": 3, "node_planes": ["uncertainty", "sounding_density"]}
    path = tmp_path / "ck.pt"
    torch.save(ck, path)
    back = torch.load(path, map_location="cpu", weights_only=True)
    assert back == ck and check_node_planes(back["node_planes"]) == rt.NODE_PLANES

    class Store:                                            # what Trainer._save_checkpoint reads off its training store
        unc, density = object(), object()
    from bathymetric_gnn_amd.training.tile_store import TileStore
    assert TileStore.node_planes.fget(Store) == ["uncertainty", "sounding_density"]
    Store.unc = None
    assert TileStore.node_planes.fget(Store) == ["sounding_density"]
    Store.density = None
    assert TileStore.node_planes.fget(Store) == []


def test_pipeline_plane_rules():
    """Stated planes are passed exactly, a missing one is named; without the key the in_channels == 8 rule holds."""
    class M:
        in_channels = 8
    p = BathymetricPipeline.__new__(BathymetricPipeline)
    p.model, p.node_planes = M(), None
    grid = BathymetricGrid(depth=np.zeros((4, 4), np.float32), uncertainty=np.ones((4, 4), np.float32))
    assert grid.density is None
    unc, den = p._grid_planes(grid)
    assert unc is grid.uncertainty and den is None and p._takes_uncertainty() and not p._takes_density()
    p.model.in_channels = 7
    assert p._grid_planes(grid) == (None, None)
    p.model.in_channels = 9
    assert p._grid_planes(grid) == (None, None)                                              # (not 8: no uncertainty, as before)
    p.node_planes = ("uncertainty", "sounding_density")
    with pytest.raises(ValueError, match="'sounding_density' and the grid has none"):
        p._grid_planes(grid)
    grid.density = np.full((4, 4), 0.5, np.float32)
    unc, den = p._grid_planes(grid)
    assert unc is grid.uncertainty and den is grid.density
    grid.uncertainty = None
    with pytest.raises(ValueError, match="'uncertainty' and the grid has none"):
        p._grid_planes(grid)
    p.node_planes = ("sounding_density",)
    assert p._grid_planes(grid)[0] is None and p._grid_planes(grid)[1] is grid.density
    with pytest.raises(NotImplementedError, match="process_grid_streamed does not carry the sounding density"):
        p._refuse_density("process_grid_streamed")
    p.node_planes = ("uncertainty",)
    p._refuse_density("process_grid_streamed")


def _want(count: np.ndarray) -> np.ndarray:
    with np.errstate(divide="ignore"):
        q = np.float32(1) / count.astype(np.float32)
    return np.where(count >= 1, q, np.float32(0)).astype(np.float32)


def test_density_plane_is_one_rounded_division():
    rng = np.random.default_rng(5)
    count = np.concatenate([np.arange(0, 4099), rng.integers(0, 2 ** 31 - 1, 3000), [2 ** 24 + 1, 2 ** 31 - 1]]).astype(np.int32)
    count = count[:7098].reshape(91, 78)
    want = _want(count)
    got = density_from_count(torch.from_numpy(count))
    assert got.dtype == torch.float32 and got.shape == (91, 78)
    assert np.array_equal(got.numpy().view(np.uint32), want.view(np.uint32))
    assert got.max().item() == 1.0 and got.min().item() == 0.0 and (got[torch.from_numpy(count) >= 1] > 0).all()
    c = torch.from_numpy(count)
    kept = torch.from_numpy((count // 2).astype(np.int32))
    z = torch.zeros(91, 78)
    plain = SoundingGrid(count=c, mean=z, std=z, min=z, max=z, valid=(c >= 1).to(torch.uint8), counters={},
                         transform=(10.0, 2.0, 0.0, 50.0, 0.0, -2.0), resolution=(2.0, 2.0))
    assert np.array_equal(plain.density_plane().numpy().view(np.uint32), want.view(np.uint32))
    four = plain.survey_tensors(density=True)
    assert len(plain.survey_tensors()) == 3 and len(four) == 4 and torch.equal(four[3], plain.density_plane())
    grid = plain.to_grid()
    assert grid.density.dtype == np.float32 and np.array_equal(grid.density.view(np.uint32), want.view(np.uint32))
    fields = {f: z for f in ("median", "mad", "kept_mean", "kept_std", "kept_min", "kept_max", "center2", "limit")}
    robust = RobustSoundingGrid(count=c, kept=kept, valid=(kept >= 1).to(torch.uint8), sorted_q=z, start=z, counters={},
                                transform=(10.0, 2.0, 0.0, 50.0, 0.0, -2.0), resolution=(2.0, 2.0), **fields)
    want_kept = _want(count // 2)
    assert np.array_equal(robust.density_plane().numpy().view(np.uint32), want_kept.view(np.uint32))       # the count is `kept`
    assert torch.equal(robust.survey_tensors(density=True)[3], robust.density_plane()) and len(robust.survey_tensors()) == 3
    assert np.array_equal(robust.to_grid().density.view(np.uint32), want_kept.view(np.uint32))
    flat = c.reshape(-1)
    vr = VRSoundingGrid(count=flat, mean=z, std=z, min=z, max=z, valid=z, counters={}, layout=None)
    assert np.array_equal(vr.density_plane().numpy().view(np.uint32), want.reshape(-1).view(np.uint32))
    rvr = RobustVRSoundingGrid(count=flat, kept=kept.reshape(-1), valid=z, sorted_q=z, start=z, counters={}, layout=None, **fields)
    assert np.array_equal(rvr.density_plane().numpy().view(np.uint32), want_kept.reshape(-1).view(np.uint32))


def _cxx():
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    for c in (shutil.which("g++"), os.path.join(rocm, "lib", "llvm", "bin", "clang++"), shutil.which("amdclang++"), shutil.which("clang++")):
        if c and os.path.exists(c):
            return c
    pytest.fail("no C++ compiler: neither g++ nor ROCm's clang++")


def test_first_extractor_image_above_8_channels(tmp_path):
    """fe_W0t is [8][hid] up to 8 channels (its bytes are pinned by tests/test_host_pack.py against the parent's packer) and
    [16][hid] above: the weight transposed into rows 0 .. in - 1, zeros behind, and the refresh plan's copy table rewrites it."""
    exe = tmp_path / "density_pack_check"
    subprocess.run([_cxx(), "-std=c++17", "-O1", os.path.join(ROOT, "tests", "density_pack_check.cpp"), "-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    doc = json.loads(r.stdout)
    assert sorted(doc) == sorted(f"{t}_in{i}" for t in ("gat", "sage") for i in (7, 8, 9, 16))
    for name, c in doc.items():
        in_ch = int(name.split("_in")[1])
        assert c["rows"] == (8 if in_ch <= 8 else 16), name
        assert c["transposed"] and c["zero_behind"] and c["refreshed"] and c["plan_error"] == "" and c["fe_W0t_off"] == 0, name
    for t in ("gat", "sage"):
        assert doc[f"{t}_in9"]["weights"] - doc[f"{t}_in8"]["weights"] == 64
        assert doc[f"{t}_in16"]["weights"] - doc[f"{t}_in8"]["weights"] == 8 * 64
