"""The reference's default geometry (``TileConfig()``: 1024 x 1024 tiles, overlap 128, min_valid_ratio 0.1) and sparse
footprints, against the float64 oracle.

A 1 M-node tile is minutes of CPU oracle, so every other oracle-checked test stops at 256 x 256.  Here the float64 reference is
``_window_oracle``'s: the eval-mode forward is local, so the oracle on a 64 x 64 crop equals the whole-tile oracle on every crop
cell at least R = 3 + layers x hop cells from each crop edge that is not the tile's own (tests/test_oracle_window.py pins that
on the CPU, residue <= 0.06 of float32 arithmetic's own distance to float64).  The acceptance rule is the project's own,
``_conditioning.float64_bound`` with BOUND_C / BOUND_FLOOR unchanged, on the windows' trusted cells: every output within
BOUND_C x the float32 oracle's distance to float64; classes equal wherever float64's top-2 gap exceeds 10 x the logit bound, and
more than 0.9 of the cells are that sure.  The float32 oracle itself is held to the same rule first (``_check``), and the heads are
calibrated on one window, so that classes and actions mix (asserted).

1. one 1024 x 1024 tile, masks V0 / V1 / a ragged footprint (diagonal band + islands, ~30 %), through ``predict`` (one graph of a
   million rows) and ``TileBatchEngine.infer`` (bgnn_infer_tiles, the fused layers' uniform walk over 8 192 blocks); 14 windows:
   the four corners, the middle of each edge, across row / column 512, across row 768 / column 256, one whose first trusted cell is
   the LAST cell of an 8 x 16 block, two across the footprint's boundary, one around an island;
2. the same tile (V1) on the other shipped paths, windows placed with each path's own R: 4-connected, 16-dilated (R = 11), bf16
   storage (the rule and constants of test_config3_bf16_storage_distance_to_float64), the unfused aggregate;
3. one uniform batch of six 512 x 512 tiles: a 10.5 % blob, 3-cell stripes, a checkerboard of 8 x 16 blocks, a one-cell diagonal +
   200 isolated cells (degree 0 under 4-connectivity: the self-loop-only softmax), an all-invalid tile, V0;
4. ``BathymetricPipeline(Config())`` with nothing overridden on a 1920 x 2000 survey whose footprint puts one tile one cell
   under the 10 % line and one exactly on it.

Worst ``dist / float32_dist`` per output and route, measured on an MI355X (every figure is printed by the tests):

    case / route                               logits   confidence   correction   hidden
    1. 8-connected V0 / V1 / ragged, predict    1.09      1.30         1.15          -
       ... asking for the backbone output       1.18      1.32         1.07         1.15
       ... TileBatchEngine.infer                  -       1.30         1.14          -
    2. 4-connected, predict | tiles             1.05   1.10 | 1.10  1.31 | 1.10     1.11
       16-dilated, predict | tiles              1.09   1.09 | 1.09  1.11 | 0.98     0.96
       unfused aggregate, predict               0.97      0.99         1.14         1.15
       bf16 storage, predict (its own rule)     max |dlogit| 0.50 against 0.83, rms 0.084 against 0.21; agreement on clear
                                                cells 0.991 (0.98 asked), flips over all cells 0.016 (0.15 allowed)
    3. sparse batch, worst tile (tiles)           -       1.33         1.37          -
    4. default-Config survey, stitched            -       1.03         1.07          -

Against BOUND_C = 4.  No kernel or host-path defect showed.  The cells compared: 39 396 / 37 433 / 11 639 per 1024 x 1024 tile (V0 / V1 /
ragged), 29 180 at R = 11, 188 .. 3 538 per sparse tile, 15 749 on the survey (68 of them with disagreeing tile labels, 2 505
firing the correction); more than 0.98 of them are sure everywhere.
"""
import functools
import json

import numpy as np
import pytest
import torch

import _window_oracle as wo
from _calibration import calibrate_heads
from _conditioning import BOUND_C, BOUND_FLOOR, OUTPUT_KEYS, distances, float64_bound
from oracle import graph_cpu

pytestmark = pytest.mark.gpu
RES = (0.5, 0.5)
T, S, LAYERS = 1024, 64, 4
GRID_KEYS = ("confidence", "correction")
NODATA = np.float32(1.0e6)


@pytest.fixture(autouse=True)
def _default_options_after():
    yield
    if torch.cuda.is_available():
        ctx = _ctx()
        ctx.set_option("matrix_path", "exact_f32"); ctx.set_option("fused", 1); ctx.set_option("bf16_layer0_af", 1)


def _ctx():
    from bathymetric_gnn_amd import runtime as rt
    return rt.get_context(torch.device("cuda:0"))


def _model(sd):
    from bathymetric_gnn_amd.models import BathymetricGNN
    m = BathymetricGNN(in_channels=7, edge_dim=3, dropout=0.0)           # the default model: GAT, hidden 64, heads 4, 4 layers
    assert (m.gnn_type, m.hidden_channels, m.heads, m.num_gnn_layers) == ("GAT", 64, 4, LAYERS)
    m.load_state_dict({k: torch.as_tensor(v) for k, v in sd.items()})
    return m.to(torch.device("cuda:0")).eval()


# ---- inputs ----------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _footprint():
    """A diagonal band |row - col| < 160 plus 40 discs (radius 3 .. 14) clear of it: about 30 % of the tile."""
    r, c = np.mgrid[0:T, 0:T]
    fp = np.abs(r - c) < 160
    rng = np.random.default_rng(77)
    islands = []
    while len(islands) < 40:
        cr, cc, rad = int(rng.integers(20, T - 20)), int(rng.integers(20, T - 20)), int(rng.integers(3, 15))
        if abs(cr - cc) < 160 + 2 * rad + 8:
            continue
        fp |= (r - cr) ** 2 + (c - cc) ** 2 <= rad * rad
        islands.append((cr, cc, rad))
    return fp, islands


@functools.lru_cache(maxsize=None)
def _tile(name):
    from bathymetric_gnn_amd import synthetic
    if name == "V0":
        d, m, _ = synthetic.synthetic_tile(T, T, 5, "V0")
        return d, m
    d, m, _ = synthetic.synthetic_tile(T, T, 5, "V1")
    if name == "ragged":
        m = m & _footprint()[0]
        d = np.where(m, d, NODATA).astype(np.float32)
        assert 0.27 < m.mean() < 0.33
    return d, m


def _windows(R):
    """The 14 windows of the 1024 x 1024 tile.  Only the block-edge window depends on R: its first trusted cell is (327, 591),
    row = 7 mod 8 and column = 15 mod 16, the last cell of an 8 x 16 block."""
    assert 327 % 8 == 7 and 591 % 16 == 15
    ir, ic, _ = _footprint()[1][0]
    return [(0, 0, S, S), (0, T - S, S, S), (T - S, 0, S, S), (T - S, T - S, S, S),            # corners
            (0, 480, S, S), (T - S, 481, S, S), (483, 0, S, S), (470, T - S, S, S),            # middle of each edge
            (480, 480, S, S),                                                                  # across row / column 512
            (736, 224, S, S),                                                                  # across row 768 / column 256
            (327 - R, 591 - R, S, S),
            (268, 428, S, S), (678, 518, S, S),                                                # across the band's two boundaries
            wo.clip_window(ir - S // 2, ic - S // 2, S, S, (T, T))]                            # around an island


CALIBRATION_WINDOW = (480, 480, S, S)


@functools.lru_cache(maxsize=None)
def _sd(conn="8-connected", spread=0.1):
    """Default-model weights, heads calibrated on one window of the V1 tile."""
    from bathymetric_gnn_amd import synthetic
    d, m = _tile("V1")
    r0, c0, h, w = CALIBRATION_WINDOW
    og = graph_cpu.build_graph(d[r0:r0 + h, c0:c0 + w], m[r0:r0 + h, c0:c0 + w], None, RES, connectivity=conn)
    return calibrate_heads(synthetic.synthetic_state_dict(seed=1234), og.x, og.edge_index, og.edge_attr, logit_spread=spread)


@functools.lru_cache(maxsize=None)
def _runs(name, conn, spread=0.1):
    d, m = _tile(name)
    R = wo.reach(LAYERS, conn)
    wins = _windows(R)
    sd = _sd(conn, spread)
    return wins, [wo.window_forward(d, m, None, RES, sd, conn, w, denormalise=False) for w in wins], R


def _reference(name, conn, denormalise, spread=0.1):
    """(ref32, ref64, rows, cols) on the trusted cells of the tile's windows -- the forwards run once per (tile, path)."""
    wins, runs, R = _runs(name, conn, spread)
    return wo.gather(wo.denormalised(runs) if denormalise else runs, wins, (T, T), R)


# ---- the rule --------------------------------------------------------------------------------------------------------
def _actions(ref):
    cls, conf = ref["predicted_class"], ref["confidence"]
    return torch.where(conf < 0.6, 2, torch.where((cls == 2) & (conf > 0.85), 1, 0))


def _assert_mixed(ref64):
    assert torch.unique(ref64["predicted_class"]).numel() >= 2, "one class on every compared cell: the class check is vacuous"
    assert set(torch.unique(_actions(ref64)).tolist()) == {0, 1, 2}, "one action on every compared cell"


def _check(name, out, ref32, ref64, keys, min_sure=0.9):
    """float64_bound, unchanged, after the float32 oracle itself has passed it."""
    ok32, rep32 = float64_bound(ref32, ref32, ref64, keys=keys)
    assert ok32 and rep32["sure_fraction"] > min_sure, (name, "the float32 oracle", rep32)
    ok, rep = float64_bound(out, ref32, ref64, keys=keys)
    ratios = {k: round(rep[k]["dist"] / rep[k]["float32_dist"], 3) if rep[k]["float32_dist"] > 0 else None for k in keys if k in rep}
    print(f"{name}: cells {int(ref64['confidence'].numel())} dist/float32_dist {json.dumps(ratios)} sure {rep['sure_fraction']:.3f} "
          f"{json.dumps({k: rep[k] for k in keys if k in rep})}")
    assert ok, (name, rep)
    return rep


def _node_index(mask):
    return (np.cumsum(mask.ravel()) - 1).reshape(mask.shape)


def _nodes_at(out, mask, rows, cols, keys=OUTPUT_KEYS + ("predicted_class",)):
    sel = torch.from_numpy(_node_index(mask)[rows, cols]).to(out["confidence"].device)
    return {k: out[k][sel] for k in keys if k in out}


def _cells_at(r, rows, cols):
    return {"predicted_class": torch.from_numpy(r["classification"][rows, cols]).long(),
            "confidence": torch.from_numpy(r["confidence"][rows, cols]), "correction": torch.from_numpy(r["correction"][rows, cols])}


def _both_routes(label, d, m, conn, refs_predict, refs_tiles, gpu_device, predict_keys=OUTPUT_KEYS):
    """``predict`` on the tile's one graph and ``TileBatchEngine.infer`` on the tile, each under the rule; and the two routes
    against each other as test_full_batch_properties / test_headline_full_batch... require: the class grid is ``predict``'s
    classes, the confidence grid holds ``predict``'s bits, cells without a node are exactly 0."""
    from bathymetric_gnn_amd.data import GraphBuilder
    from bathymetric_gnn_amd.models.pipeline import TileBatchEngine
    sd = _sd(conn)
    model, gb = _model(sd), GraphBuilder(connectivity=conn)
    p32, p64, rows, cols = refs_predict
    t32, t64, _, _ = refs_tiles
    _assert_mixed(p64)
    g = gb.build_graph(d, m, None, RES)
    assert g.num_nodes == int(m.sum())
    out = model.predict(g)
    _check(f"{label}/predict", _nodes_at(out, m, rows, cols), p32, p64, predict_keys)
    # the backbone output too (asking for it takes the last layer off the fused heads launch: another path to the same outputs)
    hid = model._run(g, 0.85, 0.6, with_flags=False, want_hidden=True)
    _check(f"{label}/hidden", _nodes_at(hid, m, rows, cols), p32, p64, predict_keys)
    del hid
    r = TileBatchEngine(model, gb, gpu_device).infer([d], [m], None, [RES])[0]
    _check(f"{label}/tiles", _cells_at(r, rows, cols), t32, t64, GRID_KEYS)
    for k in ("classification", "confidence", "correction"):
        assert r[k].shape == m.shape and not r[k][~m].any(), k
    assert np.array_equal(r["confidence"][m], out["confidence"].cpu().numpy())
    assert np.array_equal(r["classification"][m], out["predicted_class"].cpu().numpy().astype(np.float32))


# ---- 1. one 1024 x 1024 tile, both routes ------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["V0", "V1", "ragged"])
def test_one_1024_tile_against_float64_on_both_routes(name, gpu_device):
    d, m = _tile(name)
    conn = "8-connected"
    _both_routes(name, d, m, conn, _reference(name, conn, False), _reference(name, conn, True), gpu_device)


# ---- 2. the same tile on the other shipped paths -----------------------------------------------------------------------
@pytest.mark.parametrize("path", ["4-connected", "16-dilated", "bf16", "unfused"])
def test_1024_tile_on_the_other_paths(path, gpu_device):
    from bathymetric_gnn_amd.data import GraphBuilder
    d, m = _tile("V1")
    if path in ("4-connected", "16-dilated"):
        assert wo.reach(LAYERS, path) == (7 if path == "4-connected" else 11)
        _both_routes(path, d, m, path, _reference("V1", path, False), _reference("V1", path, True), gpu_device)
    elif path == "unfused":
        conn = "8-connected"
        p32, p64, rows, cols = _reference("V1", conn, False)
        with _ctx().options(fused=0):
            out = _model(_sd(conn))._run(GraphBuilder().build_graph(d, m, None, RES), 0.85, 0.6, with_flags=True, want_hidden=True)
        _check("unfused/predict", _nodes_at(out, m, rows, cols), p32, p64, OUTPUT_KEYS)
    else:
        # matrix_path = bf16 on its own stencil (configs[2]: 16-dilated), heads calibrated to a logit spread of 1.0 and every
        # assertion of test_config3_bf16_storage_distance_to_float64 -- its bound functions imported, its constants as written there
        from test_gpu_forward import TOL, _bf16_bound, _fp64_distance
        conn = "16-dilated"
        _, ref64, rows, cols = _reference("V1", conn, False, spread=1.0)
        model = _model(_sd(conn, 1.0))
        g = GraphBuilder(connectivity=conn).build_graph(d, m, None, RES)
        exact = _nodes_at(model.predict(g), m, rows, cols)
        with _ctx().options(matrix_path="bf16"):
            assert _ctx().get_option("bf16_layer0_af") == 1
            out = _nodes_at(model.predict(g), m, rows, cols)
        e_exact, e_bf16 = _fp64_distance(exact, ref64), _fp64_distance(out, ref64)
        top2 = torch.topk(ref64["class_probs"], 2, dim=-1).values
        clear = (top2[:, 0] - top2[:, 1]) > 0.02
        same = out["predicted_class"].cpu() == ref64["predicted_class"]
        classes = torch.bincount(ref64["predicted_class"], minlength=3).double() / ref64["predicted_class"].numel()
        bound = _bf16_bound(ref64)
        row = {"cells": int(same.numel()), "logit_abs_max": float(ref64["class_logits"].abs().max()), "logit_bound_scaled": bound,
               "exact_f32": {"max": e_exact[0], "rms": e_exact[1]}, "bf16_storage": {"max": e_bf16[0], "rms": e_bf16[1]},
               "class_agreement_on_clear_nodes": float(same[clear].double().mean()), "clear_fraction": float(clear.double().mean()),
               "class_flip_rate_all_nodes": float((~same).double().mean()), "float64_class_shares": [float(c) for c in classes],
               "exact_flip_rate": float((exact["predicted_class"].cpu() != ref64["predicted_class"]).double().mean())}
        print("bf16/predict", json.dumps(row))
        assert e_exact[0] < TOL
        assert e_bf16[0] < bound and e_bf16[1] < bound / 4, row
        assert float(classes.min()) > 0.05, row
        assert row["clear_fraction"] >= 0.5, row
        assert row["class_agreement_on_clear_nodes"] > 0.98, row
        assert row["class_flip_rate_all_nodes"] < 0.15, row
        assert row["exact_flip_rate"] < 1e-3, row


# ---- 3. sparse uniform batches -----------------------------------------------------------------------------------------
P = 512
EMPTY = 4


@functools.lru_cache(maxsize=None)
def _sparse_tiles():
    """Six 512 x 512 tiles: [(depth, mask)], the isolated cells of tile 3, and the windows of every tile."""
    from bathymetric_gnn_amd import synthetic
    r, c = np.mgrid[0:P, 0:P]
    blob = (r - 300) ** 2 + (c - 200) ** 2 <= 94 * 94                       # 10.6 %: whole block rows above / below are empty
    stripes = (c % 12) < 3                                                 # 25 %: every 16-column block holds one or two stripes
    checker = ((r // 8) + (c // 16)) % 2 == 0                              # 50 %: full and empty 8 x 16 blocks alternate
    line = r == c
    rng = np.random.default_rng(9)
    lattice = [(8 * i + 4, 8 * j + 4) for i in range(P // 8) for j in range(P // 8) if abs(8 * i - 8 * j) > 8]
    iso = [lattice[k] for k in rng.choice(len(lattice), 200, replace=False)]
    for ir, ic in iso:
        line[ir, ic] = True
    masks = [blob, stripes, checker, line, np.zeros((P, P), bool), np.ones((P, P), bool)]
    assert 0.104 < blob.mean() < 0.107 and 0.25 <= stripes.mean() < 0.255 and checker.mean() == 0.5 and line.sum() == P + 200
    for ir, ic in iso:                                                     # no valid cell within 3 of an isolated cell
        assert line[ir - 3:ir + 4, ic - 3:ic + 4].sum() == 1
    assert not blob[:200].any() and not blob[400:].any()
    tiles = []
    for i, mk in enumerate(masks):
        d, _, _ = synthetic.synthetic_tile(P, P, 70 + i, "V0")
        tiles.append((np.where(mk, d, NODATA).astype(np.float32), mk))
    around = lambda rr, cc, s=48: wo.clip_window(rr - s // 2, cc - s // 2, s, s, (P, P))
    wins = [[around(206, 200, S), around(300, 294, S), around(366, 134, S)],        # the blob's top, right and lower-left boundary
            [(0, 0, S, S), (230, 250, S, S), (P - S, P - 48, S, 48)],               # stripes: a corner, the interior, the far edge
            [(P - S, P - S, S, S), (200, 136, S, S)],                               # checkerboard: a corner, the interior
            [(0, 0, S, S), (229, 229, S, S), (P - S, P - S, S, S)] + [around(ir, ic) for ir, ic in iso[:4]],
            [],
            [(0, P - S, S, S)]]
    return tiles, iso, wins


@functools.lru_cache(maxsize=None)
def _sparse_sd(conn):
    """Heads calibrated on one window of every non-empty tile together (the head outputs drift with the footprint's shape: a
    calibration on one footprint leaves the others with a single class)."""
    from bathymetric_gnn_amd import synthetic
    tiles, _, wins = _sparse_tiles()
    ogs = []
    for i, ws in enumerate(wins):
        if ws:
            r0, c0, h, w = ws[-1]
            ogs.append(graph_cpu.build_graph(tiles[i][0][r0:r0 + h, c0:c0 + w], tiles[i][1][r0:r0 + h, c0:c0 + w], None, RES, connectivity=conn))
    x, ei, ea, _, _ = graph_cpu.batch_graphs(ogs)
    return calibrate_heads(synthetic.synthetic_state_dict(seed=1234), x, ei, ea)


@functools.lru_cache(maxsize=None)
def _sparse_reference(i, conn):
    tiles, _, wins = _sparse_tiles()
    d, m = tiles[i]
    return wo.windowed_reference(d, m, None, RES, _sparse_sd(conn), conn, wins[i])


def _same_bits(a, b):
    return all(np.array_equal(a[k].view(np.uint32), b[k].view(np.uint32)) for k in ("classification", "confidence", "correction"))


def test_sparse_uniform_batch(gpu_device):
    from bathymetric_gnn_amd.data import GraphBuilder
    from bathymetric_gnn_amd.models.pipeline import TileBatchEngine
    tiles, iso, _ = _sparse_tiles()
    conn = "8-connected"
    eng = TileBatchEngine(_model(_sparse_sd(conn)), GraphBuilder(connectivity=conn), gpu_device)
    infer = lambda e, idx: e.infer([tiles[i][0] for i in idx], [tiles[i][1] for i in idx], None, [RES] * len(idx))
    every = list(range(len(tiles)))
    res = infer(eng, every)
    assert all(_same_bits(a, b) for a, b in zip(res, infer(eng, every)))                      # the batch twice: the same bits
    rest = [i for i in every if i != EMPTY]
    assert all(_same_bits(res[i], b) for i, b in zip(rest, infer(eng, rest)))                 # ... without the empty tile
    for i in every:
        assert _same_bits(res[i], infer(eng, [i])[0]), i                                      # ... and every tile alone
        for k in ("classification", "confidence", "correction"):
            assert not res[i][k][~tiles[i][1]].any(), (i, k)                                  # invalid cells (all of tile 4) are 0
            assert np.isfinite(res[i][k]).all()
    refs = {i: _sparse_reference(i, conn) for i in rest}
    _assert_mixed({k: torch.cat([refs[i][1][k] for i in rest]) for k in ("predicted_class", "confidence")})
    for i in rest:
        r32, r64, rows, cols = refs[i]
        _check(f"sparse/{conn}/tile{i}", _cells_at(res[i], rows, cols), r32, r64, GRID_KEYS)
    # the diagonal + isolated-cell tile under 4-connectivity: every node has degree 0, the softmax runs over the self loop alone
    conn = "4-connected"
    d, m = tiles[3]
    og = graph_cpu.build_graph(d, m, None, RES, connectivity=conn)
    assert og.num_nodes == P + 200 and og.num_edges == 0
    eng4 = TileBatchEngine(_model(_sparse_sd(conn)), GraphBuilder(connectivity=conn), gpu_device)
    res4 = infer(eng4, every)
    r32, r64, rows, cols = _sparse_reference(3, conn)
    assert len(rows) > 100
    _check(f"sparse/{conn}/tile3", _cells_at(res4[3], rows, cols), r32, r64, GRID_KEYS)
    assert _same_bits(res4[3], infer(eng4, [3])[0]) and not any(res4[EMPTY][k].any() for k in res4[EMPTY])
    assert not res4[3]["confidence"][~m].any() and (res4[3]["confidence"][m] > 0).all()
    assert all(res4[3]["confidence"][ir, ic] > 0 for ir, ic in iso)


# ---- 4. BathymetricPipeline(Config()) with nothing overridden ----------------------------------------------------------
SH, SW = 1920, 2000
TENTH = T * T // 10                       # 104 857: 104 857 / 1 048 576 < 0.1 <= 104 858 / 1 048 576
SKIPPED_ONLY = (100, 200)                 # a valid cell that only the skipped tile covers
SURVEY_REGIONS = [(990, 1200), (940, 990), (300, 1400), (1180, 80), (500, 950), (SH - S, SW - S)]     # 64 x 64, survey coordinates


def _fill_to(valid, tile, count, row0, col0, width=300):
    """Make ``valid[tile]`` hold exactly ``count`` valid cells by filling rows of ``width`` cells from (row0, col0) down."""
    need = count - int(valid[tile].sum())
    assert need > 0
    full, part = divmod(need, width)
    assert not valid[row0:row0 + full + 1, col0:col0 + width].any()
    valid[row0:row0 + full, col0:col0 + width] = True
    valid[row0 + full, col0:col0 + part] = True
    assert int(valid[tile].sum()) == count


@functools.lru_cache(maxsize=None)
def _survey():
    """1920 x 2000: valid right of a ragged boundary near column 960 (3 % iid holes), plus a patch in the top-left tile's own
    area that brings that tile to 104 857 valid cells and one in the bottom-left tile's own area that brings it to 104 858."""
    from bathymetric_gnn_amd import synthetic
    d, _, _ = synthetic.synthetic_tile(SH, SW, 41, "V0")
    r = np.arange(SH)[:, None]; c = np.arange(SW)[None, :]
    edge = 960 + np.round(40 * np.sin(r / 37.0) + 15 * np.sin(r / 5.3)).astype(np.int64)
    valid = (c >= edge) & (np.random.default_rng(3).random((SH, SW)) >= 0.03)
    valid[330, 1430] = valid[331, 1430] = False                           # (NaN / inf depths below)
    top_left, bottom_left = (slice(0, T), slice(0, T)), (slice(SH - T, SH), slice(0, T))
    _fill_to(valid, top_left, TENTH, SKIPPED_ONLY[0], SKIPPED_ONLY[1])
    _fill_to(valid, bottom_left, TENTH + 1, 1200, 100)
    d = np.where(valid, d, NODATA).astype(np.float32)
    d[330, 1430], d[331, 1430] = np.nan, np.inf
    return d, valid


@functools.lru_cache(maxsize=None)
def _survey_sd():
    from bathymetric_gnn_amd import synthetic
    d, valid = _survey()
    cr = (slice(960, 1024), slice(1000, 1064))
    og = graph_cpu.build_graph(d[cr], valid[cr], None, RES)
    return calibrate_heads(synthetic.synthetic_state_dict(seed=1234), og.x, og.edge_index, og.edge_attr)


@functools.lru_cache(maxsize=None)
def _survey_reference():
    """The stitched float32 / float64 oracle maps on the cells where every covering kept tile's windowed oracle is trusted: per
    kept tile the windowed oracle of every region (window coordinates relative to that tile: its own edges count as edges),
    merged by the host TileMerger (the float64 one on float64 grids)."""
    from bathymetric_gnn_amd.data import BathymetricGrid, TileManager, TileMerger
    d, valid = _survey()
    sd, conn = _survey_sd(), "8-connected"
    R = wo.reach(LAYERS, conn)
    grid = BathymetricGrid(depth=d, nodata_value=1.0e6, resolution=RES)
    tm = TileManager()
    _, _, specs = tm.compute_tile_grid(grid.shape)
    by_pos = {(s.tile_row, s.tile_col): s for s in specs}
    chans = ["classification", "confidence", "correction"]
    mergers = {}
    for dt in (np.float32, np.float64):
        mergers[dt] = TileMerger(tm); mergers[dt].initialize(grid.shape, chans, {k: dt for k in chans})
    cover = np.zeros(grid.shape, np.int32); given = np.zeros(grid.shape, np.int32)
    unsure = np.zeros(grid.shape, bool)
    c1 = np.full(grid.shape, -1.0); c2 = c1.copy(); kmin = np.full(grid.shape, 9.0); kmax = np.full(grid.shape, -1.0)
    d32_logits, tile_runs = 0.0, []
    kept = list(tm.iterate_tiles(grid))
    for t in kept:
        wins = []
        for rr, cc in SURVEY_REGIONS:
            a, b = max(rr, t.row_start), min(rr + S, t.row_end)
            e, f = max(cc, t.col_start), min(cc + S, t.col_end)
            if a < b and e < f:
                wins.append((a - t.row_start, e - t.col_start, b - a, f - e))
        runs = [wo.window_forward(t.data, t.valid_mask, None, RES, sd, conn, w) for w in wins]
        tile_runs.append((wins, runs))
        for _, o32, o64 in runs:
            if o64 is not None:
                d32_logits = max(d32_logits, distances(o32, o64, ("class_logits",))["class_logits"])
    sure_gap = 10 * (BOUND_C * d32_logits + BOUND_FLOOR)                   # float64_bound's rule for a sure class
    for t, (wins, runs) in zip(kept, tile_runs):
        sp = by_pos[(t.tile_row, t.tile_col)]
        sl = (slice(sp.row_start, sp.row_end), slice(sp.col_start, sp.col_end))
        cover[sl] += 1
        grids = {dt: {k: np.full(t.shape, np.nan, dt) for k in chans} for dt in mergers}
        sure_t = np.ones(t.shape, bool)
        for w, (og, o32, o64) in zip(wins, runs):
            tr = wo.trusted(w, t.shape, R)
            wsl = (slice(w[0], w[0] + w[2]), slice(w[1], w[1] + w[3]))
            keep = tr[og.valid_rows, og.valid_cols] if o64 is not None else None
            for dt, o in ((np.float32, o32), (np.float64, o64)):
                for k, key in (("classification", "predicted_class"), ("confidence", "confidence"), ("correction", "correction")):
                    sub = grids[dt][k][wsl]
                    sub[tr] = 0.0                                          # a cell without a node: process_tile's fill
                    if o is not None:
                        sub[og.valid_rows[keep], og.valid_cols[keep]] = o[key].numpy()[keep].astype(dt)
            if o64 is not None:
                top2 = torch.topk(o64["class_probs"], 2, dim=-1).values
                gap_ok = ((top2[:, 0] - top2[:, 1]) > sure_gap).numpy()
                sure_t[wsl][og.valid_rows[keep], og.valid_cols[keep]] = gap_ok[keep]
        have = np.isfinite(grids[np.float64]["confidence"])
        given[sl] += have
        unsure[sl] |= have & ~sure_t
        cf = np.where(have, grids[np.float64]["confidence"], -1.0); kk = grids[np.float64]["classification"]
        c2[sl] = np.maximum(c2[sl], np.minimum(c1[sl], cf)); c1[sl] = np.maximum(c1[sl], cf)
        kmin[sl] = np.where(have, np.minimum(kmin[sl], kk), kmin[sl]); kmax[sl] = np.where(have, np.maximum(kmax[sl], kk), kmax[sl])
        for dt in mergers:
            mergers[dt].add_tile(sp, grids[dt])
    ref32, ref64 = mergers[np.float32].finalize(), mergers[np.float64].finalize()
    comparable = (cover > 0) & (given == cover)
    return ref32, ref64, comparable, unsure, c1, c2, kmin, kmax, specs, len(kept)


def test_default_config_pipeline_on_a_ragged_survey(gpu_device):
    from bathymetric_gnn_amd.config import Config
    from bathymetric_gnn_amd.data import BathymetricGrid, TileManager
    from bathymetric_gnn_amd.models import BathymetricPipeline
    cfg = Config()
    assert (cfg.tile.tile_size, cfg.tile.overlap, cfg.tile.min_valid_ratio) == (1024, 128, 0.1)
    d, valid = _survey()
    grid = BathymetricGrid(depth=d, nodata_value=1.0e6, resolution=RES)
    assert np.array_equal(grid.valid_mask, valid)
    pipe = BathymetricPipeline(cfg)                                           # nothing overridden
    assert SH * SW < pipe.STREAM_MIN_CELLS
    _, _, specs = pipe.tile_manager.compute_tile_grid(grid.shape)
    assert [(s.row_start, s.col_start, s.row_end, s.col_end) for s in specs] == \
        [(r0, c0, r0 + T, c0 + T) for r0 in (0, 896) for c0 in (0, 896, 976)]      # two tile rows, the last column shifted back
    counts = [int(valid[s.row_start:s.row_end, s.col_start:s.col_end].sum()) for s in specs]
    assert counts[0] == TENTH and counts[3] == TENTH + 1 and counts[3] < 0.5 * T * T and min(counts[1:]) == counts[3]
    kept = list(TileManager().iterate_tiles(grid))
    assert [(t.tile_row, t.tile_col) for t in kept] == [(0, 1), (0, 2), (1, 0), (1, 1), (1, 2)]
    covered = np.zeros(valid.shape, bool)
    for t in kept:
        covered[t.row_start:t.row_end, t.col_start:t.col_end] = True
    assert valid[SKIPPED_ONLY] and not covered[SKIPPED_ONLY]
    pipe.set_model(_model(_survey_sd()))
    res = pipe.process_grid(grid)                                             # resident survey, device stitch
    assert pipe.last_tile_counts == (len(kept), len(specs) - len(kept)) == (5, 1)
    pipe.host_stitch = True
    res_host = pipe.process_grid(grid)                                        # numpy TileMerger on the same per-tile grids
    pipe.host_stitch = False
    streamed = pipe.process_grid_streamed(grid, band_tile_rows=1)
    assert pipe.last_tile_counts == (5, 1)
    for k in res_host:
        assert np.array_equal(np.isnan(res[k]), np.isnan(res_host[k])), k
        assert np.array_equal(np.nan_to_num(res[k]).view(np.uint32), np.nan_to_num(res_host[k]).view(np.uint32)), k   # every bit
        assert res[k].shape == d.shape and np.array_equal(res[k].view(np.uint32), streamed[k].view(np.uint32)), k
    unproc = valid & ~covered
    assert unproc[SKIPPED_ONLY] and np.all(res["classification"][unproc] == 0) and np.all(res["confidence"][unproc] == 0)
    assert np.array_equal(res["cleaned_depth"][unproc], d[unproc])
    assert np.isnan(res["classification"][~valid & ~covered]).all() and not np.isnan(res["classification"][covered]).any()
    # against float64
    ref32, ref64, comparable, unsure, c1, c2, kmin, kmax, ref_specs, n_kept = _survey_reference()
    assert n_kept == 5 and comparable.sum() > 10000
    bound = {}
    for k in GRID_KEYS:
        e = float(np.abs(res[k][comparable].astype(np.float64) - ref64[k][comparable]).max())
        e32 = float(np.abs(ref32[k][comparable].astype(np.float64) - ref64[k][comparable]).max())
        bound[k] = BOUND_C * e32 + BOUND_FLOOR
        print(f"survey/{k}: cells {int(comparable.sum())} dist {e:.3e} float32_dist {e32:.3e} ratio {e / e32:.3f} bound {bound[k]:.3e}")
        assert e <= bound[k], (k, e, e32)
    pv = comparable & valid
    decided = pv & ~unsure & ((kmin == kmax) | (c1 - c2 > 2 * bound["confidence"]))
    print(f"survey/classes: decided {decided[pv].mean():.3f} of {int(pv.sum())}, tiles disagree on {int((pv & (kmin != kmax)).sum())}")
    assert decided[pv].mean() > 0.9
    assert (pv & (kmin != kmax)).sum() >= 20, "label arbitration between overlapping tiles is exercised"
    assert len(np.unique(ref64["classification"][pv])) >= 2
    assert np.array_equal(res["classification"][decided].astype(np.float64), ref64["classification"][decided])
    fire = pv & (ref64["classification"] == 2) & (ref64["confidence"] > 0.85)
    safe = decided & (np.abs(ref64["confidence"] - 0.85) > bound["confidence"])
    assert (fire & safe).sum() >= 20 and (~fire & safe).sum() >= 20
    exp = np.where(fire, d.astype(np.float64) - ref64["correction"], d.astype(np.float64))
    err = np.abs(res["cleaned_depth"][safe].astype(np.float64) - exp[safe])
    # depth - correction is rounded to float32 once more: half an ulp of the result on top of the correction's bound
    assert np.all(err <= bound["correction"] + 0.5 * np.spacing(np.abs(exp[safe]).astype(np.float32))), float(err.max())
    assert np.array_equal(res["cleaned_depth"][safe & ~fire], d[safe & ~fire])
