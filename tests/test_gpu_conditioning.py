"""The forward at survey depths with trained-like BatchNorm statistics, against the float64 oracle.

Every other forward test runs near -20 m with BatchNorm statistics drawn at random.  Depth enters the model raw, and a trained
model's layer-0 ``running_mean`` tracks the depth-driven common mode of its pre-BatchNorm activations, so its BatchNorm
subtracts two large, nearly equal numbers: float32 arithmetic itself sits 1e-4 .. 1e-3 from the true logits at -4000 m.  Here
the inputs are ``_conditioning.deep_tile`` grids at -20 .. -10000 m and the models carry ``fit_batchnorm`` statistics,
fitted either across all bands (a model trained on many surveys) or on the band alone (the worst case).  Every output is held
to ``_conditioning.float64_bound``: within ``BOUND_C`` x the float32 oracle's own distance to the float64 forward.  Where the
float32 oracle is within 2e-5 of float64, the 1e-4 bar against it applies as well.  Every figure is printed; with
BGNN_ACCURACY_DIR naming a writable directory they also go to conditioning_accuracy.json there."""
import functools
import json
import os

import numpy as np
import pytest
import torch

from _calibration import calibrate_heads
from _conditioning import BOUND_C, DEPTH_BANDS, deep_tile, distances, fit_batchnorm, float64_bound
from oracle import gat_cpu, graph_cpu

pytestmark = pytest.mark.gpu
TOL = 1e-4
RES = (0.5, 0.5)
FITS = ("across", "per_band")
HW = (48, 48)
REPORT = {}


@pytest.fixture(scope="module", autouse=True)
def _write_report():
    yield
    out_dir = os.environ.get("BGNN_ACCURACY_DIR", "")
    if REPORT and out_dir and os.path.isdir(out_dir) and os.access(out_dir, os.W_OK):
        with open(os.path.join(out_dir, "conditioning_accuracy.json"), "w") as f:
            json.dump(REPORT, f, indent=1, sort_keys=True)


@pytest.fixture(autouse=True)
def _exact_path_after():
    yield
    if torch.cuda.is_available():
        _ctx().set_option("matrix_path", "exact_f32")


def _ctx():
    from bathymetric_gnn_amd import runtime as rt
    return rt.get_context(torch.device("cuda:0"))


def _record(name, row):
    REPORT[name] = row
    print(name, json.dumps(row))


@functools.lru_cache(maxsize=None)
def _band_tile(band, conn="8-connected", unc=False, hw=HW, seed=3, variant="V1"):
    d, m, u = deep_tile(hw[0], hw[1], seed + int(-band) % 97, variant, band, with_uncertainty=unc)
    return d, m, u, graph_cpu.build_graph(d, m, u, RES, connectivity=conn)


@functools.lru_cache(maxsize=None)
def _fitted(kind="GAT", fit="across", band=None, conn="8-connected", unc=False, calibrate=True):
    """Synthetic weights with BatchNorm fitted across all bands' tiles, or on ``band``'s tile alone."""
    from bathymetric_gnn_amd import synthetic
    layers = 4 if kind == "GAT" else 3
    sd = synthetic.synthetic_state_dict(in_channels=8 if unc else 7, gnn_type=kind, num_layers=layers, seed=1234)
    bands = DEPTH_BANDS if fit == "across" else (band,)
    return fit_batchnorm(sd, [_band_tile(b, conn, unc)[3] for b in bands], calibrate=calibrate)


def _model(sd, kind="GAT", unc=False):
    from bathymetric_gnn_amd.models import BathymetricGNN
    m = BathymetricGNN(in_channels=8 if unc else 7, gnn_type=kind, num_gnn_layers=4 if kind == "GAT" else 3, edge_dim=3,
                       dropout=0.0)
    m.load_state_dict({k: torch.as_tensor(v) for k, v in sd.items()})
    return m.to(torch.device("cuda:0")).eval()


def _refs(sd, x, ei, ea):
    """(float32 oracle with the deployment flags, float64 oracle)"""
    return gat_cpu.predict(sd, x, ei, ea), gat_cpu.forward(sd, x, ei, ea, dtype=torch.float64)


def _check(name, out, ref32, ref64, keys=("class_logits", "confidence", "correction", "hidden")):
    ok, rep = float64_bound(out, ref32, ref64, keys=keys)
    _record(name, rep)
    assert ok, (name, rep)
    return rep


def _old_contract(out, ref32):
    """The 1e-4 bar against the float32 oracle (test_gpu_forward._compare) where the float32 oracle itself is within 2e-5 of
    float64: nothing gets weaker where the old contract applies."""
    from test_gpu_forward import _compare
    _compare(out, ref32, require_mixed=False)


# ---- a. predict() per tile, every band x fit, with and without the uncertainty channel ---------------------------------
@pytest.mark.parametrize("unc", [False, True])
@pytest.mark.parametrize("fit", FITS)
@pytest.mark.parametrize("band", DEPTH_BANDS)
def test_predict_at_depth_against_float64(band, fit, unc, gpu_device):
    from bathymetric_gnn_amd.data import GraphBuilder
    d, m, u, og = _band_tile(band, unc=unc)
    sd = _fitted("GAT", fit, band, unc=unc)
    model = _model(sd, unc=unc)
    g = GraphBuilder().build_graph(d, m, u, RES)
    out = model.predict(g)
    hid = model._run(g, 0.85, 0.6, with_flags=False, want_hidden=True)          # the backbone output too
    ref32, ref64 = _refs(sd, og.x, og.edge_index, og.edge_attr)
    name = f"a_{band:g}m_{fit}{'_unc' if unc else ''}"
    rep = _check(f"{name}_predict", out, ref32, ref64)
    _check(f"{name}_hidden", hid, ref32, ref64)
    # (per output: the backbone output's float32 distance is ~20 x the logits')
    if rep["class_logits"]["float32_dist"] < 2e-5:
        _old_contract(out, ref32)
    if distances(ref32, ref64, ("hidden",))["hidden"] < 2e-5:
        assert (hid["hidden"].cpu() - ref32["hidden"]).abs().max().item() < TOL


# ---- b. the tile routes of the fused kernels at -4000 m ---------------------------------------------------------------
def _grid_refs(sd, og):
    """float32 / float64 oracle outputs as the tile routes return them: per valid cell, correction de-normalised by
    max(local_std, 0.01) (models/pipeline.py:_process_tile)."""
    ref32, ref64 = _refs(sd, og.x, og.edge_index, og.edge_attr)
    ls = np.maximum(og.local_std, np.float32(0.01))
    ref32 = dict(ref32, correction=ref32["correction"] * torch.from_numpy(ls))
    ref64 = dict(ref64, correction=ref64["correction"] * torch.from_numpy(ls.astype(np.float64)))
    return ref32, ref64


def _grid_out(r, og):
    rr, cc = og.valid_rows, og.valid_cols
    return {"predicted_class": torch.from_numpy(r["classification"][rr, cc]).long(),
            "confidence": torch.from_numpy(r["confidence"][rr, cc]),
            "correction": torch.from_numpy(r["correction"][rr, cc])}


def _check_grid(name, r, sd, og):
    ref32, ref64 = _grid_refs(sd, og)
    _check(name, _grid_out(r, og), ref32, ref64, keys=("confidence", "correction"))
    mask = np.zeros(og.grid_shape, bool); mask[og.valid_rows, og.valid_cols] = True
    for k in ("classification", "confidence", "correction"):
        assert not r[k][~mask].any(), k                                     # cells without a node stay 0


@pytest.mark.parametrize("conn", ["8-connected", "4-connected", "16-dilated"])
def test_tile_batch_uniform_at_4000m(conn, gpu_device):
    from bathymetric_gnn_amd.data import GraphBuilder
    from bathymetric_gnn_amd.models.pipeline import TileBatchEngine
    band = -4000.0
    sd = _fitted("GAT", "per_band", band, conn)
    tiles = [deep_tile(HW[0], HW[1], 60 + i, "V1", band) for i in range(3)]
    eng = TileBatchEngine(_model(sd), GraphBuilder(connectivity=conn), gpu_device)
    res = eng.infer([t[0] for t in tiles], [t[1] for t in tiles], None, [RES] * len(tiles))
    for i, (t, r) in enumerate(zip(tiles, res)):
        og = graph_cpu.build_graph(t[0], t[1], None, RES, connectivity=conn)
        _check_grid(f"b_tiles_uniform_{conn}_{i}", r, sd, og)


def test_tile_batch_ragged_all_bands_equals_per_grid(gpu_device):
    """One ragged batch holding a grid of every band (the canvas walk), model fitted across the bands: every grid within
    the bound and bit-equal to the same grid inferred alone."""
    from bathymetric_gnn_amd.data import GraphBuilder
    from bathymetric_gnn_amd.models.pipeline import TileBatchEngine
    sd = _fitted("GAT", "across")
    shapes = [(37, 45), (20, 64), (48, 48), (23, 31), (40, 29)]
    grids = [deep_tile(h, w, 80 + i, "V1", b) for i, ((h, w), b) in enumerate(zip(shapes, DEPTH_BANDS))]
    eng = TileBatchEngine(_model(sd), GraphBuilder(), gpu_device)
    assert _ctx().get_option("ragged_atlas") == 1
    res = eng.infer([g[0] for g in grids], [g[1] for g in grids], None, [RES] * len(grids))
    for i, (g, r, b) in enumerate(zip(grids, res, DEPTH_BANDS)):
        alone = eng.infer([g[0]], [g[1]], None, [RES])[0]
        for k in ("classification", "confidence", "correction"):
            assert np.array_equal(r[k], alone[k]), (b, k)
        _check_grid(f"b_tiles_ragged_{b:g}m", r, sd, graph_cpu.build_graph(g[0], g[1], None, RES))


@pytest.mark.parametrize("option", ["fused", "fold_extractor"])
def test_unfused_routes_at_4000m(option, gpu_device):
    from bathymetric_gnn_amd.data import GraphBuilder
    band = -4000.0
    d, m, u, og = _band_tile(band)
    sd = _fitted("GAT", "per_band", band)
    model = _model(sd)
    g = GraphBuilder().build_graph(d, m, u, RES)
    with _ctx().options(**{option: 0}):
        out = model._run(g, 0.85, 0.6, with_flags=True, want_hidden=True)
    ref32, ref64 = _refs(sd, og.x, og.edge_index, og.edge_attr)
    _check(f"b_{option}_0", out, ref32, ref64)


def test_big_batch_w_resident_gemm_at_4000m(gpu_device):
    """More than 65 536 nodes in one batch: the W-resident lin_0 GEMM with the extractor's layer 1 fused in front."""
    from bathymetric_gnn_amd.data import GraphBuilder
    band = -4000.0
    sd = _fitted("GAT", "per_band", band)
    model = _model(sd)
    tiles = [deep_tile(120, 120, 90 + i, "V0", band) for i in range(5)]
    g = GraphBuilder().build_graphs([t[0] for t in tiles], [t[1] for t in tiles], None, [RES] * len(tiles))
    assert g.num_nodes > 65536 and _ctx().get_option("fused_front") == 1
    out = model._run(g, 0.85, 0.6, with_flags=True, want_hidden=True)
    ogs = [graph_cpu.build_graph(t[0], t[1], None, RES) for t in tiles]
    x, ei, ea, _, _ = graph_cpu.batch_graphs(ogs)
    ref32, ref64 = _refs(sd, x, ei, ea)
    _check("b_big_batch_w_resident", out, ref32, ref64)


# ---- c. the other backbones (BatchNorm folded into the last linear map) -----------------------------------------------
@pytest.mark.parametrize("kind", ["GCN", "GraphSAGE", "GIN"])
def test_other_backbones_at_4000m(kind, gpu_device):
    from bathymetric_gnn_amd.data import GraphBuilder
    band = -4000.0
    d, m, u, og = _band_tile(band)
    sd = _fitted(kind, "per_band", band)
    model = _model(sd, kind)
    out = model._run(GraphBuilder().build_graph(d, m, u, RES), 0.85, 0.6, with_flags=True, want_hidden=True)
    ref32, ref64 = _refs(sd, og.x, og.edge_index, og.edge_attr)
    _check(f"c_{kind}", out, ref32, ref64)


# ---- d. training-mode forward (batch-statistics BatchNorm) ------------------------------------------------------------
def test_training_mode_forward_at_4000m(gpu_device):
    from bathymetric_gnn_amd.data import GraphBuilder
    band = -4000.0
    sd = _fitted("GAT", "per_band", band)
    model = _model(sd).train()
    tiles = [deep_tile(37, 45, 5, "V1", band), deep_tile(20, 64, 6, "V0", band)]
    g = GraphBuilder().build_graphs([t[0] for t in tiles], [t[1] for t in tiles], None, [RES] * 2)
    out = model(g)
    ogs = [graph_cpu.build_graph(t[0], t[1], None, RES) for t in tiles]
    x, ei, ea, _, _ = graph_cpu.batch_graphs(ogs)
    s32, s64 = {}, {}
    ref32 = gat_cpu.forward(sd, x, ei, ea, train_stats=s32)
    ref64 = gat_cpu.forward(sd, x, ei, ea, dtype=torch.float64, train_stats=s64)
    _check("d_train_forward", out, ref32, ref64, keys=("class_logits", "confidence", "correction"))
    stats = {}
    for l, n in enumerate(model.gnn.norms):
        pre = f"gnn.norms.{l}.module."
        for k, t in (("running_mean", n.module.running_mean), ("running_var", n.module.running_var)):
            e, e32 = distances({"s": t}, {"s": s64[pre + k]}, ("s",))["s"], distances({"s": s32[pre + k]}, {"s": s64[pre + k]}, ("s",))["s"]
            stats[f"{l}.{k}"] = {"dist": e, "float32_dist": e32}
            assert e <= BOUND_C * e32 + 1e-6, (l, k, e, e32)
    _record("d_train_running_stats", stats)


# ---- e. the operand-split matrix paths --------------------------------------------------------------------------------
# What the split paths are held to at depth (include/bgnn.h, matrix_path).  Their operands carry fewer
# significant bits than float32's 24: fp16x3 22 (float16 hi + lo), bf16x3 16 (bf16 hi + lo).  Near -20 m with moderate
# BatchNorm statistics the float32 accumulation dominates and fp16x3 lands within 1.1 x the exact path's distance
# (test_gpu_forward.test_matrix_paths_distance_to_float64 keeps asserting that there); with fitted statistics at depth the
# amplified operand rounding dominates and it does not (measured up to 2.1 x on the max, 4.2 x on the rms).  So:
# fp16x3 is held to float64_bound itself, like the exact path; bf16x3 to the existing 5e-5 plus the float32 oracle's distance
# scaled by the 2^8 ratio of the operand precisions.
BF16X3_PRECISION_RATIO = 2.0 ** (24 - 16)


def _split_rows(model, g, ref32, ref64):
    row = {"float32_oracle": distances(ref32, ref64, ("class_logits",))["class_logits"]}
    outs = {}
    for path in ("exact_f32", "fp16x3", "bf16x3"):
        _ctx().set_option("matrix_path", path)
        outs[path] = model.predict(g)
        e = (outs[path]["class_logits"].double().cpu() - ref64["class_logits"]).abs()
        row[path] = {"max": float(e.max()), "rms": float((e ** 2).mean().sqrt())}
    _ctx().set_option("matrix_path", "exact_f32")
    row["fp16x3_over_exact"] = {k: row["fp16x3"][k] / max(row["exact_f32"][k], 1e-30) for k in ("max", "rms")}
    return row, outs


def _assert_split_claims(row, outs, ref32, ref64):
    keys = ("class_logits", "confidence", "correction")
    for path in ("exact_f32", "fp16x3"):
        ok, rep = float64_bound(outs[path], ref32, ref64, keys=keys)
        assert ok, (path, rep, row)
    assert row["bf16x3"]["max"] < 5e-5 + BF16X3_PRECISION_RATIO * row["float32_oracle"], row


@pytest.mark.parametrize("fit", FITS)
@pytest.mark.parametrize("band", DEPTH_BANDS)
def test_split_matrix_paths_at_depth(band, fit, gpu_device):
    from bathymetric_gnn_amd.data import GraphBuilder
    if not _ctx().get_option("fused"):
        pytest.skip("the split matrix paths live in the fused layer kernels")
    d, m, u, og = _band_tile(band)
    sd = _fitted("GAT", fit, band)
    ref32, ref64 = _refs(sd, og.x, og.edge_index, og.edge_attr)
    row, outs = _split_rows(_model(sd), GraphBuilder().build_graph(d, m, u, RES), ref32, ref64)
    _record(f"e_split_{band:g}m_{fit}", row)
    _assert_split_claims(row, outs, ref32, ref64)


@pytest.mark.parametrize("band", [-20.0, -4000.0])
def test_split_matrix_paths_with_an_outlier_weight(band, gpu_device):
    """A checkpoint-like outlier: one weight 1e3 x its matrix's largest in a hidden layer's lin and in the classification
    head's first layer.  fp16x3 scales each weight image by one power of two (pack_split): the outlier sets it, and the
    other columns' lo parts lose bits.  Measured: within 1.6 x the exact path's max distance (4.2 x the rms) and well inside
    float64_bound; per-column scales were not built (include/bgnn.h, matrix_path)."""
    from bathymetric_gnn_amd.data import GraphBuilder
    d, m, u, og = _band_tile(band)
    sd = dict(_fitted("GAT", "per_band", band, calibrate=False))
    for key, (i, j) in (("gnn.convs.1.lin.weight", (7, 11)), ("classification_head.mlp.0.weight", (3, 5))):
        w = np.array(sd[key], np.float32, copy=True)
        w[i, j] = 1e3 * np.abs(w).max()
        sd[key] = w
    sd = calibrate_heads(sd, og.x, og.edge_index, og.edge_attr)
    ref32, ref64 = _refs(sd, og.x, og.edge_index, og.edge_attr)
    row, outs = _split_rows(_model(sd), GraphBuilder().build_graph(d, m, u, RES), ref32, ref64)
    _record(f"e_split_outlier_{band:g}m", row)
    _assert_split_claims(row, outs, ref32, ref64)


# ---- f. matrix_path = bf16 (activations stored as bf16) ---------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _bf16_case(band, conn):
    """128 x 128 tile at ``band``; BatchNorm fitted across the bands, heads calibrated on this tile (spread 1.0, as
    test_config3_bf16_storage_distance_to_float64) so that its classes are mixed."""
    d, m, _ = deep_tile(128, 128, 1, "V1", band)
    og = graph_cpu.build_graph(d, m, None, RES, connectivity=conn)
    sd = calibrate_heads(_fitted("GAT", "across", conn=conn, calibrate=False), og.x, og.edge_index, og.edge_attr, logit_spread=1.0)
    ref64 = gat_cpu.forward(sd, og.x, og.edge_index, og.edge_attr, dtype=torch.float64)
    return d, m, og, sd, ref64


# Measured on an MI355X (the worse of bf16_layer0_af 1 / 0): with BatchNorm fitted across -20 .. -10000 m, storing the
# un-normalised layer-0 activations as bf16 misses the scaled bound at every band, -20 m included -- h1's common mode is
# 10^2 .. 10^4 x its within-tile variation, and bf16 keeps 8 significant bits.  A precision limit of the storage format
# (include/bgnn.h matrix_path 3), not a kernel defect: strict xfails, so that the day a fix
# (per-tile centring of h1, or a float32 layer 0) makes one pass, the mark has to go.
BF16_MEASURED = {
    (-20.0, "16-dilated"): "max |dlogit| 1.13 vs bound 0.71, agreement on clear nodes 0.58, flips 0.60",
    (-20.0, "8-connected"): "max |dlogit| 2.12 vs bound 1.0, agreement on clear nodes 0.58, flips 0.46",
    (-200.0, "16-dilated"): "max |dlogit| 4.62 vs bound 0.35, agreement on clear nodes 0.99, flips 0.01",
    (-200.0, "8-connected"): "max |dlogit| 5.14 vs bound 0.35, agreement on clear nodes 0.97, flips 0.03",
    (-1000.0, "16-dilated"): "max |dlogit| 6.87 vs bound 0.27, agreement on clear nodes 0.47, flips 0.53",
    (-1000.0, "8-connected"): "max |dlogit| 7.47 vs bound 0.32, agreement on clear nodes 0.85, flips 0.19",
    (-4000.0, "16-dilated"): "max |dlogit| 22.5 vs bound 0.54, agreement on clear nodes 0.17, flips 0.79",
    (-4000.0, "8-connected"): "max |dlogit| 24.2 vs bound 0.80, agreement on clear nodes 0.18, flips 0.78",
    (-10000.0, "16-dilated"): "max |dlogit| 26.7 vs bound 0.65, agreement on clear nodes 0.54, flips 0.49",
    (-10000.0, "8-connected"): "max |dlogit| 36.3 vs bound 0.94, agreement on clear nodes 0.55, flips 0.49",
}


def _bf16_params():
    for band in DEPTH_BANDS:
        for conn in ("16-dilated", "8-connected"):
            for af in (1, 0):
                why = BF16_MEASURED.get((band, conn))
                marks = [pytest.mark.xfail(strict=True, raises=AssertionError, reason=f"bf16 storage at {band:g} m: {why}")] if why else []
                yield pytest.param(band, conn, af, marks=marks, id=f"{band:g}m-{conn}-af{af}")


@pytest.mark.parametrize("band,conn,af", list(_bf16_params()))
def test_bf16_storage_at_depth(band, conn, af, gpu_device):
    from bathymetric_gnn_amd.data import GraphBuilder
    from test_gpu_forward import _bf16_bound, _fp64_distance
    d, m, og, sd, ref64 = _bf16_case(band, conn)
    model = _model(sd)
    g = GraphBuilder(connectivity=conn).build_graph(d, m, None, RES)
    ctx = _ctx()
    exact = model.predict(g)
    with ctx.options(matrix_path="bf16", bf16_layer0_af=af):
        out = model.predict(g)
    e_exact, e_bf16 = _fp64_distance(exact, ref64), _fp64_distance(out, ref64)
    top2 = torch.topk(ref64["class_probs"], 2, dim=-1).values
    clear = (top2[:, 0] - top2[:, 1]) > 0.02
    same = out["predicted_class"].cpu() == ref64["predicted_class"]
    classes = torch.bincount(ref64["predicted_class"], minlength=3).double() / ref64["predicted_class"].numel()
    bound = _bf16_bound(ref64)
    row = {"band_m": band, "connectivity": conn, "layer0_aggregate_first": af, "nodes": int(og.x.shape[0]),
           "logit_abs_max": float(ref64["class_logits"].abs().max()), "logit_bound_scaled": bound,
           "exact_f32": {"max": e_exact[0], "rms": e_exact[1]}, "bf16_storage": {"max": e_bf16[0], "rms": e_bf16[1]},
           "class_agreement_on_clear_nodes": float(same[clear].double().mean()), "clear_fraction": float(clear.double().mean()),
           "class_flip_rate_all_nodes": float((~same).double().mean()), "float64_class_shares": [float(c) for c in classes]}
    _record(f"f_bf16_{band:g}m_{conn}_af{af}", row)
    assert float(classes.min()) > 0.05, row
    assert row["clear_fraction"] >= 0.5, row
    assert e_bf16[0] < bound and e_bf16[1] < bound / 4, row
    assert row["class_agreement_on_clear_nodes"] > 0.98, row
    assert row["class_flip_rate_all_nodes"] < 0.15, row
