"""The helpers of tests/_conditioning.py on the CPU: the BatchNorm fit is a fit, and the float64 bound rule tells a defective
forward from float32 rounding at every depth band.

The defects are run through the float32 oracle itself (patched for the one call): ``h1`` rounded to bf16, layer 0's
BatchNorm shift held in bf16, one in-neighbour dropped per node -- each is rejected at every band and under both fits.  The
controls are accepted: the clean float32 oracle, the float32 oracle summing its neighbourhoods in another order, and the
float32 oracle with layer 0's BatchNorm folded in float32 as ``x * sc + (bb - rm * sc)``.  That fold is the form the
library's kernels apply (scale and shift stored as float32), and at these weights it stays within float32's own rounding
of the float64 forward (a ratio of ~1 at every band): it is no defect, and the rule must not reject it."""
import contextlib

import numpy as np
import pytest
import torch

from _conditioning import BOUND_C, DEPTH_BANDS, deep_tile, distances, fit_batchnorm, float64_bound
from oracle import gat_cpu, graph_cpu

RES = (0.5, 0.5)


def _graphs(hw=(32, 32), bands=DEPTH_BANDS, seed=3):
    return [graph_cpu.build_graph(*deep_tile(hw[0], hw[1], seed + i, "V1", b)[:2], None, RES) for i, b in enumerate(bands)]


@contextlib.contextmanager
def _patched(name, make):
    old = getattr(gat_cpu, name)
    setattr(gat_cpu, name, make(old))
    try:
        yield
    finally:
        setattr(gat_cpu, name, old)


def _bf16(t):
    return t.to(torch.bfloat16).to(t.dtype)


def _h1_bf16(old):
    def mlp2(x, sd, p0, p1, dtype, hidden_mult=None):
        y = old(x, sd, p0, p1, dtype, hidden_mult)
        return _bf16(y) if p0 == "feature_extractor.mlp.0" else y
    return mlp2


def _bn0(shift_round):
    """layer 0's BatchNorm as x * sc + (bb - rm * sc) in float32, the shift passed through ``shift_round``."""
    def make(old):
        def bn(x, sd, prefix, dtype, eps=1e-5):
            if prefix != "gnn.norms.0.module.":
                return old(x, sd, prefix, dtype, eps)
            t = lambda k: gat_cpu._t(sd[prefix + k], torch.float32)
            sc = t("weight") / torch.sqrt(t("running_var") + eps)
            return x * sc + shift_round(t("bias") - t("running_mean") * sc)
        return bn
    return make


def _drop_first_in_edge(ei):
    keep = np.ones(ei.shape[1], bool)
    keep[np.unique(ei[1], return_index=True)[1]] = False
    return keep


def _run(sd, og, variant):
    x, ei, ea = og.x, og.edge_index, og.edge_attr
    if variant == "clean":
        return gat_cpu.forward(sd, x, ei, ea)
    if variant == "edges_reversed":
        return gat_cpu.forward(sd, x, ei[:, ::-1].copy(), ea[::-1].copy())
    if variant == "bn0_fold_float32":
        with _patched("batch_norm_eval", _bn0(lambda s: s)):
            return gat_cpu.forward(sd, x, ei, ea)
    if variant == "h1_bf16":
        with _patched("_mlp2", _h1_bf16):
            return gat_cpu.forward(sd, x, ei, ea)
    if variant == "bn0_shift_bf16":
        with _patched("batch_norm_eval", _bn0(_bf16)):
            return gat_cpu.forward(sd, x, ei, ea)
    if variant == "drop_one_neighbour":
        keep = _drop_first_in_edge(ei)
        return gat_cpu.forward(sd, x, ei[:, keep], ea[keep])
    raise ValueError(variant)


@pytest.fixture(scope="module")
def band_setups():
    """(band, fit) -> (sd, oracle graph, float64 forward, float32 forward): 32 x 32 tiles, BatchNorm fitted across all bands
    or on the band's tile alone."""
    from bathymetric_gnn_amd import synthetic
    sd0 = synthetic.synthetic_state_dict(seed=1234)
    ogs = _graphs()
    sd_all = fit_batchnorm(sd0, ogs)
    out = {}
    for b, og in zip(DEPTH_BANDS, ogs):
        for fit, sd in (("across", sd_all), ("per_band", fit_batchnorm(sd0, [og]))):
            ref64 = gat_cpu.forward(sd, og.x, og.edge_index, og.edge_attr, dtype=torch.float64)
            out[b, fit] = (sd, og, ref64, gat_cpu.forward(sd, og.x, og.edge_index, og.edge_attr))
    return out


@pytest.mark.parametrize("kind", ["GAT", "GCN", "GraphSAGE", "GIN"])
def test_fit_batchnorm_normalises_the_fitting_batch(kind):
    """On the fitting batch, every layer's float64 post-BatchNorm output has per-channel mean ``bias`` and variance
    ``weight^2 var / (var + eps)``: the running statistics are that layer's batch statistics, layer by layer."""
    from bathymetric_gnn_amd import synthetic
    sd0 = synthetic.synthetic_state_dict(gnn_type=kind, num_layers=4 if kind == "GAT" else 3, seed=5)
    ogs = _graphs(hw=(24, 24), bands=(-20.0, -1000.0, -10000.0), seed=11)
    sd = fit_batchnorm(sd0, ogs, calibrate=False, stat_dtype=np.float64)
    for k in sd0:
        if ".norms." not in k or not k.endswith(("running_mean", "running_var")):
            assert sd[k] is sd0[k], k                           # nothing else changes
    post = []

    def record(old):
        def bn(x, sd_, prefix, dtype, eps=1e-5):
            y = old(x, sd_, prefix, dtype, eps)
            post.append((prefix, y))
            return y
        return bn
    x, ei, ea, _, _ = graph_cpu.batch_graphs(ogs)
    with _patched("batch_norm_eval", record):
        gat_cpu.forward(sd, x, ei, ea, dtype=torch.float64)
    L = gat_cpu.num_layers_of(sd)
    assert [p for p, _ in post] == [f"gnn.norms.{l}.module." for l in range(L)]
    for prefix, y in post:
        w, b, rv = (torch.as_tensor(np.asarray(sd[prefix + k], np.float64)) for k in ("weight", "bias", "running_var"))
        var_expected = w ** 2 * rv / (rv + 1e-5)
        scale = b.abs() + var_expected.sqrt()
        assert ((y.mean(0) - b).abs() <= 1e-9 * scale).all(), prefix
        assert ((y.var(0, unbiased=False) - var_expected).abs() <= 1e-9 * var_expected).all(), prefix
    # the common mode is really there: fitted on the -10000 m tile alone, layer 0's mean is large against its spread
    sd1 = fit_batchnorm(sd0, ogs[-1:], calibrate=False)
    rm, rv = (np.asarray(sd1[f"gnn.norms.0.module.{k}"]) for k in ("running_mean", "running_var"))
    assert np.max(np.abs(rm) / np.sqrt(rv)) > 3


def test_fit_batchnorm_calibrates_the_heads():
    from bathymetric_gnn_amd import synthetic
    ogs = _graphs(hw=(32, 32), bands=(-4000.0,))
    sd = fit_batchnorm(synthetic.synthetic_state_dict(seed=1234), ogs)
    ref = gat_cpu.predict(sd, ogs[0].x, ogs[0].edge_index, ogs[0].edge_attr)
    assert torch.unique(ref["predicted_class"]).numel() == 3
    assert set(torch.unique(ref["action"]).tolist()) == {0, 1, 2}


def test_deep_tile_shifts_valid_cells_only():
    from bathymetric_gnn_amd import synthetic
    d0, m0, _ = synthetic.synthetic_tile(40, 30, 7, "V1")
    d, m, _ = deep_tile(40, 30, 7, "V1", -4000.0)
    assert np.array_equal(m, m0) and np.all(d[~m] == np.float32(synthetic.NODATA))
    assert abs(float(np.median(d[m] - d0[m])) + 3980.0) < 0.01
    ds, _, _ = deep_tile(40, 30, 7, "V1", -4000.0, slope=0.05)
    assert abs(float(ds[m][0] - d[m][0])) < 1e-3 and float(np.max(np.abs(ds[m] - d[m]))) > 1.5


CONTROLS = ("clean", "edges_reversed", "bn0_fold_float32")
DEFECTS = ("h1_bf16", "bn0_shift_bf16", "drop_one_neighbour")


@pytest.mark.parametrize("fit", ["across", "per_band"])
@pytest.mark.parametrize("band", DEPTH_BANDS)
def test_bound_rule_rejects_defects_and_accepts_float32_rounding(band, fit, band_setups):
    sd, og, ref64, ref32 = band_setups[band, fit]
    ratios = {}
    for variant in CONTROLS + DEFECTS:
        ok, rep = float64_bound(_run(sd, og, variant), ref32, ref64)
        ratios[variant] = max(rep[k]["dist"] / max(rep[k]["float32_dist"], 1e-300) for k in ("class_logits", "hidden"))
        if variant in CONTROLS:
            assert ok, (variant, rep)
        else:
            assert not ok, (variant, rep)
            assert ratios[variant] > 10 * BOUND_C, (variant, rep)     # rejected by a wide margin, not by luck
    print(f"{band:8g} m {fit:9s} dist / float32 dist: " + "  ".join(f"{k} {v:.3g}" for k, v in ratios.items()))


def test_float32_distance_to_float64_per_band(band_setups):
    """The table of the regime: the float32 oracle's distance to the float64 forward per band and fit.  Fitted per band, it
    grows by two orders of magnitude from -20 m to -10000 m -- the amplification the deep tests are built on."""
    rows = {}
    for (band, fit), (sd, og, ref64, ref32) in sorted(band_setups.items()):
        d = distances(ref32, ref64)
        rng = float(ref64["class_logits"].max() - ref64["class_logits"].min())
        rows[band, fit] = d
        print(f"{band:8g} m {fit:9s} float32 vs float64: " + "  ".join(f"{k} {v:.2e}" for k, v in d.items())
              + f"   logit range {rng:.3f}")
    assert rows[-10000.0, "per_band"]["class_logits"] > 30 * rows[-20.0, "per_band"]["class_logits"]
    assert rows[-4000.0, "per_band"]["hidden"] > 30 * rows[-20.0, "per_band"]["hidden"]
