"""The multi-task training loss on the host: the fixtures the REFERENCE's own ``training/losses.py`` produced
(tests/golden/make_golden_loss.py -> tests/golden/loss/*.npz), the float64 numpy restatement (tests/_loss_cpu.py) against them, the
package's torch path, the drop-in signatures, the two helpers, and the C side of include/bgnn_loss.h (plain C99, every symbol
exported and bound, the workspace size without a GPU).  No GPU needed.

Bounds.  The restatement is held to the reference's float64 run at 1e-12 relative, for a gradient tensor plus 1e-12 of its
largest |element| (on the saturated row (40, -40, 0) the softmax rounds to exactly 1 and ``p - 1`` cancels: the two float64
evaluations agree to 2e-9 of that element only).  The reference forms feature_preservation and shoal_safety in float32 whatever
its input dtype (one division of exact integers), so its float64 run is compared with ``as_reference`` of the restatement, and the
two terms themselves are held EXACTLY to float32(exact ratio of the fixture's integer counts)."""
import ctypes as C
import glob
import inspect
import json
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

import _loss_cpu as lc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LOSS_DIR = os.path.join(ROOT, "tests", "golden", "loss")
FIXTURES = sorted(p for p in glob.glob(os.path.join(LOSS_DIR, "*.npz")) if not p.endswith("helpers.npz"))
NAMES = [os.path.basename(p)[:-4] for p in FIXTURES]
GRADS = ("class_logits", "confidence", "correction")
REL = 1e-12


def check_values(got, z, rel=REL):
    for k in lc.TERMS:
        want = float(z["ref64_" + k])
        if np.isnan(want):
            assert np.isnan(got[k]), (k, got[k])
        else:
            assert abs(float(got[k]) - want) <= rel * abs(want), (k, float(got[k]), want)


def check_grads(got, z, rel=REL):
    for k in GRADS:
        g = got.get(k)
        if "g64_" + k not in z.files:                 # the reference left .grad None: nothing flowed
            assert g is None or not np.any(g), k
            continue
        want = z["g64_" + k]
        assert g.shape == want.shape
        if want.size:
            err = np.abs(g - want)
            assert (err <= rel * np.abs(want) + rel * np.abs(want).max()).all(), (k, float(err.max()))


# ---- the fixtures -----------------------------------------------------------------------------------------------------------------
def test_fixture_set_covers_the_cases():
    z = {n: np.load(p) for n, p in zip(NAMES, FIXTURES)}
    assert {0, 1, 2, 257, 2049} <= {int(v["n"]) for v in z.values()}
    w = z["n257_weighted_smoothed"]
    assert w["class_weights"].tolist() == np.array([0.4, 1.7, 0.9], np.float32).tolist() and float(w["label_smoothing"]) == 0.1
    assert "class_weights" not in z["n2049_plain"].files and float(z["n2049_plain"]["label_smoothing"]) == 0.0
    assert z["c5"]["class_logits"].shape[1] == 5
    assert not z["no_masked_row"]["noise_mask"].any() and "noise_mask" not in z["no_noise_mask"].files
    assert int(z["no_false_positive"]["n_false_positives"]) == 0 and int(z["n2049_plain"]["n_false_positives"]) > 0
    assert "correction" not in z["no_correction"].files and "correction_targets" not in z["no_correction_targets"].files
    assert int((z["ignored5"]["class_labels"] == -100).sum()) == 5
    s = z["saturated"]
    hit = s["predicted_class"] == s["class_labels"]
    near = np.float32(1.0) - np.float32(2.0 ** -24)
    for v in (np.float32(0.0), np.float32(1.0), near):
        assert {bool(h) for h in hit[s["confidence"] == v]} == {True, False}
    assert s["class_logits"][0].tolist() == [40.0, -40.0, 0.0]
    for n, v in z.items():
        assert os.path.getsize(os.path.join(LOSS_DIR, n + ".npz")) <= 200_000
        assert v["class_logits"].dtype == np.float32 and v["ref32_total"].dtype == np.float32 and v["ref64_total"].dtype == np.float64
        assert v["g32_class_logits"].dtype == np.float32 and v["g64_class_logits"].dtype == np.float64


# ---- the restatement against the reference ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("path", FIXTURES, ids=NAMES)
def test_restatement_reproduces_the_reference(path):
    inp, cfg, z = lc.load_fixture(path)
    exact = lc.loss(inp, cfg)
    for k in lc.TERMS:
        print(k, float(exact[k]), float(z["ref64_" + k]))
    check_values(lc.as_reference(exact, cfg), z)
    check_grads(lc.grads(inp, cfg), z)


@pytest.mark.parametrize("path", FIXTURES, ids=NAMES)
def test_count_terms_are_the_exact_ratio_of_the_counts(path):
    inp, cfg, z = lc.load_fixture(path)
    n, k = int(z["n"]), lc.counts(inp, cfg)
    assert (k["feature_as_noise"], k["false_positives"], k["shoal_false_positives"], k["deep_false_positives"]) == \
        (int(z["n_feature_as_noise"]), int(z["n_false_positives"]), int(z["n_shoal"]), int(z["n_deep"]))
    exact = lc.loss(inp, cfg)
    if n:
        assert float(exact["feature_preservation"]) == 2.0 * k["feature_as_noise"] / n
        fp = k["false_positives"]
        want = (3.0 * k["shoal_false_positives"] + 1.0 * k["deep_false_positives"]) / fp if fp and "correction_targets" in inp else 0.0
        assert float(exact["shoal_safety"]) == want
        for name in ("feature_preservation", "shoal_safety"):
            for ref in ("ref32_", "ref64_"):
                assert float(z[ref + name]) == float(np.float32(exact[name])), (name, ref)
    else:
        assert np.isnan(z["ref64_feature_preservation"]) and float(z["ref64_shoal_safety"]) == 0.0


# ---- the package's torch path -----------------------------------------------------------------------------------------------------
def run_package(inp, cfg, dtype, device="cpu"):
    from bathymetric_gnn_amd.training import BathymetricGNNLoss
    w = None if cfg["class_weights"] is None else torch.as_tensor(np.asarray(cfg["class_weights"])).to(device=device, dtype=dtype)
    crit = BathymetricGNNLoss(class_weights=w, label_smoothing=cfg["label_smoothing"], correction_delta=cfg["delta"])
    outputs = {"predicted_class": torch.as_tensor(inp["predicted_class"]).to(device)}
    leaves = {}
    for k in GRADS:
        if inp.get(k) is not None:
            leaves[k] = outputs[k] = torch.as_tensor(inp[k]).to(device=device, dtype=dtype).requires_grad_(True)
    targets = {"class_labels": torch.as_tensor(inp["class_labels"]).to(device)}
    if inp.get("correction_targets") is not None:
        targets["correction_targets"] = torch.as_tensor(inp["correction_targets"]).to(device=device, dtype=dtype)
    if inp.get("noise_mask") is not None:
        targets["noise_mask"] = torch.as_tensor(inp["noise_mask"]).to(device)
    losses = crit(outputs, targets)
    assert tuple(losses) == lc.TERMS
    losses["total"].backward()
    return crit, losses, {k: (None if v.grad is None else v.grad.detach().cpu().numpy()) for k, v in leaves.items()}


@pytest.mark.parametrize("path", FIXTURES, ids=NAMES)
def test_cpu_path_float32_within_the_references_own_error(path):
    inp, cfg, z = lc.load_fixture(path)
    _, losses, grads = run_package(inp, cfg, torch.float32)
    for k in lc.TERMS:
        v, r32, r64 = losses[k].detach(), float(z["ref32_" + k]), float(z["ref64_" + k])
        assert v.dtype == torch.float32 and v.dim() == 0
        if np.isnan(r64):
            assert np.isnan(float(v)), k
        else:
            assert abs(float(v) - r64) <= abs(r32 - r64) + float(np.spacing(np.float32(abs(r64)))), (k, float(v), r32, r64)
    for k in GRADS:
        if "g64_" + k not in z.files:
            assert grads.get(k) is None or not grads[k].any(), k
            continue
        g, g32, g64 = grads[k].astype(np.float64), z["g32_" + k].astype(np.float64), z["g64_" + k]
        assert (np.abs(g - g64) <= np.abs(g32 - g64) + np.spacing(np.abs(g64).astype(np.float32)).astype(np.float64)).all(), k


@pytest.mark.parametrize("path", FIXTURES, ids=NAMES)
def test_cpu_path_float64_at_the_restatements_bound(path):
    inp, cfg, z = lc.load_fixture(path)
    _, losses, grads = run_package(inp, cfg, torch.float64)
    check_values({k: float(v.detach()) for k, v in losses.items()}, z)
    check_grads(grads, z)


def test_cpu_path_single_terms_and_no_grad():
    inp, cfg, z = lc.load_fixture(os.path.join(LOSS_DIR, "n257_weighted_smoothed.npz"))
    from bathymetric_gnn_amd.training import BathymetricGNNLoss
    crit = BathymetricGNNLoss(class_weights=torch.as_tensor(cfg["class_weights"]), label_smoothing=0.1)
    out = {k: torch.as_tensor(inp[k]) for k in ("class_logits", "confidence", "correction", "predicted_class")}
    tg = {k: torch.as_tensor(inp[k]) for k in ("class_labels", "correction_targets", "noise_mask")}
    with torch.no_grad():
        losses = crit(out, tg)
    assert all(v.grad_fn is None for v in losses.values()) and crit.last_stats is None
    assert float(losses["total"]) == float(z["ref32_total"])


# ---- drop-in surface --------------------------------------------------------------------------------------------------------------
def test_signatures_equal_the_references():
    from bathymetric_gnn_amd import training
    sig = json.load(open(os.path.join(LOSS_DIR, "signatures.json")))

    def params(fn):
        return [[n, None if p.default is inspect.Parameter.empty else p.default] for n, p in inspect.signature(fn).parameters.items()
                if n != "self"]
    for name in ("BathymetricGNNLoss", "ClassificationLoss", "CorrectionLoss", "ConfidenceCalibrationLoss", "FeaturePreservationLoss",
                 "ShoalSafetyLoss"):
        cls = getattr(training, name)
        assert params(cls.__init__) == sig[name]["__init__"], name
        assert params(cls.forward) == sig[name]["forward"], name
    for name in ("compute_class_weights", "compute_correction_delta"):
        assert params(getattr(training, name)) == sig[name], name
    crit = training.BathymetricGNNLoss()
    have = set(vars(crit)) | set(crit._modules)
    assert set(sig["attributes"]) <= have, set(sig["attributes"]) - have
    assert sorted(training.__all__) == sorted(["BathymetricGNNLoss", "ClassificationLoss", "CorrectionLoss", "ConfidenceCalibrationLoss",
                                               "FeaturePreservationLoss", "ShoalSafetyLoss", "compute_class_weights",
                                               "compute_correction_delta"])


def test_helpers_reproduce_their_fixtures():
    from bathymetric_gnn_amd.training import compute_class_weights, compute_correction_delta
    h = np.load(os.path.join(LOSS_DIR, "helpers.npz"))
    for j in range(3):
        nc, sm = h[f"cw{j}_args"]
        w = compute_class_weights(torch.as_tensor(h[f"cw{j}_labels"]), num_classes=int(nc), smoothing=float(sm))
        assert w.dtype == torch.float32 and w.shape == (int(nc),)
        assert np.array_equal(w.numpy(), h[f"cw{j}_weights"])                 # the same float32 operations in the same order
        assert abs(float(w.sum()) - nc) < 1e-5
        pct, md = h[f"cd{j}_args"]
        d = compute_correction_delta(h[f"cd{j}_corrections"], percentile=float(pct), min_delta=float(md))
        assert isinstance(d, float) and d == float(h[f"cd{j}_delta"])
    assert compute_correction_delta(np.zeros(0)) == 1.0 and compute_correction_delta(np.array([0.1, -0.2])) == 1.0
    assert compute_class_weights(torch.tensor([0, 0, 2])).shape == (3,)


# ---- the C side -------------------------------------------------------------------------------------------------------------------
def _declared(name):
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", name)).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(bgnn_[a-z_0-9]+)\s*\(", text)))


@pytest.fixture(scope="module")
def lib():
    from bathymetric_gnn_amd import runtime
    if not os.path.exists(runtime.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return runtime.load_library()


def test_loss_symbols_exported_and_bound(lib):
    from bathymetric_gnn_amd import runtime
    syms = _declared("bgnn_loss.h")
    assert syms == ["bgnn_loss_backward", "bgnn_loss_forward", "bgnn_loss_workspace_bytes"]
    others = set(runtime._SIGNATURES) | set(runtime._TRAIN_SIGNATURES) | set(runtime._SIDECAR_SIGNATURES) | set(runtime._NOISE_SIGNATURES)
    assert not set(syms) & others
    assert sorted(runtime._LOSS_SIGNATURES) == syms
    for s in syms:
        assert hasattr(lib, s), f"{s} declared in bgnn_loss.h but not exported"
    assert lib.bgnn_abi_version() == 7
    text = open(os.path.join(ROOT, "include", "bgnn_loss.h")).read()
    d = dict(re.findall(r"#define BGNN_LOSS_([A-Z_]+) \(?(-?\d+)\)?", text))
    assert int(d["ROWS_PER_WG"]) == runtime.LOSS_ROWS_PER_WG == 256 * int(d["ROWS_PER_THREAD"])
    assert int(d["FINISH_WIDTH"]) == runtime.LOSS_FINISH_WIDTH and int(d["MAX_CLASSES"]) == runtime.LOSS_MAX_CLASSES
    assert int(d["IGNORE_INDEX"]) == runtime.LOSS_IGNORE_INDEX == -100
    assert [int(d[k.upper()]) for k in runtime.LOSS_TERMS] == list(range(6))
    assert int(d["N_COUNTS"]) == len(runtime.LOSS_COUNTS) and int(d["N_SUMS"]) == runtime.LOSS_N_SUMS
    assert [int(d["COUNT_" + k]) for k in ("MASKED", "FALSE_POSITIVES", "SHOAL", "DEEP", "IGNORED", "INVALID", "FEATURE_AS_NOISE")] == list(range(7))
    from bathymetric_gnn_amd.training import losses
    assert (losses.ROWS_PER_WORKGROUP, losses.FINISH_WIDTH) == (runtime.LOSS_ROWS_PER_WG, runtime.LOSS_FINISH_WIDTH)


def test_workspace_bytes_needs_no_gpu(lib):
    from bathymetric_gnn_amd import runtime
    r = runtime.LOSS_ROWS_PER_WG
    one, two, big = (lib.bgnn_loss_workspace_bytes(n) for n in (1, r + 1, 1 << 20))
    assert 0 < one <= two < big and all(v % 256 == 0 for v in (one, two, big))
    assert lib.bgnn_loss_workspace_bytes(r) == one
    assert big >= ((1 << 20) // r) * (5 * 8 + (3 * 3 + len(runtime.LOSS_COUNTS)) * 4) and big < 4 << 20
    assert lib.bgnn_loss_workspace_bytes(0) == 0 and lib.bgnn_loss_workspace_bytes(-5) == 0
    assert lib.bgnn_loss_workspace_bytes((1 << 30) + 1) == 0


def test_loss_header_is_plain_c(tmp_path, lib):
    """Compiles as C99 and its structs have the layout of the ctypes mirrors."""
    if shutil.which("gcc") is None:
        pytest.skip("no gcc")
    from bathymetric_gnn_amd import runtime
    syms = _declared("bgnn_loss.h")
    src = tmp_path / "loss_abi.c"
    src.write_text('#include <dlfcn.h>\n#include <stddef.h>\n#include <stdio.h>\n#include "bgnn_loss.h"\n'
                   "int main(int argc, char **argv) {\n"
                   "  void *lib = dlopen(argv[1], RTLD_NOW | RTLD_LOCAL);\n"
                   "  if (argc < 2 || !lib) return 1;\n"
                   + "".join(f'  if (!dlsym(lib, "{s}")) {{ fprintf(stderr, "missing {s}\\n"); return 2; }}\n' for s in syms)
                   + '  printf("ok %d %d %d %d %d %d %d\\n", (int)sizeof(bgnn_loss_params), (int)sizeof(bgnn_loss_inputs),\n'
                     "         (int)offsetof(bgnn_loss_params, label_smoothing), (int)offsetof(bgnn_loss_params, feature_class),\n"
                     "         (int)offsetof(bgnn_loss_params, penalty_weight), (int)offsetof(bgnn_loss_params, term_weights),\n"
                     "         (int)offsetof(bgnn_loss_inputs, noise_mask));\n"
                     "  return 0;\n}\n")
    exe = tmp_path / "loss_abi"
    subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe),
                    "-ldl"], check=True)
    r = subprocess.run([str(exe), os.path.join(ROOT, "bathymetric-gnn_amd", "libbgnn_hip.so")], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    P, I = runtime.LossParams, runtime.LossInputs
    want = [C.sizeof(P), C.sizeof(I), P.label_smoothing.offset, P.feature_class.offset, P.penalty_weight.offset,
            P.term_weights.offset, I.noise_mask.offset]
    assert r.stdout.split() == ["ok"] + [str(v) for v in want], r.stdout
