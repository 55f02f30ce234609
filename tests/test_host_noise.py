"""Synthetic training noise on the host: the fixtures the REFERENCE's own generator produced (tests/golden/make_golden_noise.py ->
tests/golden/noise/*.npz), the numpy restatement of the kernels and of the counter-based generator (tests/_noise_cpu.py) against
them, the drop-in signatures, and the C side of include/bgnn_noise.h (plain C99, every symbol exported and bound).  No GPU
needed."""
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

import _noise_cpu as nc
from _conditioning import BOUND_C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NOISE_DIR = os.path.join(ROOT, "tests", "golden", "noise")
FIXTURES = sorted(glob.glob(os.path.join(NOISE_DIR, "*.npz")))
NAMES = [os.path.basename(p)[:-4] for p in FIXTURES]


# ---- the fixtures -----------------------------------------------------------------------------------------------------------------
def test_fixture_set_covers_the_cases():
    z = {n: np.load(p) for n, p in zip(NAMES, FIXTURES)}
    assert len(z) >= 16
    assert sorted({int(v["scalars"][2]) for v in z.values() if v["enable"][3] and v["valid_mask"].any()}) == [1, 2, 3, 4, 5, 6]
    assert {0.5, 1.0, 1.5} <= {float(v["intensity"]) for v in z.values()}
    for k in range(4):                      # each noise type enabled alone
        assert any(v["enable"].tolist() == [int(i == k) for i in range(4)] for v in z.values())
    holes = 1 - z["holes10"]["valid_mask"].mean()
    assert 0.07 < holes < 0.13 and z["holes10"]["clean_depth"].shape[0] != z["holes10"]["clean_depth"].shape[1]
    nn = z["nan_mask_none"]
    assert bool(nn["mask_none"]) and np.isnan(nn["clean_depth"]).any()
    assert np.array_equal(nn["valid_mask"], np.isfinite(nn["clean_depth"]))
    assert float(z["constant"]["std32"]) == 0.0 and z["constant"]["noise_mask"].any()
    assert np.array_equal(z["constant"]["noisy_depth"], z["constant"]["clean_depth"])
    assert not z["no_valid"]["valid_mask"].any()


@pytest.mark.parametrize("path", FIXTURES, ids=NAMES)
def test_fixture_is_self_consistent(path):
    assert os.path.getsize(path) <= 600_000
    z = np.load(path)
    d, v = z["clean_depth"], z["valid_mask"]
    assert d.dtype == np.float32 and v.dtype == bool and d.shape == v.shape
    assert z["noisy_depth"].dtype == np.float32 and z["noisy_depth64"].dtype == np.float64
    assert z["noise_mask"].dtype == bool and z["noise_magnitude"].dtype == np.float32 and z["classification"].dtype == np.int64
    for k in ("noisy_depth", "noisy_depth64", "noise_mask", "noise_magnitude", "classification", "gaussian_field", "uniform_field"):
        assert z[k].shape == d.shape, k
    assert np.array_equal(z["classification"], np.where(z["noise_mask"], 2, 0))
    assert np.array_equal(z["noisy_depth"].view(np.uint32)[~v], d.view(np.uint32)[~v])          # NaNs included
    assert not z["noise_mask"][~v].any() and not z["noise_magnitude"][~v].any()
    idx = z["spike_index"]
    assert len(idx) == len(z["spike_sign"]) == len(z["spike_magnitude"]) and v.ravel()[idx].all()
    assert set(np.unique(z["spike_sign"]).tolist()) <= {-1, 1} and z["noise_mask"].ravel()[idx].all()
    b = z["blobs"]
    assert b.shape[1] == 4 and all(v[int(r), int(c)] for r, c, _, _ in b)
    if v.any():
        assert float(z["std32"]) == float(np.std(d[v])) and float(z["std64"]) == float(np.std(d[v].astype(np.float64)))
        if float(z["std64"]) > 0:
            assert 0 < np.abs(z["noisy_depth"] - z["noisy_depth64"])[v].max() < 1e-4
    else:
        assert np.array_equal(z["noisy_depth"].view(np.uint32), d.view(np.uint32)) and not z["classification"].any()


# ---- the restatement against the reference ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("path", FIXTURES, ids=NAMES)
def test_restatement_reproduces_the_reference(path):
    """tests/_noise_cpu.py driven with the fixture's injected draws lands on the reference's outputs under the rule of
    ``check_outputs`` -- which pins it before tests/test_gpu_noise.py uses it as the yardstick for the device's own draws."""
    depth, valid, plan, params, fields, z = nc.load_fixture(path)
    out = nc.generate(depth, valid, plan, params, fields=fields)[:4]
    nc.check_fixture(out, path, BOUND_C)


def test_restatement_resolves_blob_centres_by_rank():
    valid = np.zeros((5, 7), bool)
    valid[1, 2] = valid[3, 0] = valid[4, 6] = True
    assert nc.kth_valid_cell(valid, 0.0) == (1, 2) and nc.kth_valid_cell(valid, 0.34) == (3, 0)
    assert nc.kth_valid_cell(valid, 0.999999) == (4, 6)


# ---- the documented generator -----------------------------------------------------------------------------------------------------
def test_generator_moments():
    """10^6 draws; every statistic within 5 standard errors, which follow from the sample size alone."""
    n = 10 ** 6
    idx = np.arange(n, dtype=np.uint64)
    z = nc.normal(12345, 7, idx)
    assert abs(z.mean()) <= 5 / np.sqrt(n)
    assert abs(z.var() - 1.0) <= 5 * np.sqrt(2.0 / (n - 1))
    u = nc.uniform(12345, 7, nc.STREAM_SPIKE_U, idx)
    assert 0.0 <= u.min() and u.max() < 1.0
    assert abs(u.mean() - 0.5) <= 5 * np.sqrt(1 / 12 / n)
    assert abs((u < 0.01).mean() - 0.01) <= 5 * np.sqrt(0.01 * 0.99 / n)
    s = nc.sign(12345, 7, idx).astype(np.float64)
    assert set(np.unique(s).tolist()) == {-1.0, 1.0} and abs(s.mean()) <= 5 / np.sqrt(n)


def test_generator_is_keyed_on_seed_sample_stream_and_cell():
    idx = np.arange(1000, dtype=np.uint64)
    a = nc.bits(1, 2, 3, idx)
    assert np.array_equal(a, nc.bits(1, 2, 3, idx)) and np.array_equal(a[10:20], nc.bits(1, 2, 3, idx[10:20]))
    for other in (nc.bits(2, 2, 3, idx), nc.bits(1, 3, 3, idx), nc.bits(1, 2, 4, idx)):
        assert (a != other).mean() > 0.99
    # the definition, spelled out once with Python integers
    M = (1 << 64) - 1

    def fin(z):
        z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M
        z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M
        return z ^ (z >> 31)
    key = fin((1 + 0x9E3779B97F4A7C15 * (2 + 1)) & M)
    assert int(a[5]) == fin((key + 0x9E3779B97F4A7C15 * (3 + 1) + 0xD1B54A32D192ED03 * 5) & M)


# ---- the drop-in classes ----------------------------------------------------------------------------------------------------------
def _params_of(fn):
    return [[n, None if p.default is inspect.Parameter.empty else (list(p.default) if isinstance(p.default, tuple) else p.default)]
            for n, p in inspect.signature(fn).parameters.items() if n != "self"]


def test_signatures_equal_the_reference():
    from bathymetric_gnn_amd.data import NoiseAugmentor, NoiseLabel, SyntheticNoiseGenerator
    sig = json.load(open(os.path.join(NOISE_DIR, "signatures.json")))
    assert _params_of(SyntheticNoiseGenerator.__init__) == sig["SyntheticNoiseGenerator"]
    assert _params_of(NoiseAugmentor.__init__) == sig["NoiseAugmentor"]
    assert _params_of(SyntheticNoiseGenerator.generate) == sig["generate"]
    assert [f for f in NoiseLabel.__dataclass_fields__] == sig["NoiseLabel"]
    g = SyntheticNoiseGenerator(seed=5)
    for name, default in sig["SyntheticNoiseGenerator"]:
        if name != "seed":
            got = getattr(g, name)
            assert (list(got) if isinstance(got, tuple) else got) == default, name
    a = NoiseAugmentor(g, seed=3)
    assert a.generator is g and list(a.intensity_range) == [0.5, 1.5] and hasattr(g, "rng") and hasattr(a, "rng")


def test_scalar_draws_depend_on_seed_and_sample_only():
    from bathymetric_gnn_amd.data import NoiseAugmentor, SyntheticNoiseGenerator
    g, g2 = SyntheticNoiseGenerator(seed=11), SyntheticNoiseGenerator(seed=11)
    g2.draw_plan(0), g2.draw_plan(9)
    assert g.draw_plan(4, 1.2) == g2.draw_plan(4, 1.2) != g.draw_plan(5, 1.2)
    assert SyntheticNoiseGenerator(seed=12).draw_plan(4, 1.2) != g.draw_plan(4, 1.2)
    kinds = {g.draw_plan(s)["artifact"] for s in range(200)}
    assert kinds == set(nc.ARTIFACTS) - {"none"}
    for s in range(50):
        p = g.draw_plan(s, 1.5)
        assert 0.1 <= p["gaussian_std_factor"] <= 0.5 and 0.001 <= p["spike_density_draw"] <= 0.01
        assert int(5 * 1.5) <= len(p["blobs"]) <= int(50 * 1.5)
        assert all(r == -1 and 0 <= u < 1 and 3 <= size <= 15 and 0.5 <= abs(m) <= 3.0 for r, u, size, m in p["blobs"])
    off = SyntheticNoiseGenerator(enable_gaussian=False, enable_spikes=False, enable_blobs=False, enable_systematic=False, seed=1)
    assert off.draw_plan(0)["blobs"] == [] and off.draw_plan(0)["artifact"] == "none"
    given = g.draw_plan(3, given={"artifact": 6, "blobs": [(1, 2, 3, -0.5)], "freq_a": 0.25})
    assert given["artifact"] == "gradient_diagonal" and given["blobs"] == [(1, 2, 3, -0.5)] and given["freq_a"] == 0.25
    a = NoiseAugmentor(g, seed=2)
    assert a.intensity(7) == NoiseAugmentor(g2, seed=2).intensity(7) != a.intensity(8) and 0.5 <= a.intensity(7) <= 1.5


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


def test_noise_symbols_exported_and_bound(lib):
    from bathymetric_gnn_amd import runtime
    syms = _declared("bgnn_noise.h")
    assert syms == ["bgnn_noise_generate", "bgnn_noise_workspace_bytes"]
    others = set(runtime._SIGNATURES) | set(runtime._TRAIN_SIGNATURES) | set(runtime._SIDECAR_SIGNATURES)
    assert not set(syms) & others
    assert not set(syms) & (set(_declared("bgnn.h")) | set(_declared("bgnn_train.h")) | set(_declared("bgnn_sidecar.h")))
    assert sorted(runtime._NOISE_SIGNATURES) == syms
    for s in syms:
        assert hasattr(lib, s), f"{s} declared in bgnn_noise.h but not exported"
    assert lib.bgnn_abi_version() == 7
    text = open(os.path.join(ROOT, "include", "bgnn_noise.h")).read()
    codes = dict(re.findall(r"#define BGNN_NOISE_(ARTIFACT_NONE|STRIPE_HORIZONTAL|STRIPE_VERTICAL|WAVE|GRADIENT_X|GRADIENT_Y|GRADIENT_DIAGONAL) (\d)", text))
    assert [int(codes[k]) for k in ("ARTIFACT_NONE", "STRIPE_HORIZONTAL", "STRIPE_VERTICAL", "WAVE", "GRADIENT_X", "GRADIENT_Y",
                                    "GRADIENT_DIAGONAL")] == list(range(7))
    assert runtime.NOISE_ARTIFACTS == nc.ARTIFACTS


def test_workspace_bytes_needs_no_gpu(lib):
    hw = np.array([[64, 48], [16, 300]], np.int32)
    p = hw.ctypes.data_as(C.c_void_p)
    one, two = lib.bgnn_noise_workspace_bytes(1, p, 0), lib.bgnn_noise_workspace_bytes(2, p, 10)
    assert one >= 64 * 48 * 4 and two >= one + 16 * 300 * 4 + 10 * 32 and two % 256 == 0
    assert lib.bgnn_noise_workspace_bytes(0, p, 0) == 0 and lib.bgnn_noise_workspace_bytes(2, None, 0) == 0
    assert lib.bgnn_noise_workspace_bytes(2, p, -1) == 0
    bad = np.array([[64, 0]], np.int32)
    assert lib.bgnn_noise_workspace_bytes(1, bad.ctypes.data_as(C.c_void_p), 0) == 0
    big = np.array([[40000, 8]], np.int32)
    assert lib.bgnn_noise_workspace_bytes(1, big.ctypes.data_as(C.c_void_p), 0) == 0


def test_noise_header_is_plain_c(tmp_path, lib):
    """Compiles as C99 and its structs have the layout of the ctypes mirrors."""
    if shutil.which("gcc") is None:
        pytest.skip("no gcc")
    from bathymetric_gnn_amd import runtime
    syms = _declared("bgnn_noise.h")
    src = tmp_path / "noise_abi.c"
    src.write_text('#include <dlfcn.h>\n#include <stddef.h>\n#include <stdio.h>\n#include "bgnn_noise.h"\n'
                   "int main(int argc, char **argv) {\n"
                   "  void *lib = dlopen(argv[1], RTLD_NOW | RTLD_LOCAL);\n"
                   "  if (argc < 2 || !lib) return 1;\n"
                   + "".join(f'  if (!dlsym(lib, "{s}")) {{ fprintf(stderr, "missing {s}\\n"); return 2; }}\n' for s in syms)
                   + '  printf("ok %d %d %d %d %d %d %d %d\\n", (int)sizeof(bgnn_noise_params), (int)sizeof(bgnn_noise_blob),\n'
                     "         (int)sizeof(bgnn_noise_plan), (int)sizeof(bgnn_noise_fields), (int)offsetof(bgnn_noise_params, seed),\n"
                     "         (int)offsetof(bgnn_noise_blob, magnitude), (int)offsetof(bgnn_noise_plan, artifact), BGNN_NOISE_WINDOW);\n"
                     "  return 0;\n}\n")
    exe = tmp_path / "noise_abi"
    subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe),
                    "-ldl"], check=True)
    r = subprocess.run([str(exe), os.path.join(ROOT, "bathymetric-gnn_amd", "libbgnn_hip.so")], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    want = [C.sizeof(runtime.NoiseParams), C.sizeof(runtime.NoiseBlob), C.sizeof(runtime.NoisePlan), C.sizeof(runtime.NoiseFields),
            runtime.NoiseParams.seed.offset, runtime.NoiseBlob.magnitude.offset, runtime.NoisePlan.artifact.offset, 11]
    assert r.stdout.split() == ["ok"] + [str(v) for v in want], r.stdout
