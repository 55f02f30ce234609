"""Synthetic training noise on the host: the fixtures the REFERENCE's own generator produced (tests/golden/make_golden_noise.py ->
tests/golden/noise/*.npz), the numpy restatement of the kernels and of the counter-based generator (tests/_noise_cpu.py) against
them, the drop-in signatures, and the C side of include/bgnn_noise.h (plain C99, every symbol exported and bound).  No GPU
needed."""
import ctypes as C
import functools
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


# ---- helpers and inputs of tests/test_gpu_noise_scale.py ---------------------------------------------------------------------------
def _holed(h, w, seed):
    rng = np.random.default_rng(seed)
    d = rng.normal(-20.0, 0.3, (h, w)).astype(np.float32)
    v = rng.random((h, w)) >= 0.1
    return d, v


@pytest.mark.parametrize("h,w", [(37, 19), (1, 40), (3, 70), (70, 3), (100, 90), (64, 64)])
def test_banded_local_std_has_the_bits_of_the_unbanded_one(h, w):
    d, v = _holed(h, w, h * 1000 + w)
    filled = np.where(v, d, np.float32(1.0e6) if h == 100 else np.float32(d[v].mean()))
    want = nc.local_std(filled).view(np.uint32)
    for band in (32, 7, 1, 4096):
        assert np.array_equal(nc.local_std_banded(filled, band).view(np.uint32), want), band
    assert not np.array_equal(nc.local_std_banded(filled, shift=1).view(np.uint32), want)
    info = nc.complexity_probe(d, v, BOUND_C)[2][4]
    assert np.array_equal(nc.spike_density_map(info["local_std"], nc.PROBE_DENSITY, nc.PROBE_CC).view(np.uint32), info["density"].view(np.uint32))


def test_banded_local_std_is_what_generate_uses_on_a_large_tile():
    d, v = _holed(300, 260, 5)
    info = nc.complexity_probe(d, v, BOUND_C)[2][4]
    want = nc.local_std(np.where(v, d, info["nanmean"]))
    assert d.size > 1 << 16 and np.array_equal(info["local_std"].view(np.uint32), want.view(np.uint32))


def test_blob_centre_inputs_reach_every_path_of_the_rank_select():
    tiles = nc.centre_tiles()
    assert tuple(t[0] for t in tiles) == nc.CENTRE_NAMES
    assert [t[1].shape for t in tiles] == [(260, 253), (17, 16), (7, 11), (300, 517), (300, 517), (64, 64), (260, 253), (260, 253),
                                           (260, 253), (3, 30000), (512, 512), (1024, 1024)]
    offsets = np.cumsum([t[1].size for t in tiles])[2:-1]              # where the tiles after the two small ones start in the batch
    assert (offsets % 256 != 0).all() and (offsets % 4 != 0).all()
    pers = {}
    for i, (name, depth, valid, total, cats) in enumerate(tiles):
        _, d2, v2, us = nc.centre_case(i)
        assert d2 is depth and v2 is valid and len(us) >= total and depth.dtype == np.float32 and valid.dtype == bool
        if not valid.any():
            assert i == 5 and len(us) > 0 and nc.device_rank_select(valid, 0.5) is None
            continue
        us2, ks = nc.centre_draws(valid, total, 100 + i)
        assert us2 == us and us[:3] == [0.0, float(np.nextafter(1.0, 0.0)), 1.0]
        nv = int(valid.sum())
        assert {0, nv - 1, nv // 2} <= set(ks) and all(0 <= k < nv for k in ks)
        idx = np.flatnonzero(valid.ravel())
        paths = [nc.select_path(valid, k) for k in ks]
        for u, k, p in zip(us, ks, paths):
            cell = divmod(int(idx[k]), valid.shape[1])
            assert min(int(u * nv), nv - 1) == k and nc.kth_valid_cell(valid, u) == cell and nc.device_rank_select(valid, u) == cell
            assert p["run"] == idx[k] // 256 and p["strip"] == p["run"] // p["per"]
        for c in cats:
            assert any(p[c] for p in paths), (name, c)
        pers[name] = paths[0]["per"]
        counts = nc.run_counts(valid)
        assert len(counts) == (valid.size + 255) // 256 and counts.sum() == nv
    assert pers["260x253 0.9 valid"] == 2 and pers["300x517 0.01 valid"] == 3 and pers["3x30000 0.5 valid"] == 2
    assert pers["512x512 V1"] == 4 and pers["1024x1024 V1"] == 16 and pers["17x16 full"] == 1
    assert len(nc.centre_case(0)[3]) >= 700                           # one thread of noise_finalize resolves three blobs
    # 257 runs: the last strip holds one run, of 244 cells
    p = nc.select_path(tiles[0][2], int(tiles[0][2].sum()) - 1)
    assert p["runs"] == 257 and p["strip"] == 128 and p["last_strip"] and p["final_partial_run"] and tiles[0][2].size - 256 * 256 == 244
    # rows 40..199 invalid: about a hundred consecutive strips without a valid cell
    c = nc.run_counts(tiles[4][2])
    strips = np.add.reduceat(c, np.arange(0, len(c), 3))
    assert (strips == 0).sum() >= 100 and np.ptp(np.flatnonzero(strips == 0)) + 1 == (strips == 0).sum()
    # 0.01 valid: runs with no valid cell and with a few
    c = nc.run_counts(tiles[3][2])
    assert (c == 0).any() and 0 < c.max() < 16
    assert tiles[6][2].ravel()[0] and tiles[6][2].sum() == 1 and tiles[7][2].ravel()[-1] and tiles[7][2].sum() == 1
    assert tiles[8][2].sum() > 1 and not tiles[8][2].ravel()[:256 * 256].any()


def test_unit_blob_expectation_is_the_restatement():
    d, v = _holed(40, 33, 9)
    us = [0.0, 0.999, 1.0, 0.25, 0.25, 0.5]
    plan = {"sample": 0, "intensity": 1.0, "gaussian_std_factor": 0.0, "spike_density": 0.0, "blobs": [(-1, u, 1, 1.0) for u in us],
            "artifact": 0, "amplitude_factor": 0.0, "freq_a": 0.0, "freq_b": 0.0, "phase": 0.0}
    params = {**nc.PROBE_PARAMS, "enable_spikes": False, "enable_blobs": True}
    ref = nc.generate(d, v, plan, params)
    noisy, mask, mag, rng32 = nc.expected_unit_blobs(d, v, us)
    assert rng32 == ref[4]["depth_range"] > 0 and mask.sum() == 5 and np.array_equal(mask, ref[1])
    assert np.array_equal(noisy.view(np.uint32), ref[0].view(np.uint32)) and np.array_equal(mag.view(np.uint32), ref[2].view(np.uint32))
    r, c = nc.kth_valid_cell(v, 0.25)
    assert noisy[r, c] == np.float32(np.float64(np.float32(np.float64(d[r, c]) + np.float64(rng32))) + np.float64(rng32))


def test_scalar_inputs_need_the_last_trip_and_a_two_pass_variance():
    tiles = nc.scalar_tiles()
    assert tuple(t[0] for t in tiles) == nc.SCALAR_NAMES
    n = 300 * 517
    last_trip = 9 * nc.STATS_STRIDE
    assert last_trip < n <= 10 * nc.STATS_STRIDE
    for name, d, v in tiles:
        assert d.shape == v.shape == (300, 517) and d.dtype == np.float32 and v[:, -1].any()
        lo, hi = np.where(v, d, np.inf).argmin(), np.where(v, d, -np.inf).argmax()
        if name != "valid among the last 300":
            assert lo >= last_trip and hi >= last_trip and (d[v] == d.ravel()[lo]).sum() == 1 and (d[v] == d.ravel()[hi]).sum() == 1
        x = d[v].astype(np.float64)
        assert abs(x.mean() + 4000) < 1 and x.std() < 0.1
        # float32 cannot hold the variance in one pass: E[x^2] - E[x]^2 at 1.6e7 has steps of 1 .. 2
        x32 = d[v]
        one_pass = np.float32((x32 * x32).mean(dtype=np.float32)) - np.float32(x32.mean(dtype=np.float32)) ** 2
        assert not abs(float(one_pass) - x.var()) < 0.5 * x.var()
        # the restatement's float64 two-pass value is the longdouble one to an ulp
        info = nc.expected_unit_blobs(d, v, [0.0])
        std32 = np.float32(np.sqrt(((x - x.mean()) ** 2).sum() / len(x)))
        assert abs(int(std32.view(np.int32)) - int(nc.longdouble_std32(d, v).view(np.int32))) <= 1 and info[3] > 0
    assert np.array_equal(tiles[0][2], tiles[1][2]) and (tiles[0][1][~tiles[0][2]] == np.float32(1.0e6)).all()
    assert np.isnan(tiles[1][1][~tiles[1][2]]).all() and 0.03 < (~tiles[0][2]).mean() < 0.1
    tail = tiles[2][2].ravel()
    assert not tail[:n - 300].any() and 100 < tail.sum() < 200


@functools.lru_cache(maxsize=None)
def _probes():
    return [(name, d, v) + nc.complexity_probe(d, v, BOUND_C) for name, d, v in nc.probe_tiles()]


def test_complexity_probe_inputs():
    probes = _probes()
    assert [p[1].shape for p in probes] == [(16, 16), (17, 33), (37, 19), (3, 700), (700, 3), (1, 40), (48, 40), (260, 253), (260, 253)]
    for name, d, v, fields, delta, ref, want in probes:
        h, w = d.shape
        rr, cc = np.indices((h, w))
        assert 0 < delta < 1e-4, name                                 # (a condition on the inputs)
        assert np.array_equal(want, v & ((rr + cc) % 2 == 1)) and np.array_equal(ref[1], want) and want.any() and (v & ~want).any()
        dens = ref[4]["density"].astype(np.float64)
        assert (dens > 0).all() and (np.abs(fields["uniform"] / dens - 1) >= 0.99 * delta).all()
        # a spike's value is exact: magnitude in halves, range a float32
        val = fields["magnitude"] * np.float64(ref[4]["depth_range"])
        assert set(np.unique(fields["sign"]).tolist()) == {-1, 1} and fields["magnitude"].min() == 1.0 and fields["magnitude"].max() == 5.0
        assert np.array_equal(ref[2][want], np.abs(val[want]).astype(np.float32))
    name, d, v, fields, delta, ref, want = probes[6]
    assert np.isinf(d[~v]).sum() == 1 and np.isnan(ref[4]["local_std"]).any() and not ref[4]["complexity"].any()
    assert (ref[4]["density"] == np.float32(nc.PROBE_DENSITY) * (np.float32(1) - np.float32(nc.PROBE_CC) / np.float32(2))).all()
    assert delta == BOUND_C * nc.EPS32 * 2
    assert np.isnan(probes[7][1][~probes[7][2]]).all() and (probes[8][1][~probes[8][2]] == np.float32(1.0e6)).all()
    assert probes[8][5][4]["local_std"].max() > 1.0e4 and probes[7][5][4]["local_std"].max() < 10


MUTATIONS = {"window shifted by one column": dict(shift=1), "reflect": dict(mode="reflect"), "symmetric": dict(mode="symmetric"),
             "9 x 9 window": dict(window=9), "fill 0": dict(fill=0.0)}


@pytest.mark.parametrize("mutation", list(MUTATIONS))
def test_complexity_probe_sees_a_wrong_local_std(mutation):
    """A restatement with the defect, read through the probe's uniform field, flips a valid cell on every shape where its
    density map differs from the original's at all."""
    kw = dict(MUTATIONS[mutation])
    differing = 0
    for name, d, v, fields, delta, ref, want in _probes():
        fill = np.float32(kw["fill"]) if "fill" in kw else ref[4]["nanmean"]
        with np.errstate(invalid="ignore"):
            ls = nc.local_std_banded(np.where(v, d, fill), **{k: x for k, x in kw.items() if k != "fill"})
            dens = nc.spike_density_map(ls, nc.PROBE_DENSITY, nc.PROBE_CC)
        if np.array_equal(dens[v].view(np.uint32), ref[4]["density"][v].view(np.uint32)):
            continue
        differing += 1
        flips = ((fields["uniform"] < dens.astype(np.float64)) & v) != want
        print(f"{mutation}, {name}: {int(flips.sum())} of {int(v.sum())} valid cells flip")
        assert flips[v].any(), name
    assert differing >= (2 if "fill" in kw else 8)


def _near(depth, valid, gen_seed, sample):
    from bathymetric_gnn_amd.data import SyntheticNoiseGenerator
    gen = SyntheticNoiseGenerator(seed=gen_seed)
    params = {"enable_gaussian": True, "enable_spikes": True, "enable_blobs": True, "enable_systematic": True,
              "complexity_correlation": gen.complexity_correlation, "spike_magnitude_range": gen.spike_magnitude_range}
    ref, scale = nc.own_reference(depth, valid, gen.draw_plan(sample, 1.0), params, gen.seed)
    return int(nc.near_threshold(ref[4], valid, BOUND_C * nc.EPS32 * scale).sum()), int(valid.sum())


@pytest.mark.parametrize("h,w,tile_seed,gen_seed", nc.OWN_CASES, ids=[f"{c[0]}x{c[1]}" for c in nc.OWN_CASES])
def test_own_draw_cases_stay_under_the_near_threshold_cap(h, w, tile_seed, gen_seed):
    """The 0.1 % cap of ``check_outputs`` is a property of the inputs: asserted here from the restatement alone."""
    from bathymetric_gnn_amd import synthetic
    depth, valid, _ = synthetic.synthetic_tile(h, w, tile_seed, "V1")
    near, nv = _near(depth, valid, gen_seed, 0)
    print(f"{h}x{w}: {near} near a threshold, cap {int(0.001 * nv)}")
    assert near <= 0.001 * nv


def test_own_draw_batch_stays_under_the_near_threshold_cap():
    tiles = nc.own_batch_tiles()
    assert [t[0].shape for t in tiles] == [(260, 253), (17, 16), (64, 64), (300, 517), (1, 40)] and not tiles[2][1].any()
    assert nc.OWN_BATCH_SAMPLES[3] == 0 and sorted(nc.OWN_BATCH_SAMPLES) == list(range(5))
    assert sum(t[0].size for t in tiles[:3]) % 256 != 0           # the 300 x 517 tile's runs are misaligned in the batch
    for (depth, valid), sample in zip(tiles, nc.OWN_BATCH_SAMPLES):
        if valid.any():
            near, nv = _near(depth, valid, nc.OWN_BATCH_SEED, sample)
            assert near <= 0.001 * nv, (depth.shape, near)
