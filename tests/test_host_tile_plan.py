"""Planning the tiles of a ground-truth raster without reading it (training.plan_tile_boxes, training.keep_ground_truth_boxes), the
tile-store part of the C ABI (include/bgnn_tilestore.h) and the host side of its two entry points (csrc/tile_boxes.h).  No GPU.

The reference is ``plan_ground_truth_tiles``, the host scan the package already has: the planner must list its candidates (its boxes
at ``min_valid_ratio=0``) and the keep rule on counts must restate its test, both exactly."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMS = ["bgnn_tile_cut", "bgnn_tile_scan", "bgnn_tile_workspace_bytes"]
OTHER_HEADERS = ("bgnn.h", "bgnn_train.h", "bgnn_sidecar.h", "bgnn_noise.h", "bgnn_loss.h", "bgnn_optim.h", "bgnn_trainer.h", "bgnn_eval.h",
                 "bgnn_analysis.h", "bgnn_features.h")
SHAPES = [(150, 131), (72, 96), (32, 90), (20, 100), (33, 33)]


# ---- 1. the planner ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES)
def test_plan_tile_boxes_lists_the_candidates_of_the_host_scan(shape):
    from bathymetric_gnn_amd.training import plan_ground_truth_tiles, plan_tile_boxes
    want = plan_ground_truth_tiles(np.zeros(shape, np.int32), 32, 8, min_valid_ratio=0.0)[0]
    got = plan_tile_boxes(shape[0], shape[1], 32, 8)
    assert got == want
    assert all(isinstance(v, int) for b in got for v in b)


def test_plan_tile_boxes_cases_are_the_ones_meant():
    from bathymetric_gnn_amd.training import plan_tile_boxes
    boxes = plan_tile_boxes(150, 131, 32, 8)
    assert len(boxes) == 5 * 5 + 1 and boxes[-1] == (118, 99, 150, 131) and boxes[:2] == [(0, 0, 32, 32), (0, 24, 32, 56)]
    assert len(plan_tile_boxes(72, 96, 32, 8)) == 6                       # multiples of the stride: no corner tile
    assert plan_tile_boxes(32, 90, 32, 8) == [(0, 0, 32, 32), (0, 24, 32, 56), (0, 48, 32, 80)]     # height not above the tile
    assert plan_tile_boxes(20, 100, 32, 8) == [] and plan_tile_boxes(100, 20, 32, 8) == [] and plan_tile_boxes(0, 0, 32, 8) == []
    assert plan_tile_boxes(33, 33, 32, 8) == [(0, 0, 32, 32), (1, 1, 33, 33)]
    assert len(plan_tile_boxes(20000, 20000)) == 44 * 44 + 1 and len(plan_tile_boxes(46400, 46400)) == 103 * 103 + 1


@pytest.mark.parametrize("tile,overlap", [(32, 32), (32, 40), (8, 64)])
def test_plan_tile_boxes_refuses_a_stride_of_zero_or_less(tile, overlap):
    from bathymetric_gnn_amd.training import plan_ground_truth_tiles, plan_tile_boxes
    with pytest.raises(ValueError, match="Tile size must be larger than overlap"):
        plan_tile_boxes(100, 100, tile, overlap)
    with pytest.raises(ValueError, match="Tile size must be larger than overlap"):
        plan_ground_truth_tiles(np.zeros((100, 100), np.int32), tile, overlap)


# ---- 2. the keep rule -------------------------------------------------------------------------------------------------------
def _numpy_counts(labels, boxes):
    return np.array([[(labels[r0:r1, c0:c1] >= 0).sum()] + [(labels[r0:r1, c0:c1] == c).sum() for c in (0, 1, 2)]
                     for r0, c0, r1, c1 in boxes], dtype=np.int64).reshape(-1, 4)


@pytest.mark.parametrize("seed", range(6))
def test_keep_rule_on_counts_is_the_host_scan(seed):
    from bathymetric_gnn_amd.training import keep_ground_truth_boxes, plan_ground_truth_tiles, plan_tile_boxes
    rng = np.random.default_rng(seed)
    shape = [(150, 131), (72, 96), (32, 90), (97, 64), (33, 33), (20, 100)][seed]
    labels = rng.integers(-1, 4, size=shape).astype(np.int32)                 # -1 .. 3: class 3 is valid and counted nowhere
    for _ in range(6):                                                         # rectangles of no data, so that tiles straddle the ratio
        r, c = rng.integers(0, shape[0]), rng.integers(0, shape[1])
        labels[r:r + rng.integers(8, 60), c:c + rng.integers(8, 60)] = -1
    candidates = plan_tile_boxes(shape[0], shape[1], 32, 8)
    counts = _numpy_counts(labels, candidates)
    dropped_somewhere = False
    for ratio in (0.0, 0.1, 0.5, 0.75, 0.8, 1.0):
        want_boxes, want_counts = plan_ground_truth_tiles(labels, 32, 8, ratio)
        boxes, class_counts = keep_ground_truth_boxes(candidates, counts, ratio)
        assert boxes == want_boxes and class_counts == want_counts
        dropped_somewhere |= 0 < len(boxes) < len(candidates)
    assert dropped_somewhere or len(candidates) <= 2          # (the two tiles of 33 x 33 differ by one row and column)


def test_keep_rule_at_the_line():
    """128 of 1024 cells is exactly 0.125; 0.1 lies between 102 / 1024 and 103 / 1024."""
    from bathymetric_gnn_amd.training import keep_ground_truth_boxes
    boxes = [(0, 0, 32, 32), (0, 24, 32, 56), (24, 0, 56, 32), (24, 24, 56, 56)]
    counts = np.array([[128, 128, 0, 0], [127, 0, 127, 0], [103, 0, 0, 103], [102, 102, 0, 0]], np.int64)
    assert keep_ground_truth_boxes(boxes, counts, 0.125) == ([boxes[0]], {0: 128, 1: 0, 2: 0})
    assert keep_ground_truth_boxes(boxes, counts, 0.1) == (boxes[:3], {0: 128, 1: 127, 2: 103})


# ---- 3. assembling a store from several sources -------------------------------------------------------------------------------
def test_cut_store_tables_and_running_offsets(monkeypatch):
    """``_cut_store`` with ``cut_tile_boxes`` replaced by a recorder (host tensors, nothing launched): three sources of 2, 0 and 3
    boxes of unequal extents.  One allocation per plane for all of them, one call per source that has boxes, at its running offset."""
    import torch
    from bathymetric_gnn_amd.training import tile_store
    calls = []
    monkeypatch.setattr(tile_store, "cut_tile_boxes", lambda planes, stores, boxes, offsets, **kw: calls.append(
        (planes, stores, [tuple(int(v) for v in b) for b in boxes], np.asarray(offsets).tolist(), kw)))
    shapes = [(20, 30), (8, 8), (50, 41)]
    sources = [[torch.zeros(s, dtype=torch.int32), torch.zeros(s), None, torch.zeros(s)] for s in shapes]
    boxes = [[(0, 0, 5, 7), (3, 2, 20, 30)], [], [(0, 0, 1, 41), (10, 1, 50, 2), (7, 7, 16, 16)]]
    hw, stores, mask = tile_store._cut_store(list(zip(sources, boxes)), mask_plane=1, nodata=-5.0, ctx="the context")
    want_hw = [[5, 7], [17, 28], [1, 41], [40, 1], [9, 9]]
    cells = [35, 476, 41, 40, 81]
    offsets = [0, 35, 511, 552, 592, 673]
    assert hw.dtype == np.int32 and hw.tolist() == want_hw and offsets == np.concatenate([[0], np.cumsum(cells)]).tolist()
    assert tile_store._tile_offsets(hw).dtype == np.int64 and tile_store._tile_offsets(hw).tolist() == offsets
    assert [None if s is None else (s.dtype, tuple(s.shape)) for s in stores] == \
        [(torch.int32, (673,)), (torch.float32, (673,)), None, (torch.float32, (673,))]
    assert mask.dtype == torch.uint8 and tuple(mask.shape) == (673,)
    assert len(calls) == 2                                                # the source without boxes: no call
    for call, k, first in zip(calls, (0, 2), (0, 2)):
        planes, dst, b, at, kw = call
        assert planes is sources[k] and all(d is s for d, s in zip(dst, stores)) and b == boxes[k]
        assert at == offsets[first:first + len(boxes[k])]
        assert kw["mask"] is mask and kw["mask_plane"] == 1 and kw["nodata"] == -5.0 and kw["ctx"] == "the context"
    # a tile table past 2^31 cells keeps its 64-bit offsets
    big = np.array([[46341, 46341], [3, 5]], np.int32)
    assert tile_store._tile_offsets(big).tolist() == [0, 46341 * 46341, 46341 * 46341 + 15] and 46341 * 46341 > 2 ** 31


# ---- the C ABI --------------------------------------------------------------------------------------------------------------
def _declared(name):
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", name)).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(bgnn_[a-z_0-9]+)\s*\(", text)))


def _defines(name):
    text = open(os.path.join(ROOT, "include", name)).read()
    return {k: int(v) for k, v in re.findall(r"#define\s+(BGNN_[A-Z_0-9]+)\s+(\d+)\b", text)}


@pytest.fixture(scope="module")
def lib():
    from bathymetric_gnn_amd import runtime
    if not os.path.exists(runtime.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return runtime.load_library()


def test_tilestore_symbols_exported_and_bound(lib):
    from bathymetric_gnn_amd import runtime
    syms = _declared("bgnn_tilestore.h")
    assert syms == SYMS and sorted(runtime._TILESTORE_SIGNATURES) == syms
    others = [runtime._SIGNATURES, runtime._TRAIN_SIGNATURES, runtime._SIDECAR_SIGNATURES, runtime._NOISE_SIGNATURES,
              runtime._LOSS_SIGNATURES, runtime._OPTIM_SIGNATURES, runtime._TRAINER_SIGNATURES, runtime._EVAL_SIGNATURES,
              runtime._ANALYSIS_SIGNATURES, runtime._FEATURES_SIGNATURES]
    for table in others:
        assert not set(syms) & set(table)
    for h in OTHER_HEADERS:
        assert not set(syms) & set(_declared(h)), h
    for s in syms:
        assert getattr(lib, s).argtypes == runtime._TILESTORE_SIGNATURES[s][1]
        assert getattr(lib, s).restype == runtime._TILESTORE_SIGNATURES[s][0]
    assert lib.bgnn_abi_version() == 7 == runtime.ABI_VERSION


def test_constants_match_the_header():
    from bathymetric_gnn_amd import runtime
    d = _defines("bgnn_tilestore.h")
    assert d["BGNN_TILE_VALID_LABEL"] == runtime.TILE_VALID_LABEL == 0 and d["BGNN_TILE_VALID_DEPTH"] == runtime.TILE_VALID_DEPTH == 1
    assert d["BGNN_TILE_MAX_PLANES"] == runtime.TILE_MAX_PLANES == 4 and d["BGNN_TILE_COUNTS"] == runtime.TILE_COUNTS == 4
    assert d["BGNN_TILE_BAND_ROWS"] == runtime.TILE_BAND_ROWS == 32
    dt = runtime.TILE_BOX_DTYPE
    assert d["BGNN_TILE_BOX_BYTES"] == dt.itemsize == runtime.TILE_BOX_BYTES == 32
    assert [dt.fields[k][1] for k in ("row0", "col0", "h", "w", "dst")] == [0, 8, 16, 20, 24]


def test_tilestore_header_is_plain_c(tmp_path, lib):
    if shutil.which("gcc") is None:
        pytest.skip("no gcc")
    src = tmp_path / "tilestore_abi.c"
    src.write_text('#include <dlfcn.h>\n#include <stddef.h>\n#include <stdio.h>\n#include "bgnn_tilestore.h"\n'
                   "int main(int argc, char **argv) {\n"
                   "  void *lib = dlopen(argv[1], RTLD_NOW | RTLD_LOCAL);\n"
                   "  if (argc < 2 || !lib) return 1;\n"
                   + "".join(f'  if (!dlsym(lib, "{s}")) {{ fprintf(stderr, "missing {s}\\n"); return 2; }}\n' for s in SYMS)
                   + '  printf("ok %d %d %d %d\\n", (int)sizeof(bgnn_tile_box), BGNN_TILE_BOX_BYTES, (int)offsetof(bgnn_tile_box, h),\n'
                     "         (int)offsetof(bgnn_tile_box, dst));\n  return 0;\n}\n")
    exe = tmp_path / "tilestore_abi"
    subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe),
                    "-ldl"], check=True)
    r = subprocess.run([str(exe), os.path.join(ROOT, "bathymetric-gnn_amd", "libbgnn_hip.so")], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.split() == ["ok", "32", "32", "16", "24"]


def test_workspace_bytes_is_a_formula(lib):
    ws = lib.bgnn_tile_workspace_bytes
    assert ws(0) == 0 and ws(1) == 256 and ws(8) == 256 and ws(9) == 512 and ws(1937) == (1937 * 32 + 255) // 256 * 256
    assert ws(-1) == 0 and ws(2 ** 31 - 1) == (2 ** 31 - 1) * 32 + 32 and ws(2 ** 31) == 0


def _cxx():
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    for c in (shutil.which("g++"), os.path.join(rocm, "lib", "llvm", "bin", "clang++"), shutil.which("amdclang++"), shutil.which("clang++")):
        if c and os.path.exists(c):
            return c
    pytest.fail("no C++ compiler: neither g++ nor ROCm's clang++")


def test_box_check_as_a_host_program(tmp_path):
    """tests/tile_boxes_check.cpp: csrc/tile_boxes.h compiled alone, every refusal and the planning arithmetic at the sizes that
    could overflow."""
    exe = tmp_path / "tile_boxes_check"
    subprocess.run([_cxx(), "-std=c++17", "-O1", os.path.join(ROOT, "tests", "tile_boxes_check.cpp"), "-o", str(exe)],
                   check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    lines = r.stdout.splitlines()
    assert r.returncode == 0 and len(lines) == 30 and all(": ok" in ln for ln in lines), r.stdout + r.stderr


def test_hostside_refusals_of_the_calls(lib):
    """Every argument check comes before any use of the context or the device.  (The context here is a host buffer: a call that
    touched it, or launched anything, would not come back with these codes.)"""
    from bathymetric_gnn_amd import runtime
    buf = (C.c_int64 * 4096)()
    base = C.addressof(buf) + (-C.addressof(buf)) % 16
    at = lambda off: C.c_void_p(base + off)
    p = at(0)
    box = lambda *rows: np.array(list(rows), dtype=runtime.TILE_BOX_DTYPE)
    good = box((0, 0, 4, 4, 0))

    def scan(**kw):
        a = {**dict(ctx=p, plane=p, rows=10, cols=10, mode=0, nodata=1.0e6, boxes=good, n=1, ws=at(1024), ws_bytes=256, counts=at(2048)), **kw}
        b = a["boxes"]
        a["boxes"] = None if b is None else C.c_void_p(b.ctypes.data)
        return lib.bgnn_tile_scan(*a.values())
    err = lambda: lib.bgnn_last_error()
    for name in ("ctx", "plane", "boxes", "ws", "counts"):
        assert scan(**{name: None}) == runtime.ERR_INVALID and b"NULL" in err(), name
    assert scan(rows=0) == runtime.ERR_INVALID and scan(cols=-1) == runtime.ERR_INVALID and scan(n=-1) == runtime.ERR_INVALID
    assert scan(mode=2) == runtime.ERR_INVALID and b"mode" in err()
    assert scan(n=2 ** 31) == runtime.ERR_UNSUPPORTED
    assert scan(boxes=box((0, 0, 0, 4, 0))) == runtime.ERR_INVALID and b"is empty" in err()
    assert scan(boxes=box((0, 0, 4, -1, 0))) == runtime.ERR_INVALID and b"is empty" in err()
    assert scan(boxes=box((7, 0, 4, 4, 0))) == runtime.ERR_INVALID and b"leaves the plane" in err()
    assert scan(boxes=box((0, 7, 4, 4, 0))) == runtime.ERR_INVALID and b"leaves the plane" in err()
    assert scan(boxes=box((-1, 0, 4, 4, 0))) == runtime.ERR_INVALID and b"leaves the plane" in err()
    assert scan(boxes=box((0, 0, 4, 4, 0), (6, 6, 4, 5, 0)), n=2) == runtime.ERR_INVALID and b"box 1 " in err()
    assert scan(boxes=box((0, 0, 4, 4, -1))) == runtime.ERR_INVALID and b"negative destination" in err()
    assert scan(ws_bytes=255) == runtime.ERR_INVALID and b"workspace" in err()
    assert scan(ws=at(1032)) == runtime.ERR_INVALID and b"16-byte" in err()
    assert scan(plane=at(2)) == runtime.ERR_INVALID and b"aligned" in err()
    assert scan(counts=at(2052)) == runtime.ERR_INVALID and b"aligned" in err()
    # no boxes: nothing to do, whatever the context is -- nothing is launched and nothing written
    assert scan(n=0) == 0 and scan(n=0, boxes=None, ws=None, counts=None) == 0
    assert not any(buf)

    def cut(**kw):
        a = {**dict(ctx=p, planes=[at(4096), None], dst=[at(8192), None], n_planes=2, rows=10, cols=10, mask=at(12288), mask_plane=0, mode=0,
                    nodata=1.0e6, boxes=good, n=1, dst_cells=16, ws=at(1024), ws_bytes=256), **kw}
        for k in ("planes", "dst"):
            if a[k] is not None:
                a[k] = (C.c_void_p * len(a[k]))(*[None if v is None else v.value for v in a[k]])
        b = a["boxes"]
        a["boxes"] = None if b is None else C.c_void_p(b.ctypes.data)
        return lib.bgnn_tile_cut(*a.values())
    for name in ("ctx", "planes", "dst", "boxes", "ws"):
        assert cut(**{name: None}) == runtime.ERR_INVALID and b"NULL" in err(), name
    assert cut(n_planes=0) == runtime.ERR_INVALID and cut(n_planes=5) == runtime.ERR_INVALID and b"1 to 4" in err()
    assert cut(planes=[None, None], dst=[None, None]) == runtime.ERR_INVALID and b"no plane" in err()
    assert cut(planes=[at(4096), at(4500)]) == runtime.ERR_INVALID and b"no destination" in err()
    assert cut(dst=[at(8192), at(9000)]) == runtime.ERR_INVALID and b"no source" in err()
    assert cut(mask_plane=1) == runtime.ERR_INVALID and cut(mask_plane=-1) == runtime.ERR_INVALID and b"names no given plane" in err()
    assert cut(mode=3) == runtime.ERR_INVALID and b"mode" in err()
    assert cut(dst_cells=-1) == runtime.ERR_INVALID and cut(dst_cells=15) == runtime.ERR_INVALID and b"past the store" in err()
    assert cut(boxes=box((0, 0, 4, 4, 1))) == runtime.ERR_INVALID and b"past the store" in err()
    assert cut(boxes=box((8, 8, 4, 4, 0))) == runtime.ERR_INVALID and b"leaves the plane" in err()
    assert cut(boxes=box((0, 0, 0, 0, 0))) == runtime.ERR_INVALID and b"is empty" in err()
    assert cut(dst=[at(4096 + 396), None]) == runtime.ERR_INVALID and b"overlaps" in err()       # the store begins in the plane's last cell
    assert cut(dst=[at(4096 - 60), None]) == runtime.ERR_INVALID and b"overlaps" in err()        # ... ends in its first
    assert cut(mask=at(4096 + 399)) == runtime.ERR_INVALID and b"mask overlaps" in err()
    assert cut(planes=[at(4098), None]) == runtime.ERR_INVALID and b"aligned" in err()
    assert cut(ws_bytes=100) == runtime.ERR_INVALID and cut(ws=at(1028)) == runtime.ERR_INVALID
    assert cut(n=0) == 0 and cut(n=0, boxes=None, ws=None) == 0
    assert not any(buf)
