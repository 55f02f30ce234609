"""The feature label part of the C ABI (include/bgnn_features.h) is plain C like bgnn.h: it compiles as C99 (-pedantic), a C program
resolves every entry point it declares with dlsym, and the ctypes binding (runtime._FEATURES_SIGNATURES) covers exactly that set --
beside, not inside, the symbol sets of the other headers, at the same ABI number.  The sizes are pinned as formulas, and the
refusals that need no device (they are checked before anything is launched and before the context is looked at) are exercised
here.  No GPU needed."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMS = ["bgnn_feature_labels", "bgnn_feature_labels_plan", "bgnn_feature_labels_plan_bytes", "bgnn_feature_labels_workspace_bytes"]
OTHER_HEADERS = ("bgnn.h", "bgnn_train.h", "bgnn_sidecar.h", "bgnn_noise.h", "bgnn_loss.h", "bgnn_optim.h", "bgnn_trainer.h", "bgnn_eval.h",
                 "bgnn_analysis.h")


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


def test_features_symbols_exported_and_bound(lib):
    from bathymetric_gnn_amd import runtime
    syms = _declared("bgnn_features.h")
    assert syms == SYMS
    assert sorted(runtime._FEATURES_SIGNATURES) == syms
    others = [runtime._SIGNATURES, runtime._TRAIN_SIGNATURES, runtime._SIDECAR_SIGNATURES, runtime._NOISE_SIGNATURES,
              runtime._LOSS_SIGNATURES, runtime._OPTIM_SIGNATURES, runtime._TRAINER_SIGNATURES, runtime._EVAL_SIGNATURES,
              runtime._ANALYSIS_SIGNATURES]
    for table in others:
        assert not set(syms) & set(table)
    for h in OTHER_HEADERS:
        assert not set(syms) & set(_declared(h)), h
    for s in syms:
        assert hasattr(lib, s), f"{s} declared in bgnn_features.h but not exported"
        assert getattr(lib, s).argtypes == runtime._FEATURES_SIGNATURES[s][1]
        assert getattr(lib, s).restype == runtime._FEATURES_SIGNATURES[s][0]
    assert lib.bgnn_abi_version() == 7 == runtime.ABI_VERSION


def test_constants_match_the_header():
    from bathymetric_gnn_amd import runtime
    d = _defines("bgnn_features.h")
    dt = np.dtype(runtime.FL_STATS_DTYPE)
    assert dt.itemsize == d["BGNN_FL_STATS_BYTES"] == runtime.FL_STATS_BYTES == 24
    for field in dt.names:
        assert dt.fields[field][1] == d["BGNN_FL_STATS_" + field.upper()], field
    assert d["BGNN_FL_BIN"] == runtime.FL_BIN == 64
    assert d["BGNN_FL_MAX_CELLS"] == runtime.FL_MAX_CELLS == 2 ** 31 - 1
    assert d["BGNN_FL_MAX_FEATURES"] == runtime.FL_MAX_FEATURES == 2 ** 31 - 2


def test_features_header_is_plain_c(tmp_path, lib):
    if shutil.which("gcc") is None:
        pytest.skip("no gcc")
    syms = _declared("bgnn_features.h")
    src = tmp_path / "features_abi.c"
    src.write_text('#include <dlfcn.h>\n#include <stdio.h>\n#include "bgnn_features.h"\n'
                   "int main(int argc, char **argv) {\n"
                   "  void *lib = dlopen(argv[1], RTLD_NOW | RTLD_LOCAL);\n"
                   "  if (argc < 2 || !lib) return 1;\n"
                   + "".join(f'  if (!dlsym(lib, "{s}")) {{ fprintf(stderr, "missing {s}\\n"); return 2; }}\n' for s in syms)
                   + '  printf("ok %d %d %d %d\\n", BGNN_FL_STATS_BYTES, BGNN_FL_BIN, BGNN_FL_MAX_CELLS, BGNN_FL_MAX_FEATURES);\n'
                     "  return 0;\n}\n")
    exe = tmp_path / "features_abi"
    subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe),
                    "-ldl"], check=True)
    r = subprocess.run([str(exe), os.path.join(ROOT, "bathymetric-gnn_amd", "libbgnn_hip.so")], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.split() == ["ok", "24", "64", str(2 ** 31 - 1), str(2 ** 31 - 2)]


def _a256(n):
    return (n + 255) // 256 * 256


def test_sizes_are_formulas(lib):
    """plan_bytes = 8 * (bins + 1) + 4 * entries with bins = ceil(rows / 64) * ceil(cols / 64); workspace_bytes = plan_bytes and
    16 bytes per feature, each rounded up to 256; 0 outside the contract."""
    pb, ws = lib.bgnn_feature_labels_plan_bytes, lib.bgnn_feature_labels_workspace_bytes
    assert pb(None, 0, 1, 1) == 16 and pb(None, 0, 64, 64) == 16 and pb(None, 0, 65, 64) == 24 and pb(None, 0, 97, 203) == 8 * (2 * 4 + 1)
    assert pb(None, 0, 20000, 20000) == 8 * (313 * 313 + 1)
    table = np.array([[10, 10, 3, 1], [70, 70, 10, 1], [5, 5, -1, 1], [100, 100, 256, 1]], dtype=np.int32)
    tp = table.ctypes.data
    # 128 x 128: four bins; the survey-sized disc closes all four, so the three below it never enter
    assert pb(tp, 4, 128, 128) == 8 * 5 + 4 * 4
    # without it: the radius-3 disc in bin 0, the radius-10 disc in all four (it straddles the corner at 64, 64), the negative one nowhere
    assert pb(tp, 3, 128, 128) == 8 * 5 + 4 * 5
    assert pb(None, 0, 0, 5) == pb(None, 0, 5, 0) == pb(None, 0, -1, 5) == 0
    assert pb(None, 1, 5, 5) == 0 and pb(tp, -1, 5, 5) == 0                      # no table; a negative count
    assert pb(None, 0, 1 << 16, 1 << 15) == 0 and b"limit" in lib.bgnn_last_error()
    assert pb(None, 0, 46340, 46340) > 0 and pb(None, 0, 46341, 46341) == 0
    assert pb(tp, 2 ** 31 - 1, 128, 128) == 0 and b"limit" in lib.bgnn_last_error()
    assert pb(tp, 4, 100, 128) == 0 and b"outside" in lib.bgnn_last_error()      # the centre (100, 100) is outside 100 x 128
    big = np.array([[1, 1, 300, 1]], dtype=np.int32)
    assert pb(big.ctypes.data, 1, 100, 100) == 0                                  # a radius above rows + cols: the caller clamps
    assert ws(0, 0) == 0 and ws(0, 1) == 256 and ws(1, 0) == 256 and ws(17, 257) == 512 + 512
    assert ws(100000, 8 * (313 * 313 + 1) + 4 * 123457) == _a256(8 * (313 * 313 + 1) + 4 * 123457) + _a256(1600000)
    assert ws(-1, 100) == 0 and ws(2 ** 31 - 1, 100) == 0 and ws(2 ** 31 - 2, 0) == _a256(16 * (2 ** 31 - 2))


def test_plan_refusals(lib):
    from bathymetric_gnn_amd import runtime
    plan = lib.bgnn_feature_labels_plan
    table = np.array([[10, 10, 3, 1]], dtype=np.int32)
    tp = table.ctypes.data
    need = lib.bgnn_feature_labels_plan_bytes(tp, 1, 100, 100)
    buf = (C.c_int64 * 64)()
    p = C.cast(buf, C.c_void_p)
    assert plan(tp, 1, 100, 100, p, need) == 0
    assert list(buf[:5]) == [0, 1, 1, 1, 1] and C.cast(C.addressof(buf) + 40, C.POINTER(C.c_int32))[0] == 0
    assert plan(tp, 1, 100, 100, None, need) == runtime.ERR_INVALID and b"NULL" in lib.bgnn_last_error()
    assert plan(None, 1, 100, 100, p, need) == runtime.ERR_INVALID and b"NULL" in lib.bgnn_last_error()
    assert plan(tp, 1, 100, 100, p, need - 1) == runtime.ERR_INVALID and b"needed" in lib.bgnn_last_error()
    assert plan(tp, 1, 100, 100, C.c_void_p(C.addressof(buf) + 4), 256) == runtime.ERR_INVALID and b"aligned" in lib.bgnn_last_error()
    assert plan(tp, 1, 0, 100, p, 512) == runtime.ERR_INVALID
    assert plan(tp, 1, 10, 100, p, 512) == runtime.ERR_INVALID and b"outside" in lib.bgnn_last_error()
    assert plan(tp, 1, 1 << 16, 1 << 15, p, 512) == runtime.ERR_UNSUPPORTED and b"limit" in lib.bgnn_last_error()
    assert plan(tp, 2 ** 31 - 1, 100, 100, p, 512) == runtime.ERR_UNSUPPORTED and b"limit" in lib.bgnn_last_error()


def test_hostside_refusals_of_the_call(lib):
    """The argument checks come before any use of the context or the device: NULL pointers, both planes or neither, a grid or a
    feature count over the limit, an inconsistent plan, a short workspace, misaligned pointers.  (The context here is a host buffer:
    a call that touched it, or the device, would not come back with these codes.)"""
    from bathymetric_gnn_amd import runtime
    call = lib.bgnn_feature_labels
    buf = (C.c_int64 * 128)()
    p = C.cast(buf, C.c_void_p)
    odd = C.c_void_p(C.addressof(buf) + 4)
    table = np.array([[1, 1, 1, 1]], dtype=np.int32)
    tp = table.ctypes.data
    # a 2 x 2 grid: one bin; the zeroed buffer is the plan of an empty table (bin_ptr = [0, 0])
    ok = lambda **kw: {**dict(ctx=p, depth=p, base=None, rows=2, cols=2, nodata=1.0e6, table=None, n=0, plan=p, plan_bytes=16, ws=p,
                              ws_bytes=1 << 20, labels=p, stats=p), **kw}
    run = lambda **kw: call(*ok(**kw).values())
    for name in ("ctx", "plan", "ws", "labels", "stats"):
        assert run(**{name: None}) == runtime.ERR_INVALID and b"NULL" in lib.bgnn_last_error(), name
    assert run(depth=None) == runtime.ERR_INVALID and b"neither" in lib.bgnn_last_error()
    assert run(base=p) == runtime.ERR_INVALID and b"both" in lib.bgnn_last_error()
    assert run(n=1) == runtime.ERR_INVALID and b"NULL" in lib.bgnn_last_error()             # a count without a table
    assert run(n=-1, table=tp) == runtime.ERR_INVALID
    assert run(rows=0) == runtime.ERR_INVALID and run(cols=-3) == runtime.ERR_INVALID
    assert run(rows=1 << 16, cols=1 << 15, plan_bytes=1 << 62) == runtime.ERR_UNSUPPORTED and b"limit" in lib.bgnn_last_error()
    assert run(rows=1 << 40, cols=1 << 40) == runtime.ERR_UNSUPPORTED
    assert run(n=2 ** 31 - 1, table=tp) == runtime.ERR_UNSUPPORTED and b"limit" in lib.bgnn_last_error()
    assert run(plan=odd) == runtime.ERR_INVALID and b"aligned" in lib.bgnn_last_error()
    assert run(plan_bytes=15) == runtime.ERR_INVALID and b"plan" in lib.bgnn_last_error()
    # an inconsistent plan: an entry count beyond the plan's bytes; an index outside the table; a decreasing bin_ptr
    bad = (C.c_int64 * 4)(0, 1, 0, 0)
    assert run(plan=C.cast(bad, C.c_void_p), plan_bytes=16, table=tp, n=1) == runtime.ERR_INVALID and b"beyond" in lib.bgnn_last_error()
    bad = (C.c_int64 * 4)(0, 1, 5, 0)
    assert run(plan=C.cast(bad, C.c_void_p), plan_bytes=20, table=tp, n=1) == runtime.ERR_INVALID and b"outside the table" in lib.bgnn_last_error()
    bad = (C.c_int64 * 4)(0, -1, 0, 0)
    assert run(plan=C.cast(bad, C.c_void_p), plan_bytes=32, table=tp, n=1) == runtime.ERR_INVALID and b"decreases" in lib.bgnn_last_error()
    need = lib.bgnn_feature_labels_workspace_bytes(0, 16)
    assert need == 256
    assert run(ws_bytes=need - 1) == runtime.ERR_INVALID and b"workspace" in lib.bgnn_last_error()
    assert run(ws=odd) == runtime.ERR_INVALID and b"aligned" in lib.bgnn_last_error()
    half = C.c_void_p(C.addressof(buf) + (8 if C.addressof(buf) % 16 == 0 else 16))          # 8 modulo 16
    assert run(ws=half) == runtime.ERR_INVALID and b"16-byte" in lib.bgnn_last_error()
    assert run(stats=odd) == runtime.ERR_INVALID and b"aligned" in lib.bgnn_last_error()
    assert run(labels=C.c_void_p(C.addressof(buf) + 2)) == runtime.ERR_INVALID and b"aligned" in lib.bgnn_last_error()
    far = np.array([[5, 1, 1, 1]], dtype=np.int32)                                          # a centre outside the 2 x 2 grid
    good = (C.c_int64 * 4)(0, 1, 0, 0)
    assert run(plan=C.cast(good, C.c_void_p), plan_bytes=20, table=far.ctypes.data, n=1) == runtime.ERR_INVALID and b"outside" in lib.bgnn_last_error()
