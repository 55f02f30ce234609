"""The noise pattern analysis part of the C ABI (include/bgnn_analysis.h) is plain C like bgnn.h: it compiles as C99 (-pedantic), a C
program resolves every entry point it declares with dlsym, and the ctypes binding (runtime._ANALYSIS_SIGNATURES) covers exactly
that set -- beside, not inside, the symbol sets of the other headers, at the same ABI number.  The refusals that need no device
(they are checked before anything is launched and before the context is looked at) are exercised here.  No GPU needed."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMS = ["bgnn_noise_analysis", "bgnn_noise_analysis_workspace_bytes"]
OTHER_HEADERS = ("bgnn.h", "bgnn_train.h", "bgnn_sidecar.h", "bgnn_noise.h", "bgnn_loss.h", "bgnn_optim.h", "bgnn_trainer.h", "bgnn_eval.h")


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


def test_analysis_symbols_exported_and_bound(lib):
    from bathymetric_gnn_amd import runtime
    syms = _declared("bgnn_analysis.h")
    assert syms == SYMS
    assert sorted(runtime._ANALYSIS_SIGNATURES) == syms
    others = [runtime._SIGNATURES, runtime._TRAIN_SIGNATURES, runtime._SIDECAR_SIGNATURES, runtime._NOISE_SIGNATURES,
              runtime._LOSS_SIGNATURES, runtime._OPTIM_SIGNATURES, runtime._TRAINER_SIGNATURES, runtime._EVAL_SIGNATURES]
    for table in others:
        assert not set(syms) & set(table)
    for h in OTHER_HEADERS:
        assert not set(syms) & set(_declared(h)), h
    for s in syms:
        assert hasattr(lib, s), f"{s} declared in bgnn_analysis.h but not exported"
        assert getattr(lib, s).argtypes == runtime._ANALYSIS_SIGNATURES[s][1]
        assert getattr(lib, s).restype == runtime._ANALYSIS_SIGNATURES[s][0]
    assert lib.bgnn_abi_version() == 7 == runtime.ABI_VERSION


def test_block_layout_matches_the_header():
    from bathymetric_gnn_amd import runtime
    d = _defines("bgnn_analysis.h")
    dt = np.dtype(runtime.NA_DTYPE)
    assert dt.itemsize == d["BGNN_NA_BYTES"] == runtime.NA_BYTES and runtime.NA_BYTES % 8 == 0
    macro = {"size_bins": "SIZE_BINS_OFFSET"}
    for field in dt.names:
        if field != "pad":
            assert dt.fields[field][1] == d["BGNN_NA_" + macro.get(field, field.upper())], field
    assert dt.fields["bin_noise"][0].shape == dt.fields["bin_valid"][0].shape == dt.fields["bin_abs_sum"][0].shape == (d["BGNN_NA_DEPTH_BINS"],)
    assert dt.fields["size_bins"][0].shape == (d["BGNN_NA_SIZE_BINS"],) and dt.fields["mag_rank"][0].shape == (d["BGNN_NA_MAG_RANKS"],)
    assert len(runtime.NA_DEPTH_EDGES) == d["BGNN_NA_DEPTH_BINS"] + 1 and len(runtime.NA_SIZE_EDGES) == d["BGNN_NA_SIZE_BINS"] + 1
    assert d["BGNN_NA_MAX_CELLS"] == runtime.NA_MAX_CELLS == 2 ** 31 - 1
    # the fields tile the block without overlap
    spans = sorted((dt.fields[f][1], dt.fields[f][1] + dt.fields[f][0].itemsize) for f in dt.names)
    assert spans[0][0] == 0 and spans[-1][1] == dt.itemsize and all(a[1] == b[0] for a, b in zip(spans, spans[1:]))


def test_analysis_header_is_plain_c(tmp_path, lib):
    if shutil.which("gcc") is None:
        pytest.skip("no gcc")
    from bathymetric_gnn_amd import runtime
    syms = _declared("bgnn_analysis.h")
    src = tmp_path / "analysis_abi.c"
    src.write_text('#include <dlfcn.h>\n#include <stdio.h>\n#include "bgnn_analysis.h"\n'
                   "int main(int argc, char **argv) {\n"
                   "  void *lib = dlopen(argv[1], RTLD_NOW | RTLD_LOCAL);\n"
                   "  if (argc < 2 || !lib) return 1;\n"
                   + "".join(f'  if (!dlsym(lib, "{s}")) {{ fprintf(stderr, "missing {s}\\n"); return 2; }}\n' for s in syms)
                   + '  printf("ok %d %d %d\\n", BGNN_NA_BYTES, BGNN_NA_DEPTH_BINS, BGNN_NA_MAX_CELLS);\n'
                     "  return 0;\n}\n")
    exe = tmp_path / "analysis_abi"
    subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe),
                    "-ldl"], check=True)
    r = subprocess.run([str(exe), os.path.join(ROOT, "bathymetric-gnn_amd", "libbgnn_hip.so")], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.split() == ["ok", str(runtime.NA_BYTES), "8", str(runtime.NA_MAX_CELLS)]


def test_workspace_sizes_and_hostside_refusals(lib):
    """The workspace is a function of rows and cols: a fixed head and 16 bytes per cell (two int32 planes and the float64
    roughness, each rounded up to 256 bytes); 0 outside the contract.  The argument checks come before any use of the context or
    the device: NULL pointers, a grid beyond the limit, a short workspace."""
    from bathymetric_gnn_amd import runtime
    ws = lib.bgnn_noise_analysis_workspace_bytes
    assert ws(0, 5) == ws(5, 0) == ws(-1, 5) == 0 and ws(1 << 16, 1 << 15) == 0 and ws(1 << 40, 1 << 40) == 0
    head = ws(1, 1) - 3 * 256
    assert head > 0 and head % 256 == 0 and head < (2 << 20)
    assert ws(97, 203) == ws(203, 97) == head + 2 * ((97 * 203 * 4 + 255) // 256 * 256) + (97 * 203 * 8 + 255) // 256 * 256
    assert ws(20000, 20000) == head + 16 * 20000 * 20000
    assert ws(2 ** 31 - 1, 1) > 0 and ws(46340, 46340) > 0 and ws(46341, 46341) == 0

    buf = (C.c_int64 * 128)()
    p = C.cast(buf, C.c_void_p)
    call = lib.bgnn_noise_analysis
    assert call(None, p, p, p, p, 2, 2, p, 1 << 30, p, p, p) == runtime.ERR_INVALID and b"NULL" in lib.bgnn_last_error()
    for k in range(1, 12):
        if k in (5, 6, 8):                                     # rows, cols, workspace_bytes
            continue
        args = [p, p, p, p, p, 2, 2, p, 1 << 30, p, p, p]
        args[k] = None
        assert call(*args) == runtime.ERR_INVALID and b"NULL" in lib.bgnn_last_error(), k
    assert call(p, p, p, p, p, 0, 2, p, 1 << 30, p, p, p) == runtime.ERR_INVALID
    assert call(p, p, p, p, p, 1 << 16, 1 << 15, p, 1 << 62, p, p, p) == runtime.ERR_UNSUPPORTED and b"limit" in lib.bgnn_last_error()
    assert call(p, p, p, p, p, 1 << 40, 1 << 40, p, 1 << 62, p, p, p) == runtime.ERR_UNSUPPORTED
    assert call(p, p, p, p, p, 2, 2, p, ws(2, 2) - 1, p, p, p) == runtime.ERR_INVALID and b"workspace" in lib.bgnn_last_error()
    odd = C.c_void_p(C.addressof(buf) + 4)
    assert call(p, p, p, p, p, 2, 2, odd, 1 << 30, p, p, p) == runtime.ERR_INVALID and b"aligned" in lib.bgnn_last_error()
    assert call(p, p, p, p, p, 2, 2, p, 1 << 30, odd, p, p) == runtime.ERR_INVALID and b"aligned" in lib.bgnn_last_error()
