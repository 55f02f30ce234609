"""The operating-curve part of the C ABI (include/bgnn_curve.h) is plain C like bgnn.h: it compiles as C99 (-pedantic), a C program
resolves every entry point it declares with dlsym, and the ctypes binding (runtime._CURVE_SIGNATURES) covers exactly that set --
beside, not inside, every other pinned symbol set, at the same ABI number.  The refusals that need no device (they are checked
before anything is launched) are exercised with a NULL context.  No GPU needed."""
import ctypes as C
import glob
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMS = ["bgnn_curve_accumulate", "bgnn_curve_block_bytes", "bgnn_curve_reset"]


def _declared(path):
    text = re.sub(r"/\*.*?\*/", "", open(path).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(bgnn_[a-z_0-9]+)\s*\(", text)))


@pytest.fixture(scope="module")
def lib():
    from bathymetric_gnn_amd import runtime
    if not os.path.exists(runtime.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return runtime.load_library()


def test_curve_symbols_exported_and_bound(lib):
    from bathymetric_gnn_amd import runtime
    syms = _declared(os.path.join(ROOT, "include", "bgnn_curve.h"))
    assert syms == SYMS
    assert sorted(runtime._CURVE_SIGNATURES) == syms
    tables = {k: v for k, v in vars(runtime).items() if k.endswith("_SIGNATURES") and isinstance(v, dict)}
    assert "_CURVE_SIGNATURES" in tables and "_EVAL_SIGNATURES" in tables and len(tables) >= 16
    for name, table in tables.items():
        if name != "_CURVE_SIGNATURES":
            assert not set(syms) & set(table), name
    headers = sorted(glob.glob(os.path.join(ROOT, "include", "*.h")))
    assert len(headers) >= 16
    for h in headers:
        if os.path.basename(h) != "bgnn_curve.h":
            assert not set(syms) & set(_declared(h)), h
    for s in syms:
        assert hasattr(lib, s), f"{s} declared in bgnn_curve.h but not exported"
        assert getattr(lib, s).argtypes == runtime._CURVE_SIGNATURES[s][1]
        assert getattr(lib, s).restype == runtime._CURVE_SIGNATURES[s][0]
    assert lib.bgnn_abi_version() == 7 == runtime.ABI_VERSION


def test_curve_header_is_plain_c(tmp_path, lib):
    if shutil.which("gcc") is None:
        pytest.skip("no gcc")
    import numpy as np
    from bathymetric_gnn_amd import runtime
    src = tmp_path / "curve_abi.c"
    src.write_text('#include <dlfcn.h>\n#include <stdio.h>\n#include "bgnn_curve.h"\n'
                   "int main(int argc, char **argv) {\n"
                   "  void *lib = dlopen(argv[1], RTLD_NOW | RTLD_LOCAL);\n"
                   "  if (argc < 2 || !lib) return 1;\n"
                   + "".join(f'  if (!dlsym(lib, "{s}")) {{ fprintf(stderr, "missing {s}\\n"); return 2; }}\n' for s in SYMS)
                   + '  printf("ok %d %d %d %d %d\\n", BGNN_CURVE_MAX_THRESHOLDS, BGNN_CURVE_WG_CELLS, BGNN_CURVE_BLOCK_BYTES(1),\n'
                     "         BGNN_CURVE_BLOCK_BYTES(101), BGNN_CURVE_RES_SKIPPED(BGNN_CURVE_MAX_THRESHOLDS));\n"
                     "  return 0;\n}\n")
    exe = tmp_path / "curve_abi"
    subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe),
                    "-ldl"], check=True)
    r = subprocess.run([str(exe), os.path.join(ROOT, "bathymetric-gnn_amd", "libbgnn_hip.so")], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    size = {T: np.dtype(runtime.curve_block_dtype(T)).itemsize for T in (1, 101, 128)}
    assert r.stdout.split() == ["ok", str(runtime.CURVE_MAX_THRESHOLDS), str(runtime.CURVE_WG_CELLS), str(size[1]), str(size[101]),
                                str(size[128] - 8)]


def test_block_sizes_and_hostside_refusals(lib):
    """The block is a function of the table's length alone and 0 outside 1 .. 128.  With a NULL context every call is refused, and
    the message names what is wrong with the other arguments first: a NULL plane, a table that is empty or too long, one residual
    plane without the other, a bad cell count, a misaligned block."""
    import numpy as np
    from bathymetric_gnn_amd import runtime
    size = lib.bgnn_curve_block_bytes
    assert size(0) == 0 and size(-1) == 0 and size(129) == 0
    for T in (1, 2, 101, 128):
        assert size(T) == np.dtype(runtime.curve_block_dtype(T)).itemsize == 224 * (2 * T + 2) + 72
    buf = (C.c_int64 * 64)()
    p = C.cast(buf, C.c_void_p)
    odd = C.c_void_p(p.value + 4)

    def refused(word, rc):
        assert rc == runtime.ERR_INVALID
        assert word in lib.bgnn_last_error(), lib.bgnn_last_error()

    acc = lib.bgnn_curve_accumulate
    ok = [None, p, 1, p, p, p, None, None, 4, p]                # everything in order but the context
    refused(b"NULL context", acc(*ok))
    refused(b"NULL context", acc(*ok[:8], 0, p))                # (also without cells)
    refused(b"NULL context", lib.bgnn_curve_reset(None, p, 1))
    for k in (1, 3, 4, 5, 9):                                   # thresholds, labels, pred, confidence, block
        refused(b"NULL argument", acc(*[None if j == k else v for j, v in enumerate(ok)]))
    refused(b"0 thresholds", acc(None, p, 0, p, p, p, None, None, 4, p))
    refused(b"129 thresholds", acc(None, p, 129, p, p, p, None, None, 4, p))
    refused(b"both", acc(None, p, 1, p, p, p, p, None, 4, p))
    refused(b"both", acc(None, p, 1, p, p, p, None, p, 4, p))
    refused(b"-5 cells", acc(None, p, 1, p, p, p, None, None, -5, p))
    refused(b"4294967297 cells", acc(None, p, 1, p, p, p, None, None, (1 << 32) + 1, p))
    refused(b"not 8-byte aligned", acc(None, p, 1, p, p, p, None, None, 4, odd))
    refused(b"NULL argument", lib.bgnn_curve_reset(None, None, 1))
    refused(b"0 thresholds", lib.bgnn_curve_reset(None, p, 0))
    refused(b"129 thresholds", lib.bgnn_curve_reset(None, p, 129))
    refused(b"not 8-byte aligned", lib.bgnn_curve_reset(None, odd, 1))
    assert not any(buf)
