"""The robust-gridder part of the C ABI (include/bgnn_soundings_robust.h) is plain C like bgnn.h: it compiles as C99 (-pedantic), a
C program resolves every entry point it declares with dlsym, and the ctypes binding (runtime._ROBUST_SIGNATURES) covers exactly that
set -- beside, not inside, every other pinned symbol set, at the same ABI number.  The refusals, all of which come before
anything is launched, are exercised with a NULL context: each returns its code and a message.  No GPU needed."""
import ctypes as C
import glob
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMS = ["bgnn_soundings_robust_add", "bgnn_soundings_robust_finalize", "bgnn_soundings_robust_flag", "bgnn_soundings_robust_reset",
        "bgnn_soundings_robust_stage_bytes", "bgnn_soundings_robust_workspace_bytes"]


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


def test_robust_symbols_exported_and_bound(lib):
    from bathymetric_gnn_amd import runtime
    syms = _declared(os.path.join(ROOT, "include", "bgnn_soundings_robust.h"))
    assert syms == SYMS
    assert sorted(runtime._ROBUST_SIGNATURES) == syms
    tables = {k: v for k, v in vars(runtime).items() if k.endswith("_SIGNATURES") and isinstance(v, dict)}
    assert "_ROBUST_SIGNATURES" in tables and "_SOUNDINGS_SIGNATURES" in tables and len(tables) >= 18
    for name, table in tables.items():
        if name != "_ROBUST_SIGNATURES":
            assert not set(syms) & set(table), name
    headers = sorted(glob.glob(os.path.join(ROOT, "include", "*.h")))
    assert len(headers) >= 18
    for h in headers:
        if os.path.basename(h) != "bgnn_soundings_robust.h":
            assert not set(syms) & set(_declared(h)), h
    for s in syms:
        assert hasattr(lib, s), f"{s} declared in bgnn_soundings_robust.h but not exported"
        assert getattr(lib, s).argtypes == runtime._ROBUST_SIGNATURES[s][1]
        assert getattr(lib, s).restype == runtime._ROBUST_SIGNATURES[s][0]
    assert lib.bgnn_abi_version() == 7 == runtime.ABI_VERSION


def test_robust_header_is_plain_c(tmp_path, lib):
    if shutil.which("gcc") is None:
        pytest.skip("no gcc")
    from bathymetric_gnn_amd import runtime
    src = tmp_path / "robust_abi.c"
    src.write_text('#include <dlfcn.h>\n#include <stdio.h>\n#include "bgnn_soundings_robust.h"\n'
                   "int main(int argc, char **argv) {\n"
                   "  void *lib = dlopen(argv[1], RTLD_NOW | RTLD_LOCAL);\n"
                   "  if (argc < 2 || !lib) return 1;\n"
                   + "".join(f'  if (!dlsym(lib, "{s}")) {{ fprintf(stderr, "missing {s}\\n"); return 2; }}\n' for s in SYMS)
                   + '  printf("ok %d %d %d %d %d %d %d %d %d\\n", BGNN_ROBUST_STAGE_HEADER_BYTES, BGNN_ROBUST_SLOT_BYTES,\n'
                     "         BGNN_ROBUST_MAX_CAPACITY, BGNN_ROBUST_MAX_CELLS, BGNN_ROBUST_WAVE_MAX, BGNN_ROBUST_LDS_MAX,\n"
                     "         BGNN_ROBUST_FLAG_KEPT, BGNN_ROBUST_FLAG_REJECTED, BGNN_ROBUST_FLAG_NOT_ACCEPTED);\n"
                     "  return 0;\n}\n")
    exe = tmp_path / "robust_abi"
    subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe),
                    "-ldl"], check=True)
    r = subprocess.run([str(exe), os.path.join(ROOT, "bathymetric-gnn_amd", "libbgnn_hip.so")], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.split() == ["ok"] + [str(v) for v in (
        runtime.ROBUST_STAGE_HEADER_BYTES, runtime.ROBUST_SLOT_BYTES, runtime.ROBUST_MAX_CAPACITY, runtime.ROBUST_MAX_CELLS,
        runtime.ROBUST_WAVE_MAX, runtime.ROBUST_LDS_MAX, 0, 1, 2)]
    assert runtime.ROBUST_FLAGS == ("kept", "rejected", "not_accepted")
    assert 1 < runtime.ROBUST_WAVE_MAX < runtime.ROBUST_LDS_MAX


def test_sizes(lib):
    """The stage is a function of the capacity alone, the workspace of the cell count and the capacity; both are 0 where there is
    no such stage or grid, and where the bytes would not fit size_t."""
    stage, work = lib.bgnn_soundings_robust_stage_bytes, lib.bgnn_soundings_robust_workspace_bytes
    assert stage(0) == 0 and stage(-1) == 0 and stage(2 ** 31) == 0 and stage(2 ** 62) == 0
    for cap in (1, 7, 20000, 2 ** 31 - 1):
        assert stage(cap) == 32 + 8 * cap
    assert work(0, 4, 10) == 0 and work(4, 0, 10) == 0 and work(4, 4, 0) == 0 and work(-1, 4, 10) == 0 and work(4, 4, 2 ** 31) == 0
    assert work(2 ** 31, 1, 10) == 0 and work(2 ** 16, 2 ** 15, 10) == 0          # 2^31 cells: one too many
    assert work(2 ** 31 - 1, 2 ** 31 - 1, 10) == 0 and work(2 ** 62, 2 ** 62, 2 ** 62) == 0      # (shapes whose bytes exceed size_t)
    small, more_cells, more_room = work(16, 16, 20000), work(160, 160, 20000), work(16, 16, 200000)
    assert 0 < small < more_cells and small < more_room
    assert small >= 4 * 256 + 4 * 20000 and small % 256 == 0
    top = work(2 ** 31 - 1, 1, 2 ** 31 - 1)                                       # the largest grid with the largest stage
    assert 16 * 2 ** 30 <= top < 2 ** 35
    assert work(46340, 46340, 1000) > 4 * 46340 * 46340


def test_refusals_before_any_launch(lib):
    """With a NULL context every call is refused, and the message names what is wrong with the other arguments first."""
    from bathymetric_gnn_amd import runtime
    buf = (C.c_int64 * 64)()
    p = C.cast(buf, C.c_void_p)
    odd = C.c_void_p(p.value + 4)

    def refused(word, rc, code=runtime.ERR_INVALID):
        assert rc == code, (rc, lib.bgnn_last_error())
        assert word in lib.bgnn_last_error(), lib.bgnn_last_error()

    add, fin, flag, reset = (lib.bgnn_soundings_robust_add, lib.bgnn_soundings_robust_finalize, lib.bgnn_soundings_robust_flag,
                             lib.bgnn_soundings_robust_reset)

    add_names = ["ctx", "x", "y", "z", "n", "x0", "y0", "res", "height", "width", "offered", "capacity", "stage"]
    add_ok = [None, p, p, p, 4, 0.0, 0.0, 0.5, 2, 2, 0, 8, p]  # everything in order but the context
    a = lambda **kw: add(*[kw.get(name, v) for name, v in zip(add_names, add_ok)])
    refused(b"NULL context", a())
    refused(b"NULL context", a(x=None, y=None, z=None, n=0))
    for name in ("x", "y", "z", "stage"):
        refused(b"NULL argument", a(**{name: None}))
    refused(b"resolution of 0", a(res=0.0))
    refused(b"resolution of nan", a(res=float("nan")))
    refused(b"origin", a(x0=float("inf")))
    refused(b"0 x 2 cells", a(height=0))
    refused(b"2147483648 x 2 cells", a(height=2 ** 31))
    refused(b"-5 soundings", a(n=-5))
    refused(b"-1 soundings offered before", a(offered=-1))
    refused(b"capacity of 0", a(capacity=0))
    refused(b"capacity of 2147483648", a(capacity=2 ** 31))
    refused(b"more than the capacity of 8", a(n=4, offered=5))                  # offered + n > capacity
    refused(b"more than the capacity of 8", a(n=9))
    refused(b"more than the capacity of 8", a(n=2 ** 62, offered=2 ** 62))
    refused(b"NULL context", a(n=4, offered=4))                                 # (the last ones that fit)
    refused(b"not 8-byte aligned", a(stage=odd))
    refused(b"more than 2147483647 in all", a(height=2 ** 16, width=2 ** 15), runtime.ERR_UNSUPPORTED)   # height * width = 2^31
    refused(b"NULL context", a(height=2 ** 31 - 1, width=1))

    fin_names = ["ctx", "stage", "offered", "capacity", "height", "width", "k", "floor_m", "min_count", "nodata", "ws", "ws_bytes",
                 "start", "sorted_q", "count", "kept", "median", "mad", "kept_mean", "kept_std", "kept_min", "kept_max", "valid",
                 "center2", "limit"]
    need = lib.bgnn_soundings_robust_workspace_bytes(2, 2, 8)
    fin_ok = [None, p, 8, 8, 2, 2, 4.4478, 0.0, 1, 1.0e6, p, need] + [p] * 13
    f = lambda **kw: fin(*[kw.get(name, v) for name, v in zip(fin_names, fin_ok)])
    refused(b"NULL context", f())
    for name in ["stage", "ws"] + fin_names[12:]:
        refused(b"NULL argument", f(**{name: None}))
    refused(b"multiplier k of 0.5", f(k=0.5))                                   # k < 1
    refused(b"multiplier k of nan", f(k=float("nan")))
    refused(b"multiplier k of inf", f(k=float("inf")))
    refused(b"NULL context", f(k=1.0))
    refused(b"floor of -0.01", f(floor_m=-0.01))
    refused(b"floor of nan", f(floor_m=float("nan")))
    refused(b"floor of inf", f(floor_m=float("inf")))
    refused(b"min_count of 0", f(min_count=0))
    refused(b"9 soundings offered", f(offered=9))
    refused(b"-1 soundings offered", f(offered=-1))
    refused(b"capacity of 0", f(capacity=0))
    refused(b"0 x 2 cells", f(height=0))
    refused(b"more than 2147483647 in all", f(height=2 ** 16, width=2 ** 15), runtime.ERR_UNSUPPORTED)
    refused(b"more than 2147483647 in all", f(height=2 ** 31 - 1, width=2 ** 31 - 1), runtime.ERR_UNSUPPORTED)
    refused(b"workspace of", f(ws_bytes=need - 1))
    refused(b"the stage is not 8-byte aligned", f(stage=odd))                   # misaligned stage
    refused(b"the workspace is not 8-byte aligned", f(ws=odd))
    refused(b"center2 or limit", f(center2=odd))
    refused(b"center2 or limit", f(limit=odd))

    flag_names = ["ctx", "x", "y", "z", "n", "x0", "y0", "res", "height", "width", "center2", "limit", "flags"]
    flag_ok = [None, p, p, p, 4, 0.0, 0.0, 0.5, 2, 2, p, p, p]
    g = lambda **kw: flag(*[kw.get(name, v) for name, v in zip(flag_names, flag_ok)])
    refused(b"NULL context", g())
    refused(b"NULL context", g(x=None, y=None, z=None, flags=None, n=0))
    for name in ("x", "y", "z", "center2", "limit", "flags"):
        refused(b"NULL argument", g(**{name: None}))
    refused(b"-1 soundings", g(n=-1))
    refused(b"resolution of -1", g(res=-1.0))
    refused(b"2 x 0 cells", g(width=0))
    refused(b"more than 2147483647 in all", g(height=2 ** 16, width=2 ** 15), runtime.ERR_UNSUPPORTED)
    refused(b"center2 or limit", g(limit=odd))

    refused(b"NULL context", reset(None, p))
    refused(b"NULL argument", reset(None, None))
    refused(b"not 8-byte aligned", reset(None, odd))
    assert not any(buf)
