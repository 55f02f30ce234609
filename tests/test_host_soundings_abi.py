"""The sounding-gridder part of the C ABI (include/bgnn_soundings.h) is plain C like bgnn.h: it compiles as C99 (-pedantic), a C
program resolves every entry point it declares with dlsym, and the ctypes binding (runtime._SOUNDINGS_SIGNATURES) covers exactly
that set -- beside, not inside, every other pinned symbol set, at the same ABI number.  The refusals that need no device (they are
checked before anything is launched) are exercised with a NULL context.  No GPU needed."""
import ctypes as C
import glob
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMS = ["bgnn_soundings_add", "bgnn_soundings_extent", "bgnn_soundings_finalize", "bgnn_soundings_reset", "bgnn_soundings_state_bytes"]


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


def test_soundings_symbols_exported_and_bound(lib):
    from bathymetric_gnn_amd import runtime
    syms = _declared(os.path.join(ROOT, "include", "bgnn_soundings.h"))
    assert syms == SYMS
    assert sorted(runtime._SOUNDINGS_SIGNATURES) == syms
    tables = {k: v for k, v in vars(runtime).items() if k.endswith("_SIGNATURES") and isinstance(v, dict)}
    assert "_SOUNDINGS_SIGNATURES" in tables and "_CURVE_SIGNATURES" in tables and len(tables) >= 17
    for name, table in tables.items():
        if name != "_SOUNDINGS_SIGNATURES":
            assert not set(syms) & set(table), name
    headers = sorted(glob.glob(os.path.join(ROOT, "include", "*.h")))
    assert len(headers) >= 17
    for h in headers:
        if os.path.basename(h) != "bgnn_soundings.h":
            assert not set(syms) & set(_declared(h)), h
    for s in syms:
        assert hasattr(lib, s), f"{s} declared in bgnn_soundings.h but not exported"
        assert getattr(lib, s).argtypes == runtime._SOUNDINGS_SIGNATURES[s][1]
        assert getattr(lib, s).restype == runtime._SOUNDINGS_SIGNATURES[s][0]
    assert lib.bgnn_abi_version() == 7 == runtime.ABI_VERSION


def test_soundings_header_is_plain_c(tmp_path, lib):
    if shutil.which("gcc") is None:
        pytest.skip("no gcc")
    from bathymetric_gnn_amd import runtime
    src = tmp_path / "soundings_abi.c"
    src.write_text('#include <dlfcn.h>\n#include <stdio.h>\n#include "bgnn_soundings.h"\n'
                   "int main(int argc, char **argv) {\n"
                   "  void *lib = dlopen(argv[1], RTLD_NOW | RTLD_LOCAL);\n"
                   "  if (argc < 2 || !lib) return 1;\n"
                   + "".join(f'  if (!dlsym(lib, "{s}")) {{ fprintf(stderr, "missing {s}\\n"); return 2; }}\n' for s in SYMS)
                   + '  printf("ok %d %d %d %d %d %d %d\\n", BGNN_SOUNDINGS_HEADER_BYTES, BGNN_SOUNDINGS_CELL_BYTES, BGNN_SOUNDINGS_MAX_TOTAL,\n'
                     "         BGNN_SOUNDINGS_Z_CAP, BGNN_SOUNDINGS_SCALE, BGNN_SOUNDINGS_EXTENT_BYTES, BGNN_SOUNDINGS_EXTENT_BUFFER_BYTES);\n"
                     "  return 0;\n}\n")
    exe = tmp_path / "soundings_abi"
    subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe),
                    "-ldl"], check=True)
    r = subprocess.run([str(exe), os.path.join(ROOT, "bathymetric-gnn_amd", "libbgnn_hip.so")], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.split() == ["ok"] + [str(v) for v in (
        runtime.SOUNDINGS_HEADER_BYTES, runtime.SOUNDINGS_CELL_BYTES, runtime.SOUNDINGS_MAX_TOTAL, runtime.SOUNDINGS_Z_CAP,
        runtime.SOUNDINGS_SCALE, runtime.SOUNDINGS_EXTENT_DTYPE.itemsize, runtime.SOUNDINGS_EXTENT_BUFFER_BYTES)]
    assert len(runtime.SOUNDINGS_COUNTERS) * 8 == runtime.SOUNDINGS_HEADER_BYTES


def test_state_sizes_and_hostside_refusals(lib):
    """The state is a function of the cell count alone and 0 where there is no grid.  With a NULL context every call is refused,
    and the message names what is wrong with the other arguments first: a NULL plane, a resolution that is not above 0, a grid
    without rows, a negative number of soundings, a total above 2^31 - 1, a misaligned state."""
    from bathymetric_gnn_amd import runtime
    size = lib.bgnn_soundings_state_bytes
    assert size(0, 5) == 0 and size(5, 0) == 0 and size(-1, 5) == 0 and size(2 ** 31, 1) == 0
    for H, W in ((1, 1), (16, 16), (1, 4096), (60000, 60000), (2 ** 31 - 1, 2 ** 27)):
        assert size(H, W) == 32 + 40 * H * W
    assert size(2 ** 31 - 1, 2 ** 31 - 1) == 0                  # (more bytes than size_t holds)
    buf = (C.c_int64 * 64)()
    p = C.cast(buf, C.c_void_p)
    odd = C.c_void_p(p.value + 4)

    def refused(word, rc):
        assert rc == runtime.ERR_INVALID
        assert word in lib.bgnn_last_error(), lib.bgnn_last_error()

    add, fin, ext, reset = lib.bgnn_soundings_add, lib.bgnn_soundings_finalize, lib.bgnn_soundings_extent, lib.bgnn_soundings_reset
    ok = [None, p, p, p, 4, 0.0, 0.0, 0.5, 2, 2, 0, p]          # everything in order but the context
    refused(b"NULL context", add(*ok))
    refused(b"NULL context", add(None, None, None, None, 0, 0.0, 0.0, 0.5, 2, 2, 0, p))       # (no soundings: no planes needed)
    for k in (1, 2, 3, 11):                                     # x, y, z, state
        refused(b"NULL argument", add(*[None if j == k else v for j, v in enumerate(ok)]))

    def with_(**kw):
        names = ["ctx", "x", "y", "z", "n", "x0", "y0", "res", "height", "width", "offered", "state"]
        return [kw.get(name, v) for name, v in zip(names, ok)]

    refused(b"resolution of 0", add(*with_(res=0.0)))
    refused(b"resolution of -0.5", add(*with_(res=-0.5)))
    refused(b"resolution of nan", add(*with_(res=float("nan"))))
    refused(b"resolution of inf", add(*with_(res=float("inf"))))
    refused(b"origin", add(*with_(x0=float("inf"))))
    refused(b"origin", add(*with_(y0=float("nan"))))
    refused(b"0 x 2 cells", add(*with_(height=0)))
    refused(b"2 x -3 cells", add(*with_(width=-3)))
    refused(b"2147483648 x 2 cells", add(*with_(height=2 ** 31)))
    refused(b"-5 soundings", add(*with_(n=-5)))
    refused(b"-1 soundings offered before", add(*with_(offered=-1)))
    refused(b"a total above 2147483647", add(*with_(n=2, offered=2 ** 31 - 2)))
    refused(b"a total above 2147483647", add(*with_(n=2 ** 31)))
    refused(b"a total above 2147483647", add(*with_(n=2 ** 62, offered=2 ** 62)))
    refused(b"NULL context", add(*with_(n=1, offered=2 ** 31 - 2)))                           # (the last one that fits)
    refused(b"not 8-byte aligned", add(*with_(state=odd)))

    fok = [None, p, 2, 2, 1, 1.0e6, p, p, p, p, p, p]
    refused(b"NULL context", fin(*fok))
    for k in (1, 6, 7, 8, 9, 10, 11):                           # state and the six planes
        refused(b"NULL argument", fin(*[None if j == k else v for j, v in enumerate(fok)]))
    refused(b"0 x 2 cells", fin(None, p, 0, 2, 1, 1.0e6, p, p, p, p, p, p))
    refused(b"min_count of 0", fin(None, p, 2, 2, 0, 1.0e6, p, p, p, p, p, p))
    refused(b"not 8-byte aligned", fin(None, odd, 2, 2, 1, 1.0e6, p, p, p, p, p, p))

    refused(b"NULL context", ext(None, p, p, 4, p))
    refused(b"NULL context", ext(None, None, None, 0, p))
    refused(b"NULL argument", ext(None, None, p, 4, p))
    refused(b"NULL argument", ext(None, p, p, 4, None))
    refused(b"-1 soundings", ext(None, p, p, -1, p))
    refused(b"not 8-byte aligned", ext(None, p, p, 4, odd))

    refused(b"NULL context", reset(None, p, 2, 2))
    refused(b"NULL argument", reset(None, None, 2, 2))
    refused(b"2 x 0 cells", reset(None, p, 2, 0))
    refused(b"not 8-byte aligned", reset(None, odd, 2, 2))
    assert not any(buf)
