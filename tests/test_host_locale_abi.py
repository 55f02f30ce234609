"""The locale part of the C ABI (include/bgnn_locale.h) is plain C like bgnn.h: it compiles as C99 (-pedantic), a C program
resolves the entry point it declares with dlsym, and the ctypes binding (runtime._LOCALE_SIGNATURES) covers exactly that -- beside,
not inside, every other pinned symbol set, at the same ABI number.  The refusals, all of which come before anything is launched,
are exercised with a NULL context: each returns its code and a message that names what is wrong.  No GPU needed."""
import ctypes as C
import glob
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMS = ["bgnn_locale_guide"]


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


def test_locale_symbol_exported_and_bound(lib):
    from bathymetric_gnn_amd import runtime
    syms = _declared(os.path.join(ROOT, "include", "bgnn_locale.h"))
    assert syms == SYMS
    assert sorted(runtime._LOCALE_SIGNATURES) == syms
    tables = {k: v for k, v in vars(runtime).items() if k.endswith("_SIGNATURES") and isinstance(v, dict)}
    assert "_LOCALE_SIGNATURES" in tables and "_HYPOTHESES_SIGNATURES" in tables and len(tables) >= 23
    for name, table in tables.items():
        if name != "_LOCALE_SIGNATURES":
            assert not set(syms) & set(table), name
    headers = sorted(glob.glob(os.path.join(ROOT, "include", "*.h")))
    assert len(headers) >= 23
    for h in headers:
        if os.path.basename(h) != "bgnn_locale.h":
            assert not set(syms) & set(_declared(h)), h
    for s in syms:
        assert hasattr(lib, s), f"{s} declared in bgnn_locale.h but not exported"
        assert getattr(lib, s).argtypes == runtime._LOCALE_SIGNATURES[s][1]
        assert getattr(lib, s).restype == runtime._LOCALE_SIGNATURES[s][0]
    assert len(runtime._LOCALE_SIGNATURES["bgnn_locale_guide"][1]) == 10
    assert lib.bgnn_abi_version() == 7 == runtime.ABI_VERSION
    assert runtime.HYP_RULES == ("count", "guide")                       # the C rule codes did not change
    assert "bgnn_locale.h" in runtime.load_library.__doc__


def test_locale_header_is_plain_c(tmp_path, lib):
    if shutil.which("gcc") is None:
        pytest.skip("no gcc")
    from bathymetric_gnn_amd import runtime
    src = tmp_path / "locale_abi.c"
    src.write_text('#include <dlfcn.h>\n#include <stdio.h>\n#include "bgnn_locale.h"\n'
                   "int main(int argc, char **argv) {\n"
                   "  void *lib = dlopen(argv[1], RTLD_NOW | RTLD_LOCAL);\n"
                   "  if (argc < 2 || !lib) return 1;\n"
                   + "".join(f'  if (!dlsym(lib, "{s}")) {{ fprintf(stderr, "missing {s}\\n"); return 2; }}\n' for s in SYMS)
                   + '  printf("ok %d\\n", BGNN_LOCALE_MAX_RADIUS);\n'
                     "  return 0;\n}\n")
    exe = tmp_path / "locale_abi"
    subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe),
                    "-ldl"], check=True)
    r = subprocess.run([str(exe), os.path.join(ROOT, "bathymetric-gnn_amd", "libbgnn_hip.so")], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.split() == ["ok", str(runtime.LOCALE_MAX_RADIUS)] and runtime.LOCALE_MAX_RADIUS == 8


def test_refusals_before_any_launch(lib):
    """With a NULL context every call is refused, and the message names what is wrong with the other arguments first."""
    from bathymetric_gnn_amd import runtime
    buf = (C.c_int64 * 64)()
    p = C.cast(buf, C.c_void_p)
    odd = C.c_void_p(p.value + 4)

    def refused(word, rc, code=runtime.ERR_INVALID):
        assert rc == code, (rc, lib.bgnn_last_error())
        assert word in lib.bgnn_last_error(), lib.bgnn_last_error()

    names = ["ctx", "n_hyp", "chosen", "center2", "height", "width", "radius", "min_support", "guide", "support"]
    ok = [None, p, p, p, 4, 8, 2, 3, p, p]
    g = lambda **kw: lib.bgnn_locale_guide(*[kw.get(name, v) for name, v in zip(names, ok)])
    refused(b"bgnn_locale_guide: NULL context", g())
    for name in ("n_hyp", "chosen", "center2", "guide", "support"):
        refused(b"NULL argument", g(**{name: None}))
    refused(b"0 x 8 cells", g(height=0))
    refused(b"4 x 0 cells", g(width=0))
    refused(b"-1 x 8 cells", g(height=-1))
    refused(b"4 x -3 cells", g(width=-3))
    refused(b"65536 x 32768 cells, 2147483647 at the most", g(height=65536, width=32768))          # 2^31
    refused(b"2147483648 x 1 cells", g(height=2 ** 31, width=1))
    refused(b"4611686018427387904 x 4611686018427387904 cells", g(height=2 ** 62, width=2 ** 62))
    refused(b"NULL context", g(height=2 ** 31 - 1, width=1))
    refused(b"NULL context", g(height=1, width=2 ** 31 - 1))
    refused(b"NULL context", g(height=46340, width=46341))                                         # 2147441940
    refused(b"radius of 0", g(radius=0))
    refused(b"radius of -1", g(radius=-1))
    refused(b"radius of 9, 1 .. 8 expected", g(radius=9))
    for radius in range(1, 9):
        top = (2 * radius + 1) ** 2 - 1
        refused(b"NULL context", g(radius=radius, min_support=1))
        refused(b"NULL context", g(radius=radius, min_support=top))
        refused(b"min_support of 0", g(radius=radius, min_support=0))
        refused(f"min_support of {top + 1}, 1 .. {top} expected".encode(), g(radius=radius, min_support=top + 1))
    refused(b"min_support of -5", g(min_support=-5))
    refused(b"center2 is not 8-byte aligned", g(center2=odd))
    refused(b"NULL context", g(n_hyp=odd, chosen=odd, guide=odd, support=odd))                     # int32 and float planes: 4 bytes do
    # the order of the checks: what comes first in the contract is named first
    refused(b"NULL argument", g(guide=None, height=0, radius=0, min_support=0, center2=None))
    refused(b"0 x 8 cells", g(height=0, radius=0, min_support=0, center2=odd))
    refused(b"radius of 0", g(radius=0, min_support=0, center2=odd))
    refused(b"min_support of 0", g(min_support=0, center2=odd))
    assert not any(buf)
