"""The depth-hypotheses part of the C ABI (include/bgnn_hypotheses.h) is plain C like bgnn.h: it compiles as C99 (-pedantic), a C
program resolves every entry point it declares with dlsym, and the ctypes binding (runtime._HYPOTHESES_SIGNATURES) covers exactly
that set -- beside, not inside, every other pinned symbol set, at the same ABI number.  The refusals, all of which come before
anything is launched, are exercised with a NULL context: each returns its code and a message.  No GPU needed."""
import ctypes as C
import glob
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMS = ["bgnn_hypotheses_build", "bgnn_hypotheses_workspace_bytes"]


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


def test_hypotheses_symbols_exported_and_bound(lib):
    from bathymetric_gnn_amd import runtime
    syms = _declared(os.path.join(ROOT, "include", "bgnn_hypotheses.h"))
    assert syms == SYMS
    assert sorted(runtime._HYPOTHESES_SIGNATURES) == syms
    tables = {k: v for k, v in vars(runtime).items() if k.endswith("_SIGNATURES") and isinstance(v, dict)}
    assert "_HYPOTHESES_SIGNATURES" in tables and "_ROBUST_SIGNATURES" in tables and len(tables) >= 22
    for name, table in tables.items():
        if name != "_HYPOTHESES_SIGNATURES":
            assert not set(syms) & set(table), name
    headers = sorted(glob.glob(os.path.join(ROOT, "include", "*.h")))
    assert len(headers) >= 22
    for h in headers:
        if os.path.basename(h) != "bgnn_hypotheses.h":
            assert not set(syms) & set(_declared(h)), h
    for s in syms:
        assert hasattr(lib, s), f"{s} declared in bgnn_hypotheses.h but not exported"
        assert getattr(lib, s).argtypes == runtime._HYPOTHESES_SIGNATURES[s][1]
        assert getattr(lib, s).restype == runtime._HYPOTHESES_SIGNATURES[s][0]
    assert len(runtime._HYPOTHESES_SIGNATURES["bgnn_hypotheses_build"][1]) == 26
    assert lib.bgnn_abi_version() == 7 == runtime.ABI_VERSION


def test_hypotheses_header_is_plain_c(tmp_path, lib):
    if shutil.which("gcc") is None:
        pytest.skip("no gcc")
    from bathymetric_gnn_amd import runtime
    src = tmp_path / "hyp_abi.c"
    src.write_text('#include <dlfcn.h>\n#include <stdio.h>\n#include "bgnn_hypotheses.h"\n'
                   "int main(int argc, char **argv) {\n"
                   "  void *lib = dlopen(argv[1], RTLD_NOW | RTLD_LOCAL);\n"
                   "  if (argc < 2 || !lib) return 1;\n"
                   + "".join(f'  if (!dlsym(lib, "{s}")) {{ fprintf(stderr, "missing {s}\\n"); return 2; }}\n' for s in SYMS)
                   + '  printf("ok %d %d %d %d %lld\\n", BGNN_HYP_RULE_COUNT, BGNN_HYP_RULE_GUIDE, BGNN_HYP_MAX_CELLS,\n'
                     "         BGNN_HYP_MAX_CAPACITY, (long long)BGNN_HYP_MAX_GAP_Q);\n"
                     "  return 0;\n}\n")
    exe = tmp_path / "hyp_abi"
    subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe),
                    "-ldl"], check=True)
    r = subprocess.run([str(exe), os.path.join(ROOT, "bathymetric-gnn_amd", "libbgnn_hip.so")], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.split() == ["ok"] + [str(v) for v in (
        runtime.HYP_RULES.index("count"), runtime.HYP_RULES.index("guide"), runtime.HYP_MAX_CELLS, runtime.HYP_MAX_CAPACITY,
        runtime.HYP_MAX_GAP_Q)]
    assert runtime.HYP_MAX_CELLS == runtime.ROBUST_MAX_CELLS and runtime.HYP_MAX_CAPACITY == runtime.ROBUST_MAX_CAPACITY


def test_workspace_size(lib):
    """A function of the cell count and the capacity; 0 outside the limits."""
    work = lib.bgnn_hypotheses_workspace_bytes
    assert work(0, 10) == 0 and work(-1, 10) == 0 and work(2 ** 31, 10) == 0 and work(4, 0) == 0 and work(4, -3) == 0
    assert work(4, 2 ** 31) == 0 and work(2 ** 62, 2 ** 62) == 0
    small, more_cells, more_room = work(256, 20000), work(2 ** 22, 20000), work(256, 2000000)
    assert 0 < small < more_cells and small < more_room and small % 256 == 0
    assert small >= 256 + 256 + 4 * (20000 // 65 + 1)
    top = work(2 ** 31 - 1, 2 ** 31 - 1)
    assert 4 * (2 ** 31 // 65) < top < 2 ** 28


def test_refusals_before_any_launch(lib):
    """With a NULL context every call is refused, and the message names what is wrong with the other arguments first."""
    from bathymetric_gnn_amd import runtime
    buf = (C.c_int64 * 64)()
    p = C.cast(buf, C.c_void_p)
    odd = C.c_void_p(p.value + 4)

    def refused(word, rc, code=runtime.ERR_INVALID):
        assert rc == code, (rc, lib.bgnn_last_error())
        assert word in lib.bgnn_last_error(), lib.bgnn_last_error()

    planes = ["n_hyp", "chosen", "kept", "depth", "std", "min", "max", "share", "valid", "center2", "limit"]
    records = ["hyp_start", "hyp_first", "hyp_count"]
    names = ["ctx", "start", "sorted_q", "cells", "capacity", "gap_q", "rule", "guide", "min_count", "nodata", "ws", "ws_bytes"] + \
        planes + records
    need = lib.bgnn_hypotheses_workspace_bytes(4, 8)
    ok = [None, p, p, 4, 8, 32768, 0, None, 1, 1.0e6, p, need] + [p] * 11 + [p] * 3
    b = lambda **kw: lib.bgnn_hypotheses_build(*[kw.get(name, v) for name, v in zip(names, ok)])
    refused(b"NULL context", b())
    refused(b"NULL context", b(hyp_start=None, hyp_first=None, hyp_count=None))                  # no records
    refused(b"NULL context", b(rule=1, guide=p))
    for name in ["start", "sorted_q", "ws"] + planes:
        refused(b"NULL argument", b(**{name: None}))
    refused(b"0 cells", b(cells=0))
    refused(b"-1 cells", b(cells=-1))
    refused(b"2147483648 cells", b(cells=2 ** 31))
    refused(b"capacity of 0", b(capacity=0))
    refused(b"capacity of 2147483648", b(capacity=2 ** 31))
    refused(b"gap_q of -1", b(gap_q=-1))
    refused(b"gap_q of 4294967297", b(gap_q=2 ** 32 + 1))
    refused(b"NULL context", b(gap_q=2 ** 32))
    refused(b"NULL context", b(gap_q=0))
    refused(b"unknown rule 2", b(rule=2))
    refused(b"unknown rule -1", b(rule=-1))
    refused(b"a guide with the count rule", b(guide=p))
    refused(b"no guide with the guide rule", b(rule=1))
    refused(b"min_count of 0", b(min_count=0))
    refused(b"workspace of", b(ws_bytes=need - 1))
    refused(b"the workspace is not 8-byte aligned", b(ws=odd))
    refused(b"center2 or limit", b(center2=odd))
    refused(b"center2 or limit", b(limit=odd))
    for given in records:
        refused(b"records given in part", b(**{name: None for name in records if name != given}))
        refused(b"records given in part", b(**{given: None}))
    refused(b"NULL context", b(cells=2 ** 31 - 1, capacity=2 ** 31 - 1, ws_bytes=lib.bgnn_hypotheses_workspace_bytes(2 ** 31 - 1, 2 ** 31 - 1)))
    assert not any(buf)
