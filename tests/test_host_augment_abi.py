"""The C ABI of the tile gather under the symmetries of the square without a GPU (include/bgnn_augment.h): every symbol exported and
bound, beside the other headers' sets at ABI 7; the constants and the entry's layout; the workspace formula; the refusals, all of
which come before any use of the context or the device."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from bathymetric_gnn_amd import runtime

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMS = ["bgnn_tile_gather", "bgnn_tile_gather_workspace_bytes"]
ARGS = {"bgnn_tile_gather": 12, "bgnn_tile_gather_workspace_bytes": 1}
SIGNATURES = runtime._AUGMENT_SIGNATURES


def _header(name="bgnn_augment.h"):
    return open(os.path.join(ROOT, "include", name)).read()


def _declared(name):
    text = re.sub(r"/\*.*?\*/", "", _header(name), flags=re.S)
    return {m.group(1): m.group(2) for m in re.finditer(r"\b(bgnn_[a-z_0-9]+)\s*\(([^)]*)\)", text)}


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(runtime.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return runtime.load_library()


def test_augment_symbols_exported_and_bound(lib):
    decl = _declared("bgnn_augment.h")
    assert sorted(decl) == SYMS and sorted(SIGNATURES) == SYMS
    tables = [getattr(runtime, n) for n in dir(runtime) if n.endswith("_SIGNATURES") and n != "_AUGMENT_SIGNATURES"]
    assert len(tables) >= 14 and runtime._TILESTORE_SIGNATURES in tables
    for table in tables:
        assert not set(SYMS) & set(table)
    for h in sorted(os.listdir(os.path.join(ROOT, "include"))):
        if h.endswith(".h") and h != "bgnn_augment.h":
            assert not set(SYMS) & set(_declared(h)), h
    for s in SYMS:
        assert hasattr(lib, s), f"{s} declared in bgnn_augment.h but not exported"
        assert len(decl[s].split(",")) == ARGS[s] == len(SIGNATURES[s][1]), s
        assert getattr(lib, s).argtypes == SIGNATURES[s][1]
        assert getattr(lib, s).restype == SIGNATURES[s][0]
    assert lib.bgnn_abi_version() == 7 == runtime.ABI_VERSION


def test_constants_and_entry_layout_match_the_header():
    d = {k: int(v) for k, v in re.findall(r"#define\s+(BGNN_AUG_[A-Z_0-9]+)\s+(\d+)\b", _header())}
    assert d["BGNN_AUG_OPS"] == runtime.AUG_OPS == 8
    assert d["BGNN_AUG_MAX_PLANES"] == runtime.AUG_MAX_PLANES == 4
    assert d["BGNN_AUG_BLOCK"] == runtime.AUG_BLOCK == 64
    dt = runtime.TILE_ENTRY_DTYPE
    assert d["BGNN_AUG_ENTRY_BYTES"] == dt.itemsize == runtime.AUG_ENTRY_BYTES == 32
    assert [dt.fields[k][1] for k in ("src", "dst", "h", "w", "op", "pad")] == [0, 8, 16, 20, 24, 28]


def test_augment_header_is_plain_c_and_the_entry_has_32_bytes(tmp_path, lib):
    if shutil.which("gcc") is None:
        pytest.skip("no gcc")
    src = tmp_path / "augment_abi.c"
    src.write_text('#include <dlfcn.h>\n#include <stddef.h>\n#include <stdio.h>\n#include "bgnn_augment.h"\n'
                   "int main(int argc, char **argv) {\n"
                   "  void *lib = dlopen(argv[1], RTLD_NOW | RTLD_LOCAL);\n"
                   "  if (argc < 2 || !lib) return 1;\n"
                   + "".join(f'  if (!dlsym(lib, "{s}")) {{ fprintf(stderr, "missing {s}\\n"); return 2; }}\n' for s in SYMS)
                   + '  printf("ok %d %d %d %d %d\\n", (int)sizeof(bgnn_tile_entry), BGNN_AUG_ENTRY_BYTES, (int)offsetof(bgnn_tile_entry, dst),\n'
                     "         (int)offsetof(bgnn_tile_entry, h), (int)offsetof(bgnn_tile_entry, op));\n  return 0;\n}\n")
    exe = tmp_path / "augment_abi"
    subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe),
                    "-ldl"], check=True)
    r = subprocess.run([str(exe), runtime.LIB_PATH], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.split() == ["ok", "32", "32", "8", "16", "24"]


def test_workspace_bytes_is_a_formula(lib):
    ws = lib.bgnn_tile_gather_workspace_bytes
    assert ws(0) == 0 and ws(1) == 256 and ws(8) == 256 and ws(9) == 512 and ws(2000) == (2000 * 32 + 255) // 256 * 256
    assert ws(-1) == 0 and ws(2 ** 31 - 1) == (2 ** 31 - 1) * 32 + 32 and ws(2 ** 31) == 0


def test_hostside_refusals(lib):
    """Every argument check comes before any use of the context or the device.  (The context here is a host buffer: a call that
    touched it, or launched anything, would not come back with these codes.)"""
    buf = (C.c_int64 * 8192)()
    base = C.addressof(buf) + (-C.addressof(buf)) % 16
    at = lambda off: C.c_void_p(base + off)
    p = at(0)
    SRC, DST = 4096, 20480                                  # byte offsets of the source and destination stores: 1000 cells each fit
    entry = lambda *rows: np.array([r + (0,) for r in rows], dtype=runtime.TILE_ENTRY_DTYPE)
    good = entry((0, 0, 4, 5, 3))
    four = lambda off: (C.c_void_p * 4)(base + off, None, base + off + 4000, None)

    def gather(**kw):
        a = {**dict(ctx=p, src=four(SRC), dst=four(DST), n_planes=4, src_mask=at(SRC + 8000), dst_mask=at(DST + 8000), src_cells=1000,
                    dst_cells=1000, entries=good, n=1, ws=at(1024), ws_bytes=256), **kw}
        e = a["entries"]
        a["entries"] = None if e is None else C.c_void_p(e.ctypes.data)
        return lib.bgnn_tile_gather(*a.values())
    err = lambda: lib.bgnn_last_error()
    INVALID = runtime.ERR_INVALID
    for name in ("ctx", "src", "dst", "entries", "ws"):
        assert gather(**{name: None}) == INVALID and b"NULL" in err(), name
    for op in (-1, 8, 1 << 20):
        assert gather(entries=entry((0, 0, 4, 5, op))) == INVALID and b"names no op" in err(), op
    for h, w in ((0, 5), (4, 0), (-3, 5), (4, -1)):
        assert gather(entries=entry((0, 0, h, w, 0))) == INVALID and b"is empty" in err(), (h, w)
    assert gather(entries=entry((-1, 0, 4, 5, 0))) == INVALID and b"negative offset" in err()
    assert gather(entries=entry((0, -1, 4, 5, 0))) == INVALID and b"negative offset" in err()
    assert gather(entries=entry((981, 0, 4, 5, 0))) == INVALID and b"source store" in err()
    assert gather(entries=entry((0, 981, 4, 5, 0))) == INVALID and b"destination store" in err()
    assert gather(entries=entry((0, 0, 4, 5, 0), (980, 980, 4, 5, 7), (980, 981, 4, 5, 7)), n=3, ws_bytes=0) == INVALID and \
        b"entry 2" in err()                                                      # (980 + 20 = 1000 fits: the third entry is the first bad one)
    assert gather(entries=entry((0, 0, 1 << 30, 1 << 30, 0))) == INVALID and b"source store" in err()            # h * w does not wrap
    assert gather(entries=entry((2 ** 62, 0, 4, 5, 0))) == INVALID and gather(entries=entry((0, 2 ** 62, 4, 5, 0))) == INVALID
    assert gather(src_cells=-1) == INVALID and gather(dst_cells=-1) == INVALID and gather(n=-1) == INVALID
    assert gather(n=2 ** 31) == runtime.ERR_UNSUPPORTED
    half = (C.c_void_p * 4)(base + SRC, None, None, None)
    assert gather(src=half) == INVALID and b"plane 2" in err()
    assert gather(dst=half) == INVALID and b"plane 2" in err()
    assert gather(src_mask=None) == INVALID and b"byte plane" in err()
    assert gather(dst_mask=None) == INVALID and b"byte plane" in err()
    assert gather(n_planes=5) == INVALID and b"at most 4" in err()
    assert gather(n_planes=-1) == INVALID
    none = (C.c_void_p * 4)(None, None, None, None)
    assert gather(src=none, dst=none, src_mask=None, dst_mask=None) == INVALID and b"no plane" in err()
    assert gather(ws_bytes=255) == INVALID and b"workspace" in err()
    assert gather(ws=at(1032)) == INVALID and b"aligned" in err()
    odd = (C.c_void_p * 4)(base + SRC + 2, None, base + SRC + 4000, None)
    assert gather(src=odd) == INVALID and b"aligned" in err()
    # a destination on a source: word on word, word on the byte plane, the byte plane on a word plane, byte on byte
    assert gather(dst=four(SRC + 3996)) == INVALID and b"overlaps" in err()
    assert gather(dst=(C.c_void_p * 4)(base + DST, None, base + SRC + 8996, None)) == INVALID and b"overlaps" in err()
    assert gather(dst_mask=at(SRC + 7999)) == INVALID and b"overlaps" in err()
    assert gather(dst_mask=at(SRC + 8999)) == INVALID and b"overlaps" in err()
    # n_entries == 0: nothing to check further, nothing launched (entries and ws may be NULL)
    assert gather(n=0, entries=None, ws=None, ws_bytes=0) == 0
