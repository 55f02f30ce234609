"""The C ABI of the error percentiles without a GPU (include/bgnn_quantile.h): the four symbols exported and bound in a table of their
own (runtime._QUANTILE_SIGNATURES) beside, not inside, every other pinned symbol set, at the same ABI number; the published byte
offsets against the runtime's records; the header as plain C; every argument refusal, all of which come before any use of the
context or the device."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from bathymetric_gnn_amd import runtime

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMS = ["bgnn_quantile_add", "bgnn_quantile_reset", "bgnn_quantile_select", "bgnn_quantile_workspace_bytes"]
ARGS = {"bgnn_quantile_add": 8, "bgnn_quantile_reset": 2, "bgnn_quantile_select": 9, "bgnn_quantile_workspace_bytes": 1}
SIGNATURES = runtime._QUANTILE_SIGNATURES


def _header(name="bgnn_quantile.h"):
    return open(os.path.join(ROOT, "include", name)).read()


def _declared(name):
    text = re.sub(r"/\*.*?\*/", "", _header(name), flags=re.S)
    return {m.group(1): m.group(2) for m in re.finditer(r"\b(bgnn_[a-z_0-9]+)\s*\(([^)]*)\)", text)}


def _defines():
    text = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    raw = dict(re.findall(r"#define[ \t]+(BGNN_QUANTILE_[A-Z_0-9]+)[ \t]+(\S.*)", text))
    out = {}
    for _ in range(3):                                          # (a define may use an earlier one)
        for k, v in raw.items():
            try:
                out[k] = int(eval(v, {"__builtins__": {}}, dict(out)))
            except NameError:
                pass
    assert sorted(out) == sorted(raw)
    return out


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(runtime.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return runtime.load_library()


def test_quantile_symbols_exported_and_bound(lib):
    decl = _declared("bgnn_quantile.h")
    assert sorted(decl) == SYMS and sorted(SIGNATURES) == SYMS
    tables = {n: getattr(runtime, n) for n in dir(runtime) if n.endswith("_SIGNATURES") and n != "_QUANTILE_SIGNATURES"}
    assert len(tables) >= 20 and "_SIGNATURES" in tables and "_TRAINER_SIGNATURES" in tables
    for name, table in tables.items():
        assert not set(SYMS) & set(table), name
    for h in sorted(os.listdir(os.path.join(ROOT, "include"))):
        if h.endswith(".h") and h != "bgnn_quantile.h":
            assert not set(SYMS) & set(_declared(h)), h
    for s in SYMS:
        assert hasattr(lib, s), f"{s} declared in bgnn_quantile.h but not exported"
        assert len(decl[s].split(",")) == ARGS[s] == len(SIGNATURES[s][1]), s
        assert getattr(lib, s).argtypes == SIGNATURES[s][1]
        assert getattr(lib, s).restype == SIGNATURES[s][0]
    assert lib.bgnn_abi_version() == 7 == runtime.ABI_VERSION


def test_offsets_match_the_header():
    d = _defines()
    st, out = runtime.QUANTILE_STATE_DTYPE, runtime.QUANTILE_OUT_DTYPE
    assert {k: st.fields[k][1] for k in ("rows", "filed", "nonfinite", "dropped", "cursor", "hist")} == {
        "rows": d["BGNN_QUANTILE_ST_ROWS"], "filed": d["BGNN_QUANTILE_ST_FILED"], "nonfinite": d["BGNN_QUANTILE_ST_NONFINITE"],
        "dropped": d["BGNN_QUANTILE_ST_DROPPED"], "cursor": d["BGNN_QUANTILE_ST_CURSOR"], "hist": d["BGNN_QUANTILE_ST_HIST"]}
    assert st.itemsize == d["BGNN_QUANTILE_STATE_BYTES"] == runtime.QUANTILE_STATE_BYTES == 64 + 4 * 2048
    assert st.fields["hist"][0].shape == (1 << d["BGNN_QUANTILE_TOP_BITS"],) and st.fields["hist"][0].base == np.dtype("<u4")
    assert {k: out.fields[k][1] for k in ("count", "nonfinite", "dropped", "rows", "ranks")} == {
        "count": d["BGNN_QUANTILE_OUT_COUNT"], "nonfinite": d["BGNN_QUANTILE_OUT_NONFINITE"], "dropped": d["BGNN_QUANTILE_OUT_DROPPED"],
        "rows": d["BGNN_QUANTILE_OUT_ROWS"], "ranks": d["BGNN_QUANTILE_OUT_RANKS"]}
    rank = out.fields["ranks"][0].base
    assert rank.itemsize == d["BGNN_QUANTILE_OUT_RANK_BYTES"] == 24
    assert [(n, rank.fields[n][1], rank.fields[n][0].str) for n in rank.names] == [("lo", 0, "<i8"), ("hi", 8, "<i8"), ("v_lo", 16, "<f4"),
                                                                                   ("v_hi", 20, "<f4")]
    assert out.itemsize == d["BGNN_QUANTILE_OUT_BYTES"] == runtime.QUANTILE_OUT_BYTES == 104
    assert runtime.QUANTILE_MAX_FRACTIONS == d["BGNN_QUANTILE_MAX_FRACTIONS"] == 3
    assert runtime.QUANTILE_TOP_BITS == d["BGNN_QUANTILE_TOP_BITS"] and runtime.QUANTILE_MAX_GRID == d["BGNN_QUANTILE_MAX_GRID"]
    assert runtime.QUANTILE_WG_ROWS == d["BGNN_QUANTILE_WG_ROWS"] and runtime.QUANTILE_MAX_CAPACITY == 2 ** 32 - 1


def test_quantile_header_is_plain_c(tmp_path, lib):
    if shutil.which("gcc") is None:
        pytest.skip("no gcc")
    src = tmp_path / "quantile_abi.c"
    src.write_text('#include <dlfcn.h>\n#include <stdio.h>\n#include "bgnn_quantile.h"\n'
                   "int main(int argc, char **argv) {\n"
                   "  void *lib = dlopen(argv[1], RTLD_NOW | RTLD_LOCAL);\n"
                   "  if (argc < 2 || !lib) return 1;\n"
                   + "".join(f'  if (!dlsym(lib, "{s}")) {{ fprintf(stderr, "missing {s}\\n"); return 2; }}\n' for s in SYMS)
                   + '  printf("ok %d %d %d\\n", BGNN_QUANTILE_STATE_BYTES, BGNN_QUANTILE_OUT_BYTES, BGNN_QUANTILE_ST_HIST);\n  return 0;\n}\n')
    exe = tmp_path / "quantile_abi"
    subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe),
                    "-ldl"], check=True)
    r = subprocess.run([str(exe), runtime.LIB_PATH], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.split() == ["ok", str(runtime.QUANTILE_STATE_BYTES), str(runtime.QUANTILE_OUT_BYTES), "64"]


def test_hostside_refusals(lib):
    """Every check comes before any use of the context or the device: with a NULL context a call whose other arguments are in order
    is refused for the context, and anything else wrong is named first.  (The pointers here are host buffers: a call that touched
    them, or launched anything, would not come back with these codes.)"""
    buf = (C.c_int64 * 4096)()
    base = C.addressof(buf)
    p = lambda off=0: C.c_void_p(base + off)
    ws = lib.bgnn_quantile_workspace_bytes
    assert ws(0) == 0 and ws(-1) == 0 and ws(1 << 32) == 0
    need = ws(1)
    assert need > 0 and need % 8 == 0 and ws(100) == ws((1 << 32) - 1) == need      # a function of the digits, not of the capacity
    fr = lambda *v: (C.c_double * max(len(v), 1))(*v)

    def refused(word, rc):
        assert rc == runtime.ERR_INVALID
        assert word in lib.bgnn_last_error(), lib.bgnn_last_error()

    # reset(ctx, state)
    refused(b"NULL context", lib.bgnn_quantile_reset(None, p()))
    refused(b"NULL argument", lib.bgnn_quantile_reset(None, None))
    refused(b"not 8-byte aligned", lib.bgnn_quantile_reset(None, p(4)))

    # add(ctx, n, correction, target, mask, stage, capacity, state)
    ok = dict(ctx=None, n=5, correction=p(64), target=p(128), mask=p(192), stage=p(256), capacity=16, state=p(1024))
    add = lambda **kw: lib.bgnn_quantile_add(*{**ok, **kw}.values())
    refused(b"NULL context", add())
    refused(b"NULL context", add(n=0))                          # (also without rows)
    refused(b"NULL context", add(target=None, mask=None))       # both optional
    for name in ("correction", "stage", "state"):
        refused(b"NULL argument", add(**{name: None}))
    refused(b"-1 rows", add(n=-1))
    for cap in (0, -3, 1 << 32, 1 << 40):
        refused(b"capacity", add(capacity=cap))
    refused(b"NULL context", add(capacity=(1 << 32) - 1))
    refused(b"stage is not 4-byte aligned", add(stage=p(258)))
    refused(b"plane is not 4-byte aligned", add(correction=p(66)))
    refused(b"plane is not 4-byte aligned", add(target=p(129)))
    refused(b"state block is not 8-byte aligned", add(state=p(1028)))
    refused(b"NULL context", add(mask=p(193), correction=p(68), target=p(132)))     # an odd mask and 4-byte planes are served

    # select(ctx, stage, capacity, state, fractions, n_fractions, workspace, workspace_bytes, out)
    sk = dict(ctx=None, stage=p(256), capacity=16, state=p(1024), fractions=fr(0.5, 0.95, 1.0), n=3, workspace=p(16384),
              workspace_bytes=need, out=p(512))
    sel = lambda **kw: lib.bgnn_quantile_select(*{**sk, **kw}.values())
    refused(b"NULL context", sel())
    refused(b"NULL context", sel(fractions=fr(0.0), n=1))
    for name in ("stage", "state", "fractions", "workspace", "out"):
        refused(b"NULL argument", sel(**{name: None}))
    for cap in (0, 1 << 32):
        refused(b"capacity", sel(capacity=cap))
    refused(b"0 fractions", sel(n=0))
    refused(b"4 fractions", sel(fractions=fr(0.1, 0.2, 0.3, 0.4), n=4))
    refused(b"-1 fractions", sel(n=-1))
    for bad in (-1e-9, 1.0000001, float("nan"), float("inf")):
        refused(b"outside [0, 1]", sel(fractions=fr(0.5, bad), n=2))
    refused(b"stage is not 4-byte aligned", sel(stage=p(257)))
    refused(b"state block is not 8-byte aligned", sel(state=p(1028)))
    refused(b"workspace is not 8-byte aligned", sel(workspace=p(16388)))
    refused(b"result block is not 8-byte aligned", sel(out=p(516)))
    refused(b"workspace of", sel(workspace_bytes=need - 1))
    refused(b"workspace of", sel(workspace_bytes=0))
    assert not any(buf)
