"""The variable-resolution gridding part of the C ABI (include/bgnn_soundings_vr.h) is plain C like bgnn.h: it compiles as C99
(-pedantic), a C program resolves every entry point it declares with dlsym, and the ctypes binding
(runtime._VR_SOUNDINGS_SIGNATURES) covers exactly that set -- beside, not inside, every other pinned symbol set, at the same ABI
number.  The refusals, all of which come before anything is launched, are exercised with a NULL context: each returns its code
and a message.  No GPU needed."""
import ctypes as C
import glob
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMS = ["bgnn_vr_soundings_add", "bgnn_vr_soundings_density", "bgnn_vr_soundings_flag", "bgnn_vr_soundings_plan",
        "bgnn_vr_soundings_plan_workspace_bytes", "bgnn_vr_soundings_stage"]


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


def test_vr_symbols_exported_and_bound(lib):
    from bathymetric_gnn_amd import runtime
    syms = _declared(os.path.join(ROOT, "include", "bgnn_soundings_vr.h"))
    assert syms == SYMS
    assert sorted(runtime._VR_SOUNDINGS_SIGNATURES) == syms
    tables = {k: v for k, v in vars(runtime).items() if k.endswith("_SIGNATURES") and isinstance(v, dict)}
    assert "_VR_SOUNDINGS_SIGNATURES" in tables and "_ROBUST_SIGNATURES" in tables and len(tables) >= 19
    for name, table in tables.items():
        if name != "_VR_SOUNDINGS_SIGNATURES":
            assert not set(syms) & set(table), name
    headers = sorted(glob.glob(os.path.join(ROOT, "include", "*.h")))
    assert len(headers) >= 19
    for h in headers:
        if os.path.basename(h) != "bgnn_soundings_vr.h":
            assert not set(syms) & set(_declared(h)), h
    for s in syms:
        assert hasattr(lib, s), f"{s} declared in bgnn_soundings_vr.h but not exported"
        assert getattr(lib, s).argtypes == runtime._VR_SOUNDINGS_SIGNATURES[s][1]
        assert getattr(lib, s).restype == runtime._VR_SOUNDINGS_SIGNATURES[s][0]
    assert lib.bgnn_abi_version() == 7 == runtime.ABI_VERSION


def test_vr_header_is_plain_c(tmp_path, lib):
    if shutil.which("gcc") is None:
        pytest.skip("no gcc")
    from bathymetric_gnn_amd import runtime
    src = tmp_path / "vr_abi.c"
    src.write_text('#include <dlfcn.h>\n#include <stdio.h>\n#include "bgnn_soundings_vr.h"\n'
                   "int main(int argc, char **argv) {\n"
                   "  void *lib = dlopen(argv[1], RTLD_NOW | RTLD_LOCAL);\n"
                   "  if (argc < 2 || !lib) return 1;\n"
                   + "".join(f'  if (!dlsym(lib, "{s}")) {{ fprintf(stderr, "missing {s}\\n"); return 2; }}\n' for s in SYMS)
                   + '  printf("ok %d %d %d %d %d %d %d\\n", BGNN_VR_ENTRY_BYTES, BGNN_VR_MAX_DIM, BGNN_VR_MAX_RUNGS,\n'
                     "         BGNN_VR_MAX_BASE_CELLS, BGNN_VR_MAX_RECORDS, BGNN_VR_MAX_TARGET, BGNN_VR_PLAN_TILE);\n"
                     "  return 0;\n}\n")
    exe = tmp_path / "vr_abi"
    subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe),
                    "-ldl"], check=True)
    r = subprocess.run([str(exe), os.path.join(ROOT, "bathymetric-gnn_amd", "libbgnn_hip.so")], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.split() == ["ok"] + [str(v) for v in (
        runtime.VR_ENTRY_BYTES, runtime.VR_MAX_DIM, runtime.VR_MAX_RUNGS, runtime.VR_MAX_BASE_CELLS, runtime.VR_MAX_RECORDS,
        runtime.VR_MAX_TARGET, runtime.VR_PLAN_TILE)]
    assert runtime.VR_ENTRY_DTYPE.itemsize == runtime.VR_ENTRY_BYTES == 16
    assert runtime.VR_SOUNDINGS_COUNTERS == runtime.SOUNDINGS_COUNTERS + ("unrefined",)


def test_plan_workspace_size(lib):
    work = lib.bgnn_vr_soundings_plan_workspace_bytes
    assert work(0, 4) == 0 and work(4, 0) == 0 and work(-1, 4) == 0 and work(2 ** 31, 1) == 0 and work(2 ** 16, 2 ** 15) == 0
    assert work(1, 1) == 256 and work(1, 257) == 256 and work(300, 300) == 2816 and work(1, 32 * 256 + 1) == 512
    assert work(2 ** 31 - 1, 1) == 8 * 2 ** 23


def test_refusals_before_any_launch(lib):
    """With a NULL context every call is refused, and the message names what is wrong with the other arguments first."""
    from bathymetric_gnn_amd import runtime
    buf = (C.c_int64 * 64)()
    p = C.cast(buf, C.c_void_p)
    odd = C.c_void_p(p.value + 4)

    def refused(word, rc, code=runtime.ERR_INVALID):
        assert rc == code, (rc, lib.bgnn_last_error())
        assert word in lib.bgnn_last_error(), lib.bgnn_last_error()

    def caller(fn, names, ok):
        return lambda **kw: fn(*[kw.get(name, v) for name, v in zip(names, ok)])

    cloud_names = ["ctx", "x", "y", "z", "n", "x0", "y0", "res", "bh", "bw"]
    cloud_ok = [None, p, p, p, 4, 0.0, 0.0, 8.0, 2, 2]

    def cloud_refusals(call, flags=False):
        refused(b"NULL context", call())
        none = dict(x=None, y=None, z=None, n=0, **({"flags": None} if flags else {}))
        refused(b"NULL context", call(**none))
        for name in ("x", "y", "z"):
            refused(b"NULL argument", call(**{name: None}))
        refused(b"-5 soundings", call(n=-5))
        refused(b"base resolution of 0", call(res=0.0))
        refused(b"base resolution of nan", call(res=float("nan")))
        refused(b"base resolution of -1", call(res=-1.0))
        refused(b"origin", call(x0=float("inf")))
        refused(b"origin", call(y0=float("nan")))
        refused(b"0 x 2 cells", call(bh=0))
        refused(b"2 x 2147483648 cells", call(bw=2 ** 31))
        refused(b"more than 2147483647 in all", call(bh=2 ** 16, bw=2 ** 15), runtime.ERR_UNSUPPORTED)
        refused(b"NULL context", call(bh=2 ** 31 - 1, bw=1))

    def table_refusals(call):
        refused(b"NULL argument", call(table=None))
        refused(b"layout of 0 records", call(total=0))
        refused(b"layout of 2147483648 records", call(total=2 ** 31))
        refused(b"NULL context", call(total=2 ** 31 - 1))
        refused(b"the table is not 8-byte aligned", call(table=odd))

    dens = caller(lib.bgnn_vr_soundings_density, cloud_names + ["counts"], cloud_ok + [p])
    cloud_refusals(dens)
    refused(b"NULL argument", dens(counts=None))
    refused(b"not 4-byte aligned", dens(counts=C.c_void_p(p.value + 2)))

    ladder = np.array([1, 2, 4, 8], np.int32)
    plan_names = ["ctx", "counts", "bh", "bw", "ladder", "n_rungs", "target", "min_base", "ws", "ws_bytes", "table", "total"]
    need = lib.bgnn_vr_soundings_plan_workspace_bytes(2, 2)
    plan = caller(lib.bgnn_vr_soundings_plan, plan_names, [None, p, 2, 2, ladder.ctypes.data, 4, 3, 1, p, need, p, p])
    refused(b"NULL context", plan())
    for name in ("counts", "ladder", "ws", "table", "total"):
        refused(b"NULL argument", plan(**{name: None}))
    refused(b"0 x 2 cells", plan(bh=0))
    refused(b"more than 2147483647 in all", plan(bh=2 ** 16, bw=2 ** 15), runtime.ERR_UNSUPPORTED)
    refused(b"ladder of 0 rungs", plan(n_rungs=0))
    refused(b"ladder of 17 rungs", plan(n_rungs=17))
    for bad, word in (([1, 2, 2, 8], b"not strictly ascending at rung 2"), ([4, 2, 8, 16], b"not strictly ascending at rung 1"),
                      ([0, 2, 4, 8], b"rung 0 of the ladder is 0"), ([1, 2, 4, 32769], b"rung 3 of the ladder is 32769"),
                      ([-3, 2, 4, 8], b"rung 0 of the ladder is -3")):
        arr = np.array(bad, np.int32)
        refused(word, plan(ladder=arr.ctypes.data))
    top = np.array([1, 32768], np.int32)
    refused(b"NULL context", plan(ladder=top.ctypes.data, n_rungs=2))
    refused(b"target_count of 0", plan(target=0))
    refused(b"target_count of 2147483648", plan(target=2 ** 31))
    refused(b"min_base_count of 0", plan(min_base=0))
    refused(b"workspace of", plan(ws_bytes=need - 1))
    refused(b"the workspace is not 8-byte aligned", plan(ws=odd))
    refused(b"the table is not 8-byte aligned", plan(table=odd))
    refused(b"total is not 8-byte aligned", plan(total=odd))

    add = caller(lib.bgnn_vr_soundings_add, cloud_names + ["table", "total", "offered", "state", "unrefined"], cloud_ok + [p, 16, 0, p, p])
    cloud_refusals(add)
    table_refusals(add)
    refused(b"NULL argument", add(state=None))
    refused(b"NULL argument", add(unrefined=None))
    refused(b"-1 soundings offered before", add(offered=-1))
    refused(b"a total above 2147483647", add(n=4, offered=2 ** 31 - 4))
    refused(b"a total above 2147483647", add(n=2 ** 62, offered=2 ** 62))
    refused(b"NULL context", add(n=4, offered=2 ** 31 - 5))
    refused(b"the state is not 8-byte aligned", add(state=odd))
    refused(b"the unrefined counter is not 8-byte aligned", add(unrefined=odd))

    stage = caller(lib.bgnn_vr_soundings_stage, cloud_names + ["table", "total", "offered", "capacity", "stage", "unrefined"],
                   cloud_ok + [p, 16, 0, 8, p, p])
    cloud_refusals(stage)
    table_refusals(stage)
    refused(b"NULL argument", stage(stage=None))
    refused(b"NULL argument", stage(unrefined=None))
    refused(b"capacity of 0", stage(capacity=0))
    refused(b"capacity of 2147483648", stage(capacity=2 ** 31))
    refused(b"-1 soundings offered before", stage(offered=-1))
    refused(b"more than the capacity of 8", stage(n=4, offered=5))
    refused(b"more than the capacity of 8", stage(n=9))
    refused(b"NULL context", stage(n=4, offered=4))
    refused(b"the stage is not 8-byte aligned", stage(stage=odd))
    refused(b"the unrefined counter is not 8-byte aligned", stage(unrefined=odd))

    flag = caller(lib.bgnn_vr_soundings_flag, cloud_names + ["table", "total", "center2", "limit", "flags"], cloud_ok + [p, 16, p, p, p])
    cloud_refusals(flag, flags=True)
    table_refusals(flag)
    for name in ("center2", "limit", "flags"):
        refused(b"NULL argument", flag(**{name: None}))
    refused(b"center2 or limit", flag(center2=odd))
    refused(b"center2 or limit", flag(limit=odd))
    assert not any(buf)
