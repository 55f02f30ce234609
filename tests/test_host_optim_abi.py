"""The optimizer part of the C ABI (include/bgnn_optim.h: fused clip + AdamW on the blob, in-place model refresh) is plain C like
bgnn.h: it compiles as C99 (-pedantic), a C program resolves every entry point it declares with dlsym, and the ctypes binding
(runtime._OPTIM_SIGNATURES) covers exactly that set -- beside, not inside, the pinned symbol sets of bgnn.h and bgnn_train.h, at
the same ABI number.  No GPU needed."""
import ctypes as C
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _declared(name):
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", name)).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(bgnn_[a-z_0-9]+)\s*\(", text)))


@pytest.fixture(scope="module")
def lib():
    from bathymetric_gnn_amd import runtime
    if not os.path.exists(runtime.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return runtime.load_library()


def test_optimizer_symbols_exported_and_bound(lib):
    from bathymetric_gnn_amd import runtime
    syms = _declared("bgnn_optim.h")
    assert syms == ["bgnn_adamw_step", "bgnn_model_refresh", "bgnn_model_refresh_prepare"]
    assert sorted(runtime._OPTIM_SIGNATURES) == syms
    assert not set(syms) & set(runtime._SIGNATURES)
    assert not set(syms) & set(runtime._TRAIN_SIGNATURES)
    assert not set(syms) & (set(_declared("bgnn.h")) | set(_declared("bgnn_train.h")))
    for s in syms:
        assert hasattr(lib, s), f"{s} declared in bgnn_optim.h but not exported"
        assert getattr(lib, s).argtypes == runtime._OPTIM_SIGNATURES[s][1]
    assert lib.bgnn_abi_version() == 7 == runtime.ABI_VERSION
    assert C.sizeof(runtime.AdamWSlot) == 24 and C.sizeof(runtime.AdamWParams) == 48


def test_optimizer_header_is_plain_c(tmp_path, lib):
    if shutil.which("gcc") is None:
        pytest.skip("no gcc")
    from bathymetric_gnn_amd import runtime
    syms = _declared("bgnn_optim.h")
    src = tmp_path / "optim_abi.c"
    src.write_text('#include <dlfcn.h>\n#include <stdio.h>\n#include "bgnn_optim.h"\n'
                   "int main(int argc, char **argv) {\n"
                   "  bgnn_adamw_slot s = {0, 0, 1};\n"
                   "  bgnn_adamw_params p = {1e-3, 0.9, 0.999, 1e-8, 1e-2, 0.0};\n"
                   "  void *lib = dlopen(argv[1], RTLD_NOW | RTLD_LOCAL);\n"
                   "  if (argc < 2 || !lib) return 1;\n"
                   + "".join(f'  if (!dlsym(lib, "{s}")) {{ fprintf(stderr, "missing {s}\\n"); return 2; }}\n' for s in syms)
                   + '  printf("ok %d %d %d %d %d\\n", (int)sizeof(s), (int)sizeof(p), BGNN_ADAMW_CHUNK, BGNN_REFRESH_ALL, BGNN_REFRESH_STATS);\n'
                     "  return (int)s.step - 1 + (p.max_norm > 0.0);\n}\n")
    exe = tmp_path / "optim_abi"
    subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe),
                    "-ldl"], check=True)
    r = subprocess.run([str(exe), os.path.join(ROOT, "bathymetric-gnn_amd", "libbgnn_hip.so")], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    # the struct sizes and constants the ctypes mirror assumes
    assert r.stdout.split() == ["ok", str(C.sizeof(runtime.AdamWSlot)), str(C.sizeof(runtime.AdamWParams)), str(runtime.ADAMW_CHUNK),
                                str(runtime.REFRESH_ALL), str(runtime.REFRESH_STATS)]
