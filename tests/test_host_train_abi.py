"""The training part of the C ABI (include/bgnn_train.h: the backward pass) is plain C like bgnn.h: it compiles as C99
(-pedantic), a C program resolves every entry point it declares with dlsym, and the ctypes binding (runtime._TRAIN_SIGNATURES)
covers exactly that set.  No GPU needed."""
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


def test_training_symbols_exported_and_bound(lib):
    from bathymetric_gnn_amd import runtime
    syms = _declared("bgnn_train.h")
    assert syms == ["bgnn_backward", "bgnn_forward_train_tape", "bgnn_tape_bytes"]
    assert not set(syms) & set(runtime._SIGNATURES)
    assert sorted(runtime._TRAIN_SIGNATURES) == syms
    for s in syms:
        assert hasattr(lib, s), f"{s} declared in bgnn_train.h but not exported"
    assert C.sizeof(runtime.OutputGrads) == 4 * C.sizeof(C.c_void_p)


def test_training_header_is_plain_c(tmp_path, lib):
    if shutil.which("gcc") is None:
        pytest.skip("no gcc")
    syms = _declared("bgnn_train.h")
    src = tmp_path / "train_abi.c"
    src.write_text('#include <dlfcn.h>\n#include <stdio.h>\n#include "bgnn_train.h"\n'
                   "int main(int argc, char **argv) {\n"
                   "  bgnn_output_grads g = {0, 0, 0, 0};\n"
                   "  void *lib = dlopen(argv[1], RTLD_NOW | RTLD_LOCAL);\n"
                   "  if (argc < 2 || !lib) return 1;\n"
                   + "".join(f'  if (!dlsym(lib, "{s}")) {{ fprintf(stderr, "missing {s}\\n"); return 2; }}\n' for s in syms)
                   + '  printf("ok %d\\n", (int)sizeof(g));\n  return 0;\n}\n')
    exe = tmp_path / "train_abi"
    subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe),
                    "-ldl"], check=True)
    r = subprocess.run([str(exe), os.path.join(ROOT, "bathymetric-gnn_amd", "libbgnn_hip.so")], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.startswith("ok")
