"""The ground-truth / evaluation part of the C ABI (include/bgnn_eval.h) is plain C like bgnn.h: it compiles as C99 (-pedantic), a C
program resolves every entry point it declares with dlsym, and the ctypes binding (runtime._EVAL_SIGNATURES) covers exactly that
set -- beside, not inside, the pinned symbol sets of bgnn.h and bgnn_train.h, at the same ABI number.  The refusals that need no
device (they are checked before anything is launched) are exercised with a NULL context.  No GPU needed."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMS = ["bgnn_eval_accumulate", "bgnn_eval_reset", "bgnn_eval_workspace_bytes", "bgnn_ground_truth_build",
        "bgnn_ground_truth_workspace_bytes"]


def _declared(name):
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", name)).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(bgnn_[a-z_0-9]+)\s*\(", text)))


def _defines(name):
    text = open(os.path.join(ROOT, "include", name)).read()
    return {k: int(v) for k, v in re.findall(r"#define\s+(BGNN_[A-Z_0-9]+)\s+(\d+)\b", text)}


@pytest.fixture(scope="module")
def lib():
    from bathymetric_gnn_amd import runtime
    if not os.path.exists(runtime.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return runtime.load_library()


def test_eval_symbols_exported_and_bound(lib):
    from bathymetric_gnn_amd import runtime
    syms = _declared("bgnn_eval.h")
    assert syms == SYMS
    assert sorted(runtime._EVAL_SIGNATURES) == syms
    others = [runtime._SIGNATURES, runtime._TRAIN_SIGNATURES, runtime._SIDECAR_SIGNATURES, runtime._NOISE_SIGNATURES,
              runtime._LOSS_SIGNATURES, runtime._OPTIM_SIGNATURES, runtime._TRAINER_SIGNATURES]
    for table in others:
        assert not set(syms) & set(table)
    for h in ("bgnn.h", "bgnn_train.h", "bgnn_sidecar.h", "bgnn_noise.h", "bgnn_loss.h", "bgnn_optim.h", "bgnn_trainer.h"):
        assert not set(syms) & set(_declared(h)), h
    for s in syms:
        assert hasattr(lib, s), f"{s} declared in bgnn_eval.h but not exported"
        assert getattr(lib, s).argtypes == runtime._EVAL_SIGNATURES[s][1]
        assert getattr(lib, s).restype == runtime._EVAL_SIGNATURES[s][0]
    assert lib.bgnn_abi_version() == 7 == runtime.ABI_VERSION


def test_block_layouts_match_the_header():
    """The numpy record types the host derivations read are the byte offsets the header documents."""
    from bathymetric_gnn_amd import runtime
    d = _defines("bgnn_eval.h")
    st = np.dtype(runtime.GT_STATS_DTYPE)
    assert st.itemsize == d["BGNN_GT_STATS_BYTES"] == runtime.GT_STATS_BYTES
    for field, macro in (("valid", "VALID"), ("noise", "NOISE"), ("seafloor", "SEAFLOOR"), ("noise_abs_sum", "NOISE_ABS_SUM"),
                         ("seafloor_sum", "SEAFLOOR_SUM"), ("offset", "OFFSET"), ("noise_abs_max", "NOISE_ABS_MAX")):
        assert st.fields[field][1] == d["BGNN_GT_STATS_" + macro], field
    acc = np.dtype(runtime.EVAL_ACC_DTYPE)
    assert acc.itemsize == d["BGNN_EVAL_ACC_BYTES"] == runtime.EVAL_ACC_BYTES
    for field in ("total", "correct", "confusion", "covered", "covered_correct", "conf_sum", "conf_sq", "conf_correct_sum",
                  "conf_incorrect_sum", "conf_cells"):
        assert acc.fields[field][1] == d["BGNN_EVAL_ACC_" + field.upper()], field
    assert len(runtime.EVAL_THRESHOLDS) == d["BGNN_EVAL_THRESHOLDS"] == acc.fields["covered"][0].shape[0]


def test_eval_header_is_plain_c(tmp_path, lib):
    if shutil.which("gcc") is None:
        pytest.skip("no gcc")
    from bathymetric_gnn_amd import runtime
    syms = _declared("bgnn_eval.h")
    src = tmp_path / "eval_abi.c"
    src.write_text('#include <dlfcn.h>\n#include <stdio.h>\n#include "bgnn_eval.h"\n'
                   "int main(int argc, char **argv) {\n"
                   "  void *lib = dlopen(argv[1], RTLD_NOW | RTLD_LOCAL);\n"
                   "  if (argc < 2 || !lib) return 1;\n"
                   + "".join(f'  if (!dlsym(lib, "{s}")) {{ fprintf(stderr, "missing {s}\\n"); return 2; }}\n' for s in syms)
                   + '  printf("ok %d %d %d\\n", BGNN_GT_STATS_BYTES, BGNN_EVAL_ACC_BYTES, BGNN_EVAL_THRESHOLDS);\n'
                     "  return 0;\n}\n")
    exe = tmp_path / "eval_abi"
    subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe),
                    "-ldl"], check=True)
    r = subprocess.run([str(exe), os.path.join(ROOT, "bathymetric-gnn_amd", "libbgnn_hip.so")], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.split() == ["ok", str(runtime.GT_STATS_BYTES), str(runtime.EVAL_ACC_BYTES), str(len(runtime.EVAL_THRESHOLDS))]


def test_workspace_sizes_and_hostside_refusals(lib):
    """The workspace is a function of ``cells`` alone, grows with the grid up to its cap, and is 0 for a negative count; a NULL
    context is refused before anything else is looked at."""
    from bathymetric_gnn_amd import runtime
    gt, ev = lib.bgnn_ground_truth_workspace_bytes, lib.bgnn_eval_workspace_bytes
    assert gt(-1) == 0 and ev(-1) == 0
    assert 0 < gt(0) == gt(1) == gt(1024) <= gt(1025) < gt(100 * 1024) < gt(1 << 40) == gt(20000 * 20000)     # (rounded up to 256 bytes)
    assert 0 < ev(0) == ev(1) == ev(1024) < ev(1025) < ev(100 * 1024) < ev(1 << 40) == ev(20000 * 20000)
    assert gt(20000 * 20000) < (1 << 20) and ev(20000 * 20000) <= (1 << 20)
    buf = (C.c_int64 * 64)()
    p = C.cast(buf, C.c_void_p)
    rc = lib.bgnn_ground_truth_build(None, p, p, None, 4, 1.0e6, 0.15, p, 512, p, p, None, p)
    assert rc == runtime.ERR_INVALID and b"NULL" in lib.bgnn_last_error()
    assert lib.bgnn_eval_accumulate(None, p, p, None, 4, p, 512, p) == runtime.ERR_INVALID and b"NULL" in lib.bgnn_last_error()
    assert lib.bgnn_eval_reset(None, p) == runtime.ERR_INVALID and b"NULL" in lib.bgnn_last_error()
