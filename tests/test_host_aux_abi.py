"""The C ABI of the auxiliary node-feature planes without a GPU (include/bgnn_aux.h): both symbols exported and bound, beside the other
headers' sets at ABI 7; the constants; the refusals, all of which come before any use of the context or the device; the weight blob
of a model with more than 8 input channels."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from bathymetric_gnn_amd import runtime

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMS = ["bgnn_graph_build_aux", "bgnn_infer_tiles_aux"]
ARGS = {"bgnn_graph_build_aux": 6, "bgnn_infer_tiles_aux": 13}
SIGNATURES = runtime._AUX_SIGNATURES
DEFAULT7 = ["depth", "local_mean", "local_std", "gradient_x", "gradient_y", "gradient_magnitude", "curvature"]
EDGES = ["distance", "depth_difference", "slope"]


def _header(name="bgnn_aux.h"):
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


def test_aux_symbols_exported_and_bound(lib):
    decl = _declared("bgnn_aux.h")
    assert sorted(decl) == SYMS and sorted(SIGNATURES) == SYMS
    tables = [getattr(runtime, n) for n in dir(runtime) if n.endswith("_SIGNATURES") and n != "_AUX_SIGNATURES"]
    assert len(tables) >= 19 and runtime._SIGNATURES in tables
    for table in tables:
        assert not set(SYMS) & set(table)
    for h in sorted(os.listdir(os.path.join(ROOT, "include"))):
        if h.endswith(".h") and h != "bgnn_aux.h":
            assert not set(SYMS) & set(_declared(h)), h
    for s in SYMS:
        assert hasattr(lib, s), f"{s} declared in bgnn_aux.h but not exported"
        assert len(decl[s].split(",")) == ARGS[s] == len(SIGNATURES[s][1]), s
        assert getattr(lib, s).argtypes == SIGNATURES[s][1]
        assert getattr(lib, s).restype == SIGNATURES[s][0]
    assert lib.bgnn_abi_version() == 7 == runtime.ABI_VERSION


def test_constants_match_the_header():
    d = {k: int(v) for k, v in re.findall(r"#define\s+(BGNN_AUX_[A-Z_0-9]+)\s+(\d+)\b", _header())}
    assert d == {"BGNN_AUX_MAX_PLANES": 8, "BGNN_AUX_ROW_FLOATS": 16}
    assert runtime.AUX_MAX_PLANES == 8 and runtime.AUX_ROW_FLOATS == 16
    assert runtime.NODE_PLANES == ("uncertainty", "sounding_density")


def test_aux_header_is_plain_c(tmp_path, lib):
    if shutil.which("gcc") is None:
        pytest.skip("no gcc")
    src = tmp_path / "aux_abi.c"
    src.write_text('#include <dlfcn.h>\n#include <stdio.h>\n#include "bgnn_aux.h"\n'
                   "int main(int argc, char **argv) {\n"
                   "  void *lib = dlopen(argv[1], RTLD_NOW | RTLD_LOCAL);\n"
                   "  if (argc < 2 || !lib) return 1;\n"
                   + "".join(f'  if (!dlsym(lib, "{s}")) {{ fprintf(stderr, "missing {s}\\n"); return 2; }}\n' for s in SYMS)
                   + '  printf("ok %d %d\\n", BGNN_AUX_MAX_PLANES, BGNN_AUX_ROW_FLOATS);\n  return 0;\n}\n')
    exe = tmp_path / "aux_abi"
    subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe),
                    "-ldl"], check=True)
    r = subprocess.run([str(exe), runtime.LIB_PATH], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.split() == ["ok", "8", "16"]


def test_hostside_refusals(lib):
    """Every check of the planes comes before any use of the context, the model or the device.  (Context and model here are host
    buffers: a call that touched them, or launched anything, would not come back with these codes.)"""
    buf = (C.c_int64 * 1024)()
    base = C.addressof(buf)
    fake = lambda off: C.c_void_p(base + off)
    hw = np.array([[4, 5]], np.int32)
    res = np.array([[1.0, 1.0]], np.float64)

    def tiles(unc: bool):
        t = runtime.Tiles()
        t.n_tiles = 1
        t.hw = hw.ctypes.data_as(C.POINTER(C.c_int32))
        t.resolution = res.ctypes.data_as(C.POINTER(C.c_double))
        t.depth, t.mask = base + 2048, base + 4096
        t.uncertainty = base + 6144 if unc else None
        return t
    opts7 = runtime.make_graph_opts("8-connected", False, DEFAULT7, EDGES)
    opts8 = runtime.make_graph_opts("8-connected", False, DEFAULT7 + ["depth"], EDGES)      # 8 listed, none of them uncertainty
    planes = lambda n, hole=None: (C.c_void_p * max(n, 1))(*[None if i == hole else base + 1024 + 64 * i for i in range(max(n, 1))])
    out = C.c_void_p()
    INVALID, UNSUPPORTED = runtime.ERR_INVALID, runtime.ERR_UNSUPPORTED
    err = lambda: lib.bgnn_last_error()

    def build(**kw):
        a = {**dict(ctx=fake(0), tiles=C.byref(tiles(False)), opts=C.byref(opts7), n_aux=1, aux=planes(1), out=C.byref(out)), **kw}
        return lib.bgnn_graph_build_aux(*a.values())

    def infer(**kw):
        a = {**dict(ctx=fake(0), model=fake(512), tiles=C.byref(tiles(False)), opts=C.byref(opts7), n_aux=1, aux=planes(1),
                    thr_auto=0.85, thr_review=0.6, floor=0.01, cls=fake(7168), conf=fake(7424), corr=fake(7680), n_nodes=None), **kw}
        return lib.bgnn_infer_tiles_aux(*a.values())

    for name in ("ctx", "tiles", "opts", "out"):
        assert build(**{name: None}) == INVALID and b"NULL" in err(), name
    for name in ("ctx", "model", "tiles", "opts"):
        assert infer(**{name: None}) == INVALID and b"NULL" in err(), name
    for call in (build, infer):
        for n in (-1, 9, 1 << 20):
            assert call(n_aux=n, aux=planes(8)) == INVALID and b"out of range" in err(), n
        assert call(aux=None) == INVALID and b"aux is NULL" in err()
        assert call(n_aux=3, aux=planes(3, hole=0)) == INVALID and b"plane 0 is NULL" in err()
        assert call(n_aux=3, aux=planes(3, hole=2)) == INVALID and b"plane 2 is NULL" in err()
        # 8 listed features and uncertainty appended are 9 columns: with 8 planes 17, one more than the wide table holds
        assert call(tiles=C.byref(tiles(True)), opts=C.byref(opts8), n_aux=8, aux=planes(8)) == UNSUPPORTED and b"exceed" in err()
        # the same 8 planes behind 7 + uncertainty = 8 columns fill the table exactly: not refused HERE (the next check is the
        # context's, which these host buffers cannot pass -- so only the code above is asked for)
    assert out.value is None


def _count(lib, in_channels, gnn_type="GAT"):
    import torch  # noqa: F401
    from bathymetric_gnn_amd.models import BathymetricGNN
    m = BathymetricGNN(in_channels=in_channels, edge_dim=3, gnn_type=gnn_type, num_gnn_layers=3)
    d = m._desc()
    params = sum(p.numel() for p in m.parameters())
    stats = sum(b.numel() for n, b in m.named_buffers() if n.endswith(("running_mean", "running_var")))
    return lib.bgnn_model_weight_count(C.byref(d)), params + stats, m.pack_weights().size


@pytest.mark.parametrize("gnn_type", ["GAT", "GraphSAGE"])
@pytest.mark.parametrize("in_channels", [9, 16])
def test_weight_count_above_8_channels(lib, in_channels, gnn_type):
    got, want, packed = _count(lib, in_channels, gnn_type)
    assert got == want == packed
    assert got - _count(lib, 8, gnn_type)[0] == 64 * (in_channels - 8)          # one weight column of the first Linear per channel


def test_in_channels_17_is_refused(lib):
    """bgnn_model_create checks the shape before it touches the context (a host buffer here) or the weights."""
    buf = (C.c_int64 * 64)()
    w = (C.c_float * 4)()
    out = C.c_void_p()
    d = runtime.ModelDesc(in_channels=17, hidden=64, num_layers=3, heads=4, num_classes=3, edge_dim=3, predict_correction=1,
                          bn_eps=1e-5, gnn_type=0)
    assert lib.bgnn_model_create(C.c_void_p(C.addressof(buf)), C.byref(d), w, 4, C.byref(out)) == runtime.ERR_INVALID
    assert b"in_channels=17 unsupported (1..16)" in lib.bgnn_last_error()
    for ok in (9, 16):                                     # accepted as a shape: the next check, the blob's size, answers
        d.in_channels = ok
        assert lib.bgnn_model_create(C.c_void_p(C.addressof(buf)), C.byref(d), w, 4, C.byref(out)) == runtime.ERR_INVALID
        assert b"weight blob has 4 floats" in lib.bgnn_last_error()
    d.in_channels = 0
    assert lib.bgnn_model_create(C.c_void_p(C.addressof(buf)), C.byref(d), w, 4, C.byref(out)) == runtime.ERR_INVALID
    assert b"in_channels=0" in lib.bgnn_last_error()
