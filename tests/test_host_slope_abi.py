"""The C ABI of the slope-based feature labels without a GPU (include/bgnn_slope.h): every symbol exported and bound, beside the
other headers' sets at ABI 7; the constants; the workspace formula; the refusals that come before any use of the device."""
import ctypes as C
import os
import re

import pytest

from bathymetric_gnn_amd import runtime

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMS = ["bgnn_slope_features", "bgnn_slope_features_workspace_bytes"]
SIGNATURES = runtime._SLOPE_SIGNATURES


def _header():
    return open(os.path.join(ROOT, "include", "bgnn_slope.h")).read()


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(runtime.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return runtime.load_library()


def test_slope_symbols_exported_and_bound(lib):
    text = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    syms = sorted(set(re.findall(r"\b(bgnn_[a-z_0-9]+)\s*\(", text)))
    assert syms == SYMS and sorted(SIGNATURES) == syms
    for table in (runtime._SIGNATURES, runtime._ANALYSIS_SIGNATURES, runtime._FEATURES_SIGNATURES, runtime._TILESTORE_SIGNATURES,
                  runtime._REVIEW_SIGNATURES):
        assert not set(syms) & set(table)
    for s in syms:
        assert hasattr(lib, s), f"{s} declared in bgnn_slope.h but not exported"
        assert getattr(lib, s).argtypes == SIGNATURES[s][1]
        assert getattr(lib, s).restype == SIGNATURES[s][0]
    assert lib.bgnn_abi_version() == 7 == runtime.ABI_VERSION


def test_constants_match_the_header():
    d = {k: int(v) for k, v in re.findall(r"#define\s+(BGNN_SL_[A-Z_0-9]+)\s+(\d+)\b", _header())}
    assert d["BGNN_SL_MAX_CELLS"] == runtime.SL_MAX_CELLS == runtime.RV_MAX_CELLS == 2 ** 31 - 1
    assert d["BGNN_SL_STATS"] == runtime.SL_STATS == len(runtime.SL_STATS_NAMES) == 6
    assert d["BGNN_SL_STATS_BYTES"] == runtime.SL_STATS_BYTES == 8 * runtime.SL_STATS


def test_workspace_sizes(lib):
    ws = lib.bgnn_slope_features_workspace_bytes
    up = lambda b: (b + 255) // 256 * 256
    assert ws(1, 5) == ws(5, 1) == ws(0, 5) == ws(-1, 5) == ws(5, -1) == 0
    assert ws(1 << 16, 1 << 15) == 0 and ws(1 << 40, 1 << 40) == 0 and ws(46341, 46341) == 0
    assert ws(46340, 46340) > 0 and ws(2, (2 ** 31 - 1) // 2) > 0
    for rows, cols in ((2, 2), (97, 203), (16, 64), (20000, 20000)):
        assert ws(rows, cols) == 2 * up(4 * rows * cols)


def test_hostside_refusals(lib):
    """The argument checks come before any use of the context or the device."""
    buf = (C.c_int64 * 128)()
    p = C.cast(buf, C.c_void_p)
    odd4, odd2 = C.c_void_p(C.addressof(buf) + 4), C.c_void_p(C.addressof(buf) + 2)
    call = lib.bgnn_slope_features

    def args(**kw):
        a = dict(ctx=p, depth=p, base=None, rows=2, cols=2, nodata=1.0e6, cut=0.07, min_size=100, ws=p, ws_bytes=1 << 30, labels=p,
                 mask=None, stats=p)
        a.update(kw)
        return list(a.values())

    for name in ("ctx", "depth", "ws", "labels", "stats"):
        assert call(*args(**{name: None})) == runtime.ERR_INVALID and b"NULL" in lib.bgnn_last_error(), name
    for rows, cols in ((1, 9), (9, 1), (0, 4), (4, -3)):
        assert call(*args(rows=rows, cols=cols)) == runtime.ERR_INVALID and b"gradient" in lib.bgnn_last_error()
    assert call(*args(rows=1 << 16, cols=1 << 15, ws_bytes=1 << 62)) == runtime.ERR_UNSUPPORTED and b"limit" in lib.bgnn_last_error()
    assert call(*args(rows=1 << 40, cols=1 << 40, ws_bytes=1 << 62)) == runtime.ERR_UNSUPPORTED
    assert call(*args(ws_bytes=lib.bgnn_slope_features_workspace_bytes(2, 2) - 1)) == runtime.ERR_INVALID and b"workspace" in lib.bgnn_last_error()
    for name, ptr in (("ws", odd2), ("stats", odd4), ("depth", odd2), ("base", odd2), ("labels", odd2)):
        assert call(*args(**{name: ptr})) == runtime.ERR_INVALID and b"aligned" in lib.bgnn_last_error(), name
