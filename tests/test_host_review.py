"""The review-region export without a GPU: the C ABI part (include/bgnn_review.h: every symbol exported and bound, beside the other
headers' sets at ABI 7; the workspace formula; the refusals that come before any use of the device), the Python layer's refusals,
and the CPU oracle itself -- its two restatements against each other and against the fixture the reference's own
``scripts/export_for_review.py`` wrote (tests/golden/make_golden_review.py)."""
import ctypes as C
import json
import os
import re

import numpy as np
import pytest

from _review_cpu import fast_regions, float32_mean_bound, load_fixture, same_regions, slow_regions, uncertain_mask

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMS = ["bgnn_review_regions", "bgnn_review_workspace_bytes"]
CASES = load_fixture()


def _header():
    return open(os.path.join(ROOT, "include", "bgnn_review.h")).read()


def _declared():
    text = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    return sorted(set(re.findall(r"\b(bgnn_[a-z_0-9]+)\s*\(", text)))


@pytest.fixture(scope="module")
def lib():
    from bathymetric_gnn_amd import runtime
    if not os.path.exists(runtime.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return runtime.load_library()


def test_review_symbols_exported_and_bound(lib):
    from bathymetric_gnn_amd import runtime
    syms = _declared()
    assert syms == SYMS and sorted(runtime._REVIEW_SIGNATURES) == syms
    for table in (runtime._SIGNATURES, runtime._ANALYSIS_SIGNATURES, runtime._FEATURES_SIGNATURES, runtime._TILESTORE_SIGNATURES):
        assert not set(syms) & set(table)
    for s in syms:
        assert hasattr(lib, s), f"{s} declared in bgnn_review.h but not exported"
        assert getattr(lib, s).argtypes == runtime._REVIEW_SIGNATURES[s][1]
        assert getattr(lib, s).restype == runtime._REVIEW_SIGNATURES[s][0]
    assert lib.bgnn_abi_version() == 7 == runtime.ABI_VERSION


def test_constants_match_the_header():
    from bathymetric_gnn_amd import runtime
    d = {k: int(v) for k, v in re.findall(r"#define\s+(BGNN_RV_[A-Z_0-9]+)\s+(\d+)\b", _header())}
    assert d["BGNN_RV_MAX_CELLS"] == runtime.RV_MAX_CELLS == runtime.NA_MAX_CELLS == 2 ** 31 - 1
    assert d["BGNN_RV_COUNTS"] == runtime.RV_COUNTS == len(runtime.RV_COUNT_NAMES)
    assert d["BGNN_RV_RECORD_BYTES"] == runtime.RV_RECORD_BYTES == runtime.RV_RECORD_DTYPE.itemsize and runtime.RV_RECORD_BYTES % 8 == 0
    assert d["BGNN_RV_FIXED_BYTES"] == runtime.RV_FIXED_BYTES
    # the struct's members in the header's order, packed without holes
    body = re.search(r"typedef struct bgnn_review_record \{(.*?)\}", _header(), flags=re.S).group(1)
    members = re.findall(r"\b(?:u?int(?:32|64)_t)\s+([a-z_]+);", re.sub(r"/\*.*?\*/", "", body, flags=re.S))
    assert tuple(members) == runtime.RV_RECORD_DTYPE.names
    spans = sorted((runtime.RV_RECORD_DTYPE.fields[f][1], runtime.RV_RECORD_DTYPE.fields[f][1] + runtime.RV_RECORD_DTYPE.fields[f][0].itemsize)
                   for f in members)
    assert spans[0][0] == 0 and spans[-1][1] == runtime.RV_RECORD_BYTES and all(a[1] == b[0] for a, b in zip(spans, spans[1:]))


def test_workspace_sizes(lib):
    """0 outside the contract; else the header's formula: the fixed part, six int32 planes and one 64-bit plane, each rounded up to
    256 bytes: at most 32 bytes per cell plus a fixed part."""
    from bathymetric_gnn_amd import runtime
    ws = lib.bgnn_review_workspace_bytes
    up = lambda b: (b + 255) // 256 * 256
    assert ws(0, 5) == ws(5, 0) == ws(-1, 5) == ws(5, -1) == 0
    assert ws(1 << 16, 1 << 15) == 0 and ws(1 << 40, 1 << 40) == 0 and ws(46341, 46341) == 0
    assert ws(2 ** 31 - 1, 1) > 0 and ws(1, 2 ** 31 - 1) > 0 and ws(46340, 46340) > 0
    for rows, cols in ((1, 1), (97, 203), (203, 97), (16, 64), (20000, 20000)):
        cells = rows * cols
        assert ws(rows, cols) == runtime.RV_FIXED_BYTES + 6 * up(4 * cells) + up(8 * cells)
        assert ws(rows, cols) <= 32 * cells + runtime.RV_FIXED_BYTES + 7 * 255
    assert ws(20000, 20000) == runtime.RV_FIXED_BYTES + 32 * 20000 * 20000


def test_hostside_refusals(lib):
    """The argument checks come before any use of the context or the device."""
    from bathymetric_gnn_amd import runtime
    buf = (C.c_int64 * 128)()
    p = C.cast(buf, C.c_void_p)
    odd4, odd2 = C.c_void_p(C.addressof(buf) + 4), C.c_void_p(C.addressof(buf) + 2)
    call = lib.bgnn_review_regions
    big = 1 << 30

    def args(**kw):
        a = dict(ctx=p, conf=p, rows=2, cols=2, low=0.4, high=0.7, min_size=1, ws=p, ws_bytes=big, rec=p, cap=4, counts=p, mask=p)
        a.update(kw)
        return list(a.values())

    for name in ("ctx", "conf", "ws", "counts"):
        assert call(*args(**{name: None})) == runtime.ERR_INVALID and b"NULL" in lib.bgnn_last_error(), name
    assert call(*args(rec=None)) == runtime.ERR_INVALID and b"NULL" in lib.bgnn_last_error()
    assert call(*args(rows=0)) == runtime.ERR_INVALID and call(*args(cols=-3)) == runtime.ERR_INVALID
    assert call(*args(min_size=0)) == runtime.ERR_INVALID and b"min_region_size" in lib.bgnn_last_error()
    assert call(*args(cap=-1)) == runtime.ERR_INVALID and b"capacity" in lib.bgnn_last_error()
    for low, high in ((0.7, 0.4), (-0.1, 0.5), (0.5, 1.5), (float("nan"), 0.5), (0.5, float("nan")), (0.0, float("inf")),
                      (float("-inf"), 0.5)):
        assert call(*args(low=low, high=high)) == runtime.ERR_INVALID and b"bounds" in lib.bgnn_last_error(), (low, high)
    assert call(*args(rows=1 << 16, cols=1 << 15, ws_bytes=1 << 62)) == runtime.ERR_UNSUPPORTED and b"limit" in lib.bgnn_last_error()
    assert call(*args(rows=1 << 40, cols=1 << 40, ws_bytes=1 << 62)) == runtime.ERR_UNSUPPORTED
    assert call(*args(ws_bytes=lib.bgnn_review_workspace_bytes(2, 2) - 1)) == runtime.ERR_INVALID and b"workspace" in lib.bgnn_last_error()
    for name, ptr in (("ws", odd4), ("rec", odd4), ("counts", odd4), ("conf", odd2), ("mask", odd2)):
        assert call(*args(**{name: ptr})) == runtime.ERR_INVALID and b"aligned" in lib.bgnn_last_error(), name


def test_python_layer_refuses_without_a_gpu():
    from bathymetric_gnn_amd import runtime
    from bathymetric_gnn_amd.data import export_review_regions
    over = np.broadcast_to(np.float32(0.5), (1 << 16, 1 << 15))            # (a shape only: one float of storage)
    with pytest.raises(NotImplementedError, match=str(runtime.RV_MAX_CELLS)):
        export_review_regions(None, over)
    conf = np.full((4, 4), 0.5, np.float32)
    for low, high in ((0.7, 0.4), (-0.1, 0.5), (0.5, 1.5), (float("nan"), 0.5), (0.2, float("inf"))):
        with pytest.raises(ValueError, match="bounds"):
            export_review_regions(None, conf, low, high)
    with pytest.raises(ValueError, match="min_region_size"):
        export_review_regions(None, conf, min_region_size=0)
    with pytest.raises(ValueError):
        export_review_regions(None, np.zeros((0, 4), np.float32))
    with pytest.raises(ValueError):
        export_review_regions(np.zeros((3, 4), np.float32), conf)
    with pytest.raises(ValueError):
        export_review_regions(None)


@pytest.mark.parametrize("seed", range(4))
def test_fast_and_slow_restatements_agree(seed):
    rng = np.random.default_rng([20240902, seed])
    h, w = rng.integers(5, 60, 2)
    conf = rng.random((h, w)).astype(np.float32)
    conf[rng.random((h, w)) < 0.05] = np.nan
    conf[rng.random((h, w)) < 0.05] = np.float32(0.4)
    conf[rng.random((h, w)) < 0.05] = np.float32(0.7)
    conf[0, 0], conf[h - 1, w - 1] = np.inf, -np.inf
    for min_size in (1, 3, 10):
        fast, fast_mask, counts = fast_regions(conf, 0.4, 0.7, min_size)
        slow, slow_mask = slow_regions(conf, 0.4, 0.7, min_size)
        same_regions(fast, slow)
        assert np.array_equal(fast_mask, slow_mask)
        for f, s in zip(fast, slow):
            assert abs(f["mean_confidence"] - s["mean_confidence"]) <= float32_mean_bound(f["size"], f["mean_confidence"])
        assert counts["uncertain_cells"] == int(uncertain_mask(conf, 0.4, 0.7).sum()) >= counts["kept_cells"] == int(fast_mask.sum())
        assert counts["kept_regions"] == len(fast) <= counts["regions"]


@pytest.mark.parametrize("name", sorted(CASES))
def test_restatement_reproduces_the_reference(name):
    c = CASES[name]
    regions, mask, counts = fast_regions(c["confidence"], c["low"], c["high"], c["min_region_size"])
    same_regions(regions, c["regions"])
    assert np.array_equal(mask, c["review_mask"].astype(bool))
    for got, want in zip(regions, c["regions"]):
        assert abs(got["mean_confidence"] - want["mean_confidence"]) <= float32_mean_bound(got["size"], got["mean_confidence"]), (got, want)
    assert counts["kept_regions"] == len(c["regions"]) and counts["kept_cells"] == int(c["review_mask"].sum())


def test_fixture_covers_its_cases():
    c = CASES["smooth_150x333"]
    conf, unc = c["confidence"], uncertain_mask(c["confidence"], c["low"], c["high"])
    assert np.isnan(conf).any() and (unc & (conf == np.float32(0.4))).any() and (unc & (conf == np.float32(0.7))).any()
    sizes = [r["size"] for r in c["regions"]]
    all_sizes = [r["size"] for r in fast_regions(conf, c["low"], c["high"], 1)[0]]
    assert c["min_region_size"] in sizes and c["min_region_size"] - 1 in all_sizes and len(all_sizes) > len(sizes) >= 5
    assert np.isinf(CASES["strip_301x67"]["confidence"]).sum() == 2 and CASES["none_40x50"]["regions"] == []
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "review", "review_regions.npz")) < 200 * 1024


def test_regions_from_records_and_save_json(tmp_path):
    """The host half: records -> the reference's dictionaries (the mean: one correctly rounded division of the fixed-point sum),
    and ``save_json`` writes what ``json.dump(regions, f, indent=2)`` writes."""
    from bathymetric_gnn_amd import runtime
    from bathymetric_gnn_amd.data.review_regions import ReviewRegions, regions_from_records
    c = CASES["smooth_150x333"]
    want, mask, counts = fast_regions(c["confidence"], c["low"], c["high"], c["min_region_size"])
    records = np.zeros(len(want), runtime.RV_RECORD_DTYPE)
    for rec, r in zip(records, want):
        b = r["bounds"]
        rec["size"], rec["min_row"], rec["max_row"], rec["min_col"], rec["max_col"] = r["size"], b["min_row"], b["max_row"], b["min_col"], b["max_col"]
        rec["conf_sum"] = int(round(r["mean_confidence"] * r["size"] * 2 ** 32))
    got = regions_from_records(records)
    same_regions(got, want)
    for g, r in zip(got, records):
        assert g["mean_confidence"] == int(r["conf_sum"]) / (int(r["size"]) * 2 ** 32)
    result = ReviewRegions(records, counts, None, c["confidence"], c["classification"])
    path = tmp_path / "review.json"
    result.save_json(path)
    with open(tmp_path / "want.json", "w") as f:
        json.dump(got, f, indent=2)
    assert path.read_bytes() == (tmp_path / "want.json").read_bytes() and json.loads(path.read_text()) == got
    bands = result.bands()
    assert bands[0] is None and bands[1] is c["confidence"] and bands[2] is c["classification"]
