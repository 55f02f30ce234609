"""Operating curves, the host side (training/operating_curve.py): the two numpy restatements of _curve_cpu.py agree through
``curve_from_block`` (which guards the restatement the GPU tests compare against), the block's record is the header's layout,
``recommend_thresholds`` reads hand-made curves, and the threshold table is validated before anything is uploaded.  No GPU needed."""
import os
import re

import numpy as np
import pytest

import _curve_cpu as cc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header_macros():
    """The header's ``#define``s as Python: plain numbers, and functions of T for the layout."""
    text = open(os.path.join(ROOT, "include", "bgnn_curve.h")).read()
    env = {k: int(v) for k, v in re.findall(r"#define\s+(BGNN_CURVE_[A-Z_0-9]+)\s+(\d+)\b", text)}
    for name, expr in re.findall(r"#define\s+(BGNN_CURVE_[A-Z_0-9]+)\(T\)\s+(.+?)\s*(?:/\*.*)?$", text, flags=re.M):
        assert re.fullmatch(r"[A-Z_0-9()T+* ]+", expr), expr
        env[name] = eval("lambda T: " + expr, env)              # (later macros use earlier ones: the header's own order)
    return env


@pytest.mark.parametrize("n_thresholds", [1, 2, 101, 128])
@pytest.mark.parametrize("kind", ["random", "adversarial", "one_value"])
def test_brute_force_equals_the_histogram_form(kind, n_thresholds):
    from bathymetric_gnn_amd.training import curve_from_block
    thr = cc.thresholds_for(n_thresholds)
    n = 6007
    planes = {"random": lambda: cc.random_planes(n, 3), "adversarial": lambda: cc.adversarial_planes(thr, n, 4),
              "one_value": lambda: cc.one_value_planes(n, float(thr[0]))}[kind]()
    blk = cc.numpy_block(thr, *planes)
    assert blk.dtype == cc.block_dtype(n_thresholds)
    got = curve_from_block(blk, thr)
    want = cc.brute_curve(thr, *planes)
    assert "residual" in got and got["total"] > 0
    cc.assert_curves_equal(got, want)
    if kind == "adversarial":
        assert got["nan_confidence_cells"] > 0 and got["residual"]["skipped"] > 0
        assert 0 < got["residual"]["corrected_cells"][0] < got["auto_correct"]["cells"][0]
    # without the residual planes: the same counts, no residual part
    bare = curve_from_block(cc.numpy_block(thr, *planes[:3]), thr)
    assert "residual" not in bare
    cc.assert_curves_equal(bare, cc.brute_curve(thr, *planes[:3]))
    # two halves accumulate to the whole
    h = n // 2 + 1
    halves = cc.add_blocks(cc.numpy_block(thr, *(p[:h] for p in planes)), cc.numpy_block(thr, *(p[h:] for p in planes)))
    assert halves.tobytes() == blk.tobytes()


def test_codes_decide_the_three_comparisons():
    """c > t_k <=> code >= 2k + 2, c >= t_k <=> code >= 2k + 1, c < t_k <=> code <= 2k, NaN none of them: on every special value."""
    thr = cc.thresholds_for(101)
    _, _, conf, _, _ = cc.adversarial_planes(thr, 4001, 9)
    code = cc.confidence_codes(thr, conf)
    T = thr.size
    assert code.min() == 0 and code.max() == 2 * T + 1 and (code[np.isnan(conf)] == 2 * T + 1).all()
    ranked = code <= 2 * T
    with np.errstate(invalid="ignore"):
        for k, t in enumerate(thr):
            assert np.array_equal(conf > t, ranked & (code >= 2 * k + 2))
            assert np.array_equal(conf >= t, ranked & (code >= 2 * k + 1))
            assert np.array_equal(conf < t, code <= 2 * k)


def test_block_record_is_the_header_layout():
    from bathymetric_gnn_amd import runtime as rt
    m = _header_macros()
    assert m["BGNN_CURVE_MAX_THRESHOLDS"] == rt.CURVE_MAX_THRESHOLDS == 128
    assert m["BGNN_CURVE_WG_CELLS"] == rt.CURVE_WG_CELLS and m["BGNN_CURVE_MAX_GRID"] == rt.CURVE_MAX_GRID
    assert m["BGNN_CURVE_RES_CAP"] == rt.CURVE_RES_CAP == 32768 and m["BGNN_CURVE_RES_SCALE"] == rt.CURVE_RES_SCALE == 65536
    for T in (1, 2, 101, 128):
        dt = np.dtype(rt.curve_block_dtype(T))
        assert dt == cc.block_dtype(T)
        assert dt.itemsize == m["BGNN_CURVE_BLOCK_BYTES"](T)
        assert dt.fields["counts"][0].shape == (m["BGNN_CURVE_CODES"](T), 4, 4)
        for field in ("counts", "res_cells", "abs_before", "abs_after", "base_cells", "base_abs", "res_skipped"):
            assert dt.fields[field][1] == m["BGNN_CURVE_" + field.upper()](T), (field, T)
            assert dt.fields[field][0].base == np.dtype("<i8")


def _curve(thr, cells, precision, recall=None, review_share=None):
    n = len(thr)
    return {"thresholds": list(thr), "auto_correct": {"cells": list(cells), "precision": list(precision),
                                                      "recall": list(recall or [0.5] * n)},
            "review": {"share": list(review_share or [0.0] * n)}}


def test_recommend_thresholds_on_hand_made_curves():
    from bathymetric_gnn_amd.training import recommend_thresholds
    thr = [0.5, 0.6, 0.7, 0.8]
    # the smallest that qualifies, with its own precision and recall
    r = recommend_thresholds(_curve(thr, [90, 50, 20, 5], [0.7, 0.91, 0.95, 1.0], [0.9, 0.8, 0.4, 0.1]))
    assert r == {"auto_correct_threshold": 0.6, "precision": 0.91, "recall": 0.8}
    # none qualifies
    r = recommend_thresholds(_curve(thr, [90, 50, 20, 5], [0.7, 0.8, 0.85, 0.89]))
    assert r == {"auto_correct_threshold": None, "precision": None, "recall": None}
    # ties: equal precision at two thresholds, the bound met exactly -> the smaller threshold
    r = recommend_thresholds(_curve(thr, [90, 50, 20, 5], [0.7, 0.9, 0.9, 0.95]))
    assert r["auto_correct_threshold"] == 0.6
    # empty sets never qualify (their precision is 0 by convention, and a bound of 0 must not pick them)
    r = recommend_thresholds(_curve(thr, [0, 0, 0, 0], [0, 0, 0, 0]), min_noise_precision=0.0)
    assert r["auto_correct_threshold"] is None
    r = recommend_thresholds(_curve(thr, [10, 4, 0, 0], [0.5, 0.95, 0, 0]))
    assert r["auto_correct_threshold"] == 0.6
    # a precision that dips again: still the smallest threshold that meets the bound
    r = recommend_thresholds(_curve(thr, [90, 50, 20, 5], [0.92, 0.85, 0.95, 1.0]))
    assert r["auto_correct_threshold"] == 0.5
    # the review threshold: the largest within the share; ties on the share -> the larger threshold; none -> None
    c = _curve(thr, [90, 50, 20, 5], [0.7, 0.91, 0.95, 1.0], review_share=[0.0, 0.1, 0.1, 0.4])
    r = recommend_thresholds(c, max_review_share=0.1)
    assert r["review_threshold"] == 0.7 and r["review_share"] == 0.1 and r["auto_correct_threshold"] == 0.6
    assert recommend_thresholds(c, max_review_share=1.0)["review_threshold"] == 0.8
    c["review"]["share"] = [0.2, 0.3, 0.3, 0.4]
    r = recommend_thresholds(c, max_review_share=0.1)
    assert r["review_threshold"] is None and r["review_share"] is None
    assert "review_threshold" not in recommend_thresholds(c)


def test_recommend_thresholds_on_a_counted_curve():
    from bathymetric_gnn_amd.training import curve_from_block, recommend_thresholds
    thr = cc.thresholds_for(101)
    rng = np.random.default_rng(2)
    n = 20000
    labels = rng.choice([0, 2], n, p=[.8, .2]).astype(np.int32)
    conf = rng.random(n).astype(np.float32)
    # predictions are right with probability equal to their confidence: the precision of the noise set grows with the threshold
    pred = np.where(rng.random(n) < conf, labels, 2 - labels).astype(np.float32)
    curve = curve_from_block(cc.numpy_block(thr, labels, pred, conf), thr)
    r = recommend_thresholds(curve, 0.90, max_review_share=0.25)
    k = curve["thresholds"].index(r["auto_correct_threshold"])
    a = curve["auto_correct"]
    assert a["precision"][k] >= 0.90 and a["cells"][k] > 0 and r["recall"] == a["recall"][k]
    assert all(a["precision"][j] < 0.90 or a["cells"][j] == 0 for j in range(k))
    j = curve["thresholds"].index(r["review_threshold"])
    assert curve["review"]["share"][j] <= 0.25 and (j == 100 or curve["review"]["share"][j + 1] > 0.25)


@pytest.mark.parametrize("bad,word", [
    ([0.5, 0.4], "increasing"),                               # unsorted
    ([0.5, 0.5], "increasing"),                               # duplicate
    ([0.1, 0.1 + 1e-10], "increasing"),                       # duplicate only after the rounding to float32
    ([0.1, float("nan")], "finite"),
    ([float("nan")], "finite"),
    ([0.1, float("inf")], "finite"),
    ([0.1, 1e39], "finite"),                                  # inf after the rounding to float32
    ([], "0 entries"),                                        # T = 0
    (np.linspace(0, 1, 129), "129 entries"),                  # T = 129
    (np.zeros((2, 2)), "vector"),
])
def test_threshold_validation(bad, word):
    from bathymetric_gnn_amd.training.operating_curve import OperatingCurve, check_thresholds
    with pytest.raises(ValueError, match=word):
        check_thresholds(bad)
    with pytest.raises(ValueError, match=word):              # (raised before a device is looked for)
        OperatingCurve(bad, device="cuda:0")


def test_threshold_tables_that_pass():
    from bathymetric_gnn_amd.training.operating_curve import check_thresholds, default_thresholds
    d = default_thresholds()
    assert d.dtype == np.float32 and d.size == 101 and d[0] == 0 and d[-1] == 1 and (d[1:] > d[:-1]).all()
    assert np.array_equal(d, np.linspace(0, 1, 101).astype(np.float32))
    assert check_thresholds(np.linspace(0, 1, 128)).size == 128
    assert check_thresholds([0.5]).dtype == np.float32
    assert np.array_equal(check_thresholds((0, 1)), np.array([0, 1], np.float32))
    for T in (1, 2, 101, 128):
        assert check_thresholds(cc.thresholds_for(T)).size == T
