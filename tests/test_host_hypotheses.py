"""The restatement of the depth hypotheses (_hypotheses_cpu.py) against brute force on hand-made segments, the range identity that
lets the flag passes apply a hypothesis result, the argument refusals of ``hypotheses()`` (all before anything is launched), and
the guards on the shared cloud that keep the device tests from being satisfied trivially.  No GPU needed."""
import itertools

import numpy as np
import pytest
import torch

import _hypotheses_cpu as hc
import _robust_cpu as rc
import _soundings_cpu as sc

M = 65536


def _robust_of(segments):
    """The part of ``rc.grid``'s result that the restatement reads, for hand-made cells on a 1 x K grid."""
    segments = [sorted(int(v) for v in s) for s in segments]
    start = np.concatenate([[0], np.cumsum([len(s) for s in segments])]).astype(np.int64)
    flat = [v for s in segments for v in s]
    return {"count": np.array([[len(s) for s in segments]], np.int32), "start": start, "sorted_q": np.asarray(flat, np.int32)}


def _brute(s, gap_q, min_count, g2):
    """Every pair of neighbours tested on its own; the candidates sorted by the whole key."""
    s = sorted(s)
    label = [0] * len(s)
    for i in range(1, len(s)):
        label[i] = label[i - 1] + (1 if s[i] - s[i - 1] > gap_q else 0)
    groups = [[v for v, lab in zip(s, label) if lab == h] for h in range(label[-1] + 1)] if s else []
    med2 = lambda v: v[(len(v) - 1) // 2] + v[len(v) // 2]
    cand = [(h, v) for h, v in enumerate(groups) if len(v) >= min_count]
    if g2 is None:
        cand.sort(key=lambda hv: (-len(hv[1]), abs(med2(hv[1]) - med2(s)), hv[0]))
    else:
        cand.sort(key=lambda hv: (abs(med2(hv[1]) - g2), -len(hv[1]), hv[0]))
    return groups, (cand[0][0] if cand else -1)


def test_restatement_against_brute_force():
    rng = np.random.default_rng(5)
    hand = [[], [5], [5, 5], [5, 6], [-2 * M, -1 * M, 1 * M, 2 * M],                             # the last: both keys tie
            [-40 * M, -39 * M, -10 * M, -9 * M, -8 * M, 20 * M, 21 * M, 22 * M, 30 * M, 31 * M, 32 * M],
            [-(2 ** 31 - M), 2 ** 31 - M], [-30 * M] * 3 + [-20 * M] * 2, [-30 * M] * 2 + [-20 * M] * 3]
    hand += [sorted(rng.integers(-50, 50, n).tolist()) for n in (3, 7, 20, 64, 65, 300)]
    guide = np.array([[0.0, 1.0, np.nan, np.inf, 0.0, -9.0, 40000.0, -25.0, -25.0, 1.0e6, -32768.0, 0.0003, -0.0002, 0.0, 0.0004]],
                     np.float32)
    assert guide.shape[1] == len(hand)
    robust = _robust_of(hand)
    for gap_q, min_count, rule in itertools.product((0, 1, 3, M, 2 ** 32 - 2 ** 17, 2 ** 32), (1, 2, 4), hc.RULES):
        got = hc.grid(robust, gap_q / 65536.0, rule, guide if rule == "guide" else None, min_count)
        assert got["gap_q"] == gap_q
        for c, s in enumerate(hand):
            g2 = hc.guide2_of(guide[0, c]) if rule == "guide" else None
            groups, chosen = _brute(s, gap_q, min_count, g2)
            assert got["n_hyp"][0, c] == len(groups) and got["chosen"][0, c] == chosen, (c, gap_q, min_count, rule)
            lo, hi = got["hyp_start"][c:c + 2]
            assert hi - lo == len(groups) and got["hyp_count"][lo:hi].tolist() == [len(v) for v in groups]
            assert [robust["sorted_q"][f] for f in got["hyp_first"][lo:hi]] == [v[0] for v in groups]
            assert [h["count"] for h in got["hyps"][c]] == [len(v) for v in groups]
            if chosen < 0:
                assert got["valid"][0, c] == 0 and got["kept"][0, c] == 0 and got["limit"][0, c] == -1 and got["center2"][0, c] == 0
                assert all(got[k][0, c] == np.float32(1.0e6) for k in hc.FLOATS)
                assert got["ambiguity"][0, c] == (1.0 if s else 0.0)
                continue
            run = groups[chosen]
            assert got["kept"][0, c] == len(run) and got["valid"][0, c] == 1
            assert abs(float(got["depth"][0, c]) - float(np.mean(run)) / 65536.0) <= 1e-6 * max(1.0, abs(float(np.mean(run)) / 65536.0))
            assert got["min"][0, c] == np.float32(run[0] / 65536.0) and got["max"][0, c] == np.float32(run[-1] / 65536.0)
            assert got["share"][0, c] == np.float32(len(run) / len(s))
            assert got["ambiguity"][0, c] == np.float32((len(s) - len(run)) / len(s))
    # the cases by name
    got = hc.grid(robust, 1.0, "count", None, 1)
    assert got["n_hyp"][0, 4] == 2 and got["chosen"][0, 4] == 0                  # symmetric: the lower index
    assert got["n_hyp"][0, 5] == 4 and got["chosen"][0, 5] == 2                  # three runs of 3: the nearest to the median (20 m)
    got = hc.grid(robust, 1.0, "guide", guide, 1)
    assert got["chosen"][0, 7] == 0 and got["chosen"][0, 8] == 1                 # a guide halfway: the larger count
    assert hc.grid(robust, 65536.0, "count", None, 1)["n_hyp"][0, 6] == 1        # 2^32 - 2^17 apart: one run at gap_q = 2^32 ...
    assert hc.grid(robust, (2 ** 32 - 2 ** 18) / 65536.0, "count", None, 1)["n_hyp"][0, 6] == 2      # ... and two below


def test_range_identity_of_center2_and_limit():
    """``|2q - center2| <= limit`` iff ``lo <= q <= hi`` for ``center2 = lo + hi``, ``limit = hi - lo``; nothing passes (0, -1)."""
    rng = np.random.default_rng(8)
    top = 2 ** 31 - M
    lo = rng.integers(-top, top + 1, 100000)
    hi = np.maximum(lo, rng.integers(-top, top + 1, 100000))
    hi[::7] = lo[::7]
    q = rng.integers(-top, top + 1, 100000)
    near = rng.integers(0, 4, 100000)
    q = np.where(near == 0, lo - rng.integers(0, 3, 100000), np.where(near == 1, hi + rng.integers(0, 3, 100000), q))
    q = np.clip(q, -top, top)
    inside = (lo <= q) & (q <= hi)
    assert inside.sum() > 10000 and (~inside).sum() > 10000
    assert np.array_equal(np.abs(2 * q - (lo + hi)) <= hi - lo, inside)
    assert not (np.abs(2 * q - 0) <= -1).any()


def _cpu_robust(shape=(2, 3)):
    from bathymetric_gnn_amd.data import RobustSoundingGrid
    cells = shape[0] * shape[1]
    plane = lambda dtype: torch.zeros(shape, dtype=dtype)
    return RobustSoundingGrid(count=plane(torch.int32), kept=plane(torch.int32), median=plane(torch.float32), mad=plane(torch.float32),
                              kept_mean=plane(torch.float32), kept_std=plane(torch.float32), kept_min=plane(torch.float32),
                              kept_max=plane(torch.float32), valid=plane(torch.uint8), center2=plane(torch.int64),
                              limit=plane(torch.int64), sorted_q=torch.zeros(4, dtype=torch.int32),
                              start=torch.zeros(cells + 1, dtype=torch.int32), counters={}, transform=(0.0, 1.0, 0.0, 2.0, 0.0, -1.0),
                              resolution=(1.0, 1.0))


def test_python_refusals_before_any_launch():
    """Every bad argument is refused before the context is asked for: host tensors never reach the library."""
    from bathymetric_gnn_amd.data import HypothesisGrid, VRHypothesisGrid, sounding_hypotheses as sh
    assert HypothesisGrid is sh.HypothesisGrid and VRHypothesisGrid is sh.VRHypothesisGrid
    g = _cpu_robust()
    with pytest.raises(TypeError):
        g.hypotheses()                                                           # gap_m is required
    for bad in (float("nan"), float("inf"), -0.001, 65536.001, -1):
        with pytest.raises(ValueError, match="gap_m"):
            g.hypotheses(bad)
    for bad in ("0.5", None, True, torch.tensor(0.5)):
        with pytest.raises(TypeError, match="gap_m"):
            g.hypotheses(bad)
    with pytest.raises(ValueError, match="rule"):
        g.hypotheses(0.5, rule="largest")
    with pytest.raises(ValueError, match="takes no guide"):
        g.hypotheses(0.5, guide=torch.zeros(2, 3))
    with pytest.raises(ValueError, match="needs a guide"):
        g.hypotheses(0.5, rule="guide")
    with pytest.raises(TypeError, match="guide"):
        g.hypotheses(0.5, rule="guide", guide=np.zeros((2, 3), np.float32))
    with pytest.raises(TypeError, match="float32"):
        g.hypotheses(0.5, rule="guide", guide=torch.zeros(2, 3, dtype=torch.float64))
    with pytest.raises(ValueError, match="shape"):
        g.hypotheses(0.5, rule="guide", guide=torch.zeros(3, 2))
    with pytest.raises(ValueError, match="min_count"):
        g.hypotheses(0.5, min_count=0)
    assert sh._check_gap(0.0) == (0.0, 0) and sh._check_gap(65536) == (65536.0, 2 ** 32) and sh._check_gap(0.5)[1] == 32768
    assert sh._check_gap(np.float32(0.05))[1] == hc.gap_q_of(np.float32(0.05))
    none = dict.fromkeys(sh.HYPOTHESIS_PLANES + ("sorted_q", "start", "hyp_first", "hyp_count"))
    no_records = HypothesisGrid(**none, hyp_start=None, gap_m=0.5, rule="count", transform=g.transform, resolution=g.resolution)
    with pytest.raises(ValueError, match="records"):
        no_records._hypotheses_of_cell(0)


def test_guards_on_the_mixed_cloud():
    """The shared cloud has many hypotheses per cell at every gap the device tests use, so no plane is right by default."""
    want = rc.mixed_want()
    assert want["counters"]["accepted"] == 17976 and want["count"].shape == sc.MIXED_SHAPE
    for gap_m, lo, hi, total in ((0.5, 2, 14, 1786), (0.05, 35, 64, 13079), (0.0, 44, 98, 17976)):
        got = hc.grid(want, gap_m)
        n = got["n_hyp"]
        assert (int(n.min()), int(n.max()), int(n.sum())) == (lo, hi, total), gap_m
        assert got["hyp_start"][-1] == total == got["hyp_first"].size == got["hyp_count"].size
        assert int(got["hyp_count"].sum()) == 17976 and (got["valid"] == 1).all()
        assert np.array_equal(got["kept"], np.array([max(h["count"] for h in hs) for hs in got["hyps"]]).reshape(n.shape))
    by_count = hc.grid(want, 0.5)
    guide = want["median"].copy()
    guide[0, 0], guide[3, 4], guide[7, 7], guide[15, 15] = np.nan, np.inf, 40000.0, 1.0e6
    by_guide = hc.grid(want, 0.5, "guide", guide, 2)
    assert (by_guide["chosen"] != by_count["chosen"]).any()
    for cell in ((0, 0), (3, 4), (7, 7), (15, 15)):                              # the cells without a usable guide: the count key
        assert by_guide["chosen"][cell] == hc.grid(want, 0.5, "count", None, 2)["chosen"][cell]
