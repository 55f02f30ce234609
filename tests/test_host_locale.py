"""The restatements of the locale guide (_locale_cpu.py) against each other and against brute force (``np.sort`` of the gathered
witnesses) on planes up to 9 x 11 at every radius 1 .. 8, and ``data.guide_from_coarser`` against hand-made planes and its refusals,
on CPU tensors.  No GPU needed."""
import numpy as np
import pytest
import torch

import _locale_cpu as lc


def _brute(n_hyp, chosen, center2, radius, min_support):
    height, width = n_hyp.shape
    guide = np.full((height, width), lc.NAN_BITS, np.uint32)
    support = np.zeros((height, width), np.int32)
    witness = (n_hyp == 1) & (chosen == 0)
    for r in range(height):
        for c in range(width):
            rows = slice(max(r - radius, 0), min(r + radius, height - 1) + 1)
            cols = slice(max(c - radius, 0), min(c + radius, width - 1) + 1)
            mask = witness[rows, cols].copy()
            mask[r - rows.start, c - cols.start] = False
            w = np.sort(center2[rows, cols][mask])
            support[r, c] = w.size
            if w.size >= min_support:
                med2 = int(w[(w.size - 1) // 2]) + int(w[w.size // 2])
                guide[r, c] = np.float32(med2 / 262144.0).view(np.uint32)          # (med2 < 2^53: the quotient is exact)
    return guide, support


@pytest.mark.parametrize("radius", range(1, 9))
def test_restatements_agree(radius):
    rng = np.random.default_rng(100 + radius)
    window = (2 * radius + 1) ** 2 - 1
    seen_nan = seen_value = 0
    for shape in ((1, 1), (1, 7), (6, 1), (3, 5), (9, 11)):
        for share in (0.0, 0.3, 1.0):
            for spread in (8, lc.VALUE_TOP):
                planes = lc.random_planes(rng, shape, share, spread)
                for min_support in sorted({1, 3, window}):
                    want = _brute(*planes, radius, min_support)
                    for got in (lc.locale_guide(*planes, radius, min_support), lc.locale_guide_np(*planes, radius, min_support),
                                lc.locale_guide_np(*planes, radius, min_support, chunk_rows=2)):
                        assert got[0].dtype == np.uint32 and got[1].dtype == np.int32
                        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
                    seen_nan += int((want[0] == lc.NAN_BITS).sum())
                    seen_value += int((want[0] != lc.NAN_BITS).sum())
    assert seen_nan > 100 and seen_value > 100


def test_hand_made_cells():
    """3 x 3, radius 1: the centre's window is the eight cells around it."""
    n_hyp = np.ones((3, 3), np.int32)
    chosen = np.zeros((3, 3), np.int32)
    c2 = np.array([[10, 20, 30], [40, 2 ** 32 - 1, 50], [60, 70, 81]], np.int64)      # the centre is wild: not its own witness
    g, s = lc.locale_guide(n_hyp, chosen, c2, 1, 8)
    assert s[1, 1] == 8 and g[1, 1] == lc.guide_bits(40 + 50)                          # k even: the two middle ones
    assert s[0, 0] == 3 and g[0, 0] == lc.NAN_BITS                                     # a corner sees 3 < 8
    g, s = lc.locale_guide(n_hyp, chosen, c2, 1, 3)
    assert g[0, 0] == lc.guide_bits(2 * 40)                                            # 20, 40, 2^32 - 1: k odd, the middle twice
    n_hyp[0, 0], chosen[2, 2] = 2, -1                                                  # two ways of being no witness
    g, s = lc.locale_guide(n_hyp, chosen, c2, 1, 6)
    assert s[1, 1] == 6 and g[1, 1] == lc.guide_bits(40 + 50) and s[0, 1] == 4 and g[0, 1] == lc.NAN_BITS
    # one rounding: med2 = 2^33 - 2 needs 34 bits with its sign and is no float32; 2^-18 of it rounds to 32768.0
    top = np.full((1, 3), lc.VALUE_TOP, np.int64)
    g, s = lc.locale_guide(np.ones((1, 3), np.int32), np.zeros((1, 3), np.int32), top, 1, 1)
    assert s.tolist() == [[1, 2, 1]] and g[0, 1] == np.float32(32768.0).view(np.uint32) == lc.guide_bits(2 ** 33 - 2)
    assert lc.guide_bits(-(2 ** 33 - 2)) == np.float32(-32768.0).view(np.uint32)
    assert np.isnan(np.uint32(lc.NAN_BITS).view(np.float32))


# ---- guide_from_coarser ---------------------------------------------------------------------------------------------------------------

def _robust(median, valid, origin, res):
    from bathymetric_gnn_amd.data import RobustSoundingGrid
    median = torch.as_tensor(median, dtype=torch.float32)
    z32 = torch.zeros(median.shape, dtype=torch.int32)
    z64 = torch.zeros(median.shape, dtype=torch.int64)
    return RobustSoundingGrid(count=z32, kept=z32, median=median, mad=median, kept_mean=median + 1, kept_std=median, kept_min=median,
                              kept_max=median, valid=torch.as_tensor(valid, dtype=torch.uint8), center2=z64, limit=z64,
                              sorted_q=torch.zeros(1, dtype=torch.int32), start=torch.zeros(median.numel() + 1, dtype=torch.int32),
                              counters={}, transform=(origin[0], res, 0.0, origin[1], 0.0, -res), resolution=(res, res))


def _hyp(depth, valid, origin, res):
    from bathymetric_gnn_amd.data import HypothesisGrid
    depth = torch.as_tensor(depth, dtype=torch.float32)
    z32 = torch.zeros(depth.shape, dtype=torch.int32)
    z64 = torch.zeros(depth.shape, dtype=torch.int64)
    return HypothesisGrid(n_hyp=z32, chosen=z32, kept=z32, depth=depth, std=depth, min=depth - 1, max=depth, share=depth,
                          valid=torch.as_tensor(valid, dtype=torch.uint8), center2=z64, limit=z64, hyp_start=None, hyp_first=None,
                          hyp_count=None, sorted_q=torch.zeros(1, dtype=torch.int32), start=torch.zeros(depth.numel() + 1, dtype=torch.int32),
                          gap_m=0.5, rule="count", transform=(origin[0], res, 0.0, origin[1], 0.0, -res), resolution=(res, res))


def test_guide_from_coarser():
    from bathymetric_gnn_amd.data import guide_from_coarser
    coarse = _robust([[-10.0, -20.0], [-30.0, 1.0e6]], [[1, 1], [1, 0]], (500.0, 900.0), 3.0)
    like = _robust(np.zeros((5, 4)), np.ones((5, 4)), (500.0, 900.0), 1.0)
    g = guide_from_coarser(coarse, like)
    nan = float("nan")
    want = np.array([[-10, -10, -10, -20]] * 3 + [[-30, -30, -30, nan]] * 2, np.float32)
    assert g.dtype == torch.float32 and tuple(g.shape) == (5, 4) and g.is_contiguous()
    assert np.array_equal(g.numpy().view(np.uint32), want.view(np.uint32))
    assert torch.equal(guide_from_coarser(coarse, like, plane="kept_mean")[:3, :3], torch.full((3, 3), -9.0))
    # the same resolution: the plane itself, NaN where not valid; a HypothesisGrid on either side
    same = guide_from_coarser(coarse, _hyp(np.zeros((2, 2)), np.ones((2, 2)), (500.0, 900.0), 3.0))
    assert np.array_equal(same.numpy().view(np.uint32), np.array([[-10, -20], [-30, nan]], np.float32).view(np.uint32))
    hyp = _hyp([[-5.0, -6.0]], [[1, 1]], (500.0, 900.0), 2.0)
    assert guide_from_coarser(hyp, like := _robust(np.zeros((2, 3)), np.ones((2, 3)), (500.0, 900.0), 1.0), plane="depth").tolist() == \
        [[-5.0, -5.0, -6.0]] * 2
    assert guide_from_coarser(hyp, like, plane="min").tolist() == [[-6.0, -6.0, -7.0]] * 2
    # a full cover of 6 x 6 by 2 x 2 at three times the resolution
    full = guide_from_coarser(coarse, _robust(np.zeros((6, 6)), np.ones((6, 6)), (500.0, 900.0), 1.0))
    assert tuple(full.shape) == (6, 6) and full[2, 3] == -20.0 and torch.isnan(full[3:, 3:]).all() and not torch.isnan(full[:3]).any()


def test_guide_from_coarser_refusals():
    from bathymetric_gnn_amd.data import guide_from_coarser
    coarse = _robust(np.zeros((2, 2)), np.ones((2, 2)), (500.0, 900.0), 3.0)
    ok = _robust(np.zeros((5, 4)), np.ones((5, 4)), (500.0, 900.0), 1.0)
    guide_from_coarser(coarse, ok)
    with pytest.raises(ValueError, match="whole multiple"):
        guide_from_coarser(coarse, _robust(np.zeros((2, 2)), np.ones((2, 2)), (500.0, 900.0), 2.0))
    with pytest.raises(ValueError, match="whole multiple"):                           # finer, not coarser
        guide_from_coarser(ok, coarse)
    with pytest.raises(ValueError, match="origins"):
        guide_from_coarser(coarse, _robust(np.zeros((5, 4)), np.ones((5, 4)), (501.0, 900.0), 1.0))
    with pytest.raises(ValueError, match="origins"):
        guide_from_coarser(coarse, _robust(np.zeros((5, 4)), np.ones((5, 4)), (500.0, 899.0), 1.0))
    with pytest.raises(ValueError, match="coverage"):
        guide_from_coarser(coarse, _robust(np.zeros((7, 4)), np.ones((7, 4)), (500.0, 900.0), 1.0))
    with pytest.raises(ValueError, match="coverage"):
        guide_from_coarser(coarse, _robust(np.zeros((5, 7)), np.ones((5, 7)), (500.0, 900.0), 1.0))
    with pytest.raises(ValueError, match="plane"):
        guide_from_coarser(coarse, ok, plane="depth")
    with pytest.raises(ValueError, match="plane"):
        guide_from_coarser(_hyp(np.zeros((2, 2)), np.ones((2, 2)), (500.0, 900.0), 3.0), ok)       # "median" is no plane of a HypothesisGrid
    with pytest.raises(TypeError):
        guide_from_coarser(torch.zeros(2, 2), ok)
    with pytest.raises(TypeError):
        guide_from_coarser(coarse, None)
