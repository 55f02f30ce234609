"""The robust sounding gridder without a GPU: the restatement (_robust_cpu.py) against the float64 median and MAD of the raw
values, the structural facts of the rule, and its agreement with the first gridder's restatement where every sounding is kept.

The bounds.  median: every q is within 2^-17 m of its z and the median is 1-Lipschitz in every sample under the maximum norm, so
the median of the q (the mean of the two middle ones for an even count) is within 2^-17 m of the median of the z; the rounding to
float32 adds half a float32 ulp.  mad: |z_i - med| moves by at most 2^-17 m for the sample and 2^-17 m for the median, so the MAD
is within 2^-16 m; again half a float32 ulp for the rounding."""
import numpy as np
import pytest

import _robust_cpu as rc
import _soundings_cpu as sc


def _raw_cells(x, y, z):
    cell, finite_xy, inside = sc.cell_index(x, y, sc.MIXED_ORIGIN[0], sc.MIXED_ORIGIN[1], sc.MIXED_RES, sc.MIXED_SHAPE)
    acc = finite_xy & inside & np.isfinite(z) & (np.abs(z) < 32768)
    return {int(c): z[acc & (cell == c)].astype(np.float64) for c in np.unique(cell[acc])}


def test_restatement_against_float64_median_and_mad():
    x, y, z = sc.mixed_cloud()
    want = rc.mixed_want()
    raw = _raw_cells(x, y, z)
    assert len(raw) == 256 and 44 <= min(v.size for v in raw.values()) and max(v.size for v in raw.values()) <= 98
    worst_med = worst_mad = 0.0
    for i, v in raw.items():
        assert want["count"].reshape(-1)[i] == v.size and want["valid"].reshape(-1)[i] == 1
        med = float(np.median(v))
        mad = float(np.median(np.abs(v - med)))
        e_med = abs(float(want["median"].reshape(-1)[i]) - med)
        e_mad = abs(float(want["mad"].reshape(-1)[i]) - mad)
        b_med = 2.0 ** -17 + 0.5 * float(np.spacing(np.float32(abs(med))))
        b_mad = 2.0 ** -16 + 0.5 * float(np.spacing(np.float32(mad)))
        worst_med, worst_mad = max(worst_med, e_med / b_med), max(worst_mad, e_mad / b_mad)
        assert e_med <= b_med and e_mad <= b_mad, i
    print(f"median: {worst_med:.2f} of its bound at most, mad: {worst_mad:.2f}")


def test_rule_structure():
    """The kept soundings are contiguous (cell_rule asserts it for every cell), at least (n - 1) // 2 + 1 at k = 1, and all of them
    with floor_m = 65536."""
    x, y, z = sc.mixed_cloud()
    tight = rc.mixed_want(k=1.0)
    n, kept = tight["count"].astype(np.int64), tight["kept"].astype(np.int64)
    assert (kept >= (n - 1) // 2 + 1).all() and (kept < n).any()
    everything = rc.mixed_want(floor_m=65536.0)
    assert np.array_equal(everything["kept"], everything["count"]) and not everything["flags"].tolist().count(1)
    default = rc.mixed_want()
    rejected = int((default["count"].astype(np.int64) - default["kept"]).sum())
    assert rejected == 77 == int((default["flags"] == 1).sum())
    assert int((default["flags"] == 2).sum()) == z.size - default["counters"]["accepted"]
    assert default["start"][-1] == default["counters"]["accepted"] == default["sorted_q"].size
    # segments of every small shape: one, two, equal, two-valued, the widest values
    top = 2 ** 31 - 65536
    for s in ([5], [3, 9], [7, 7, 7], [1, 1, 9, 9], [-top, top], [-top, -top, top], [0, 1, 2, 1000]):
        m2, D, L, lo, hi = rc.cell_rule(sorted(s), 1.0, 0.0)
        assert hi - lo >= (len(s) - 1) // 2 + 1
        assert rc.cell_rule(sorted(s), 1.0, 65536.0)[3:] == (0, len(s))
    assert rc.cell_rule([7, 7, 7], rc.DEFAULT_K, 0.0) == (14, 0, 0, 0, 3)          # MAD 0, limit 0, all kept
    assert rc.cell_rule([3, 4], 1.0, 0.0)[:3] == (7, 2, 1)                          # a half-integer median
    assert rc.limit_of(2 ** 34, 1e300, 0.0) == 2 ** 34 == rc.limit_of(0, 1.0, 1e300)


@pytest.mark.parametrize("min_count", [1, 3])
def test_all_kept_equals_the_first_gridder(min_count):
    """With every sounding kept, count, kept_mean and kept_std are the first gridder's count, mean and std bit for bit."""
    robust = rc.mixed_want(floor_m=65536.0, min_count=min_count)
    first = sc.mixed_want(min_count)
    assert robust["counters"] == first["counters"]
    assert np.array_equal(robust["count"], first["count"]) and np.array_equal(robust["valid"], first["valid"])
    assert robust["kept_mean"].tobytes() == first["mean"].tobytes()
    assert robust["kept_std"].tobytes() == first["std"].tobytes()
    # kept_min / kept_max are the quantised extremes: within 2^-17 m (and half a float32 ulp) of the raw ones
    v = first["valid"].astype(bool)
    for mine, theirs in (("kept_min", "min"), ("kept_max", "max")):
        gap = np.abs(robust[mine][v].astype(np.float64) - first[theirs][v].astype(np.float64))
        assert (gap <= 2.0 ** -17 + 0.5 * np.spacing(np.abs(first[theirs][v])).astype(np.float64)).all()
