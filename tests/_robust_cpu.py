"""Host restatement of the robust sounding gridder's contract (include/bgnn_soundings_robust.h): the cell index, the clouds and
the constants of _soundings_cpu.py; ``np.lexsort((q, cell))`` for the sorted segments; Python / int64 integers for the median, the
distances, the MAD and the sums; numpy float64, operation by operation, for the rejection limit.  The device tests compare with it
bit for bit; test_host_soundings_robust.py holds it against the float64 median and MAD of the raw values."""
import functools
import math

import numpy as np

from _soundings_cpu import MIXED_ORIGIN, MIXED_RES, MIXED_SHAPE, SCALE, Z_CAP, cell_index, mixed_cloud

DEFAULT_K = 3 * 1.4826
PLANES = ("count", "kept", "median", "mad", "kept_mean", "kept_std", "kept_min", "kept_max", "valid", "center2", "limit")
LIMIT_CAP = 2.0 ** 34


def stage(x, y, z, shape, origin, res):
    """``(cell int64, q int64, counters)`` per sounding, in the order given: cell = -1 (and q = 0) where it is not accepted."""
    z = np.ascontiguousarray(z, np.float32)
    assert z.dtype == np.float32 and np.asarray(x).dtype == np.float64 and np.asarray(y).dtype == np.float64
    cell, finite_xy, inside = cell_index(x, y, origin[0], origin[1], res, shape)
    finite = finite_xy & np.isfinite(z)
    in_range = np.abs(z) < np.float32(Z_CAP)
    acc = finite & inside & in_range
    counters = {"accepted": int(acc.sum()), "nonfinite": int((~finite).sum()), "outside": int((finite & ~inside).sum()),
                "out_of_range": int((finite & inside & ~in_range).sum())}
    assert sum(counters.values()) == z.size
    q = np.zeros(z.size, np.int64)
    q[acc] = np.rint(z[acc].astype(np.float64) * SCALE).astype(np.int64)        # exact product, ties to even
    return np.where(acc, cell, -1), q, counters


def limit_of(D, k, floor_m):
    """``L = (int64)floor(min(max(k * (D * 0.5), floor_m * 131072), 2^34))`` in float64."""
    with np.errstate(over="ignore"):                             # (a product that overflows is +inf, and the cap takes it)
        td = max(np.float64(k) * (np.float64(D) * np.float64(0.5)), np.float64(floor_m) * np.float64(131072.0))
    return int(math.floor(min(td, np.float64(LIMIT_CAP))))


def cell_rule(s, k, floor_m):
    """``(m2, D, L, lo, hi)`` of one ascending segment of Python integers: the kept soundings are ``s[lo:hi]``."""
    n = len(s)
    m2 = s[(n - 1) // 2] + s[n // 2]
    d = sorted(abs(2 * v - m2) for v in s)
    D = d[(n - 1) // 2] + d[n // 2]
    L = limit_of(D, k, floor_m)
    keep = [abs(2 * v - m2) <= L for v in s]
    lo = keep.index(True)
    hi = n - keep[::-1].index(True)
    assert all(keep[lo:hi]) and sum(keep) == hi - lo             # contiguous
    return m2, D, L, lo, hi


def grid(x, y, z, shape, origin, res, k=DEFAULT_K, floor_m=0.0, min_count=1, nodata=1.0e6):
    """The planes, ``sorted_q`` (the accepted soundings filed by cell, ascending inside a cell; as long as there are accepted
    ones), ``start`` (``H * W + 1``), ``counters`` and ``flags`` (uint8 per sounding given) of the contract."""
    H, W = shape
    cells = H * W
    cell, q, counters = stage(x, y, z, shape, origin, res)
    acc = cell >= 0
    c, qa = cell[acc], q[acc]
    order = np.lexsort((qa, c))
    sorted_q = qa[order]
    n = np.bincount(c, minlength=cells).astype(np.int64)
    start = np.concatenate([[0], np.cumsum(n)]).astype(np.int64)
    out = {"count": n.astype(np.int32), "kept": np.zeros(cells, np.int32), "valid": np.zeros(cells, np.uint8),
           "center2": np.zeros(cells, np.int64), "limit": np.full(cells, -1, np.int64)}
    for name in ("median", "mad", "kept_mean", "kept_std", "kept_min", "kept_max"):
        out[name] = np.full(cells, nodata, np.float32)
    for i in np.flatnonzero(n):
        s = [int(v) for v in sorted_q[start[i]:start[i + 1]]]                    # Python integers from here
        m2, D, L, lo, hi = cell_rule(s, k, floor_m)
        kept = s[lo:hi]
        nk = len(kept)
        out["kept"][i], out["center2"][i], out["limit"][i] = nk, m2, L
        if nk < min_count:
            continue
        out["valid"][i] = 1
        out["median"][i] = np.float32(float(m2) * 2.0 ** -17)
        out["mad"][i] = np.float32(float(D) * 2.0 ** -18)
        S1, S2 = sum(kept), sum(v * v for v in kept)
        out["kept_mean"][i] = np.float32(float(S1) / float(nk) * 2.0 ** -16)
        num = nk * S2 - S1 * S1
        assert num >= 0
        out["kept_std"][i] = np.float32(math.sqrt(float(num) / (float(nk) * float(nk))) * 2.0 ** -16)  # float(int): one rounding
        out["kept_min"][i] = np.float32(float(kept[0]) * 2.0 ** -16)
        out["kept_max"][i] = np.float32(float(kept[-1]) * 2.0 ** -16)
    out = {name: v.reshape(H, W) for name, v in out.items()}
    out.update(sorted_q=sorted_q.astype(np.int32), start=start, counters=counters,
               flags=flags(x, y, z, shape, origin, res, out["center2"], out["limit"]))
    return out


def flags(x, y, z, shape, origin, res, center2, limit):
    """0 kept, 1 accepted but ``|2q - center2| > limit`` (every accepted sounding where ``limit == -1``), 2 not accepted."""
    cell, q, _ = stage(x, y, z, shape, origin, res)
    acc = cell >= 0
    f = np.full(cell.size, 2, np.uint8)
    c = cell[acc]
    d = np.abs(2 * q[acc] - np.asarray(center2, np.int64).reshape(-1)[c])
    f[acc] = (d > np.asarray(limit, np.int64).reshape(-1)[c]).astype(np.uint8)
    return f


@functools.lru_cache(maxsize=None)
def mixed_want(k=DEFAULT_K, floor_m=0.0, min_count=1):
    return grid(*mixed_cloud(), MIXED_SHAPE, MIXED_ORIGIN, MIXED_RES, k=k, floor_m=floor_m, min_count=min_count)
