"""Host restatement of the sounding gridder's contract (include/bgnn_soundings.h): numpy float64 for the cell index, Python
integers for S1, S2 and the variance numerator.  The device tests compare with it bit for bit; test_host_soundings.py holds it
against the float64 mean and standard deviation of the raw values.  Also the shared test clouds (built once, read-only)."""
import functools
import math

import numpy as np

SCALE = 65536
Z_CAP = 32768.0
COUNTERS = ("accepted", "nonfinite", "outside", "out_of_range")


def cell_index(x, y, x0, y0, res, shape):
    """``(cell, finite_xy, inside)``: float64, true division, floor; cell is int64 ``row * W + col`` where inside, -1 elsewhere."""
    H, W = shape
    x, y = np.asarray(x, np.float64), np.asarray(y, np.float64)
    finite = np.isfinite(x) & np.isfinite(y)
    with np.errstate(invalid="ignore", over="ignore"):
        col = np.floor((x - np.float64(x0)) / np.float64(res))
        row = np.floor((np.float64(y0) - y) / np.float64(res))
        inside = finite & (col >= 0) & (col < W) & (row >= 0) & (row < H)
    cell = np.full(x.shape, -1, np.int64)
    cell[inside] = row[inside].astype(np.int64) * np.int64(W) + col[inside].astype(np.int64)
    return cell, finite, inside


def order_key(z):
    """float32 onto uint32, order-preserving (-0.0 below +0.0)."""
    u = np.ascontiguousarray(z, np.float32).view(np.uint32)
    return np.where(u & np.uint32(0x80000000), ~u, u | np.uint32(0x80000000)).astype(np.uint32)


def order_value(key):
    key = np.asarray(key, np.uint32)
    u = np.where(key & np.uint32(0x80000000), key & np.uint32(0x7FFFFFFF), ~key).astype(np.uint32)
    return u.view(np.float32)


def grid(x, y, z, shape, origin, res, min_count=1, nodata=1.0e6):
    """The six planes and the counters of the contract: a dict of ``count`` int32, ``mean`` / ``std`` / ``min`` / ``max`` float32,
    ``valid`` uint8 (all ``[H, W]``) and ``counters``."""
    H, W = shape
    z = np.ascontiguousarray(z, np.float32)
    assert z.dtype == np.float32 and np.asarray(x).dtype == np.float64 and np.asarray(y).dtype == np.float64
    cell, finite_xy, inside = cell_index(x, y, origin[0], origin[1], res, shape)
    finite = finite_xy & np.isfinite(z)
    in_range = np.abs(z) < np.float32(Z_CAP)
    acc = finite & inside & in_range
    counters = {"accepted": int(acc.sum()), "nonfinite": int((~finite).sum()), "outside": int((finite & ~inside).sum()),
                "out_of_range": int((finite & inside & ~in_range).sum())}
    assert sum(counters.values()) == z.size
    c, za = cell[acc], z[acc]
    q = np.rint(za.astype(np.float64) * SCALE).astype(np.int64)                 # exact product, ties to even
    cells = H * W
    n = np.bincount(c, minlength=cells).astype(np.int64)
    s1 = np.zeros(cells, np.int64)
    np.add.at(s1, c, q)                                                          # |S1| < 2^62
    q2 = q * q                                                                   # < 2^62
    lo, hi = np.zeros(cells, np.int64), np.zeros(cells, np.int64)
    np.add.at(lo, c, q2 & 0xFFFFFFFF)
    np.add.at(hi, c, q2 >> 32)
    key = order_key(za)
    kmin = np.full(cells, 0xFFFFFFFF, np.uint32)
    kmax = np.zeros(cells, np.uint32)
    np.minimum.at(kmin, c, key)
    np.maximum.at(kmax, c, key)
    mean = np.full(cells, nodata, np.float32)
    std = np.full(cells, nodata, np.float32)
    valid = n >= min_count
    for i in np.flatnonzero(valid):
        ni, S1, S2 = int(n[i]), int(s1[i]), (int(hi[i]) << 32) + int(lo[i])     # Python integers from here
        mean[i] = np.float32(float(S1) / float(ni) * 2.0 ** -16)
        num = ni * S2 - S1 * S1
        assert num >= 0
        std[i] = np.float32(math.sqrt(float(num) / (float(ni) * float(ni))) * 2.0 ** -16)    # float(int): one rounding, ties to even
    zmin = np.where(valid, order_value(kmin), np.float32(nodata)).astype(np.float32)
    zmax = np.where(valid, order_value(kmax), np.float32(nodata)).astype(np.float32)
    r = lambda a: a.reshape(H, W)
    return {"count": r(n.astype(np.int32)), "mean": r(mean), "std": r(std), "min": r(zmin), "max": r(zmax),
            "valid": r(valid.astype(np.uint8)), "counters": counters}


# ---- the shared clouds -----------------------------------------------------------------------------------------------------------
MIXED_SHAPE, MIXED_ORIGIN, MIXED_RES = (16, 16), (500000.0, 4000000.0), 0.3


def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


@functools.lru_cache(maxsize=None)
def mixed_cloud(n=20000, seed=11):
    """Test 1's cloud: ``n`` soundings over the 16 x 16 grid at res 0.3, origin (500000, 4000000); one in ten spread beyond every
    border; planted NaN in each of x, y, z, +-inf, z = 40000, z = -32768, z = 32767.99, and soundings on the outer borders."""
    rng = np.random.default_rng(seed)
    (H, W), (x0, y0), res = MIXED_SHAPE, MIXED_ORIGIN, MIXED_RES
    x = x0 + rng.uniform(0, W * res, n)
    y = y0 - rng.uniform(0, H * res, n)
    z = (-25.0 + 3.0 * rng.standard_normal(n)).astype(np.float32)
    out = rng.random(n) < 0.10
    side = rng.integers(0, 4, n)
    far = rng.uniform(0.0, 3.0, n)
    x = np.where(out & (side == 0), x0 - far, x)
    x = np.where(out & (side == 1), x0 + W * res + far, x)
    y = np.where(out & (side == 2), y0 + far + 1e-9, y)
    y = np.where(out & (side == 3), y0 - H * res - far, y)
    p = rng.choice(np.flatnonzero(~out), 16, replace=False)                     # planted on soundings that lie inside
    x[p[0]] = np.nan; y[p[1]] = np.nan; z[p[2]] = np.nan
    x[p[3]] = np.inf; y[p[4]] = -np.inf; z[p[5]] = np.inf; z[p[6]] = -np.inf
    z[p[7]] = 40000.0; z[p[8]] = -32768.0; z[p[9]] = 32767.99; z[p[10]] = -32767.99
    x[p[11]] = x0; y[p[12]] = y0                                                # on the upper-left borders: inside
    x[p[13]] = x0 + W * res; y[p[14]] = y0 - H * res                            # at the lower-right borders, as float64 puts them
    z[p[15]] = -0.0
    return _frozen(x, y, z)


@functools.lru_cache(maxsize=None)
def mixed_want(min_count=1):
    return grid(*mixed_cloud(), MIXED_SHAPE, MIXED_ORIGIN, MIXED_RES, min_count=min_count)


@functools.lru_cache(maxsize=None)
def border_cloud(res, n_cells=4096, seed=5):
    """Test 2's coordinates: ``k * res`` for every k < n_cells and one float64 step on either side of each (3 * n_cells values,
    from origin 0), and depths to go with them."""
    k = np.arange(n_cells, dtype=np.float64)
    on = k * np.float64(res)
    t = np.concatenate([on, np.nextafter(on, -np.inf), np.nextafter(on, np.inf)])
    z = (-10.0 + np.random.default_rng(seed).standard_normal(t.size)).astype(np.float32)
    return _frozen(t, z)


@functools.lru_cache(maxsize=None)
def runs_cloud(max_run=130, seed=3):
    """Test 4's stream on an 8 x 8 grid at res 1, origin (0, 8): equal-cell runs of lengths 1 .. max_run laid end to end, the cell
    changing from run to run, so that runs straddle wave (64) and workgroup (256, 1024) boundaries."""
    rng = np.random.default_rng(seed)
    cells = np.concatenate([np.full(L, (7 * L + 3) % 64) for L in range(1, max_run + 1)])
    n = cells.size
    x = (cells % 8) + rng.uniform(0.01, 0.99, n)
    y = 8.0 - ((cells // 8) + rng.uniform(0.01, 0.99, n))
    z = (-40.0 + 5.0 * rng.standard_normal(n)).astype(np.float32)
    return _frozen(x.astype(np.float64), y.astype(np.float64), z)
