"""Host restatement of the variable-resolution sounding gridders' contract (include/bgnn_soundings_vr.h): numpy float64,
operation by operation, for the base cell and the record address; Python integers for the planner.  The per-record statistics are
those of _soundings_cpu.py and _robust_cpu.py, which are called, not copied: a layout of ``total`` records is handed to them as a
``1 x total`` grid of unit cells, every sounding at the centre of its record.  The device tests compare with it bit for bit."""
import functools

import numpy as np

import _robust_cpu
import _soundings_cpu
from _soundings_cpu import Z_CAP

COUNTERS = ("accepted", "nonfinite", "outside", "out_of_range", "unrefined")
ACCEPTED, NONFINITE, OUTSIDE, OUT_OF_RANGE, UNREFINED = range(5)
DEFAULT_LADDER = (1, 2, 4, 8, 16, 32, 64)
MAX_DIM = 32768


def make_layout(base_shape, origin, B, dx, dy, index=None):
    """A layout as a dict: ``dx``, ``dy`` ``[BH, BW]`` (0: not refined), ``index`` (default: the exclusive sum of ``dx * dy`` in
    row-major order from the south-west), ``total`` the end of the last record range."""
    BH, BW = base_shape
    dx = np.asarray(dx, np.int64).reshape(BH, BW)
    dy = np.asarray(dy, np.int64).reshape(BH, BW)
    cells = np.where((dx > 0) & (dy > 0), dx * dy, 0).reshape(-1)
    if index is None:
        index = np.concatenate([[0], np.cumsum(cells)[:-1]]).astype(np.int64)
    index = np.asarray(index, np.int64).reshape(BH, BW)
    total = int((index.reshape(-1) + cells)[cells > 0].max()) if (cells > 0).any() else 0
    return {"base_shape": (BH, BW), "origin": (float(origin[0]), float(origin[1])), "B": float(B), "dx": dx, "dy": dy,
            "index": index, "total": total}


def base_cell(x, y, origin, B, base_shape):
    """``(b, fu, fv, finite_xy, on_grid)``: float64, true divisions, floor; b is int64 ``br * BW + bc`` on the grid, -1 elsewhere."""
    BH, BW = base_shape
    x, y = np.asarray(x, np.float64), np.asarray(y, np.float64)
    finite = np.isfinite(x) & np.isfinite(y)
    with np.errstate(invalid="ignore", over="ignore"):
        u = (x - np.float64(origin[0])) / np.float64(B)
        v = (y - np.float64(origin[1])) / np.float64(B)
        bc, br = np.floor(u), np.floor(v)
        on = finite & (bc >= 0) & (bc < BW) & (br >= 0) & (br < BH)
        fu, fv = u - bc, v - br
    b = np.full(x.shape, -1, np.int64)
    b[on] = br[on].astype(np.int64) * np.int64(BW) + bc[on].astype(np.int64)
    return b, np.where(on, fu, 0.0), np.where(on, fv, 0.0), finite, on


def classify(x, y, z, layout):
    """``(kind, record)`` per sounding: the kind in the contract's order of checks, the record (int64) where accepted, else -1."""
    z = np.ascontiguousarray(z, np.float32)
    assert z.dtype == np.float32 and np.asarray(x).dtype == np.float64 and np.asarray(y).dtype == np.float64
    b, fu, fv, finite_xy, on = base_cell(x, y, layout["origin"], layout["B"], layout["base_shape"])
    dx, dy, index = (layout[k].reshape(-1)[np.maximum(b, 0)] for k in ("dx", "dy", "index"))
    refined = on & (dx > 0) & (dy > 0)
    sc = np.floor(fu * dx.astype(np.float64)).astype(np.int64)
    sr = np.floor(fv * dy.astype(np.float64)).astype(np.int64)
    record = index + sr * dx + sc
    finite = finite_xy & np.isfinite(z)
    in_range = np.abs(z) < np.float32(Z_CAP)
    kind = np.full(z.shape, ACCEPTED, np.int64)
    kind[~in_range] = OUT_OF_RANGE                       # (the later assignments are the earlier checks)
    kind[~refined] = UNREFINED
    kind[~on] = OUTSIDE
    kind[~finite] = NONFINITE
    return kind, np.where(kind == ACCEPTED, record, -1)


def counters_of(kind):
    return {name: int((kind == i).sum()) for i, name in enumerate(COUNTERS)}


def _proxy(x, y, z, layout):
    """The cloud as the uniform restatements take it on the ``1 x total`` grid with origin (0, 1) and unit cells: a sounding that
    is accepted or out of range at the centre of its record, a nonfinite one at NaN, an outside or unrefined one off the grid."""
    kind, _ = classify(x, y, z, layout)
    _, record = classify(x, y, np.zeros(len(z), np.float32), layout)       # the record of an out-of-range sounding too
    xp = np.where(record >= 0, record.astype(np.float64) + 0.5, -1.0)
    xp[kind == NONFINITE] = np.nan
    xp[(kind == OUTSIDE) | (kind == UNREFINED)] = -1.0
    return kind, xp, np.full(len(z), 0.5, np.float64)


def _fix_counters(out, kind):
    want = counters_of(kind)
    got = out["counters"]
    assert got["outside"] == want["outside"] + want["unrefined"] and all(got[k] == want[k] for k in COUNTERS[:2] + COUNTERS[3:4])
    out["counters"] = want
    return out


def grid(x, y, z, layout, min_count=1, nodata=1.0e6):
    """The six planes of _soundings_cpu.grid as flat ``[total]`` arrays, and the five counters."""
    kind, xp, yp = _proxy(x, y, z, layout)
    out = _soundings_cpu.grid(xp, yp, z, (1, layout["total"]), (0.0, 1.0), 1.0, min_count=min_count, nodata=nodata)
    out = {k: (v.reshape(-1) if isinstance(v, np.ndarray) else v) for k, v in out.items()}
    return _fix_counters(out, kind)


def robust_grid(x, y, z, layout, k=_robust_cpu.DEFAULT_K, floor_m=0.0, min_count=1, nodata=1.0e6):
    """The planes, ``sorted_q``, ``start``, ``flags`` of _robust_cpu.grid over the records, and the five counters."""
    kind, xp, yp = _proxy(x, y, z, layout)
    out = _robust_cpu.grid(xp, yp, z, (1, layout["total"]), (0.0, 1.0), 1.0, k=k, floor_m=floor_m, min_count=min_count, nodata=nodata)
    out = {name: (v.reshape(-1) if name in _robust_cpu.PLANES else v) for name, v in out.items()}
    return _fix_counters(out, kind)


def robust_flags(x, y, z, layout, center2, limit):
    _, xp, yp = _proxy(x, y, z, layout)
    return _robust_cpu.flags(xp, yp, z, (1, layout["total"]), (0.0, 1.0), 1.0, center2, limit)


def density(x, y, z, origin, B, base_shape):
    """The soundings per base cell that pass every check but ``unrefined``: int64 ``[BH, BW]``."""
    z = np.ascontiguousarray(z, np.float32)
    b, _, _, finite_xy, on = base_cell(x, y, origin, B, base_shape)
    ok = on & finite_xy & np.isfinite(z) & (np.abs(z) < np.float32(Z_CAP))
    return np.bincount(b[ok], minlength=base_shape[0] * base_shape[1]).astype(np.int64).reshape(base_shape)


def plan_dim(n, target_count, ladder=DEFAULT_LADDER, min_base_count=1):
    """The dimension of a base cell of ``n`` soundings, in Python integers."""
    n = int(n)
    if n < min_base_count:
        return 0
    fits = [int(d) for d in ladder if n >= int(target_count) * int(d) * int(d)]
    return max(fits) if fits else 0


def plan(counts, target_count, ladder=DEFAULT_LADDER, min_base_count=1):
    """``(index, d, total)``: ``d`` int64 ``[BH, BW]``, ``index`` the exclusive sum of ``d * d`` in row-major order, ``total``."""
    counts = np.asarray(counts)
    d = [plan_dim(n, target_count, ladder, min_base_count) for n in counts.reshape(-1).tolist()]
    index, run = [], 0
    for v in d:
        index.append(run)
        run += v * v
    return np.asarray(index, np.int64).reshape(counts.shape), np.asarray(d, np.int64).reshape(counts.shape), run


def metadata(layout):
    """The varres_metadata of a layout, as ``VRLayout.metadata`` documents it."""
    md = np.zeros(layout["base_shape"], [("index", "<u4"), ("dimensions_x", "<u4"), ("dimensions_y", "<u4"), ("resolution_x", "<f4"),
                                         ("resolution_y", "<f4"), ("sw_corner_x", "<f4"), ("sw_corner_y", "<f4")])
    ref = (layout["dx"] > 0) & (layout["dy"] > 0)
    md["index"] = np.where(ref, layout["index"], 0xFFFFFFFF)
    md["dimensions_x"], md["dimensions_y"] = np.where(ref, layout["dx"], 0), np.where(ref, layout["dy"], 0)
    for name, d in (("resolution_x", layout["dx"]), ("resolution_y", layout["dy"])):
        md[name] = np.where(ref, np.float64(layout["B"]) / np.maximum(d, 1), 0.0).astype(np.float32)
    return md


def uniform_to_records(plane, base_shape, d):
    """A north-up ``[BH * d, BW * d]`` plane of the uniform gridders regrouped into the records of the uniform layout (every base
    cell ``d x d``, row-major from the south-west): flipud, then base cell after base cell."""
    BH, BW = base_shape
    return np.flipud(plane).reshape(BH, d, BW, d).transpose(0, 2, 1, 3).reshape(-1)


# ---- the shared layouts and clouds (built once, read-only) -------------------------------------------------------------------------
MIXED_BASE, MIXED_ORIGIN = (7, 5), (5.0e5 + 0.3, 4.1e6)
_MIXED_DX = [[0, 1, 2, 3, 5], [8, 64, 0, 3, 5], [2, 2, 1, 0, 8], [5, 3, 64, 1, 2], [0, 0, 3, 5, 8], [1, 2, 3, 5, 3], [8, 5, 2, 1, 0]]
_MIXED_DY = [[0, 1, 2, 5, 3], [8, 64, 0, 3, 5], [2, 2, 1, 0, 8], [5, 3, 64, 1, 2], [0, 0, 5, 3, 8], [1, 2, 3, 5, 3], [8, 5, 2, 1, 0]]


def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


@functools.lru_cache(maxsize=None)
def mixed_layout(B):
    """Test 1's layout: base grid 7 x 5, dimensions from {0, 1, 2, 3, 5, 8, 64}, with 3 x 5 and 5 x 3 (dx x dy) grids."""
    return make_layout(MIXED_BASE, MIXED_ORIGIN, B, _MIXED_DX, _MIXED_DY)


@functools.lru_cache(maxsize=None)
def mixed_cloud(B, n=200000, seed=17):
    """Test 1's cloud: ``n`` soundings over the 7 x 5 base grid; one in ten beyond a border; a contaminated tenth; planted NaN /
    inf in each of x, y, z, |z| at and beside 32768, soundings on the outer borders."""
    rng = np.random.default_rng(seed)
    (BH, BW), (x0, y0) = MIXED_BASE, MIXED_ORIGIN
    x = x0 + rng.uniform(0, BW * B, n)
    y = y0 + rng.uniform(0, BH * B, n)
    z = (-25.0 + 0.2 * rng.standard_normal(n)).astype(np.float32)
    burst = rng.random(n) < 0.1
    z[burst] += (3.0 * rng.standard_normal(int(burst.sum()))).astype(np.float32)
    out = rng.random(n) < 0.10
    side = rng.integers(0, 4, n)
    far = rng.uniform(0.0, 3.0, n)
    x = np.where(out & (side == 0), x0 - far - 1e-9, x)
    x = np.where(out & (side == 1), x0 + BW * B + far, x)
    y = np.where(out & (side == 2), y0 - far - 1e-9, y)
    y = np.where(out & (side == 3), y0 + BH * B + far, y)
    p = rng.choice(np.flatnonzero(~out), 16, replace=False)
    x[p[0]] = np.nan; y[p[1]] = np.nan; z[p[2]] = np.nan
    x[p[3]] = np.inf; y[p[4]] = -np.inf; z[p[5]] = np.inf; z[p[6]] = -np.inf
    z[p[7]] = 40000.0; z[p[8]] = -32768.0; z[p[9]] = 32767.99; z[p[10]] = -32767.99
    x[p[11]] = x0; y[p[12]] = y0
    x[p[13]] = x0 + BW * B; y[p[14]] = y0 + BH * B
    z[p[15]] = -0.0
    # out-of-range depths inside refined cells (base cell (1, 1), 64 x 64) and an unrefined one (base cell (0, 0))
    q = rng.choice(np.flatnonzero(~out), 8, replace=False)
    x[q[:4]] = x0 + 1.5 * B; y[q[:4]] = y0 + 1.5 * B; z[q[:4]] = 5.0e4
    x[q[4:]] = x0 + 0.5 * B; y[q[4:]] = y0 + 0.5 * B; z[q[4:]] = -5.0e4
    return _frozen(x, y, z)


BORDER_BASE_CELLS, BORDER_X0 = 16, 5.0e5 + 0.3


@functools.lru_cache(maxsize=None)
def border_cloud(B, d, seed=5):
    """Test 2's coordinates: ``x0 + (b + s / d) * B`` for every base cell b < 16 and s < d, and one float64 step on either side of
    each (``3 * 16 * d`` values), and depths to go with them."""
    b, s = np.meshgrid(np.arange(BORDER_BASE_CELLS, dtype=np.float64), np.arange(d, dtype=np.float64), indexing="ij")
    on = (np.float64(BORDER_X0) + (b + s / np.float64(d)) * np.float64(B)).reshape(-1)
    t = np.concatenate([on, np.nextafter(on, -np.inf), np.nextafter(on, np.inf)])
    z = (-10.0 + np.random.default_rng(seed).standard_normal(t.size)).astype(np.float32)
    return _frozen(t, z)


def border_layout(B, d, along_x=True):
    """A row (or a column) of 16 base cells at ``BORDER_X0``, each ``d x d``."""
    shape = (1, BORDER_BASE_CELLS) if along_x else (BORDER_BASE_CELLS, 1)
    return make_layout(shape, (BORDER_X0, BORDER_X0), B, np.full(shape, d), np.full(shape, d))
