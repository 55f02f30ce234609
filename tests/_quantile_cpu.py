"""The judges of the error-percentile tests (test_gpu_error_quantile.py, test_gpu_error_quantile_scale.py): the order-preserving key
of the header, the masked finite errors in numpy, numpy's float64 percentile, and ``check``, which holds everything a tracker has
(counters, the sorted stage, the top-digit histogram, the selected ranks, the percentiles) to them for equal bits."""
import math

import numpy as np
import torch

from bathymetric_gnn_amd import runtime as rt

PS = [50.0, 95.0, 99.9]


def _keys(e):
    """The order-preserving uint32 image of float32 values, as the header defines it."""
    u = np.ascontiguousarray(e, dtype=np.float32).view(np.uint32)
    return np.where(u & np.uint32(0x80000000), ~u, u | np.uint32(0x80000000)).astype(np.uint32)


def _errors(c, t, mask):
    """The masked rows' |c - t| in float32, and how many of them are not finite."""
    with np.errstate(invalid="ignore", over="ignore"):
        e = np.abs(c - t) if t is not None else c.copy()
    assert e.dtype == np.float32
    if mask is not None:
        e = e[mask.astype(bool)]
    fin = np.isfinite(e)
    return e[fin], int((~fin).sum())


def _want(e, p):
    return float(np.percentile(e.astype(np.float64), p))


def _ranks(m, p):
    lo = int(math.floor((m - 1) * (p / 100)))
    return lo, min(lo + 1, m - 1)


def _dev(a, dev, offset=0):
    """``a`` on the device; offset > 0: as a view that starts ``offset`` elements into a larger allocation (unaligned planes)."""
    if a is None:
        return None
    t = torch.from_numpy(np.ascontiguousarray(a))
    if offset == 0:
        return t.to(dev)
    big = torch.zeros(t.numel() + offset, dtype=t.dtype, device=dev)
    big[offset:] = t.to(dev)
    return big[offset:]


def _staged(tracker, count):
    return np.sort(tracker._stage[:count].cpu().numpy().view(np.uint32))


def _check(tracker, e, nonfinite, ps=PS):
    """Everything the tracker holds against the finite masked errors ``e`` (numpy), and the percentiles ``ps``."""
    st = tracker.state()
    m = e.size
    assert (int(st["rows"]), int(st["filed"]), int(st["nonfinite"]), int(st["dropped"]), int(st["cursor"])) == (m + nonfinite, m, nonfinite, 0, m)
    keys = np.sort(_keys(e))
    assert np.array_equal(_staged(tracker, m), keys)
    assert np.array_equal(st["hist"], np.bincount(keys >> 21, minlength=2048).astype(np.uint32))
    block = tracker.select(ps)
    assert (int(block["count"]), int(block["nonfinite"]), int(block["dropped"]), int(block["rows"])) == (m, nonfinite, 0, m + nonfinite)
    s = np.sort(e)
    for k in range(rt.QUANTILE_MAX_FRACTIONS):
        r = block["ranks"][k]
        if k < len(ps) and m > 0:
            lo, hi = _ranks(m, ps[k])
            assert (int(r["lo"]), int(r["hi"])) == (lo, hi)
            assert r["v_lo"].tobytes() == s[lo].tobytes() and r["v_hi"].tobytes() == s[hi].tobytes(), (k, r, s[lo], s[hi])
        else:
            assert int(r["lo"]) == int(r["hi"]) == -1 and np.isnan(r["v_lo"]) and np.isnan(r["v_hi"])
    got = tracker.percentiles(ps)
    assert (got["count"], got["nonfinite"], got["dropped"]) == (m, nonfinite, 0)
    if m == 0:
        assert got["values"] == [None] * len(ps)
    else:
        want = [_want(e, p) for p in ps]
        print(f"M={m} nonfinite={nonfinite} p={ps}: {got['values']} (numpy {want})")
        assert got["values"] == want
    return got


def _tracker(capacity, dev):
    from bathymetric_gnn_amd.training import CorrectionErrorTracker
    tr = CorrectionErrorTracker(capacity, device=dev)
    tr.reset()
    return tr


def _planes(n, seed, scale=3.0):
    rng = np.random.default_rng(seed)
    c = (rng.standard_normal(n) * scale).astype(np.float32)
    t = (rng.standard_normal(n) * scale).astype(np.float32)
    return rng, c, t
