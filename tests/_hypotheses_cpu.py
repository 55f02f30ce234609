"""Host restatement of the depth hypotheses' contract (include/bgnn_hypotheses.h) on top of ``_robust_cpu.grid``: the runs, the keys,
the planes, the records and ``ambiguity`` written out in Python integers over the ``sorted_q`` / ``start`` of the robust
restatement; float64 only where the contract rounds (once per value).  The device tests compare with it bit for bit;
test_host_hypotheses.py holds it against brute force on hand-made segments."""
import math

import numpy as np

PLANES = ("n_hyp", "chosen", "kept", "depth", "std", "min", "max", "share", "valid", "center2", "limit")
FLOATS = ("depth", "std", "min", "max", "share")
RECORDS = ("hyp_start", "hyp_first", "hyp_count")
RULES = ("count", "guide")
MAX_GAP_Q = 2 ** 32


def gap_q_of(gap_m):
    """``llrint(gap_m * 65536)``: float64 product, ties to even."""
    return int(np.rint(np.float64(gap_m) * np.float64(65536.0)))


def runs_of(s, gap_q):
    """``[(a, n_h), ..]`` of one ascending segment of Python integers: a break sits before i iff ``s[i] - s[i-1] > gap_q``."""
    runs, a = [], 0
    for i in range(1, len(s) + 1):
        if i == len(s) or s[i] - s[i - 1] > gap_q:
            runs.append((a, i - a))
            a = i
    return runs


def guide2_of(g):
    """Twice the guide in units of 2^-17 m, or ``None`` where the cell takes the count key (not finite, or ``|g| >= 32768``)."""
    g = np.float32(g)
    if not np.isfinite(g) or abs(float(g)) >= 32768.0:
        return None
    return 2 * int(np.rint(np.float64(g) * np.float64(65536.0)))


def choose(s, runs, min_count, g2=None):
    """The index of the chosen run or -1: the smallest ``(-n_h, |m2_h - c2|, h)``, or ``(|m2_h - g2|, -n_h, h)`` under a guide."""
    n = len(s)
    keys = []
    for h, (a, nh) in enumerate(runs):
        if nh < min_count:
            continue
        m2 = s[a + (nh - 1) // 2] + s[a + nh // 2]
        if g2 is None:
            keys.append((-nh, abs(m2 - (s[(n - 1) // 2] + s[n // 2])), h))
        else:
            keys.append((abs(m2 - g2), -nh, h))
    return min(keys)[2] if keys else -1


def grid(robust, gap_m, rule="count", guide=None, min_count=1, nodata=1.0e6):
    """The eleven planes (in the shape of ``robust["count"]``), the three records (``hyp_first`` / ``hyp_count`` as long as there
    are hypotheses), ``ambiguity`` and ``hyps`` (per cell the ``hypotheses_of`` list) from the ``sorted_q`` / ``start`` of
    ``_robust_cpu.grid``."""
    assert rule in RULES and (guide is None) == (rule == "count") and min_count >= 1
    gap_q = gap_q_of(gap_m)
    assert 0 <= gap_q <= MAX_GAP_Q
    shape = robust["count"].shape
    start, sorted_q = robust["start"], robust["sorted_q"]
    cells = start.size - 1
    g = None if guide is None else np.asarray(guide, np.float32).reshape(-1)
    out = {"n_hyp": np.zeros(cells, np.int32), "chosen": np.full(cells, -1, np.int32), "kept": np.zeros(cells, np.int32),
           "valid": np.zeros(cells, np.uint8), "center2": np.zeros(cells, np.int64), "limit": np.full(cells, -1, np.int64),
           "ambiguity": np.zeros(cells, np.float32)}
    for name in FLOATS:
        out[name] = np.full(cells, nodata, np.float32)
    hyp_start, first, count, hyps = [0], [], [], []
    for c in range(cells):
        b = int(start[c])
        s = [int(v) for v in sorted_q[b:int(start[c + 1])]]                      # Python integers from here
        n = len(s)
        runs = runs_of(s, gap_q)
        out["n_hyp"][c] = len(runs)
        first += [b + a for a, _ in runs]
        count += [nh for _, nh in runs]
        hyp_start.append(len(first))
        hyps.append([{"first": b + a, "count": nh, "min": s[a] / 65536, "max": s[a + nh - 1] / 65536,
                      "median": (s[a + (nh - 1) // 2] + s[a + nh // 2]) / 131072, "mean": sum(s[a:a + nh]) / (nh * 65536)}
                     for a, nh in runs])
        h = choose(s, runs, min_count, None if g is None else guide2_of(g[c]))
        if n:
            out["ambiguity"][c] = np.float32(float(n) / float(n))            # (none chosen: nothing is kept)
        if h < 0:
            continue
        a, nh = runs[h]
        run = s[a:a + nh]
        out["chosen"][c], out["kept"][c], out["valid"][c] = h, nh, 1
        S1, S2 = sum(run), sum(v * v for v in run)
        out["depth"][c] = np.float32(float(S1) / float(nh) * 2.0 ** -16)
        num = nh * S2 - S1 * S1
        assert num >= 0
        out["std"][c] = np.float32(math.sqrt(float(num) / (float(nh) * float(nh))) * 2.0 ** -16)     # float(int): one rounding
        out["min"][c] = np.float32(float(run[0]) * 2.0 ** -16)
        out["max"][c] = np.float32(float(run[-1]) * 2.0 ** -16)
        out["share"][c] = np.float32(float(nh) / float(n))
        out["center2"][c] = run[0] + run[-1]
        out["limit"][c] = run[-1] - run[0]
        out["ambiguity"][c] = np.float32(float(n - nh) / float(n))
    out = {name: v.reshape(shape) for name, v in out.items()}
    out.update(hyp_start=np.asarray(hyp_start, np.int64), hyp_first=np.asarray(first, np.int64), hyp_count=np.asarray(count, np.int32),
               hyps=hyps, gap_q=gap_q)
    return out
