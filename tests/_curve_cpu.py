"""Operating curves restated in numpy, twice and independently (include/bgnn_curve.h, training/operating_curve.py):

(a) ``brute_curve``   one boolean mask per threshold with the literal comparisons ``conf > t``, ``conf >= t``, ``conf < t`` on the
                      float32 planes, int64 ``np.rint`` sums: what a user would write per threshold
(b) ``numpy_block``   the confidence code of every cell and the histogram over it: the block the kernel fills

and the planes both are fed: random ones, and ones salted with every value the header singles out."""
import functools

import numpy as np

CAP = np.float32(32768.0)
SCALE = 65536.0
NAMES = ("seafloor", "feature", "noise")


def thresholds_for(n):
    """The tables of the tests: T = 1, 2, 101 (the default), 128 (the limit; it reaches below 0 and above 1)."""
    if n == 1:
        return np.array([0.5], np.float32)
    if n == 2:
        return np.array([0.25, 0.75], np.float32)
    if n == 101:
        return np.unique(np.linspace(0, 1, 101).astype(np.float32))
    t = np.linspace(-0.1, 1.1, n).astype(np.float32)
    assert (t[1:] > t[:-1]).all()
    return t


def counted(labels, pred):
    """The cells that count, their true and predicted class (clamped to 0, 1, 2, ">= 3")."""
    with np.errstate(invalid="ignore"):
        ok = (labels >= 0) & (pred >= 0) & np.isfinite(pred)
    row = np.minimum(np.where(ok, labels, 0), 3).astype(np.int64)
    col = np.minimum(np.trunc(np.where(ok, pred, 0).astype(np.float64)), 3.0).astype(np.int64)
    return ok, row, col


def fixed_point(v):
    return np.rint(v.astype(np.float64) * SCALE).astype(np.int64)


def residual_terms(ok, col, difference, correction):
    """has_base, res (the cell enters the per-code sums), q(|d|), q(|d - c|) with d - c formed in float32."""
    d = difference.astype(np.float32, copy=False)
    with np.errstate(invalid="ignore", over="ignore"):
        left = np.abs(d - correction.astype(np.float32, copy=False))
        mag = np.abs(d)
        has_base = ok & (mag < CAP)
        res = has_base & (col == 2) & (left < CAP)
    qb = np.where(has_base, fixed_point(np.where(has_base, mag, 0)), 0)
    qa = np.where(res, fixed_point(np.where(res, left, 0)), 0)
    return has_base, res, qb, qa


# ---- (b) the code / histogram form ---------------------------------------------------------------------------------------
def confidence_codes(thr, conf):
    """2 * #{k : t_k < c} + [c == t_k for some k]; 2T + 1 for NaN.  The count is the literal one, in chunks."""
    T = thr.size
    code = np.empty(conf.size, np.int64)
    with np.errstate(invalid="ignore"):
        for a in range(0, conf.size, 1 << 16):
            c = conf[a:a + (1 << 16), None]
            code[a:a + (1 << 16)] = 2 * (thr[None, :] < c).sum(axis=1) + (thr[None, :] == c).any(axis=1)
    code[np.isnan(conf)] = 2 * T + 1
    return code


def block_dtype(T):
    b = 2 * T + 2
    return np.dtype([("counts", "<i8", (b, 4, 4)), ("res_cells", "<i8", (b, 4)), ("abs_before", "<i8", (b, 4)),
                     ("abs_after", "<i8", (b, 4)), ("base_cells", "<i8", (4,)), ("base_abs", "<i8", (4,)), ("res_skipped", "<i8")])


def numpy_block(thr, labels, pred, conf, difference=None, correction=None):
    thr = np.asarray(thr, np.float32)
    labels, pred, conf = (np.asarray(p).reshape(-1) for p in (labels, pred, conf))
    T, B = thr.size, 2 * thr.size + 2
    blk = np.zeros((), block_dtype(T))
    ok, row, col = counted(labels, pred)
    code = confidence_codes(thr, conf.astype(np.float32, copy=False))
    blk["counts"] = np.bincount((code * 16 + row * 4 + col)[ok], minlength=B * 16).reshape(B, 4, 4)
    if difference is not None:
        has_base, res, qb, qa = residual_terms(ok, col, np.asarray(difference).reshape(-1), np.asarray(correction).reshape(-1))
        idx = (code * 4 + row)[res]
        for field, w in (("res_cells", np.ones(idx.size, np.int64)), ("abs_before", qb[res]), ("abs_after", qa[res])):
            acc = np.zeros(B * 4, np.int64)
            np.add.at(acc, idx, w)
            blk[field] = acc.reshape(B, 4)
        for j in range(4):
            mine = has_base & (row == j)
            blk["base_cells"][j], blk["base_abs"][j] = int(mine.sum()), int(qb[mine].sum())
        blk["res_skipped"] = int((ok & ~has_base).sum())
    return blk


def add_blocks(a, b):
    out = a.copy()
    for f in a.dtype.names:
        out[f] = a[f] + b[f]
    return out


# ---- (a) brute force ---------------------------------------------------------------------------------------------------
def _ratio(num, den):
    return num / den if den > 0 else 0


def brute_curve(thr, labels, pred, conf, difference=None, correction=None):
    """The dictionary of ``curve_from_block`` from one mask per threshold."""
    thr = np.asarray(thr, np.float32)
    labels, pred, conf = (np.asarray(p).reshape(-1) for p in (labels, pred, conf))
    conf = conf.astype(np.float32, copy=False)
    ok, row, col = counted(labels, pred)
    total = int(ok.sum())
    wrong = ok & (row != col)
    errors = int(wrong.sum())
    noise_support = int((ok & (row == 2)).sum())
    residual = difference is not None
    if residual:
        has_base, res, qb, qa = residual_terms(ok, col, np.asarray(difference).reshape(-1), np.asarray(correction).reshape(-1))
        n_base = int(has_base.sum())
    auto = {k: [] for k in ("cells", "true_noise", "on_seafloor", "on_feature", "precision", "recall", "f1", "share_of_valid")}
    review = {k: [] for k in ("cells", "share", "errors_caught", "errors_caught_share")}
    coverage = {k: [] for k in ("coverage", "accuracy")}
    mae_after, corrected = [], []
    per_class = {name: {"mae_after": [], "corrected_cells": []} for name in NAMES}
    for t in thr:
        with np.errstate(invalid="ignore"):
            gt, ge, lt = conf > t, conf >= t, conf < t
        applied = ok & (col == 2) & gt
        cells, true_noise = int(applied.sum()), int((applied & (row == 2)).sum())
        precision, recall = _ratio(true_noise, cells), _ratio(true_noise, noise_support)
        f1 = 2 * precision * recall / (precision + recall) if (precision + recall) > 0 else 0
        auto["cells"].append(cells); auto["true_noise"].append(true_noise)
        auto["on_seafloor"].append(int((applied & (row == 0)).sum())); auto["on_feature"].append(int((applied & (row == 1)).sum()))
        auto["precision"].append(float(precision)); auto["recall"].append(float(recall)); auto["f1"].append(float(f1))
        auto["share_of_valid"].append(float(_ratio(cells, total)))
        r_cells, caught = int((ok & lt).sum()), int((wrong & lt).sum())
        review["cells"].append(r_cells); review["share"].append(float(_ratio(r_cells, total)))
        review["errors_caught"].append(caught); review["errors_caught_share"].append(float(_ratio(caught, errors)))
        covered = int((ok & ge).sum())
        coverage["coverage"].append(float(_ratio(covered, total)))
        coverage["accuracy"].append(float(_ratio(int((ok & ge & (row == col)).sum()), covered)))
        if residual:
            now = np.where(res & gt, qa, qb)                    # the residual of every cell once the set is corrected
            mae_after.append(float(_ratio(int(now[has_base].sum()), n_base) / SCALE))
            corrected.append(int((res & gt).sum()))
            for j, name in enumerate(NAMES):
                mine = has_base & (row == j)
                per_class[name]["mae_after"].append(float(_ratio(int(now[mine].sum()), int(mine.sum())) / SCALE))
                per_class[name]["corrected_cells"].append(int((res & gt & (row == j)).sum()))
    confusion = np.bincount((row * 4 + col)[ok], minlength=16).reshape(4, 4)
    out = {
        "thresholds": [float(t) for t in thr],
        "total": total,
        "confusion_matrix": [[int(v) for v in r] for r in confusion],
        "support": {name: int((ok & (row == j)).sum()) for j, name in enumerate(NAMES)},
        "nan_confidence_cells": int((ok & np.isnan(conf)).sum()),
        "auto_correct": auto, "review": review, "coverage": coverage,
    }
    if residual:
        for j, name in enumerate(NAMES):
            mine = has_base & (row == j)
            per_class[name] = {"cells": int(mine.sum()), "mae_before": float(_ratio(int(qb[mine].sum()), int(mine.sum())) / SCALE),
                               **per_class[name]}
        out["residual"] = {"cells": n_base, "mae_before": float(_ratio(int(qb[has_base].sum()), n_base) / SCALE),
                           "mae_after": mae_after, "corrected_cells": corrected, "per_class": per_class,
                           "skipped": int((ok & ~has_base).sum())}
    return out


def assert_curves_equal(got, want, path=""):
    """Exact equality of two curve dictionaries, types of the numbers included."""
    assert type(got) is type(want), (path, type(got), type(want))
    if isinstance(want, dict):
        assert sorted(got) == sorted(want), (path, sorted(got), sorted(want))
        for k in want:
            assert_curves_equal(got[k], want[k], f"{path}/{k}")
    elif isinstance(want, list):
        assert len(got) == len(want), path
        for i, (g, w) in enumerate(zip(got, want)):
            assert_curves_equal(g, w, f"{path}[{i}]")
    else:
        assert got == want, (path, got, want)


# ---- planes ------------------------------------------------------------------------------------------------------------
def random_planes(n, seed, noise_share=0.3):
    """Plain planes: labels 0 / 1 / 2 with some -1, mostly right predictions with some NaN, confidences in [0, 1)."""
    rng = np.random.default_rng(seed)
    labels = rng.choice([-1, 0, 1, 2], n, p=[.1, .6 - noise_share / 2, .1, .2 + noise_share / 2]).astype(np.int32)
    pred = np.where(rng.random(n) < 0.8, np.maximum(labels, 0), rng.choice([0, 1, 2], n)).astype(np.float32)
    pred[rng.random(n) < 0.03] = np.nan
    conf = rng.random(n).astype(np.float32)
    diff = (rng.standard_normal(n) * 0.4).astype(np.float32)
    diff[labels < 0] = np.nan
    corr = (diff * rng.random(n) + rng.standard_normal(n) * 0.05).astype(np.float32)
    corr[np.isnan(corr)] = 0.0
    return labels, pred, conf, diff, corr


def adversarial_planes(thr, n, seed):
    """Planes salted with what the header singles out.  Confidences: exactly t_k and its two float32 neighbours, NaN, +-inf,
    -0.0, negative, above 1.  Labels -1, 0, 1, 2, 3, 7; predictions NaN, -1, 0.0, 1.0, 2.0, 2.9, 3.0, 1e9.  Residual planes: NaN,
    +-inf, |d| = 32767.99 and 32768, d - c that rounds in float32 (1 - 2^-25, 0.1 - 0.3), |d - c| past the cap with |d| inside it,
    fixed-point ties (0.5, 1.5, 2.5 / 65536), corrections of exactly 0 and exactly d."""
    rng = np.random.default_rng(seed)
    thr = np.asarray(thr, np.float32)
    f = np.float32
    near = np.concatenate([thr, np.nextafter(thr, f(np.inf)), np.nextafter(thr, f(-np.inf))]).astype(f)
    odd = np.array([np.nan, np.inf, -np.inf, -0.0, 0.0, -0.3, 1.7, 1.0, 3.0e38, -3.0e38], f)
    labels = rng.choice(np.array([-1, 0, 1, 2, 3, 7], np.int32), n, p=[.1, .3, .1, .4, .05, .05]).astype(np.int32)
    pred = rng.choice(np.array([np.nan, -1, 0.0, 1.0, 2.0, 2.9, 3.0, 1e9], f), n, p=[.05, .05, .15, .1, .35, .2, .05, .05]).astype(f)
    conf = rng.random(n).astype(f)
    salt = rng.random(n)
    conf[salt < 0.3] = rng.choice(near, int((salt < 0.3).sum()))
    conf[salt > 0.8] = rng.choice(odd, int((salt > 0.8).sum()))
    diff = (rng.standard_normal(n) * 0.4).astype(f)
    corr = (diff * rng.random(n)).astype(f)
    pairs = np.array([(np.nan, 0.1), (0.1, np.nan), (np.inf, 0.1), (-np.inf, 0.1), (0.1, np.inf), (0.1, -np.inf), (np.inf, np.inf),
                      (32767.99, 0.5), (-32767.99, -0.5), (32768.0, 0.5), (-32768.0, 0.0), (32767.0, -10.0), (-32767.0, 10.0),
                      (3.0e38, -3.0e38), (1.0, 2.0 ** -25), (0.1, 0.3), (1.0e-3, 1.0e-3), (0.25, 0.0), (-0.0, 0.0),
                      (0.5 / 65536, 0.0), (1.5 / 65536, 0.0), (2.5 / 65536, 0.0), (1.0, 1.0 - 0.5 / 65536), (1.0, 1.0 - 1.5 / 65536),
                      (2.0 ** -30, 0.0), (100.0, 99.75)], f)
    salt = rng.random(n) < 0.4
    pick = rng.integers(0, len(pairs), int(salt.sum()))
    diff[salt], corr[salt] = pairs[pick, 0], pairs[pick, 1]
    return labels, pred, conf, diff, corr


def one_value_planes(n, value=0.5):
    """Every cell on one confidence, one label and one prediction: the worst contention on one histogram entry."""
    labels = np.full(n, 2, np.int32)
    pred = np.full(n, 2.0, np.float32)
    conf = np.full(n, value, np.float32)
    diff = ((np.arange(n) % 977).astype(np.float32) - 488.0) / np.float32(64.0)
    corr = (diff * np.float32(0.75)).astype(np.float32)
    return labels, pred, conf, diff, corr


@functools.lru_cache(maxsize=None)
def adversarial_case(n_thresholds, cells):
    """One adversarial case and its block, computed once per (T, cells) and shared; the arrays are read-only."""
    thr = thresholds_for(n_thresholds)
    planes = adversarial_planes(thr, cells, seed=1000 * n_thresholds + cells % 997)
    blk = numpy_block(thr, *planes)
    for p in planes:
        p.setflags(write=False)
    return thr, planes, blk
