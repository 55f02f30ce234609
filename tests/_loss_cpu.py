"""Float64 numpy restatement of the multi-task training loss (include/bgnn_loss.h, INTEGRATION.md "Training loss"): the six
values, the gradients with respect to class_logits / confidence / correction, and the integer counts.  tests/test_host_loss.py
pins it against the reference's float64 run (tests/golden/loss/*.npz); tests/test_gpu_loss.py uses it as the yardstick at the
sizes the fixtures do not reach.

``loss`` returns the exact float64 terms.  The reference forms its two count-derived terms (feature_preservation, shoal_safety)
in float32 whatever the dtype of its inputs -- one division of exactly represented integers, i.e. float32(exact ratio) -- and
multiplies them by their weights in float32 before they enter its total; ``as_reference`` applies those roundings, and is what a
float64 run of the reference is compared with.
"""
import numpy as np

TERMS = ("classification", "correction", "confidence", "feature_preservation", "shoal_safety", "total")
IGNORE = -100
BCE_FLOOR = float(np.float32(1e-12))        # torch's clamp constant as torch holds it
DEFAULTS = dict(class_weights=None, label_smoothing=0.0, delta=1.0, feature_class=1, feature_noise_class=2, seafloor_class=0,
                shoal_noise_class=2, penalty_weight=2.0, shoal_penalty=3.0, deep_penalty=1.0,
                term_weights=(1.0, 0.5, 0.2, 0.3, 0.5))


def config(**kw):
    c = dict(DEFAULTS)
    c.update(kw)
    return c


def _prep(inp, cfg):
    x = np.asarray(inp["class_logits"], np.float64)
    n, c = x.shape
    y = np.asarray(inp["class_labels"], np.int64).reshape(-1)
    q = np.asarray(inp["predicted_class"], np.int64).reshape(-1)
    w = np.ones(c) if cfg["class_weights"] is None else np.asarray(cfg["class_weights"], np.float64)
    m = x.max(axis=1, keepdims=True) if n else np.zeros((0, 1))
    lp = x - (m + np.log(np.exp(x - m).sum(axis=1, keepdims=True)))
    valid = (y >= 0) & (y < c)
    corr, tgt = inp.get("correction"), inp.get("correction_targets")
    has_corr = corr is not None and tgt is not None
    sel = np.zeros(n, bool)
    if has_corr:
        sel = np.ones(n, bool) if inp.get("noise_mask") is None else np.asarray(inp["noise_mask"]).astype(bool).reshape(-1)
    return x, n, c, y, q, w, lp, valid, has_corr, sel


def counts(inp, cfg):
    """The integers of bgnn_loss_forward's ``counts``: confusion [C, C] and the named ones."""
    x, n, c, y, q, w, lp, valid, has_corr, sel = _prep(inp, cfg)
    conf = np.zeros((c, c), np.int64)
    both = valid & (q >= 0) & (q < c)
    np.add.at(conf, (y[both], q[both]), 1)
    fp = (y == cfg["seafloor_class"]) & (q == cfg["shoal_noise_class"])
    tgt = inp.get("correction_targets")
    shoal = fp & (np.asarray(tgt).reshape(-1) < 0) if tgt is not None else np.zeros(n, bool)
    deep = fp & ~shoal if tgt is not None else np.zeros(n, bool)
    return dict(confusion=conf, n_masked=int(sel.sum()), false_positives=int(fp.sum()), shoal_false_positives=int(shoal.sum()),
                deep_false_positives=int(deep.sum()), n_ignored=int((y == IGNORE).sum()), n_invalid=int((~valid & (y != IGNORE)).sum()),
                feature_as_noise=int(((y == cfg["feature_class"]) & (q == cfg["feature_noise_class"])).sum()))


def loss(inp, cfg):
    """The six exact float64 terms."""
    x, n, c, y, q, w, lp, valid, has_corr, sel = _prep(inp, cfg)
    k = counts(inp, cfg)
    eps = float(cfg["label_smoothing"])
    t = {}
    with np.errstate(all="ignore"):
        yk = y[valid]
        W = w[yk].sum()
        nll = -(w[yk] * lp[valid, yk]).sum()
        smooth = -(lp[valid] * w[None, :]).sum()
        t["classification"] = np.float64(np.nan) if k["n_invalid"] else ((1 - eps) * nll + (eps / c) * smooth) / np.float64(W)
        if has_corr and sel.any():
            d = np.asarray(inp["correction"], np.float64).reshape(-1)[sel] - np.asarray(inp["correction_targets"], np.float64).reshape(-1)[sel]
            delta = float(cfg["delta"])
            t["correction"] = np.where(np.abs(d) < delta, 0.5 * d * d, delta * (np.abs(d) - 0.5 * delta)).sum() / sel.sum()
        else:
            t["correction"] = np.float64(0.0)
        p = np.asarray(inp["confidence"], np.float64).reshape(-1)
        hit = q == y
        l1, l0 = np.maximum(np.log(p), -100.0), np.maximum(np.log1p(-p), -100.0)
        t["confidence"] = -np.where(hit, l1, l0).sum() / np.float64(n)
        t["feature_preservation"] = cfg["penalty_weight"] * np.float64(k["feature_as_noise"]) / np.float64(n)
        if k["false_positives"] and inp.get("correction_targets") is not None:
            t["shoal_safety"] = (cfg["shoal_penalty"] * k["shoal_false_positives"] + cfg["deep_penalty"] * k["deep_false_positives"]) / np.float64(k["false_positives"])
        else:
            t["shoal_safety"] = np.float64(0.0)
        t["total"] = sum(wt * t[name] for wt, name in zip(cfg["term_weights"], TERMS[:5]))
    return {name: np.float64(v) for name, v in t.items()}


def as_reference(terms, cfg):
    """The terms as the reference returns them: the two count-derived ones rounded to float32, and their weighted share of the
    total formed in float32 (a Python float times a float32 tensor)."""
    t = dict(terms)
    total = np.float64(0.0)
    for wt, name in zip(cfg["term_weights"], TERMS[:5]):
        if name in ("feature_preservation", "shoal_safety"):
            t[name] = np.float64(np.float32(t[name]))
            total = total + np.float64(np.float32(wt) * np.float32(t[name]))
        else:
            total = total + wt * t[name]
    t["total"] = np.float64(total)
    return t


def grads(inp, cfg, upstream=None):
    """d(sum_k upstream_k term_k) / d(class_logits, confidence, correction), float64; ``upstream`` = (classification, confidence,
    correction), by default the three term weights (the gradient of ``total``).  correction: None when the input is absent."""
    x, n, c, y, q, w, lp, valid, has_corr, sel = _prep(inp, cfg)
    tw = cfg["term_weights"]
    u_cls, u_conf, u_corr = (tw[0], tw[2], tw[1]) if upstream is None else upstream
    eps = float(cfg["label_smoothing"])
    with np.errstate(all="ignore"):
        p = np.exp(lp)
        W = w[y[valid]].sum()
        onehot = np.zeros((n, c))
        onehot[valid, y[valid]] = 1.0
        wy = np.where(valid, w[np.where(valid, y, 0)], 0.0)[:, None]
        g = ((1 - eps) * wy * (p - onehot) + (eps / c) * (p * w.sum() - w[None, :])) / np.float64(W)
        g = u_cls * g
        g[y == IGNORE] = 0.0
        g[~valid & (y != IGNORE)] = np.nan
        pc = np.asarray(inp["confidence"], np.float64).reshape(-1)
        gc = u_conf * ((pc - (q == y)) / np.maximum((1 - pc) * pc, BCE_FLOOR) / np.float64(n))
        gr = None
        if inp.get("correction") is not None:
            gr = np.zeros(n)
            if has_corr and sel.any():
                d = np.asarray(inp["correction"], np.float64).reshape(-1) - np.asarray(inp["correction_targets"], np.float64).reshape(-1)
                delta = float(cfg["delta"])
                h = np.where(np.abs(d) < delta, d, delta * np.sign(d))
                gr = np.where(sel, u_corr * (h / sel.sum()), 0.0)
    return dict(class_logits=g, confidence=gc, correction=gr)


def load_fixture(path):
    """(inputs, config, npz) of one tests/golden/loss fixture."""
    z = np.load(path, allow_pickle=False)
    inp = dict(class_logits=z["class_logits"], confidence=z["confidence"], predicted_class=z["predicted_class"].astype(np.int64),
               class_labels=z["class_labels"].astype(np.int64))
    for k in ("correction", "correction_targets", "noise_mask"):
        if k in z.files:
            inp[k] = z[k]
    cfg = config(label_smoothing=float(z["label_smoothing"]), delta=float(z["delta"]),
                 class_weights=z["class_weights"] if "class_weights" in z.files else None)
    return inp, cfg, z
