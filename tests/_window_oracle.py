"""A float64 reference for tiles too large for the whole-tile CPU oracle: the oracle run on small windows of the tile.

The eval-mode forward is local.  A valid cell's node features reach 3 cells (the 5 x 5 masked mean that fills invalid cells
reaches 2, ``np.gradient`` / the Laplacian of the filled grid one more, the 3 x 3 valid count of the curvature fits inside);
an edge attribute reaches one stencil offset; every conv layer reaches one hop (1 cell on the 4- / 8-connected stencils, 2 on
``16-dilated``); eval-mode BatchNorm, the heads and the ``local_std`` de-normalisation are pointwise.  So the float64 oracle on
a crop equals the whole-tile float64 oracle on every crop cell at least ``R = 3 + layers x hop`` cells from each crop edge that
is not also a tile edge -- where the crop's edge IS the tile's, the boundary rules (``np.gradient``'s one-sided differences,
``laplace``'s reflect mode, zero-padded box sums) are the same in both.  GCN's degree normalisation reaches one cell further
and training mode (batch statistics) is not local at all: neither is covered.

The equality holds up to the oracle's own float32 feature storage (``uniform_filter``'s running float64 sums round differently
in a crop, so a feature can land one float32 ulp away): tests/test_oracle_window.py measures that residue against the
whole-tile oracle and pins it below a tenth of float32 arithmetic's own distance to float64.
"""
import numpy as np
import torch

from oracle import gat_cpu, graph_cpu

HOP = {"4-connected": 1, "8-connected": 1, "16-dilated": 2}
FEATURE_REACH = 3
NORM_FLOOR = np.float32(0.01)                      # config/constants.py: correction = normalised x max(local_std, 0.01)
KEYS = ("class_logits", "class_probs", "predicted_class", "confidence", "correction", "hidden")


def reach(num_layers, connectivity):
    """R: how far (in cells) a cell's eval-mode outputs look."""
    return FEATURE_REACH + int(num_layers) * HOP[connectivity]


def trusted(window, tile_shape, R):
    """Boolean [h, w] mask of the cells of ``window`` = (row, col, h, w) whose windowed outputs equal the whole tile's: at
    least ``R`` cells from every window edge that is not an edge of the ``tile_shape`` tile."""
    r0, c0, h, w = (int(v) for v in window)
    H, W = (int(v) for v in tile_shape)
    if not (0 <= r0 and 0 <= c0 and h > 0 and w > 0 and r0 + h <= H and c0 + w <= W):
        raise ValueError(f"window {window} does not lie inside a {H} x {W} tile")
    rows = np.arange(h); cols = np.arange(w)
    ok_r = ((rows >= R) | (r0 == 0)) & ((rows < h - R) | (r0 + h == H))
    ok_c = ((cols >= R) | (c0 == 0)) & ((cols < w - R) | (c0 + w == W))
    return ok_r[:, None] & ok_c[None, :]


def window_forward(depth, valid, uncertainty, resolution, sd, connectivity, window, denormalise=True):
    """The oracle on one crop: (graph, float32 outputs, float64 outputs), every node of the crop, nothing selected yet.
    ``denormalise``: correction x max(local_std, 0.01) as ``process_tile`` returns it (the tile routes); False leaves the
    head's normalised output (``predict``)."""
    r0, c0, h, w = (int(v) for v in window)
    sl = (slice(r0, r0 + h), slice(c0, c0 + w))
    og = graph_cpu.build_graph(np.ascontiguousarray(depth[sl]), np.ascontiguousarray(valid[sl]),
                               None if uncertainty is None else np.ascontiguousarray(uncertainty[sl]),
                               resolution, connectivity=connectivity)
    if og.num_nodes == 0:
        return og, None, None
    o32 = gat_cpu.forward(sd, og.x, og.edge_index, og.edge_attr)
    o64 = gat_cpu.forward(sd, og.x, og.edge_index, og.edge_attr, dtype=torch.float64)
    run = (og, o32, o64)
    return denormalised([run])[0] if denormalise else run


def denormalised(runs):
    """``window_forward(..., denormalise=False)`` results with ``process_tile``'s de-normalisation applied: what
    ``denormalise=True`` returns, without running the forward again."""
    out = []
    for og, o32, o64 in runs:
        if o64 is not None and "correction" in o64:
            ls = np.maximum(og.local_std, NORM_FLOOR)
            o32 = dict(o32, correction=o32["correction"] * torch.from_numpy(ls))
            o64 = dict(o64, correction=o64["correction"] * torch.from_numpy(ls.astype(np.float64)))
        out.append((og, o32, o64))
    return out


def gather(runs, windows, tile_shape, R):
    """Select the trusted valid cells of every window's run (``window_forward`` results, in ``windows``' order) and
    concatenate them: (ref32, ref64, rows, cols), rows / cols in tile coordinates."""
    parts32 = {k: [] for k in KEYS}; parts64 = {k: [] for k in KEYS}
    rr, cc = [], []
    for (og, o32, o64), win in zip(runs, windows):
        if o64 is None:
            continue
        keep = torch.from_numpy(trusted(win, tile_shape, R)[og.valid_rows, og.valid_cols])
        for parts, o in ((parts32, o32), (parts64, o64)):
            for k in KEYS:
                if k in o:
                    parts[k].append(o[k][keep])
        rr.append(og.valid_rows[keep.numpy()] + int(win[0])); cc.append(og.valid_cols[keep.numpy()] + int(win[1]))
    cat = lambda parts: {k: torch.cat(v) for k, v in parts.items() if v}
    rows = np.concatenate(rr) if rr else np.zeros(0, np.int64)
    cols = np.concatenate(cc) if cc else np.zeros(0, np.int64)
    return cat(parts32), cat(parts64), rows, cols


def windowed_reference(depth, valid, uncertainty, resolution, sd, connectivity, windows, margin=None, denormalise=True):
    """The float32 and float64 oracles of a tile on the trusted valid cells of ``windows`` (a list of (row, col, h, w) inside
    the tile), concatenated in the windows' order and row-major inside each: two dicts shaped like ``gat_cpu.predict``'s
    (class_logits, class_probs, predicted_class, confidence, correction, hidden) and the cells' tile coordinates.  The dicts go
    straight into ``_conditioning.float64_bound`` / ``distances``.  ``margin``: the distance kept from interior window edges
    (default ``reach(layers, connectivity)``; anything smaller is only for showing that the default is needed)."""
    R = reach(gat_cpu.num_layers_of(sd), connectivity) if margin is None else int(margin)
    runs = [window_forward(depth, valid, uncertainty, resolution, sd, connectivity, w, denormalise) for w in windows]
    return gather(runs, windows, depth.shape, R)


def clip_window(row, col, h, w, tile_shape):
    """(row, col, h, w) moved so that it lies inside the tile (a helper for placing windows around a feature)."""
    H, W = tile_shape
    h, w = min(h, H), min(w, W)
    return (int(min(max(row, 0), H - h)), int(min(max(col, 0), W - w)), int(h), int(w))
