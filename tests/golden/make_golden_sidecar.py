#!/usr/bin/env python3
"""Golden vectors for the VR BAG sidecar raster (reference data/vr_bag.py, SidecarBuilder.add_refinement_results), produced by
the REFERENCE's own class in the build container:

    python tests/golden/make_golden_sidecar.py

``data/vr_bag.py`` is loaded as a submodule of an empty stand-in package (the reference's ``data/__init__`` pulls in GDAL / PyG
modules).  Its ``SidecarBuilder.__init__`` reads the raster's georeferencing with GDAL; here the object is made with
``object.__new__`` and given the attributes that constructor would have set.  The fixture (``sidecar/sidecar_reference.npz``:
a subdirectory, the top level of tests/golden is globbed for graph goldens) holds inputs and the reference's outputs only.

Every assert below looks at the reference's output alone: the cases must cover rounding ties, overlaps, the sticky mask and
clipping whatever implementation is later tested against them.
"""
import importlib
import os
import sys
import types

sys.dont_write_bytecode = True
import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
pkg = types.ModuleType("refdata")
pkg.__path__ = ["/root/reference/data"]
sys.modules["refdata"] = pkg
vr = importlib.import_module("refdata.vr_bag")


class Handler:
    def __init__(self, base_shape):
        self.base_shape = base_shape
        self.path = None


def ref_builder(base_shape, shape, gt):
    sb = object.__new__(vr.SidecarBuilder)
    sb.handler = Handler(base_shape)
    sb.shape = shape
    sb.geotransform = gt
    sb.crs = ""
    sb.resolution = abs(gt[1])
    sb.bounds = (gt[0], gt[3] + shape[0] * gt[5], gt[0] + shape[1] * gt[1], gt[3])
    sb.classification = np.full(shape, np.nan, np.float32)
    sb.confidence = np.full(shape, np.nan, np.float32)
    sb.correction = np.full(shape, np.nan, np.float32)
    sb.valid_mask = np.zeros(shape, np.float32)
    return sb


def planes_of(sb):
    return np.stack([sb.classification, sb.confidence, sb.correction, sb.valid_mask])


def make_grid(rng, spec, start):
    br, bc, rows, cols, rx, ry, sx, sy, bad = spec
    depth = (-30 + 5 * rng.standard_normal((rows, cols))).astype(np.float32)
    hole = rng.random((rows, cols)) < bad
    depth[hole] = np.where(rng.random(int(hole.sum())) < 0.5, np.float32(1.0e6), np.float32(np.nan))
    g = vr.RefinementGrid(base_row=br, base_col=bc, depth=depth, uncertainty=np.zeros_like(depth), resolution=(rx, ry),
                          dimensions=(rows, cols), sw_corner=(sx, sy), start_index=start)
    res = (rng.integers(0, 3, (rows, cols)).astype(np.float32), rng.random((rows, cols)).astype(np.float32),
           (0.2 * rng.standard_normal((rows, cols))).astype(np.float32))
    return g, res


def case(out, name, base_shape, shape, gt, specs, seed):
    rng = np.random.default_rng(seed)
    sb = ref_builder(base_shape, shape, gt)
    grids, singles, start = [], [], 0
    for spec in specs:
        g, res = make_grid(rng, spec, start)
        start += g.depth.size
        grids.append((g, res))
        sb.add_refinement_results(g, *res)
        one = ref_builder(base_shape, shape, gt)          # the same grid alone: which pixels it paints, and their mask
        one.add_refinement_results(g, *res)
        singles.append(planes_of(one))
    out[f"{name}_base_shape"] = np.array(base_shape, np.int64)
    out[f"{name}_shape"] = np.array(shape, np.int64)
    out[f"{name}_geotransform"] = np.array(gt, np.float64)
    out[f"{name}_grids"] = np.array([s[:8] for s in specs], np.float64)   # base_row, base_col, rows, cols, res_x, res_y, sw_x, sw_y
    out[f"{name}_depth"] = np.concatenate([g.depth.reshape(-1) for g, _ in grids])
    for k, nm in enumerate(("classification", "confidence", "correction")):
        out[f"{name}_{nm}"] = np.concatenate([r[k].reshape(-1) for _, r in grids])
    out[f"{name}_planes"] = planes_of(sb)
    return sb, grids, singles


MAIN_SPECS = [(0, 0, 10, 12, 1.0, 1.0, .5, .5, .1), (0, 1, 20, 20, 1.5 * .4, 1.5 * .4, .2, .2, .1), (0, 1, 30, 30, .2, .2, 1.0, 1.0, .6),
              (1, 3, 12, 9, 2.0, 1.0, 3.0, 0.0, .1), (2, 0, 8, 8, 4.0, 4.0, -6.0, 10.0, .1), (0, 2, 6, 6, 2.0, 2.0, 0.0, -9.0, .1),
              (2, 3, 5, 5, 1.0, 1.0, 200.0, 200.0, .1), (1, 1, 16, 16, 1.0, 1.0, .1, .3, .1), (1, 2, 16, 16, 1.0, 1.0, -7.9, .3, .1)]
MAIN_SCALES = [2, 2, 1, 5, 10, 5, 2, 2, 2]      # 1.0 / 0.4 = 2.5 -> 2 and (1.5 * 0.4) / 0.4 = 1.5 -> 2 (half to even; the literal 0.6 / 0.4 is 1.4999999999999998); 0.2 / 0.4 = 0.5 -> 0 -> 1


def block_side(painted):
    rows = np.nonzero(painted.any(1))[0]; cols = np.nonzero(painted.any(0))[0]
    return rows, cols


def check_main(sb, grids, singles):
    H, W = sb.shape
    cover = np.stack([~np.isnan(s[0]) for s in singles])                  # [grid, H, W]
    n_cover = cover.sum(0)
    idx = np.arange(len(singles))[:, None, None]
    first = np.where(cover, idx, 99).min(0); last = np.where(cover, idx, -1).max(0)
    # the later grid wins, bit for bit
    final = planes_of(sb)
    for i, s in enumerate(singles):
        own = last == i
        assert np.array_equal(final[:3][:, own].view(np.uint32), s[:3][:, own].view(np.uint32))
    multi = n_cover >= 2
    assert int((multi & (first != last)).sum()) >= 500, int(multi.sum())
    assert (multi & (last == 2) & (first == 1)).any(), "two grids of one base cell must overlap"
    assert (multi & (last == 8) & (first == 7)).any(), "grids of neighbouring base cells must overlap"
    # sticky mask: the final owner's cell is invalid, an earlier grid's valid cell had set the mask
    owner_valid = np.zeros((H, W), bool)
    for i, s in enumerate(singles):
        owner_valid |= (last == i) & (s[3] == 1)
    sticky = (n_cover >= 1) & ~owner_valid & (final[3] == 1)
    assert int(sticky.sum()) >= 100, int(sticky.sum())
    # scales (ties to even, the lift to 1, res_x alone) and clipping at each edge, from what each grid painted alone
    dropped = {"north": 0, "south": 0, "west": 0, "east": 0}
    for i, ((g, _), s, sc) in enumerate(zip(grids, singles, MAIN_SCALES)):
        rows, cols = block_side(cover[i])
        full_r, full_c = g.dimensions[0] * sc, g.dimensions[1] * sc
        if i == 6:
            assert rows.size == 0, "one grid lies entirely outside"
            continue
        assert rows.size <= full_r and cols.size <= full_c
        assert cover[i].sum() == rows.size * cols.size
        if rows.size == full_r and cols.size == full_c:          # unclipped: the block's size is cells * scale
            continue
        if rows.size < full_r:
            assert rows[0] == 0 or rows[-1] == H - 1
            dropped["north" if rows[0] == 0 else "south"] += (full_r - rows.size) * cols.size
        if cols.size < full_c:
            assert cols[0] == 0 or cols[-1] == W - 1
            dropped["west" if cols[0] == 0 else "east"] += (full_c - cols.size) * rows.size
    assert all(v > 0 for v in dropped.values()), dropped
    # the tie and lift cases show their scale in a side that is not clipped
    for i in (0, 7):
        rows, cols = block_side(cover[i])
        assert rows.size == grids[i][0].dimensions[0] * MAIN_SCALES[i] and cols.size == grids[i][0].dimensions[1] * MAIN_SCALES[i], i
    for i in (1, 2):
        assert block_side(cover[i])[1].size == grids[i][0].dimensions[1] * MAIN_SCALES[i], i
    assert grids[3][0].resolution[0] != grids[3][0].resolution[1]
    return int((multi & (first != last)).sum()), int(sticky.sum()), dropped


def placement_records(out, n=2400, seed=17):
    """Single-cell grids, each painted by the reference on a fresh 64 x 64 raster of its own.  Every value lies on a binary grid
    (multiples of 1/32), so the arithmetic before the rounding is exact and a fraction of .5 chosen here IS a tie there."""
    rng = np.random.default_rng(seed)
    H = W = 64
    rec_in = np.zeros((n, 12), np.float64); rec_out = np.zeros((n, 3), np.int64)
    ties = np.zeros(3, np.int64)
    for k in range(n):
        p = float(rng.choice([0.25, 0.5, 1.0, 2.0]))
        gt = (float(rng.integers(-4000, 4000)) * 0.125, p, 0.0, float(rng.integers(-4000, 4000)) * 0.125, 0.0, -p)
        base_shape = (int(rng.choice([1, 2, 4])), int(rng.choice([1, 2, 4])))
        br, bc = int(rng.integers(0, base_shape[0])), int(rng.integers(0, base_shape[1]))
        fr, fc, fs = (float(v) for v in rng.choice([0.0, 0.25, 0.5, 0.75], 3))
        row, col, ks = int(rng.integers(8, 40)), int(rng.integers(8, 40)), int(rng.integers(0, 7))
        res_x = max(ks + fs, 0.25) * p
        fs = fs if ks + fs >= 0.25 else 0.25
        res_y = float(rng.integers(1, 64)) * 0.125
        cell_w, cell_h = W * p / base_shape[1], H * p / base_shape[0]
        sw_x = (col + fc) * p - bc * cell_w
        top = gt[3] - (row + fr) * p
        sw_y = top - res_y - ((gt[3] - H * p) + br * cell_h)
        vals = np.array([res_x, res_y, sw_x, sw_y])
        assert np.array_equal(vals.astype(np.float32).astype(np.float64), vals), "metadata values must be exact in float32"
        ties += [fr == 0.5, fc == 0.5, fs == 0.5]
        sb = ref_builder(base_shape, (H, W), gt)
        g = vr.RefinementGrid(base_row=br, base_col=bc, depth=np.full((1, 1), -10.0, np.float32), uncertainty=np.zeros((1, 1), np.float32),
                              resolution=(res_x, res_y), dimensions=(1, 1), sw_corner=(sw_x, sw_y), start_index=0)
        sb.add_refinement_results(g, np.ones((1, 1), np.float32), np.ones((1, 1), np.float32), np.ones((1, 1), np.float32))
        rows, cols = block_side(~np.isnan(sb.classification))
        assert rows.size == cols.size >= 1 and (~np.isnan(sb.classification)).sum() == rows.size ** 2
        assert rows[0] > 0 and cols[0] > 0 and rows[-1] < H - 1 and cols[-1] < W - 1, "margins: nothing may be clipped"
        rec_in[k] = [gt[0], gt[1], gt[3], gt[5], base_shape[0], base_shape[1], br, bc, res_x, res_y, sw_x, sw_y]
        rec_out[k] = [rows[0], cols[0], rows.size]
    assert (ties >= 50).all(), ties
    out["placement_in"] = rec_in          # gt0, gt1, gt3, gt5, base_rows, base_cols, base_row, base_col, res_x, res_y, sw_x, sw_y
    out["placement_out"] = rec_out        # top-left painted pixel (row, col), edge of the painted block
    return ties


def main():
    out = {}
    sb, grids, singles = case(out, "main", (3, 4), (120, 200), (500.0, 0.4, 0.0, 9048.0, 0.0, -0.4), MAIN_SPECS, 3)
    print("main: overwritten pixels, sticky pixels, dropped:", *check_main(sb, grids, singles))
    # a single-resolution BAG as one grid: base_shape is the grid's shape (SRBagHandler), raster at half the cell size
    sr, g_sr, s_sr = case(out, "sr", (40, 50), (80, 100), (0.0, 0.5, 0.0, 40.0, 0.0, -0.5), [(0, 0, 40, 50, 1.0, 1.0, 0.0, 0.0, .2)], 5)
    assert (~np.isnan(sr.classification)).sum() > 0 and sr.valid_mask.sum() > 0
    print("placement ties (row, col, scale):", placement_records(out))
    os.makedirs(os.path.join(HERE, "sidecar"), exist_ok=True)
    path = os.path.join(HERE, "sidecar", "sidecar_reference.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes,", len(out), "arrays")


if __name__ == "__main__":
    main()
