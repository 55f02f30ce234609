"""The reference's plan for native-resolution ground truth (docs/TRAINING_PLAN.md step 1.2, ``compute_ground_truth_native``) restated
on the host, in its own iteration order, and the VR BAG pairs the tests feed it.  No GPU.

``native_truth_cpu`` is the plan's loop, statement for statement: the dictionary of the noisy file's grids, the walk over the clean
file's grids, ``noisy.depth - clean.depth``, the two valid masks, the labels, the magnitude list with ``np.mean`` / ``np.max`` /
``np.median`` on its float64 copy.  Its per-cell output is laid out flat, grid after grid in the NOISY file's iteration order: a grid
the loop skips (no twin, other dimensions) keeps ``labels = -1``, ``difference = NaN``, ``mask = 0``; noisy depth and uncertainty are
copied for every grid."""
import math

import numpy as np

from bathymetric_gnn_amd import synthetic
from bathymetric_gnn_amd.data.vr_bag import VARRES_METADATA_DTYPE, VARRES_REFINEMENT_DTYPE, VRBagHandler

CLASS_SEAFLOOR, CLASS_NOISE = 0, 2
NODATA = np.float32(1.0e6)


def native_truth_cpu(clean_handler, noisy_handler, noise_threshold=0.15):
    if clean_handler.base_shape != noisy_handler.base_shape:
        raise ValueError(f"Base shape mismatch: clean {clean_handler.base_shape} vs noisy {noisy_handler.base_shape}")
    noisy_grids, order = {}, []
    for grid in noisy_handler.iterate_refinements(min_valid_ratio=0.0):
        noisy_grids[(grid.base_row, grid.base_col)] = grid
        order.append((grid.base_row, grid.base_col))
    cells = np.array([noisy_grids[k].depth.size for k in order], np.int64)
    offsets = np.concatenate([[0], np.cumsum(cells)]).astype(np.int64)
    place = {k: i for i, k in enumerate(order)}
    total = int(offsets[-1])
    out = {"labels": np.full(total, -1, np.int32), "difference": np.full(total, np.nan, np.float32),
           "mask": np.zeros(total, np.uint8), "noisy_depth": np.empty(total, np.float32), "uncertainty": np.empty(total, np.float32),
           "grid_counts": np.zeros((len(order), 4), np.int64), "paired": np.zeros(len(order), bool), "offsets": offsets,
           "hw": np.array([noisy_grids[k].dimensions for k in order], np.int32).reshape(-1, 2),
           "res": np.array([noisy_grids[k].resolution for k in order], np.float64).reshape(-1, 2), "order": order}
    for k in order:
        a, b = offsets[place[k]], offsets[place[k] + 1]
        out["noisy_depth"][a:b] = noisy_grids[k].depth.ravel()
        out["uncertainty"][a:b] = noisy_grids[k].uncertainty.ravel()

    stats = {"grids_processed": 0, "total_valid_cells": 0, "noise_cells": 0, "seafloor_cells": 0, "noise_magnitudes": []}
    labels_by_grid = {}
    for clean_grid in clean_handler.iterate_refinements(min_valid_ratio=0.0):
        key = (clean_grid.base_row, clean_grid.base_col)
        if key not in noisy_grids:
            continue
        noisy_grid = noisy_grids[key]
        if clean_grid.dimensions != noisy_grid.dimensions:
            continue
        with np.errstate(invalid="ignore"):
            difference = noisy_grid.depth - clean_grid.depth
            valid = clean_grid.valid_mask & noisy_grid.valid_mask
            labels = np.full(clean_grid.depth.shape, CLASS_SEAFLOOR, dtype=np.int32)
            noise_mask = np.abs(difference) > noise_threshold
        labels[noise_mask & valid] = CLASS_NOISE
        labels[~valid] = -1
        labels_by_grid[key] = {"labels": labels, "difference": difference, "resolution": clean_grid.resolution,
                               "dimensions": clean_grid.dimensions}
        stats["grids_processed"] += 1
        stats["total_valid_cells"] += int(np.sum(valid))
        stats["noise_cells"] += int(np.sum(labels == CLASS_NOISE))
        stats["seafloor_cells"] += int(np.sum(labels == CLASS_SEAFLOOR))
        if np.any(noise_mask & valid):
            stats["noise_magnitudes"].extend(np.abs(difference[noise_mask & valid]).tolist())
        g = place[key]
        a, b = offsets[g], offsets[g + 1]
        out["labels"][a:b] = labels.ravel(); out["difference"][a:b] = difference.ravel(); out["mask"][a:b] = valid.ravel()
        out["paired"][g] = True
        out["grid_counts"][g] = [int(valid.sum()), int((labels == 0).sum()), 0, int((labels == 2).sum())]

    stats_output = {
        "noise_threshold": noise_threshold, "processing_mode": "native_vr", "base_shape": list(clean_handler.base_shape),
        "grids_processed": stats["grids_processed"], "valid_cells": stats["total_valid_cells"], "noise_cells": stats["noise_cells"],
        "noise_percentage": float(100 * stats["noise_cells"] / max(1, stats["total_valid_cells"])),
        "seafloor_cells": stats["seafloor_cells"],
    }
    if stats["noise_magnitudes"]:
        magnitudes = np.array(stats["noise_magnitudes"])
        stats_output["mean_noise_magnitude"] = float(np.mean(magnitudes))
        stats_output["max_noise_magnitude"] = float(np.max(magnitudes))
        stats_output["median_noise_magnitude"] = float(np.median(magnitudes))
        stats_output["fsum_mean"] = math.fsum(stats["noise_magnitudes"]) / len(stats["noise_magnitudes"])
        stats_output["abs_sum"] = math.fsum(stats["noise_magnitudes"])
    out["stats"] = stats_output
    out["labels_by_grid"] = labels_by_grid
    return out


# ---- VR BAG pairs ------------------------------------------------------------------------------------------------------------
def bag_grids(md, ref):
    """{(row, col): [depth, uncertainty, (res_x, res_y), (sw_x, sw_y)]} of a VR BAG's arrays (copies)."""
    h = VRBagHandler.from_arrays(md, ref)
    return {(g.base_row, g.base_col): [g.depth.copy(), g.uncertainty.copy(), g.resolution, g.sw_corner]
            for g in h.iterate_refinements(0.0)}


def assemble_bag(base_shape, grids, reverse_records=False, shuffle_seed=None):
    """The two arrays of a VR BAG holding ``grids``; the records laid out in base-grid row-major order, in the reverse of it, or
    grid by grid in a drawn order."""
    md = np.zeros(base_shape, VARRES_METADATA_DTYPE)
    md["index"] = 4294967295
    keys = sorted(grids)
    layout = keys[::-1] if reverse_records else keys
    if shuffle_seed is not None:
        layout = [keys[i] for i in np.random.default_rng(shuffle_seed).permutation(len(keys))]
    pos, recs = 0, []
    for k in layout:
        d, u, res, sw = grids[k]
        h, w = d.shape
        md[k] = (pos, w, h, res[0], res[1], sw[0], sw[1])
        rec = np.empty(h * w, VARRES_REFINEMENT_DTYPE)
        rec["depth"] = d.ravel(); rec["depth_uncrt"] = u.ravel()
        recs.append(rec)
        pos += h * w
    ref = (np.concatenate(recs) if recs else np.empty(0, VARRES_REFINEMENT_DTYPE))[None, :]
    return VRBagHandler.from_arrays(md, ref)


def make_pair(variant="odd", seed=7, lo=1):
    """A clean / noisy pair of array-backed handlers and the cases it holds.  From ``synthetic_vr_bag(4, 5, lo=1, hi=9)`` with one
    grid set to 50 x 53.  The noisy copy: spikes of +-0.3 .. 2 m on about 5 % of the cells, jitter of +-0.05 on about 20 %, cells
    whose difference is exactly +-float32(0.15) and one an ulp above it, nodata and NaN cells in either file, a +inf depth, one
    grid dropped from the noisy file, one from the clean file, one with transposed dimensions, one paired grid with a single valid cell and one
    with none; the clean file's records lie in
    the reverse index order.  ``variant``: ``"odd"`` / ``"even"`` (the parity of the number of noise cells), ``"none"`` (no noise
    cell at all), ``"ties"`` (every spike 0.5 or 1.0 exactly, on depths of 8.0).  ``lo``: the shortest side of a grid; a
    BAG that holds a grid of one cell a side can be labelled but not classified (no gradient features)."""
    rng = np.random.default_rng(seed)
    md, ref = synthetic.synthetic_vr_bag(4, 5, lo=lo, hi=9)
    clean = bag_grids(md, ref)
    keys = sorted(clean)
    assert len(keys) >= 10
    big, drop_noisy, drop_clean, exact = keys[2], keys[4], keys[6], keys[1]
    transposed = next(k for k in keys[7:] if clean[k][0].shape[0] != clean[k][0].shape[1])
    rest = [k for k in keys[7:] if k != transposed and clean[k][0].size >= 4]
    sparse, empty = rest[0], rest[1]
    # the grid that crosses workgroup boundaries, and a small one with room for the exact differences
    depth = (20.0 + rng.random((50, 53)) * 5).astype(np.float32)
    clean[big] = [depth, np.full((50, 53), 0.25, np.float32), clean[big][2], clean[big][3]]
    clean[exact] = [np.full((3, 4), 12.0, np.float32), np.full((3, 4), 0.5, np.float32), clean[exact][2], clean[exact][3]]
    t015 = np.float32(0.15)
    clean[exact][0][0, :3] = [t015, t015 * 2, 0.0]
    clean[sparse][0].ravel()[1:] = NODATA                                      # one valid cell: below any ratio worth asking for
    clean[sparse][0].ravel()[0] = 15.0
    clean[empty][0][:] = 15.0
    noisy = {k: [v[0].copy(), v[1] + np.float32(0.125), v[2], v[3]] for k, v in clean.items()}
    for k, v in noisy.items():
        d = v[0]
        valid = np.isfinite(d) & (d != NODATA)
        jitter = (rng.random(d.shape) < 0.2) & valid
        d[jitter] += rng.uniform(-0.05, 0.05, int(jitter.sum())).astype(np.float32)
        if variant == "none":
            continue
        spike = (rng.random(d.shape) < 0.05) & valid & ~jitter
        if variant == "ties":
            clean[k][0][spike] = 8.0
            d[spike] = 8.0 + rng.choice(np.array([0.5, -0.5, 1.0], np.float32), int(spike.sum()))
        else:
            d[spike] += (rng.choice([-1.0, 1.0], int(spike.sum())) * rng.uniform(0.3, 2.0, int(spike.sum()))).astype(np.float32)
    clean[exact][0][0, :3] = [t015, t015 * 2, 0.0]                             # (again: a tie spike may have landed here)
    noisy[exact][0][0, :3] = [t015 * 2, t015, np.nextafter(t015, np.float32(1)) if variant != "none" else t015]
    noisy[exact][0][1, :] = clean[exact][0][1, :]                              # (no jitter on the cells set by hand below)
    noisy[big][0][3, 5] = NODATA; noisy[big][0][3, 6] = np.nan; noisy[big][0][3, 7] = np.inf
    clean[big][0][9, 5] = NODATA; clean[big][0][9, 6] = np.nan; clean[big][0][3, 6] = np.nan
    clean[big][0][9, 7] = np.inf; noisy[big][0][9, 7] = np.inf                 # inf - inf
    noisy[empty][0][:] = NODATA                                                # paired, and not a single valid cell
    noisy[sparse][0].ravel()[0] = 15.0
    del noisy[drop_noisy], clean[drop_clean]
    d, u, res, sw = noisy[transposed]
    noisy[transposed] = [np.ascontiguousarray(d.T), np.ascontiguousarray(u.T), res, sw]
    handlers = lambda: (assemble_bag((4, 5), clean, reverse_records=True), assemble_bag((4, 5), noisy))
    if variant in ("odd", "even"):
        n = native_truth_cpu(*handlers())["stats"]["noise_cells"]
        if n % 2 != (1 if variant == "odd" else 0):                            # one valid cell changes sides
            c, z = clean[big][0], noisy[big][0]
            z[20, 20] = c[20, 20] if abs(z[20, 20] - c[20, 20]) > t015 else c[20, 20] + np.float32(1.0)
            assert native_truth_cpu(*handlers())["stats"]["noise_cells"] == n + (1 if z[20, 20] != c[20, 20] else -1)
    clean_h, noisy_h = handlers()
    cases = {"big": big, "drop_noisy": drop_noisy, "drop_clean": drop_clean, "transposed": transposed, "exact": exact,
             "sparse": sparse, "empty": empty}
    return clean_h, noisy_h, cases


TRAINING_RESOLUTIONS = [(0.5, 0.5), (1.0, 2.0), (3.7, 0.25), (2.0, 2.0), (0.25, 4.0)]


def make_training_pair(seed=0):
    """A clean / noisy pair shaped like a VR training batch, both files with an uncertainty, and the base cells of its cases.
    From ``synthetic_vr_bag(4, 5, lo=2, hi=9)``, with these grids set by hand:

    ``big``         24 x 31 cells, spikes of +-0.3 .. 2 m on about 5 % of them, nodata on about 1 % (in either file)
    ``g22``         2 x 2: the noisy file constant, the clean file 0.75 m deeper (local_std 0, every quotient below -cap)
    ``g29``, ``g92``  2 x 9 and 9 x 2: every gradient feature along the short side is one-sided
    ``sparse``      3 x 4 with one valid cell, 0.75 m off its twin: an isolated node, local_std 0, the quotient above +cap
    ``flat``        7 x 7 of constant depth with one spike at a corner of the noisy file: local_std 0 three cells away from it
    ``no_twin``     dropped from the clean file; ``transposed``: other dimensions in the noisy file -- neither reaches a store
    Of the remaining grids those are kept, in index order, whose cells add up to at most 150, so that every grid but ``big``
    holds fewer than 256 cells together; they get jitter of +-0.05 m on about 20 % of their cells and spikes on about 10 %.
    Resolutions: ``TRAINING_RESOLUTIONS`` round-robin over the grids a store keeps, in the noisy file's order."""
    rng = np.random.default_rng([seed, 77])
    md, ref = synthetic.synthetic_vr_bag(4, 5, seed=1000 + seed, lo=2, hi=9, empty_fraction=0.0, sparse_fraction=0.0)
    clean = bag_grids(md, ref)
    keys = sorted(clean)
    assert len(keys) >= 11, len(keys)
    names = ("g29", "flat", "big", "no_twin", "sparse", "g22", "transposed", "g92")
    cases = dict(zip(names, keys[:len(names)]))
    budget, extras = 150, []
    for k in keys[len(names):]:
        if clean[k][0].size <= budget:
            extras.append(k); budget -= clean[k][0].size
        else:
            del clean[k]
    assert len(extras) >= 3, extras

    def put(name, depth, unc=None):
        k = cases[name]
        depth = np.ascontiguousarray(depth, np.float32)
        unc = np.full(depth.shape, 0.25, np.float32) if unc is None else unc
        clean[k] = [depth, unc, clean[k][2], clean[k][3]]
    put("big", 20.0 + rng.random((24, 31)) * 5, (0.05 + 0.25 * rng.random((24, 31))).astype(np.float32))
    put("g22", np.full((2, 2), 10.25))
    put("g29", 14.0 + rng.random((2, 9)))
    put("g92", 16.0 + rng.random((9, 2)))
    put("sparse", np.full((3, 4), NODATA))
    clean[cases["sparse"]][0][1, 2] = 15.0
    put("flat", np.full((7, 7), 12.0))
    if clean[cases["transposed"]][0].shape[0] == clean[cases["transposed"]][0].shape[1]:
        put("transposed", 18.0 + rng.random((3, 5)))
    noisy = {k: [v[0].copy(), v[1] + np.float32(0.125), v[2], v[3]] for k, v in clean.items()}
    for k in [cases["big"], cases["g29"], cases["g92"]] + extras:
        d = noisy[k][0]
        valid = d != NODATA
        jitter = (rng.random(d.shape) < 0.2) & valid
        d[jitter] += rng.uniform(-0.05, 0.05, int(jitter.sum())).astype(np.float32)
        spike = (rng.random(d.shape) < (0.05 if k == cases["big"] else 0.1)) & valid & ~jitter
        d[spike] += (rng.choice([-1.0, 1.0], int(spike.sum())) * rng.uniform(0.3, 2.0, int(spike.sum()))).astype(np.float32)
    for file in (clean, noisy):                                                # nodata on about 1 % of the big grid, in either file
        file[cases["big"]][0][rng.random((24, 31)) < 0.005] = NODATA
    noisy[cases["g22"]][0][:] = 9.5
    noisy[cases["sparse"]][0][1, 2] = 15.75
    noisy[cases["flat"]][0][0, 0] = 13.0
    del clean[cases["no_twin"]]
    d, u, res, sw = noisy[cases["transposed"]]
    noisy[cases["transposed"]] = [np.ascontiguousarray(d.T), np.ascontiguousarray(u.T), res, sw]
    kept = [k for k in sorted(noisy) if k not in (cases["no_twin"], cases["transposed"])]
    for i, k in enumerate(kept):
        res = TRAINING_RESOLUTIONS[i % len(TRAINING_RESOLUTIONS)]
        clean[k][2] = noisy[k][2] = res
    return assemble_bag((4, 5), clean, reverse_records=True), assemble_bag((4, 5), noisy), cases


def make_isolated_pair():
    """Two grids with one valid cell each, at different anisotropic resolutions: the smallest batch ``train()`` takes.  One
    cell is noise (0.75 m off its twin), the other seafloor."""
    clean, noisy = {}, {}
    for key, shape, at, depth, off, res in (((0, 0), (3, 4), (1, 2), 15.0, 0.75, (1.0, 2.0)), ((0, 1), (5, 2), (4, 0), 22.5, 0.0, (3.7, 0.25))):
        d = np.full(shape, NODATA, np.float32)
        d[at] = depth
        z = d.copy()
        z[at] = depth + off
        u = np.full(shape, 0.25, np.float32)
        clean[key] = [d, u, res, (0.5, 0.5)]
        noisy[key] = [z, u + np.float32(0.125 * (1 + key[1])), res, (0.5, 0.5)]
    return assemble_bag((1, 2), clean), assemble_bag((1, 2), noisy)


def store_batch_cpu(ref, kept, indices, resolutions):
    """The oracle's batch of the store tiles ``indices`` (``kept[i]``: the grid of ``native_truth_cpu``'s planes behind store tile
    ``i``; ``resolutions[i]`` its resolution): one ``graph_cpu.build_graph(noisy_depth, labels >= 0, uncertainty, res)`` per tile in
    that order, then ``graph_cpu.batch_graphs``.  ``labels`` / ``difference``: per node, the valid cells row-major, grid after
    grid; ``nodes``: the node count of every tile."""
    from oracle import graph_cpu
    graphs, labels, difference = [], [], []
    for i in indices:
        g = int(kept[int(i)])
        a, b = int(ref["offsets"][g]), int(ref["offsets"][g + 1])
        shape = tuple(int(v) for v in ref["hw"][g])
        lab = ref["labels"][a:b].reshape(shape)
        valid = lab >= 0
        res = (float(resolutions[int(i)][0]), float(resolutions[int(i)][1]))
        graphs.append(graph_cpu.build_graph(ref["noisy_depth"][a:b].reshape(shape), valid, ref["uncertainty"][a:b].reshape(shape), res))
        labels.append(lab[valid]); difference.append(ref["difference"][a:b].reshape(shape)[valid])
    x, ei, ea, ls, batch = graph_cpu.batch_graphs(graphs)
    return {"x": x, "edge_index": ei, "edge_attr": ea, "local_std": ls, "batch": batch,
            "pos": np.concatenate([g.pos for g in graphs], 0), "nodes": np.array([g.num_nodes for g in graphs], np.int64),
            "labels": np.concatenate(labels), "difference": np.concatenate(difference)}


def make_scale_pair(seed=3):
    """A pair past 2 * 2048 tiles of 1024 cells, so that a workgroup of the label pass walks from tile to tile: a 45 x 60 base
    grid, every cell refined, 20 .. 60 cells a side, except a run of 700 base cells of 1 x 1 and 1 x 2 grids (more than 256 grids
    meet one tile: the offsets are staged in several rounds).  Spikes on 2 % of the cells, nodata on 1 %, every 97th grid without a
    twin; the clean file's records grid by grid in a drawn order."""
    rng = np.random.default_rng(seed)
    clean, noisy = {}, {}
    for i in range(45 * 60):
        k = (i // 60, i % 60)
        h, w = (1, 1 + i % 2) if 1000 <= i < 1700 else (int(rng.integers(20, 61)), int(rng.integers(20, 61)))
        d = (30.0 + 10.0 * rng.random((h, w))).astype(np.float32)
        d[rng.random((h, w)) < 0.01] = NODATA
        z = d.copy()
        spike = rng.random((h, w)) < 0.02
        z[spike] += rng.uniform(-2.0, 2.0, int(spike.sum())).astype(np.float32)
        u = rng.random((h, w)).astype(np.float32)
        res = (1.0, 1.0)
        noisy[k] = [z, u, res, (0.5, 0.5)]
        if i % 97 != 5:
            clean[k] = [d, u, res, (0.5, 0.5)]
    return assemble_bag((45, 60), clean, shuffle_seed=seed), assemble_bag((45, 60), noisy)
