"""Depth hypotheses per cell on the device (bgnn_hypotheses_build, data/sounding_hypotheses.py) against the Python-integer
restatement of _hypotheses_cpu.py (test_host_hypotheses.py guards the restatement itself).  Every plane, the records,
``ambiguity_plane``, ``hypotheses_of`` and the flags of a hypothesis result are compared for equal bits; any two device runs on
the same soundings, in any order and any split over ``add`` calls, must leave equal bytes."""
import functools

import numpy as np
import pytest
import torch

import _hypotheses_cpu as hc
import _robust_cpu as rc
import _soundings_cpu as sc
import _vr_soundings_cpu as vc

pytestmark = pytest.mark.gpu


def _dev(device, *arrays):
    return [torch.from_numpy(np.array(a)).to(device) for a in arrays]           # (a copy: the shared clouds are read-only)


def _host(hyp):
    """Everything a hypothesis result holds, as host arrays; the records cut to the hypotheses there are (None where not kept)."""
    out = {k: getattr(hyp, k).cpu().numpy() for k in hc.PLANES}
    out["ambiguity"] = hyp.ambiguity_plane().cpu().numpy()
    if hyp.hyp_start is not None:
        out["hyp_start"] = hyp.hyp_start.cpu().numpy().view(np.uint32).astype(np.int64)
        total = int(out["hyp_start"][-1])
        out["hyp_first"] = hyp.hyp_first.cpu().numpy().view(np.uint32).astype(np.int64)[:total]
        out["hyp_count"] = hyp.hyp_count.cpu().numpy()[:total]
    return out


def _check(hyp, want, records=True):
    got = _host(hyp)
    for k in hc.PLANES + ("ambiguity",):
        assert got[k].shape == want[k].shape and got[k].dtype == want[k].dtype, k
        differ = np.flatnonzero((got[k].reshape(-1).view(np.uint8).reshape(got[k].size, -1) !=
                                 want[k].reshape(-1).view(np.uint8).reshape(got[k].size, -1)).any(axis=1))
        assert differ.size == 0, (k, differ.size, differ[:4], got[k].reshape(-1)[differ[:4]], want[k].reshape(-1)[differ[:4]])
    assert (hyp.hyp_start is not None) == records and (hyp.hyp_first is None) == (hyp.hyp_count is None) == (not records)
    if records:
        for k in hc.RECORDS:
            assert got[k].dtype == want[k].dtype and np.array_equal(got[k], want[k]), k
    return got


def _planes_differ(a, b):
    return [k for k in hc.PLANES + ("ambiguity",) if a[k].tobytes() != b[k].tobytes()]


def _gridder(device, shape, origin, res, capacity, **kw):
    from bathymetric_gnn_amd.data import RobustSoundingGridder
    return RobustSoundingGridder(shape, origin, res, capacity, device=device, **kw)


# ---- 1. the mixed cloud -------------------------------------------------------------------------------------------------------------

def _mixed_guide(want):
    guide = want["median"].copy()
    guide[0, 0], guide[3, 4], guide[7, 7], guide[15, 15] = np.nan, np.inf, 40000.0, want["median"].dtype.type(1.0e6)
    guide[9, 2] += np.float32(1.5)
    return guide


@functools.lru_cache(maxsize=None)
def _mixed_hyp_want(gap_m, rule, min_count):
    want = rc.mixed_want()
    return hc.grid(want, gap_m, rule, _mixed_guide(want) if rule == "guide" else None, min_count)


@pytest.fixture(scope="module")
def mixed_run(gpu_device):
    x, y, z = sc.mixed_cloud()
    g = _gridder(gpu_device, sc.MIXED_SHAPE, sc.MIXED_ORIGIN, sc.MIXED_RES, 20000)
    cloud = _dev(gpu_device, x, y, z)
    g.add(*cloud)
    return g, g.finalize(), cloud


@pytest.mark.parametrize("rule,min_count", [("count", 1), ("count", 3), ("guide", 2)])
@pytest.mark.parametrize("gap_m", [0.5, 0.05, 0.0])
def test_mixed_cloud(gap_m, rule, min_count, mixed_run, gpu_device):
    """The 16 x 16 grid of test_gpu_soundings_robust (44 to 98 soundings a cell: both size classes) at three gaps: 2 to 14, 35 to 64
    and 44 to 98 hypotheses a cell.  With and without records, which leaves the planes as they are."""
    from bathymetric_gnn_amd.data import HypothesisGrid
    g, grid, (dx, dy, dz) = mixed_run
    x, y, z = sc.mixed_cloud()
    want = _mixed_hyp_want(gap_m, rule, min_count)
    guide = torch.from_numpy(_mixed_guide(rc.mixed_want())).to(gpu_device) if rule == "guide" else None
    hyp = grid.hypotheses(gap_m, rule=rule, guide=guide, min_count=min_count)
    assert isinstance(hyp, HypothesisGrid) and hyp.sorted_q is grid.sorted_q and hyp.start is grid.start
    assert (hyp.gap_m, hyp.rule, hyp.min_count, hyp.transform, hyp.resolution, hyp.nodata_value) == \
        (gap_m, rule, min_count, grid.transform, grid.resolution, grid.nodata_value)
    a = _check(hyp, want)
    bare = grid.hypotheses(gap_m, rule=rule, guide=guide, min_count=min_count, records=False)
    assert _planes_differ(_check(bare, want, records=False), a) == []
    with pytest.raises(ValueError, match="records"):
        bare.hypotheses_of(0, 0)
    for row, col in ((0, 0), (5, 7), (15, 15)):
        assert hyp.hypotheses_of(row, col) == want["hyps"][row * 16 + col]
    flags = g.flag(dx, dy, dz, hyp).cpu().numpy()
    assert np.array_equal(flags, rc.flags(x, y, z, sc.MIXED_SHAPE, sc.MIXED_ORIGIN, sc.MIXED_RES, want["center2"], want["limit"]))
    assert int((flags == 0).sum()) == int(want["kept"].sum())
    assert torch.equal(hyp.density_plane(), torch.where(hyp.kept >= 1, 1.0 / hyp.kept.float(), torch.zeros((), device=gpu_device)))
    d, v, u, dens = hyp.survey_tensors(density=True)
    assert d is hyp.depth and v is hyp.valid and u is hyp.std and torch.equal(dens, hyp.density_plane())
    assert hyp.survey_tensors("min")[0] is hyp.min and hyp.survey_tensors("max")[0] is hyp.max
    with pytest.raises(ValueError):
        hyp.survey_tensors("median")
    host = hyp.to_grid()
    assert np.array_equal(host.depth, a["depth"]) and np.array_equal(host.uncertainty, a["std"]) and host.transform == grid.transform


# ---- 2. the boundary grid -------------------------------------------------------------------------------------------------------------

BOUNDARY_SHAPE = (4, 8)
BIG = 70000
SHARE = -(-BIG // 256)                                   # 274: thread t of hyp_choose_long takes positions t * 274 .. of such a cell
MID = 256 * 137                                          # = 128 * SHARE: a multiple of 256 that is a share boundary as well
LATTICE = 1.0 / 1024.0                                   # 64 units of 2^-16 m: exact in float32 at these depths


def _lattice(n, breaks=(), base=-100.0):
    """n distinct depths ascending on the lattice, 4 m more before every index in ``breaks``."""
    jump = np.zeros(n)
    jump[list(breaks)] = 4.0
    return (base + np.arange(n) * LATTICE + np.cumsum(jump)).astype(np.float32)


@functools.lru_cache(maxsize=None)
def _boundary_cloud():
    """One cell each, shuffled, a few soundings that are not accepted riding along.  Under a gap of 0.5 m: n = 0, 1, 2, 63, 64, 65,
    4095, 4096, 4097 and 70 000 as one run (at a gap of 0 every sounding is its own run); long cells of two runs with the break at
    256 k - 1, 256 k, 256 k + 1 (k = 137, also a share boundary), at 1 and at n - 1; and the cells of the ties (see the test)."""
    from bathymetric_gnn_amd import runtime as rt
    assert rt.ROBUST_WAVE_MAX == 64 and rt.ROBUST_LDS_MAX == 4096 and MID == 128 * SHARE
    rng = np.random.default_rng(41)
    m = lambda *v: np.array(v, np.float32)
    cells = [m(), m(-12.5), m(-12.5, -11.5), _lattice(63), _lattice(64, [32]), _lattice(65), _lattice(4095), _lattice(4096, [1]),
             _lattice(4097, [4096]), _lattice(BIG)]                                                           # 0 .. 9
    cells += [_lattice(BIG, [MID - 1]), _lattice(BIG, [MID]), _lattice(BIG, [MID + 1]), _lattice(BIG, [1]), _lattice(BIG, [BIG - 1])]   # 10 .. 14
    cells += [m(-40, -39.75, -10, -9.75, -9.5, 20, 20.25, 20.5, 30, 30.25, 30.5),   # 15: three runs of 3, the one nearest to the median (20)
              m(-2, -1.75, 1.75, 2),                                               # 16: symmetric, both keys tie, the lower index
              m(-30, -30, -30, -20, -20), m(-30, -30, -20, -20, -20),              # 17, 18: a guide of -25 halfway, the larger count
              m(-32767.5, 32767.5),                                                # 19: 2^32 - 2^16 apart
              _lattice(130, [1, 2, 66, 129]),                                      # 20: runs of 1, 1, 64, 63, 1 in the long class
              _lattice(300, [SHARE - 1, SHARE, SHARE + 1, 299]),                   # 21
              np.concatenate([_lattice(40), _lattice(40, base=-50.0), _lattice(39, base=-20.0)])]   # 22: 40, 40, 39: count ties, the median decides
    assert len(cells) <= BOUNDARY_SHAPE[0] * BOUNDARY_SHAPE[1]
    xs, ys, zs = [], [], []
    for i, depths in enumerate(cells):
        r, c = divmod(i, BOUNDARY_SHAPE[1])
        xs.append(c + rng.uniform(0.05, 0.95, depths.size)); ys.append(BOUNDARY_SHAPE[0] - (r + rng.uniform(0.05, 0.95, depths.size)))
        zs.append(depths)
    xs.append(np.array([-0.5, 2.5, np.nan, 3.5])); ys.append(np.array([1.5, 1.5, 1.5, 9.0])); zs.append(np.array([-5, 40000, -5, -5], np.float32))
    x, y, z = np.concatenate(xs), np.concatenate(ys), np.concatenate(zs).astype(np.float32)
    p = rng.permutation(z.size)
    return sc._frozen(x[p].astype(np.float64), y[p].astype(np.float64), z[p]) + (tuple(c.size for c in cells),)


@functools.lru_cache(maxsize=None)
def _boundary_want():
    x, y, z, _ = _boundary_cloud()
    return rc.grid(x, y, z, BOUNDARY_SHAPE, (0.0, float(BOUNDARY_SHAPE[0])), 1.0)


def test_boundary_grid(gpu_device):
    x, y, z, sizes = _boundary_cloud()
    robust = _boundary_want()
    origin = (0.0, float(BOUNDARY_SHAPE[0]))
    n = robust["count"].reshape(-1)
    assert tuple(n[:len(sizes)]) == sizes and {0, 1, 2, 63, 64, 65, 4095, 4096, 4097, BIG} <= set(n.tolist())
    g = _gridder(gpu_device, BOUNDARY_SHAPE, origin, 1.0, z.size + 3)
    dx, dy, dz = _dev(gpu_device, x, y, z)
    g.add(dx, dy, dz)
    grid = g.finalize()
    assert np.array_equal(grid.sorted_q.cpu().numpy()[:robust["sorted_q"].size], robust["sorted_q"])

    def run(gap_m, rule="count", guide=None, min_count=1):
        want = hc.grid(robust, gap_m, rule, guide, min_count)
        hyp = grid.hypotheses(gap_m, rule=rule, guide=None if guide is None else torch.from_numpy(guide).to(gpu_device),
                              min_count=min_count)
        _check(hyp, want)
        bare = grid.hypotheses(gap_m, rule=rule, guide=None if guide is None else torch.from_numpy(guide).to(gpu_device),
                               min_count=min_count, records=False)
        _check(bare, want, records=False)
        flags = g.flag(dx, dy, dz, hyp).cpu().numpy()
        assert np.array_equal(flags, rc.flags(x, y, z, BOUNDARY_SHAPE, origin, 1.0, want["center2"], want["limit"]))
        return {k: v.reshape(-1) if isinstance(v, np.ndarray) and k in hc.PLANES else v for k, v in want.items()}, hyp, flags

    # a gap of 0.5 m: the conditions on the restatement first, so that the comparison above is not about the wrong thing
    w, hyp, _ = run(0.5)
    assert w["n_hyp"][:15].tolist() == [0, 1, 2, 1, 2, 1, 1, 2, 2, 1, 2, 2, 2, 2, 2]
    assert w["kept"][:15].tolist() == [0, 1, 1, 63, 32, 65, 4095, 4095, 4096, BIG, MID - 1, MID, MID + 1, BIG - 1, BIG - 1]
    assert w["chosen"][:15].tolist() == [-1, 0, 0, 0, 0, 0, 0, 1, 0, 0, 0, 0, 0, 1, 0]      # (n = 2 and n = 64: ties, the lower index)
    assert (w["n_hyp"][15], w["chosen"][15], w["kept"][15]) == (4, 2, 3)                    # equal counts: the median distance
    assert (w["n_hyp"][16], w["chosen"][16], w["kept"][16]) == (2, 0, 2)                    # symmetric: the lower index
    assert (w["n_hyp"][20], w["chosen"][20], w["kept"][20]) == (5, 2, 64)
    assert (w["n_hyp"][21], w["kept"][21]) == (5, SHARE - 1)
    assert (w["n_hyp"][22], w["chosen"][22], w["kept"][22]) == (3, 1, 40)                   # 40, 40, 39: the run the median lies in
    assert w["n_hyp"][19] == 2 and w["valid"][0] == 0 and w["limit"][0] == -1
    assert hyp.hypotheses_of(1, 2) == w["hyps"][10] and [h["count"] for h in w["hyps"][10]] == [MID - 1, BIG - MID + 1]
    # a gap of 0: every sounding of a lattice cell is a run of its own
    w, hyp, _ = run(0.0)
    lattice = [3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 20, 21]
    assert np.array_equal(w["n_hyp"][lattice], n[lattice]) and (w["kept"][lattice] == 1).all() and w["n_hyp"][17] == 2
    assert int(w["hyp_start"][-1]) > 6 * BIG
    # by guide: halfway between two runs the larger count wins; NaN elsewhere (the count key) but where a run is pointed at
    guide = np.full(BOUNDARY_SHAPE, np.nan, np.float32)
    guide.reshape(-1)[[17, 18]] = -25.0
    guide.reshape(-1)[[4, 11, 15, 22]] = [-95.9, -40.0, 30.2, -20.0]             # the second run of 64 and of 70 000, the last of 3, the 39
    guide.reshape(-1)[[2, 16]] = [np.inf, -1.0e6]
    w, _, _ = run(0.5, "guide", guide)
    assert (w["chosen"][17], w["chosen"][18]) == (0, 1) and (w["kept"][17], w["kept"][18]) == (3, 3)
    assert (w["chosen"][4], w["chosen"][11], w["chosen"][15], w["chosen"][22]) == (1, 1, 3, 2) and w["kept"][22] == 39
    assert (w["chosen"][2], w["chosen"][16]) == (0, 0)
    # both signs just under 32768 m: one run at gap_q = 2^32, two at 2^32 - 2^18
    q = robust["sorted_q"][robust["start"][19]:robust["start"][20]].astype(np.int64)
    assert int(q[1] - q[0]) >= 2 ** 32 - 2 ** 17
    w, _, _ = run(65536.0)
    assert w["gap_q"] == 2 ** 32 and (w["n_hyp"][1:23] == 1).all() and (w["kept"] == n).all()
    assert (w["limit"][19], w["center2"][19]) == (int(q[1] - q[0]), 0)
    w, _, _ = run((2 ** 32 - 2 ** 18) / 65536.0)
    assert w["gap_q"] == 2 ** 32 - 2 ** 18 and w["n_hyp"][19] == 2 and (w["n_hyp"][1:23][np.arange(1, 23) != 19] == 1).all()
    # min_count above every run of some cells: none chosen, everything nodata, every accepted sounding of the cell rejected
    w, hyp, flags = run(0.5, min_count=41)
    none = np.flatnonzero((w["chosen"] == -1) & (n > 0))
    assert set(none.tolist()) == {1, 2, 4, 15, 16, 17, 18, 19, 22}
    assert (w["limit"][none] == -1).all() and (w["kept"][none] == 0).all() and (w["valid"][none] == 0).all()
    assert all((w[k][none] == np.float32(1.0e6)).all() for k in hc.FLOATS) and (w["ambiguity"].reshape(-1)[none] == 1.0).all()
    cell, _, _ = rc.stage(x, y, z, BOUNDARY_SHAPE, origin, 1.0)
    assert (flags[np.isin(cell, none)] == 1).all() and int(np.isin(cell, none).sum()) == int(n[none].sum())
    w, _, flags = run(0.5, min_count=BIG + 1)
    assert (w["chosen"] == -1).all() and set(flags.tolist()) == {1, 2}


# ---- 3. planted surfaces ------------------------------------------------------------------------------------------------------------

PLANTED_SHAPE, PLANTED_ORIGIN = (24, 24), (1000.0, 2024.0)
DEEP, SHOAL = -35.0, -31.0


@functools.lru_cache(maxsize=None)
def _planted_cloud():
    """Every cell of a 24 x 24 grid at res 1: ``a`` soundings about -35 m and ``b`` about -31 m, sd 0.1 m, a and b from 5 .. 60; the
    depths lie on the 2^-16 m lattice, so that their float64 mean is the mean of the quantised soundings.  ``member``: 0 or 1."""
    rng = np.random.default_rng(47)
    cells = PLANTED_SHAPE[0] * PLANTED_SHAPE[1]
    a, b = rng.integers(5, 61, cells), rng.integers(5, 61, cells)
    cell = np.concatenate([np.repeat(np.arange(cells), a), np.repeat(np.arange(cells), b)])
    member = np.concatenate([np.zeros(int(a.sum()), np.int64), np.ones(int(b.sum()), np.int64)])
    z = np.where(member == 0, DEEP, SHOAL) + 0.1 * rng.standard_normal(cell.size)
    z = (np.rint(z * 65536.0) / 65536.0).astype(np.float32)
    assert np.array_equal(z.astype(np.float64) * 65536.0, np.rint(z.astype(np.float64) * 65536.0))
    x = PLANTED_ORIGIN[0] + cell % PLANTED_SHAPE[1] + rng.uniform(0.02, 0.98, cell.size)
    y = PLANTED_ORIGIN[1] - (cell // PLANTED_SHAPE[1] + rng.uniform(0.02, 0.98, cell.size))
    p = rng.permutation(cell.size)
    return sc._frozen(x[p], y[p], z[p], cell[p], member[p], a, b)


def _planted_facts(group, z, member, n_groups):
    """Per group (a cell or a record): the sizes of its two clusters, the float64 mean of each, its worst inner gap and the
    separation of the two."""
    size = np.zeros((n_groups, 2), np.int64)
    mean = np.zeros((n_groups, 2))
    inner, apart = np.zeros(n_groups), np.zeros(n_groups)
    order = np.lexsort((z, group))
    bounds = np.searchsorted(group[order], np.arange(n_groups + 1))
    for i in range(n_groups):
        sel = order[bounds[i]:bounds[i + 1]]
        zi, mi = z[sel].astype(np.float64), member[sel]
        lo, hi = zi[mi == 0], zi[mi == 1]
        size[i] = lo.size, hi.size
        mean[i] = lo.sum() / lo.size, hi.sum() / hi.size
        inner[i] = max(np.diff(lo).max(initial=0.0), np.diff(hi).max(initial=0.0))
        apart[i] = hi.min() - lo.max()
    return size, mean, inner, apart


def _check_planted(hyp_count, hyp_guide, flags, group, member, size, mean, chosen_want):
    n_groups = size.shape[0]
    larger = np.where(size[:, 0] == size[:, 1], chosen_want, (size[:, 1] > size[:, 0]).astype(np.int64))     # (a tie: the rule's own)
    smaller = np.where(size[:, 0] == size[:, 1], chosen_want, 1 - larger)
    rows = np.arange(n_groups)
    assert (hyp_count.n_hyp.cpu().numpy().reshape(-1) == 2).all()
    assert np.array_equal(hyp_count.kept.cpu().numpy().reshape(-1), size.max(axis=1))
    assert np.array_equal(hyp_count.chosen.cpu().numpy().reshape(-1), larger)
    assert np.array_equal(hyp_count.depth.cpu().numpy().reshape(-1).view(np.uint32), mean[rows, larger].astype(np.float32).view(np.uint32))
    assert np.array_equal(hyp_guide.kept.cpu().numpy().reshape(-1), size.min(axis=1))
    differ = size[:, 0] != size[:, 1]
    assert np.array_equal(hyp_guide.chosen.cpu().numpy().reshape(-1)[differ], smaller[differ])
    assert np.array_equal(flags == 0, member == larger[group]) and set(flags.tolist()) == {0, 1}


def test_planted_surfaces(gpu_device):
    from bathymetric_gnn_amd.data import RobustVRSoundingGridder, VRHypothesisGrid, VRLayout
    x, y, z, cell, member, a, b = _planted_cloud()
    cells = a.size
    size, mean, inner, apart = _planted_facts(cell, z, member, cells)
    assert np.array_equal(size, np.stack([a, b], axis=1)) and (a == b).any() and (a != b).sum() > 500
    assert inner.max() < 0.5 < apart.min()                                       # the test's own input: one run a cluster, two a cell
    robust = rc.grid(x, y, z, PLANTED_SHAPE, PLANTED_ORIGIN, 1.0)
    assert np.array_equal(robust["count"].reshape(-1), a + b)
    want = hc.grid(robust, 0.5)
    smaller_centre = np.where(a <= b, DEEP, SHOAL)
    guide = (smaller_centre + 0.3).astype(np.float32).reshape(PLANTED_SHAPE)
    g = _gridder(gpu_device, PLANTED_SHAPE, PLANTED_ORIGIN, 1.0, z.size)
    dx, dy, dz = _dev(gpu_device, x, y, z)
    g.add(dx, dy, dz)
    grid = g.finalize()
    by_count = grid.hypotheses(0.5)
    by_guide = grid.hypotheses(0.5, rule="guide", guide=torch.from_numpy(guide).to(gpu_device))
    _check(by_count, want)
    _check(by_guide, hc.grid(robust, 0.5, "guide", guide))
    flags = g.flag(dx, dy, dz, by_count).cpu().numpy()
    _check_planted(by_count, by_guide, flags, cell, member, size, mean, want["chosen"].reshape(-1))

    # the same cloud on a two-rung layout: 6 x 6 base cells of 4 m, 4 x 4 records of 1 m or 2 x 2 of 2 m
    d = np.where(np.add.outer(np.arange(6), np.arange(6)) % 2 == 0, 4, 2)
    lay = vc.make_layout((6, 6), (PLANTED_ORIGIN[0], PLANTED_ORIGIN[1] - 24.0), 4.0, d, d)
    kind, record = vc.classify(x, y, z, lay)
    assert (kind == vc.ACCEPTED).all() and lay["total"] == 18 * 16 + 18 * 4
    rsize, rmean, rinner, rapart = _planted_facts(record, z, member, lay["total"])
    assert rinner.max() < 0.5 < rapart.min() and rsize.sum() == z.size
    vrobust = vc.robust_grid(x, y, z, lay)
    vwant = hc.grid(vrobust, 0.5)
    layout = VRLayout(lay["base_shape"], lay["origin"], lay["B"], lay["index"], lay["dx"], lay["dy"], lay["total"], device=gpu_device)
    vg = RobustVRSoundingGridder(layout, z.size)
    vg.add(dx, dy, dz)
    vgrid = vg.finalize()
    vguide = (np.where(rsize[:, 0] <= rsize[:, 1], DEEP, SHOAL) + 0.3).astype(np.float32)
    v_count = vgrid.hypotheses(0.5)
    v_guide = vgrid.hypotheses(0.5, rule="guide", guide=torch.from_numpy(vguide).to(gpu_device))
    assert isinstance(v_count, VRHypothesisGrid) and v_count.layout is layout and tuple(v_count.depth.shape) == (lay["total"],)
    _check(v_count, vwant)
    _check(v_guide, hc.grid(vrobust, 0.5, "guide", vguide))
    vflags = vg.flag(dx, dy, dz, v_count).cpu().numpy()
    assert np.array_equal(vflags, vc.robust_flags(x, y, z, lay, vwant["center2"], vwant["limit"]))
    _check_planted(v_count, v_guide, vflags, record, member, rsize, rmean, vwant["chosen"].reshape(-1))
    assert v_count.hypotheses_of(7) == vwant["hyps"][7]
    # handler("depth") round-trips the records
    recs = v_count.records().cpu().numpy()
    assert recs.shape == (lay["total"], 2) and np.array_equal(recs[:, 0], vwant["depth"]) and np.array_equal(recs[:, 1], vwant["std"])
    handler = v_count.handler("depth")
    back = np.asarray(handler.varres_refinements).reshape(-1)
    assert np.array_equal(back["depth"], vwant["depth"]) and np.array_equal(back["depth_uncrt"], vwant["std"])
    first, dy_, dx_ = layout.grid_slice(0, 0)
    assert torch.equal(v_count.grid(0, 0, "depth"), v_count.depth[first:first + dy_ * dx_].view(dy_, dx_))


# ---- 4. determinism -----------------------------------------------------------------------------------------------------------------

def test_order_and_split(gpu_device):
    """The mixed cloud in one call, permuted, and in a three-call split: equal bytes in every hypothesis output, under both rules."""
    x, y, z = sc.mixed_cloud()
    dx, dy, dz = _dev(gpu_device, x, y, z)
    perm = torch.from_numpy(np.random.default_rng(9).permutation(z.size)).to(gpu_device)
    guide = torch.from_numpy(_mixed_guide(rc.mixed_want())).to(gpu_device)
    runs = []
    for cuts, order in (((0, 20000), None), ((0, 20000), perm), ((0, 7001, 7002, 20000), None), ((0, 4097, 16000, 20000), perm)):
        g = _gridder(gpu_device, sc.MIXED_SHAPE, sc.MIXED_ORIGIN, sc.MIXED_RES, 20000)
        cx, cy, cz = (dx, dy, dz) if order is None else (dx[order], dy[order], dz[order])
        for lo, hi in zip(cuts[:-1], cuts[1:]):
            g.add(cx[lo:hi], cy[lo:hi], cz[lo:hi])
        grid = g.finalize()
        out = {}
        for name, kw in (("count", dict(gap_m=0.05)), ("guide", dict(gap_m=0.5, rule="guide", guide=guide, min_count=2))):
            out.update({f"{name}.{k}": v for k, v in _host(grid.hypotheses(**kw)).items()})
        runs.append(out)
    for r in runs[1:]:
        assert r.keys() == runs[0].keys()
        for k in r:
            assert r[k].tobytes() == runs[0][k].tobytes(), k
    assert np.array_equal(runs[0]["count.kept"], _mixed_hyp_want(0.05, "count", 1)["kept"])
