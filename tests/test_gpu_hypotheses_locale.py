"""``rule="locale"`` end to end through ``RobustSoundingGridder``: a seabed at -30 m under two fish schools at -26 m that outnumber it
in every cell they cover.  The count rule takes the school in all of those cells; the locale rule puts a school of 3 x 3 cells back
on the seabed, and a school of 5 x 5 cells everywhere but in its centre, whose window holds no witness -- the limit of one pass of
the rule, which this test writes down.  Every plane and the records are compared for equal bits with the restatements composed
(_robust_cpu, _hypotheses_cpu, _locale_cpu), no cell left out; a shuffled cloud and a three-call split must leave equal bytes."""
import functools

import numpy as np
import pytest
import torch

import _hypotheses_cpu as hc
import _locale_cpu as lc
import _robust_cpu as rc
import _soundings_cpu as sc
import _vr_soundings_cpu as vc

pytestmark = pytest.mark.gpu

SHAPE, ORIGIN, RES = (24, 24), (1000.0, 2024.0), 1.0
GAP_M = 0.5
SEABED, SCHOOL = -30.0, -26.0
N_SEABED, N_SCHOOL = 25, 40
SMALL = (slice(3, 6), slice(4, 7))                       # 3 x 3 cells
LARGE = (slice(14, 19), slice(13, 18))                   # 5 x 5 cells, more than the radius away from the other
LARGE_CENTRE = (16, 15)
RADIUS, MIN_SUPPORT = 2, 3


@functools.lru_cache(maxsize=None)
def _cloud():
    """``x, y, z, cell, member`` (0 seabed, 1 school), shuffled; the depths lie on the 2^-16 m lattice."""
    rng = np.random.default_rng(61)
    school = np.zeros(SHAPE, bool)
    school[SMALL] = school[LARGE] = True
    assert school.sum() == 34
    cells = SHAPE[0] * SHAPE[1]
    cell = np.concatenate([np.repeat(np.arange(cells), N_SEABED), np.repeat(np.flatnonzero(school.reshape(-1)), N_SCHOOL)])
    member = np.concatenate([np.zeros(cells * N_SEABED, np.int64), np.ones(34 * N_SCHOOL, np.int64)])
    z = np.where(member == 0, SEABED, SCHOOL) + rng.uniform(-0.1, 0.1, cell.size)
    z = (np.rint(z * 65536.0) / 65536.0).astype(np.float32)
    x = ORIGIN[0] + cell % SHAPE[1] + rng.uniform(0.02, 0.98, cell.size)
    y = ORIGIN[1] - (cell // SHAPE[1] + rng.uniform(0.02, 0.98, cell.size))
    p = rng.permutation(cell.size)
    return sc._frozen(x[p], y[p], z[p], cell[p], member[p]) + (school,)


@functools.lru_cache(maxsize=None)
def _want():
    """The restatements composed: robust, by count, the locale guide, by that guide."""
    x, y, z, _, _, _ = _cloud()
    robust = rc.grid(x, y, z, SHAPE, ORIGIN, RES)
    count = hc.grid(robust, GAP_M)
    bits, support = lc.locale_guide(count["n_hyp"], count["chosen"], robust["center2"], RADIUS, MIN_SUPPORT)
    guide = bits.view(np.float32)
    return robust, count, guide, support, hc.grid(robust, GAP_M, "guide", guide)


def _dev(device, *arrays):
    return [torch.from_numpy(np.array(a)).to(device) for a in arrays]


def _host(hyp):
    out = {k: getattr(hyp, k).cpu().numpy() for k in hc.PLANES}
    if hyp.hyp_start is not None:
        out["hyp_start"] = hyp.hyp_start.cpu().numpy().view(np.uint32).astype(np.int64)
        total = int(out["hyp_start"][-1])
        out["hyp_first"] = hyp.hyp_first.cpu().numpy().view(np.uint32).astype(np.int64)[:total]
        out["hyp_count"] = hyp.hyp_count.cpu().numpy()[:total]
    if hyp.guide is not None:
        out["guide"] = hyp.guide.cpu().numpy().view(np.uint32)
        out["support"] = hyp.support.cpu().numpy()
    return out


def _same_bits(got, want, names):
    for k in names:
        g, w = np.asarray(got[k]), np.asarray(want[k])
        assert g.shape == w.shape and g.dtype == w.dtype, (k, g.shape, w.shape, g.dtype, w.dtype)
        assert g.tobytes() == w.tobytes(), (k, np.argwhere(g.view(np.uint8) != w.view(np.uint8))[:4].tolist())


@pytest.fixture(scope="module")
def run(gpu_device):
    from bathymetric_gnn_amd.data import RobustSoundingGridder
    x, y, z, _, _, _ = _cloud()
    g = RobustSoundingGridder(SHAPE, ORIGIN, RES, z.size, device=gpu_device)
    cloud = _dev(gpu_device, x, y, z)
    g.add(*cloud)
    return g, g.finalize(), cloud


def test_schools_over_a_seabed(run, gpu_device):
    from bathymetric_gnn_amd.data import HypothesisGrid, locale_guide
    g, grid, (dx, dy, dz) = run
    x, y, z, cell, member, school = _cloud()
    robust, w_count, w_guide, w_support, w_locale = _want()
    assert np.array_equal(robust["count"], np.where(school, N_SEABED + N_SCHOOL, N_SEABED))
    assert np.array_equal(w_count["n_hyp"], np.where(school, 2, 1))                   # the test's own input: two runs under a school

    by_count = grid.hypotheses(GAP_M)
    _same_bits(_host(by_count), w_count, hc.PLANES + hc.RECORDS)
    assert by_count.guide is None and by_count.support is None
    depth = by_count.depth.cpu().numpy()
    assert (np.abs(depth[school] - SCHOOL) < 0.1).all() and (by_count.kept.cpu().numpy()[school] == N_SCHOOL).all()      # all 34
    assert (np.abs(depth[~school] - SEABED) < 0.1).all()

    hyp = grid.hypotheses(GAP_M, rule="locale", radius=RADIUS, min_support=MIN_SUPPORT)
    assert isinstance(hyp, HypothesisGrid) and hyp.rule == "locale" and hyp.sorted_q is grid.sorted_q and hyp.start is grid.start
    assert (hyp.gap_m, hyp.min_count, hyp.transform, hyp.resolution) == (GAP_M, 1, grid.transform, grid.resolution)
    got = _host(hyp)
    _same_bits(got, w_locale, hc.PLANES + hc.RECORDS)                                 # every cell
    _same_bits(got, {"guide": w_guide.view(np.uint32), "support": w_support}, ("guide", "support"))
    # the 3 x 3 school: every cell on the seabed, with the seabed's soundings and no others
    assert (got["kept"][SMALL] == N_SEABED).all() and (got["chosen"][SMALL] == 0).all()
    assert (np.abs(got["depth"][SMALL] - SEABED) < 0.1).all() and (got["support"][SMALL] >= 16).all()
    flags = g.flag(dx, dy, dz, hyp).cpu().numpy()
    assert np.array_equal(flags, rc.flags(x, y, z, SHAPE, ORIGIN, RES, w_locale["center2"], w_locale["limit"]))
    small = np.zeros(SHAPE, bool)
    small[SMALL] = True
    in_small = small.reshape(-1)[cell]
    assert np.array_equal(flags[in_small] == 0, member[in_small] == 0) and set(flags[in_small].tolist()) == {0, 1}
    # the 5 x 5 school: the centre sees no witness and keeps the count rule's answer; the 24 cells around it are resolved
    r, c = LARGE_CENTRE
    assert got["support"][r, c] == 0 and got["guide"][r, c] == 0x7FC00000
    assert got["kept"][r, c] == N_SCHOOL and got["chosen"][r, c] == 1 and abs(got["depth"][r, c] - SCHOOL) < 0.1
    ring = np.zeros(SHAPE, bool)
    ring[LARGE] = True
    ring[r, c] = False
    assert (got["kept"][ring] == N_SEABED).all() and (got["support"][ring] >= 5).all()
    assert (got["kept"][~school] == N_SEABED).all() and int((got["kept"] == N_SCHOOL).sum()) == 1
    assert torch.equal(hyp.density_plane(), 1.0 / hyp.kept.float())

    # the same from its parts: the guide of a count build, then rule="guide"
    guide, support = locale_guide(grid, by_count, RADIUS, MIN_SUPPORT)
    assert torch.equal(guide.view(torch.int32), hyp.guide.view(torch.int32)) and torch.equal(support, hyp.support)
    by_parts = grid.hypotheses(GAP_M, rule="guide", guide=guide)
    assert by_parts.rule == "guide" and by_parts.guide is None
    _same_bits(_host(by_parts), got, hc.PLANES + hc.RECORDS)
    built, _ = locale_guide(grid, gap_m=GAP_M, radius=RADIUS, min_support=MIN_SUPPORT)            # hyp=None: a count build of its own
    assert torch.equal(built.view(torch.int32), guide.view(torch.int32))
    defaults = grid.hypotheses(GAP_M, rule="locale", records=False)                               # radius 2, min_support 3
    assert defaults.hyp_start is None
    _same_bits(_host(defaults), got, hc.PLANES + ("guide", "support"))
    # a wider window reaches past the 5 x 5 school: radius 3 resolves its centre as well
    wide = grid.hypotheses(GAP_M, rule="locale", radius=3, min_support=3, records=False)
    assert int((wide.kept == N_SCHOOL).sum()) == 0 and int(wide.support[r, c]) == 24


def test_order_and_split(run, gpu_device):
    """The cloud permuted, and in a three-call split: equal bytes in every output of the locale rule."""
    from bathymetric_gnn_amd.data import RobustSoundingGridder
    _, grid, (dx, dy, dz) = run
    first = _host(grid.hypotheses(GAP_M, rule="locale"))
    perm = torch.from_numpy(np.random.default_rng(9).permutation(int(dz.shape[0]))).to(gpu_device)
    for cuts, order in (((0, int(dz.shape[0])), perm), ((0, 7001, 7002, int(dz.shape[0])), None), ((0, 4097, 12000, int(dz.shape[0])), perm)):
        g = RobustSoundingGridder(SHAPE, ORIGIN, RES, int(dz.shape[0]), device=gpu_device)
        cx, cy, cz = (dx, dy, dz) if order is None else (dx[order], dy[order], dz[order])
        for lo, hi in zip(cuts[:-1], cuts[1:]):
            g.add(cx[lo:hi], cy[lo:hi], cz[lo:hi])
        other = _host(g.finalize().hypotheses(GAP_M, rule="locale"))
        assert other.keys() == first.keys()
        _same_bits(other, first, first.keys())


def test_refusals(run, gpu_device):
    from bathymetric_gnn_amd.data import RobustVRSoundingGridder, VRLayout, locale_guide
    _, grid, (dx, dy, dz) = run
    guide = torch.zeros(SHAPE, dtype=torch.float32, device=gpu_device)
    with pytest.raises(ValueError, match="takes none"):
        grid.hypotheses(GAP_M, rule="locale", guide=guide)
    for rule, kw in (("count", dict(radius=2)), ("count", dict(min_support=3)), ("guide", dict(guide=guide, radius=2))):
        with pytest.raises(ValueError, match='go with rule="locale"'):
            grid.hypotheses(GAP_M, rule=rule, **kw)
    for kw in (dict(radius=0), dict(radius=9), dict(min_support=0), dict(min_support=25), dict(radius=1, min_support=9)):
        with pytest.raises(ValueError, match="radius|min_support"):
            grid.hypotheses(GAP_M, rule="locale", **kw)
    with pytest.raises(TypeError, match="integer"):
        grid.hypotheses(GAP_M, rule="locale", radius=2.0)
    with pytest.raises(ValueError, match="rule"):
        grid.hypotheses(GAP_M, rule="nearest")
    with pytest.raises(ValueError, match="gap_m"):
        locale_guide(grid)
    by_count = grid.hypotheses(GAP_M, records=False)
    with pytest.raises(ValueError, match="gap_m"):
        locale_guide(grid, by_count, gap_m=GAP_M)
    with pytest.raises(TypeError, match="HypothesisGrid"):
        locale_guide(grid, by_count.n_hyp)
    with pytest.raises(TypeError, match="RobustSoundingGrid"):
        locale_guide(by_count, by_count)
    # variable resolution: the rule is for uniform grids
    x, y, z, _, _, _ = _cloud()
    d = np.where(np.add.outer(np.arange(6), np.arange(6)) % 2 == 0, 4, 2)
    lay = vc.make_layout((6, 6), (ORIGIN[0], ORIGIN[1] - 24.0), 4.0, d, d)
    layout = VRLayout(lay["base_shape"], lay["origin"], lay["B"], lay["index"], lay["dx"], lay["dy"], lay["total"], device=gpu_device)
    vg = RobustVRSoundingGridder(layout, z.size)
    vg.add(dx, dy, dz)
    vgrid = vg.finalize()
    with pytest.raises(ValueError, match="uniform grids"):
        vgrid.hypotheses(GAP_M, rule="locale")
    with pytest.raises(TypeError, match="RobustSoundingGrid"):
        locale_guide(vgrid, gap_m=GAP_M)
    assert int(vgrid.hypotheses(GAP_M).n_hyp.max()) == 2                               # (the other rules are as they were)
