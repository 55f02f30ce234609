"""Survey geometry on the host (models/survey.py): SurveyTilePlan against a restatement from TileManager's specs, the band / ring
arithmetic of the streamed route as properties, the blend tables against _create_1d_blend, and the min_valid_ratio rule against
Tile.valid_ratio.  Needs no device and no library."""
import inspect
import re

import numpy as np
import pytest

from bathymetric_gnn_amd.data import TileManager
from bathymetric_gnn_amd.data.tiling import Tile
from bathymetric_gnn_amd.models import survey
from bathymetric_gnn_amd.models.survey import SurveyTilePlan, keep_from_counts

SHAPES = [(64, 16, (700, 611)), (64, 16, (500, 430)), (64, 16, (200, 170)), (64, 16, (40, 50)), (64, 16, (64, 64)), (64, 16, (65, 64)),
          (1024, 128, (2500, 1100))]


def _plan(tile, overlap, shape):
    tm = TileManager(tile, overlap, 0.1)
    return tm, SurveyTilePlan(tm, shape)


@pytest.mark.parametrize("tile,overlap,shape", SHAPES)
def test_plan_fields_equal_the_specs(tile, overlap, shape):
    tm, p = _plan(tile, overlap, shape)
    ntr, ntc, specs = tm.compute_tile_grid(shape)
    assert (p.H, p.W) == shape and (p.ntr, p.ntc) == (ntr, ntc) and len(specs) == ntr * ntc
    assert (p.th, p.tw) == (min(tile, shape[0]), min(tile, shape[1]))
    assert p.cells == p.th * p.tw and p.pitch == max(p.th, p.tw)
    assert all(a.dtype == np.int64 for a in (p.rs, p.re, p.cs, p.ce)) and (len(p.rs), len(p.cs)) == (ntr, ntc)
    assert p.origins.dtype == np.int32 and p.origins.shape == (ntr * ntc, 2) and p.origins.flags.c_contiguous
    for k, s in enumerate(specs):                                   # spec order: tile row major
        assert (s.tile_row, s.tile_col) == divmod(k, ntc)
        assert (s.row_end - s.row_start, s.col_end - s.col_start) == (p.th, p.tw)
        assert (p.rs[s.tile_row], p.re[s.tile_row], p.cs[s.tile_col], p.ce[s.tile_col]) == (s.row_start, s.row_end, s.col_start, s.col_end)
        assert tuple(p.origins[k]) == (s.row_start, s.col_start)
    if shape == (700, 611):                                         # the last tile is shifted back on both axes
        stride = tile - overlap
        assert p.rs[-1] == 700 - 64 != (ntr - 1) * stride and p.cs[-1] == 611 - 64 != (ntc - 1) * stride
    # rows_touching: the tile rows that hold at least one of the rows
    for R0, R1 in [(0, 1), (0, shape[0]), (shape[0] - 1, shape[0]), (shape[0] // 3, shape[0] // 2 + 1)]:
        want = [t for t in range(ntr) if any(p.rs[t] <= r < p.re[t] for r in range(R0, R1))]
        assert p.rows_touching(R0, R1).tolist() == want
    assert p.reach == max(sum(1 for u in range(t) if p.re[u] > p.rs[t]) for t in range(ntr))


def test_tiles_of_unequal_extent_are_refused():
    class Uneven(TileManager):
        def compute_tile_grid(self, shape):
            ntr, ntc, specs = super().compute_tile_grid(shape)
            specs[-1].col_start += 1
            return ntr, ntc, specs
    with pytest.raises(ValueError, match="differ in extent"):
        SurveyTilePlan(Uneven(64, 16, 0.1), (200, 170))


@pytest.mark.parametrize("tile,overlap,shape", SHAPES)
def test_bands_partition_the_survey_and_stay_in_the_ring(tile, overlap, shape):
    _, p = _plan(tile, overlap, shape)
    for nb in (1, 2, 3, p.ntr + 3):
        K = p.ring_slots(nb)
        assert K == min(p.ntr, nb + p.reach)
        bands = p.bands(nb)
        assert [b[0] for b in bands] == [(a, min(a + nb, p.ntr)) for a in range(0, p.ntr, nb)]
        edge = 0
        for (ta, tb), (R0, R1) in bands:
            assert R0 == edge and R1 >= R0                          # the final rows partition [0, H) in order
            edge = R1
            assert all(p.rs[t] >= R1 for t in range(tb, p.ntr))    # no later tile row touches them
            if R1 > R0:
                inv = p.rows_touching(R0, R1)
                assert len(inv) and inv.max() < tb and inv.min() > tb - 1 - K      # the ring invariant of the streamed route
        assert edge == p.H


@pytest.mark.parametrize("tile,overlap,shape", SHAPES)
def test_blend_tables_equal_create_1d_blend(tile, overlap, shape):
    tm, p = _plan(tile, overlap, shape)
    cw = p.col_weights
    assert cw.shape == (p.ntc, p.pitch) and cw.dtype == np.float32
    for j in range(p.ntc):
        n = int(p.ce[j] - p.cs[j])
        assert np.array_equal(cw[j, :n], tm._create_1d_blend(n)) and not cw[j, n:].any()
    rows = np.arange(p.ntr)[::-1][:3]                               # any subset, any order
    R0 = int(p.rs[rows.min()]) + 5
    rs_b, re_b, rw = p.stitch_tables(rows, R0)
    assert rs_b.dtype == np.int32 and re_b.dtype == np.int32 and rw.shape == (len(rows), p.pitch) and rw.dtype == np.float32
    assert np.array_equal(rw, p.row_weights(rows))
    for i, t in enumerate(rows):
        n = int(p.re[t] - p.rs[t])
        assert (rs_b[i], re_b[i]) == (p.rs[t] - R0, p.re[t] - R0)
        assert np.array_equal(rw[i, :n], tm._create_1d_blend(n)) and not rw[i, n:].any()


@pytest.mark.parametrize("ratio", [0.1, 0.3, 1 / 3])
def test_keep_rule_equals_the_tile_valid_ratio_test(ratio):
    cells = 64 * 64
    counts = np.arange(cells + 1)
    order = np.arange(cells).reshape(64, 64)
    z = np.zeros((64, 64), np.float32)
    want = [not (Tile(z, None, 0, 0, 64, 64, 0, 0, order < c).valid_ratio < ratio) for c in counts]      # iterate_tiles skips on `<`
    got = keep_from_counts(counts, cells, ratio)
    assert got.dtype == bool and got.tolist() == want
    assert 0 < got.sum() < len(got)


def test_survey_rows_of_rank_spans_the_rank_s_tile_rows():
    from bathymetric_gnn_amd.models.pipeline import BathymetricPipeline, survey_shard_plan
    pipe = BathymetricPipeline.__new__(BathymetricPipeline)
    pipe.tile_manager = TileManager(64, 16, 0.3)
    ntr, ntc, specs = pipe.tile_manager.compute_tile_grid((700, 611))
    rs = [specs[i * ntc].row_start for i in range(ntr)]; re_ = [specs[i * ntc].row_end for i in range(ntr)]
    for world in (1, 2, 3, ntr + 2):
        want = survey_shard_plan(rs, re_, 700, world)
        for rank in range(world):
            (lo, hi), plan = pipe.survey_rows_of_rank((700, 611), rank, world)
            assert plan == want
            ta, tb = want[rank]["tile_rows"]
            assert (lo, hi) == ((rs[ta], re_[tb - 1]) if tb > ta else (0, 0))


def test_no_assert_guards_the_survey_routes():
    """Argument checks and invariants of the survey routes raise: ``python -O`` must not remove them."""
    from bathymetric_gnn_amd.models.pipeline import BathymetricPipeline
    for src in (inspect.getsource(survey), inspect.getsource(BathymetricPipeline.process_survey_device),
                inspect.getsource(BathymetricPipeline.process_grid_streamed)):
        assert not re.search(r"^\s*assert\b", src, re.M)
