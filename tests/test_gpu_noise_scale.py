"""Synthetic training noise at the tile sizes training uses (csrc/synthetic_noise.hip; the trainer cuts 512 x 512 tiles, Config
tiles at 1024), against float64 / bit-exact restatements in numpy (tests/_noise_cpu.py).

tests/test_gpu_noise.py compares tiles of fewer than 16 384 cells: there the strided loops of the statistics passes make at most
one trip per workgroup, and the rank-select of the blob centres has one run of 256 cells per strip.  The tiles here reach the
other paths -- several trips, strips of 2 .. 16 runs, strips without a valid cell, the final partial run, surplus workgroups in
a ragged batch -- with inputs under which a wrong result cannot hide:
  1. blobs of size 1: the marked cells ARE the selected centres, and their values are depth_range, bit for bit;
  2. a gradient_x artifact of amplitude factor 1: the last column's magnitude IS depth_std, held to one ulp of a longdouble
     two-pass standard deviation;
  3. an injected uniform field that sits a few float32 ulps beside the density map at every cell, so that every valid cell
     reports its local_std;
  4. the device's own draws under the rule of ``check_outputs`` with the bounds of tests/test_gpu_noise.py.
The inputs, their categories and the near-threshold counts are checked on the host by tests/test_host_noise.py.
"""
import functools

import numpy as np
import pytest

import _noise_cpu as nc
from _conditioning import BOUND_C
from test_gpu_noise import _params, _split, _upload

from bathymetric_gnn_amd import synthetic
from bathymetric_gnn_amd.data import SyntheticNoiseGenerator

pytestmark = pytest.mark.gpu

OFF = dict(enable_gaussian=False, enable_spikes=False, enable_blobs=False, enable_systematic=False)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32) if a.dtype == np.float32 else a


def _check_exact(out, want, label):
    """Every output bit for bit: ``want`` = (noisy f32, mask bool, magnitude f32); classification is 2 x mask."""
    noisy, mask, mag, cls = out
    assert noisy.dtype == np.float32 and mask.dtype == bool and mag.dtype == np.float32 and cls.dtype == np.int64, label
    diff = mask != want[1]
    assert not diff.any(), f"{label}: noise_mask differs at {int(diff.sum())} cells, first {np.argwhere(diff)[:4].tolist()}"
    for name, a, b in (("noisy_depth", noisy, want[0]), ("noise_magnitude", mag, want[2])):
        bad = _bits(a) != _bits(b)
        assert not bad.any(), f"{label}: {name} differs in its bits at {int(bad.sum())} cells, first {np.argwhere(bad)[:4].tolist()}"
    assert np.array_equal(cls, np.where(want[1], 2, 0)), label


# ---- 1. blob centres, exactly ---------------------------------------------------------------------------------------------------------
def _unit_blobs(tiles, dev):
    """[(depth, valid, us)] -> per tile outputs of a blobs-only generator with one size-1 blob of magnitude draw 1.0 per u."""
    gen = SyntheticNoiseGenerator(**{**OFF, "enable_blobs": True}, seed=1)
    hw, depth_t, mask_t = _upload([(d, v) for d, v, _ in tiles], dev)
    b = gen.generate_batch(hw, depth_t, mask_t, [1.0] * len(tiles), [{"blobs": [(-1, u, 1, 1.0) for u in us]} for _, _, us in tiles])
    return _split(b)


@functools.lru_cache(maxsize=None)
def _centre(i):
    name, depth, valid, us = nc.centre_case(i)
    return name, depth, valid, us, nc.expected_unit_blobs(depth, valid, us)


@pytest.mark.parametrize("i", range(len(nc.CENTRE_NAMES)), ids=nc.CENTRE_NAMES)
def test_blob_centres_of_one_tile(i, gpu_device):
    name, depth, valid, us, want = _centre(i)
    out = _unit_blobs([(depth, valid, us)], gpu_device)[0]
    assert int(out[1].sum()) == len({nc.kth_valid_cell(valid, u) for u in us}) if valid.any() else not out[1].any()
    _check_exact(out, want, name)


def test_blob_centres_of_the_ragged_batch(gpu_device):
    """All the tiles as one batch: the 272-cell and 77-cell tiles put every later tile at an offset that is no multiple of 256
    or 4, and the tile without a valid cell returns early with a non-empty blob list between tiles that have one."""
    cases = [_centre(i) for i in range(len(nc.CENTRE_NAMES))]
    offsets = np.cumsum([c[1].size for c in cases])[2:-1]
    assert (offsets % 4 != 0).all() and (offsets % 256 != 0).all() and cases[-1][1].size == 1024 * 1024
    assert not cases[5][2].any() and len(cases[5][3]) > 0 and cases[6][2].any()
    assert len(cases[0][3]) >= 700
    for c, out in zip(cases, _unit_blobs([c[1:4] for c in cases], gpu_device)):
        _check_exact(out, c[4], "batch, " + c[0])


# ---- 2. per-tile scalars past one trip ------------------------------------------------------------------------------------------------
def _ulps(a, b):
    return abs(int(np.float32(a).view(np.int32)) - int(np.float32(b).view(np.int32)))          # (both positive)


def _check_scalars(tiles, dev):
    """depth_range from unit blobs, depth_std from the last column of a gradient_x artifact.  Returns the ulp distances of
    depth_std to the longdouble reference."""
    us = [0.0, 0.5, 0.75, 1.0]
    for (name, depth, valid), out in zip(tiles, _unit_blobs([(d, v, us) for _, d, v in tiles], dev)):
        want = nc.expected_unit_blobs(depth, valid, us)
        assert float(want[3]) > 0
        _check_exact(out, want[:3], f"depth_range, {name}")
    gen = SyntheticNoiseGenerator(**{**OFF, "enable_systematic": True}, seed=1)
    hw, depth_t, mask_t = _upload([(d, v) for _, d, v in tiles], dev)
    b = gen.generate_batch(hw, depth_t, mask_t, [1.0] * len(tiles), [{"artifact": "gradient_x", "amplitude_factor": 1.0}] * len(tiles))
    dist = []
    for (name, depth, valid), out in zip(tiles, _split(b)):
        noisy, mask, mag, cls = out
        last = mag[:, -1][valid[:, -1]]
        assert len(last) > 0 and (_bits(last) == _bits(last[:1])).all(), f"{name}: the last column does not hold one amplitude"
        amp, ref = last[0], nc.longdouble_std32(depth, valid)
        dist.append(_ulps(amp, ref))
        print(f"depth_std, {name}: device {amp!r}, longdouble two-pass {ref!r}, {dist[-1]} ulp apart")
        assert dist[-1] <= 1, f"{name}: depth_std {amp!r} is {dist[-1]} ulp from {ref!r}"
        # every other column from the device's own amplitude, bit for bit
        a32 = (np.float64(amp) * nc.linspace_pm1(depth.shape[1])).astype(np.float32)[None, :]
        with np.errstate(invalid="ignore"):
            want_noisy = np.where(valid, depth + a32, depth)
        want = (want_noisy, valid & (np.abs(a32) > amp * np.float32(0.5)), np.where(valid, np.abs(a32), np.float32(0)))
        _check_exact(out, want, f"gradient_x, {name}")
    return dist


@pytest.mark.parametrize("i", range(len(nc.SCALAR_NAMES)), ids=nc.SCALAR_NAMES)
def test_tile_scalars_after_ten_trips(i, gpu_device):
    """300 x 517 at -4000 m with centimetre relief; 30 of the 64 workgroups of a statistics pass make a tenth trip, and the
    extrema lie in cells only that trip reads.  depth_std sums in float64 on both sides (error over 155 100 terms far below
    2^-24 relative), so only a rounding boundary can separate it from the longdouble value: at most 1 ulp.  Measured on an
    MI355X: 0 ulp on all three tiles."""
    _check_scalars([nc.scalar_tiles()[i]], gpu_device)


def test_tile_scalars_in_a_batch(gpu_device):
    """The three tiles behind a 272-cell one (measured on an MI355X: 0 ulp each)."""
    first = ("17x16", synthetic.synthetic_tile(17, 16, 2, "V0")[0], np.ones((17, 16), bool))
    _check_scalars([first] + list(nc.scalar_tiles()), gpu_device)


# ---- 3. complexity probe for noise_local_std --------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _probes():
    out = []
    for name, depth, valid in nc.probe_tiles():
        fields, delta, ref, want = nc.complexity_probe(depth, valid, BOUND_C)
        assert delta < 1e-4 and np.array_equal(ref[1], want), name
        out.append((name, depth, valid, fields, ref, want))
    return out


def _check_probe(cases, dev):
    gen = SyntheticNoiseGenerator(**{**OFF, "enable_spikes": True}, complexity_correlation=nc.PROBE_CC, seed=1)
    hw, depth_t, mask_t = _upload([(c[1], c[2]) for c in cases], dev)
    b = gen.generate_batch(hw, depth_t, mask_t, [1.0] * len(cases), [{"spike_density_draw": nc.PROBE_DENSITY, **c[3]} for c in cases])
    for (name, depth, valid, fields, ref, want), out in zip(cases, _split(b)):
        flips = out[1] != want
        print(f"probe, {name}: {int(flips.sum())} of {int(valid.sum())} valid cells off the chessboard")
        _check_exact(out, ref[:3], "probe, " + name)


def test_complexity_probe_ragged_batch(gpu_device):
    """Every valid cell spikes exactly on the -1 squares; the largest tile sets the grid of noise_local_std, so the surplus
    workgroups of the smaller tiles must exit."""
    _check_probe(_probes(), gpu_device)


def test_complexity_probe_largest_tile_alone(gpu_device):
    _check_probe(_probes()[-1:], gpu_device)


# ---- 4. own draws against the restatement at real sizes ----------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _own_reference(h, w, tile_seed, variant, no_valid, gen_seed, sample):
    depth, valid = synthetic.synthetic_tile(h, w, tile_seed, variant)[:2]
    if no_valid:
        valid = np.zeros_like(valid)
    gen = SyntheticNoiseGenerator(seed=gen_seed)
    return depth, valid, nc.own_reference(depth, valid, gen.draw_plan(sample, 1.0), _params(gen), gen.seed)


def _check_own(out, key, plan, label):
    depth, valid, (ref, scale) = _own_reference(*key)
    gen = SyntheticNoiseGenerator(seed=key[5])
    assert plan == gen.draw_plan(key[6], 1.0)
    rep = nc.check_outputs(out, depth, valid, ref[4], ref[0].astype(np.float64), ref[1], ref[2], ref[3],
                           BOUND_C * nc.EPS32 * scale, BOUND_C * nc.EPS32, label)
    if valid.any():
        assert ref[1].any() and out[1].any()
    print(f"{label}: {rep}")
    return rep


@pytest.mark.parametrize("h,w,tile_seed,gen_seed", nc.OWN_CASES, ids=[f"{c[0]}x{c[1]}" for c in nc.OWN_CASES])
def test_own_draws_at_training_sizes(h, w, tile_seed, gen_seed, gpu_device):
    key = (h, w, tile_seed, "V1", False, gen_seed, 0)
    depth, valid, _ = _own_reference(*key)
    gen = SyntheticNoiseGenerator(seed=gen_seed)
    hw, depth_t, mask_t = _upload([(depth, valid)], gpu_device)
    b = gen.generate_batch(hw, depth_t, mask_t, [1.0])
    _check_own(_split(b)[0], key, b.plans[0], f"own draws, {h}x{w}")


def test_own_draws_ragged_batch_and_alone(gpu_device):
    """260 x 253, 17 x 16, a tile without a valid cell, 300 x 517 and 1 x 40 as one batch; the 300 x 517 tile, at a cell offset
    that is no multiple of 256, has the bits it has alone."""
    tiles = nc.own_batch_tiles()
    keys = [(260, 253, 3, "V1", False), (17, 16, 5, "V1", False), (64, 64, 1, "V1", True), (300, 517, 4, "V1", False), (1, 40, 6, "V0", False)]
    keys = [k + (nc.OWN_BATCH_SEED, s) for k, s in zip(keys, nc.OWN_BATCH_SAMPLES)]
    for (d, v), k in zip(tiles, keys):
        rd, rv, _ = _own_reference(*k)
        assert np.array_equal(_bits(d), _bits(rd)) and np.array_equal(v, rv)
    hw, depth_t, mask_t = _upload(tiles, gpu_device)
    assert int(hw[:3, 0].astype(np.int64) @ hw[:3, 1]) % 256 != 0
    b = SyntheticNoiseGenerator(seed=nc.OWN_BATCH_SEED).generate_batch(hw, depth_t, mask_t, sample_indices=list(nc.OWN_BATCH_SAMPLES))
    outs = _split(b)
    for out, k, plan in zip(outs, keys, b.plans):
        _check_own(out, k, plan, f"own draws in a batch, {k[0]}x{k[1]}")
    assert np.array_equal(_bits(outs[2][0]), _bits(tiles[2][0])) and not outs[2][1].any() and not outs[2][3].any()
    h1, d1, m1 = _upload([tiles[3]], gpu_device)
    alone = _split(SyntheticNoiseGenerator(seed=nc.OWN_BATCH_SEED).generate_batch(h1, d1, m1, sample_indices=[0]))[0]
    for x, y in zip(alone, outs[3]):
        assert np.array_equal(_bits(x), _bits(y))
