"""Synthetic training noise on the GPU (data/synthetic_noise.py, csrc/synthetic_noise.hip).

Parity with the REFERENCE runs with injected draws: the fixtures of tests/golden/noise hold every draw the reference's generator
made and its outputs on the float32 tile (ref32) and on the float64 copy of it (ref64).  The rule (tests/_noise_cpu.py,
``check_outputs``): ``noisy_depth`` within BOUND_C x max |ref32 - ref64| of ref64, separately over spike cells, blob cells and the
rest; ``noise_magnitude`` within BOUND_C x (r + eps32) of ref32 relatively, r the relative distance of the fixture's float32 and
float64 ``std``; ``noise_mask`` / ``classification`` equal except where a float64 evaluation of the compared quantity lies within
the noisy_depth bound of its threshold (at most 0.1 % of the valid cells; blob membership without exception); invalid cells
bit-identical to the input.

The device's own draws are held against the numpy restatement (pinned against the reference by tests/test_host_noise.py) driven
by the documented generator with the same seed, under the same rule.  No ref32 / ref64 pair exists there, so the bounds come
from the number formats: both sides run the same float32 / float64 operation sequence and differ by the last bit of the float64
library functions (log, cos, exp, sin) and by the order of the float64 sums, which moves a float32 rounding of the running depth
by at most one ulp: noisy_depth bound = BOUND_C x eps32 x max |noisy_depth|, magnitude bound = BOUND_C x eps32.
"""
import glob
import math
import os

import numpy as np
import pytest
import torch

import _noise_cpu as nc
from _conditioning import BOUND_C

from bathymetric_gnn_amd import synthetic
from bathymetric_gnn_amd.config.constants import CORRECTION_NORM_CAP, CORRECTION_NORM_FLOOR
from bathymetric_gnn_amd.data import GraphBuilder, NoiseAugmentor, NoiseLabel, SyntheticNoiseGenerator, training_targets
from bathymetric_gnn_amd.models import BathymetricGNN

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURES = sorted(glob.glob(os.path.join(ROOT, "tests", "golden", "noise", "*.npz")))
NAMES = [os.path.basename(p)[:-4] for p in FIXTURES]
DEFAULT_BATCH = [n for n in NAMES if n.startswith(("all_", "holes", "intensity_"))]       # fixtures made with the default generator


def _generator(params, seed=0):
    return SyntheticNoiseGenerator(enable_gaussian=params["enable_gaussian"], enable_spikes=params["enable_spikes"],
                                   enable_blobs=params["enable_blobs"], enable_systematic=params["enable_systematic"],
                                   complexity_correlation=params["complexity_correlation"],
                                   spike_magnitude_range=tuple(params["spike_magnitude_range"]), seed=seed)


def _draws(plan, fields, z):
    d = {"gaussian_std_factor": plan["gaussian_std_factor"], "spike_density_draw": float(z["scalars"][1]), "blobs": plan["blobs"],
         "artifact": plan["artifact"], "amplitude_factor": plan["amplitude_factor"], "freq_a": plan["freq_a"],
         "freq_b": plan["freq_b"], "phase": plan["phase"]}
    d.update(fields)
    return d


def _upload(tiles, dev, with_mask=True):
    """[(depth f32 [h, w], valid bool)] -> hw, flat depth tensor, flat mask tensor."""
    hw = np.array([d.shape for d, _ in tiles], np.int32)
    depth_t = torch.from_numpy(np.concatenate([np.ascontiguousarray(d, np.float32).ravel() for d, _ in tiles])).to(dev)
    mask_t = torch.from_numpy(np.concatenate([v.ravel() for _, v in tiles]).view(np.uint8)).to(dev) if with_mask else None
    return hw, depth_t, mask_t


def _split(batch):
    """NoiseBatch -> per tile (noisy, mask, magnitude, classification) numpy arrays [h, w]."""
    out, off = [], 0
    n, m, g, c = (t.cpu().numpy() for t in (batch.noisy_depth, batch.noise_mask, batch.noise_magnitude, batch.classification))
    for h, w in batch.hw:
        k = int(h) * int(w)
        out.append(tuple(a[off:off + k].reshape(int(h), int(w)) for a in (n, m, g, c)))
        off += k
    return out


def _cpu_plan(p):
    q = dict(p)
    q["spike_density"] = float(p["spike_density_draw"]) * p["intensity"]
    q["artifact"] = nc.ARTIFACTS.index(p["artifact"])
    return q


def _params(g):
    return {"enable_gaussian": g.enable_gaussian, "enable_spikes": g.enable_spikes, "enable_blobs": g.enable_blobs,
            "enable_systematic": g.enable_systematic, "complexity_correlation": g.complexity_correlation,
            "spike_magnitude_range": g.spike_magnitude_range}


def _tile(h, w, seed, variant="V1"):
    d, m, _ = synthetic.synthetic_tile(h, w, seed, variant)
    return d, m


# ---- parity with the reference, injected draws --------------------------------------------------------------------------------------
@pytest.mark.parametrize("path", FIXTURES, ids=NAMES)
def test_parity_with_injected_draws(path, gpu_device):
    depth, valid, plan, params, fields, z = nc.load_fixture(path)
    gen = _generator(params)
    hw, depth_t, mask_t = _upload([(depth, valid)], gpu_device, with_mask=not bool(z["mask_none"]))
    b = gen.generate_batch(hw, depth_t, mask_t, [plan["intensity"]], [_draws(plan, fields, z)])
    nc.check_fixture(_split(b)[0], path, BOUND_C)


def test_parity_of_a_ragged_batch_with_injected_draws(gpu_device):
    """The default-generator fixtures (64 x 48 and 48 x 40 tiles, three intensities, holes) as ONE batch."""
    loaded = [nc.load_fixture(FIXTURES[NAMES.index(n)]) for n in DEFAULT_BATCH]
    assert len(loaded) >= 9 and len({l[0].shape for l in loaded}) >= 2
    gen = _generator(loaded[0][3])
    hw, depth_t, mask_t = _upload([(l[0], l[1]) for l in loaded], gpu_device)
    b = gen.generate_batch(hw, depth_t, mask_t, [l[2]["intensity"] for l in loaded], [_draws(l[2], l[4], l[5]) for l in loaded])
    for n, out in zip(DEFAULT_BATCH, _split(b)):
        nc.check_fixture(out, FIXTURES[NAMES.index(n)], BOUND_C)


# ---- own draws against the restatement ----------------------------------------------------------------------------------------------
def _check_own(gen, tiles, batch):
    """(The near-threshold count of ``check_outputs`` is a property of the inputs: the tiles and seeds below were chosen so that
    it stays under 0.1 % of the valid cells, which needs tiles of a few thousand cells or, for the tiny ones, no such cell.)"""
    for (depth, valid), plan, out in zip(tiles, batch.plans, _split(batch)):
        ref = nc.generate(depth, valid, _cpu_plan(plan), _params(gen), seed=gen.seed)
        info = ref[4]
        info.setdefault("blob_cells", np.zeros(valid.shape, bool))
        scale = float(np.abs(ref[0][valid]).max()) if valid.any() else 0.0
        rep = nc.check_outputs(out, depth, valid, info, ref[0].astype(np.float64), ref[1], ref[2], ref[3],
                               BOUND_C * nc.EPS32 * scale, BOUND_C * nc.EPS32, f"own draws, sample {plan['sample']}")
        if valid.any():           # the blob centres the device selected are the restatement's
            assert ref[1].any() and out[1].any()


def test_own_draws_one_tile(gpu_device):
    gen = SyntheticNoiseGenerator(seed=2024)
    tiles = [_tile(96, 80, 3)]
    assert not tiles[0][1].all()
    hw, depth_t, mask_t = _upload(tiles, gpu_device)
    _check_own(gen, tiles, gen.generate_batch(hw, depth_t, mask_t, [1.0]))


def test_own_draws_batch_of_unequal_tiles(gpu_device):
    gen = SyntheticNoiseGenerator(seed=77)
    tiles = [_tile(64, 64, 1), _tile(72, 88, 3), _tile(120, 50, 4, "V0"), _tile(17, 16, 5), _tile(1, 40, 6, "V0")]
    tiles.append((tiles[0][0].copy(), np.zeros((64, 64), bool)))          # a tile without a valid cell, mid-batch semantics
    tiles.append(_tile(70, 90, 8))
    hw, depth_t, mask_t = _upload(tiles, gpu_device)
    b = gen.generate_batch(hw, depth_t, mask_t, [0.5, 1.0, 1.5, 1.0, 1.0, 1.0, 2.0])
    assert b.sample_indices == list(range(7)) and gen.next_sample == 7
    _check_own(gen, tiles, b)
    empty = _split(b)[5]
    assert np.array_equal(empty[0].view(np.uint32), tiles[5][0].view(np.uint32)) and not empty[1].any() and not empty[3].any()


# ---- statistics of own draws --------------------------------------------------------------------------------------------------------
def test_statistics_of_own_draws_on_a_512_tile(gpu_device):
    depth, valid = _tile(512, 512, 21)
    hw, depth_t, mask_t = _upload([(depth, valid)], gpu_device)
    off = dict(enable_gaussian=False, enable_spikes=False, enable_blobs=False, enable_systematic=False)
    nv = int(valid.sum())
    # spikes alone: every marked cell is a spike
    gen = SyntheticNoiseGenerator(**{**off, "enable_spikes": True}, seed=5)
    b = gen.generate_batch(hw, depth_t, mask_t, [1.0])
    count = int(b.noise_mask.sum())
    info = nc.generate(depth, valid, _cpu_plan(b.plans[0]), _params(gen), seed=gen.seed)[4]
    p = info["density"].astype(np.float64)[valid]
    want, sd = float(p.sum()), math.sqrt(float((p * (1 - p)).sum()))
    print(f"spikes: {count} on the device, {want:.1f} +- {sd:.1f} expected from the density map")
    assert abs(count - want) <= 5 * sd
    # Gaussian alone: a cell is marked where |z| > 2
    gen = SyntheticNoiseGenerator(**{**off, "enable_gaussian": True}, seed=6)
    b = gen.generate_batch(hw, depth_t, mask_t, [1.0])
    share = float(b.noise_mask.sum()) / nv
    p2 = math.erfc(2 / math.sqrt(2))
    print(f"Gaussian: share marked {share:.5f}, P(|z| > 2) = {p2:.5f}")
    assert abs(share - p2) <= 5 * math.sqrt(p2 * (1 - p2) / nv)


# ---- determinism ----------------------------------------------------------------------------------------------------------------------
def _same(a, b):
    return all(torch.equal(x.view(torch.int32) if x.dtype == torch.float32 else x, y.view(torch.int32) if y.dtype == torch.float32 else y)
               for x, y in ((a.noisy_depth, b.noisy_depth), (a.noise_mask, b.noise_mask), (a.noise_magnitude, b.noise_magnitude),
                            (a.classification, b.classification)))


def test_same_seed_gives_the_same_bits(gpu_device):
    tiles = [_tile(64, 64, s) for s in range(4)]
    hw, depth_t, mask_t = _upload(tiles, gpu_device)
    a = SyntheticNoiseGenerator(seed=9).generate_batch(hw, depth_t, mask_t)
    b = SyntheticNoiseGenerator(seed=9).generate_batch(hw, depth_t, mask_t)
    c = SyntheticNoiseGenerator(seed=10).generate_batch(hw, depth_t, mask_t)
    assert _same(a, b) and not _same(a, c) and bool(a.noise_mask.any())


def test_sample_is_the_same_in_a_batch_and_alone(gpu_device):
    tiles = [_tile(48 + 4 * (s % 3), 64, s) for s in range(16)]
    hw, depth_t, mask_t = _upload(tiles, gpu_device)
    gen = SyntheticNoiseGenerator(seed=31)
    aug = NoiseAugmentor(gen, seed=4)
    whole = aug.augment_batch(hw, depth_t, mask_t)
    assert whole.sample_indices == list(range(16)) and len({p["intensity"] for p in whole.plans}) == 16
    parts = _split(whole)
    for i in (0, 7, 15):
        h1, d1, m1 = _upload([tiles[i]], gpu_device)
        alone = _split(aug.augment_batch(h1, d1, m1, sample_indices=[i]))[0]
        for x, y in zip(alone, parts[i]):
            assert np.array_equal(x.view(np.uint32) if x.dtype == np.float32 else x, y.view(np.uint32) if y.dtype == np.float32 else y), i


# ---- scale ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,side", [(16, 256), (4, 512)])
def test_scale(n, side, gpu_device):
    tiles = [_tile(side, side, 40 + s) for s in range(n)]
    hw, depth_t, mask_t = _upload(tiles, gpu_device)
    b = SyntheticNoiseGenerator(seed=1).generate_batch(hw, depth_t, mask_t)
    valid = mask_t.bool()
    assert b.noisy_depth.shape == depth_t.shape and b.noisy_depth.dtype == torch.float32 and b.classification.dtype == torch.int64
    assert bool(torch.isfinite(b.noisy_depth[valid]).all()) and bool(torch.isfinite(b.noise_magnitude).all())
    assert not bool((b.noise_mask & ~valid).any())
    assert set(torch.unique(b.classification).tolist()) == {0, 2}
    assert torch.equal(b.classification == 2, b.noise_mask)
    assert torch.equal(b.noisy_depth.view(torch.int32)[~valid], depth_t.view(torch.int32)[~valid])
    share = float(b.noise_mask.sum()) / float(valid.sum())
    assert 0.02 < share < 0.98, share


# ---- drop-in --------------------------------------------------------------------------------------------------------------------------
def test_generate_is_the_reference_drop_in(gpu_device):
    depth, valid = _tile(40, 56, 12)
    gen = SyntheticNoiseGenerator(seed=8)
    lab = gen.generate(depth, valid, intensity=1.2)
    assert isinstance(lab, NoiseLabel) and lab.clean_depth is depth
    for a, dt in ((lab.noisy_depth, np.float32), (lab.noise_mask, np.bool_), (lab.noise_magnitude, np.float32), (lab.classification, np.int64)):
        assert isinstance(a, np.ndarray) and a.dtype == dt and a.shape == depth.shape
    assert np.array_equal(lab.classification, np.where(lab.noise_mask, 2, 0)) and lab.noise_mask.any() and not lab.noise_mask[~valid].any()
    again = SyntheticNoiseGenerator(seed=8).generate(depth, valid, intensity=1.2)
    assert np.array_equal(again.noisy_depth.view(np.uint32), lab.noisy_depth.view(np.uint32))
    nan = np.where(valid, depth, np.float32(np.nan))
    lab2 = SyntheticNoiseGenerator(seed=8).generate(nan)                    # valid_mask=None: isfinite
    assert np.array_equal(lab2.noise_mask, lab2.noise_mask & valid) and np.isnan(lab2.noisy_depth[~valid]).all()
    lab3 = NoiseAugmentor(SyntheticNoiseGenerator(seed=8), seed=1)(depth, valid)
    assert isinstance(lab3, NoiseLabel) and lab3.noisy_depth.shape == depth.shape
    with pytest.raises(ValueError):
        gen.generate(depth[0])


def test_unsupported_and_invalid_arguments(gpu_device):
    depth, valid = _tile(16, 16, 1)
    hw, depth_t, mask_t = _upload([(depth, valid)], gpu_device)
    gen = SyntheticNoiseGenerator(seed=1)
    with pytest.raises(ValueError):
        gen.generate_batch(hw, depth_t, mask_t, draws=[{"artifact": "spiral"}])
    with pytest.raises(ValueError):
        gen.generate_batch(hw, depth_t[:-1], mask_t)
    with pytest.raises(ValueError):
        gen.generate_batch(hw, depth_t, mask_t, draws=[{"gaussian": np.zeros((4, 4))}])
    with pytest.raises(ValueError):
        gen.generate_batch(hw, depth_t, mask_t, draws=[{"blobs": [(1, 1, -3, 1.0)]}])
    # the C entry point itself: an artifact code the library does not know is BGNN_ERR_UNSUPPORTED with a message
    import ctypes as C
    from bathymetric_gnn_amd import runtime as rt
    ctx = rt.get_context(gpu_device)
    hw_p = hw.ctypes.data_as(C.c_void_p)
    plans = (rt.NoisePlan * 1)()
    plans[0].intensity, plans[0].artifact = 1.0, 9
    params = gen._params()
    nbytes = ctx.lib.bgnn_noise_workspace_bytes(1, hw_p, 0)
    assert nbytes > 0
    ws = torch.empty(nbytes, dtype=torch.uint8, device=gpu_device)
    outs = [torch.zeros(256, dtype=dt, device=gpu_device) for dt in (torch.float32, torch.uint8, torch.float32, torch.int64)]
    args = [ctx.handle, 1, hw_p, rt.ptr(depth_t), rt.ptr(mask_t), C.byref(params), plans, None, 0, None, rt.ptr(ws)]
    rc = ctx.lib.bgnn_noise_generate(*args, nbytes, *[rt.ptr(o) for o in outs])
    assert rc == rt.ERR_UNSUPPORTED and b"artifact" in ctx.lib.bgnn_last_error()
    with pytest.raises(NotImplementedError, match="artifact"):
        rt.check(rc)
    rc = ctx.lib.bgnn_noise_generate(*args, nbytes - 256, *[rt.ptr(o) for o in outs])
    assert rc == rt.ERR_INVALID and b"workspace" in ctx.lib.bgnn_last_error()
    torch.cuda.synchronize()
    assert not any(bool(o.any()) for o in outs)            # a refused call launches nothing


# ---- end to end -----------------------------------------------------------------------------------------------------------------------
def test_end_to_end_targets_and_one_training_step(gpu_device):
    """generate_batch -> build_from_device -> training_targets against the trainer's formula on the host, then one training
    step of a GAT model: cross-entropy on y + Huber on correction_target under noise_mask + the confidence calibration term,
    all in torch; every parameter receives a finite, non-zero gradient."""
    tiles = [_tile(64, 64, 50), _tile(48, 80, 51), _tile(64, 64, 52, "V0")]
    hw, clean_t, mask_t = _upload(tiles, gpu_device)
    gen = SyntheticNoiseGenerator(seed=123)
    b = NoiseAugmentor(gen, seed=5).augment_batch(hw, clean_t, mask_t)
    gb = GraphBuilder()
    res = np.ones((len(tiles), 2), np.float64)
    graph = gb.build_from_device(hw, res, b.noisy_depth, mask_t, None)
    y, target, nmask = training_targets(graph, clean_t, b.noisy_depth, b.classification, b.noise_mask)
    N = graph.num_nodes
    assert N == int(mask_t.sum()) and y.shape == target.shape == nmask.shape == (N,)
    assert y.dtype == torch.int64 and target.dtype == torch.float32 and nmask.dtype == torch.bool and y.is_cuda
    # the trainer's formula on the host, tile by tile
    rows, cols, bat = (t.cpu().numpy() for t in (graph.valid_rows, graph.valid_cols, graph.batch))
    lstd = graph.local_std.cpu()
    outs = _split(b)
    want_y, want_raw, want_m = [], [], []
    for t, (clean, _) in enumerate(tiles):
        sel = bat == t
        r, c = rows[sel], cols[sel]
        want_y.append(outs[t][3][r, c]); want_m.append(outs[t][1][r, c])
        want_raw.append(outs[t][0][r, c] - clean[r, c])
    want_t = torch.clamp(torch.tensor(np.concatenate(want_raw), dtype=torch.float32) / torch.clamp(lstd, min=CORRECTION_NORM_FLOOR),
                         min=-CORRECTION_NORM_CAP, max=CORRECTION_NORM_CAP)
    assert np.array_equal(y.cpu().numpy(), np.concatenate(want_y)) and np.array_equal(nmask.cpu().numpy(), np.concatenate(want_m))
    assert torch.equal(target.cpu(), want_t)
    assert float(target.abs().max()) <= CORRECTION_NORM_CAP and bool(nmask.any()) and set(torch.unique(y).tolist()) == {0, 2}
    # one training step on that batch
    torch.manual_seed(0)
    m = BathymetricGNN(in_channels=7, num_gnn_layers=3, edge_dim=3).to(gpu_device)
    m.train()
    m.zero_grad(set_to_none=True)
    out = m(graph)
    loss = torch.nn.functional.cross_entropy(out["class_logits"], y)
    loss = loss + torch.nn.functional.huber_loss(out["correction"].reshape(-1)[nmask], target[nmask])
    # the confidence head is reached by neither term: the reference's training loss adds its calibration term (BCE of the
    # confidence against "the predicted class is right"), and so does this step -- otherwise four parameters have no gradient
    correct = (out["class_logits"].detach().argmax(-1) == y).float()
    loss = loss + 0.2 * torch.nn.functional.binary_cross_entropy(out["confidence"].reshape(-1), correct)
    loss.backward()
    assert math.isfinite(float(loss))
    for name, p in m.named_parameters():
        assert p.grad is not None and bool(torch.isfinite(p.grad).all()) and int(torch.count_nonzero(p.grad)) > 0, name
