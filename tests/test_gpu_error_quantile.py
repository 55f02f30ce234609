"""Error percentiles on the GPU (include/bgnn_quantile.h, csrc/error_quantile.hip, training/huber_delta.py) against numpy, exactly:
the multiset of staged keys, every counter, the top-digit histogram, the selected ranks and order statistics, and the percentile
``float(np.percentile(errors.astype(np.float64), p))`` bit for bit -- over partial waves and several workgroups, every kind of mask,
values that keep all ranks in one group to the last level or part them at the first, zeros and denormals, non-finite rows,
uneven calls, overflow of the stage beside a guard region, unaligned planes, and the one-shot forms."""
import numpy as np
import pytest
import torch

from _quantile_cpu import PS, _check, _dev, _errors, _keys, _planes, _ranks, _staged, _tracker, _want

pytestmark = pytest.mark.gpu
SIZES = [1, 63, 64, 65, 1000, 1025, 70001]


@pytest.fixture(scope="module")
def big(gpu_device):
    """70001 rows with a 20 % mask, shared by the tests that need the large case; never modified."""
    rng, c, t = _planes(70001, 7)
    mask = (rng.random(70001) < 0.2).astype(np.uint8)
    e, nf = _errors(c, t, mask)
    return c, t, mask, e, nf


@pytest.mark.parametrize("mask_kind", ["ones", "zeros", "fifth", "null"])
@pytest.mark.parametrize("n", SIZES)
def test_sizes_and_masks(n, mask_kind, gpu_device):
    rng, c, t = _planes(n, 100 + n)
    mask = {"ones": np.ones(n, np.uint8), "zeros": np.zeros(n, np.uint8), "fifth": (rng.random(n) < 0.2).astype(np.uint8), "null": None}[mask_kind]
    if mask_kind == "fifth":
        mask[mask != 0] = rng.integers(1, 256, int((mask != 0).sum()))      # any non-zero byte selects the row
    e, nf = _errors(c, t, mask)
    tr = _tracker(n, gpu_device)
    dm = _dev(mask, gpu_device)
    if mask_kind == "ones":
        dm = dm.bool()                                                     # a bool mask is taken as it is
    tr.add(_dev(c, gpu_device), _dev(t, gpu_device), dm)
    _check(tr, e, nf)


@pytest.mark.parametrize("offset", [1, 3])
def test_unaligned_planes(offset, gpu_device):
    """Planes that start 4 / 12 bytes (the mask 1 / 3 bytes) into their allocations take the scalar loads."""
    n = 5000
    rng, c, t = _planes(n, 31)
    mask = (rng.random(n) < 0.5).astype(np.uint8)
    e, nf = _errors(c, t, mask)
    tr = _tracker(n, gpu_device)
    dc, dt, dm = _dev(c, gpu_device, offset), _dev(t, gpu_device, offset), _dev(mask, gpu_device, offset)
    assert dc.data_ptr() % 16 != 0 and dm.data_ptr() % 4 != 0
    tr.add(dc, dt, dm)
    _check(tr, e, nf)


def test_all_errors_equal(gpu_device):
    """Every rank stays in one group through every level; the worst contention on one histogram bin."""
    n = 3001
    c = np.full(n, 2.75, np.float32)
    t = np.full(n, 1.5, np.float32)
    tr = _tracker(n, gpu_device)
    tr.add(_dev(c, gpu_device), _dev(t, gpu_device), None)
    got = _check(tr, *_errors(c, t, None), ps=[0.0, 50.0, 100.0])
    assert got["values"] == [1.25, 1.25, 1.25]


def test_errors_that_differ_in_the_last_mantissa_bits(gpu_device):
    """All keys share the first two digits (22 bits): the ranks part only at the last level."""
    n = 4099
    rng = np.random.default_rng(5)
    base = np.float32(1.5).view(np.uint32)
    e = (base + rng.integers(0, 1024, n).astype(np.uint32)).view(np.float32)
    c, t = e.copy(), np.zeros(n, np.float32)
    assert len(np.unique(_keys(e) >> 10)) == 1
    tr = _tracker(n, gpu_device)
    tr.add(_dev(c, gpu_device), _dev(t, gpu_device), None)
    _check(tr, *_errors(c, t, None), ps=[50.0, 95.0, 99.9])


def test_bimodal_groups_part_at_the_top_digit(gpu_device):
    n = 6000
    rng = np.random.default_rng(6)
    c = np.where(rng.random(n) < 0.6, rng.uniform(1e-3, 2e-3, n), rng.uniform(40.0, 50.0, n)).astype(np.float32)
    t = np.zeros(n, np.float32)
    e, nf = _errors(c, t, None)
    s = np.sort(_keys(e))
    lo50, lo999 = _ranks(n, 50.0)[0], _ranks(n, 99.9)[0]
    assert s[lo50] >> 21 != s[lo999] >> 21
    tr = _tracker(n, gpu_device)
    tr.add(_dev(c, gpu_device), _dev(t, gpu_device), None)
    _check(tr, e, nf, ps=[50.0, 99.9])


def test_zeros_negative_zero_and_denormals(gpu_device):
    tiny = np.float32(1e-45)
    c = np.array([0.0, -0.0, 0.0, tiny, -tiny, 3 * tiny, 1e-39, -1e-39, 1.17549435e-38, 0.0, 5.0, -0.0], np.float32)
    t = np.array([0.0, 0.0, -0.0, 0.0, 0.0, tiny, 0.0, 1e-39, 0.0, 1e-40, 5.0, -0.0], np.float32)
    c, t = np.tile(c, 11), np.tile(t, 11)
    e, nf = _errors(c, t, None)
    assert nf == 0 and not np.signbit(e).any() and (e == 0).sum() >= 33 and ((e > 0) & (e < 1.2e-38)).sum() >= 44
    tr = _tracker(c.size, gpu_device)
    tr.add(_dev(c, gpu_device), _dev(t, gpu_device), None)
    _check(tr, e, nf, ps=[0.0, 40.0, 75.0])


def test_nonfinite_rows_are_counted_not_filed(gpu_device):
    n = 777
    rng, c, t = _planes(n, 8)
    mask = (rng.random(n) < 0.7).astype(np.uint8)
    bad = [np.nan, np.inf, -np.inf]
    for k, i in enumerate(rng.choice(n, 60, replace=False)):
        (c if k % 2 else t)[i] = bad[k % 3]
    c[5], t[5] = np.inf, np.inf                                   # inf - inf = NaN
    c[6], t[6] = 3.0e38, -3.0e38                                  # the difference overflows to inf
    mask[5] = mask[6] = 1
    e, nf = _errors(c, t, mask)
    assert nf >= 20
    tr = _tracker(n, gpu_device)
    tr.add(_dev(c, gpu_device), _dev(t, gpu_device), _dev(mask, gpu_device))
    _check(tr, e, nf)


def test_one_add_equals_seven_uneven_adds(big, gpu_device):
    c, t, mask, e, nf = big
    dc, dt, dm = _dev(c, gpu_device), _dev(t, gpu_device), _dev(mask, gpu_device)
    one = _tracker(c.size, gpu_device)
    one.add(dc, dt, dm)
    first = _check(one, e, nf)
    parts = _tracker(c.size, gpu_device)
    cuts = [0, 1, 64, 4097, 4100, 30011, 61000, 70001]
    for a, b in zip(cuts[:-1], cuts[1:]):
        parts.add(dc[a:b], dt[a:b], dm[a:b])
    second = _check(parts, e, nf)
    assert first == second
    assert np.array_equal(_staged(one, e.size), _staged(parts, e.size))
    sa, sb = one.state(), parts.state()
    assert sa.tobytes() == sb.tobytes()


def test_two_runs_give_equal_bits(big, gpu_device):
    c, t, mask, e, nf = big
    blocks = []
    for _ in range(2):
        tr = _tracker(c.size, gpu_device)
        tr.add(_dev(c, gpu_device), _dev(t, gpu_device), _dev(mask, gpu_device))
        blocks.append((tr.select(PS).tobytes(), tr.state().tobytes()))
    assert blocks[0] == blocks[1]


def test_three_percentiles_in_one_call_equal_three_calls(big, gpu_device):
    c, t, mask, e, nf = big
    tr = _tracker(c.size, gpu_device)
    tr.add(_dev(c, gpu_device), _dev(t, gpu_device), _dev(mask, gpu_device))
    ps = [12.5, 95.0, 100.0]
    together = tr.percentiles(ps)
    singles = [tr.percentiles([p]) for p in ps]
    assert together["values"] == [s["values"][0] for s in singles] == [_want(e, p) for p in ps]
    assert all(s["count"] == together["count"] == e.size for s in singles)
    tb = tr.select(ps)
    for k, p in enumerate(ps):
        assert tr.select([p])["ranks"][0].tobytes() == tb["ranks"][k].tobytes()
    with pytest.raises(ValueError):
        tr.percentiles([1.0, 2.0, 3.0, 4.0])
    with pytest.raises(ValueError):
        tr.percentiles([101.0])


def test_overflow_is_counted_and_nothing_passes_the_stage(gpu_device):
    from bathymetric_gnn_amd.training import CorrectionErrorTracker
    capacity, guard, front = 100, 64, 32
    n = 400
    rng, c, t = _planes(n, 9)
    mask = np.zeros(n, np.uint8)
    mask[rng.choice(n, 260, replace=False)] = 1
    hit = np.flatnonzero(mask)
    c[hit[:3]] = np.nan                                           # 257 finite masked rows, 3 that are not
    e, nf = _errors(c, t, mask)
    assert (e.size, nf) == (257, 3)
    pattern = np.arange(front + capacity + guard, dtype=np.int32) * 7 - 1000003
    buffer = torch.from_numpy(pattern.copy()).to(gpu_device)
    tr = CorrectionErrorTracker(capacity, device=gpu_device, stage=buffer[front:front + capacity])
    tr.reset()
    dc, dt, dm = _dev(c, gpu_device), _dev(t, gpu_device), _dev(mask, gpu_device)
    tr.add(dc[:150], dt[:150], dm[:150])
    tr.add(dc[150:], dt[150:], dm[150:])
    got = tr.percentiles([95.0])
    assert got == {"count": 100, "nonfinite": 3, "dropped": 157, "values": [None]}
    st = tr.state()
    assert int(st["filed"]) + int(st["dropped"]) == 257 == int(st["cursor"]) and int(st["rows"]) == 260
    assert int(st["hist"].sum()) == 100
    after = buffer.cpu().numpy()
    assert np.array_equal(after[:front], pattern[:front])
    assert np.array_equal(after[front + capacity:], pattern[front + capacity:])          # the 64-word guard region
    staged = after[front:front + capacity].view(np.uint32)
    all_keys = _keys(e)
    assert np.isin(staged, all_keys).all()                       # whichever rows arrived first, they are rows of the input
    assert np.array_equal(np.bincount(staged >> 21, minlength=2048), st["hist"])


def test_device_percentile_and_correction_delta(gpu_device):
    from bathymetric_gnn_amd.training import compute_correction_delta, device_percentile
    rng = np.random.default_rng(12)
    x = (rng.standard_normal((37, 53)) * 4.0).astype(np.float32)
    x[3, 4], x[5, 6], x[7, 8] = np.nan, np.inf, -np.inf
    dx = torch.from_numpy(x).to(gpu_device)
    fin = x[np.isfinite(x)]
    signed = device_percentile(dx, [5.0, 50.0, 95.0])
    assert (signed["count"], signed["nonfinite"], signed["dropped"]) == (fin.size, 3, 0)
    assert signed["values"] == [_want(fin, p) for p in (5.0, 50.0, 95.0)] and signed["values"][0] < 0 < signed["values"][2]
    magnitude = device_percentile(dx, 95.0, absolute=True)
    assert magnitude["values"] == [_want(np.abs(fin), 95.0)] and magnitude["nonfinite"] == 3
    assert device_percentile(dx[:0], 50.0) == {"count": 0, "nonfinite": 0, "dropped": 0, "values": [None]}
    with pytest.raises(TypeError):
        device_percentile(dx.double(), 50.0)
    capped = np.clip(fin, -50.0, 50.0)
    d_capped = torch.from_numpy(capped).to(gpu_device)
    for p, floor in ((95.0, 1.0), (50.0, 1.0), (95.0, 100.0)):
        want = max(float(np.percentile(np.abs(capped).astype(np.float64), p)), floor)
        assert compute_correction_delta(d_capped, percentile=p, min_delta=floor) == want
    assert compute_correction_delta(d_capped[:0]) == 1.0
    # a host array stays exactly what it was: numpy's float32 percentile
    assert compute_correction_delta(capped, 95.0, 1.0) == max(float(np.percentile(np.abs(capped), 95.0)), 1.0)
