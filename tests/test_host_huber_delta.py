"""The adaptive Huber delta without a GPU (training/huber_delta.py): the policy ``AdaptiveHuberDelta`` against a hand replay in both
modes, its state through ``torch.save`` / ``torch.load(weights_only=True)``, its refusals, and the host half of the percentile:
``percentile_from_ranks`` from the two order statistics the device selects equals ``np.percentile`` of the float64-cast values
bit for bit."""
import math

import numpy as np
import pytest
import torch

from bathymetric_gnn_amd.training import AdaptiveHuberDelta, percentile_from_ranks
from bathymetric_gnn_amd.training.huber_delta import _check_percentiles

QS = [3.0, 0.25, None, 0.1, 0.1, 0.2, 7.5, None, 12.0, 1.75]


def _replay(mode, initial, ceiling, momentum, min_delta, qs):
    running, out = initial, []
    ceiling = initial if ceiling is None else ceiling
    for q in qs:
        if q is not None:
            running = momentum * running + (1 - momentum) * q
        out.append(max(min_delta, min(running, ceiling)) if mode == "hybrid" else max(min_delta, running))
    return out


@pytest.mark.parametrize("mode", ["hybrid", "error"])
@pytest.mark.parametrize("ceiling", [None, 2.0])
def test_policy_equals_a_hand_replay(mode, ceiling):
    policy = AdaptiveHuberDelta(ceiling=ceiling, momentum=0.6, min_delta=1.0, mode=mode)
    assert policy.start(2.5) == policy.delta == (2.5 if mode == "error" or ceiling is None else 2.0)
    want = _replay(mode, 2.5, ceiling, 0.6, 1.0, QS)
    got = []
    for q in QS:
        before = policy.delta
        got.append(policy.update(q))
        assert got[-1] == policy.delta
        if q is None:
            assert got[-1] == before                           # an epoch without a percentile changes nothing
    assert got == want
    top = 2.5 if ceiling is None else ceiling
    if mode == "hybrid":
        assert all(1.0 <= d <= top for d in got)
        assert min(got) == 1.0                                  # the floor was reached (running fell below it) ...
        assert max(got) == top                                  # ... and so was the ceiling
    else:
        assert all(d >= 1.0 for d in got) and max(got) > 2.5    # Option 2 may pass the initial delta


def test_defaults_are_the_reference_option_3():
    policy = AdaptiveHuberDelta()
    assert (policy.mode, policy.percentile, policy.momentum, policy.min_delta, policy.ceiling) == ("hybrid", 95.0, 0.9, 1.0, None)
    with pytest.raises(RuntimeError):
        policy.delta
    with pytest.raises(RuntimeError):
        policy.update(1.0)
    policy.start(4.0)
    assert policy.ceiling == 4.0 and policy.running == 4.0 and policy.delta == 4.0
    assert policy.update(2.0) == 0.9 * 4.0 + (1 - 0.9) * 2.0
    assert policy.update(100.0) == 4.0                          # capped by the data-derived delta


def test_state_dict_round_trip_mid_sequence(tmp_path):
    a = AdaptiveHuberDelta(momentum=0.7, mode="error", percentile=90.0, min_delta=0.5)
    a.start(3.25)
    for q in QS[:4]:
        a.update(q)
    state = a.state_dict()
    assert all(type(v) in (float, int, str) for v in state.values())
    torch.save({"adaptive_delta": state}, tmp_path / "p.pt")
    loaded = torch.load(tmp_path / "p.pt", weights_only=True)["adaptive_delta"]
    assert loaded == state
    b = AdaptiveHuberDelta()
    b.load_state_dict(loaded)
    assert b.state_dict() == state and b.delta == a.delta
    for q in QS[4:]:
        assert a.update(q) == b.update(q)
    assert a.state_dict() == b.state_dict() and a.updates == sum(q is not None for q in QS)


@pytest.mark.parametrize("kw", [dict(momentum=1.0), dict(momentum=-0.1), dict(momentum=float("nan")), dict(percentile=-1.0),
                                dict(percentile=100.5), dict(percentile=float("nan")), dict(min_delta=0.0), dict(min_delta=-1.0),
                                dict(min_delta=float("nan")), dict(mode="median"), dict(mode=""), dict(ceiling=0.5),
                                dict(ceiling=1.0, min_delta=2.0), dict(ceiling=float("nan"))])
def test_policy_refusals(kw):
    with pytest.raises(ValueError):
        AdaptiveHuberDelta(**kw)


def test_policy_accepts_the_edges():
    for kw in (dict(momentum=0.0), dict(percentile=0.0), dict(percentile=100.0), dict(ceiling=1.0), dict(min_delta=1e-9, ceiling=1e-9)):
        AdaptiveHuberDelta(**kw).start(2.0)
    p = AdaptiveHuberDelta(momentum=0.0)
    p.start(5.0)
    assert p.update(2.0) == 2.0                                 # no memory: the epoch's value itself
    with pytest.raises(ValueError):
        p.update(float("nan"))
    with pytest.raises(ValueError):
        p.load_state_dict({**p.state_dict(), "mode": "other"})


def test_percentile_lists():
    assert _check_percentiles(95) == [95.0] and _check_percentiles([0, 50.0, 100]) == [0.0, 50.0, 100.0]
    for bad in ([], [1, 2, 3, 4], [-0.5], [100.1], [float("nan")]):
        with pytest.raises(ValueError):
            _check_percentiles(bad)


def _ranks(m, p):
    vi = (m - 1) * (p / 100)
    lo = int(math.floor(vi))
    return lo, min(lo + 1, m - 1)


def test_host_interpolation_equals_numpy_on_float64():
    rng = np.random.default_rng(20261021)
    fixed = [0.0, 50.0, 95.0, 99.0, 100.0]
    checked = 0
    for case in range(3000):
        n = int(rng.integers(1, 301))
        scale = float(10.0 ** rng.uniform(-3, math.log10(50.0)))
        x = (rng.standard_normal(n) * scale).astype(np.float32)
        kind = case % 4
        if kind == 1:                                           # ties: a handful of distinct values
            x = rng.choice(x[:max(1, n // 8)], size=n)
        elif kind == 2:                                         # magnitudes, as the tracker files them
            x = np.abs(x)
        elif kind == 3 and n > 2:                               # neighbours that differ in the last bits
            x = np.nextafter(np.float32(scale), np.float32(np.inf), dtype=np.float32) + np.zeros(n, np.float32)
            x[::2] = np.float32(scale)
        s = np.sort(x)
        for p in fixed + [float(rng.uniform(0, 100))]:
            lo, hi = _ranks(n, p)
            got = percentile_from_ranks(n, p, lo, hi, s[lo], s[hi])
            want = float(np.percentile(x.astype(np.float64), p))
            assert got == want, (n, p, got, want)
            checked += 1
    assert checked == 18000


def test_host_interpolation_edges():
    assert percentile_from_ranks(0, 50.0, -1, -1, float("nan"), float("nan")) is None
    assert percentile_from_ranks(1, 73.0, 0, 0, np.float32(2.5), np.float32(2.5)) == 2.5
    with pytest.raises(ValueError):
        percentile_from_ranks(10, 50.0, 3, 4, 1.0, 2.0)          # (the ranks of p = 50 over 10 values are 4 and 5)
    x = np.array([1.0, 1.5], np.float32)
    assert percentile_from_ranks(2, 99.9, 0, 1, x[0], x[1]) == float(np.percentile(x.astype(np.float64), 99.9))
