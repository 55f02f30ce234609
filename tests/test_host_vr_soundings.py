"""The restatement of the variable-resolution sounding gridders (tests/_vr_soundings_cpu.py) held against the contract of
include/bgnn_soundings_vr.h without a GPU: every accepted sounding's record lies in its base cell's range, the address is monotone
in x within a row of records, ``floor(fu * d) < d`` for the largest ``fu`` and every dimension, a uniform layout equals the
uniform restatement after flipud and regrouping, the planner's thresholds -- and the address header itself
(csrc/sounding_vr_cell.h), compiled alone into a program of its own with the address and undefined-behaviour sanitizers and
compared with the restatement on the border clouds."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import _soundings_cpu as sc
import _vr_soundings_cpu as vc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("B", [8.0, 6.3])
def test_records_lie_in_their_base_cell(B):
    lay = vc.mixed_layout(B)
    x, y, z = vc.mixed_cloud(B)
    kind, record = vc.classify(x, y, z, lay)
    c = vc.counters_of(kind)
    assert sum(c.values()) == z.size and all(v > 0 for v in c.values()), c
    acc = kind == vc.ACCEPTED
    b, _, _, _, on = vc.base_cell(x, y, lay["origin"], lay["B"], lay["base_shape"])
    first = lay["index"].reshape(-1)[b[acc]]
    cells = (lay["dx"] * lay["dy"]).reshape(-1)[b[acc]]
    assert np.all(cells > 0) and np.all(record[acc] >= first) and np.all(record[acc] < first + cells)
    assert record[acc].max() < lay["total"] and np.all(record[~acc] == -1)
    assert np.unique(record[acc]).size > 0.5 * lay["total"]              # the cloud reaches most records


@pytest.mark.parametrize("B", [0.7, 1.1, 6.3, 8.0, 64.0])
def test_address_is_monotone_in_x(B):
    """Along one row of records (y fixed inside refinement row 1 of base row 0) the record never decreases with x, through every
    base cell of a row whose dimensions differ from cell to cell."""
    dims = [1, 2, 3, 5, 7, 8, 12, 64, 255]
    lay = vc.make_layout((1, len(dims)), (5.0e5 + 0.3, 4.1e6), B, [dims], [[2] * len(dims)])
    rng = np.random.default_rng(3)
    x = np.sort(lay["origin"][0] + rng.uniform(0, len(dims) * B, 200000))
    on = np.concatenate([lay["origin"][0] + (b + np.arange(d) / d) * B for b, d in enumerate(dims)])
    x = np.sort(np.concatenate([x, on, np.nextafter(on, -np.inf), np.nextafter(on, np.inf)]))
    y = np.full(x.size, lay["origin"][1] + 0.75 * B)
    kind, record = vc.classify(x, y, np.zeros(x.size, np.float32), lay)
    r = record[kind == vc.ACCEPTED]
    # row 1 of a grid of dx columns: records index + dx .. index + 2 dx - 1, and index grows from base cell to base cell
    assert r.size > 200000 and np.all(np.diff(r) >= 0)
    assert set(np.unique(r)) == {int(i) + d + s for i, d in zip(lay["index"].reshape(-1), dims) for s in range(d)}


def test_no_clamp_is_needed():
    """``fl(fu * d) < d`` for the largest ``fu`` there is, ``nextafter(1, 0)``, and every dimension 1 .. 32768."""
    fu = np.nextafter(np.float64(1.0), np.float64(0.0))
    d = np.arange(1, vc.MAX_DIM + 1, dtype=np.float64)
    assert fu == 1.0 - 2.0 ** -53
    assert np.all(np.floor(fu * d) < d) and np.all(np.floor(fu * d) == d - 1)


@pytest.mark.parametrize("d", [1, 4])
def test_uniform_layout_is_the_uniform_grid(d):
    """Every base cell ``d x d``: the records are the cells of the north-up uniform grid at ``B / d`` after flipud and regrouping, on
    a cloud whose points keep 0.1 cell away from every border (there the two arithmetics may differ, and that is documented)."""
    (BH, BW), B, (x0, y0) = (5, 6), 8.0, (5.0e5, 4.1e6)
    lay = vc.make_layout((BH, BW), (x0, y0), B, np.full((BH, BW), d), np.full((BH, BW), d))
    res, H, W = B / d, BH * d, BW * d
    rng = np.random.default_rng(9)
    n = 30000
    x = x0 + (rng.integers(0, W, n) + rng.uniform(0.1, 0.9, n)) * res
    y = y0 + (rng.integers(0, H, n) + rng.uniform(0.1, 0.9, n)) * res
    z = (-30.0 + rng.standard_normal(n)).astype(np.float32)
    got = vc.grid(x, y, z, lay, min_count=2)
    want = sc.grid(x, y, z, (H, W), (x0, y0 + BH * B), res, min_count=2)
    assert got["counters"]["accepted"] == n == want["counters"]["accepted"]
    for name in ("count", "mean", "std", "min", "max", "valid"):
        w = vc.uniform_to_records(want[name], (BH, BW), d)
        assert got[name].dtype == w.dtype and np.array_equal(got[name].view(np.uint8), np.ascontiguousarray(w).view(np.uint8)), name


def test_planner_thresholds():
    """A rung is reached at exactly ``target * d * d`` soundings, for every rung; below ``min_base_count`` there is no grid."""
    for target in (1, 3, 10):
        for i, d in enumerate(vc.DEFAULT_LADDER):
            t = target * d * d
            below = vc.DEFAULT_LADDER[i - 1] if i else 0
            assert vc.plan_dim(t - 1, target) == below and vc.plan_dim(t, target) == d and vc.plan_dim(t + 1, target) == d
    assert vc.plan_dim(10 ** 9, 1) == 64 and vc.plan_dim(0, 1) == 0
    assert vc.plan_dim(49, 1, min_base_count=50) == 0 and vc.plan_dim(50, 1, min_base_count=50) == 4
    assert vc.plan_dim(2 ** 32 - 1, 2 ** 31 - 1, ladder=(1, 32768)) == 1            # (the comparison needs 64 bits: 2^31 * 2^30)
    assert vc.plan_dim(17, 2, ladder=(3, 5)) == 0 and vc.plan_dim(18, 2, ladder=(3, 5)) == 3
    index, dd, total = vc.plan(np.array([[4, 0, 16], [3, 64, 1]]), 1, (1, 2, 4))
    assert dd.tolist() == [[2, 0, 4], [1, 4, 1]] and index.tolist() == [[0, 4, 4], [20, 21, 37]] and total == 38


def _cxx():
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    for c in (shutil.which("g++"), os.path.join(rocm, "lib", "llvm", "bin", "clang++"), shutil.which("amdclang++"), shutil.which("clang++")):
        if c and os.path.exists(c):
            return c
    pytest.fail("no C++ compiler: neither g++ nor ROCm's clang++")


def test_address_header_on_the_host(tmp_path):
    """csrc/sounding_vr_cell.h alone, by a host compiler, in a program of its own built with -fsanitize=address,undefined: the
    border clouds of the device test along x and along y, the outer borders of the mixed layout and one float64 step on either
    side, NaN and +-inf, coordinates too large for any integer, a record above 2^31 -- all equal to the restatement."""
    exe = tmp_path / "vr_cell_host_check"
    subprocess.run([_cxx(), "-std=c++17", "-O1", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    os.path.join(ROOT, "tests", "vr_cell_host_check.cpp"), "-o", str(exe)], check=True)
    clouds = []                                                   # (layout, x, y)
    for B in (0.7, 1.1):
        for d in (3, 5, 7, 64):
            t, _ = vc.border_cloud(B, d)
            t = t[::5] if d == 64 else t
            mid = np.full(t.size, vc.BORDER_X0 + 0.5 * B)
            clouds.append((vc.border_layout(B, d, True), t, mid))
            clouds.append((vc.border_layout(B, d, False), mid, t))
    lay = vc.mixed_layout(6.3)
    (BH, BW), (x0, y0), B = lay["base_shape"], lay["origin"], lay["B"]
    xs, ys = [], []
    for bx in (x0, x0 + BW * B):
        for by in (y0, y0 + BH * B):
            for sx in (-np.inf, None, np.inf):
                for sy in (-np.inf, None, np.inf):
                    xs.append(bx if sx is None else float(np.nextafter(bx, sx)))
                    ys.append(by if sy is None else float(np.nextafter(by, sy)))
    for bad in (np.nan, np.inf, -np.inf, 1e300, -1e300):
        xs += [bad, x0 + 1.0]
        ys += [y0 + 1.0, bad]
    x, y, _ = vc.mixed_cloud(6.3)
    clouds.append((lay, np.concatenate([xs, x[:3000]]), np.concatenate([ys, y[:3000]])))
    big = vc.make_layout((2, 2), (0.0, 0.0), 64.0, [[0, 0], [0, 32768]], [[0, 0], [0, 32768]], index=[[0, 0], [0, 2 ** 31 - 2 ** 30 - 1]])
    clouds.append((big, np.array([127.999, 64.0, 100.0]), np.array([127.999, 64.0, 64.0])))
    fmt = lambda v: float(v).hex() if np.isfinite(v) else repr(float(v))
    lines, want = [], []
    for lay, x, y in clouds:
        (BH, BW), (x0, y0), B = lay["base_shape"], lay["origin"], lay["B"]
        kind, record = vc.classify(x, y, np.zeros(len(x), np.float32), lay)
        b = vc.base_cell(x, y, lay["origin"], B, lay["base_shape"])[0]
        e = np.maximum(b, 0)
        for i in range(len(x)):
            lines.append(" ".join([fmt(x[i]), fmt(y[i]), fmt(x0), fmt(y0), fmt(B), str(BH), str(BW)] +
                                  [str(int(lay[k].reshape(-1)[e[i]])) for k in ("index", "dx", "dy")] + [str(lay["total"])]))
            want.append((int(b[i]), int(kind[i] == vc.ACCEPTED), int(record[i])))
    path = tmp_path / "cases.txt"
    path.write_text("\n".join(lines) + "\n")
    r = subprocess.run([str(exe), str(path)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    got = [tuple(int(v) for v in line.split()) for line in r.stdout.splitlines()]
    assert len(got) == len(want) > 5000
    assert got == want
    assert got[-3] == (3, 1, 2 ** 31 - 2) and got[-2] == (3, 1, 2 ** 31 - 2 ** 30 - 1)          # the last record there can be
    # the border clouds decide the arithmetic: many soundings "on" s / d fall into the record before
    t, _ = vc.border_cloud(0.7, 7)
    lay = vc.border_layout(0.7, 7, True)
    _, rec = vc.classify(t, np.full(t.size, vc.BORDER_X0 + 0.007), np.zeros(t.size, np.float32), lay)
    n_on = t.size // 3
    nominal = np.arange(n_on)                                    # base cell b, column s: record 49 b + s in row 0
    nominal = (nominal // 7) * 49 + nominal % 7
    assert 5 < np.count_nonzero(rec[:n_on] != nominal) < n_on
