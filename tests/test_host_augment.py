"""The host side of the geometric augmentation (training.dihedral_ops, training.transformed_tile_table, Trainer.augment_plan) against
numpy: the op numbering ``op = k + 4 * f`` of include/bgnn_augment.h, the draw rules of the four flag combinations, the inverse
table the header states, and the plan of an epoch as a pure function of (seed, epoch).  No GPU."""
import os
import re
from types import SimpleNamespace

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
A = np.arange(15, dtype=np.int32).reshape(3, 5) * 7 + 1          # asymmetric: no symmetry of the rectangle maps it to itself
INVERSE = [0, 3, 2, 1, 4, 5, 6, 7]                               # rotations: (4 - k) % 4; every op with f = 1: itself


def apply_op(t, op):
    """The transform as the header defines it."""
    k, f = op & 3, op >> 2
    return np.rot90(np.fliplr(t) if f else t, k)


def test_the_eight_ops_are_the_dihedral_group():
    images = [apply_op(A, op) for op in range(8)]
    assert np.array_equal(images[0], A)
    assert all(im.shape == ((5, 3) if op & 1 else (3, 5)) for op, im in enumerate(images))
    assert len({(im.shape, im.tobytes()) for im in images}) == 8
    sq = np.arange(16).reshape(4, 4)                             # closed under composition (on a square, where shapes agree)
    group = {apply_op(sq, op).tobytes() for op in range(8)}
    assert len(group) == 8
    assert all(apply_op(apply_op(sq, a), b).tobytes() in group for a in range(8) for b in range(8))


def test_the_headers_cell_table_is_numpy():
    """op by op, out[i][j] as include/bgnn_augment.h lists it."""
    h, w = A.shape
    cell = {0: lambda i, j: (i, j), 1: lambda i, j: (j, w - 1 - i), 2: lambda i, j: (h - 1 - i, w - 1 - j), 3: lambda i, j: (h - 1 - j, i),
            4: lambda i, j: (i, w - 1 - j), 5: lambda i, j: (j, i), 6: lambda i, j: (h - 1 - i, j), 7: lambda i, j: (h - 1 - j, w - 1 - i)}
    for op in range(8):
        out = apply_op(A, op)
        want = np.array([[A[cell[op](i, j)] for j in range(out.shape[1])] for i in range(out.shape[0])])
        assert np.array_equal(out, want), op
    assert np.array_equal(apply_op(A, 5), A.T)


def test_inverse_table():
    for op in range(8):
        k, f = op & 3, op >> 2
        assert INVERSE[op] == (op if f else (4 - k) % 4)
        assert np.array_equal(apply_op(apply_op(A, op), INVERSE[op]), A), op
    assert INVERSE[0] == 0 and all(INVERSE[INVERSE[op]] == op for op in range(8))
    text = open(os.path.join(ROOT, "include", "bgnn_augment.h")).read()
    assert "(4 - k) % 4" in text and re.search(r"f = 1 .{0,20}is its own inverse", text)


def test_dihedral_ops_both_flags():
    from bathymetric_gnn_amd.training import dihedral_ops
    ops = dihedral_ops(4000, True, True, np.random.default_rng(5))
    assert ops.dtype == np.int8 and ops.shape == (4000,)
    rng = np.random.default_rng(5)
    k = rng.integers(0, 4, 4000)
    f = rng.integers(0, 2, 4000)
    assert np.array_equal(ops, k + 4 * f)
    counts = np.bincount(ops, minlength=8)
    assert len(counts) == 8 and counts.min() > 400 and counts.max() < 600          # 500 expected, sd 21
    assert np.array_equal(ops, dihedral_ops(4000, True, True, np.random.default_rng(5)))


def test_dihedral_ops_rotations_only():
    from bathymetric_gnn_amd.training import dihedral_ops
    ops = dihedral_ops(500, True, False, np.random.default_rng(6))
    assert ops.dtype == np.int8 and set(ops.tolist()) == {0, 1, 2, 3}
    assert np.array_equal(ops, np.random.default_rng(6).integers(0, 4, 500))


def test_dihedral_ops_flips_only():
    from bathymetric_gnn_amd.training import dihedral_ops
    ops = dihedral_ops(500, False, True, np.random.default_rng(7))
    assert ops.dtype == np.int8 and set(ops.tolist()) == {0, 2, 4, 6}
    rng = np.random.default_rng(7)
    fh = rng.integers(0, 2, 500)
    fv = rng.integers(0, 2, 500)
    seen = set()
    for op, h, v in zip(ops.tolist(), fh.tolist(), fv.tolist()):
        if (h, v) in seen:
            continue
        seen.add((h, v))
        want = A
        if h:
            want = np.fliplr(want)
        if v:
            want = np.flipud(want)
        assert np.array_equal(apply_op(A, op), want), (h, v, op)
        assert op == {(0, 0): 0, (1, 0): 4, (0, 1): 6, (1, 1): 2}[(h, v)]
    assert len(seen) == 4
    assert np.array_equal(ops, np.array([0, 4, 6, 2])[fh + 2 * fv])


def test_dihedral_ops_no_flag_draws_nothing():
    from bathymetric_gnn_amd.training import dihedral_ops
    rng = np.random.default_rng(8)
    before = rng.bit_generator.state
    ops = dihedral_ops(17, False, False, rng)
    assert ops.dtype == np.int8 and ops.shape == (17,) and not ops.any()
    assert rng.bit_generator.state == before
    assert dihedral_ops(0, True, True, rng).shape == (0,)


def test_transformed_tile_table_swaps_for_odd_k():
    from bathymetric_gnn_amd.training import transformed_tile_table
    hw = np.array([(3 + op, 20 + op) for op in range(8)], np.int32)
    res = np.array([(0.5 + op, 8.0 + op) for op in range(8)], np.float64)
    ops = np.arange(8, dtype=np.int8)
    hw2, res2 = transformed_tile_table(hw, res, ops)
    assert hw2.dtype == np.int32 and res2.dtype == np.float64 and hw2.flags.c_contiguous and res2.flags.c_contiguous
    for op in range(8):
        assert tuple(hw2[op]) == apply_op(np.zeros(tuple(hw[op])), op).shape
        assert tuple(hw2[op]) == (tuple(hw[op][::-1]) if op & 1 else tuple(hw[op]))
        assert tuple(res2[op]) == (tuple(res[op][::-1]) if op & 1 else tuple(res[op]))
    assert np.array_equal(hw, [(3 + op, 20 + op) for op in range(8)])              # the inputs are not written
    with pytest.raises(ValueError):
        transformed_tile_table(hw, res, ops[:5])
    with pytest.raises(ValueError):
        transformed_tile_table(hw, res, np.full(8, 8))
    with pytest.raises(ValueError):
        transformed_tile_table(hw, res, np.full(8, -1))


class _Len:
    def __init__(self, n):
        self.n = n

    def __len__(self):
        return self.n


def _planner(seed, n=23, rotations=True, flips=True):
    """A Trainer with nothing but what ``augment_plan`` may read: the store's length, the seed, the settings."""
    from bathymetric_gnn_amd.training import Trainer
    t = Trainer.__new__(Trainer)
    t.train_store, t.seed = _Len(n), seed
    t.settings = SimpleNamespace(augment_rotations=rotations, augment_flips=flips)
    return t


def test_augment_plan_is_a_function_of_seed_and_epoch():
    from bathymetric_gnn_amd.training import dihedral_ops
    a, b = _planner(3), _planner(3)
    for epoch in (0, 1, 7):
        plan = a.augment_plan(epoch)
        assert plan.dtype == np.int8 and plan.shape == (23,)
        assert np.array_equal(plan, dihedral_ops(23, True, True, np.random.default_rng([3, epoch, 0xA6])))
        assert np.array_equal(plan, b.augment_plan(epoch))
    assert np.array_equal(a.augment_plan(1), b.augment_plan(1))                    # whatever was asked before
    assert not np.array_equal(a.augment_plan(0), a.augment_plan(1))
    assert not np.array_equal(a.augment_plan(0), _planner(4).augment_plan(0))
    assert set(_planner(3, 200, True, False).augment_plan(0).tolist()) == {0, 1, 2, 3}
    assert set(_planner(3, 200, False, True).augment_plan(0).tolist()) == {0, 2, 4, 6}
    assert not _planner(3, 200, False, False).augment_plan(0).any()


def test_training_defaults_keep_both_flags():
    from bathymetric_gnn_amd.training import training_settings
    s = training_settings(None)
    assert s.augment_rotations is True and s.augment_flips is True
    s = training_settings({"augment_rotations": False})
    assert s.augment_rotations is False and s.augment_flips is True
