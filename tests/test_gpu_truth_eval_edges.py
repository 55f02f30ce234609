"""Ground truth and evaluation on the device (csrc/ground_truth.hip) where the fixtures do not reach: planes past the largest grid
a streaming pass launches, so that every workgroup walks its grid-stride loop two or three times and the finishing kernels add a
full set of partial rows; the selection on keys built to be awkward; evaluation on odd values.  The yardstick throughout is the
numpy oracle of _eval_checks.py (``truth_oracle``, ``numpy_eval_block``): labels and integers with ``==``, planes and the offset by
value, float sums within ``sum_tolerance``.  tests/test_host_ground_truth.py checks the inputs themselves without a GPU."""
import numpy as np
import pytest
import torch

from _eval_checks import (ADVERSARIAL_CASES, PAST_ONE_GRID_CELLS, adversarial_case, adversarial_truth, check_metrics, check_truth,
                          numpy_eval_block, odd_eval_planes, past_one_grid_eval, past_one_grid_pair, past_one_grid_truth)

pytestmark = pytest.mark.gpu
INT_FIELDS = ("total", "correct", "confusion", "covered", "covered_correct", "conf_cells")
SUM_FIELDS = ("conf_sum", "conf_sq", "conf_correct_sum", "conf_incorrect_sum")


def _device(arrays, device):
    return tuple(torch.from_numpy(np.array(a)).to(device) for a in arrays)      # (a copy: the shared arrays are read-only)


def _build(*args, **kw):
    """``ground_truth_build`` with everything copied to the host: ``(labels, difference, uncertainty or None, block record)``."""
    from bathymetric_gnn_amd import runtime
    from bathymetric_gnn_amd.data.ground_truth import ground_truth_build
    lab, diff, unc, stats = ground_truth_build(*args, **kw)
    block = np.frombuffer(stats.cpu().numpy().tobytes(), np.dtype(runtime.GT_STATS_DTYPE))[0]
    return lab.cpu().numpy(), diff.cpu().numpy(), None if unc is None else unc.cpu().numpy(), block


def _assert_equal_bits(a, b, planes=(0, 1, 2, 3)):
    for k in planes:
        assert (a[k] is None and b[k] is None) or a[k].tobytes() == b[k].tobytes(), k


def _assert_integers(got, want, fields=INT_FIELDS):
    for field in fields:
        assert np.array_equal(got[field], want[field]), (field, got[field], want[field])


def test_the_planes_are_past_the_largest_grid(gpu_device):
    """The workspaces hold one partial row per workgroup: they grow with the grid and stop growing at the largest one."""
    from bathymetric_gnn_amd import runtime as rt
    lib = rt.get_context(gpu_device).lib
    cells = PAST_ONE_GRID_CELLS
    for size in (lib.bgnn_ground_truth_workspace_bytes, lib.bgnn_eval_workspace_bytes):
        assert size(cells) == size(2 * cells) > size(cells // 4)
        assert size(cells - 1) == size(cells) == size(cells - 4101) == size(cells // 2 + 1)     # the slices and parts used below


# ---- 1. ground truth past one grid ------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def pair(gpu_device):
    """The pair on the device and the host copy of one call on it."""
    planes = _device(past_one_grid_pair(), gpu_device)
    assert all(t.data_ptr() % 16 == 0 and t.numel() == PAST_ONE_GRID_CELLS for t in planes)
    return planes, _build(*planes, 0.15)


def test_ground_truth_past_one_grid_against_numpy(pair):
    _, got = pair
    check_truth(*got, past_one_grid_truth())


def test_ground_truth_past_one_grid_unaligned_slices(pair):
    """``[1:]`` of each plane starts 4 bytes off a 16-byte boundary: the element-wise path through its later trips and tail."""
    planes, _ = pair
    sliced = tuple(t[1:] for t in planes)
    assert all(t.data_ptr() % 16 == 4 and t.is_contiguous() for t in sliced)
    got = _build(*sliced, 0.15)
    check_truth(*got, past_one_grid_truth(1))
    aligned = tuple(t.clone() for t in sliced)
    assert all(t.data_ptr() % 16 == 0 for t in aligned)
    _assert_equal_bits(got, _build(*aligned, 0.15))           # the statistics block too, bit for bit


def test_ground_truth_past_one_grid_twice_gives_equal_bits(pair):
    planes, first = pair
    _assert_equal_bits(first, _build(*planes, 0.15))


def test_ground_truth_past_one_grid_without_uncertainty(pair):
    planes, first = pair
    got = _build(planes[0], planes[1], None, 0.15)
    assert got[2] is None
    _assert_equal_bits(first, got, planes=(0, 1, 3))


# ---- 2. evaluation past one grid --------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def eval_planes(gpu_device):
    """The planes on the device, the block of one ``add`` of all three and the numpy block."""
    from bathymetric_gnn_amd.training import Evaluator
    planes = _device(past_one_grid_eval(), gpu_device)
    assert all(t.data_ptr() % 16 == 0 for t in planes)
    ev = Evaluator(gpu_device)
    ev.add(*planes)
    return planes, ev.block(), numpy_eval_block(*past_one_grid_eval())


def test_evaluation_past_one_grid_against_numpy(eval_planes, gpu_device):
    from bathymetric_gnn_amd.training import Evaluator, metrics_from_block
    planes, got, want = eval_planes
    _assert_integers(got, want)
    check_metrics(metrics_from_block(got), metrics_from_block(want), *past_one_grid_eval(), fixture=False)
    again = Evaluator(gpu_device)
    again.add(*planes)
    assert again.block().tobytes() == got.tobytes()


def test_evaluation_past_one_grid_unaligned_slices(eval_planes, gpu_device):
    from bathymetric_gnn_amd.training import Evaluator
    planes, _, _ = eval_planes
    sliced = tuple(t[1:] for t in planes)
    assert all(t.data_ptr() % 16 == 4 for t in sliced)
    ev = Evaluator(gpu_device)
    ev.add(*sliced)
    _assert_integers(ev.block(), numpy_eval_block(*(a[1:] for a in past_one_grid_eval())))


def test_evaluation_past_one_grid_in_two_calls(eval_planes, gpu_device):
    """One part past the largest grid, one of 4101 cells; the split is no multiple of 4, so the second part is read element-wise."""
    from bathymetric_gnn_amd.training import Evaluator, metrics_from_block
    planes, whole, _ = eval_planes
    split = PAST_ONE_GRID_CELLS - 4101
    assert split % 4 == 2 and planes[1][split:].data_ptr() % 16 == 8
    ev = Evaluator(gpu_device)
    ev.add(*(t[:split] for t in planes))
    ev.add(*(t[split:] for t in planes))
    _assert_integers(ev.block(), whole)
    check_metrics(ev.metrics(), metrics_from_block(eval_planes[2]), *past_one_grid_eval(), fixture=False)


def test_evaluation_past_one_grid_without_confidence(eval_planes, gpu_device):
    from bathymetric_gnn_amd.training import Evaluator
    planes, whole, _ = eval_planes
    ev = Evaluator(gpu_device)
    ev.add(planes[0], planes[1])
    got = ev.block()
    _assert_integers(got, whole, ("total", "correct", "confusion"))
    assert int(got["conf_cells"]) == 0 and not got["covered"].any() and not got["covered_correct"].any()
    assert all(got[k].tobytes() == bytes(8) for k in SUM_FIELDS)


# ---- 3. the selection on adversarial keys -----------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ADVERSARIAL_CASES)
def test_selection_on_adversarial_keys(name, gpu_device):
    c, want = adversarial_case(name), adversarial_truth(name)
    planes = _device((c.clean, c.noisy, c.unc), gpu_device)
    got = _build(*planes, c.threshold, nodata=c.nodata)
    print(f"{name}: offset {got[3]['offset']!r} against {want.offset!r}")
    check_truth(*got, want, sums=c.sums)
    if name == "overflow_tails":
        with np.errstate(over="ignore"):
            inf = np.isinf(c.noisy - c.clean) & want.valid
        assert inf.sum() == 7 and (got[0][inf] == 2).all() and np.isinf(got[1][inf]).all() and got[3]["noise_abs_max"] == np.inf
    if name == "denormals":                                   # equal in value is not enough to tell a flushed zero's sign apart
        assert np.array_equal(got[1][want.valid].view(np.uint32), want.difference[want.valid].view(np.uint32))
        assert np.float32(got[3]["offset"]).view(np.uint32) == want.offset.view(np.uint32)


# ---- 4. evaluation on odd values --------------------------------------------------------------------------------------------
def test_evaluation_on_odd_values(gpu_device):
    """351 cells against ``numpy_eval_block``.  Not pinned by the fixtures of make_golden_eval.py before: the predictions -0.0
    (class 0), 2.9999998 (class 2), 1e30 (counted, ">= 3") and -0.5 (dropped; the fixtures' only negative is -1.0); the labels
    INT32_MAX and INT32_MIN; confidences below 0 and above 1; and the threshold edges on anything but label 0 with predictions
    0 / 1.  Already there, and repeated in the mix: +-inf predictions (``random``), label and prediction 3 (``high_classes``),
    ``float32(t)`` with both neighbours (``threshold_edges``)."""
    from bathymetric_gnn_amd.training import Evaluator, metrics_from_block
    labels, pred, conf = odd_eval_planes()
    ev = Evaluator(gpu_device)
    ev.add(labels.copy(), pred.copy(), conf.copy())
    got, want = ev.block(), numpy_eval_block(labels, pred, conf)
    _assert_integers(got, want)
    check_metrics(ev.metrics(), metrics_from_block(want), labels, pred, conf, fixture=False)
