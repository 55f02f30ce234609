"""The host halves of ground truth and evaluation against the reference's fixtures (tests/golden/truth, tests/golden/eval; written
by the reference's own scripts, see make_golden_truth.py / make_golden_eval.py): the alignment of a survey pair, and the two
dictionaries derived from a device block -- here from blocks built in numpy by the blocks' definitions.  No GPU needed."""
import json
import os

import numpy as np
import pytest

from _eval_checks import (EVAL_CASES, GOLDEN, TRUTH_CASES, check_metrics, check_stats, grids_of, load_case, numpy_eval_block,
                          numpy_stats_block, truth_bands)


def test_fixture_sets():
    assert len(TRUTH_CASES) == 16 and "extents" in TRUTH_CASES and "large" in TRUTH_CASES
    assert len(EVAL_CASES) == 11 and "threshold_edges" in EVAL_CASES


@pytest.mark.parametrize("name", TRUTH_CASES)
def test_align_survey_pair_cuts_what_the_reference_cut(name):
    from bathymetric_gnn_amd.data import align_survey_pair
    g, _ = load_case("truth", name)
    clean, noisy = grids_of(g)
    al = align_survey_pair(clean, noisy)
    bands = truth_bands(g)
    cr0, cr1, cc0, cc1 = al.clean_window
    nr0, nr1, nc0, nc1 = al.noisy_window
    assert al.shape == g["labels"].shape == (cr1 - cr0, cc1 - cc0) == (nr1 - nr0, nc1 - nc0)
    assert np.array_equal(clean.depth[cr0:cr1, cc0:cc1].view(np.uint32), bands[3].view(np.uint32))
    assert np.array_equal(noisy.depth[nr0:nr1, nc0:nc1].view(np.uint32), bands[2].view(np.uint32))
    assert al.transform == tuple(float(v) for v in g["geotransform"])
    if name == "extents":
        assert al.clean_window == (3, 40, 6, 50) and al.noisy_window == (0, 37, 0, 44)      # 1.3 m / 0.5 m rounds to 3, 3.2 / 0.5 to 6
    else:
        assert al.clean_window == al.noisy_window == (0, clean.depth.shape[0], 0, clean.depth.shape[1])


def test_align_survey_pair_refusals_carry_the_reference_messages():
    from bathymetric_gnn_amd.data import BathymetricGrid, align_survey_pair
    errors = json.load(open(os.path.join(GOLDEN, "truth", "errors.json")))
    assert sorted(errors) == ["no_overlap", "resolution"]
    for name, e in errors.items():
        grids = [BathymetricGrid(depth=np.zeros((8, 8), np.float32), transform=tuple(e[s + "_transform"]),
                                 resolution=tuple(e[s + "_resolution"]), bounds=tuple(e[s + "_bounds"])) for s in ("clean", "noisy")]
        with pytest.raises(ValueError) as info:
            align_survey_pair(*grids)
        assert str(info.value) == e["message"], name


@pytest.mark.parametrize("name", TRUTH_CASES)
def test_stats_from_a_block(name):
    """``ground_truth_stats`` on a block filled in numpy from the reference's own planes gives the reference's JSON."""
    from bathymetric_gnn_amd.data import ground_truth_stats
    g, want = load_case("truth", name)
    bands = truth_bands(g)
    block = numpy_stats_block(g["labels"], bands[1], g["offset"])
    got = ground_truth_stats(block, float(g["threshold"]), g["labels"].shape, f"{name}_clean.bag", f"{name}_noisy.bag")
    assert got["clean_survey"] == want["clean_survey"] and got["noisy_survey"] == want["noisy_survey"]
    check_stats(got, want, g["labels"], bands[1])
    assert json.dumps(got)                                    # plain Python types throughout


@pytest.mark.parametrize("name", EVAL_CASES)
def test_metrics_from_a_block(name):
    """``metrics_from_block`` on a block counted in numpy gives the reference's dictionary: keys, Python types, integers and ratios
    exactly, the float sums within the float64 bound."""
    from bathymetric_gnn_amd.training import metrics_from_block
    g, want = load_case("eval", name)
    conf = g.get("confidence")
    got = metrics_from_block(numpy_eval_block(g["labels"], g["classification"], conf), with_confidence=conf is not None)
    check_metrics(got, want, g["labels"], g["classification"], conf)
    assert json.dumps(got)


def test_blocks_accumulate_like_one_call():
    """Adding the blocks of three uneven row bands field by field is the block of the whole plane in every integer."""
    g, _ = load_case("eval", "random")
    whole = numpy_eval_block(g["labels"], g["classification"], g["confidence"])
    parts = [numpy_eval_block(g["labels"][a:b], g["classification"][a:b], g["confidence"][a:b]) for a, b in ((0, 5), (5, 31), (31, 48))]
    for field in ("total", "correct", "confusion", "covered", "covered_correct", "conf_cells"):
        assert np.array_equal(sum(p[field] for p in parts), whole[field]), field
