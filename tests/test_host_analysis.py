"""The host half of the noise pattern analysis without a GPU: the result block of include/bgnn_analysis.h is built in numpy / scipy
from every fixture's planes (_analysis_cpu.numpy_analysis_block), the package's own ``analysis_from_block`` assembles the
dictionary, and that dictionary is held to the one the reference returned for the same planes (tests/golden/analysis, written by
make_golden_analysis.py) under the rules of _analysis_cpu.  ``print_analysis`` must write the reference's text."""
import math

import numpy as np
import pytest

from _analysis_cpu import (ANALYSIS_CASES, MAGNITUDE_KEY_CASES, STRICT_CASES, check_analysis, load_analysis_case, magnitude_key_case,
                           numpy_analysis, numpy_analysis_block, ulps_apart)

EXPECTED = {"mixed_97x203", "serpentine_128", "comb_130x67", "checkerboard_64", "all_noise_128", "two_clusters_even", "no_noise",
            "no_seafloor", "bin_edges", "inf_neighbour", "one_row_1x300", "one_col_300x1", "one_cell", "percentile_ranks_101",
            "percentile_ranks_1001", "percentile_ranks_157", "ties"}


def test_the_fixtures_are_all_there():
    assert set(ANALYSIS_CASES) == EXPECTED and set(STRICT_CASES) == {n for n in EXPECTED if n.startswith(("percentile", "ties"))}


@pytest.mark.parametrize("name", ANALYSIS_CASES)
def test_fixture_dictionary(name):
    planes, want, _ = load_analysis_case(name)
    got = numpy_analysis(*planes, file=name + ".tif")
    check_analysis(got, want, planes, strict=name in STRICT_CASES)


@pytest.mark.parametrize("name", ANALYSIS_CASES)
def test_report_text(name, capsys):
    from bathymetric_gnn_amd.data import print_analysis
    _, want, report = load_analysis_case(name)
    print_analysis(want)
    assert capsys.readouterr().out == report


def test_float32_label_band_reads_as_the_reference_reads_it():
    planes, want, _ = load_analysis_case("mixed_97x203")
    band = planes[0].astype(np.float32)
    got = numpy_analysis(band, *planes[1:], file="mixed_97x203.tif")
    check_analysis(got, want, planes)


def test_percentile_ranks_follow_numpy():
    """The ranks and weights ``np.percentile`` itself uses on float32 data, over counts around every rounding case."""
    from bathymetric_gnn_amd.data.noise_analysis import _lerp, magnitude_ranks
    rng = np.random.default_rng(7)
    for n in list(range(1, 60)) + [101, 102, 157, 1000, 1001, 4097]:
        v = np.sort(rng.random(n, dtype=np.float32))
        ranks, g90, g99 = magnitude_ranks(n)
        assert float(np.median(v)) == float(v[ranks[0]] if n % 2 else np.float32(v[ranks[0]] + v[ranks[1]]) / np.float32(2))
        assert np.percentile(v, 90) == _lerp(v[ranks[2]], v[ranks[3]], g90), n
        assert np.percentile(v, 99) == _lerp(v[ranks[4]], v[ranks[5]], g99), n


@pytest.mark.parametrize("name", MAGNITUDE_KEY_CASES)
def test_restatement_takes_the_ground_truths_adversarial_keys(name):
    """What tests/test_gpu_noise_analysis.py holds the six-rank selection to: the restatement accepts the ground truth's
    constructed keys as magnitudes (all finite, every cell noise), and its order statistics are numpy's own."""
    from bathymetric_gnn_amd.data.noise_analysis import analysis_from_block
    planes, block, cn, cv = magnitude_key_case(name)
    mag = planes[1].reshape(-1)
    assert int(block["noise"]) == mag.size and int(block["nonfinite"]) == 0 and 1001 <= mag.size <= 4099
    m = analysis_from_block(block, cn, cv, planes[0].shape, name)["magnitude"]
    assert m["median"] == float(np.median(mag)) and m["max"] == float(mag.max())
    assert ulps_apart(m["p90"], np.percentile(mag, 90)) <= 1 and ulps_apart(m["p99"], np.percentile(mag, 99)) <= 1


def test_nonfinite_noise_difference_is_refused():
    from bathymetric_gnn_amd.data.noise_analysis import analysis_from_block
    planes, _, _ = load_analysis_case("two_clusters_even")
    difference = planes[1].copy()
    difference[2, 4] = np.inf
    block, cn, cv = numpy_analysis_block(planes[0], difference, planes[2], planes[3])
    assert int(block["nonfinite"]) == 1
    with pytest.raises(ValueError, match="not finite"):
        analysis_from_block(block, cn, cv, planes[0].shape)


def test_restatement_content():
    """What the block holds for cases whose answer is known by construction."""
    block, cn, cv = numpy_analysis_block(*load_analysis_case("checkerboard_64")[0])
    assert int(block["num_clusters"]) == int(block["isolated"]) == 2048 == int(block["noise"]) and list(block["size_mid"]) == [1, 1]
    assert cn.tolist() == [32] * 64 and cv.tolist() == [64] * 64
    block, _, _ = numpy_analysis_block(*load_analysis_case("all_noise_128")[0])
    assert int(block["num_clusters"]) == 1 and int(block["max_cluster"]) == 16384 and not block["size_bins"].any()
    assert int(block["rough_count"][1]) == 0 and math.isnan(float(block["rough_mid"][2]))
