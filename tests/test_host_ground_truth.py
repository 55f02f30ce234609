"""The host halves of ground truth and evaluation against the reference's fixtures (tests/golden/truth, tests/golden/eval; written
by the reference's own scripts, see make_golden_truth.py / make_golden_eval.py): the alignment of a survey pair, and the two
dictionaries derived from a device block -- here from blocks built in numpy by the blocks' definitions.  No GPU needed."""
import json
import os

import numpy as np
import pytest

from _eval_checks import (ADVERSARIAL_CASES, BIN_OWNER_KEYS, DENORMAL_LIMIT, EVAL_CASES, GOLDEN, NODATA, ODD_LABELS, ODD_PREDICTIONS,
                          PAST_ONE_GRID_CELLS, STRADDLE_KEYS, THRESHOLDS, TRUTH_CASES, adversarial_case, adversarial_truth, check_metrics,
                          check_stats, check_truth, counted_cells, grids_of, key_digits, key_value, load_case, median_rule,
                          numpy_eval_block, numpy_stats_block, odd_eval_planes, order_key, past_one_grid_eval, past_one_grid_pair,
                          past_one_grid_truth, truth_bands, truth_oracle)


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


# ---- the constructed inputs of test_gpu_truth_eval_edges.py: what each is named for, seen through the numpy key ----------------
F32 = np.float32


def _median_by_numpy(t):
    with np.errstate(invalid="ignore", over="ignore"):
        return np.median(t.raw[t.valid])


def test_order_key_and_its_inverse():
    v = np.array([-np.inf, -3e38, -1.0, -1e-45, -0.0, 0.0, 1e-45, 0.87499994, 0.875, 3e38, np.inf], F32)
    k = order_key(v)
    assert k.dtype == np.uint32 and (np.diff(k.astype(np.int64)) > 0).all() and int(k[5]) - int(k[4]) == 1
    assert np.array_equal(key_value(k).view(np.uint32), v.view(np.uint32))
    bits = np.random.default_rng(3).integers(0, 2 ** 32, 10000, dtype=np.uint64).astype(np.uint32)
    assert np.array_equal(order_key(key_value(bits)), bits)
    a, b = key_value(bits[:5000]), key_value(bits[5000:])
    with np.errstate(invalid="ignore"):
        ordered = ~np.isnan(a) & ~np.isnan(b) & (a != b)
        assert np.array_equal((a < b)[ordered], (bits[:5000] < bits[5000:])[ordered])
    assert key_digits(0xFFFFFFFF) == (0x7FF, 0x7FF, 0x3FF) and key_digits((5 << 21) | (6 << 10) | 7) == (5, 6, 7)


def test_median_rule_on_small_sets():
    assert np.isnan(median_rule([])) and median_rule([3.0]) == 3 and median_rule([4.0, 1.0]) == 2.5 and median_rule([9.0, 1.0, 2.0]) == 2
    lo, hi = F32(0.87499994), F32(0.875)
    assert median_rule([hi, lo]) == F32(lo + hi) / F32(2) == np.median(np.array([lo, hi]))


def test_past_one_grid_pair():
    clean, noisy, unc = past_one_grid_pair()
    t = past_one_grid_truth()
    n = int(t.valid.sum())
    assert clean.shape == (PAST_ONE_GRID_CELLS,) and PAST_ONE_GRID_CELLS % 2 == 1 and PAST_ONE_GRID_CELLS % 1024 == 3
    assert 0.955 * clean.size < n < 0.965 * clean.size and (clean == F32(NODATA)).any() and np.isnan(noisy).any()
    assert _median_by_numpy(t) == t.offset and abs(float(t.offset) + 0.05) < 0.001
    assert int(t.block["noise"]) > n // 2 > int(t.block["seafloor"]) > n // 4 and np.isnan(t.uncertainty[~t.valid]).all()
    shifted = past_one_grid_truth(1)                          # the cells of the unaligned slices
    assert shifted.labels.size == clean.size - 1 and _median_by_numpy(shifted) == shifted.offset
    assert np.array_equal(shifted.valid, t.valid[1:])


def test_truth_oracle_is_the_fixtures_rule():
    """The oracle of the new tests on a fixture the reference wrote: the same labels, planes, offset and block."""
    for name in ("even_low_bits", "holes", "large"):
        g, _ = load_case("truth", name)
        bands = truth_bands(g)
        t = truth_oracle(bands[3], bands[2], float(g["threshold"]), unc=bands[4])
        check_truth(g["labels"], bands[1], bands[4], numpy_stats_block(g["labels"], bands[1], g["offset"]), t)


@pytest.mark.parametrize("name", ADVERSARIAL_CASES)
def test_adversarial_case_has_the_property_it_is_named_for(name):
    c, t = adversarial_case(name), adversarial_truth(name)
    raw = t.raw[t.valid]
    n, keys = raw.size, np.sort(order_key(raw))               # (sorted as keys: numpy's sort leaves -0.0 and +0.0 as they come)
    lo, hi = int(keys[(n - 1) // 2]), int(keys[n // 2])       # the two middle keys (one key twice for an odd count)
    assert c.clean.ndim == 1 and c.clean.shape == c.noisy.shape == c.unc.shape and 1000 < c.clean.size < 5000
    assert 4 <= int((~t.valid).sum()) and n < c.clean.size    # invalid cells are mixed in
    assert _median_by_numpy(t) == t.offset, (name, _median_by_numpy(t), t.offset)
    assert not (raw == F32(c.nodata)).any() and (np.isfinite(raw).all() or name == "overflow_tails")
    if c.values is not None and name != "overflow_tails":     # clean is 0: the raw differences are the values, bit for bit
        assert np.array_equal(np.sort(order_key(c.values)), keys)
    if name.startswith("uniform_keys_"):
        assert n == int(name.rsplit("_", 1)[1]) and np.abs(raw).max() < 1e38
        for shift, bins in ((21, 2048), (10, 2048), (0, 1024)):
            # about two keys a bin: no bin holds even one key in a hundred, so a wave of 64 finds no bin to peel
            assert np.bincount((keys >> shift) & (bins - 1), minlength=bins).max() < n // 100, shift
        assert (np.sign(raw) < 0).sum() > n // 3 and (np.sign(raw) > 0).sum() > n // 3
        assert np.log2(np.abs(raw[raw != 0])).max() - np.log2(np.abs(raw[raw != 0])).min() > 200
    elif name in STRADDLE_KEYS:
        assert n % 2 == 0 and (lo, hi) == STRADDLE_KEYS[name] and hi == lo + 1
        dl, dh = key_digits(lo), key_digits(hi)
        if name == "straddle_level1":
            assert dh[0] == dl[0] + 1 and dl[1:] == (0x7FF, 0x3FF) and dh[1:] == (0, 0)
            assert (float(key_value(lo)), float(key_value(hi))) == (float(F32(0.87499994)), 0.875)
        else:
            assert dh[0] == dl[0] and dh[1] == dl[1] + 1 and dl[1] ^ dh[1] == 0x7FF and dl[2] == 0x3FF and dh[2] == 0
        assert (keys == lo).sum() == (keys == hi).sum() == 300              # many duplicates of both
        assert ((keys >> 21) == dl[0]).sum() > 350 and ((keys >> 21) == dh[0]).sum() > 350     # and other keys in their top bins
        assert (keys < lo).sum() == (keys > hi).sum() and t.offset == F32(key_value(lo) + key_value(hi)) / F32(2)
    elif name in BIN_OWNER_KEYS:
        assert n % 2 == 1 and lo == hi == BIN_OWNER_KEYS[name] and (keys == lo).sum() == 200
        first = name == "first_bin_owner"
        assert key_digits(lo)[1:] == ((0, 0) if first else (0x7FF, 0x3FF))
        # the rank sits on the bin's edge: the first copy of the smallest key under its prefix, or the last of the largest
        assert ((keys < lo).sum() == (n - 1) // 2) if first else ((keys <= lo).sum() == (n - 1) // 2 + 1)
        assert ((keys >> 21) == lo >> 21).sum() > 300
    elif name == "denormals":
        tiny = np.finfo(F32).tiny
        assert n == 1001 and (raw != 0).all() and (np.abs(raw) < DENORMAL_LIMIT).all() and (raw < 0).sum() > 400 < (raw > 0).sum()
        assert t.offset != 0 and abs(t.offset) < tiny
        d = t.difference[t.valid]
        assert (np.abs(d) < tiny).all() and (d != 0).sum() >= 999 and not t.labels[t.valid].any()            # numpy does not flush
        assert np.unique(raw).size > 990 and np.array_equal(d, raw - t.offset)
    elif name == "signed_zeros":
        zeros = raw == 0
        assert n % 2 == 0 and zeros.sum() > n // 2 and (np.signbit(raw[zeros]).sum(), (~np.signbit(raw[zeros])).sum()) == (300, 300)
        assert (float(key_value(lo)), float(key_value(hi))) == (0.0, 0.0) and hi == lo + 1 == 0x80000000     # -0.0 | +0.0
        assert t.offset == 0 and np.array_equal(t.difference[t.valid], raw)
    elif name == "overflow_tails":
        inf = np.isinf(t.raw) & t.valid
        assert (t.raw[inf] > 0).sum() == 3 and (t.raw[inf] < 0).sum() == 4 and np.isfinite(c.clean[inf]).all() and np.isfinite(c.noisy[inf]).all()
        assert np.isfinite(key_value(lo)) and np.isfinite(key_value(hi)) and np.isfinite(t.offset)
        assert (t.labels[inf] == 2).all() and t.block["noise_abs_max"] == np.inf
    elif name == "other_nodata":
        assert c.nodata == -9999.0 and c.values is None
        million = (c.clean == F32(1.0e6)) | (c.noisy == F32(1.0e6))
        assert ((c.clean == F32(-9999)) | (c.noisy == F32(-9999))).sum() > 100 and million.sum() > 30
        assert (t.valid & million).sum() > 25 and (t.labels[t.valid & million] == 2).all() and t.block["noise_abs_max"] > 9.0e5
        assert not t.valid[(c.clean == F32(-9999)) | (c.noisy == F32(-9999))].any()
        default = truth_oracle(c.clean, c.noisy, c.threshold, unc=c.unc)                 # the default nodata counts other cells
        assert int(default.block["valid"]) != int(t.block["valid"]) and default.block["noise_abs_max"] != t.block["noise_abs_max"]


def test_past_one_grid_eval_planes():
    labels, pred, conf = past_one_grid_eval()
    assert labels.shape == pred.shape == conf.shape == (PAST_ONE_GRID_CELLS,) and labels.dtype == np.int32 and pred.dtype == conf.dtype == F32
    assert sorted(np.unique(labels)) == [-1, 0, 1, 2, 4]
    b = numpy_eval_block(labels, pred, conf)
    valid, yt, yp = counted_cells(labels, pred)
    assert int(b["total"]) == int(valid.sum()) == int(b["conf_cells"]) and 0.86 * labels.size < int(b["total"]) < 0.885 * labels.size
    assert 0.85 < int(b["correct"]) / int(b["total"]) < 0.9 and int(b["confusion"].sum()) == int(b["total"]) and b["confusion"].all()
    assert int(b["correct"]) == int(np.trace(b["confusion"][:3, :3])) + int(((yt == 4) & (yp == 4)).sum())
    split = labels.size - 4101                                # the two-call test's split: no multiple of 4, one part past the grid
    parts = [numpy_eval_block(labels[a:z], pred[a:z], conf[a:z]) for a, z in ((0, split), (split, labels.size))]
    assert split % 4 != 0 and split > labels.size // 2
    for field in ("total", "correct", "confusion", "covered", "covered_correct", "conf_cells"):
        assert np.array_equal(parts[0][field] + parts[1][field], b[field]), field


def test_odd_eval_planes():
    from bathymetric_gnn_amd.training import metrics_from_block
    labels, pred, conf = odd_eval_planes()
    assert labels.shape == pred.shape == conf.shape == (351,) and np.isfinite(conf).all()
    cells = set(zip(labels.tolist(), pred.view(np.uint32).tolist()))
    assert cells == {(l, int(F32(p).view(np.uint32))) for l in ODD_LABELS for p in ODD_PREDICTIONS}
    for t in THRESHOLDS:
        e = F32(t)
        for v in (np.nextafter(e, F32(0)), e, np.nextafter(e, F32(1))):
            assert (conf == v).sum() >= 16
    assert (conf < 0).sum() > 30 and (conf > 1).sum() > 30
    valid, yt, yp = counted_cells(labels, pred)
    # counted: labels 0, 1, 2, 3, INT32_MAX with predictions -0.0, 2.9999998, 3.0, 1e30, 0.0, 1.0, 2.0
    assert 5 * 7 * 5 <= int(valid.sum()) <= 5 * 7 * 5 + 1     # (five times the pairs, and the one cell more)
    assert not valid[(pred == F32(-0.5)) | np.isinf(pred) | (labels < 0)].any() and valid[(labels >= 0) & np.signbit(pred) & (pred == 0)].all()
    assert (yp[(pred[valid] == F32(2.9999998))] == 2).all() and yp.max() == 2 ** 62 and yt.max() == 2 ** 31 - 1
    b = numpy_eval_block(labels, pred, conf)
    assert int(b["total"]) == int(valid.sum()) and int(b["confusion"].sum()) == int(b["total"]) and (b["confusion"][3] > 0).all()
    # -0.0 is class 0, 2.9999998 is class 2, 3.0 on label 3 is correct and outside the 3 x 3 matrix
    assert int(b["correct"]) == int((((labels == 0) & (pred == 0)) | ((labels == 1) & (pred == 1)) | ((labels == 2) & ((pred == 2) | (pred == F32(2.9999998))))
                                     | ((labels == 3) & (pred == 3))).sum())
    for j, t in enumerate(THRESHOLDS):
        assert int(b["covered"][j]) == int((conf[valid].astype(np.float64) >= float(F32(t))).sum())
    m = metrics_from_block(b)
    check_metrics(m, m, labels, pred, conf, fixture=False)
    assert json.dumps(m)
