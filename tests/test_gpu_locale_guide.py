"""The locale guide on the device (bgnn_locale_guide, data.locale_guide_planes) on raw planes against the restatement of
_locale_cpu.py (test_host_locale.py guards the restatement itself): ``guide`` and ``support`` for equal bits, on grids smaller than
the window, partial tiles on both axes, every share of witnesses, ties and the full range of values, and hand-made cells.  Two
device runs must leave equal bytes."""
import numpy as np
import pytest
import torch

import _locale_cpu as lc

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1), (1, 40), (40, 1), (3, 5), (17, 33), (37, 53)]
RADII = [1, 2, 3, 8]
SHARES = [0.0, 0.1, 0.5, 1.0]
SPREADS = [8, lc.VALUE_TOP]                              # a 16-value range (ties), and the full one
PYTHON_CELLS = 200                                       # up to here the Python-integer restatement, the numpy one above


def _run(device, n_hyp, chosen, center2, radius, min_support):
    from bathymetric_gnn_amd.data import locale_guide_planes
    planes = [torch.from_numpy(np.ascontiguousarray(a)).to(device) for a in (n_hyp, chosen, center2)]
    guide, support = locale_guide_planes(*planes, radius, min_support)
    assert guide.dtype == torch.float32 and support.dtype == torch.int32 and guide.device == support.device == planes[0].device
    assert tuple(guide.shape) == tuple(support.shape) == n_hyp.shape and guide.is_contiguous() and support.is_contiguous()
    return guide.cpu().numpy().view(np.uint32), support.cpu().numpy()


def _same(got, want, what):
    for name, g, w in zip(("guide", "support"), got, want):
        assert g.dtype == w.dtype and g.shape == w.shape, (name, what)
        differ = np.argwhere(g != w)
        assert differ.size == 0, (name, what, len(differ), differ[:4].tolist(), [int(g[tuple(i)]) for i in differ[:4]],
                                  [int(w[tuple(i)]) for i in differ[:4]])


@pytest.mark.parametrize("radius", RADII)
@pytest.mark.parametrize("shape", SHAPES)
def test_planes(shape, radius, gpu_device):
    rng = np.random.default_rng(1000 * radius + 53 * shape[0] + shape[1])
    restate = lc.locale_guide if shape[0] * shape[1] <= PYTHON_CELLS else lc.locale_guide_np
    seen_nan = seen_value = 0
    for share in SHARES:
        for spread in SPREADS:
            planes = lc.random_planes(rng, shape, share, spread)
            for min_support in (1, 3, (2 * radius + 1) ** 2 - 1):
                want = restate(*planes, radius, min_support)
                got = _run(gpu_device, *planes, radius, min_support)
                _same(got, want, (share, spread, min_support))
                seen_nan += int((want[0] == lc.NAN_BITS).sum())
                seen_value += int((want[0] != lc.NAN_BITS).sum())
    assert seen_nan > 0 and (seen_value > 0 or shape == (1, 1))
    # two runs, equal bytes
    a, b = (_run(gpu_device, *planes, radius, 1) for _ in range(2))
    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()


def test_python_restatement_on_the_larger_shapes(gpu_device):
    """The numpy form stands in for the Python integers above 200 cells; here the Python integers themselves, once per shape."""
    rng = np.random.default_rng(7)
    for shape, radius, share in (((17, 33), 3, 0.5), ((37, 53), 2, 0.1), ((17, 33), 8, 1.0)):
        planes = lc.random_planes(rng, shape, share, lc.VALUE_TOP)
        _same(_run(gpu_device, *planes, radius, 3), lc.locale_guide(*planes, radius, 3), (shape, radius))


def _cells(shape, witnesses, others=()):
    """Planes where only ``witnesses`` ({(r, c): value}) are witnesses; ``others`` ({(r, c): value}) carry a value without being
    one (two hypotheses)."""
    n_hyp, chosen, c2 = np.zeros(shape, np.int32), np.full(shape, -1, np.int32), np.zeros(shape, np.int64)
    for (r, c), v in witnesses.items():
        n_hyp[r, c], chosen[r, c], c2[r, c] = 1, 0, v
    for (r, c), v in dict(others).items():
        n_hyp[r, c], chosen[r, c], c2[r, c] = 2, 0, v
    return n_hyp, chosen, c2


def test_hand_made_cells(gpu_device):
    bits = lambda v: int(np.float32(v).view(np.uint32))
    M = 131072                                                                        # one metre of center2
    # k = min_support - 1 and k = min_support; k odd and k even; the centre's own wild value
    w = {(4, 4): -30 * M, (4, 6): -31 * M, (6, 4): -29 * M, (5, 5): lc.VALUE_TOP}
    planes = _cells((11, 12), w)
    for min_support, want_55 in ((3, bits(-30.0)), (4, lc.NAN_BITS)):
        g, s = _run(gpu_device, *planes, 1, min_support)
        _same((g, s), lc.locale_guide(*planes, 1, min_support), min_support)
        assert s[5, 5] == 3 and g[5, 5] == want_55                                     # k odd: the middle one, twice
        assert s[4, 5] == 3 and g[4, 5] == (bits(-30.0) if min_support == 3 else lc.NAN_BITS)     # -30, -31 and the wild one
        assert s[5, 4] == 3 and s[4, 4] == 1 and s[0, 0] == 0 and g[0, 0] == lc.NAN_BITS
    w[(6, 6)] = -33 * M
    planes = _cells((11, 12), w)
    g, s = _run(gpu_device, *planes, 1, 4)
    _same((g, s), lc.locale_guide(*planes, 1, 4), "k even")
    assert s[5, 5] == 4 and g[5, 5] == bits(-30.5)                                     # -33, -31 | -30, -29: the two middle ones
    assert s[6, 5] == 3 and g[6, 5] == lc.NAN_BITS                                     # -29, -33 and the wild one: k = min_support - 1
    # a cell that carries a value without being a witness does not count, whatever it holds
    planes = _cells((11, 12), w, {(5, 4): -1000 * M, (5, 6): lc.VALUE_TOP})
    g, s = _run(gpu_device, *planes, 1, 4)
    assert s[5, 5] == 4 and g[5, 5] == bits(-30.5)
    # med2 = 2^33 - 2 needs 34 bits with its sign: one rounding, and it rounds to 32768.0, which the guide rule reads as "by count"
    planes = _cells((1, 3), {(0, 0): lc.VALUE_TOP, (0, 2): lc.VALUE_TOP})
    g, s = _run(gpu_device, *planes, 1, 2)
    assert s.tolist() == [[0, 2, 0]] and g[0, 1] == bits(32768.0) == lc.guide_bits(2 ** 33 - 2) and g[0, 0] == lc.NAN_BITS
    planes = _cells((3, 1), {(0, 0): -lc.VALUE_TOP, (2, 0): -lc.VALUE_TOP})
    g, s = _run(gpu_device, *planes, 8, 1)
    assert s.tolist() == [[1], [2], [1]] and g[:, 0].tolist() == [bits(-32768.0)] * 3
    # the sum is formed in integers: 2^25 + 1 and 2^25 + 5 are no float32 each, their sum 2^26 + 6 rounds up to 256 + 2^-15
    planes = _cells((1, 3), {(0, 0): 2 ** 25 + 1, (0, 2): 2 ** 25 + 5})
    g, s = _run(gpu_device, *planes, 1, 2)
    assert g[0, 1] == lc.guide_bits(2 ** 26 + 6) == bits(256.0 + 2.0 ** -15)
    # NaN bits exactly 0x7FC00000 in a plane without any witness
    g, s = _run(gpu_device, *_cells((9, 70), {}), 2, 1)
    assert (g == 0x7FC00000).all() and (s == 0).all()


def test_argument_checks(gpu_device):
    from bathymetric_gnn_amd.data import locale_guide_planes
    n_hyp = torch.ones((6, 7), dtype=torch.int32, device=gpu_device)
    chosen = torch.zeros((6, 7), dtype=torch.int32, device=gpu_device)
    c2 = torch.zeros((6, 7), dtype=torch.int64, device=gpu_device)
    g, s = locale_guide_planes(n_hyp, chosen, c2)                                     # radius 2, min_support 3
    assert s[0, 0] == 8 and s[3, 3] == 24 and (g == 0).all()
    with pytest.raises(TypeError, match="n_hyp"):
        locale_guide_planes(n_hyp.long(), chosen, c2)
    with pytest.raises(TypeError, match="chosen"):
        locale_guide_planes(n_hyp, chosen.float(), c2)
    with pytest.raises(TypeError, match="center2"):
        locale_guide_planes(n_hyp, chosen, c2.int())
    with pytest.raises(TypeError, match="device tensor"):
        locale_guide_planes(n_hyp, chosen.cpu().numpy(), c2)
    with pytest.raises(TypeError, match="chosen is on cpu"):
        locale_guide_planes(n_hyp, chosen.cpu(), c2)
    with pytest.raises(TypeError, match="GPU tensor"):
        locale_guide_planes(n_hyp.cpu(), chosen.cpu(), c2.cpu())
    with pytest.raises(ValueError, match="shape"):
        locale_guide_planes(n_hyp, chosen[:5], c2)
    with pytest.raises(ValueError, match="shape"):
        locale_guide_planes(n_hyp.view(-1), chosen.view(-1), c2.view(-1))
    with pytest.raises(ValueError, match="contiguous"):
        locale_guide_planes(n_hyp, chosen, torch.zeros((7, 6), dtype=torch.int64, device=gpu_device).t())
    for radius in (0, 9, -1):
        with pytest.raises(ValueError, match="radius"):
            locale_guide_planes(n_hyp, chosen, c2, radius, 1)
    for radius, min_support in ((1, 0), (1, 9), (2, 25), (8, 289)):
        with pytest.raises(ValueError, match="min_support"):
            locale_guide_planes(n_hyp, chosen, c2, radius, min_support)
    for radius, min_support in ((2.0, 3), (2, 3.0), (True, 3), ("2", 3)):
        with pytest.raises(TypeError, match="integer"):
            locale_guide_planes(n_hyp, chosen, c2, radius, min_support)
