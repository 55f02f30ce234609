"""The locale guide past one launch grid: 800 x 700 planes are more than 2048 tiles of 256 cells, so the stride over the tiles takes
a second trip, with partial tiles along every row of tiles.  ``guide`` and ``support`` for equal bits against the numpy restatement
(_locale_cpu.locale_guide_np; test_host_locale.py holds it against the Python integers), at the default radius and the largest."""
import functools

import numpy as np
import pytest
import torch

import _locale_cpu as lc

pytestmark = pytest.mark.gpu

SHAPE = (800, 700)


@functools.lru_cache(maxsize=None)
def _planes():
    """Half of the cells witnesses in the west, one in ten in the east, a band of rows without any: supports from 0 to the whole
    window.  Depths of a sloping seabed plus noise, so that neighbouring values are close but rarely equal, and a block of ties."""
    rng = np.random.default_rng(83)
    n_hyp, chosen, _ = lc.random_planes(rng, SHAPE, 0.5, 1)
    thin = lc.random_planes(rng, SHAPE, 0.1, 1)
    n_hyp[:, 350:], chosen[:, 350:] = thin[0][:, 350:], thin[1][:, 350:]
    n_hyp[400:420], chosen[400:420] = 2, 1
    slope = -20.0 - 0.05 * np.arange(SHAPE[0])[:, None] - 0.02 * np.arange(SHAPE[1])[None, :]
    c2 = np.rint((slope + 0.2 * rng.standard_normal(SHAPE)) * 131072.0).astype(np.int64)
    c2[100:140, 100:160] = -25 * 131072
    for a in (n_hyp, chosen, c2):
        a.setflags(write=False)
    return n_hyp, chosen, c2


@pytest.mark.parametrize("radius,min_support", [(2, 3), (8, 20)])
def test_past_one_grid(radius, min_support, gpu_device):
    from bathymetric_gnn_amd.data import locale_guide_planes
    planes = _planes()
    tiles = -(-SHAPE[0] * SHAPE[1] // 256)
    assert tiles > 2048 and SHAPE[1] % 32 and SHAPE[1] % 16
    want_g, want_s = lc.locale_guide_np(*planes, radius, min_support)
    window = (2 * radius + 1) ** 2 - 1
    assert want_s.min() == 0 and want_s.max() > window // 2 and (want_g == lc.NAN_BITS).any() and (want_g != lc.NAN_BITS).sum() > 300000
    dev = [torch.from_numpy(a.copy()).to(gpu_device) for a in planes]
    guide, support = locale_guide_planes(*dev, radius, min_support)
    got_g, got_s = guide.cpu().numpy().view(np.uint32), support.cpu().numpy()
    for name, g, w in (("support", got_s, want_s), ("guide", got_g, want_g)):
        differ = np.argwhere(g != w)
        assert differ.size == 0, (name, len(differ), differ[:4].tolist())
    again = locale_guide_planes(*dev, radius, min_support)
    assert torch.equal(again[1], support) and torch.equal(again[0].view(torch.int32), guide.view(torch.int32))
