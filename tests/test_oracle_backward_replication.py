"""The identity the replication tests of ``tests/test_gpu_backward_training.py`` rest on, checked on the oracle alone (no GPU):
B copies of one tile in one batch, dropout off, the per-node loss weights tiled B times -- in float64 the parameter gradient is
B x the single tile's, to float64 rounding.  The training-mode BatchNorm batch statistics of the copies are the tile's, and every
copy's self loops carry its own mean edge attributes."""
import numpy as np
import pytest
import torch

from oracle import graph_cpu
from test_gpu_backward import _loss_weights, oracle_grads

REL = 1e-12


@pytest.mark.parametrize("copies", [2, 4])
def test_copies_scale_the_float64_gradient(copies, monkeypatch):
    from bathymetric_gnn_amd import synthetic
    sd = synthetic.synthetic_state_dict(in_channels=7, num_layers=4, seed=61)
    d, m, u = synthetic.synthetic_tile(30, 34, 17, "V1")
    og = graph_cpu.build_graph(d, m, u, (0.5, 0.5))
    x, ei, ea, _, _ = graph_cpu.batch_graphs([og])
    xb, eib, eab, _, _ = graph_cpu.batch_graphs([og] * copies)
    w = _loss_weights(x.shape[0], 3)
    wb = {k: np.tile(v, (copies,) + (1,) * (v.ndim - 1)) for k, v in w.items()}
    g1, _ = oracle_grads(sd, x, ei, ea, torch.float64, None, w, monkeypatch)
    gb, _ = oracle_grads(sd, xb, eib, eab, torch.float64, None, wb, monkeypatch)
    assert set(g1) == set(gb)
    gmax = max(v.abs().max().item() for v in g1.values())
    bad = []
    for k in g1:
        dist = (gb[k] / copies - g1[k]).abs().max().item()
        if not dist <= REL * gmax:
            bad.append(f"{k}: {dist:.3e} (max |g| {gmax:.3e})")
    assert not bad, "\n".join(bad)
