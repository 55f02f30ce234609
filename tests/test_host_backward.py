"""The gradient blob of bgnn_backward maps back onto the parameters: BathymetricGNN.grad_slots covers the weight blob of
pack_weights (bgnn_model_weight_count floats, include/bgnn.h order) slot after slot, and names every trainable parameter exactly
once, at the offset where pack_weights put its values.  No GPU needed."""
import ctypes as C

import numpy as np
import pytest
import torch


@pytest.fixture(scope="module")
def lib():
    import os
    from bathymetric_gnn_amd import runtime
    if not os.path.exists(runtime.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return runtime.load_library()


@pytest.mark.parametrize("edge_dim", [3, None])
@pytest.mark.parametrize("predict_correction", [True, False])
@pytest.mark.parametrize("graph_edge_dim", [1, 3])
def test_grad_slots_cover_every_parameter_once(edge_dim, predict_correction, graph_edge_dim, lib):
    from bathymetric_gnn_amd.models import BathymetricGNN
    torch.manual_seed(0)
    m = BathymetricGNN(in_channels=7, hidden_channels=32, num_gnn_layers=3, heads=2, edge_dim=edge_dim,
                       predict_correction=predict_correction)
    with torch.no_grad():
        for n, b in m.named_buffers():
            if b.dtype.is_floating_point:
                b.uniform_(0.5, 1.5)
    ged = graph_edge_dim if edge_dim is None else edge_dim
    slots = m.grad_slots(ged)
    desc = m._desc(ged)
    total = lib.bgnn_model_weight_count(C.byref(desc))
    # contiguous, in order, covering the whole blob
    off = 0
    for _, o, n in slots:
        assert o == off and n > 0
        off += n
    assert off == total
    blob = m.pack_weights(ged)
    assert blob.size == total
    named = [s[0] for s in slots if s[0] is not None]
    params = dict(m.named_parameters())
    assert sorted(named) == sorted(params), set(named) ^ set(params)
    assert len(named) == len(set(named))
    # order: the parameters appear in the order of the blob, and each slot holds that parameter's values
    for name, o, n in slots:
        if name is None:
            continue
        assert n == params[name].numel()
        np.testing.assert_array_equal(blob[o:o + n], params[name].detach().numpy().ravel())
    # the unnamed slots are the BatchNorm running statistics and (edge_dim=None) the zero edge weights
    unnamed = [(o, n) for name, o, n in slots if name is None]
    n_bn = 2 * m.num_gnn_layers
    assert len(unnamed) == n_bn + (2 * m.num_gnn_layers if edge_dim is None else 0)
