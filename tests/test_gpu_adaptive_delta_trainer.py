"""``Trainer(adaptive_delta=...)`` on the GPU: the per-epoch error percentile against numpy on the very tensors the criterion saw, the
delta history against a Python replay of the policy, the delta every step trained with, the validation criterion that stays put,
resume against a straight run, the checkpoint through ``weights_only`` and ``BathymetricPipeline.load_model``, and the unchanged
behaviour without the option."""
import copy
import math

import numpy as np
import pytest
import torch

from test_gpu_backward_training import _tile
from test_gpu_trainer import _config, _model

pytestmark = pytest.mark.gpu
RES = (0.5, 0.5)
OLD_KEYS = ["train_loss", "val_loss", "train_acc", "val_acc"]


def _stores(seed=0):
    from bathymetric_gnn_amd.training import TileStore
    tr = [_tile(24, 24, 140 + i) for i in range(6)]
    va = [_tile(24, 24, 150 + i) for i in range(2)]
    return (TileStore.from_tiles([t[0] for t in tr], [t[1] for t in tr], None, [RES] * 6, seed=seed),
            TileStore.from_tiles([t[0] for t in va], [t[1] for t in va], None, [RES] * 2, seed=seed + 1))


def _record(trainer):
    """Wrap the training criterion's forward: every call leaves (epoch, delta, correction, targets, mask) on the host."""
    steps = []
    crit = trainer.criterion
    inner = crit.forward

    def forward(outputs, targets):
        steps.append((trainer.current_epoch, float(crit.correction_loss.delta), outputs["correction"].detach().reshape(-1).cpu().numpy(),
                      targets["correction_targets"].detach().reshape(-1).cpu().numpy(),
                      targets["noise_mask"].detach().reshape(-1).cpu().numpy().astype(bool)))
        return inner(outputs, targets)
    crit.forward = forward
    return steps


def _epoch_percentile(steps, epoch, p):
    errs = []
    for ep, _, c, t, m in steps:
        if ep == epoch:
            assert c.dtype == np.float32 and t.dtype == np.float32
            e = np.abs(c - t)[m]
            errs.append(e[np.isfinite(e)])
    e = np.concatenate(errs)
    return (float(np.percentile(e.astype(np.float64), p)) if e.size else None), e.size


def _replay_policy(policy_like, initial, qs):
    from bathymetric_gnn_amd.training import AdaptiveHuberDelta
    p = AdaptiveHuberDelta(ceiling=None, percentile=policy_like.percentile, momentum=policy_like.momentum,
                           min_delta=policy_like.min_delta, mode=policy_like.mode)
    p.start(initial)
    trained_with = []
    for q in qs:
        trained_with.append(p.delta)
        p.update(q)
    return trained_with, p.delta


def _check_run(trainer, steps, history, epochs):
    policy = trainer.delta_policy
    initial = float(trainer.val_criterion.correction_loss.delta)
    qs = []
    for e in range(epochs):
        q, rows = _epoch_percentile(steps, e, policy.percentile)
        assert rows > 0
        qs.append(q)
    print(f"initial delta {initial}, percentiles {history['correction_error_percentile']} (numpy {qs}), deltas {history['huber_delta']}")
    assert history["correction_error_percentile"] == qs
    want_deltas, final = _replay_policy(policy, initial, qs)
    assert history["huber_delta"] == want_deltas and history["huber_delta"][0] == initial
    for ep, delta, *_ in steps:
        assert delta == want_deltas[ep]                         # epoch e + 1 trains with what epoch e produced, from its first step on
    assert trainer.criterion.correction_loss.delta == final == policy.delta
    assert trainer.val_criterion is not trainer.criterion and trainer.val_criterion.correction_loss.delta == initial
    return qs, want_deltas


@pytest.fixture(scope="module")
def default_run(tmp_path_factory, gpu_device):
    """Three epochs under ``adaptive_delta=True`` with every step recorded: (trainer, steps, history, output directory)."""
    from bathymetric_gnn_amd.training import Trainer
    out = tmp_path_factory.mktemp("adaptive_default")
    t = Trainer(_config(epochs=3), _model("GAT"), *_stores(), output_dir=out, seed=4, adaptive_delta=True)
    steps = _record(t)
    return t, steps, copy.deepcopy(t.train()), out


def test_default_policy_history_equals_numpy_and_replay(default_run, gpu_device):
    from bathymetric_gnn_amd.training import AdaptiveHuberDelta
    trainer, steps, history, _ = default_run
    policy = trainer.delta_policy
    assert isinstance(policy, AdaptiveHuberDelta) and (policy.mode, policy.percentile, policy.momentum) == ("hybrid", 95.0, 0.9)
    assert sorted(history) == sorted(OLD_KEYS + ["huber_delta", "correction_error_percentile"])
    assert all(len(v) == 3 for v in history.values()) and len(steps) == 9
    assert trainer.error_tracker.capacity == int(np.sum(trainer.train_store.node_counts))
    _, deltas = _check_run(trainer, steps, history, 3)
    ceiling = policy.ceiling
    assert ceiling == trainer.val_criterion.correction_loss.delta and all(1.0 <= d <= ceiling for d in deltas)
    assert trainer.val_criterion.classification_loss.class_weights is trainer.criterion.classification_loss.class_weights
    for name in ("classification_weight", "correction_weight", "confidence_weight", "feature_preservation_weight", "shoal_safety_weight"):
        assert getattr(trainer.val_criterion, name) == getattr(trainer.criterion, name)


def test_checkpoint_carries_the_policy(default_run, gpu_device):
    from bathymetric_gnn_amd.config import Config
    from bathymetric_gnn_amd.models.pipeline import BathymetricPipeline
    trainer, _, history, out = default_run
    ck = torch.load(out / "final_model.pt", map_location="cpu", weights_only=True)
    assert ck["adaptive_delta"] == trainer.delta_policy.state_dict() and ck["adaptive_delta"]["updates"] == 3
    assert ck["history"]["huber_delta"] == history["huber_delta"]
    assert ck["history"]["correction_error_percentile"] == history["correction_error_percentile"]
    pipe = BathymetricPipeline(Config())
    pipe.load_model(out / "final_model.pt")
    a, b = trainer.model.state_dict(), pipe.model.state_dict()
    assert list(a) == list(b) and all(torch.equal(a[k].cpu(), b[k].cpu()) for k in a)


def _error_policy():
    from bathymetric_gnn_amd.training import AdaptiveHuberDelta
    return AdaptiveHuberDelta(mode="error", momentum=0.5, percentile=90.0, min_delta=0.25)


def test_resume_continues_the_policy(tmp_path, gpu_device):
    """Option 2 with a short memory, so that the delta moves every epoch: three epochs straight against two, a resume from
    final_model.pt in a fresh Trainer, and one more."""
    from bathymetric_gnn_amd.training import Trainer
    straight = Trainer(_config(epochs=3, scheduler="plateau"), _model("GAT"), *_stores(), output_dir=tmp_path / "a", seed=6,
                       adaptive_delta=_error_policy())
    steps = _record(straight)
    h3 = copy.deepcopy(straight.train())
    qs, deltas = _check_run(straight, steps, h3, 3)
    assert len(set(deltas)) == 3 and straight.criterion.correction_loss.delta != deltas[0]       # it moved
    first = Trainer(_config(epochs=2, scheduler="plateau"), _model("GAT"), *_stores(), output_dir=tmp_path / "b", seed=6,
                    adaptive_delta=_error_policy())
    h2 = copy.deepcopy(first.train())
    assert h2 == {k: v[:2] for k, v in h3.items()}
    second = Trainer(_config(epochs=3, scheduler="plateau"), _model("GAT", seed=99), *_stores(), output_dir=tmp_path / "c", seed=6,
                     adaptive_delta=_error_policy())
    second.resume(tmp_path / "b" / "final_model.pt")
    assert second.history == h2 and second.delta_policy.state_dict() == first.delta_policy.state_dict()
    assert second.criterion.correction_loss.delta == first.criterion.correction_loss.delta == first.delta_policy.delta
    h = second.train()
    assert h["huber_delta"] == h3["huber_delta"] and h["correction_error_percentile"] == h3["correction_error_percentile"]
    assert h == h3
    assert second.delta_policy.state_dict() == straight.delta_policy.state_dict()
    # a checkpoint without the key (a run without the option) resumes at the Option-1 delta
    plain = Trainer(_config(epochs=1), _model("GAT"), *_stores(), output_dir=tmp_path / "d", seed=6)
    plain.train()
    third = Trainer(_config(epochs=2), _model("GAT"), *_stores(), output_dir=tmp_path / "e", seed=6, adaptive_delta=_error_policy())
    start = third.criterion.correction_loss.delta
    third.resume(tmp_path / "d" / "final_model.pt")
    assert third.criterion.correction_loss.delta == start and third.history["huber_delta"] == []


def test_overflow_discards_the_epoch(tmp_path, gpu_device, caplog):
    from bathymetric_gnn_amd.training import Trainer
    t = Trainer(_config(epochs=2), _model("GAT"), *_stores(), output_dir=tmp_path, seed=4, adaptive_delta=True, max_tracked_errors=5)
    assert t.error_tracker.capacity == 5
    start = t.criterion.correction_loss.delta
    with caplog.at_level("WARNING"):
        h = t.train()
    assert h["huber_delta"] == [start, start] and all(math.isnan(v) for v in h["correction_error_percentile"])
    assert t.delta_policy.updates == 0 and any("slots full" in r.getMessage() for r in caplog.records)
    with pytest.raises(ValueError):
        Trainer(_config(), _model("GAT"), *_stores(), output_dir=tmp_path, max_tracked_errors=0)
    with pytest.raises(TypeError):
        Trainer(_config(), _model("GAT"), *_stores(), output_dir=tmp_path, adaptive_delta="hybrid")


@pytest.mark.parametrize("off", [None, False])
def test_without_the_option_nothing_changes(off, tmp_path, gpu_device):
    from bathymetric_gnn_amd.training import Trainer
    t = Trainer(_config(epochs=1), _model("GAT"), *_stores(), output_dir=tmp_path, seed=4, adaptive_delta=off)
    assert t.val_criterion is t.criterion and t.delta_policy is None and t.error_tracker is None
    h = t.train()
    assert list(h) == OLD_KEYS
    ck = torch.load(tmp_path / "final_model.pt", map_location="cpu", weights_only=True)
    assert "adaptive_delta" not in ck and list(ck["history"]) == OLD_KEYS
    if off is None:                                             # the run of a Trainer that was never given the keyword
        base = Trainer(_config(epochs=1), _model("GAT"), *_stores(), output_dir=tmp_path / "base", seed=4)
        assert base.train() == h
