"""``Trainer`` -- the reference's ``training/trainer.py`` on this package's device path: tiles resident in HBM (``TileStore``,
tile_store.py), per-node targets gathered by one kernel (``bgnn_training_targets``), the step's bookkeeping added up on the device
(``EpochMetrics`` over ``bgnn_epoch_accumulate``), and the reference's epoch loop with validation, scheduler, early stopping
(``StopRule``) and checkpoints around the taped forward, ``BathymetricGNNLoss`` and ``FusedAdamW``.

What stays out: GDAL / survey file reading, torch_geometric loaders (``num_workers``, ``pin_memory``), progress bars, wandb,
multi-GPU training, and the models the backward refuses (GCN, zero-padded shapes, layers wider than 256 columns: ``Trainer``
raises at construction).

Geometric augmentation.  The reference's ``augment_rotations`` / ``augment_flips`` flags, which it never reads, are honoured by
``Trainer(augment_geometry=True)``: every training tile is gathered from the store under one of the eight symmetries of the square
(``dihedral_ops``, ``TileStore.gather`` over ``bgnn_tile_gather``, include/bgnn_augment.h) before its graph is built, all planes
alike, so features and targets are those of the turned tile.  Off by default; validation and the training statistics never turn.

Determinism.  An epoch draws from three places only: ``Trainer.step_plan(epoch)`` (the shuffle and the dropout seed of every
step), ``Trainer.augment_plan(epoch)`` (the op of every tile, when ``augment_geometry`` is on) and the noise of a synthetic store,
a function of ``(seed, epoch, tile)``.  Two runs with equal seeds give equal bits, whatever ran before, and a resumed run continues
the run it was saved from bit for bit."""
from __future__ import annotations

import dataclasses
import logging
from pathlib import Path
from types import SimpleNamespace
from typing import Any, Dict, List, Optional, Tuple

import numpy as np
import torch
from torch.optim.lr_scheduler import CosineAnnealingWarmRestarts, ReduceLROnPlateau

from .. import runtime as rt
from ..config.constants import CORRECTION_NORM_CAP, CORRECTION_NORM_FLOOR
from .huber_delta import AdaptiveHuberDelta, CorrectionErrorTracker
from .losses import BathymetricGNNLoss, compute_class_weights, compute_correction_delta
from .optim import FusedAdamW
from .tile_store import TileStore, dihedral_ops

logger = logging.getLogger(__name__)

# the reference's TrainingConfig (config/config.py:53-81): what an empty ``Config.training`` dict stands for
TRAINING_DEFAULTS: Dict[str, Any] = {
    "learning_rate": 1e-3, "weight_decay": 1e-4, "batch_size": 4, "epochs": 100, "scheduler": "cosine", "warmup_epochs": 5,
    "patience": 15, "min_delta": 1e-4, "classification_weight": 1.0, "correction_weight": 0.5, "confidence_weight": 0.2,
    "class_weights": None, "augment_rotations": True, "augment_flips": True, "augment_noise_intensity": True,
}


def training_settings(training: Any = None) -> SimpleNamespace:
    """The training settings as attributes, with the reference's defaults filled in.  ``training``: the plain dict this package's
    ``Config.training`` carries, an object with attributes (the reference's ``TrainingConfig``), a ``Config`` of either kind
    (its ``training`` member is taken), or None.  Keys the reference does not know are ignored."""
    if training is not None and not isinstance(training, dict) and hasattr(training, "training"):
        training = training.training
    out = dict(TRAINING_DEFAULTS)
    for k in TRAINING_DEFAULTS:
        if isinstance(training, dict):
            if k in training:
                out[k] = training[k]
        elif training is not None and hasattr(training, k):
            out[k] = getattr(training, k)
    return SimpleNamespace(**out)


def dropout_seed(seed: int, global_step: int) -> int:
    """The dropout seed of training step ``global_step`` (epoch * steps per epoch + step) of a run seeded ``seed``:
    ``(seed mod 2^31) * 2^32 + (global_step mod 2^32)``."""
    return ((int(seed) % (1 << 31)) << 32) | (int(global_step) % (1 << 32))


class EpochMetrics:
    """One accumulator block of ``bgnn_epoch_accumulate`` (include/bgnn_trainer.h) and its single read-back."""

    def __init__(self, device=None):
        self.device = rt.resolve_device(device)
        self._ctx = rt.get_context(self.device)
        self._acc = torch.zeros(rt.EPOCH_ACC_BYTES // 8, dtype=torch.int64, device=self.device)
        self._idle = None            # zero terms / counts for a step that has no loss statistics (an empty batch)
        self.num_classes = None

    def reset(self):
        ctx = self._ctx
        ctx.begin()
        rt.check(ctx.lib.bgnn_epoch_reset(ctx.handle, rt.ptr(self._acc)))
        ctx.end()

    def accumulate(self, graph, terms: torch.Tensor, counts: torch.Tensor, num_classes: int):
        """The raw entry point: ``terms`` float32 [6], ``counts`` int64 [C * C + 7] on the device; n comes from ``graph``."""
        if terms.dtype != torch.float32 or terms.numel() < 6 or counts.dtype != torch.int64 or \
                counts.numel() < num_classes * num_classes + len(rt.LOSS_COUNTS) or not terms.is_contiguous() or not counts.is_contiguous():
            raise ValueError("terms must be float32 [6] and counts int64 [C * C + 7], contiguous")
        ctx = self._ctx
        self.num_classes = int(num_classes)
        ctx.begin()
        rt.check(ctx.lib.bgnn_epoch_accumulate(ctx.handle, graph._handle, rt.ptr(terms), rt.ptr(counts), int(num_classes),
                                               rt.ptr(self._acc)))
        ctx.end()

    def update(self, graph, losses: Dict[str, torch.Tensor], criterion: BathymetricGNNLoss):
        """Add one step: ``losses`` as ``criterion`` returned them for ``graph``'s batch, ``criterion.last_stats`` from that call.
        No host wait."""
        stats = criterion.last_stats
        if stats is None:
            # the loss took its torch path: an empty batch (nothing to add; the kernel sees n = 0 and reads nothing)
            if graph.num_nodes != 0:
                raise rt.BgnnError("EpochMetrics.update: the loss call left no device statistics (BathymetricGNNLoss ran its torch path)")
            if self._idle is None:
                c = rt.EPOCH_MAX_CLASSES
                self._idle = (torch.zeros(6, dtype=torch.float32, device=self.device),
                              torch.zeros(c * c + len(rt.LOSS_COUNTS), dtype=torch.int64, device=self.device))
            known = self.num_classes
            self.accumulate(graph, self._idle[0], self._idle[1], known or 2)
            self.num_classes = known
            return
        conf = stats["confusion"]
        c = int(conf.shape[0])
        if stats["n_masked"].data_ptr() != conf.data_ptr() + 8 * c * c:       # not the loss pass's own block: assemble one
            counts = torch.cat([conf.reshape(-1)] + [stats[k].reshape(1) for k in rt.LOSS_COUNTS])
        else:
            counts = torch.as_strided(conf, (c * c + len(rt.LOSS_COUNTS),), (1,))
        first = losses[rt.LOSS_TERMS[0]]
        if all(losses[k].data_ptr() == first.data_ptr() + 4 * i and losses[k].dtype == torch.float32
               for i, k in enumerate(rt.LOSS_TERMS)):
            terms = torch.as_strided(first.detach(), (6,), (1,))
        else:
            terms = torch.stack([losses[k].detach().to(torch.float32) for k in rt.LOSS_TERMS])
        self.accumulate(graph, terms, counts, c)

    def result(self) -> Dict[str, Any]:
        """The epoch's single device-to-host copy: ``loss`` (sum of total * n over the nodes, 0 when empty), ``accuracy``, the
        five term means, ``confusion`` [C, C], ``nodes``, ``steps``."""
        host = self._acc.cpu().numpy()
        sums = host[:6].view(np.float64)
        nodes, correct, steps = (int(v) for v in host[6:9])
        c = self.num_classes or 0
        out = {"loss": float(sums[5]) / nodes if nodes > 0 else 0, "accuracy": correct / nodes if nodes > 0 else 0}
        for i, k in enumerate(rt.LOSS_TERMS[:5]):
            out[k] = float(sums[i]) / nodes if nodes > 0 else 0
        out["confusion"] = host[9:9 + c * c].reshape(c, c).copy()
        out["nodes"], out["steps"] = nodes, steps
        return out


class StopRule:
    """Early stopping as the reference's loop does it (trainer.py:698-706): an epoch improves when its validation loss is below
    the best so far by more than ``min_delta``; ``patience`` epochs in a row without improvement stop the run."""

    def __init__(self, patience: int, min_delta: float):
        self.patience, self.min_delta = patience, min_delta
        self.best = float("inf")
        self.counter = 0

    def update(self, val_loss: float) -> Tuple[bool, bool]:
        """``(improved, stop)``."""
        if val_loss < self.best - self.min_delta:
            self.best = val_loss
            self.counter = 0
            return True, False
        self.counter += 1
        return False, self.counter >= self.patience


class Trainer:
    """Training manager for bathymetric GNN (the reference's ``Trainer``), over ``TileStore`` s.

    ``config``: a ``Config`` of this package (``training`` a plain dict) or of the reference; the training settings are read
    through ``training_settings``.  The model is moved to the store's GPU.  A model the backward pass refuses (GCN, a
    zero-padded shape, layers wider than 256 columns) raises here, with the backward's message.

    ``batch_nodes`` (None: steps of ``batch_size`` tiles, as the reference cuts them): steps cut by cell count instead, for stores
    whose tiles differ widely in size (``TileStore.from_refinement_pairs``: refinement grids of 9 to 2500 cells); see
    ``step_plan``.  Under either rule a step whose tiles would hold fewer than two nodes is joined to a neighbouring step, which
    may then pass ``batch_nodes`` by that tile's cells; a training store whose tiles hold fewer than two nodes altogether raises
    ``ValueError`` here.

    ``augment_geometry`` (None or False: off, the tiles train as they are stored): True turns every training tile by one of the
    eight symmetries of the square per epoch, as the settings' ``augment_rotations`` / ``augment_flips`` allow (``augment_plan``;
    both flags False: every op is the identity, through the same path).

    ``adaptive_delta`` (None or False: off, the Huber delta is the one ``_compute_training_stats`` derives from the training data,
    for the whole run -- the reference's Option 1): True, or an ``AdaptiveHuberDelta`` of the caller's, moves the training
    criterion's delta between epochs (huber_delta.py; the reference's Options 2 and 3).  The policy starts at the Option-1 delta.
    Every step files ``|correction - correction_targets|`` of its noise rows into a ``CorrectionErrorTracker`` (one more launch, no
    host wait); at the end of the epoch the policy's percentile of those errors is read with the epoch's metrics, and the
    policy's new delta is what the NEXT epoch trains with.  ``history`` gains ``huber_delta`` (the delta the epoch trained with) and
    ``correction_error_percentile`` (the epoch's measured value, NaN when there was none), the checkpoint ``adaptive_delta`` (the
    policy's state; ``resume`` restores it and the criterion's delta).  While the delta moves, ``train_loss`` is not comparable
    across epochs: its correction term is measured with a different delta each epoch.  Validation therefore keeps a criterion
    of its own (``val_criterion``: the same class weights and term weights) at the fixed Option-1 delta, so that early stopping,
    ``ReduceLROnPlateau`` and ``best_model.pt`` compare like with like.  The tracker's stage holds one slot (4 bytes) per node of
    the training store, which bounds the noise rows of an epoch; ``max_tracked_errors`` lowers that.  An epoch that overflows the
    stage is reported with a warning, its percentile is discarded and the delta stays as it was."""

    def __init__(self, config, model, train_store: TileStore, val_store: Optional[TileStore] = None, output_dir=None,
                 seed: int = 0, batch_nodes: Optional[int] = None, augment_geometry: Optional[bool] = None,
                 adaptive_delta=None, max_tracked_errors: Optional[int] = None):
        if max_tracked_errors is not None and int(max_tracked_errors) < 1:
            raise ValueError(f"max_tracked_errors {max_tracked_errors}: a positive number of rows, or None")
        if batch_nodes is not None and int(batch_nodes) < 1:
            raise ValueError(f"batch_nodes {batch_nodes}: a positive number of cells, or None")
        nodes = getattr(train_store, "node_counts", None)
        if nodes is not None and int(np.sum(nodes)) < 2:
            raise ValueError(f"the training store's {len(train_store)} tiles hold {int(np.sum(nodes))} node(s) altogether: a training "
                             "step needs at least 2 (BatchNorm's batch statistics)")
        self.batch_nodes = None if batch_nodes is None else int(batch_nodes)
        self.augment_geometry = bool(augment_geometry)
        self.config = config
        self.model = model
        self.train_dataset = self.train_store = train_store
        self.val_dataset = self.val_store = val_store
        self.output_dir = Path(output_dir) if output_dir else Path("./outputs")
        self.output_dir.mkdir(parents=True, exist_ok=True)
        self.seed = int(seed)
        self.settings = training_settings(config)
        self.device = train_store.device
        self.model.to(self.device)
        self._refuse_untrainable()

        self.optimizer = FusedAdamW(model, lr=self.settings.learning_rate, weight_decay=self.settings.weight_decay,
                                    max_grad_norm=1.0)
        if self.settings.scheduler == "cosine":
            self.scheduler = CosineAnnealingWarmRestarts(self.optimizer, T_0=10, T_mult=2)
        elif self.settings.scheduler == "plateau":
            self.scheduler = ReduceLROnPlateau(self.optimizer, mode="min", factor=0.5, patience=5)
        else:
            self.scheduler = None

        class_weights, correction_delta = self._compute_training_stats()
        if class_weights is not None:
            class_weights = class_weights.to(self.device)
            logger.info(f"Class weights: {class_weights.tolist()}")
        logger.info(f"Correction Huber delta: {correction_delta:.3f}")
        self.criterion = BathymetricGNNLoss(
            class_weights=class_weights,
            classification_weight=self.settings.classification_weight,
            correction_weight=self.settings.correction_weight,
            confidence_weight=self.settings.confidence_weight,
            correction_delta=correction_delta,
        )
        self.val_criterion = self.criterion
        self.delta_policy: Optional[AdaptiveHuberDelta] = None
        self.error_tracker: Optional[CorrectionErrorTracker] = None
        if adaptive_delta is not None and adaptive_delta is not False:
            self.delta_policy = AdaptiveHuberDelta() if adaptive_delta is True else adaptive_delta
            if not isinstance(self.delta_policy, AdaptiveHuberDelta):
                raise TypeError("adaptive_delta: None, a bool or an AdaptiveHuberDelta expected")
            self.criterion.correction_loss.delta = self.delta_policy.start(correction_delta)
            self.val_criterion = BathymetricGNNLoss(
                class_weights=class_weights,
                classification_weight=self.settings.classification_weight,
                correction_weight=self.settings.correction_weight,
                confidence_weight=self.settings.confidence_weight,
                correction_delta=correction_delta,
            )
            counts = getattr(train_store, "node_counts", None)
            capacity = int(np.sum(counts)) if counts is not None else int(np.asarray(train_store.offsets)[-1])
            if max_tracked_errors is not None:
                capacity = min(capacity, int(max_tracked_errors))
            self.error_tracker = CorrectionErrorTracker(max(capacity, 1), device=self.device)
            logger.info(f"Adaptive Huber delta ({self.delta_policy.mode}): p{self.delta_policy.percentile:g} of the epoch's "
                        f"correction errors, {self.error_tracker.capacity} tracked rows")

        self.current_epoch = 0
        self.stop_rule = StopRule(self.settings.patience, self.settings.min_delta)
        self.history: Dict[str, List[float]] = {"train_loss": [], "val_loss": [], "train_acc": [], "val_acc": []}
        if self.delta_policy is not None:
            self.history["huber_delta"] = []
            self.history["correction_error_percentile"] = []
        self._next_epoch = 0
        self.train_metrics = EpochMetrics(self.device)
        self.val_metrics = EpochMetrics(self.device)
        logger.info(f"Trainer initialized, device: {self.device}")

    # (the reference keeps these two as plain members; here they live in the stop rule)
    best_val_loss = property(lambda self: self.stop_rule.best, lambda self, v: setattr(self.stop_rule, "best", v))
    patience_counter = property(lambda self: self.stop_rule.counter, lambda self, v: setattr(self.stop_rule, "counter", v))

    def _refuse_untrainable(self):
        """Ask the library whether this model has a backward pass (``bgnn_tape_bytes`` on a 4 x 4 graph)."""
        from ..data import GraphBuilder
        ctx = rt.get_context(self.device)
        gb = self.train_store.graph_builder
        probe = GraphBuilder(connectivity=gb.connectivity, include_self_loops=gb.include_self_loops, node_features=gb.node_features,
                             edge_features=gb.edge_features, device=self.device)
        g = probe.build_graphs([np.zeros((4, 4), np.float32)], None, None, [(1.0, 1.0)])
        handle = self.model.native(ctx, g.edge_dim)
        if int(ctx.lib.bgnn_tape_bytes(handle, g._handle)) == 0:
            raise NotImplementedError(ctx.lib.bgnn_last_error().decode(errors="replace"))

    # ---- statistics of the training set ----------------------------------------------------------------------------------
    def _compute_training_stats(self) -> Tuple[Optional[torch.Tensor], float]:
        """Class weights and the Huber delta from the training store (trainer.py:549-660): a synthetic store's first
        ``min(len, 50)`` samples (epoch 0) give the class counts and the normalised corrections of their noise cells; a
        ground-truth store brings its scanned class counts and ``linspace`` of ``min(len, 100)`` samples give the corrections.
        Counting and selection run on the device; the selected magnitudes come to the host once."""
        num_classes = int(self.config.model.num_classes) if hasattr(self.config, "model") else int(self.model.num_classes)
        try:
            store = self.train_store
            counts = torch.zeros(num_classes, dtype=torch.long, device=self.device)
            selected = []
            scanned = hasattr(store, "_class_counts")
            if scanned:
                counts = torch.tensor([int(store._class_counts.get(c, 0)) for c in range(num_classes)], dtype=torch.long,
                                      device=self.device)
                num_samples = min(len(store), 100)
                logger.info(f"Sampling {num_samples} tiles for correction statistics...")
                sample_indices = [int(i) for i in np.linspace(0, len(store) - 1, num_samples, dtype=int)]
            else:
                sample_indices = list(range(min(len(store), 50)))
            for piece in self._pieces(store, np.asarray(sample_indices, dtype=np.int64)):
                _, t = store.batch(piece, epoch=0)
                y, mask, target = t["class_labels"], t["noise_mask"], t["correction_targets"]
                if not scanned and y.numel() > 0:
                    ok = (y >= 0) & (y < num_classes)
                    counts += torch.bincount(y[ok], minlength=num_classes)
                norm = target[mask]
                selected.append(norm[torch.isfinite(norm)])
            counts = counts.cpu()
            class_weights = None
            if counts.sum() > 0:
                logger.info(f"Class distribution: {dict(enumerate(counts.tolist()))}")
                # (on the host, as the reference computes them: the weights are then the same bits as a host replay's)
                class_weights = compute_class_weights(torch.arange(num_classes).repeat_interleave(counts.clamp(min=1)),
                                                      num_classes=num_classes, smoothing=0.1)
            else:
                logger.warning("No valid labels found, skipping class weights")
            combined = torch.cat(selected).cpu().numpy() if selected else np.zeros(0, np.float32)
            if combined.size > 0:
                capped = np.clip(combined, -CORRECTION_NORM_CAP, CORRECTION_NORM_CAP)
                correction_delta = compute_correction_delta(capped, percentile=95.0, min_delta=1.0)
                logger.info(f"Correction stats (normalized by local_std): mean |correction|={np.mean(np.abs(combined)):.3f}, "
                            f"max |correction|={np.max(np.abs(combined)):.3f}, "
                            f"95th percentile={np.percentile(np.abs(combined), 95):.3f}")
            else:
                correction_delta = 1.0
                logger.warning("No noise corrections found, using default delta=1.0")
            return class_weights, correction_delta
        except Exception as e:
            logger.warning(f"Failed to compute training stats: {e}")
            return None, 1.0

    # ---- the plan of an epoch --------------------------------------------------------------------------------------------
    def _pieces(self, store, order: np.ndarray, trainable: bool = False) -> List[np.ndarray]:
        """``order`` cut into the tile lists of consecutive steps: ``batch_size`` tiles each, or, with ``batch_nodes``, greedily by
        the tiles' cell counts.  ``trainable``: no piece may hold fewer than two nodes (BatchNorm's batch statistics need two
        rows, and ``train()`` refuses one); such a piece is joined to the piece before it, the first one to the piece after
        it, and every other piece stays as it was cut.  Needs ``store.node_counts``; without them the cut stands."""
        limit = getattr(self, "batch_nodes", None)
        if limit is None:
            bs = max(1, int(self.settings.batch_size))
            pieces = [order[k:k + bs] for k in range(0, len(order), bs)]
        else:
            cells = np.diff(np.asarray(store.offsets, dtype=np.int64))[order].tolist()
            cuts, run = [0], 0
            for k, c in enumerate(cells):
                if k > cuts[-1] and run + c > limit:
                    cuts.append(k); run = 0
                run += c
            cuts.append(len(cells))
            pieces = [order[a:b] for a, b in zip(cuts[:-1], cuts[1:]) if b > a]
        nodes = getattr(store, "node_counts", None) if trainable else None
        if nodes is None or len(pieces) < 2:
            return pieces
        nodes = np.asarray(nodes, dtype=np.int64)
        joined: List[np.ndarray] = []
        for p in pieces:
            if joined and int(nodes[p].sum()) < 2:
                joined[-1] = np.concatenate([joined[-1], p])
            else:
                joined.append(p)
        if len(joined) > 1 and int(nodes[joined[0]].sum()) < 2:
            joined[1] = np.concatenate([joined[0], joined[1]])
            del joined[0]
        return joined

    def step_plan(self, epoch: int, validation: bool = False) -> List[Tuple[np.ndarray, Optional[int]]]:
        """``(tile indices, dropout seed)`` of every step of epoch ``epoch``.  Training: the tiles in the order
        ``np.random.default_rng([seed, epoch]).permutation(len(train_store))``, cut into pieces of ``batch_size``; the dropout
        seed of step ``k`` is ``dropout_seed(seed, epoch * steps_per_epoch + k)`` and is written to ``model.dropout_seed``
        before the step's forward.  ``validation=True``: the validation store in its own order, seed None (no dropout in
        ``eval()``).  This method, with the stores' noise (a function of (seed, epoch, tile)), is the whole source of randomness
        of an epoch.

        With ``batch_nodes`` set the same order is cut greedily by cell count instead: a piece closes before the tile that would
        take its cells (``store.offsets`` differences) above ``batch_nodes``; a tile larger than that forms a piece alone.  Seeds
        are numbered by piece, as above.

        Under either rule a training piece whose tiles hold fewer than two nodes in total (``store.node_counts``: a refinement
        grid with one valid cell, a last piece of one such tile) cannot train -- ``train()`` needs two rows for BatchNorm's batch
        statistics -- and is joined to the piece before it, or, when it is the first, to the piece after it.  A joined piece may
        therefore pass ``batch_size`` by those tiles and ``batch_nodes`` by their cells; every other piece is as the rule cut it,
        and the seeds are numbered over the pieces that remain.  Validation plans are not joined (``eval()`` takes one node), and
        neither is the plan over a store that carries no node counts."""
        store = self.val_store if validation else self.train_store
        n = len(store)
        order = np.arange(n, dtype=np.int64) if validation else \
            np.random.default_rng([self.seed, int(epoch)]).permutation(n).astype(np.int64)
        pieces = self._pieces(store, order, trainable=not validation)
        if validation:
            return [(p, None) for p in pieces]
        return [(p, dropout_seed(self.seed, int(epoch) * len(pieces) + k)) for k, p in enumerate(pieces)]

    def augment_plan(self, epoch: int) -> np.ndarray:
        """The geometric op (``dihedral_ops``, int8) of every tile of the training store in epoch ``epoch``, as the settings'
        ``augment_rotations`` / ``augment_flips`` ask, drawn from ``np.random.default_rng([seed, epoch, 0xA6])``.  With
        ``augment_geometry`` on, the training step over the tiles ``indices`` passes ``ops[indices]`` to ``TileStore.batch``: the op
        of a tile is a function of (seed, epoch, tile) and does not depend on how the epoch is cut into steps.  Validation, the
        training statistics and the construction-time probe never turn a tile."""
        s = self.settings
        return dihedral_ops(len(self.train_store), bool(s.augment_rotations), bool(s.augment_flips),
                            np.random.default_rng([self.seed, int(epoch), 0xA6]))

    # ---- epochs ------------------------------------------------------------------------------------------------------------
    def _train_epoch(self) -> Dict[str, float]:
        """Run one training epoch."""
        self.model.train()
        metrics = self.train_metrics
        metrics.reset()
        tracker = getattr(self, "error_tracker", None)
        if tracker is not None:
            tracker.reset()
        ops = self.augment_plan(self.current_epoch) if getattr(self, "augment_geometry", False) else None
        for indices, drop_seed in self.step_plan(self.current_epoch):
            graph, targets = self.train_store.batch(indices, self.current_epoch, ops=None if ops is None else ops[indices])
            self.model.dropout_seed = drop_seed
            self.optimizer.zero_grad()
            outputs = self.model(graph)
            losses = self.criterion(outputs, targets)
            if tracker is not None and outputs.get("correction") is not None and targets.get("correction_targets") is not None:
                tracker.add(outputs["correction"], targets["correction_targets"], targets.get("noise_mask"))
            losses["total"].backward()
            self.optimizer.step()
            metrics.update(graph, losses, self.criterion)
        result = metrics.result()
        if tracker is not None:
            result.update(self._adapt_delta())
        return result

    def _adapt_delta(self) -> Dict[str, float]:
        """The end of an epoch under ``adaptive_delta``: the epoch's error percentile (the tracker's single read-back) through
        the policy; the training criterion gets the new delta.  Returns the epoch's two history entries."""
        policy, tracker = self.delta_policy, self.error_tracker
        trained_with = float(self.criterion.correction_loss.delta)
        measured = tracker.percentiles([policy.percentile])
        q = measured["values"][0]
        if measured["dropped"] > 0:
            logger.warning(f"Epoch {self.current_epoch + 1}: {measured['dropped']} correction errors found the tracker's "
                           f"{tracker.capacity} slots full; the epoch's percentile is discarded and the Huber delta stays "
                           f"{trained_with:.4f}")
        self.criterion.correction_loss.delta = policy.update(q)
        if q is not None:
            logger.info(f"Epoch {self.current_epoch + 1}: p{policy.percentile:g} of |correction error| = {q:.4f} over "
                        f"{measured['count']} rows; Huber delta {trained_with:.4f} -> {self.criterion.correction_loss.delta:.4f}")
        return {"huber_delta": trained_with, "correction_error_percentile": float("nan") if q is None else float(q)}

    def _validate_epoch(self) -> Dict[str, float]:
        """Run one validation epoch."""
        self.model.eval()
        metrics = self.val_metrics
        metrics.reset()
        with torch.no_grad():
            for indices, _ in self.step_plan(self.current_epoch, validation=True):
                graph, targets = self.val_store.batch(indices, self.current_epoch)
                outputs = self.model(graph)
                criterion = getattr(self, "val_criterion", self.criterion)
                losses = criterion(outputs, targets)
                metrics.update(graph, losses, criterion)
        return metrics.result()

    def train(self) -> Dict[str, List[float]]:
        """Run the full training loop (trainer.py:662-728; after ``resume`` it continues at the epoch after the checkpoint's).
        Returns the history: ``train_loss``, ``val_loss``, ``train_acc``, ``val_acc``; under ``adaptive_delta`` also ``huber_delta``
        and ``correction_error_percentile``."""
        history = self.history
        epochs = int(self.settings.epochs)
        for epoch in range(self._next_epoch, epochs):
            self.current_epoch = epoch
            train_metrics = self._train_epoch()
            history["train_loss"].append(train_metrics["loss"])
            history["train_acc"].append(train_metrics["accuracy"])
            if "huber_delta" in train_metrics:
                history["huber_delta"].append(train_metrics["huber_delta"])
                history["correction_error_percentile"].append(train_metrics["correction_error_percentile"])
            if self.val_store is not None:
                val_metrics = self._validate_epoch()
                history["val_loss"].append(val_metrics["loss"])
                history["val_acc"].append(val_metrics["accuracy"])
                if self.scheduler is not None:
                    if isinstance(self.scheduler, ReduceLROnPlateau):
                        self.scheduler.step(val_metrics["loss"])
                    else:
                        self.scheduler.step()
                improved, stop = self.stop_rule.update(val_metrics["loss"])
                if improved:
                    self._save_checkpoint("best_model.pt")
                elif stop:
                    logger.info(f"Early stopping at epoch {epoch}")
                    break
                logger.info(f"Epoch {epoch+1}/{epochs} - Train Loss: {train_metrics['loss']:.4f}, "
                            f"Val Loss: {val_metrics['loss']:.4f}, Val Acc: {val_metrics['accuracy']:.4f}")
            else:
                logger.info(f"Epoch {epoch+1}/{epochs} - Train Loss: {train_metrics['loss']:.4f}, "
                            f"Train Acc: {train_metrics['accuracy']:.4f}")
            if (epoch + 1) % 10 == 0:
                self._save_checkpoint(f"checkpoint_epoch_{epoch+1}.pt")
        self._next_epoch = self.current_epoch + 1
        self._save_checkpoint("final_model.pt")
        return history

    # ---- checkpoints -------------------------------------------------------------------------------------------------------
    def _config_dict(self):
        cfg = self.config
        if dataclasses.is_dataclass(cfg) and not isinstance(cfg, type):
            return dataclasses.asdict(cfg)
        return dict(cfg) if isinstance(cfg, dict) else {"training": dict(vars(self.settings))}

    def _save_checkpoint(self, filename: str):
        """The reference's checkpoint (trainer.py:811-825) from plain containers and tensors only, so that
        ``torch.load(weights_only=True)`` and ``BathymetricPipeline.load_model`` read it: ``config`` is a nested dict,
        ``model_config`` holds the model's own shape, ``edge_dim`` is the model's; ``patience_counter``, ``history`` and ``seed``
        let ``resume`` continue the run."""
        m = self.model
        checkpoint = {
            "epoch": int(self.current_epoch),
            "model_state_dict": {k: v.detach().clone() for k, v in m.state_dict().items()},
            "optimizer_state_dict": self.optimizer.state_dict(),
            "best_val_loss": float(self.best_val_loss),
            "config": self._config_dict(),
            "in_channels": int(m.feature_extractor.mlp[0].in_features),
            "edge_dim": m.edge_dim,
            "correction_norm_floor": CORRECTION_NORM_FLOOR,
            "correction_norm_cap": CORRECTION_NORM_CAP,
            "model_config": {"gnn_type": m.gnn_type, "gnn_hidden_channels": int(m.hidden_channels),
                             "gnn_num_layers": int(m.num_gnn_layers), "gnn_heads": int(m.heads),
                             "gnn_dropout": float(m.gnn.dropout), "num_classes": int(m.num_classes),
                             "predict_correction": bool(m.predict_correction)},
            "patience_counter": int(self.patience_counter),
            "history": {k: [float(v) for v in vs] for k, vs in self.history.items()},
            "seed": int(self.seed),
        }
        if self.scheduler is not None:
            checkpoint["scheduler_state_dict"] = self.scheduler.state_dict()
        # the planes the training graphs carried beside the computed node features, in column order ("uncertainty",
        # "sounding_density" or a sublist): BathymetricPipeline.load_model passes exactly those
        planes = getattr(self.train_store, "node_planes", None)
        if planes is not None:
            checkpoint["node_planes"] = [str(p) for p in planes]
        if getattr(self, "delta_policy", None) is not None:
            checkpoint["adaptive_delta"] = self.delta_policy.state_dict()
        path = self.output_dir / filename
        torch.save(checkpoint, path)
        logger.info(f"Saved checkpoint: {path}")

    def resume(self, path):
        """Restore model, optimizer, scheduler, epoch, best loss, patience counter and history from a checkpoint of this
        class; the next ``train()`` continues at the following epoch.  Under ``adaptive_delta`` the policy's state and the
        training criterion's delta come back too (a checkpoint without them resumes at the Option-1 delta)."""
        ckpt = torch.load(Path(path), map_location="cpu", weights_only=True)
        self.model.load_state_dict(ckpt["model_state_dict"])
        self.model.to(self.device)
        self.optimizer.load_state_dict(ckpt["optimizer_state_dict"])
        if self.scheduler is not None and "scheduler_state_dict" in ckpt:
            self.scheduler.load_state_dict(ckpt["scheduler_state_dict"])
        self.current_epoch = int(ckpt["epoch"])
        self._next_epoch = self.current_epoch + 1
        self.best_val_loss = float(ckpt["best_val_loss"])
        self.patience_counter = int(ckpt.get("patience_counter", 0))
        hist = ckpt.get("history") or {}
        self.history = {k: [float(v) for v in hist.get(k, [])] for k in ("train_loss", "val_loss", "train_acc", "val_acc")}
        policy = getattr(self, "delta_policy", None)
        if policy is not None:
            for k in ("huber_delta", "correction_error_percentile"):
                self.history[k] = [float(v) for v in hist.get(k, [])]
            if "adaptive_delta" in ckpt:
                policy.load_state_dict(ckpt["adaptive_delta"])
                self.criterion.correction_loss.delta = policy.delta
        return ckpt
