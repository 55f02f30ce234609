"""Adaptive Huber delta: the two options the reference's ``training/losses.py::compute_correction_delta`` documents and defers
("for future implementation once diverse data is available"), with the percentile they need measured on the device.

Option 2: the delta is the percentile of ``|predicted - target|`` at the end of each epoch, smoothed by an exponential moving
average, with a floor.  Option 3: Option 2 capped by the data-derived Option-1 delta: ``effective = min(running, ceiling)``.
``AdaptiveHuberDelta`` is that policy in Python floats.  ``CorrectionErrorTracker`` owns what measures the percentile without a
host round trip in the training step (include/bgnn_quantile.h, csrc/error_quantile.hip): every step appends the masked errors of
its batch to a stage in HBM with one launch, and ``percentiles`` runs one exact radix selection over the stage and reads 104
bytes back.  ``percentile_from_ranks`` restates numpy's linear interpolation on float64 values from the two order statistics, so
the result is ``float(np.percentile(errors.astype(np.float64), p))`` bit for bit.  ``device_percentile`` is the same two kernels as
a one-shot percentile of any float32 device tensor."""
from __future__ import annotations

import ctypes as C
import math
from typing import Any, Dict, List, Optional, Sequence

import numpy as np
import torch

from .. import runtime as rt

MAX_PERCENTILES = rt.QUANTILE_MAX_FRACTIONS
MODES = ("hybrid", "error")


def percentile_from_ranks(count: int, p: float, lo: int, hi: int, v_lo: float, v_hi: float) -> Optional[float]:
    """``np.percentile(x.astype(np.float64), p)`` (method "linear") of ``count`` float32 values from the order statistics
    ``v_lo = sort(x)[lo]`` and ``v_hi = sort(x)[hi]`` at ``lo = floor((count - 1) * (p / 100))`` and ``hi = min(lo + 1, count - 1)``:
    numpy's own sequence of float64 operations (``_lerp``), in Python floats.  None for no values; ``ValueError`` when the ranks are
    not those of ``p``."""
    count = int(count)
    if count <= 0:
        return None
    vi = (count - 1) * (float(p) / 100)
    want_lo = int(math.floor(vi))
    if int(lo) != want_lo or int(hi) != min(want_lo + 1, count - 1):
        raise ValueError(f"ranks ({lo}, {hi}) are not those of the {p}th percentile of {count} values "
                         f"({want_lo}, {min(want_lo + 1, count - 1)})")
    g = vi - want_lo
    a, b = float(v_lo), float(v_hi)
    d = b - a
    r = a + d * g
    if g >= 0.5:
        r = b - d * (1 - g)
    if d == 0:
        r = a
    return r


def _check_percentiles(ps) -> List[float]:
    ps = [float(p) for p in (ps if isinstance(ps, (list, tuple, np.ndarray)) else [ps])]
    if not 1 <= len(ps) <= MAX_PERCENTILES:
        raise ValueError(f"{len(ps)} percentiles, 1 .. {MAX_PERCENTILES} expected")
    for p in ps:
        if not 0 <= p <= 100:                               # (NaN fails both comparisons)
            raise ValueError(f"percentile {p} outside [0, 100]")
    return ps


class CorrectionErrorTracker:
    """The errors of an epoch, staged on the device: ``reset()``, ``add(correction, target, mask)`` once per step (one launch, no
    host wait), ``percentiles(ps)`` at the end (one selection, one read-back).

    ``capacity``: the slots of the stage (4 bytes each), 1 .. 2^32 - 1: an upper bound of the masked rows between two resets.  Rows
    beyond it are counted in ``dropped`` and the percentiles are then None.  ``stage``: a uint32 device tensor of ``capacity``
    entries to use instead of an allocation of this object's (a view into a larger buffer, say)."""

    def __init__(self, capacity: int, device=None, stage: Optional[torch.Tensor] = None):
        capacity = int(capacity)
        if not 1 <= capacity <= rt.QUANTILE_MAX_CAPACITY:
            raise ValueError(f"capacity {capacity}: 1 .. 2^32 - 1 slots expected")
        self.capacity = capacity
        self.device = rt.resolve_device(stage.device if stage is not None and device is None else device)
        self._ctx = rt.get_context(self.device)
        if stage is None:
            stage = torch.empty(capacity, dtype=torch.int32, device=self.device)
        elif stage.is_floating_point() or stage.element_size() != 4 or stage.numel() != capacity or not stage.is_contiguous() or \
                stage.device != self.device:
            raise TypeError(f"stage must be a contiguous 32-bit integer tensor of {capacity} entries on {self.device}")
        self._stage = stage
        self._state = torch.zeros(rt.QUANTILE_STATE_BYTES // 8, dtype=torch.int64, device=self.device)
        self._out = torch.zeros(rt.QUANTILE_OUT_BYTES // 8, dtype=torch.int64, device=self.device)
        ws = int(self._ctx.lib.bgnn_quantile_workspace_bytes(capacity))
        self._ws_bytes = ws
        self._ws = torch.empty(ws // 8, dtype=torch.int64, device=self.device)

    def reset(self):
        ctx = self._ctx
        ctx.begin()
        rt.check(ctx.lib.bgnn_quantile_reset(ctx.handle, rt.ptr(self._state)))
        ctx.end()

    def _rows(self, t, what: str, n: Optional[int]) -> torch.Tensor:
        if not isinstance(t, torch.Tensor) or t.dtype != torch.float32 or t.device != self.device:
            raise TypeError(f"{what} must be a float32 tensor on {self.device}")
        t = t.detach().reshape(-1).contiguous()
        if n is not None and t.numel() != n:
            raise ValueError(f"{what} has {t.numel()} entries, correction has {n}")
        return t

    def add(self, correction: torch.Tensor, target: Optional[torch.Tensor], mask: Optional[torch.Tensor] = None):
        """File ``|correction - target|`` of the rows of ``mask`` (bool or uint8; None: every row).  float32 device tensors of one
        length, detached here.  ``target=None`` files ``correction`` itself, sign included.  No host wait."""
        c = self._rows(correction, "correction", None)
        n = c.numel()
        t = None if target is None else self._rows(target, "target", n)
        m = None
        if mask is not None:
            if not isinstance(mask, torch.Tensor) or mask.dtype not in (torch.bool, torch.uint8) or mask.device != self.device:
                raise TypeError(f"mask must be a bool or uint8 tensor on {self.device}")
            m = mask.detach().reshape(-1).contiguous()
            if m.numel() != n:
                raise ValueError(f"mask has {m.numel()} entries, correction has {n}")
            m = m.view(torch.uint8) if m.dtype == torch.bool else m
        if n == 0:
            return
        ctx = self._ctx
        ctx.begin()
        rt.check(ctx.lib.bgnn_quantile_add(ctx.handle, n, rt.ptr(c), rt.ptr(t), rt.ptr(m), rt.ptr(self._stage), self.capacity,
                                           rt.ptr(self._state)))
        ctx.end()

    def select(self, ps: Sequence[float]) -> np.void:
        """The raw result block (``runtime.QUANTILE_OUT_DTYPE``) of the percentiles ``ps``: the one device-to-host copy."""
        ps = _check_percentiles(ps)
        fr = (C.c_double * len(ps))(*[p / 100 for p in ps])
        ctx = self._ctx
        ctx.begin()
        rt.check(ctx.lib.bgnn_quantile_select(ctx.handle, rt.ptr(self._stage), self.capacity, rt.ptr(self._state), fr, len(ps),
                                              rt.ptr(self._ws), self._ws_bytes, rt.ptr(self._out)))
        ctx.end()
        return np.frombuffer(self._out.cpu().numpy().tobytes(), dtype=rt.QUANTILE_OUT_DTYPE)[0]

    def percentiles(self, ps) -> Dict[str, Any]:
        """``{"count", "nonfinite", "dropped", "values"}`` over everything added since the last ``reset``: ``count`` values were
        filed, ``nonfinite`` masked rows were NaN or infinite and left out, ``dropped`` found the stage full.  ``values[k]`` is
        ``float(np.percentile(errors.astype(np.float64), ps[k]))`` of the filed errors; every value is None when nothing was filed
        or anything was dropped."""
        ps = _check_percentiles(ps)
        block = self.select(ps)
        count, nonfinite, dropped = int(block["count"]), int(block["nonfinite"]), int(block["dropped"])
        values: List[Optional[float]] = [None] * len(ps)
        if count > 0 and dropped == 0:
            for k, p in enumerate(ps):
                r = block["ranks"][k]
                values[k] = percentile_from_ranks(count, p, int(r["lo"]), int(r["hi"]), float(r["v_lo"]), float(r["v_hi"]))
        return {"count": count, "nonfinite": nonfinite, "dropped": dropped, "values": values}

    def state(self) -> np.void:
        """The state block on the host (``runtime.QUANTILE_STATE_DTYPE``): counters and the top-digit histogram.  A host wait."""
        return np.frombuffer(self._state.cpu().numpy().tobytes(), dtype=rt.QUANTILE_STATE_DTYPE)[0]


def device_percentile(values: torch.Tensor, p, absolute: bool = False) -> Dict[str, Any]:
    """A one-shot percentile of a float32 device tensor (any shape) through ``CorrectionErrorTracker``'s kernels: ``p`` one value or
    up to three in [0, 100]; ``absolute``: of ``|values|``.  Non-finite entries are left out and reported.  Returns the tracker's
    ``{"count", "nonfinite", "dropped", "values"}`` with one value per ``p``, each equal to ``np.percentile`` of the finite entries
    cast to float64 (None when there is none)."""
    if not isinstance(values, torch.Tensor) or not values.is_cuda or values.dtype != torch.float32:
        raise TypeError("values must be a float32 device tensor")
    ps = _check_percentiles(p)
    flat = values.detach().reshape(-1)
    if flat.numel() == 0:
        return {"count": 0, "nonfinite": 0, "dropped": 0, "values": [None] * len(ps)}
    tracker = CorrectionErrorTracker(flat.numel(), device=flat.device)
    tracker.add(flat.abs() if absolute else flat, None)
    return tracker.percentiles(ps)


class AdaptiveHuberDelta:
    """The policy of the adaptive delta, in Python floats.

    ``start(initial_delta)`` sets the running value to the Option-1 delta (and the ceiling, when none was given); ``update(q)``
    takes an epoch's measured error percentile: ``running = momentum * running + (1 - momentum) * q`` and the effective delta is
    ``max(min_delta, min(running, ceiling))`` in mode ``"hybrid"`` (Option 3) or ``max(min_delta, running)`` in mode ``"error"``
    (Option 2).  ``update(None)`` -- an epoch without noise rows, a stage that overflowed -- changes nothing.  ``delta`` is the
    effective delta.  ``state_dict()`` holds floats, ints and strings only."""

    def __init__(self, ceiling: Optional[float] = None, percentile: float = 95.0, momentum: float = 0.9, min_delta: float = 1.0,
                 mode: str = "hybrid"):
        momentum, percentile, min_delta = float(momentum), float(percentile), float(min_delta)
        if not 0 <= momentum < 1:
            raise ValueError(f"momentum {momentum} outside [0, 1)")
        if not 0 <= percentile <= 100:
            raise ValueError(f"percentile {percentile} outside [0, 100]")
        if not min_delta > 0:
            raise ValueError(f"min_delta {min_delta}: a positive value expected")
        if mode not in MODES:
            raise ValueError(f"mode {mode!r}: one of {MODES} expected")
        if ceiling is not None and not float(ceiling) >= min_delta:
            raise ValueError(f"ceiling {ceiling} below min_delta {min_delta}")
        self.ceiling = None if ceiling is None else float(ceiling)
        self.percentile, self.momentum, self.min_delta, self.mode = percentile, momentum, min_delta, mode
        self.running: Optional[float] = None
        self.updates = 0

    def start(self, initial_delta: float) -> float:
        initial_delta = float(initial_delta)
        if not math.isfinite(initial_delta):
            raise ValueError(f"initial delta {initial_delta}")
        self.running = initial_delta
        if self.ceiling is None:
            self.ceiling = initial_delta
        self.updates = 0
        return self.delta

    @property
    def delta(self) -> float:
        if self.running is None:
            raise RuntimeError("AdaptiveHuberDelta: start() has not been called")
        r = min(self.running, self.ceiling) if self.mode == "hybrid" else self.running
        return max(self.min_delta, r)

    def update(self, q: Optional[float]) -> float:
        if self.running is None:
            raise RuntimeError("AdaptiveHuberDelta: start() has not been called")
        if q is not None:
            q = float(q)
            if not math.isfinite(q):
                raise ValueError(f"error percentile {q}: a finite value or None expected")
            self.running = self.momentum * self.running + (1 - self.momentum) * q
            self.updates += 1
        return self.delta

    def state_dict(self) -> Dict[str, Any]:
        return {"mode": self.mode, "percentile": self.percentile, "momentum": self.momentum, "min_delta": self.min_delta,
                "ceiling": self.ceiling, "running": self.running, "updates": int(self.updates)}

    def load_state_dict(self, state: Dict[str, Any]):
        mode = str(state["mode"])
        if mode not in MODES:
            raise ValueError(f"mode {mode!r}: one of {MODES} expected")
        self.mode = mode
        self.percentile, self.momentum, self.min_delta = float(state["percentile"]), float(state["momentum"]), float(state["min_delta"])
        self.ceiling = None if state.get("ceiling") is None else float(state["ceiling"])
        self.running = None if state.get("running") is None else float(state["running"])
        self.updates = int(state.get("updates", 0))
