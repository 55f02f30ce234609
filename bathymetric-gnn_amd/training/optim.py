"""``FusedAdamW``: the last two lines of the reference's training loop (``training/trainer.py:759-761``: ``clip_grad_norm_`` and
``optimizer.step()``) as a few HIP launches over flat blobs (``bgnn_adamw_step``), with the packed model brought up to date where it
lies (``bgnn_model_refresh``) -- a training step then never repacks the weights through the host.

The interface is a torch optimizer's (it IS a ``torch.optim.Optimizer``: LR schedulers take it), the checkpoint format is
``torch.optim.AdamW``'s, so a ``state_dict`` moves between the two."""
from __future__ import annotations

import ctypes as C
import math
from typing import Optional

import torch

from .. import runtime as rt


class FusedAdamW(torch.optim.Optimizer):
    """AdamW (decoupled weight decay, per-parameter bias correction; no amsgrad, no maximize) with optional gradient clipping
    (``max_grad_norm``: ``torch.nn.utils.clip_grad_norm_`` over the parameters that have a gradient) for ONE ``BathymetricGNN``.

    On construction the model gets a flat float32 device master in ``pack_weights`` order; its parameters and BatchNorm buffers
    become views into it (``state_dict``, ``load_state_dict``, ``.to()``, assignment keep working -- whatever breaks the views
    falls back to the host repack, and the next ``step()`` flattens again).  ``step()`` gathers the gradients into blob order
    (or takes the backward's own blob when every ``.grad`` is still a view of it), runs ``bgnn_adamw_step``, refreshes the
    packed model(s) in place and bumps the parameters' version counters, so autograd refuses a stale ``backward()`` exactly as
    after a torch optimizer.  ``last_grad_norm`` is the total gradient norm of the last step (0-d device tensor)."""

    def __init__(self, model, lr: float = 1e-3, betas=(0.9, 0.999), eps: float = 1e-8, weight_decay: float = 1e-2,
                 max_grad_norm: Optional[float] = None, amsgrad: bool = False, maximize: bool = False):
        from ..models.gnn import BathymetricGNN
        if isinstance(model, (list, tuple)) and model and all(isinstance(g, dict) for g in model):
            raise ValueError("FusedAdamW takes one BathymetricGNN, not param groups: it keeps a single group over the model's blob")
        if isinstance(model, (list, tuple)) and len(model) > 1 and all(isinstance(m, BathymetricGNN) for m in model):
            raise ValueError("FusedAdamW updates the parameters of ONE model: the step runs over that model's weight blob")
        if not isinstance(model, BathymetricGNN):
            raise ValueError(f"FusedAdamW takes a BathymetricGNN (its parameters are updated in the model's blob layout), got "
                             f"{type(model).__name__}")
        if amsgrad or maximize:
            raise ValueError("FusedAdamW: amsgrad / maximize are not implemented by bgnn_adamw_step")
        if not 0.0 <= lr or not 0.0 <= eps or not 0.0 <= weight_decay or not all(0.0 <= b < 1.0 for b in betas):
            raise ValueError(f"FusedAdamW: invalid lr={lr} betas={betas} eps={eps} weight_decay={weight_decay}")
        if max_grad_norm is not None and math.isnan(float(max_grad_norm)):
            raise ValueError("FusedAdamW: max_grad_norm is NaN")
        if model.gnn_type == "GAT":
            pad_h = 1 << max(0, int(model.heads) - 1).bit_length()
        else:
            pad_h = int(model.heads)
        if model.hidden_channels not in (32, 64, 128) or pad_h != int(model.heads):
            raise ValueError(f"FusedAdamW: hidden_channels={model.hidden_channels} / heads={model.heads} run zero-padded; such a model "
                             "has no training path (hidden 32 / 64 / 128 and power-of-two head counts only)")
        ed = model._edge_width(None)
        slots = model.grad_slots(ed)
        named = dict(model.named_parameters())
        order = [(n, off, cnt) for n, off, cnt in slots if n is not None]
        if {n for n, _, _ in order} != set(named):
            raise ValueError("FusedAdamW: the model has parameters outside its weight blob: " +
                             ", ".join(sorted(set(named) - {n for n, _, _ in order})))
        # (parameters in model.parameters() order, as torch.optim.AdamW(model.parameters()) numbers them in a checkpoint)
        where = {n: (off, cnt) for n, off, cnt in order}
        order = [(n, *where[n]) for n in named]
        params = [named[n] for n, _, _ in order]
        for (n, _, _), p in zip(order, params):
            if p.dtype != torch.float32 or p.device.type != "cuda":
                raise ValueError(f"FusedAdamW: parameter {n} is {p.dtype} on {p.device}; the step runs on float32 parameters on the GPU")
            if p.device != params[0].device:
                raise ValueError(f"FusedAdamW: parameter {n} is on {p.device}, others on {params[0].device}")
        # torch.optim.AdamW's own group keys, so that a state_dict of this optimizer loads into that one and back
        defaults = dict(torch.optim.AdamW([torch.zeros(1)]).defaults)
        defaults.update(lr=float(lr), betas=(float(betas[0]), float(betas[1])), eps=float(eps), weight_decay=float(weight_decay),
                        amsgrad=False, maximize=False)
        super().__init__(params, defaults)
        self._model = model
        self._ed = ed
        self._names = [n for n, _, _ in order]
        self._slot_of = [(off, cnt) for _, off, cnt in order]
        self._steps = [0] * len(params)
        self.max_grad_norm = None if max_grad_norm is None else float(max_grad_norm)
        self._m1 = self._m2 = self._gbuf = None
        self.last_grad_norm = None
        self._ensure_flat()
        ctx = rt.get_context(params[0].device)
        model.native(ctx, ed)                    # the packed model (from the master: one download) and its gather tables

    # ---- flat state ------------------------------------------------------------------------------
    @property
    def _params(self):
        return self.param_groups[0]["params"]

    def _ensure_flat(self):
        model = self._model
        fl = model._flat_ok()
        if fl is None or fl["ed"] != self._ed:
            # (the views were broken -- .to(), load_state_dict, a parameter assigned by hand: the parameters are the model's
            #  current ones under the same names; the moments stay with their slots)
            named = dict(model.named_parameters())
            if list(named) != self._names:
                raise ValueError("FusedAdamW: the model's parameters are no longer the ones this optimizer was built over")
            for n, p in named.items():
                if p.dtype != torch.float32 or p.device.type != "cuda":
                    raise ValueError(f"FusedAdamW: parameter {n} is {p.dtype} on {p.device}; the step runs on float32 parameters on the GPU")
            self.param_groups[0]["params"][:] = [named[n] for n in self._names]
            fl = model._flatten(self._ed)
        if self._m1 is None or self._m1.device != fl["master"].device:
            old = (self._m1, self._m2)
            self._m1 = torch.zeros_like(fl["master"])
            self._m2 = torch.zeros_like(fl["master"])
            if old[0] is not None:
                self._m1.copy_(old[0]); self._m2.copy_(old[1])
            self._gbuf = None
        return fl

    def _grad_pointer(self, live, fl):
        """Device pointer of a gradient blob in the master's layout.  The backward's own blob, when every ``.grad`` is still the
        view of it that ``bgnn_backward`` handed out (one storage of the blob's size, every gradient at its slot); else the
        gradients are copied into a buffer of this optimizer."""
        n, dev = fl["n"], fl["master"].device
        g0 = live[0][1].grad
        base = g0.data_ptr() - 4 * self._slot_of[live[0][0]][0]
        st = g0.untyped_storage()
        direct = st.data_ptr() == base and st.nbytes() >= 4 * n
        for i, p in live:
            g = p.grad
            if g.dtype != torch.float32 or g.device != dev or g.is_sparse:
                raise ValueError(f"FusedAdamW: a gradient is {g.dtype} on {g.device}; dense float32 gradients on {dev} only")
            if direct and not (g.is_contiguous() and g.data_ptr() == base + 4 * self._slot_of[i][0] and
                               g.untyped_storage().data_ptr() == base):
                direct = False
        if direct:
            return C.c_void_p(base)
        if self._gbuf is None:
            self._gbuf = torch.zeros(n, dtype=torch.float32, device=dev)
        views = [self._gbuf[o:o + c].view(p.shape) for (o, c), p in ((self._slot_of[i], p) for i, p in live)]
        torch._foreach_copy_(views, [p.grad for _, p in live])
        return C.c_void_p(self._gbuf.data_ptr())

    # ---- the step --------------------------------------------------------------------------------
    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        if len(self.param_groups) != 1:
            raise ValueError("FusedAdamW keeps a single param group")
        group = self.param_groups[0]
        if group.get("amsgrad") or group.get("maximize"):
            raise ValueError("FusedAdamW: amsgrad / maximize are not implemented by bgnn_adamw_step")
        model = self._model
        fl = self._ensure_flat()
        dev = fl["master"].device
        params = self._params
        live = [(i, p) for i, p in enumerate(params) if p.grad is not None]
        norm = torch.zeros((), dtype=torch.float32, device=dev)
        ctx = rt.get_context(dev)
        if live:
            gptr = self._grad_pointer(live, fl)
            slots = (rt.AdamWSlot * len(live))()
            for k, (i, _) in enumerate(live):
                slots[k].offset, slots[k].count = self._slot_of[i]
                slots[k].step = self._steps[i] + 1
            prm = rt.AdamWParams(float(group["lr"]), float(group["betas"][0]), float(group["betas"][1]), float(group["eps"]),
                                 float(group["weight_decay"]), float(self.max_grad_norm) if self.max_grad_norm is not None else 0.0)
            ctx.begin()
            rt.check(ctx.lib.bgnn_adamw_step(ctx.handle, rt.ptr(fl["master"]), gptr, rt.ptr(self._m1), rt.ptr(self._m2), fl["n"],
                                             slots, len(live), C.byref(prm), rt.ptr(norm)))
            ctx.end()
            for i, _ in live:
                self._steps[i] += 1
            # the kernels wrote behind torch's back: autograd must see the parameters as modified in place
            for _, p in live:
                torch.autograd.graph.increment_version(p)
            model._refresh_native(rt.REFRESH_ALL)
            model._native_key = model._weights_version()
        self.last_grad_norm = norm
        return loss

    # ---- checkpoints: torch.optim.AdamW's format -------------------------------------------------------
    def _export_state(self):
        self.state.clear()
        if self._m1 is None:
            return
        for i, p in enumerate(self._params):
            if self._steps[i] == 0:
                continue                                   # (torch creates a parameter's state at its first step)
            o, c = self._slot_of[i]
            self.state[p] = {"step": torch.tensor(float(self._steps[i]), dtype=torch.float32),
                             "exp_avg": self._m1[o:o + c].view(p.shape).clone(),
                             "exp_avg_sq": self._m2[o:o + c].view(p.shape).clone()}

    def state_dict(self):
        self._export_state()
        try:
            return super().state_dict()
        finally:
            self.state.clear()

    def load_state_dict(self, state_dict):
        if len(state_dict.get("param_groups", [])) != 1:
            raise ValueError("FusedAdamW keeps a single param group")
        g = state_dict["param_groups"][0]
        if g.get("amsgrad") or g.get("maximize"):
            raise ValueError("FusedAdamW: a checkpoint with amsgrad / maximize cannot be continued by bgnn_adamw_step")
        super().load_state_dict(state_dict)
        self._ensure_flat()
        self._m1.zero_(); self._m2.zero_()
        for i, p in enumerate(self._params):
            st = self.state.get(p)
            o, c = self._slot_of[i]
            if not st:
                self._steps[i] = 0
                continue
            self._steps[i] = int(round(float(st["step"])))
            self._m1[o:o + c].copy_(st["exp_avg"].reshape(-1))
            self._m2[o:o + c].copy_(st["exp_avg_sq"].reshape(-1))
        self.state.clear()
