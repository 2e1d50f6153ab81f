"""Fused AdamW for the flat parameter arenas (Trainer.py:31,75).

`FusedAdamW(model.parameters(), lr=..., weight_decay=...)` has the constructor of torch.optim.AdamW
(defaults betas (0.9, 0.999), eps 1e-8, decoupled weight decay on every parameter).  Parameters that
are views of a ViT arena are updated by ONE nv_adamw_step launch per arena (which also refreshes the
bf16 shadow the MFMA kernels read); the 4D model's temporal head is a second, 10 k-parameter arena
(temporal.TemporalHead, fp32 only) stepped the same way; any other parameter is delegated to torch.optim.AdamW.
`ModelEma` averages the same arenas into a second model with one nv_ema_update launch each.
"""
from __future__ import annotations

import ctypes
import math
from typing import Dict, List

import torch

from . import _cabi, ops
from .arena import FlatArena


class LossScaler:
    """torch.amp.GradScaler (src/Trainer.py:29,74-76: scaler.scale(loss).backward(); scaler.step(optimizer); scaler.update()) for
    training on fp16 operands, kept on the DEVICE: the scale, the inf / NaN flag, the growth tracker and the count of applied
    optimizer updates live in one 16-float block (csrc/optim.hip, nv_loss_scale_*), and the fused AdamW reads that block - so a
    step costs no host synchronisation, where the reference's scaler.step() reads found_inf back every step.  Same policy and
    defaults as GradScaler: the loss gradient is multiplied by `scale`; any non-finite gradient skips the update and multiplies the
    scale by backoff_factor; growth_interval clean steps in a row multiply it by growth_factor."""

    def __init__(self, device, init_scale: float = 65536.0, growth_factor: float = 2.0, backoff_factor: float = 0.5, growth_interval: int = 2000,
                 start_step: int = 0):
        self.state = torch.zeros(16, dtype=torch.float32, device=device)
        ops.loss_scale_init(self.state, init_scale, growth_factor, backoff_factor, growth_interval, start_step)

    def scale(self, loss: torch.Tensor) -> torch.Tensor:
        """loss * current scale, as a device-side product (GradScaler.scale): backward() of the result carries the scale."""
        return loss * self.state[0]

    def check(self, grads: torch.Tensor) -> None:
        ops.loss_scale_check(grads, self.state)

    def update(self, lr: float, betas) -> None:
        """Decide skip-or-step for the gradients checked since the last update, adjust the scale, prepare AdamW's constants."""
        ops.loss_scale_update(self.state, lr, betas)

    # host-side views (each synchronises: logging / tests only)
    def get_scale(self) -> float:
        return float(self.state[0])

    def steps_applied(self) -> int:
        return int(self.state[5])

    def steps_skipped(self) -> int:
        return int(self.state[11])

    def last_step_skipped(self) -> bool:
        return bool(self.state[3] != 0)


def check_max_norm(max_norm) -> float:
    """max_norm of gradient clipping: a finite number > 0 (ValueError otherwise)."""
    try:
        value = float(max_norm)
    except (TypeError, ValueError):
        raise ValueError(f"max_grad_norm must be a finite number > 0, got {max_norm!r}")
    if isinstance(max_norm, bool) or not math.isfinite(value) or value <= 0.0:
        raise ValueError(f"max_grad_norm must be a finite number > 0, got {max_norm!r}")
    return value


class GradClipper:
    """torch.nn.utils.clip_grad_norm_(parameters, max_norm) (norm_type 2) kept on the DEVICE, for the fused AdamW: the squares of every
    gradient buffer are summed in double by one streaming pass each (`add`), `finish` turns the sum into the norm of the un-scaled
    gradient and the coefficient min(max_norm / (norm + 1e-6), 1), and FusedAdamW.step(clip=...) multiplies the gradients by that
    coefficient INSIDE the update - the gradient buffers keep the raw values.  Nothing is read back: `total_norm` and `coef` are 0-dim
    fp32 views of the device block (csrc/grad_clip.hip), valid after `finish` in stream order.  With a LossScaler the summing pass also
    raises its inf / NaN flag, so no separate overflow check reads the arena."""

    def __init__(self, device, max_norm: float):
        self.max_norm = check_max_norm(max_norm)
        self.state = torch.zeros(ops.GRAD_CLIP_FLOATS, dtype=torch.float32, device=device)
        self.total_norm = self.state[ops.GC_TOTAL_NORM]
        self.coef = self.state[ops.GC_COEF]

    def add(self, tensor: torch.Tensor, scaler: "LossScaler" = None, max_blocks: int = 0) -> None:
        """Running sum of squares += sum of tensor ** 2 (fp32 or the current 16-bit operand format; any other dtype is widened to fp32)."""
        if tensor.dtype not in (torch.float32, ops.op16()):
            tensor = tensor.float()
        ops.grad_sumsq(tensor.contiguous().view(-1), self.state, None if scaler is None else scaler.state, max_blocks)

    def finish(self, grad_scale: float = 1.0, scaler: "LossScaler" = None) -> None:
        """Norm and coefficient of what was added: the summed gradients carry 1 / grad_scale (data-parallel sum, static loss scale) and,
        with `scaler`, its loss scale - call after scaler.update, which is what writes the 1 / scale of these gradients."""
        ops.grad_clip_finish(self.state, self.max_norm, grad_scale, None if scaler is None else scaler.state)


def ema_decay_at(t: int, decay: float, warmup: bool = True, update_every: int = 1) -> float:
    """Decay of the averaging that runs on update call `t` (t >= 1 counts the calls, this one included), formed in double:
    d_t = min(decay, (1 + t) / (10 + t)) with `warmup` (timm's rule), else `decay`; with update_every = k the averaging runs on calls
    k, 2k, ... and stands for k of them: d_t ** k."""
    d = min(decay, (1.0 + t) / (10.0 + t)) if warmup else decay
    return d ** update_every


def ema_weight(d: float) -> float:
    """float32(1 - d) as a Python float: the `weight` nv_ema_update gets (the subtraction in double, one rounding to fp32)."""
    return ctypes.c_float(1.0 - d).value


def _flat_holders(model: torch.nn.Module) -> list:
    """The FlatArena objects of `model`, in module order: every ViT, then the 4D model's TemporalHead (no module: hung on one)."""
    holders = [m for m in model.modules() if isinstance(m, FlatArena)]
    for m in model.modules():
        th = getattr(m, "_temporal_head", None)
        if th is not None:
            holders.append(th)
    return holders


class ModelEma:
    """Exponential moving average of a NeuroEncoder's weights (timm's ModelEmaV2 / V3), kept on the DEVICE in a second model:
    `module` is a NeuroEncoder of the same config - same state_dict keys, operand format and eval precision - in eval() with
    requires_grad_(False), starting as a copy of `model`'s parameters.  `update()` averages every flat arena (the ViT's and, for the
    4D model, the temporal head's) with ONE nv_ema_update launch each on the current stream,
        ema = ema + (model - ema) * float32(1 - d_t),     d_t = ema_decay_at(t, decay, warmup, update_every),
    each fp32 operation rounded on its own: a parameter that equals its average stays put bit for bit, so frozen parameters, the
    frozen encoder of the 4D model and the constant slots of a ViT without output projection never drift.  Parameters outside any
    arena are averaged by the same expression in torch.  Nothing is read back and nothing synchronises.  After an update the
    averaged model's 16-bit shadow, folded and fp8 weights are stale and are rebuilt on their next use (mark_arena_rewritten).
    Known limit of an fp32 average: an element stops following once |p - ema| * weight is below half an ulp of ema - at decay 0.9999
    within about 6e-4 relative (timm's fp32 EMA has the same limit)."""

    def __init__(self, model: torch.nn.Module, decay: float = 0.9999, warmup: bool = True, update_every: int = 1):
        from .NeuroEncoder import NeuroEncoder, twin_of
        self.check_args(decay, update_every)
        if not isinstance(model, NeuroEncoder):
            raise TypeError(f"ModelEma: model must be a neurovit_amd.NeuroEncoder, got {type(model).__name__}")
        device = next(model.parameters()).device
        if device.type != "cuda":
            raise ValueError(f"ModelEma: the model must live on the MI355X (cuda) device, it is on {device} - there is no CPU fallback")
        self.decay, self.warmup, self.update_every = float(decay), bool(warmup), int(update_every)
        self.num_updates = 0
        self._model = model
        self.module = twin_of(model).to(device)
        self.module.eval()
        self.module.requires_grad_(False)
        self._paired = None
        self._pairs(model)

    @staticmethod
    def check_args(decay, update_every) -> None:
        """decay: a number in [0, 1); update_every: an integer >= 1 (TypeError / ValueError otherwise)."""
        if isinstance(decay, bool) or not isinstance(decay, (int, float)):
            raise TypeError(f"ModelEma: decay must be a number in [0, 1), got {decay!r}")
        if not (0.0 <= float(decay) < 1.0):
            raise ValueError(f"ModelEma: decay must be in [0, 1), got {decay!r}")
        if isinstance(update_every, bool) or not isinstance(update_every, int):
            raise TypeError(f"ModelEma: update_every must be an integer >= 1, got {update_every!r}")
        if update_every < 1:
            raise ValueError(f"ModelEma: update_every must be >= 1, got {update_every!r}")

    def _pairs(self, model):
        """[(the average's holder, the model's holder)] per flat arena, and [(average, parameter)] of what lies outside every arena -
        found once per model; every arena size is checked before any device work."""
        got = self._paired[1] if self._paired is not None and self._paired[0] is model else None
        if got is None:
            mine, theirs = _flat_holders(self.module), _flat_holders(model)
            if len(mine) != len(theirs):
                raise ValueError(f"ModelEma.update: the model has {len(theirs)} flat arenas, the average {len(mine)}")
            inside = set()
            for a, b in zip(mine, theirs):
                na, nb = a.flat_parameters()[0].numel(), b.flat_parameters()[0].numel()
                if na != nb:
                    raise ValueError(f"ModelEma.update: arena sizes differ - the model's {type(b).__name__} arena has {nb} elements, the average's {na}")
                inside.update(id(p) for p in a.arena_parameters())
            ep, mp = list(self.module.parameters()), list(model.parameters())
            if len(ep) != len(mp) or any(e.shape != p.shape for e, p in zip(ep, mp)):
                raise ValueError("ModelEma.update: the model's parameters do not match the average's")
            rest = [(e, p) for e, p in zip(ep, mp) if id(e) not in inside]
            got = (list(zip(mine, theirs)), rest)
            self._paired = (model, got)      # (the model itself is kept: the pairs are its, and only its)
        return got

    @torch.no_grad()
    def update(self, model: torch.nn.Module = None) -> None:
        """One averaging call (see the class): counts in num_updates whether or not this call averages (update_every)."""
        arenas, rest = self._pairs(self._model if model is None else model)
        self.num_updates += 1
        if self.num_updates % self.update_every != 0:
            return
        weight = ema_weight(ema_decay_at(self.num_updates, self.decay, self.warmup, self.update_every))
        for mine, theirs in arenas:
            ops.ema_update(mine.flat_parameters()[0], theirs.flat_parameters()[0], weight)
            mine.mark_arena_rewritten()
        for e, p in rest:
            e.copy_(e + (p.detach() - e) * weight)

    def state_dict(self) -> dict:
        return {"module": self.module.state_dict(), "num_updates": self.num_updates, "decay": self.decay, "warmup": self.warmup,
                "update_every": self.update_every}

    def load_state_dict(self, state: dict) -> None:
        """Copies state["module"] into the existing arenas in place (addresses do not change) and takes over num_updates; decay, warmup
        and update_every stay those of the constructor."""
        self.module.load_state_dict(state["module"], strict=True)
        for holder in _flat_holders(self.module):
            holder.mark_arena_rewritten()
        self.num_updates = int(state["num_updates"])


class FusedAdamW(torch.optim.Optimizer):
    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, *, model: torch.nn.Module = None):
        defaults = dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay)
        super().__init__(params, defaults)
        self._model = model
        self._arenas: List[FlatArena] = []   # ViT modules and TemporalHead objects
        self._ranged = set()                 # ids of the arenas that step_range has stepped since the last step_rest
        self._state_mv: Dict[int, tuple] = {}
        self._rest = None
        self._bound = False
        self._steps = 0

    def bind(self, model: torch.nn.Module):
        """Tell the optimizer which module tree owns the parameters (needed to find the arenas)."""
        self._model = model
        self._bound = False
        return self

    def _bind(self):
        mine = {id(p) for g in self.param_groups for p in g["params"]}
        claimed = set()
        self._arenas = []
        for holder in _flat_holders(self._model) if self._model is not None else ():
            plist = holder.arena_parameters()
            if all(id(p) in mine and p.requires_grad for p in plist):
                self._arenas.append(holder)
                claimed.update(id(p) for p in plist)
        rest = [p for g in self.param_groups for p in g["params"] if id(p) not in claimed and p.requires_grad]
        g0 = self.param_groups[0]
        self._rest = torch.optim.AdamW(rest, lr=g0["lr"], betas=g0["betas"], eps=g0["eps"], weight_decay=g0["weight_decay"]) if rest else None
        self._bound = True

    @torch.no_grad()
    def step(self, closure=None, grad_scale: float = 1.0, reduced_bf16=None, scaler: "LossScaler" = None, clip: "GradClipper" = None):
        """reduced_bf16: {id(vit): flat bf16 gradient buffer} - when the data-parallel all-reduce ran on bf16 messages the
        optimizer reads the reduced gradients straight from that buffer (no cast back into the fp32 gradient arena).
        scaler: a LossScaler whose scale the gradients carry (GradScaler.step + GradScaler.update, Trainer.py:75-76): every arena's
        gradients are checked for inf / NaN, then the update is applied - un-scaled - or skipped, all on the device.
        clip: a GradClipper (scaler.unscale_(opt); clip_grad_norm_(params, max_norm); scaler.step(opt)): the squares of every arena -
        or of its reduced 16-bit buffer - and of every stock gradient are summed (with a scaler that pass is the inf / NaN check as
        well), the scaler decides, the coefficient is formed from the norm of the un-scaled gradients (sqrt(sum) * |grad_scale| / loss
        scale - every summed buffer is taken to carry the same factors) and each update multiplies its gradients by it.  The
        gradient buffers themselves keep the raw values, except stock parameters' .grad, which is multiplied in place."""
        if not self._bound:
            self._bind()
        self._steps += 1
        g0 = self.param_groups[0]
        live = [h for h in self._arenas if not h.no_gradients()]
        if clip is not None:
            for holder in live:
                holder.gather_foreign_grads()
                red = None if reduced_bf16 is None else reduced_bf16.get(id(holder))
                _cabi.set_operand_format(holder.operands)      # what a 16-bit reduced buffer holds
                summed = holder.flat_gradients() if red is None else red
                for o, const in holder._phantom:      # arena slots that are no parameter (the nn.Identity to_out of a heads == 1 ViT):
                    summed[o:o + const.numel()].zero_()                # what the backward pass left there is no gradient of the model
                clip.add(summed, scaler)
            if self._rest is not None:
                for g in self._rest.param_groups:
                    for p in g["params"]:
                        if p.grad is not None:
                            clip.add(p.grad.float(), scaler)
            if scaler is not None:
                scaler.update(g0["lr"], g0["betas"])
            clip.finish(grad_scale, scaler)
        elif scaler is not None:
            for holder in live:
                holder.gather_foreign_grads()
                red = None if reduced_bf16 is None else reduced_bf16.get(id(holder))
                scaler.check(holder.flat_gradients() if red is None else red.float())
            if self._rest is not None:
                for g in self._rest.param_groups:
                    for p in g["params"]:
                        if p.grad is not None:
                            scaler.check(p.grad.contiguous().float())
            scaler.update(g0["lr"], g0["betas"])
        for holder in live:
            self._step_arena(holder, grad_scale, None if reduced_bf16 is None else reduced_bf16.get(id(holder)), scaler, clip)
        if self._rest is not None:
            if scaler is not None:
                if scaler.last_step_skipped():          # (stock parameters beside a scaled arena: the one place that reads the flag back)
                    return None
                for g in self._rest.param_groups:
                    for p in g["params"]:
                        if p.grad is not None:
                            p.grad.mul_(scaler.state[1])
            if clip is not None:
                for g in self._rest.param_groups:
                    for p in g["params"]:
                        if p.grad is not None:
                            p.grad.mul_(clip.coef)
            for g in self._rest.param_groups:
                g["lr"] = g0["lr"]
            self._rest.step()
        return None

    def step_range(self, vit: FlatArena, begin: int, end: int, grad_scale: float = 1.0, max_blocks: int = 0):
        """AdamW on arena elements [begin, end) only (DP: run per gradient bucket behind its all-reduce).
        The caller advances the step counter once per optimizer step with `begin_step()`."""
        arena, shadow = vit.flat_parameters()
        grads = vit.flat_gradients()
        key = id(vit)
        if key not in self._state_mv:
            self._state_mv[key] = (torch.zeros_like(arena), torch.zeros_like(arena))
        m, v = self._state_mv[key]
        g0 = self.param_groups[0]
        _cabi.set_operand_format(vit.operands)
        ops.adamw_step(arena[begin:end], grads[begin:end], m[begin:end], v[begin:end], shadow[begin:end], self._steps, g0["lr"],
                       g0["betas"], g0["eps"], g0["weight_decay"], grad_scale, max_blocks)
        vit.bump_generation()                  # the arena changed under derived copies (fp8 weights re-quantise on their next use)
        self._ranged.add(id(vit))

    def begin_step(self):
        if not self._bound:
            self._bind()
        self._steps += 1

    def arenas(self):
        """The flat arenas (ViT modules, TemporalHead objects) this optimizer steps with one fused launch each."""
        if not self._bound:
            self._bind()
        return list(self._arenas)

    def arena_state(self, holder):
        """(exp_avg, exp_avg_sq) arenas of `holder` (a ViT or a TemporalHead), created on first use."""
        arena, _ = holder.flat_parameters()
        key = id(holder)
        if key not in self._state_mv or self._state_mv[key][0].data_ptr() == 0 or self._state_mv[key][0].device != arena.device:
            self._state_mv[key] = (torch.zeros_like(arena), torch.zeros_like(arena))
        return self._state_mv[key]

    def _step_arena(self, holder, grad_scale, reduced=None, scaler=None, clip=None):
        arena, shadow = holder.flat_parameters()
        grads = holder.flat_gradients()
        holder.gather_foreign_grads()
        m, v = self.arena_state(holder)
        g0 = self.param_groups[0]
        _cabi.set_operand_format(holder.operands)      # the format of the shadow this launch rewrites
        ops.adamw_step(arena, grads if reduced is None else reduced, m, v, shadow, self._steps, g0["lr"], g0["betas"], g0["eps"], g0["weight_decay"], grad_scale,
                       scale_state=None if scaler is None else scaler.state, clip_state=None if clip is None else clip.state)
        holder.mark_shadow_fresh()

    @torch.no_grad()
    def step_rest(self, grad_scale: float = 1.0):
        """What step_range has not stepped bucket by bucket since the last call: the other arenas (the temporal head's) with
        `grad_scale`, stock parameters as they are."""
        for holder in self._arenas:
            if id(holder) not in self._ranged and not holder.no_gradients():
                self._step_arena(holder, grad_scale)
        self._ranged.clear()
        if self._rest is not None:
            g0 = self.param_groups[0]
            for g in self._rest.param_groups:
                g["lr"] = g0["lr"]
            self._rest.step()
