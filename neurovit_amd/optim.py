"""Fused AdamW for the flat parameter arenas (Trainer.py:31,75).

`FusedAdamW(model.parameters(), lr=..., weight_decay=...)` has the constructor of torch.optim.AdamW
(defaults betas (0.9, 0.999), eps 1e-8, decoupled weight decay on every parameter).  Parameters that
are views of a ViT arena are updated by ONE nv_adamw_step launch per arena (which also refreshes the
bf16 shadow the MFMA kernels read); the 4D model's temporal head is a second, 10 k-parameter arena
(temporal.TemporalHead, fp32 only) stepped the same way; any other parameter is delegated to torch.optim.AdamW.
Parameter groups are honoured: an arena whose groups carry two or more (lr, weight_decay) pairs is stepped by ONE nv_adamw_step_grouped
launch; `param_groups` builds the fine-tuning recipe's groups (no weight decay on biases / norms / embeddings, layer-wise learning-rate
decay) and `LRSchedule` is the warm-up / cosine / linear learning rate of a step.
`ModelEma` averages the same arenas into a second model with one nv_ema_update launch each.
"""
from __future__ import annotations

import ctypes
import fnmatch
import math
import re
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


MAX_ARENA_GROUPS, MAX_ARENA_SEGMENTS = _cabi.ADAMW_MAX_GROUPS, _cabi.ADAMW_MAX_SEGMENTS


def arena_segments(offsets, numels, total: int, groups):
    """The segment table of one flat arena for nv_adamw_step_grouped, as (ends, group indices): entry i of the arena - offsets[i],
    numels[i], ascending - belongs to groups[i].  What lies between an entry and the next one (alignment padding, the constant slots
    of a ViT without output projection) joins the entry in front of it, what lies in front of the first entry joins the first;
    adjacent entries of one group are merged.  The segments cover [0, total) exactly, ends ascending strictly.  Pure Python."""
    n = len(offsets)
    if n == 0 or len(numels) != n or len(groups) != n:
        raise ValueError(f"arena_segments: {n} offsets, {len(numels)} sizes, {len(groups)} group indices - the same number (>= 1) of each is needed")
    ends, idx, at = [], [], 0
    for i in range(n):
        o, k = int(offsets[i]), int(numels[i])
        if o < at or k < 0:
            raise ValueError(f"arena_segments: entry {i} at offset {o} overlaps the one before it, which ends at {at}")
        at = o + k
        end = int(offsets[i + 1]) if i + 1 < n else int(total)
        if end < at:
            raise ValueError(f"arena_segments: entry {i} ends at {at}, beyond {'the next entry' if i + 1 < n else 'the arena'} at {end}")
        if end == (ends[-1] if ends else 0):
            continue                                   # (an empty entry with nothing behind it)
        if idx and idx[-1] == int(groups[i]):
            ends[-1] = end
        else:
            ends.append(end)
            idx.append(int(groups[i]))
    if not ends:
        raise ValueError("arena_segments: the arena is empty")
    return ends, idx


_NO_DECAY_LEAVES = ("pos_embedding", "cls_token")


def layer_id_of(name: str, depth: int) -> int:
    """Layer id of the parameter `name` (as named_parameters gives it, on a NeuroEncoder or a bare ViT) for layer-wise learning-rate
    decay: pos_embedding, cls_token and to_patch_embedding.* -> 0; transformer.layers.{l}.* -> l + 1; mlp_head.*, the 4D model's
    temporal transformer and projection head, and whatever else sits behind the encoder -> depth + 1."""
    if name.startswith(("temporal_transformer.", "projection_head.")):
        return depth + 1
    m = re.search(r"(?:^|\.)transformer\.layers\.(\d+)\.", name)
    if m:
        return int(m.group(1)) + 1
    if name.rsplit(".", 1)[-1] in _NO_DECAY_LEAVES or re.search(r"(?:^|\.)to_patch_embedding\.", name):
        return 0
    return depth + 1


def encoder_depth(model: torch.nn.Module) -> int:
    """L: the number of transformer layers of the (3D) encoder in `model`, read from its parameter names (frozen ones included)."""
    depth = 0
    for name, _ in model.named_parameters():
        if not name.startswith(("temporal_transformer.", "projection_head.")):
            m = re.search(r"(?:^|\.)transformer\.layers\.(\d+)\.", name)
            if m:
                depth = max(depth, int(m.group(1)) + 1)
    return depth


def in_no_decay_set(name: str, param, extra_no_decay=()) -> bool:
    """The no-decay rule: ndim <= 1 (biases, LayerNorm weights and biases), pos_embedding, cls_token, and names that contain or
    fnmatch one of `extra_no_decay`."""
    if param.ndim <= 1 or name.rsplit(".", 1)[-1] in _NO_DECAY_LEAVES:
        return True
    return any(pat in name or fnmatch.fnmatchcase(name, pat) for pat in extra_no_decay)


def param_groups(model: torch.nn.Module, weight_decay: float, no_decay: bool = True, layer_decay=None, extra_no_decay=()) -> list:
    """Torch-style parameter groups of the fine-tuning recipe (DeiT / BEiT / MAE; timm's param_groups_layer_decay), for FusedAdamW or
    any torch optimizer: [{"params": [...], "weight_decay": w, "lr_scale": s, "names": [...]}].
      no_decay     the no-decay set (in_no_decay_set) gets weight_decay 0.0, everything else `weight_decay`;
      layer_decay  None = off; a number in (0, 1]: a parameter of layer id i (layer_id_of) gets lr_scale = layer_decay ** (L + 1 - i),
                   formed in double, L = encoder_depth(model) - the head keeps the base learning rate, the embeddings get the smallest.
    Frozen parameters (requires_grad False) are left out; every trainable one is in exactly one group.  The groups carry no "lr": the
    optimizer's default is the base learning rate, and whoever schedules sets group["lr"] = base * group["lr_scale"] (set_group_lrs;
    TrainStep does it every step).  With both features off the result is one group."""
    if isinstance(weight_decay, bool) or not isinstance(weight_decay, (int, float)):
        raise TypeError(f"param_groups: weight_decay must be a number >= 0, got {weight_decay!r}")
    if not (math.isfinite(weight_decay) and weight_decay >= 0.0):
        raise ValueError(f"param_groups: weight_decay must be finite and >= 0, got {weight_decay!r}")
    if layer_decay is not None:
        if isinstance(layer_decay, bool) or not isinstance(layer_decay, (int, float)):
            raise TypeError(f"param_groups: layer_decay must be None or a number in (0, 1], got {layer_decay!r}")
        if not (0.0 < float(layer_decay) <= 1.0):
            raise ValueError(f"param_groups: layer_decay must be in (0, 1], got {layer_decay!r}")
    if isinstance(extra_no_decay, str):
        extra_no_decay = (extra_no_decay,)
    depth = encoder_depth(model)
    found = {}
    for name, p in model.named_parameters():
        if not p.requires_grad:
            continue
        lid = None if layer_decay is None else layer_id_of(name, depth)
        skip = bool(no_decay) and in_no_decay_set(name, p, extra_no_decay)
        g = found.get((lid, skip))
        if g is None:
            scale = 1.0 if lid is None else float(layer_decay) ** (depth + 1 - lid)
            g = found[(lid, skip)] = {"params": [], "weight_decay": 0.0 if skip else float(weight_decay), "lr_scale": scale, "names": []}
        g["params"].append(p)
        g["names"].append(name)
    return [found[k] for k in sorted(found, key=lambda k: (-1 if k[0] is None else k[0], k[1]))]


def set_group_lrs(optimizer, base_lr: float) -> None:
    """group["lr"] = base_lr * group["lr_scale"] (1.0 where a group has none) for every group of `optimizer`, in double."""
    for g in optimizer.param_groups:
        g["lr"] = float(base_lr) * float(g.get("lr_scale", 1.0))


class LRSchedule:
    """Learning rate of the k-th optimizer step, k >= 1, as a pure function in double (lr_at): linear warm-up
        k <= warmup_steps:  base_lr * k / warmup_steps                     (so the first update never runs at lr = 0)
    then, with q = (k - warmup_steps) / max(1, total_steps - warmup_steps) clamped to [0, 1],
        "cosine":    min_lr + (base_lr - min_lr) * 0.5 * (1 + cos(pi q))
        "linear":    base_lr + (min_lr - base_lr) * q
        "constant":  base_lr
    and min_lr itself, exactly, from total_steps on (q = 1).  Nothing is stored per step: a resumed run continues from its step count."""
    KINDS = ("cosine", "linear", "constant")

    def __init__(self, base_lr: float, total_steps: int, warmup_steps: int = 0, kind: str = "cosine", min_lr: float = 0.0):
        for what, value in (("base_lr", base_lr), ("min_lr", min_lr)):
            if isinstance(value, bool) or not isinstance(value, (int, float)):
                raise TypeError(f"LRSchedule: {what} must be a number, got {value!r}")
        for what, value in (("total_steps", total_steps), ("warmup_steps", warmup_steps)):
            if isinstance(value, bool) or not isinstance(value, int):
                raise TypeError(f"LRSchedule: {what} must be an integer, got {value!r}")
        if not isinstance(kind, str):
            raise TypeError(f"LRSchedule: kind must be one of {self.KINDS}, got {kind!r}")
        if kind not in self.KINDS:
            raise ValueError(f"LRSchedule: kind must be one of {self.KINDS}, got {kind!r}")
        if not (math.isfinite(base_lr) and base_lr > 0.0):
            raise ValueError(f"LRSchedule: base_lr must be finite and > 0, got {base_lr!r}")
        if not (math.isfinite(min_lr) and 0.0 <= min_lr <= base_lr):
            raise ValueError(f"LRSchedule: min_lr must be in [0, base_lr], got {min_lr!r}")
        if total_steps < 1:
            raise ValueError(f"LRSchedule: total_steps must be >= 1, got {total_steps!r}")
        if not (0 <= warmup_steps <= total_steps):
            raise ValueError(f"LRSchedule: warmup_steps must be in [0, total_steps], got {warmup_steps!r}")
        self.base_lr, self.min_lr = float(base_lr), float(min_lr)
        self.total_steps, self.warmup_steps, self.kind = total_steps, warmup_steps, kind

    def lr_at(self, k: int) -> float:
        if isinstance(k, bool) or not isinstance(k, int):
            raise TypeError(f"LRSchedule.lr_at: k must be an integer >= 1, got {k!r}")
        if k < 1:
            raise ValueError(f"LRSchedule.lr_at: k counts optimizer steps from 1, got {k!r}")
        if k <= self.warmup_steps:
            return self.base_lr * k / self.warmup_steps
        if self.kind == "constant":
            return self.base_lr
        q = min(1.0, max(0.0, (k - self.warmup_steps) / max(1, self.total_steps - self.warmup_steps)))
        if q >= 1.0:
            return self.min_lr              # (exactly: base + (min - base) * 1 rounds in double)
        if self.kind == "cosine":
            return self.min_lr + (self.base_lr - self.min_lr) * 0.5 * (1.0 + math.cos(math.pi * q))
        return self.base_lr + (self.min_lr - self.base_lr) * q


class FusedAdamW(torch.optim.Optimizer):
    """Parameter groups are honoured: at bind time every arena entry is mapped to the group that holds its parameter
    (arena_segments).  An arena whose groups all carry one (lr, weight_decay) on a given step is stepped by ONE nv_adamw_step launch,
    as without groups; one with two or more pairs by ONE nv_adamw_step_grouped launch.  lr and weight_decay are read from the groups
    on every step, so any scheduler that writes group["lr"] works.  betas and eps must agree between the groups that touch one arena."""

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, *, model: torch.nn.Module = None):
        defaults = dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay)
        super().__init__(params, defaults)
        self._arena_groups: Dict[int, dict] = {}     # id(holder) -> its groups and segment table (see _bind)
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
        if self._bound:
            return
        group_of = {}
        for gi, g in enumerate(self.param_groups):
            for p in g["params"]:
                if id(p) in group_of:
                    raise ValueError(f"FusedAdamW: a parameter of shape {tuple(p.shape)} appears in parameter groups {group_of[id(p)]} and {gi}")
                group_of[id(p)] = gi
        claimed = set()
        arenas, arena_groups = [], {}
        for holder in _flat_holders(self._model) if self._model is not None else ():
            plist = holder.arena_parameters()
            if all(id(p) in group_of and p.requires_grad for p in plist):
                # the groups that touch this arena, in group order, and the arena's segments in terms of them - all on the host
                used = sorted({group_of[id(p)] for p in plist})
                if len(used) > MAX_ARENA_GROUPS:
                    raise ValueError(f"FusedAdamW: {len(used)} parameter groups hold parameters of one {type(holder).__name__} arena, "
                                     f"the fused launch takes {MAX_ARENA_GROUPS} (lr, weight_decay) pairs")
                self._check_shared(used, type(holder).__name__)
                local = {gi: k for k, gi in enumerate(used)}
                ends, idx = arena_segments(holder._offsets, holder._numels, holder._arena.numel(), [local[group_of[id(p)]] for p in plist])
                if len(ends) > MAX_ARENA_SEGMENTS:
                    raise ValueError(f"FusedAdamW: the groups cut one {type(holder).__name__} arena into {len(ends)} segments, the fused launch takes {MAX_ARENA_SEGMENTS}")
                arenas.append(holder)
                arena_groups[id(holder)] = {"used": used, "ends": ends, "index": idx, "table": None}
                claimed.update(id(p) for p in plist)
        self._arenas, self._arena_groups = arenas, arena_groups
        # the stock optimizer of what lies outside every arena gets the same groups (lr and weight_decay follow them on every step)
        rest, self._rest_source = [], []
        for gi, g in enumerate(self.param_groups):
            ps = [p for p in g["params"] if id(p) not in claimed and p.requires_grad]
            if ps:
                rest.append({"params": ps, "lr": g["lr"], "betas": g["betas"], "eps": g["eps"], "weight_decay": g["weight_decay"]})
                self._rest_source.append(gi)
        g0 = self.param_groups[0]
        self._rest = torch.optim.AdamW(rest, lr=g0["lr"], betas=g0["betas"], eps=g0["eps"], weight_decay=g0["weight_decay"]) if rest else None
        self._bound = True

    def _check_shared(self, used, what: str) -> None:
        """betas and eps are one per launch: the groups `used` (indices), which touch one arena, must agree on them"""
        first = self.param_groups[used[0]]
        for gi in used[1:]:
            g = self.param_groups[gi]
            if tuple(g["betas"]) != tuple(first["betas"]) or g["eps"] != first["eps"]:
                raise ValueError(f"FusedAdamW: parameter groups {used[0]} and {gi} hold parameters of one {what} arena but differ in betas / eps "
                                 f"({tuple(first['betas'])}, {first['eps']} against {tuple(g['betas'])}, {g['eps']}): one launch has one of each")

    def _arena_pairs(self, holder):
        """(the groups that touch `holder`'s arena, their (lr, weight_decay) pairs as they are now)"""
        groups = [self.param_groups[gi] for gi in self._arena_groups[id(holder)]["used"]]
        return groups, [(float(g["lr"]), float(g["weight_decay"])) for g in groups]

    def is_grouped(self, holder=None) -> bool:
        """Whether `holder`'s arena (None: any arena) carries two or more distinct (lr, weight_decay) pairs right now - then its
        update is the one nv_adamw_step_grouped launch behind the backward pass, and nothing else can apply it."""
        self._bind()
        for h in self._arenas if holder is None else [holder]:
            if id(h) in self._arena_groups and len(set(self._arena_pairs(h)[1])) > 1:
                return True
        return False

    def _sync_rest(self):
        for g, gi in zip(self._rest.param_groups, self._rest_source):
            g["lr"], g["weight_decay"] = self.param_groups[gi]["lr"], self.param_groups[gi]["weight_decay"]

    def _rest_grads(self):
        """.grad of every parameter of the stock optimizer that has one"""
        for g in self._rest.param_groups if self._rest is not None else ():
            for p in g["params"]:
                if p.grad is not None:
                    yield p.grad

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
        self._bind()
        self._steps += 1
        g0 = self.param_groups[0]
        live = [h for h in self._arenas if not h.no_gradients()]
        reduced = reduced_bf16 or {}
        if clip is not None or scaler is not None:
            # the scan before the update, every gradient buffer once: summed for the clip (with a scaler that pass raises its flag too), else checked for the scaler
            for holder in live:
                holder.gather_foreign_grads()
                buf = reduced.get(id(holder))
                if clip is None:
                    scaler.check(holder.flat_gradients() if buf is None else buf.float())
                    continue
                _cabi.set_operand_format(holder.operands)      # what a 16-bit reduced buffer holds
                buf = holder.flat_gradients() if buf is None else buf
                for o, const in holder._phantom:      # arena slots that are no parameter (the nn.Identity to_out of a heads == 1 ViT):
                    buf[o:o + const.numel()].zero_()                   # what the backward pass left there is no gradient of the model
                clip.add(buf, scaler)
            for grad in self._rest_grads():
                if clip is None:
                    scaler.check(grad.contiguous().float())
                else:
                    clip.add(grad.float(), scaler)
            if scaler is not None:
                scaler.update(g0["lr"], g0["betas"])
            if clip is not None:
                clip.finish(grad_scale, scaler)
        for holder in live:
            self.step_arena(holder, grad_scale, reduced.get(id(holder)), scaler, clip)
        if self._rest is not None:
            if scaler is not None:
                if scaler.last_step_skipped():          # (stock parameters beside a scaled arena: the one place that reads the flag back)
                    return None
                for grad in self._rest_grads():
                    grad.mul_(scaler.state[1])
            if clip is not None:
                for grad in self._rest_grads():
                    grad.mul_(clip.coef)
            self._sync_rest()
            self._rest.step()
        return None

    def step_range(self, vit: FlatArena, begin: int, end: int, grad_scale: float = 1.0, max_blocks: int = 0):
        """AdamW on arena elements [begin, end) only (DP: run per gradient bucket behind its all-reduce).
        The caller advances the step counter once per optimizer step with `begin_step()`."""
        if id(vit) in self._arena_groups and self.is_grouped(vit):
            raise ValueError("FusedAdamW.step_range: this arena carries more than one (lr, weight_decay) pair - its update is one nv_adamw_step_grouped "
                             "launch over the whole arena, not a launch per gradient bucket (no overlap_optimizer with parameter groups)")
        arena, shadow = vit.flat_parameters()
        grads = vit.flat_gradients()
        m, v = self.arena_state(vit)
        g0 = self.param_groups[self._arena_groups[id(vit)]["used"][0]] if id(vit) in self._arena_groups else self.param_groups[0]
        _cabi.set_operand_format(vit.operands)
        ops.adamw_step(arena[begin:end], grads[begin:end], m[begin:end], v[begin:end], shadow[begin:end], self._steps, g0["lr"],
                       g0["betas"], g0["eps"], g0["weight_decay"], grad_scale, max_blocks)
        vit.bump_generation()                  # the arena changed under derived copies (fp8 weights re-quantise on their next use)
        self._ranged.add(id(vit))

    def begin_step(self):
        """Count one optimizer step whose launches the caller issues: step_range per bucket, step_arena, the native train step's own."""
        self._bind()
        self._steps += 1

    @property
    def steps(self) -> int:
        """optimizer steps counted so far (step and begin_step count; AdamW's t of the next one is steps + 1)"""
        return self._steps

    def arenas(self):
        """The flat arenas (ViT modules, TemporalHead objects) this optimizer steps with one fused launch each."""
        self._bind()
        return list(self._arenas)

    def arena_state(self, holder):
        """(exp_avg, exp_avg_sq) arenas of `holder` (a ViT or a TemporalHead), created on first use."""
        arena, _ = holder.flat_parameters()
        key = id(holder)
        if key not in self._state_mv or self._state_mv[key][0].data_ptr() == 0 or self._state_mv[key][0].device != arena.device:
            self._state_mv[key] = (torch.zeros_like(arena), torch.zeros_like(arena))
        return self._state_mv[key]

    # ------------------------------------------------------------------ the optimizer's part of a resumable state (TrainStep.state_dict)
    def fused_state(self) -> dict:
        """steps, group 0's hyper, clones of the moment arenas, the stock optimizer's state (rest) and, where there are any, the groups"""
        arenas = []
        for holder in self.arenas():
            m, v = self.arena_state(holder)
            arenas.append({"numel": m.numel(), "exp_avg": m.detach().clone(), "exp_avg_sq": v.detach().clone()})
        g0 = self.param_groups[0]
        state = {"steps": int(self._steps), "hyper": {k: g0[k] for k in ("lr", "betas", "eps", "weight_decay")}, "arenas": arenas,
                 "rest": None if self._rest is None else self._rest.state_dict()}
        if len(self.param_groups) > 1 or "lr_scale" in g0:      # (one default group saves what it always saved; a schedule is a function of "steps")
            state["groups"] = [{"lr": g["lr"], "lr_scale": g.get("lr_scale"), "weight_decay": g["weight_decay"]} for g in self.param_groups]
        return state

    def check_fused_state(self, state: dict) -> None:
        """ValueError naming the mismatch (arena count and sizes, group count, a stock optimizer on one side) unless the state fits"""
        holders = self.arenas()
        if len(state["arenas"]) != len(holders):
            raise ValueError(f"FusedAdamW: the state holds {len(state['arenas'])} moment arenas, this optimizer steps {len(holders)}")
        for i, (saved, holder) in enumerate(zip(state["arenas"], holders)):
            n = holder.flat_parameters()[0].numel()
            if saved["numel"] != n or saved["exp_avg"].numel() != n or saved["exp_avg_sq"].numel() != n:
                raise ValueError(f"FusedAdamW: arena {i} has {n} elements, the state's has {saved['numel']}")
        if state.get("groups") is not None and len(state["groups"]) != len(self.param_groups):
            raise ValueError(f"FusedAdamW: the state holds {len(state['groups'])} parameter groups, this optimizer has {len(self.param_groups)}")
        if (state["rest"] is None) != (self._rest is None):
            raise ValueError("FusedAdamW: parameters outside the arenas (a stock optimizer) must be on both sides or on neither")

    @torch.no_grad()
    def load_fused_state(self, state: dict) -> None:
        """Restore what fused_state returned into the existing buffers, in place (call check_fused_state first)."""
        for saved, holder in zip(state["arenas"], self.arenas()):
            m, v = self.arena_state(holder)
            m.copy_(saved["exp_avg"])
            v.copy_(saved["exp_avg_sq"])
        if self._rest is not None:
            self._rest.load_state_dict(state["rest"])
        self._steps = int(state["steps"])
        for k, value in state["hyper"].items():
            for g in self.param_groups:
                g[k] = value
        for g, saved in zip(self.param_groups, state.get("groups") or ()):      # (a state from before parameter groups has no such key)
            g["lr"], g["weight_decay"] = saved["lr"], saved["weight_decay"]
            if saved.get("lr_scale") is not None:
                g["lr_scale"] = saved["lr_scale"]

    def step_arena(self, holder, grad_scale, reduced=None, scaler=None, clip=None):
        """The one fused launch over `holder`'s arena (+ its 16-bit shadow) at the current step count, which the caller has advanced."""
        arena, shadow = holder.flat_parameters()
        grads = holder.flat_gradients()
        holder.gather_foreign_grads()
        m, v = self.arena_state(holder)
        self._bind()
        info = self._arena_groups[id(holder)]
        groups, pairs = self._arena_pairs(holder)
        if len(groups) > 1:
            self._check_shared(info["used"], type(holder).__name__)      # (a group's betas / eps may have been rewritten since _bind)
        g0 = groups[0]
        _cabi.set_operand_format(holder.operands)      # the format of the shadow this launch rewrites
        scale_state, clip_state = None if scaler is None else scaler.state, None if clip is None else clip.state
        # one pair: the launch without groups.  (Under a dynamic loss scale that launch takes its step size from the scaler's block,
        # which LossScaler.update forms from group 0's lr: an arena whose one lr is another goes through the grouped launch.)
        if len(set(pairs)) == 1 and (scaler is None or pairs[0][0] == float(self.param_groups[0]["lr"])):
            ops.adamw_step(arena, grads if reduced is None else reduced, m, v, shadow, self._steps, g0["lr"], g0["betas"], g0["eps"], g0["weight_decay"], grad_scale,
                           scale_state=scale_state, clip_state=clip_state)
        else:
            if info["table"] is None or info["table"].table.device != arena.device:
                info["table"] = ops.AdamwSegments(info["ends"], info["index"], len(groups), arena.numel(), arena.device)
            ops.adamw_step_grouped(arena, grads if reduced is None else reduced, m, v, shadow, self._steps, info["table"], [pr[0] for pr in pairs],
                                   [pr[1] for pr in pairs], g0["betas"], g0["eps"], grad_scale, scale_state=scale_state, clip_state=clip_state)
        holder.mark_shadow_fresh()

    @torch.no_grad()
    def step_rest(self, grad_scale: float = 1.0):
        """What step_range has not stepped bucket by bucket since the last call: the other arenas (the temporal head's) with
        `grad_scale`, stock parameters as they are."""
        for holder in self._arenas:
            if id(holder) not in self._ranged and not holder.no_gradients():
                self.step_arena(holder, grad_scale)
        self._ranged.clear()
        if self._rest is not None:
            self._sync_rest()
            self._rest.step()
