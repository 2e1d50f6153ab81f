"""Masked-volume pretraining of the 3D encoder (SimMIM / MAE on volumes): learn from volumes that have no label.

    labels = a fresh random mask per sample; masked = x with the masked patches replaced by a constant
    tokens = encoder(masked); pred = Linear(LayerNorm(tokens)); loss = L1 / L2 (pred, patches of the ORIGINAL x) over the masked patches
    backward through the decoder and the encoder; AdamW over both

`MaskedPretrainStep(model)(x)` runs that sequence with the gfx950 kernels and no host synchronisation: nv_mim_labels (the mask is drawn
on the device), nv_mask_patches, the engine's training forward, the decoder as nv_ln_fwd + one GEMM, nv_recon_loss (csrc/pretrain.hip),
the decoder's backward, nv_vit_backward_tokens, one FusedAdamW step over the encoder's arena and the decoder's.  The encoder's forward
needs no new input form: a masked patch is a constant patch of the input volume, its patch LayerNorm output is exactly `beta`, so its
embedding is a learned constant - a mask token made of parameters the model already has.  The encoder that comes out loads into a
NeuroEncoder for fine-tuning (`encoder_state_dict`; optim.param_groups(layer_decay=) is the BEiT / MAE recipe for that).
"""
from __future__ import annotations

import math
from typing import Optional

import torch
from torch import nn

from . import _cabi, ops
from .arena import FlatArena
from .optim import FusedAdamW, LRSchedule, LossScaler, param_groups, set_group_lrs


class ReconstructionHead(FlatArena, nn.Module):
    """The decoder of SimMIM: LayerNorm(dim) + Linear(dim, patch_dim) on every token.  A flat-arena holder like temporal.TemporalHead, so
    FusedAdamW steps it with one launch and it has a 16-bit shadow for the GEMMs.  In the arena the Linear's weight has P8 = 8 ceil(P / 8)
    rows and its bias P8 elements (the GEMMs take multiples of 8): `proj.weight` / `proj.bias` - and so state_dict - are the first
    patch_dim rows / elements, the pad rows stay zero and receive zero gradients (the loss kernel zeroes their columns of dpred)."""

    def __init__(self, dim: int, patch_dim: int, eps: float = 1e-5):
        super().__init__()
        if dim < 8 or dim % 8 or patch_dim < 1:
            raise ValueError(f"ReconstructionHead: dim must be a positive multiple of 8 and patch_dim positive, got {dim}, {patch_dim}")
        self.dim, self.patch_dim, self.padded_dim = int(dim), int(patch_dim), (int(patch_dim) + 7) // 8 * 8
        self.norm = nn.LayerNorm(dim, eps=eps)
        self.proj = nn.Linear(dim, patch_dim)
        self._init_arena()
        self._shadow_key = None

    # ------------------------------------------------------------------ arena: [norm.weight d | norm.bias d | proj.weight P8 d | proj.bias P8]
    def _build_arena(self):
        d, P, P8 = self.dim, self.patch_dim, self.padded_dim
        plist = [self.norm.weight, self.norm.bias, self.proj.weight, self.proj.bias]
        self._pack(plist, [0, d, 2 * d, 2 * d + P8 * d], [d, d, P * d, P], 2 * d + P8 * d + P8)

    def _packed(self):
        self._shadow = torch.empty(self._arena.numel(), dtype=self._dtype16(), device=self._arena.device)
        self._shadow_key = None
        self._param_generation += 1

    def _dtype16(self) -> torch.dtype:
        return torch.float16 if self.operands == "fp16" else torch.bfloat16

    def set_operands(self, fmt: str):
        if fmt not in _cabi.OPERAND_FORMATS:
            raise ValueError(f"ReconstructionHead: operands must be 'bf16' or 'fp16', got {fmt!r}")
        if fmt != self.operands:
            self.operands = fmt
            if self._shadow is not None:
                self._shadow = torch.empty(self._shadow.numel(), dtype=self._dtype16(), device=self._shadow.device)
            self._shadow_key = None
        return self

    def gather_foreign_grads(self):
        """Nothing is gathered: the pretraining step writes the gradient arena itself (as for the encoder, ViT.gather_foreign_grads)."""

    def mark_shadow_fresh(self):
        """the fused AdamW wrote the arena and the shadow through raw pointers"""
        self._shadow_key = tuple(p._version for p in self._plist)
        self._param_generation += 1

    def mark_arena_rewritten(self):
        self._shadow_key = None
        self._param_generation += 1

    def _refresh_shadow(self):
        key = tuple(p._version for p in self._plist)
        if key != self._shadow_key:
            _cabi.set_operand_format(self.operands)
            ops.cast_bf16(self._arena.view(1, -1), out=self._shadow.view(1, -1))
            self._shadow_key = key

    def _views(self, flat: torch.Tensor):
        """(gamma, beta, weight [P8, d], bias [P8]) of a flat tensor with the arena's layout"""
        d, P8 = self.dim, self.padded_dim
        return flat[:d], flat[d:2 * d], flat[2 * d:2 * d + P8 * d].view(P8, d), flat[2 * d + P8 * d:]

    # ------------------------------------------------------------------ the native decoder (device tensors; the step calls these)
    def predict(self, tokens: torch.Tensor):
        """tokens fp32 [M, d] -> (pred fp32 [M, P8], what backward_into needs)"""
        self.flat_parameters()
        self._refresh_shadow()
        _cabi.set_operand_format(self.operands)
        gamma, beta, _, bias = self._views(self._arena)
        xn, st = ops.ln_fwd(tokens, gamma, beta, self.norm.eps)
        pred = ops.gemm(ops.NT, ops.EPI_BIAS_F32, xn, self._views(self._shadow)[2], bias=bias)
        return pred, (tokens, xn, st)

    def backward_into(self, dpred: torch.Tensor, saved) -> torch.Tensor:
        """dpred [M, P8] (operand format) -> dtokens fp32 [M, d]; the head's gradient arena is overwritten (weight: one TN GEMM; bias: column
        sums; LayerNorm: nv_ln_bwd's reductions)"""
        tokens, xn, st = saved
        grads = self.flat_gradients()
        dgamma, dbeta, dW, dbias = self._views(grads)
        ops.gemm(ops.TN, ops.EPI_STORE_F32, dpred, xn, out=dW)
        ops.colsum_bf16(dpred, out=dbias)
        dxn = ops.gemm(ops.NN, ops.EPI_STORE_F32, dpred, self._views(self._shadow)[2])
        dtokens = ops.ln_bwd(dxn, tokens, st, self._views(self._arena)[0], want_g16=False, dgamma=dgamma, dbeta=dbeta)[0]
        self.ensure_grad_views()
        return dtokens

    def forward(self, tokens: torch.Tensor) -> torch.Tensor:
        """[..., d] -> [..., patch_dim] (no autograd: inspection and inference; training goes through MaskedPretrainStep)"""
        flat = tokens.reshape(-1, self.dim).contiguous().float()
        with torch.no_grad():
            pred, _ = self.predict(flat)
        return pred[:, :self.patch_dim].reshape(*tokens.shape[:-1], self.patch_dim)


class _Pretrained(nn.Module):
    """the module tree FusedAdamW and param_groups see: the encoder and the decoder side by side"""

    def __init__(self, model, head):
        super().__init__()
        self.model, self.head = model, head


LOSSES = ("l1", "l2")


def check_mask_options(grid: int, mask_ratio, mask_unit, loss, norm_pix) -> None:
    """The arguments that need no device to judge (ValueError / TypeError): a ratio in (0, 1), a unit that divides the grid and leaves at
    least two units, loss 'l1' or 'l2', norm_pix a bool."""
    if isinstance(mask_ratio, bool) or not isinstance(mask_ratio, (int, float)) or not (0.0 < float(mask_ratio) < 1.0):
        raise ValueError(f"mask_ratio must be a number in (0, 1), got {mask_ratio!r}")
    if isinstance(mask_unit, bool) or not isinstance(mask_unit, int) or mask_unit < 1 or grid % mask_unit != 0 or grid // mask_unit < 2:
        raise ValueError(f"mask_unit must be a positive integer that divides the patch grid ({grid} per axis) into at least two units, got {mask_unit!r}")
    if loss not in LOSSES:
        raise ValueError(f"loss must be one of {LOSSES}, got {loss!r}")
    if not isinstance(norm_pix, bool):
        raise TypeError(f"norm_pix must be True or False, got {norm_pix!r}")


class MaskedPretrainStep:
    """MaskedPretrainStep(model)(x[B, H, W, D]) -> loss (0-dim device tensor): one masked-reconstruction step, see the module docstring.
    model: a 3D NeuroEncoder with one input channel; its dropout applies in train mode.
    mask_ratio, mask_unit: the share of masked patches and the edge (in patches) of the cubes that are masked as a whole; the masked-patch
      count m = clamp(round(ratio U), 1, U - 1) unit^3 is the same for every sample and known on the host (`masked_patches`).
    fill: the constant written into masked patches.  loss: "l1" (SimMIM) or "l2" (MAE); norm_pix: targets standardised per patch (MAE).
    lr, weight_decay, no_decay, layer_decay, lr_schedule: as TrainStep.  mlp_head takes no part in the objective: it sits in a parameter
      group with lr 0 and weight_decay 0 and stays bit-unchanged.
    loss_scale: a static factor on the loss gradient, divided out by the update (None = 1 on bf16 operands, 1024 on fp16).
    seed, rank: the mask draw is a function of (seed, rank, optimizer step, sample, unit) - a step can be replayed, ranks differ.
    After a call: `last_labels` (int32 [B, N], label < masked_patches = masked), `last_lr`."""
    STATE_VERSION = 1
    ema = None                       # (the Trainer shell asks)
    last_grad_norm = None
    last_outputs = None

    def __init__(self, model, mask_ratio: float = 0.6, mask_unit: int = 1, fill: float = 0.0, loss: str = "l1", norm_pix: bool = True,
                 lr: Optional[float] = None, weight_decay: Optional[float] = None, no_decay: bool = False, layer_decay: Optional[float] = None,
                 lr_schedule: Optional[LRSchedule] = None, loss_scale=None, seed: int = 0, rank: int = 0, process_group=None):
        from .NeuroEncoder import NeuroEncoder
        if not isinstance(model, NeuroEncoder):
            raise TypeError(f"MaskedPretrainStep: model must be a neurovit_amd.NeuroEncoder, got {type(model).__name__}")
        if model.config.get('TRAINING_DIM') != 3:
            raise NotImplementedError("MaskedPretrainStep: pretraining is for the 3D model - the 4D model adopts a (pretrained, then fine-tuned) 3D encoder")
        vit = self._vit = model.volume_encoder.vit3d
        vit.refuse_drop_path("MaskedPretrainStep")
        c = vit._cfg
        if c.channels != 1:
            raise ValueError(f"MaskedPretrainStep: the reconstruction target is a one-channel volume, the encoder has channels = {c.channels}")
        if process_group is not None:
            raise NotImplementedError("MaskedPretrainStep: data parallel is not built yet - run one process")
        if isinstance(loss_scale, (str, LossScaler)):
            raise NotImplementedError("MaskedPretrainStep: a dynamic loss scale is not built - pass a static number (a power of two)")
        S, p = c.image_size, c.image_patch_size
        if (c.image_width or S) != S or c.frames != S or (c.patch_width or p) != p or c.frame_patch_size != p:
            raise ValueError("MaskedPretrainStep: cubic volumes and patches only")
        self.grid = S // p
        check_mask_options(self.grid, mask_ratio, mask_unit, loss, norm_pix)
        for what, value in (("fill", fill), ("seed", seed), ("rank", rank)):
            if isinstance(value, bool) or not isinstance(value, (int, float) if what == "fill" else int) or (what != "fill" and value < 0):
                raise ValueError(f"MaskedPretrainStep: {what} must be a {'number' if what == 'fill' else 'non-negative integer'}, got {value!r}")
        if loss_scale is None:
            loss_scale = 1024.0 if vit.operands == "fp16" else 1.0
        if isinstance(loss_scale, bool) or not isinstance(loss_scale, (int, float)) or not (math.isfinite(loss_scale) and loss_scale > 0):
            raise ValueError(f"MaskedPretrainStep: loss_scale must be a finite number > 0, got {loss_scale!r}")
        if lr_schedule is not None and not isinstance(lr_schedule, LRSchedule):
            raise TypeError(f"MaskedPretrainStep: lr_schedule must be an optim.LRSchedule or None, got {type(lr_schedule).__name__}")
        if not all(q.requires_grad for q in vit.parameters()):
            raise ValueError("MaskedPretrainStep: every parameter of the encoder must be trainable")
        self.model = model
        self.mask_ratio, self.mask_unit, self.fill, self.loss, self.norm_pix = float(mask_ratio), int(mask_unit), float(fill), loss, norm_pix
        self.loss_scale, self.seed, self.rank = float(loss_scale), int(seed), int(rank)
        self.size, self.patch = S, p
        U = (self.grid // self.mask_unit) ** 3
        self.masked_patches = min(max(int(math.floor(self.mask_ratio * U + 0.5)), 1), U - 1) * self.mask_unit ** 3     # (nv_mim_masked_count's rule)
        self.head = ReconstructionHead(c.dim, p ** 3, eps=c.ln_eps).to(next(vit.parameters()).device).set_operands(vit.operands)
        self._tree = _Pretrained(model, self.head)
        cfg = model.config
        self._base_lr = float(cfg.get("TRAINING_LEARNING_RATE", 1e-4) if lr is None else lr)
        wd = cfg.get("TRAINING_WEIGHT_DECAY", 1e-2) if weight_decay is None else weight_decay
        self.lr_schedule = lr_schedule
        groups = param_groups(self._tree, wd, no_decay=bool(no_decay), layer_decay=layer_decay)
        idle = {id(q) for q in vit.mlp_head.parameters()}
        for g in groups:                                   # mlp_head leaves its groups ...
            keep = [i for i, q in enumerate(g["params"]) if id(q) not in idle]
            g["params"], g["names"] = [g["params"][i] for i in keep], [g["names"][i] for i in keep]
        groups = [g for g in groups if g["params"]]
        groups.append({"params": list(vit.mlp_head.parameters()), "weight_decay": 0.0, "lr_scale": 0.0,       # ... for one that never moves it
                       "names": ["model.volume_encoder.vit3d.mlp_head." + k for k, _ in vit.mlp_head.named_parameters()]})
        self.optimizer = FusedAdamW(groups, lr=self._base_lr, weight_decay=wd, model=self._tree)
        self.last_lr = lr_schedule.lr_at(1) if lr_schedule is not None else self._base_lr
        set_group_lrs(self.optimizer, self.last_lr)
        self.last_labels = None
        self._jobs = {}

    # ------------------------------------------------------------------ one step
    def _check_input(self, x):
        S = self.size
        if not torch.is_tensor(x) or x.dim() != 4 or tuple(x.shape[1:]) != (S, S, S):
            raise ValueError(f"MaskedPretrainStep: expected volumes [B, {S}, {S}, {S}], got {tuple(x.shape) if torch.is_tensor(x) else type(x).__name__}")
        if not x.is_cuda:
            raise ValueError("MaskedPretrainStep: the volumes must live on the MI355X (cuda) device - there is no CPU fallback")
        return x.contiguous().float()

    def _masked_forward(self, x, seed: int, step: int, dropout):
        """labels, the masked copy's training forward (every row of the last block), pred: (labels, pass, pred, saved)"""
        vit, B, G = self._vit, x.shape[0], self.grid
        vit.flat_parameters()
        if vit._arena.device != x.device:
            raise ValueError(f"MaskedPretrainStep: parameters on {vit._arena.device}, volumes on {x.device}")
        labels = ops.mim_labels(B, (G,) * 3, self.mask_unit, seed, step, self.rank, device=x.device)
        jobs = self._jobs.get((B, str(x.device)))
        if jobs is None:
            jobs = self._jobs[(B, str(x.device))] = torch.tensor([[b, 0, self.masked_patches] for b in range(B)], dtype=torch.int32, device=x.device)
        masked = ops.mask_patches(x, labels, jobs, self.patch, self.fill)
        video = masked.permute(0, 3, 1, 2).unsqueeze(1)                  # NeuroEncoder.py:200-202 as a view
        vit.check_video(video, arena_checked=True)
        vit._refresh_shadow()
        vit._last_logits = vit._rt.forward(video, vit._arena, vit._shadow, training=True, dropout=dropout, rows_form=1)
        rec = vit._rt.current
        n, d = vit.pos_embedding.shape[1:]
        tokens = vit._rt.tap("x2", vit._cfg.depth - 1, (B * n, d), torch.float32)
        pred, saved = self.head.predict(tokens)
        return labels, rec, pred, saved

    def __call__(self, x: torch.Tensor) -> torch.Tensor:
        x = self._check_input(x)
        vit, opt, head = self._vit, self.optimizer, self.head
        vit.refuse_drop_path("MaskedPretrainStep")        # (the rate is a plain attribute: it may have been set since the step was built)
        if head.operands != vit.operands:                  # (the model's operand format was switched after this step was built)
            head.set_operands(vit.operands)
        self.last_lr = self._base_lr if self.lr_schedule is None else self.lr_schedule.lr_at(opt.steps + 1)
        set_group_lrs(opt, self.last_lr)
        labels, rec, pred, saved = self._masked_forward(x, self.seed, opt.steps, vit.draw_dropout())
        loss, dpred, _ = ops.recon_loss(pred, x, labels, self.masked_patches, self.patch, self.loss, self.norm_pix, self.loss_scale)
        dtokens = head.backward_into(dpred, saved)
        vit._rt.backward(None, vit._arena, vit._shadow, vit.gradient_arena(), accumulate=False, of=rec, dtokens=dtokens)
        vit.ensure_grad_views()
        vit.linear_weight_grads(present=True)
        opt.step(grad_scale=1.0 / self.loss_scale)
        self.last_labels = labels
        return loss.reshape(())

    @torch.no_grad()
    def validation_loss(self, x: torch.Tensor, index: int = 0, seed: Optional[int] = None) -> torch.Tensor:
        """The reconstruction loss of `x` under the masks of a FIXED draw (seed, default this step's seed + 1, and `index` in the place of
        the optimizer step): no dropout, nothing updated - the same volumes give the same number whenever the weights are the same."""
        x = self._check_input(x)
        labels, rec, pred, _ = self._masked_forward(x, self.seed + 1 if seed is None else int(seed), int(index), (0.0, 0.0, 0))
        rec.finish()
        return ops.recon_loss(pred, x, labels, self.masked_patches, self.patch, self.loss, self.norm_pix, 1.0)[0].reshape(())

    # ------------------------------------------------------------------ state
    def encoder_state_dict(self) -> dict:
        """model.state_dict(), cloned: loads strict=True into a NeuroEncoder of the same config (mlp_head as it was before pretraining)"""
        return {k: v.detach().clone() for k, v in self.model.state_dict().items()}

    def state_dict(self) -> dict:
        """What a restarted run needs beside the encoder's parameters: the optimizer's step count (which is also the mask draw's step),
        the moment arenas of both holders, the groups, and the decoder.  Clones."""
        return {"version": self.STATE_VERSION, "operands": self._vit.operands, **self.optimizer.fused_state(),
                "head": {k: v.detach().clone() for k, v in self.head.state_dict().items()}}

    def load_state_dict(self, state: dict) -> None:
        """Restore state_dict's result into the existing buffers, in place; everything is checked before the first copy (ValueError)."""
        if not isinstance(state, dict) or state.get("version") != self.STATE_VERSION:
            raise ValueError(f"MaskedPretrainStep.load_state_dict: state version {state.get('version') if isinstance(state, dict) else None!r}, "
                             f"this class reads version {self.STATE_VERSION}")
        if state["operands"] != self._vit.operands:
            raise ValueError(f"MaskedPretrainStep.load_state_dict: the state was saved on {state['operands']} operands, this model runs on {self._vit.operands}")
        mine = self.head.state_dict()
        if set(mine) != set(state["head"]) or any(mine[k].shape != state["head"][k].shape for k in mine):
            raise ValueError("MaskedPretrainStep.load_state_dict: the decoder of the state has other keys or shapes than this one")
        self.optimizer.check_fused_state(state)
        self.optimizer.load_fused_state(state)
        self.head.load_state_dict(state["head"], strict=True)
        self.head.mark_arena_rewritten()
