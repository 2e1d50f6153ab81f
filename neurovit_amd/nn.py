"""Loss module of the train step (Trainer.py:30,70): nn.CrossEntropyLoss() on the gfx950 path."""
from __future__ import annotations

import torch

from . import ops


class _CEFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logits, target):
        loss, dlogits = ops.ce_loss(logits.contiguous().float(), target.contiguous().long(), 1.0, want_grad=logits.requires_grad)
        ctx.save_for_backward(dlogits)
        return loss.reshape(())

    @staticmethod
    def backward(ctx, g):
        (dlogits,) = ctx.saved_tensors
        return dlogits * g, None


class _SoftCEFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logits, target, eps, weight, mix):
        loss, dlogits = ops.ce_loss_soft(logits.contiguous().float(), target.contiguous().long(), eps, weight, mix, 1.0, want_grad=logits.requires_grad)
        ctx.save_for_backward(dlogits)
        return loss.reshape(())

    @staticmethod
    def backward(ctx, g):
        (dlogits,) = ctx.saved_tensors
        return dlogits * g, None, None, None, None


class CrossEntropyLoss(torch.nn.Module):
    """Drop-in for nn.CrossEntropyLoss(weight=, label_smoothing=) (mean reduction, class-index targets): forward and d(loss)/d(logits)
    come from one launch - nv_ce_loss with the default arguments, nv_ce_loss_soft otherwise.  forward's optional `mix` (int32 [B, 12],
    VolumeMix.last_mix) trains against the Mixup / CutMix target lam onehot(y) + (1 - lam) onehot(y[partner]).  With a weight AND a
    mix the loss is normalised by the unsmoothed weight of the mixed target (the rule is in include/neurovit_hip.h)."""

    def __init__(self, weight=None, label_smoothing: float = 0.0):
        super().__init__()
        if isinstance(label_smoothing, bool) or not isinstance(label_smoothing, (int, float)):
            raise TypeError(f"CrossEntropyLoss: label_smoothing must be a number, got {label_smoothing!r}")
        if not (0.0 <= float(label_smoothing) < 1.0):
            raise ValueError(f"CrossEntropyLoss: label_smoothing {label_smoothing} outside [0, 1)")
        self.label_smoothing = float(label_smoothing)
        if weight is not None:
            if not torch.is_tensor(weight):
                weight = torch.tensor([float(w) for w in weight], dtype=torch.float32)
            if weight.dim() != 1 or weight.numel() == 0 or not weight.is_floating_point():
                raise ValueError(f"CrossEntropyLoss: weight must be a floating-point vector [C], got {tuple(weight.shape)} {weight.dtype}")
            weight = weight.detach().to(torch.float32).contiguous()
        self.register_buffer("weight", weight)

    def forward(self, logits, target, mix=None):
        if not logits.is_cuda:
            raise RuntimeError("neurovit_amd.nn.CrossEntropyLoss runs on MI355X only")
        if self.label_smoothing == 0.0 and self.weight is None and mix is None:
            return _CEFunction.apply(logits, target)
        weight = self.weight
        if weight is not None and weight.device != logits.device:
            weight = self.weight = weight.to(logits.device)
        return _SoftCEFunction.apply(logits, target, self.label_smoothing, weight, mix)
