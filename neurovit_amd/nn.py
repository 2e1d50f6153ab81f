"""Loss modules of the train step on the gfx950 path: nn.CrossEntropyLoss() (Trainer.py:30,70) and the regression loss."""
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


class _RegFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, pred, target, module, mix):
        B, K = pred.shape
        opts = ops.reg_opts(module.kind, module.delta, module.target_mean, module.target_std, module.weight, mix, B, K, pred.device)
        loss, dpred = ops.reg_loss(pred.contiguous().float(), target, opts, 1.0, want_grad=pred.requires_grad)
        ctx.save_for_backward(dpred)
        return loss.reshape(())

    @staticmethod
    def backward(ctx, g):
        (dpred,) = ctx.saved_tensors
        return dpred * g, None, None, None


class RegressionLoss(torch.nn.Module):
    """Regression loss on standardised targets: "mse", "l1" or "huber" (F.huber_loss's delta) of pred - (target - target_mean) / target_std,
    averaged over the OBSERVED cells - a NaN target is missing and receives no gradient - with optional per-target weights (the rule is in
    include/neurovit_hip.h; a batch with nothing observed gives loss 0).  forward and d(loss)/d(pred) come from one launch (nv_reg_loss).
    pred: float [B, K]; target: [B] (K = 1) or [B, K], any real dtype; forward's optional `mix` (int32 [B, 12], VolumeMix.last_mix) trains
    against lam t + (1 - lam) t[partner]."""

    def __init__(self, kind: str = "mse", delta: float = 1.0, target_mean=None, target_std=None, weight=None):
        super().__init__()
        ops.reg_opts(kind, delta)                     # the refusals that need no device
        self.kind, self.delta = kind, float(delta)

        def vec(t, name, lowest, strict):
            if t is None:
                return None
            t = torch.as_tensor(t, dtype=torch.float64).detach().reshape(-1)
            bad = t.numel() == 0 or not bool(torch.isfinite(t).all())
            if not bad and lowest is not None:
                bad = bool((t <= lowest).any()) if strict else bool((t < lowest).any())
            if bad:
                raise ValueError(f"RegressionLoss: {name} must be a finite vector [K]" + ("" if lowest is None else (" > 0" if strict else " >= 0")))
            return t.to(torch.float32).contiguous()
        self.register_buffer("target_mean", vec(target_mean, "target_mean", None, False))
        self.register_buffer("target_std", vec(target_std, "target_std", 0.0, True))
        self.register_buffer("weight", vec(weight, "weight", 0.0, False))

    def forward(self, pred, target, mix=None):
        if not pred.is_cuda:
            raise RuntimeError("neurovit_amd.nn.RegressionLoss runs on MI355X only")
        if pred.dim() != 2:
            raise ValueError(f"RegressionLoss: pred must be [B, K], got {tuple(pred.shape)}")
        for name in ("target_mean", "target_std", "weight"):
            t = getattr(self, name)
            if t is not None and t.device != pred.device:
                setattr(self, name, t.to(pred.device))
        target = ops.reg_targets(target, pred.shape[0], pred.shape[1]).to(pred.device)
        return _RegFunction.apply(pred, target, self, mix)
