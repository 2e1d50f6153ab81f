"""Native temporal head of the 4D model (src/models/NeuroEncoder.py:60-66, 207-230).

The reference's `TemporalTransformer` (one nn.TransformerEncoderLayer, d_model 2, nhead 2) and `ProjectionHead` (nn.Linear(2, 2))
stay what they are in the module tree - same classes, same state_dict keys, same initialisation - but their 16 parameters are
packed into one flat fp32 arena (every nn.Parameter a view of it, gradients views of a second arena) and

    per_volume [B, T, 2] -> encoder layer -> mean over time -> projection -> [B, 2]

runs as ONE launch forward and ONE backward (csrc/temporal.hip) instead of ~60 stock launches per train micro-step; the fused
AdamW steps the arena in one more.  `TemporalHead` is a plain object hung on the NeuroEncoder (not an nn.Module: it owns no state).
"""
from __future__ import annotations

import torch
from torch import nn

from . import ops
from .arena import FlatArena

MAX_TIMEPOINTS = 64      # csrc/temporal.hip: TH_MAXT
MAX_FEEDFORWARD = 2048   # TH_THREADS * TH_KPT


class _TemporalHeadFunction(torch.autograd.Function):
    """Parameters are inputs only so that autograd sees the dependency; their gradients go straight into the gradient arena
    (which `param.grad` views), like the encoder's node (vit_3d._ViTFunction)."""

    @staticmethod
    def forward(ctx, head, x, *params):
        ctx.head = head
        ctx.drop = head._draw_dropout()
        ctx.save_for_backward(x)
        return ops.temporal_head_fwd(x, head._arena, head.ff, head.eps, ctx.drop[1], ctx.drop[0])

    @staticmethod
    def backward(ctx, dout):
        (x,) = ctx.saved_tensors
        dx = ctx.head._run_backward(x, dout.contiguous().float(), ctx.drop, ctx.needs_input_grad[1])
        return (None, dx) + (None,) * len(ctx.head._plist)


class TemporalHead(FlatArena):
    _direct_when_partly_frozen = False     # a partially frozen head computes into scratch (FlatArena._backward_to_grads)

    def __init__(self, temporal_transformer: nn.Module, projection_head: nn.Module):
        self.temporal_transformer, self.projection_head = temporal_transformer, projection_head
        self._layer = temporal_transformer.transformer.layers[0]
        self._init_arena()
        lay = self._layer
        self.ff = lay.linear1.out_features
        self.eps = float(lay.norm1.eps)

    # ------------------------------------------------------------------ what the kernel implements
    def supported(self, x: torch.Tensor) -> bool:
        return x.is_cuda and x.dim() == 3 and x.shape[2] == 2 and self.supports(x.shape[1])

    def supports(self, timepoints: int) -> bool:
        """the modules are what the kernel computes, for sequences of `timepoints` elements (no tensor needed: decided before any device work)"""
        lay, mha, proj = self._layer, self._layer.self_attn, self.projection_head.projection_head
        drops = {float(lay.dropout.p), float(lay.dropout1.p), float(lay.dropout2.p), float(mha.dropout)}
        return (1 <= timepoints <= MAX_TIMEPOINTS and self.ff <= MAX_FEEDFORWARD
                and self.ff % 4 == 0 and len(self.temporal_transformer.transformer.layers) == 1
                and self.temporal_transformer.transformer.norm is None
                and mha.embed_dim == 2 and mha.num_heads == 2 and mha._qkv_same_embed_dim and mha.in_proj_bias is not None
                and mha.bias_k is None and not mha.add_zero_attn and not lay.norm_first
                and (lay.activation is torch.nn.functional.relu or isinstance(lay.activation, nn.ReLU))
                and float(lay.norm2.eps) == self.eps and len(drops) == 1
                and proj.in_features == 2 and proj.out_features == 2 and proj.bias is not None)

    # ------------------------------------------------------------------ arena (arena.FlatArena; no 16-bit shadow - the head computes in fp32)
    def _params(self):
        return [p for _, p in self.temporal_transformer.named_parameters()] + [p for _, p in self.projection_head.named_parameters()]

    def _build_arena(self):
        plist = self._params()
        F = self.ff
        sizes = [12, 6, 4, 2, 2 * F, F, 2 * F, 2, 2, 2, 2, 2, 4, 2]
        assert [p.numel() for p in plist] == sizes, "temporal head: parameter list does not match csrc/temporal.hip's arena layout"
        total = ops.temporal_head_param_count(F)
        assert total == sum(sizes)
        self._pack(plist, [sum(sizes[:i]) for i in range(len(sizes))], sizes, total)

    def _packed(self):
        self._param_generation += 1

    def _arena_ok(self) -> bool:
        """stricter than the base check: the modules' CURRENT parameters are the packed ones (a replaced nn.Parameter object is noticed)"""
        cur = self._params()
        return len(cur) == len(self._plist) and all(p is q for p, q in zip(cur, self._plist)) and super()._arena_ok()

    def mark_shadow_fresh(self):
        self._param_generation += 1

    def mark_arena_rewritten(self):
        """ViT.mark_arena_rewritten for the head: no shadow to go stale (it computes in fp32), the generation counter moves."""
        self._param_generation += 1

    # ------------------------------------------------------------------ forward / backward
    def _draw_dropout(self):
        p = float(self._layer.dropout.p)
        if not self.temporal_transformer.training or p <= 0.0:
            return (0.0, 0)
        return (p, int(torch.randint(0, 2 ** 62, (1,)).item()))        # a fresh seed per forward from torch's CPU generator

    def __call__(self, per_volume: torch.Tensor) -> torch.Tensor:
        x = per_volume.contiguous().float()
        self.flat_parameters()
        if torch.is_grad_enabled() and (x.requires_grad or any(p.requires_grad for p in self._plist)):
            return _TemporalHeadFunction.apply(self, x, *self._plist)
        p, seed = self._draw_dropout()
        return ops.temporal_head_fwd(x, self._arena, self.ff, self.eps, seed, p)

    def _run_backward(self, x, dout, drop, want_dx):
        def run(target, accumulate, scratch):
            return ops.temporal_head_bwd(x, self._arena, self.ff, dout, target, accumulate=accumulate, eps=self.eps, drop_seed=drop[1],
                                         drop_p=drop[0], want_dx=want_dx)
        return self._backward_to_grads(run)
