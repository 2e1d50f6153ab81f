"""Drop-in for the reference's src/models/vit_3d.py on MI355X.

Same classes, constructor signatures, attribute paths and state_dict keys as the reference
(vit_3d.py:14-126): FeedForward, Attention, Transformer, ViT.  The module tree is built from the same
torch building blocks in the same order, so `torch.manual_seed(s)` yields bit-identical initial
weights to the reference; the compute, however, never goes through those blocks:

  ViT.forward runs the whole encoder through the native gfx950 engine (csrc/engine.hip) in ONE
  C-ABI call, and its backward in one more.  Parameters are views into a flat fp32 arena with a
  bf16 shadow (see engine.py), gradients are written straight into a flat gradient arena that
  `param.grad` views.

There is no CPU / eager fallback: a CPU input raises.
"""
from __future__ import annotations

from typing import List, Optional

import torch
from torch import nn

from . import _cabi, engine, ops
from .arena import FlatArena


def pair(t):
    return t if isinstance(t, tuple) else (t, t)


def check_target(target, B: int, C: int) -> None:
    """ValueError for a `target` that cannot name one class per volume: an int outside [0, C), or a tensor that does not hold B classes"""
    if torch.is_tensor(target):
        if target.numel() != B:
            raise ValueError(f"neurovit_amd.ViT: target must hold one class per volume ({B}), got {tuple(target.shape)}")
    elif target is not None and not 0 <= int(target) < C:
        raise ValueError(f"neurovit_amd.ViT: target class {target} outside [0, {C})")


def target_classes(target, logits: torch.Tensor) -> torch.Tensor:
    """The explained class of every volume as a contiguous LongTensor [B] on logits.device: `target` None = the arg-max of its logits,
    an int = that class for all, a tensor = one class per volume.  Nothing is validated (check_target): a class outside [0, C) reaches
    the kernels, which answer with NaN."""
    if target is None:
        return logits.argmax(dim=1)
    if torch.is_tensor(target):
        return target.to(device=logits.device, dtype=torch.long).reshape(-1).contiguous()
    return torch.full((logits.shape[0],), int(target), dtype=torch.long, device=logits.device)


def cached_table(owner, name: str, key, build):
    """build() once per key, kept in the dict `owner.<name>`: the job tables and labels of one geometry - device tensors made by integer
    arithmetic on torch.arange.  At most 16 entries; a 17th clears the cache first."""
    cache = owner.__dict__.setdefault(name, {})
    if key not in cache:
        if len(cache) >= 16:
            cache.clear()
        cache[key] = build()
    return cache[key]


def _w16(w: torch.Tensor) -> torch.Tensor:
    """16-bit MFMA operand copy (the process's current operand format, _cabi.set_operand_format) of an fp32 [out, in] weight
    (standalone modules; inside a ViT the arena's shadow serves)."""
    return ops.cast_bf16(w.detach().reshape(w.shape[0], -1).float())


def _new_seed(p: float, training: bool) -> int:
    return int(torch.randint(0, 2 ** 62, (1,)).item()) if (training and p > 0) else 0


def _as_rows(x: torch.Tensor):
    if not x.is_cuda:
        raise RuntimeError("neurovit_amd: module inputs must live on the MI355X (cuda) device - there is no CPU fallback")
    d = x.shape[-1]
    return x.reshape(-1, d).float().contiguous(), d


class _FeedForwardFn(torch.autograd.Function):
    """vit_3d.py:16-26 standalone: LayerNorm -> Linear -> exact-erf GELU -> Dropout -> Linear -> Dropout, the same gfx950
    kernels (and cast points) the fused engine runs, one C-ABI call per stage."""

    @staticmethod
    def forward(ctx, x, gamma, beta, w1, b1, w2, b2, p, seeds):
        x2, d = _as_rows(x)
        xn, st = ops.ln_fwd(x2, gamma.detach(), beta.detach())
        w1_16, w2_16 = _w16(w1), _w16(w2)
        u = torch.empty((x2.shape[0], w1.shape[0]), dtype=ops.op16(), device=x.device)
        h = ops.gemm(ops.NT, ops.EPI_BIAS_GELU, xn, w1_16, bias=b1.detach(), aux_out=u, drop_seed=seeds[0], drop_p=p if seeds[0] else 0.0)
        y = ops.gemm(ops.NT, ops.EPI_BIAS_F32, h, w2_16, bias=b2.detach())
        if seeds[1]:
            y = ops.dropout_apply(y, seeds[1], p, want16=False, want32=True)[1]
        ctx.save_for_backward(x2, xn, st, u, h, w1_16, w2_16, gamma.detach())
        ctx.p, ctx.seeds, ctx.shape = p, seeds, x.shape
        return y.view(*x.shape[:-1], w2.shape[0])

    @staticmethod
    def backward(ctx, dy):
        x2, xn, st, u, h, w1_16, w2_16, gamma = ctx.saved_tensors
        p, seeds = ctx.p, ctx.seeds
        dy2 = dy.reshape(-1, dy.shape[-1]).float().contiguous()
        dy16 = ops.dropout_apply(dy2, seeds[1], p if seeds[1] else 0.0)[0]
        dw2 = ops.gemm(ops.TN, ops.EPI_STORE_F32, dy16, h)
        db2 = ops.colsum_bf16(dy16)
        du = ops.gemm(ops.NN, ops.EPI_DGELU, dy16, w2_16, aux_in=u, drop_seed=seeds[0], drop_p=p if seeds[0] else 0.0)
        dw1 = ops.gemm(ops.TN, ops.EPI_STORE_F32, du, xn)
        db1 = ops.colsum_bf16(du)
        dxn = ops.gemm(ops.NN, ops.EPI_STORE_F32, du, w1_16)
        dx, _, dgamma, dbeta, _ = ops.ln_bwd(dxn, x2, st, gamma, want_g16=False)
        return dx.view(ctx.shape), dgamma, dbeta, dw1, db1, dw2, db2, None, None


class _AttentionFn(torch.autograd.Function):
    """vit_3d.py:48-60 standalone: LayerNorm -> to_qkv -> softmax(q k^T * scale) (+Dropout) -> attn v -> to_out (+Dropout)."""

    @staticmethod
    def forward(ctx, x, gamma, beta, wqkv, wo, bo, heads, dim_head, p, seeds, attend=None):
        ctx.attend = attend               # the module's nn.Softmax: its backward hooks are looked up when the backward runs
        if x.dim() != 3:
            raise ValueError("neurovit_amd.Attention: expected x of shape [batch, tokens, dim]")
        B, n, _ = x.shape
        x2, d = _as_rows(x)
        xn, st = ops.ln_fwd(x2, gamma.detach(), beta.detach())
        wqkv16, wo16 = _w16(wqkv), _w16(wo)
        qkv = ops.gemm(ops.NT, ops.EPI_STORE_BF16, xn, wqkv16)
        ao, lse = ops.attn_fwd(qkv, B, n, heads, dim_head, drop_seed=seeds[0], drop_p=p if seeds[0] else 0.0)
        y = ops.gemm(ops.NT, ops.EPI_BIAS_F32, ao, wo16, bias=bo.detach())
        if seeds[1]:
            y = ops.dropout_apply(y, seeds[1], p, want16=False, want32=True)[1]
        ctx.save_for_backward(x2, xn, st, qkv, ao, lse, wqkv16, wo16, gamma.detach())
        ctx.meta = (B, n, heads, dim_head, p, seeds, x.shape)
        return y.view(B, n, wo.shape[0])

    @staticmethod
    def backward(ctx, dy):
        x2, xn, st, qkv, ao, lse, wqkv16, wo16, gamma = ctx.saved_tensors
        B, n, heads, dim_head, p, seeds, shape = ctx.meta
        dy2 = dy.reshape(-1, dy.shape[-1]).float().contiguous()
        dy16 = ops.dropout_apply(dy2, seeds[1], p if seeds[1] else 0.0)[0]
        dwo = ops.gemm(ops.TN, ops.EPI_STORE_F32, dy16, ao)
        dbo = ops.colsum_bf16(dy16)
        dao = ops.gemm(ops.NN, ops.EPI_STORE_BF16, dy16, wo16)
        dqkv, _ = ops.attn_bwd(qkv, ao, dao, lse, B, n, heads, dim_head, drop_seed=seeds[0], drop_p=p if seeds[0] else 0.0)
        hooks = _attend_backward_hooks(ctx.attend) if ctx.attend is not None else []
        if hooks:
            if seeds[0]:
                raise NotImplementedError("neurovit_amd.Attention: backward hooks on `attend` with attention dropout active - the mask is not "
                                          "replayed into the gradient of the probabilities; run the attribution in eval mode")
            _fire_attend_backward_hooks(ctx.attend, hooks, ops.attn_grad(qkv, dao, B, n, heads, dim_head), "neurovit_amd.Attention")
        dwqkv = ops.gemm(ops.TN, ops.EPI_STORE_F32, dqkv, xn)
        dxn = ops.gemm(ops.NN, ops.EPI_STORE_F32, dqkv, wqkv16)
        dx, _, dgamma, dbeta, _ = ops.ln_bwd(dxn, x2, st, gamma, want_g16=False)
        return dx.view(shape), dgamma, dbeta, dwqkv, dwo, dbo, None, None, None, None, None


def _attend_backward_hooks(attend) -> list:
    """The backward hooks registered on an `attend` module (register_full_backward_hook, or the legacy register_backward_hook), the global
    module backward hooks first - looked up when the backward runs, as autograd does."""
    from torch.nn.modules import module as _module
    return list(_module._global_backward_hooks.values()) + list(attend._backward_hooks.values())


def _check_no_backward_pre_hooks(attend, who: str) -> None:
    from torch.nn.modules import module as _module
    if getattr(attend, "_backward_pre_hooks", None) or getattr(_module, "_global_backward_pre_hooks", None):
        raise NotImplementedError(f"{who}: backward pre-hooks on `attend` are not supported - they may replace the gradient w.r.t. the "
                                  "attention probabilities, which the fused attention backward never reads back; register a full backward hook")


def _fire_attend_backward_hooks(attend, hooks, dP, who: str) -> None:
    """hook(attend, grad_input, grad_output) = hook(attend, (None,), (dP,)): dP fp32 [B, heads, n, n] on the device = the gradient w.r.t.
    the output of `attend`.  grad_input is (None,): the input of `attend`, the score matrix q k^T * scale, is never an autograd input
    here (the fused kernels form it tile by tile), so no gradient w.r.t. it exists to hand over."""
    for hook in hooks:
        if hook(attend, (None,), (dP,)) is not None:
            raise RuntimeError(f"{who}: a backward hook on `attend` returned a value - in PyTorch it would replace the gradient w.r.t. the "
                               "score matrix, which the native backward cannot honour; return None")


class FeedForward(nn.Module):
    """vit_3d.py:14-26 - parameter container (net.0 LayerNorm, net.1 Linear, net.4 Linear)."""

    def __init__(self, dim, hidden_dim, dropout=0.):
        super().__init__()
        self.net = nn.Sequential(
            nn.LayerNorm(dim),
            nn.Linear(dim, hidden_dim),
            nn.GELU(),
            nn.Dropout(dropout),
            nn.Linear(hidden_dim, dim),
            nn.Dropout(dropout)
        )

    def forward(self, x):
        """Standalone use (vit_3d.py:25-26; inside ViT.forward the block runs fused in the native engine): x [..., dim] fp32
        on the device -> net(x), differentiable, dropout honoured in train mode."""
        ln, fc1, fc2 = self.net[0], self.net[1], self.net[4]
        p = float(self.net[3].p)
        seeds = (_new_seed(p, self.training), _new_seed(p, self.training))
        return _FeedForwardFn.apply(x, ln.weight, ln.bias, fc1.weight, fc1.bias, fc2.weight, fc2.bias, p, seeds)


class Attention(nn.Module):
    """vit_3d.py:28-60 - parameter container (norm, to_qkv without bias, to_out.0)."""

    def __init__(self, dim, heads=8, dim_head=64, dropout=0.):
        super().__init__()
        inner_dim = dim_head * heads
        project_out = not (heads == 1 and dim_head == dim)
        self.heads = heads
        self.dim_head = dim_head
        self.scale = dim_head ** -0.5
        self.norm = nn.LayerNorm(dim)
        self.attend = nn.Softmax(dim=-1)
        self.dropout = nn.Dropout(dropout)
        self.to_qkv = nn.Linear(dim, inner_dim * 3, bias=False)
        self.to_out = nn.Sequential(
            nn.Linear(inner_dim, dim),
            nn.Dropout(dropout)
        ) if project_out else nn.Identity()

    def forward(self, x):
        """Standalone use (vit_3d.py:48-60): x [batch, tokens, dim] fp32 on the device -> to_out(attention(norm(x)))."""
        if self.dim_head % 8 or not 8 <= self.dim_head <= 128:
            raise NotImplementedError("neurovit_amd: dim_head must be a multiple of 8 up to 128 (64, the vit_3d.py:78 default and "
                                      "the only value the NeuroEncoder path uses, runs the MFMA attention kernels; the others scalar ones)")
        p = float(self.dropout.p)
        self._attend_hooks(x)
        if isinstance(self.to_out, nn.Identity):
            # heads == 1, dim_head == dim: no projection and no trailing dropout (vit_3d.py:43-46) - the same kernels with the
            # identity as the weight (x I + 0 is exact) and the output-dropout site off
            dim = self.heads * self.dim_head
            eye, zero = torch.eye(dim, device=x.device), torch.zeros(dim, device=x.device)
            return _AttentionFn.apply(x, self.norm.weight, self.norm.bias, self.to_qkv.weight, eye, zero, self.heads, self.dim_head, p,
                                      (_new_seed(p, self.training), 0), self.attend)
        seeds = (_new_seed(p, self.training), _new_seed(p, self.training))
        return _AttentionFn.apply(x, self.norm.weight, self.norm.bias, self.to_qkv.weight, self.to_out[0].weight, self.to_out[0].bias,
                                  self.heads, self.dim_head, p, seeds, self.attend)


    def _attend_hooks(self, x):
        """Forward hooks on `attend` (nn.Softmax, vit_3d.py:54): the fused kernels never materialise its output, so with hooks registered
        the probabilities are recomputed from the same qkv (nv_attn_probs, fp32 [B, heads, n, n], pre-dropout) and the hooks are called
        with them as hook(attend, (), P), before the attention itself runs."""
        from torch.nn.modules import module as _module
        if self.attend._forward_pre_hooks:
            raise NotImplementedError("neurovit_amd.Attention: forward pre-hooks on `attend` are not supported - the score matrix is never "
                                      "materialised; register a forward hook to read the probabilities")
        _check_no_backward_pre_hooks(self.attend, "neurovit_amd.Attention")
        hooks = list(_module._global_forward_hooks.items()) + list(self.attend._forward_hooks.items())
        if not hooks:
            return
        if x.dim() != 3:
            raise ValueError("neurovit_amd.Attention: expected x of shape [batch, tokens, dim]")
        B, n, _ = x.shape
        x2, _ = _as_rows(x.detach())
        xn, _ = ops.ln_fwd(x2, self.norm.weight.detach(), self.norm.bias.detach())
        qkv = ops.gemm(ops.NT, ops.EPI_STORE_BF16, xn, _w16(self.to_qkv.weight))
        P = ops.attn_probs(qkv, B, n, self.heads, self.dim_head)
        for hid, hook in hooks:
            result = hook(self.attend, (), {}, P) if hid in self.attend._forward_hooks_with_kwargs else hook(self.attend, (), P)
            if result is not None:
                raise RuntimeError("neurovit_amd.Attention: a forward hook on `attend` returned a value - it would replace the attention "
                                   "probabilities, which the fused kernels cannot honour; return None")


class Transformer(nn.Module):
    """vit_3d.py:62-75."""

    def __init__(self, dim, depth, heads, dim_head, mlp_dim, dropout=0.):
        super().__init__()
        self.layers = nn.ModuleList([])
        for _ in range(depth):
            self.layers.append(nn.ModuleList([
                Attention(dim, heads=heads, dim_head=dim_head, dropout=dropout),
                FeedForward(dim, mlp_dim, dropout=dropout)
            ]))

    # stochastic depth of the ViT that owns this module (ViT.drop_path_rate / drop_path_schedule read and write these): the per-sample
    # factors live in the native engine's residual adds, which a standalone call of this module does not run
    drop_path_rate = 0.0
    drop_path_schedule = "linear"

    def forward(self, x):
        """Standalone use (vit_3d.py:72-75): pre-norm residual blocks, no final LayerNorm."""
        if self.training and self.drop_path_rate > 0:
            raise NotImplementedError("neurovit_amd.Transformer: called on its own in train mode with drop_path_rate > 0 - stochastic depth is "
                                      "applied by ViT.forward (the native engine's residual adds); call eval() or set the rate to 0")
        for attn, ff in self.layers:
            x = attn(x) + x
            x = ff(x) + x
        return x


class PatchRearrange(nn.Module):
    """Placeholder for einops `Rearrange('b c (f pf) (h p1) (w p2) -> b (f h w) (p1 p2 pf c)')`
    (vit_3d.py:92): keeps `to_patch_embedding.{1,2,3}` state_dict indices.  The index map itself is
    executed inside the patch-gather kernel (csrc/norm.hip::patch_ln_fwd_kernel)."""

    def __init__(self, p1, p2, pf):
        super().__init__()
        self.p1, self.p2, self.pf = p1, p2, pf

    def extra_repr(self):
        return f"'b c (f pf) (h p1) (w p2) -> b (f h w) (p1 p2 pf c)', p1={self.p1}, p2={self.p2}, pf={self.pf}"


def _batch_dense(t: torch.Tensor) -> bool:
    """every sample of t is one run of t[0].numel() elements of its storage (in any axis order), one sample after the other"""
    V, expect = t[0].numel(), 1
    if t.shape[0] > 1 and t.stride(0) != V:
        return False
    for stride, size in sorted((st, sz) for sz, st in zip(t.shape[1:], t.stride()[1:]) if sz > 1):
        if stride != expect:
            return False
        expect *= size
    return True


class _ViTFunction(torch.autograd.Function):
    """Whole-encoder autograd node.  Parameters are passed as inputs only so autograd knows the output
    depends on them; their gradients are written by the engine directly into the module's gradient
    arena (which `param.grad` views), so backward returns None for them (no per-tensor accumulate copies).
    The gradient w.r.t. `video` is returned in its slot when autograd asks for it (ctx.needs_input_grad[1])."""

    @staticmethod
    def forward(ctx, module, video, need_grad, extra, *params):
        # need_grad is decided by the caller: grad mode is always off inside Function.forward, and ctx.needs_input_grad
        # reflects requires_grad alone (it stays True under torch.no_grad()), so neither tells whether a graph is being built
        ctx.module = module
        out = module._run_forward(video, need_grad, extra, paths=True)
        ctx.rec = module._rt.current if need_grad else None   # THIS pass's workspace and input ...
        ctx.claim = ctx.rec.claim() if need_grad else None    # ... held until its backward has run or the graph is gone
        return out

    @staticmethod
    def backward(ctx, dlogits):
        rt, rec = ctx.module._rt, ctx.rec
        if rec is None or not rt.pass_is_live(rec):
            raise RuntimeError(
                "neurovit_amd.ViT: backward() of a forward pass whose activations have been overwritten - a pass keeps its workspace "
                "until one whole backward of it has run; a second backward (retain_graph) after another training forward or a train "
                "step of the same module finds it refilled.")
        dvideo = None
        if ctx.needs_input_grad[1]:
            # the input's own strides when they describe a dense, non-overlapping tensor (the [B, H, W, D] -> [B, 1, D, H, W] permute view
            # of ViT3DEncoder: the kernel then writes the memory order it read), contiguous otherwise
            dvideo = torch.empty_like(rec.video, memory_format=torch.preserve_format)
        ctx.module._run_backward(rec, dlogits, dvideo)     # several passes may be pending (siamese / two-forward losses): each runs against its own workspace
        return (None, dvideo, None, None) + (None,) * len(ctx.module._plist)


class _ViTTokensFunction(torch.autograd.Function):
    """_ViTFunction's sibling for ViT.forward_tokens: the output is the last block's tokens, and backward hands their gradient to the
    engine's token-level entry (nv_vit_backward_tokens).  Parameter gradients land in the gradient arena; the head gets zeros."""

    @staticmethod
    def forward(ctx, module, video, need_grad, *params):
        ctx.module = module
        out = module._run_forward_tokens(video)
        ctx.rec = module._rt.current if need_grad else None
        ctx.claim = ctx.rec.claim() if need_grad else None
        return out

    @staticmethod
    def backward(ctx, dtokens):
        rt, rec = ctx.module._rt, ctx.rec
        if rec is None or not rt.pass_is_live(rec):
            raise RuntimeError("neurovit_amd.ViT: backward() of a forward_tokens pass whose activations have been overwritten - a pass keeps its "
                               "workspace until one whole backward of it has run")
        dvideo = torch.empty_like(rec.video, memory_format=torch.preserve_format) if ctx.needs_input_grad[1] else None
        ctx.module._run_backward_tokens(rec, dtokens, dvideo)
        return (None, dvideo, None) + (None,) * len(ctx.module._plist)


class ViT(FlatArena, nn.Module):
    """vit_3d.py:77-126, MI355X-native.  forward(video[B, C, F, H, W]) -> [B, num_classes] (fp32)."""

    def __init__(self, *, image_size, image_patch_size, frames, frame_patch_size, num_classes, dim, depth, heads, mlp_dim,
                 pool='cls', channels=3, dim_head=64, dropout=0., emb_dropout=0., drop_path_rate=0.0, drop_path_schedule="linear"):
        super().__init__()
        ops.check_drop_path(drop_path_rate, drop_path_schedule)
        image_height, image_width = pair(image_size)
        patch_height, patch_width = pair(image_patch_size)

        assert image_height % patch_height == 0 and image_width % patch_width == 0, 'Image dimensions must be divisible by the patch size.'
        assert frames % frame_patch_size == 0, 'Frames must be divisible by frame patch size'

        num_patches = (image_height // patch_height) * (image_width // patch_width) * (frames // frame_patch_size)
        patch_dim = channels * patch_height * patch_width * frame_patch_size

        assert pool in {'cls', 'mean'}, 'pool type must be either cls (cls token) or mean (mean pooling)'

        self.to_patch_embedding = nn.Sequential(
            PatchRearrange(patch_height, patch_width, frame_patch_size),
            nn.LayerNorm(patch_dim),
            nn.Linear(patch_dim, dim),
            nn.LayerNorm(dim),
        )

        self.pos_embedding = nn.Parameter(torch.randn(1, num_patches + 1, dim))
        self.cls_token = nn.Parameter(torch.randn(1, 1, dim))
        self.dropout = nn.Dropout(emb_dropout)

        self.transformer = Transformer(dim, depth, heads, dim_head, mlp_dim, dropout)
        # stochastic depth (beyond the reference; timm's drop_path_rate): in train mode branch c of block l is dropped per sample with probability
        # q_l ("linear": rate * l / (depth - 1), "constant": rate) and kept samples are scaled by 1 / (1 - q_l).  Plain attributes, also of a loaded model.
        self.drop_path_rate, self.drop_path_schedule = drop_path_rate, drop_path_schedule
        self.last_drop_path = None      # the factor table [depth, 2, B] of the most recent training forward or native step (device; None before)
        self._path_bufs = {}

        self.pool = pool
        self.to_latent = nn.Identity()

        self.mlp_head = nn.Sequential(
            nn.LayerNorm(dim),
            nn.Linear(dim, num_classes)
        )

        # ---- native engine state (not part of the reference surface) ----
        # heads == 1 with dim_head == dim: the reference drops to_out (nn.Identity, vit_3d.py:32,43-46).  The engine's parameter
        # table always carries the projection, so the arena keeps those slots as CONSTANTS no nn.Parameter views - weight = identity,
        # bias = 0: x + I ao + 0 is exactly x + ao (products with 1.0 and sums with 0.0 are exact), its data gradient g I is
        # exactly g, and the optimizer never sees them (see _packed / mark_shadow_fresh)
        self._no_proj = (heads == 1 and dim_head == dim)
        self._dropout_p = (float(dropout), float(emb_dropout))
        self._cfg = engine.make_config(image_size=image_height, image_patch_size=patch_height, image_width=image_width, patch_width=patch_width, frames=frames,
                                       frame_patch_size=frame_patch_size, num_classes=num_classes, dim=dim, depth=depth,
                                       heads=heads, mlp_dim=mlp_dim, channels=channels, dim_head=dim_head,
                                       pool=pool)
        self._rt = engine.VitRuntime(self._cfg)
        self._init_arena()                              # arena.FlatArena: _arena, _grads, _plist, ...; _shadow and _phantom are set in _packed
        self._layout = None                             # (offsets, numels, total) of engine.param_layout without the constant slots
        self._shadow_key = None
        self._last_logits = None   # most recent forward's logits (the Trainer shell reads them without a second forward)
        self._grad_sync = None     # parallel.GradSync: all-reduce gradient buckets while backward still runs
        self._fp8 = None           # enable_fp8(): e4m3 weights + scales for inference forwards
        self.fp8_training = False  # enable_fp8(training=True): training forwards on e4m3 operands too
        # Arithmetic of eval-mode forwards that record no graph: "bf16" (bf16 MFMA operands, the training arithmetic) or "fp32"
        # (every operand fp32 on the fp32 MFMA: what the reference's validate computes, Trainer.py:101-118 - logits within 1e-5
        # of its CPU forward, about 3x the time).  Set directly, through `precision(...)`, or by the config key
        # TRAINING_VIT_EVAL_PRECISION of ViT3DEncoder.
        self.eval_precision = "bf16"
        # 16-bit MFMA operand format: "bf16" (default, BASELINE.json's dtype) or "fp16" - the reference's own training arithmetic
        # (torch.autocast(float16), Trainer.py:68): 11 instead of 8 significand bits at the same MFMA rate, which puts the logits
        # within 1e-3 of the reference's fp32 CPU forward; TrainStep then scales the loss (GradScaler, Trainer.py:29,74-76).  set_operands().
        self.operands = "bf16"
        # inference forwards (eval mode or no dropout, no graph recorded) run their blocks with the LayerNorms folded into the GEMMs around them
        # (engine.VitRuntime.forward_lnfold: 21 of ViT3D-base's 24 LayerNorm launches gone); NEUROVIT_LN_FOLD=0 / fold_layernorm = False: the plain launches
        import os as _os
        self.fold_layernorm = _os.environ.get("NEUROVIT_LN_FOLD", "1") != "0"
        self._fold = None

    def _fresh_fold(self):
        """folded weights of the current parameters (recomputed in place when the stock or the fused optimizer changed them)"""
        key = (self._param_key(), self.operands)
        if self._fold is None or self._fold["key"] != key:
            self._fold = dict(self._rt.lnfold_prepare(self._arena, reuse=self._fold), key=key)
        return self._fold

    def set_operands(self, fmt: str):
        """Switch the operand format of the shadow arena, the activations and the MFMA kernels: "bf16" or "fp16"."""
        if fmt not in _cabi.OPERAND_FORMATS:
            raise ValueError(f"neurovit_amd.ViT: operands must be 'bf16' or 'fp16', got {fmt!r}")
        if fmt != self.operands:
            if fmt == "fp16" and self._fp8 is not None:
                raise RuntimeError("neurovit_amd.ViT: the fp8 path is built beside bf16 operands - disable_fp8() first")
            self.operands = fmt
            self._rt.operands = fmt
            if self._shadow is not None:
                self._shadow = torch.empty(self._shadow.numel(), dtype=self._dtype16(), device=self._shadow.device)
            self._shadow_key = None
        return self

    def _dtype16(self) -> torch.dtype:
        return torch.float16 if self.operands == "fp16" else torch.bfloat16

    # ------------------------------------------------------------------ arena management
    # entries of the native parameter table (engine.param_layout): 8 ahead of the blocks, 11 per block l at 8 + 11 l + k
    _QKV_W, _OUT_W, _OUT_B, _FC1_W, _FC2_W = 2, 3, 4, 7, 9

    def _block_entries(self, *which):
        return [8 + 11 * l + k for l in range(self._cfg.depth) for k in which]

    def _build_arena(self):
        """The layout is the engine's parameter table, less the constant slots (see __init__); FlatArena._pack does the rest."""
        plist = [p for _, p in self.named_parameters()]
        if self._layout is None:
            off, num, total = engine.param_layout(self._cfg)
            # to_out.0.weight / .bias of every block are no module parameter without the projection
            out_w, out_b = (self._block_entries(self._OUT_W), self._block_entries(self._OUT_B)) if self._no_proj else ([], [])
            drop = sorted(out_w + out_b)
            kept = [i for i in range(len(off)) if i not in drop]
            self._phantom_slots = [(off[i], num[i], i in out_w) for i in drop]
            assert len(kept) == len(plist) and all(p.numel() == num[i] for p, i in zip(plist, kept)), \
                "parameter table of the native engine does not match the module tree"
            self._layout = ([off[i] for i in kept], [num[i] for i in kept], total)
            # positions in _plist of the blocks' Linear weights (linear_weight_grads)
            self._linear_weights = [kept.index(i) for i in self._block_entries(self._QKV_W, self._OUT_W, self._FC1_W, self._FC2_W) if i in kept]
        self._pack(plist, *self._layout)

    def _packed(self):
        """the constant slots, and a 16-bit shadow that is cast on its next use"""
        arena = self._arena
        self._phantom = []
        for o, n, is_weight in self._phantom_slots:
            if is_weight:
                arena[o:o + n].copy_(torch.eye(self._cfg.dim, dtype=torch.float32, device=arena.device).reshape(-1))
            self._phantom.append((o, arena[o:o + n].clone()))
        self._shadow = torch.empty(arena.numel(), dtype=self._dtype16(), device=arena.device)
        self._shadow_key = None

    def gather_foreign_grads(self):
        """Nothing is gathered for the encoder: the fused step applies what the gradient arena holds, which is what its backward
        passes write unless foreign code has set a .grad of its own (FlatArena._backward_to_grads adds into such a tensor)."""

    def linear_weight_grads(self, present: bool):
        """.grad of the blocks' Linear weights (to_qkv, to_out, FC1, FC2): their views of the gradient arena, or - after a step
        that updated them inside their weight-gradient GEMMs and never stored their gradients (TrainStep fuse_update = 1) - None
        rather than a stale gradient.  The first of them stands for all: they are set and cleared together."""
        have = self._plist[self._linear_weights[0]].grad is not None
        if present and not have:
            self.install_grad_views(self._linear_weights)
        elif have and not present:
            for i in self._linear_weights:
                self._plist[i].grad = None

    def mark_shadow_fresh(self):
        """Called by the fused AdamW, which writes the arena and the bf16 shadow itself (through raw pointers: no tensor
        `_version` moves, so the generation counter is what tells derived copies - the fp8 weights - that they are stale)."""
        for o, const in self._phantom:           # the fused step ran over the whole arena: put the constant slots back
            self._arena[o:o + const.numel()].copy_(const)
            self._shadow[o:o + const.numel()].copy_(const)
        self._shadow_key = tuple(p._version for p in self._plist)
        self._param_generation += 1

    def mark_arena_rewritten(self):
        """Called by whatever rewrites the arena through raw pointers WITHOUT writing the 16-bit shadow (optim.ModelEma.update): the
        shadow is stale and is cast again before its next use, and the generation counter tells the folded and the fp8 weights so.
        (The constant slots need no repair: the average of a constant with itself is that constant, bit for bit.)"""
        self._shadow_key = None
        self._param_generation += 1

    def _param_key(self):
        return (self._param_generation, tuple(p._version for p in self._plist))

    def _refresh_shadow(self):
        key = tuple(p._version for p in self._plist)
        if key != self._shadow_key:
            _cabi.set_operand_format(self.operands)
            ops.cast_bf16(self._arena.view(1, -1), out=self._shadow.view(1, -1))
            self._shadow_key = key

    # ------------------------------------------------------------------ fp8 inference (BASELINE.json configs[4])
    def enable_fp8(self, calibration_video: torch.Tensor, headroom: float = 2.0, out_proj: bool = True, training: bool = False):
        """Switch inference forwards (no grad being recorded) to the fp8 path: qkv / out-projection / FC1 / FC2 of every block on OCP
        e4m3 MFMA operands (out_proj = False keeps the out-projection, 8 % of the linear FLOPs, on bf16).  `calibration_video` ([B, C, F, H, W] on the device) fixes the per-tensor activation scales; weights are
        re-quantised from the fp32 master parameters whenever they have changed.
        training = True additionally runs TRAINING forwards with qkv / FC1 / FC2 on e4m3 operands (nv_vit_forward_fp8_train; the
        backward pass stays on bf16 operands and reads the bf16 activations the same forward kernels write): the weights are
        re-quantised after every optimizer step (in place), the activation scales stay those of the calibration batch - call
        enable_fp8 again to recalibrate.  Dropout works as in the bf16 forward (same masks).  Default: training forwards keep using bf16."""
        if self.operands != "bf16":
            raise RuntimeError("neurovit_amd.ViT: the fp8 path is built beside bf16 operands - set_operands('bf16') first")
        if training:
            self.refuse_drop_path("enable_fp8(training=True)")
        self.flat_parameters()
        self._refresh_shadow()
        scales = self._rt.calibrate_fp8(calibration_video.float(), self._arena, self._shadow, headroom, out_proj)
        self._fp8 = self._rt.quantize_fp8(self._arena, scales)
        self._fp8["key"] = self._param_key()
        self.fp8_training = bool(training)
        return scales

    def disable_fp8(self):
        self._fp8 = None
        self.fp8_training = False

    def _fresh_fp8(self):
        """the e4m3 weights of the current parameters (re-quantised in place when the stock or the fused optimizer changed them)"""
        if self._fp8["key"] != self._param_key():
            self._fp8 = dict(self._rt.quantize_fp8(self._arena, self._fp8["act_list"], reuse=self._fp8), key=self._param_key())
        return self._fp8

    def precision(self, mode: str):
        """Context manager: eval-mode no-grad forwards inside it run in `mode`: "fp32" (every operand fp32), or "bf16" / "fp16" - both
        name the 16-bit operand path, which runs in this module's operand format (`operands`)."""
        import contextlib
        if mode not in ("bf16", "fp16", "fp32"):
            raise ValueError(f"neurovit_amd.ViT: precision must be 'bf16', 'fp16' or 'fp32', got {mode!r}")

        @contextlib.contextmanager
        def scope():
            before, self.eval_precision = self.eval_precision, mode
            try:
                yield self
            finally:
                self.eval_precision = before
        return scope()

    # ------------------------------------------------------------------ stochastic depth
    @property
    def drop_path_rate(self) -> float:
        return self.transformer.drop_path_rate

    @drop_path_rate.setter
    def drop_path_rate(self, rate) -> None:
        ops.check_drop_path(rate, self.transformer.drop_path_schedule)
        self.transformer.drop_path_rate = float(rate)

    @property
    def drop_path_schedule(self) -> str:
        return self.transformer.drop_path_schedule

    @drop_path_schedule.setter
    def drop_path_schedule(self, schedule) -> None:
        ops.check_drop_path(self.transformer.drop_path_rate, schedule)
        self.transformer.drop_path_schedule = schedule

    def refuse_drop_path(self, who: str) -> None:
        """NotImplementedError for the paths that carry no path factors, on a model whose rate is positive"""
        if self.drop_path_rate > 0:
            raise NotImplementedError(f"neurovit_amd.ViT: {who} runs without stochastic depth, this model has drop_path_rate = {self.drop_path_rate} - "
                                      "set it to 0 for this path (it is a plain attribute)")

    def draw_drop_path(self, B: int, seed: int, device):
        """The factor table fp32 [depth, 2, B] of the next training forward of B volumes, drawn on the device from the step's dropout seed
        (nv_drop_path_draw: nothing is read back) into a buffer kept per B; None in eval mode or at rate 0.  Also left in `last_drop_path`."""
        if not (self.training and self.drop_path_rate > 0):
            return None
        buf = self._path_bufs.get((B, str(device)))
        cur = self._rt.current
        if buf is not None and cur is not None and cur.drop_path is buf and cur.held and not cur.done:
            buf = None          # a pending pass (siamese / two-forward losses) still needs its table for its backward: this forward takes another
        table = ops.drop_path_draw(seed, B, self._cfg.depth, self.drop_path_rate, self.drop_path_schedule, device=device, out=buf)
        if len(self._path_bufs) >= 16:
            self._path_bufs.clear()
        self._path_bufs[(B, str(device))] = self.last_drop_path = table
        return table

    # ------------------------------------------------------------------ execution
    def draw_dropout(self):
        """(p of the blocks, p of the embedding, seed) of the next forward: (0, 0, 0) in eval mode or without dropout and stochastic depth
        (a positive drop_path_rate draws a seed - the table's - even when both dropout rates are 0)."""
        if self.training and (self._dropout_p[0] > 0 or self._dropout_p[1] > 0 or self.drop_path_rate > 0):
            # nn.Dropout semantics (vit_3d.py:21,23,39,45,100) with a counter-based mask: a fresh seed per forward from
            # torch's CPU generator (so torch.manual_seed reproduces runs); backward recomputes the same masks.
            seed = int(torch.randint(0, 2 ** 62, (1,)).item())
            return (self._dropout_p[0], self._dropout_p[1], seed)
        return (0.0, 0.0, 0)

    def _run_forward(self, video, need_grad, extra=(None, 0, None), paths=False):
        """paths: the forward of ViT.forward - in train mode with a positive drop_path_rate it draws a factor table and runs under it; the
        attribution passes (recording_forward, integrated_gradients) never do."""
        vol_sigma, time_points, export = (tuple(extra) + (None,))[:3]
        drop = self.draw_dropout()
        if self.eval_precision not in ("bf16", "fp16", "fp32"):
            raise ValueError(f"neurovit_amd.ViT: eval_precision must be 'bf16', 'fp16' or 'fp32', got {self.eval_precision!r}")
        if paths and self.training and self.drop_path_rate > 0:
            if time_points:
                raise NotImplementedError("neurovit_amd.ViT: no stochastic depth through the fused 4D input form (time_points) - pass the [B*T, C, F, H, W] volumes")
            if self._fp8 is not None and self.fp8_training:
                raise NotImplementedError("neurovit_amd.ViT: no stochastic depth in the fp8 training forward - disable_fp8() / enable_fp8(training=False), or drop_path_rate = 0")
            self._refresh_shadow()
            table = self.draw_drop_path(video.shape[0], drop[2], video.device)
            # (the training layout also without a graph: the factors live in the training forward's residual adds)
            self._last_logits = self._rt.forward(video, self._arena, self._shadow, training=True, dropout=drop, vol_sigma=vol_sigma, attn_export=export,
                                                 drop_path=table)
            return self._last_logits
        if self.eval_precision == "fp32" and not need_grad and not self.training:
            self._last_logits = self._rt.forward_f32(video, self._arena, vol_sigma=vol_sigma, time_points=time_points, attn_export=export)
            return self._last_logits
        self._refresh_shadow()
        if self._fp8 is not None and not need_grad and not self.training:
            self._last_logits = self._rt.forward_fp8(video, self._arena, self._shadow, self._fresh_fp8(), vol_sigma=vol_sigma, time_points=time_points)
            return self._last_logits
        if self._fp8 is not None and self.fp8_training and need_grad and not time_points:
            self._last_logits = self._rt.forward_fp8_train(video, self._arena, self._shadow, self._fresh_fp8(), dropout=drop, vol_sigma=vol_sigma)
            return self._last_logits
        if self.fold_layernorm and not need_grad and drop[0] == 0.0 and drop[1] == 0.0:
            self._last_logits = self._rt.forward_lnfold(video, self._arena, self._shadow, self._fresh_fold(), vol_sigma=vol_sigma, time_points=time_points,
                                                        attn_export=export)
            return self._last_logits
        self._last_logits = self._rt.forward(video, self._arena, self._shadow, training=need_grad, dropout=drop, vol_sigma=vol_sigma,
                                             time_points=time_points, attn_export=export)
        return self._last_logits

    # ------------------------------------------------------------------ attention probabilities (the output of every block's `attend`)
    def _uses_fp8(self, need_grad: bool) -> bool:
        """the forward about to run is one of the fp8 forwards (which export no attention probabilities)"""
        if self._fp8 is None:
            return False
        return (self.fp8_training and need_grad) or (not need_grad and not self.training and self.eval_precision != "fp32")

    def _attend_hooked_layers(self) -> List[int]:
        """Blocks whose `attend` (nn.Softmax, vit_3d.py:54) has forward hooks - all of them while a global forward hook is registered.
        The native attention never runs that module: the forward exports those layers' probabilities and fires the hooks itself."""
        from torch.nn.modules import module as _module
        layers = []
        for l, (attn, _) in enumerate(self.transformer.layers):
            if attn.attend._forward_pre_hooks:
                raise NotImplementedError("neurovit_amd.ViT: forward pre-hooks on `attend` are not supported - its input, the score matrix "
                                          "q k^T * scale, is never materialised; register a forward hook to read the probabilities")
            if attn.attend._forward_hooks or _module._global_forward_hooks:
                layers.append(l)
        return layers

    def _attend_backward_hooked_layers(self) -> List[int]:
        """Blocks whose `attend` has backward hooks - all of them while a global module backward hook is registered.  The native backward
        never runs that module: it exports those layers' dP = dO V^T behind their attention backward (nv_vit_backward_attn) and fires the
        hooks itself, in reverse layer order."""
        from torch.nn.modules import module as _module
        return [l for l, (attn, _) in enumerate(self.transformer.layers) if attn.attend._backward_hooks or _module._global_backward_hooks]

    def _fire_attend_hooks(self, maps) -> None:
        """hook(attend, (), P_l) for every exported layer, in layer order; P_l fp32 [B, heads, n, n], pre-dropout."""
        from torch.nn.modules import module as _module
        for l in sorted(maps):
            attend = self.transformer.layers[l][0].attend
            hooks = list(_module._global_forward_hooks.items()) + list(attend._forward_hooks.items())
            for hid, hook in hooks:
                if hid in attend._forward_hooks_with_kwargs:
                    result = hook(attend, (), {}, maps[l])
                else:
                    result = hook(attend, (), maps[l])
                if result is not None:
                    raise RuntimeError("neurovit_amd.ViT: a forward hook on `attend` returned a value - in PyTorch it would replace the "
                                       "attention probabilities, which the native forward cannot honour; return None")

    def attention_maps(self, video, layers=None, head_fusion=None, rows="all", vol_sigma=None, time_points=0):
        """One forward in the module's current mode and precision that also returns the attention probabilities of `layers` (default
        all): (logits, {layer: fp32 map}).  Per head (head_fusion None): [B, heads, R, n] - the output of the block's `attend`
        (vit_3d.py:54), pre-dropout; head_fusion "mean" / "max" / "min": [B, R, n].  rows "all": R = n, "cls": R = 1 (row 0).
        Input forms as forward(); for the fused 4D form B counts the B*T volumes.  Hooks on `attend` fire as in forward()."""
        if head_fusion not in _cabi.ATTN_FUSIONS or rows not in _cabi.ATTN_ROWS:
            raise ValueError(f"neurovit_amd.ViT: head_fusion must be None, 'mean', 'max' or 'min' and rows 'all' or 'cls', got {head_fusion!r}, {rows!r}")
        layers = list(range(self._cfg.depth)) if layers is None else sorted({int(l) for l in layers})
        if any(not 0 <= l < self._cfg.depth for l in layers):
            raise ValueError(f"neurovit_amd.ViT: layers must lie in [0, {self._cfg.depth}), got {layers}")
        return self._forward_export(video, vol_sigma, time_points, (layers, head_fusion, rows))

    def attention_rollout(self, video, head_fusion="mean", vol_sigma=None, time_points=0):
        """Attention rollout (the head-fused (A + I) / 2, row-renormalised rule, multiplied over the layers): (logits, [B, N]) - the row
        of the token the head reads (the cls row for pool='cls', the mean of all rows for pool='mean') over the N patch tokens, in
        token order.  One forward exports the fused maps; nv_attn_rollout multiplies them (no [n, n] product is formed)."""
        if head_fusion not in ("mean", "max", "min"):
            raise ValueError(f"neurovit_amd.ViT: rollout fuses the heads by 'mean', 'max' or 'min', got {head_fusion!r}")
        logits, maps = self.attention_maps(video, head_fusion=head_fusion, vol_sigma=vol_sigma, time_points=time_points)
        return logits, ops.attn_rollout([maps[l] for l in range(self._cfg.depth)], start_mean=self.pool == "mean")

    def attention_gradients(self, video, target=None, layers=None, form="per_head", vol_sigma=None, time_points=0, score_grad=None):
        """The gradient of a class score w.r.t. the attention probabilities of `layers` (default all): (logits, {layer: fp32 map}).
        form "per_head": [B, heads, n, n] = d logit_target / d P_l, the gradient w.r.t. the output of the block's `attend` (vit_3d.py:54)
        that attn.register_hook / a backward hook on `attend` give on the reference; form "relevance": [B, n, n] =
        mean_h relu(dP_l * P_l), the layer term of gradient-weighted attention relevance (Chefer et al.).
        target: None = the arg-max class of each volume (as get_attention_map), an int, or a LongTensor [B].
        score_grad (instead of `target`): fp32 [B, C] on the device, the gradient of ANY score w.r.t. the logits, one row per volume - the
        backward is seeded with it in place of the one-hot (the 4D model's seed through its temporal head); the one-hot of c gives the bits
        of target = c.
        Runs one graph-recording forward (the training arithmetic, 16-bit operands: precision("fp32") does not apply) and the data-only
        backward of the one-hot of `target` itself, down to the lowest requested layer: it works under torch.no_grad(), touches no p.grad
        and no gradient arena, and leaves last_attn_norm_grad as a normal backward would.  Forward hooks on `attend` fire as in forward();
        backward hooks do not (no autograd backward runs).  Not available (NotImplementedError) with the fp8 training forward, the fused
        4D input form (time_points) or attention dropout active (train mode with dropout > 0)."""
        if form not in _cabi.ATTN_GRAD_FORMS:
            raise ValueError(f"neurovit_amd.ViT: form must be 'per_head' or 'relevance', got {form!r}")
        depth, C = self._cfg.depth, self._cfg.num_classes
        layers = list(range(depth)) if layers is None else sorted({int(l) for l in layers})
        if not layers or any(not 0 <= l < depth for l in layers):
            raise ValueError(f"neurovit_amd.ViT: layers must be a non-empty subset of [0, {depth}), got {layers}")
        self._check_data_backward(time_points)
        self.check_video(video)
        B = video.shape[0]
        check_target(target, B, C)
        self._check_score_grad(target, score_grad, B, video.device)
        logits = self.recording_forward(video, vol_sigma)
        maps = self.data_backward(target_classes(target, logits) if score_grad is None else score_grad, layers, form)
        return logits, maps

    def _check_data_backward(self, time_points=0):
        """what the recording forward + data-only backward pair cannot serve (NotImplementedError), decided before any device work"""
        if time_points:
            raise NotImplementedError("neurovit_amd.ViT: no attention gradients through the fused 4D input form (time_points) - it is "
                                      "forward-only; pass the [B*T, C, F, H, W] volumes instead")
        if self._fp8 is not None and self.fp8_training:
            raise NotImplementedError("neurovit_amd.ViT: no attention gradients through the fp8 training forward - disable_fp8() or "
                                      "enable_fp8(training=False) first")
        if self.training and self._dropout_p[0] > 0:
            raise NotImplementedError("neurovit_amd.ViT: no attention gradients with attention dropout active (train mode, dropout > 0): the mask "
                                      "is not replayed into the gradient of the probabilities - call eval() for attribution")

    def _check_score_grad(self, target, score_grad, B: int, device) -> None:
        """ValueError for a `score_grad` that is not fp32 [B, C] on the input's device, or that comes together with a `target`"""
        if score_grad is None:
            return
        if target is not None:
            raise ValueError("neurovit_amd.ViT: score_grad and target are mutually exclusive (score_grad IS the gradient of the explained score)")
        C = self._cfg.num_classes
        if not torch.is_tensor(score_grad) or tuple(score_grad.shape) != (B, C) or score_grad.dtype != torch.float32 or score_grad.device != device:
            raise ValueError(f"neurovit_amd.ViT: score_grad must be fp32 [{B}, {C}] on {device} (one row of d score / d logits per volume)")

    def recording_forward(self, video, vol_sigma=None):
        """The forward half of the attribution passes: one graph-recording forward (the training arithmetic) under no_grad, `attend`
        forward hooks fired; returns the logits.  data_backward() runs against it.  The caller has done the checks (_check_data_backward,
        check_video)."""
        B = video.shape[0]
        hooked = self._attend_hooked_layers()
        fwd_export, fwd_maps = self._rt.make_attn_export(B, hooked, None, "all", video.device) if hooked else (None, {})
        with torch.no_grad():
            logits = self._run_forward(video.detach().float(), True, (vol_sigma, 0, fwd_export))
            if hooked:
                self._fire_attend_hooks(fwd_maps)
        return logits

    def data_backward(self, seed, layers=None, form="per_head"):
        """The data-only backward of the most recent recording_forward(), seeded with `seed`: a LongTensor [B] of classes (their one-hot)
        or fp32 [B, C] rows of d score / d logits.  With `layers` it runs down to the lowest of them and returns their attention gradients
        {layer: map} in `form` (attention_gradients); without, through the head and the last block only - enough for the Grad-CAM hook
        gradient - and returns {}.  No p.grad, no gradient arena; leaves last_attn_norm_grad as a normal backward would."""
        depth, C = self._cfg.depth, self._cfg.num_classes
        with torch.no_grad():
            dlogits = torch.nn.functional.one_hot(seed, C).to(torch.float32) if seed.dtype == torch.long else seed
            rec = self._rt.current
            export, maps = self._rt.make_attn_grad_export(rec.B, layers, form, rec.video.device) if layers else (None, {})
            # stages 0 (head) .. depth - min(layers): the layers below the lowest requested one and the embedding add nothing; nothing more
            # of this pass will run, and the last block's hook gradient (stage 1) is in the workspace (final)
            self._rt.backward(dlogits, self._arena, self._shadow, None, accumulate=False, stages=(0, depth - layers[0] if layers else 1),
                              weight_grads=False, attn_grad=export, final=True)
        return maps

    def gradcam_taps(self, video, score_grad, vol_sigma=None):
        """The Grad-CAM taps for a given gradient of the logits, without an autograd graph and without an input gradient: one
        recording forward and the data-only backward of score_grad (fp32 [B, C] on the device) through the head and the last block.
        Returns the logits; last_attn_norm_output_raw() / last_attn_norm_grad_raw() then hold the activation and the hook gradient.
        Exports no attention; refusals and side effects (none) as attention_gradients."""
        self._check_data_backward()
        self.check_video(video)
        self._check_score_grad(None, score_grad, video.shape[0], video.device)
        if score_grad is None:
            raise ValueError("neurovit_amd.ViT: gradcam_taps needs score_grad, fp32 [B, C] on the device")
        logits = self.recording_forward(video, vol_sigma)
        self.data_backward(score_grad)
        return logits

    def attention_relevance(self, video, target=None, score_grad=None):
        """Class-specific relevance of the patch tokens (gradient-weighted attention relevance, Chefer et al. "Generic Attention-model
        Explainability": A_l = mean_h relu(dP_l * P_l), R <- R + A_l R from R = I): (logits, [B, N]) - the row of the token the head
        reads (the cls row for pool='cls', the mean of all rows for pool='mean') over the N patch tokens, in token order.  One forward
        and one data-only backward export the A_l (attention_gradients, form "relevance"); nv_attn_relevance accumulates
        u <- u + u A_l from the last layer down (no [n, n] product is formed).  target / score_grad as attention_gradients."""
        logits, maps = self.attention_gradients(video, target=target, form="relevance", score_grad=score_grad)
        return logits, ops.attn_relevance([maps[l] for l in range(self._cfg.depth)], start_mean=self.pool == "mean")

    def integrated_gradients(self, video, target=None, baseline=0.0, steps=50, method="gausslegendre", score="logit", chunk=None,
                             vol_sigma=None, time_points=0):
        """Integrated gradients of a class score along the straight path from a baseline to the input (Sundararajan et al.; captum's
        IntegratedGradients): attributions = (x - bl) * sum_k w_k dF/dx(bl + alpha_k (x - bl)), for every volume of the batch.
          video      [B, C, F, H, W] fp32 on the device, non-overlapping and dense with the batch outermost (a contiguous tensor, or the
                     permute view ViT3DEncoder.forward makes of a contiguous [B, H, W, D]); anything else raises ValueError.  The kernels work
                     on the storage order: the point and gradient buffers have `video`'s strides;
          target     None = the arg-max class of each input volume, an int, or a LongTensor [B];
          baseline   a float, or a tensor of video's shape or [1, C, F, H, W] (shared);
          steps, method   the K points and weights of NeuroEncoder.path_quadrature ("gausslegendre", captum's default, "riemann_middle",
                     "riemann_trapezoid");
          score      "logit" or "prob" (the fp32 softmax probability of ops.class_scores);
          chunk      points per pass (None: max(1, min(64, 2^29 // (4 V))), V floats per volume - two [chunk, V] buffers live at once).
        Jobs are volume-major (b, 0 .. K - 1).  Every slice of `chunk` jobs: nv_path_points into one reused buffer, one graph-recording
        forward (as attention_gradients: the training arithmetic, 16-bit operands - precision("fp32") does not apply), nv_class_score_grads,
        the data-only backward into one reused gradient buffer, nv_path_accumulate; nv_path_finish after the loop.  One plain forward of
        cat(x, baseline), in the module's current mode and precision, gives class_idx and the two end scores.
        Returns a dict of device tensors: attributions (video's shape and strides), class_idx [B], score_input / score_baseline [B],
        delta [B] float64 = sum(attributions) - (score_input - score_baseline) with the sum in double (the completeness residual: the
        quadrature error plus the 16-bit arithmetic), alphas / weights [K].
        Works under torch.no_grad(); touches no p.grad and no gradient arena whether the model is trainable or frozen; no autograd
        backward runs, so backward hooks do not fire, and forward hooks on `attend` fire for the plain forward only; nothing is read back
        and nothing synchronises with the host.  Runs in the module's current mode - call eval() first: in train mode every pass
        draws its own dropout masks.  Not available (NotImplementedError) with the fp8 training forward, the fused 4D input form
        (time_points) or RAW volumes (vol_sigma)."""
        from .NeuroEncoder import path_quadrature
        if score not in ops.SCORE_KINDS:
            raise ValueError(f"neurovit_amd.ViT: score must be 'prob' or 'logit', got {score!r}")
        if chunk is not None and (isinstance(chunk, bool) or int(chunk) != chunk or chunk < 1):
            raise ValueError(f"neurovit_amd.ViT: chunk must be a positive integer, got {chunk!r}")
        alphas, weights = path_quadrature(method, steps)             # (ValueError for a bad rule or step count, before any device work)
        if time_points:
            raise NotImplementedError("neurovit_amd.ViT: no integrated gradients through the fused 4D input form (time_points) - it is "
                                      "forward-only; pass the [B*T, C, F, H, W] volumes instead")
        if vol_sigma is not None:
            raise NotImplementedError("neurovit_amd.ViT: no integrated gradients of RAW volumes (vol_sigma / forward_raw): the folded z-score "
                                      "treats sigma as a constant - normalise the volume first and attribute w.r.t. that")
        if self._fp8 is not None and self.fp8_training:
            raise NotImplementedError("neurovit_amd.ViT: no integrated gradients through the fp8 training forward - disable_fp8() or "
                                      "enable_fp8(training=False) first")
        self.check_video(video)
        B, C = video.shape[0], self._cfg.num_classes
        V = video[0].numel()
        if video.dtype != torch.float32 or not _batch_dense(video):
            raise ValueError(f"neurovit_amd.ViT: integrated_gradients needs an fp32 video that is non-overlapping and dense with the batch "
                             f"outermost, got {video.dtype} with shape {tuple(video.shape)} and strides {tuple(video.stride())}")
        baseline = ops.check_baseline("neurovit_amd.ViT", baseline, video.shape)
        check_target(target, B, C)
        K = alphas.shape[0]
        chunk = min(max(1, min(64, 2 ** 29 // (4 * V))) if chunk is None else int(chunk), B * K)
        device, inner = video.device, tuple(video.stride()[1:])

        def like_video(rows):                                        # [rows, C, F, H, W] in the storage order of `video`
            return torch.empty_strided((rows,) + tuple(video.shape[1:]), (V,) + inner, dtype=torch.float32, device=device)

        def flat(t):                                                 # the same memory as dense [rows, V]
            return t.as_strided((t.shape[0], V), (V, 1), t.storage_offset())

        with torch.no_grad():
            video = video.detach()
            alphas, weights = alphas.to(device), weights.to(device)
            ends = like_video(2 * B)
            ends[:B].copy_(video)
            if torch.is_tensor(baseline):
                ends[B:].copy_(baseline.to(device=device, dtype=torch.float32).expand_as(video))
                base = flat(ends[B:]) if baseline.shape[0] == B else flat(ends[B:B + 1])
            else:
                ends[B:].fill_(baseline)
                base = baseline
            x = flat(ends[:B])                                       # (a copy of the input: 16-byte aligned whatever `video` was)
            end_logits = self(ends).float().contiguous()
            cls = target_classes(target, end_logits[:B])

            def build():
                b = torch.arange(B, device=device, dtype=torch.int64)
                jobs = torch.stack([b.repeat_interleave(K), torch.arange(K, device=device, dtype=torch.int64).repeat(B)], 1).to(torch.int32).contiguous()
                zero = torch.zeros(2 * B, device=device, dtype=torch.int64)
                return jobs, torch.stack([b.repeat(2), zero, zero], 1).to(torch.int32).contiguous()      # rows (b, 0, 0): the end scores
            jobs, end_jobs = cached_table(self, "_path_tables", (str(device), B, K), build)
            end_scores = ops.class_scores(end_logits, end_jobs, cls, kind=score)

            points, grads = like_video(chunk), like_video(chunk)
            acc = torch.empty((B, V), dtype=torch.float32, device=device).zero_()
            for first in range(0, B * K, chunk):
                count = min(chunk, B * K - first)
                part = jobs[first:first + count]
                ops.path_points(x, part, alphas, base, out=flat(points[:count]))
                logits = self._run_forward(points[:count], True, (None, 0, None))
                dlogits = ops.class_score_grads(logits.float().contiguous(), part, cls, kind=score)
                self._rt.backward(dlogits, self._arena, self._shadow, None, accumulate=False, dvideo=grads[:count], weight_grads=False)
                ops.path_accumulate(flat(grads[:count]), part, weights, acc)
            attributions = like_video(B)
            ops.path_finish(acc, x, base, out=flat(attributions))
            score_input, score_baseline = end_scores[:B], end_scores[B:]
            delta = flat(attributions).sum(dim=1, dtype=torch.float64) - (score_input.double() - score_baseline.double())
        return {"attributions": attributions, "class_idx": cls, "score_input": score_input, "score_baseline": score_baseline, "delta": delta,
                "alphas": alphas, "weights": weights}

    def _run_backward(self, rec, dlogits, dvideo=None):
        """The backward of pass `rec` (the engine's record of the forward): parameter gradients of every parameter that requires one;
        dvideo (or None): receives d loss / d video.  With no parameter requiring a gradient (a frozen model fed an input that requires one) the data-only backward runs: no gradient arena, no p.grad.
        Backward hooks on a block's `attend` are looked up here: the hooked layers' dP is exported by the same backward (without hooks
        nothing extra is launched) and the hooks fire once it has been queued, in reverse layer order."""
        hooked = self._attend_backward_hooked_layers()
        export, dP = (None, {})
        if hooked:
            if rec.dropout[0] > 0:
                raise NotImplementedError("neurovit_amd.ViT: backward hooks on `attend` with attention dropout active (train mode, dropout > 0) - "
                                          "the mask is not replayed into the gradient of the probabilities; run the attribution in eval mode")
            export, dP = self._rt.make_attn_grad_export(rec.B, hooked, "per_head", rec.video.device)
        self._run_backward_export(rec, dlogits, dvideo, export)
        for l in sorted(dP, reverse=True):
            attend = self.transformer.layers[l][0].attend
            _fire_attend_backward_hooks(attend, _attend_backward_hooks(attend), dP[l], "neurovit_amd.ViT")

    def _run_backward_export(self, rec, dlogits, dvideo, export):
        if not any(p.requires_grad for p in self._plist):
            if dvideo is not None or export is not None:
                self._rt.backward(dlogits, self._arena, self._shadow, None, accumulate=False, dvideo=dvideo, weight_grads=False, attn_grad=export, of=rec)
            return

        def run(target, accumulate, scratch):
            if scratch:       # foreign .grad tensors: one plain backward, no gradient-bucket pipeline
                self._rt.backward(dlogits, self._arena, self._shadow, target, accumulate=False, dvideo=dvideo, attn_grad=export, of=rec)
            else:
                self._backward_into(dlogits, target, accumulate=accumulate, dvideo=dvideo, attn_grad=export, of=rec)
        self._backward_to_grads(run)

    def mirrored_ranges(self):
        """Arena element ranges whose gradients nv_vit_backward_stages16 also writes, rounded to bf16, into `grads16`: the weights of
        the Linear layers (to_qkv, to_out, FC1, FC2 of every block; the patch embedding's when patch_dim % 8 == 0) - 99.4 % of
        ViT3D-base's gradient bytes.  Sorted, disjoint."""
        if getattr(self, "_mirrored", None) is not None:
            return self._mirrored
        off, num, _ = self._layout
        P = self._cfg.channels * self._cfg.image_patch_size * (self._cfg.patch_width or self._cfg.image_patch_size) * self._cfg.frame_patch_size
        out = []
        for (name, _), o, n in zip(self.named_parameters(), off, num):
            if name.startswith("transformer.layers.") and name.endswith((".to_qkv.weight", ".to_out.0.weight", ".net.1.weight", ".net.4.weight")):
                out.append((o, o + n))
            elif name == "to_patch_embedding.2.weight" and P % 8 == 0:
                out.append((o, o + n))
        self._mirrored = sorted(out)          # the layout never changes for a constructed module
        return self._mirrored

    def _backward_into(self, dlogits, grads, accumulate, dvideo=None, attn_grad=None, of=None):
        sync = self._grad_sync
        if sync is None:
            self._rt.backward(dlogits, self._arena, self._shadow, grads, accumulate=accumulate, dvideo=dvideo, attn_grad=attn_grad, of=of)
            return
        from .parallel import bucket_stages
        sync.begin()
        last_stage = self._cfg.depth + 1
        # bf16 messages: the weight-gradient GEMMs write their share of the message buffer themselves (no cast pass over it)
        msg = sync.message_buffer(grads) if (grads.is_cuda and sync.world > 1) else None
        sync.mirrored = self.mirrored_ranges() if msg is not None else None
        plan = getattr(self, "_bucket_plan", None)
        if plan is None or plan[0] != sync.n_buckets:    # stage groups and their arena ranges: fixed per module, computed once
            groups = list(bucket_stages(self._cfg.depth + 2, sync.n_buckets))
            plan = self._bucket_plan = (sync.n_buckets, [(f, l) + tuple(self._rt.stage_range(f, l)) for f, l in groups])
        for first, last, begin, end in plan[1]:
            # intermediate buckets do not stall the main stream on the auxiliary (weight-gradient) stream: the bucket's
            # all-reduce is ordered after both streams instead
            self._rt.backward(dlogits, self._arena, self._shadow, grads, accumulate=accumulate, stages=(first, last),
                              join_aux=(last == last_stage), grads16=msg, dvideo=dvideo if last == last_stage else None,
                              attn_grad=attn_grad, of=of)   # (each call exports the layers inside its stage range)
            sync.bucket_ready(grads, begin, end, also_after=None if last == last_stage else self._rt.aux_stream_object(grads.device))
        sync.finish()

    def check_video(self, video, time_points=0, arena_checked=False):
        """Device, extents and arena placement of an input batch (raises as the reference's einops / pos_embedding add would)."""
        if not video.is_cuda:
            raise RuntimeError("neurovit_amd.ViT: input must live on the MI355X (cuda) device - there is no CPU fallback")
        c = self._cfg
        width = c.image_width or c.image_size
        if time_points:
            if video.dim() != 5 or tuple(video.shape[1:]) != (c.image_size, width, c.frames, time_points):
                raise ValueError(f"neurovit_amd.ViT: expected a 4D batch [B, {c.image_size}, {width}, {c.frames}, {time_points}], got {tuple(video.shape)}")
        elif video.dim() != 5 or tuple(video.shape[1:]) != (c.channels, c.frames, c.image_size, width):
            # the reference fails here too (einops Rearrange / the pos_embedding add, vit_3d.py:92,118); the gather kernel
            # takes its extents from the config, so a wrong-sized volume must never reach it
            raise ValueError(f"neurovit_amd.ViT: expected video [B, {c.channels}, {c.frames}, {c.image_size}, {width}] "
                             f"(channels, frames, height, width), got {tuple(video.shape)}")
        if not arena_checked:
            self.flat_parameters()
        if self._arena.device != video.device:
            raise RuntimeError(f"neurovit_amd.ViT: parameters on {self._arena.device}, input on {video.device}")

    def forward(self, video, vol_sigma=None, time_points=0):
        """video [B, C, F, H, W] -> [B, num_classes] (vit_3d.py:112-126).  Beyond the reference (both optional):
        vol_sigma [B] marks `video` as RAW volumes whose per-volume z-score (std + 1e-8) is folded into the patch LayerNorm;
        time_points = T > 0 takes a contiguous 4D batch [B, H, W, D, T] and encodes its B*T volumes without the regroup copy.

        Gradient w.r.t. the input: when `video` requires grad (and grad mode is on) the forward records a graph even if every
        parameter is frozen, and backward returns d loss / d video (x.grad, torch.autograd.grad, captum).  It is computed in the
        training arithmetic (16-bit operands: `operands`, bf16 or fp16; `eval_precision = "fp32"` does not apply to forwards that
        record a graph), dropout masks replay as for parameter gradients.  Parameter gradients follow requires_grad as before -
        torch.autograd.grad(out, video) on a trainable model still fills p.grad - so freeze the model for attribution: a model
        without trainable parameters runs the cheaper data-only backward and touches no p.grad.  Not available (NotImplementedError)
        with vol_sigma, time_points or the fp8 training forward."""
        need_grad = self._check_forward(video, vol_sigma, time_points)
        hooked = self._attend_hooked_layers()
        if not hooked:
            return _ViTFunction.apply(self, video.float(), need_grad, (vol_sigma, int(time_points)), *self._plist)
        return self._forward_export(video, vol_sigma, time_points, None, checked=(need_grad, hooked))[0]

    # ------------------------------------------------------------------ token-level objectives (masked reconstruction, distillation, patch contrast)
    def forward_tokens(self, video):
        """video [B, C, F, H, W] -> fp32 [B, n, dim]: the output of the last transformer block, cls token first - what the reference's
        `self.transformer(x)` returns (vit_3d.py:121), in front of pooling and mlp_head.  A VIEW of the pass's workspace (clone what must
        outlive the next forward of this module); the forward is the training one with the last block on every row, with this module's
        dropout in train mode.  Under autograd any torch loss on the tokens differentiates the native encoder: backward runs
        nv_vit_backward_tokens, parameter gradients land in .grad as after forward() - mlp_head takes no part and gets zeros - and a
        `video` that requires grad receives its gradient.  16-bit operand arithmetic (`operands`); not with the fp8 training forward,
        data parallel gradient buckets or backward hooks on `attend`."""
        self.check_video(video)
        self.refuse_drop_path("forward_tokens")
        if self._fp8 is not None and self.fp8_training:
            raise NotImplementedError("neurovit_amd.ViT: forward_tokens runs the 16-bit training forward - disable_fp8() or enable_fp8(training=False) first")
        need_grad = torch.is_grad_enabled() and (video.requires_grad or any(p.requires_grad for p in self._plist))
        if need_grad and self._attend_backward_hooked_layers():
            raise NotImplementedError("neurovit_amd.ViT: forward_tokens exports no attention gradients - remove the backward hooks on `attend`")
        return _ViTTokensFunction.apply(self, video.float(), need_grad, *self._plist)

    # ------------------------------------------------------------------ frozen features (kNN probe, feature export: neurovit_amd.features)
    @torch.no_grad()
    def forward_features(self, video, pool=None, normalize=False, out=None, row0=0, time_points=0):
        """video [B, C, F, H, W] -> fp32 [B, dim]: one embedding per volume, from the EVAL-mode forward of this model's `eval_precision`
        (whatever self.training says; no dropout, no stochastic depth), under no_grad - no graph is recorded and no .grad is touched, on a
        frozen or a trainable model.
          pool       None = the model's own pooling: the vector mlp_head reads (its cls row, or nv_token_mean's mean of a pool='mean' model) -
                     ops.head_fwd on it returns forward()'s logits bit for bit; "cls" | "mean" (all n rows) | "patch_mean" (the n - 1 patch
                     rows: MAE's global pool, the feature of a masked-pretrained model whose cls token no loss ever touched).  A pooling
                     that needs every row of the last block on a cls-pooled model runs that forward with rows_form=1.
          normalize  F.normalize's rule (nv_pool_features)
          out, row0  write rows row0 .. row0 + B of a preallocated fp32 [*, dim] bank instead of a fresh tensor; returns those rows
        Refused (NotImplementedError): the fused 4D input form (time_points), the fp8 forwards (enable_fp8 with a 16-bit eval_precision -
        disable_fp8() or precision("fp32")), and forward hooks on `attend` (they expect per-head attention maps this forward does not export)."""
        if time_points:
            raise NotImplementedError("neurovit_amd.ViT: forward_features takes [B, C, F, H, W] volumes, not the fused 4D input form (time_points) - "
                                      "pass the [B*T, C, F, H, W] volumes")
        if pool not in (None, "cls", "mean", "patch_mean"):
            raise ValueError(f"neurovit_amd.ViT: forward_features pool must be None, 'cls', 'mean' or 'patch_mean', got {pool!r}")
        self.check_video(video)
        if self.eval_precision not in ("bf16", "fp16", "fp32"):
            raise ValueError(f"neurovit_amd.ViT: eval_precision must be 'bf16', 'fp16' or 'fp32', got {self.eval_precision!r}")
        if self._fp8 is not None and self.eval_precision != "fp32":
            raise NotImplementedError("neurovit_amd.ViT: no features from the fp8 forwards (enable_fp8) - disable_fp8() first, or run under precision('fp32')")
        if self._attend_hooked_layers():
            raise NotImplementedError("neurovit_amd.ViT: forward_features exports no attention probabilities - remove the forward hooks on `attend` "
                                      "(they expect per-head maps)")
        mode = self.pool if pool is None else pool
        rows_form = 1 if mode != "cls" else None                 # every row of the last block, or this runtime's default form
        video = video.float()
        if self.eval_precision == "fp32":
            self._last_logits = self._rt.forward_f32(video, self._arena, rows_form=rows_form)
        else:
            self._refresh_shadow()
            if self.fold_layernorm:
                self._last_logits = self._rt.forward_lnfold(video, self._arena, self._shadow, self._fresh_fold(), rows_form=rows_form)
            else:
                self._last_logits = self._rt.forward(video, self._arena, self._shadow, training=False, rows_form=rows_form)
        return ops.pool_features(self._last_tokens(), mode, normalize, out=out, row0=row0)

    def _last_tokens(self) -> torch.Tensor:
        """fp32 [B, n, dim] view of the last block's output in the workspace of the most recent INFERENCE forward (valid until the next one).
        The inference layouts ping-pong a block's output between two buffers: an odd last block leaves it in x0."""
        last = self._rt.last
        n, d = self.pos_embedding.shape[1], self.pos_embedding.shape[2]
        L = self._cfg.depth
        if last.layout == 0 and (L - 1) & 1:
            return self._rt.tap("x0", -1, (last.B, n, d), torch.float32)
        return self._rt.tap("x2", L - 1, (last.B, n, d), torch.float32)

    def _run_forward_tokens(self, video):
        self._refresh_shadow()
        self._last_logits = self._rt.forward(video, self._arena, self._shadow, training=True, dropout=self.draw_dropout(), rows_form=1)
        B, (n, d) = video.shape[0], self.pos_embedding.shape[1:]
        return self._rt.tap("x2", self._cfg.depth - 1, (B, n, d), torch.float32)

    def _run_backward_tokens(self, rec, dtokens, dvideo=None):
        """The backward of pass `rec` from the gradient on its tokens; see _run_backward for where the parameter gradients go."""
        if self._grad_sync is not None:
            raise NotImplementedError("neurovit_amd.ViT: the token-level backward is not pipelined over data-parallel gradient buckets")
        if not any(p.requires_grad for p in self._plist):
            if dvideo is not None:
                self._rt.backward(None, self._arena, self._shadow, None, accumulate=False, dvideo=dvideo, weight_grads=False, of=rec, dtokens=dtokens)
            return

        def run(target, accumulate, scratch):
            self._rt.backward(None, self._arena, self._shadow, target, accumulate=accumulate and not scratch, dvideo=dvideo, of=rec, dtokens=dtokens)
        self._backward_to_grads(run)

    def _check_forward(self, video, vol_sigma, time_points) -> bool:
        """forward()'s argument checks; returns whether the forward records a graph"""
        self.check_video(video, time_points)
        input_grad = torch.is_grad_enabled() and video.requires_grad
        need_grad = input_grad or (torch.is_grad_enabled() and any(p.requires_grad for p in self._plist))
        for attn, _ in self.transformer.layers:
            _check_no_backward_pre_hooks(attn.attend, "neurovit_amd.ViT")
        if need_grad and self._attend_backward_hooked_layers():
            # (the hooks themselves are looked up when the backward runs; what that backward could not serve is refused up front)
            if self._fp8 is not None and self.fp8_training:
                raise NotImplementedError("neurovit_amd.ViT: no backward hooks on `attend` through the fp8 training forward - disable_fp8() or "
                                          "enable_fp8(training=False) first")
            if self.training and self._dropout_p[0] > 0:
                raise NotImplementedError("neurovit_amd.ViT: backward hooks on `attend` with attention dropout active (train mode, dropout > 0) - "
                                          "the mask is not replayed into the gradient of the probabilities; run the attribution in eval mode")
        if input_grad:
            if vol_sigma is not None:
                raise NotImplementedError("neurovit_amd.ViT: no gradient w.r.t. RAW volumes (vol_sigma / forward_raw): the folded z-score treats "
                                          "sigma as a constant - normalise the volume first and differentiate w.r.t. that")
            if time_points:
                raise NotImplementedError("neurovit_amd.ViT: no input gradient through the fused 4D input form (time_points) - pass the "
                                          "[B*T, C, F, H, W] volumes instead")
            if self._fp8 is not None and self.fp8_training:
                raise NotImplementedError("neurovit_amd.ViT: no input gradient through the fp8 training forward - disable_fp8() or "
                                          "enable_fp8(training=False) first")
        if time_points and need_grad:
            raise NotImplementedError("neurovit_amd.ViT: the fused 4D input form is forward-only (frozen encoder of the 4D model)")
        return need_grad

    def _forward_export(self, video, vol_sigma, time_points, request, checked=None):
        """forward() with an attention-probability export: `request` = (layers, head_fusion, rows) of attention_maps or None; the layers
        with `attend` hooks are exported per head with every row and their hooks fire once the forward has been queued.
        Returns (logits, {layer: map} of the request)."""
        need_grad, hooked = checked if checked is not None else (self._check_forward(video, vol_sigma, time_points), self._attend_hooked_layers())
        if self._uses_fp8(need_grad):
            raise NotImplementedError("neurovit_amd.ViT: no attention probabilities from the fp8 forwards (enable_fp8) - disable_fp8() first")
        layers, fusion, rows = request if request is not None else ([], None, "all")
        if hooked and request is not None and (fusion is not None or rows != "all"):
            raise RuntimeError("neurovit_amd.ViT: forward hooks on `attend` receive per-head maps of every row - remove them, or ask "
                               "attention_maps for head_fusion=None, rows='all'")
        B = video.shape[0] * (int(time_points) or 1)
        export, maps = self._rt.make_attn_export(B, sorted(set(layers) | set(hooked)), fusion, rows, video.device)
        logits = _ViTFunction.apply(self, video.float(), need_grad, (vol_sigma, int(time_points), export), *self._plist)
        if hooked:
            self._fire_attend_hooks({l: maps[l] for l in hooked})
        return logits, {l: maps[l] for l in layers}

    # activations / gradients of the last block's attention LayerNorm output (Grad-CAM contract, NeuroEncoder.py:70-82)
    def last_attn_norm_output_raw(self) -> torch.Tensor:
        """[B, n, d] view into the workspace of the most recent forward (no copy): the operand format, or fp32 after an fp32 inference forward."""
        last = self._rt.last
        n, d = self.pos_embedding.shape[1], self.pos_embedding.shape[2]
        return self._rt.tap("xn1", self._cfg.depth - 1, (last.B, n, d), torch.float32 if last.layout == 2 else self._dtype16())

    def last_attn_norm_grad_raw(self) -> torch.Tensor:
        """fp32 [B, n, d] view into the workspace; valid once a backward of the most recent training forward has run."""
        last = self._rt.last
        if last is None or not last.grad_ready:
            raise RuntimeError("neurovit_amd.ViT: no backward pass has run for the most recent forward - the hook gradient is not available")
        n, d = self.pos_embedding.shape[1], self.pos_embedding.shape[2]
        return self._rt.tap("hookg", -1, (last.B, n, d), torch.float32)

    def last_attn_norm_output(self) -> torch.Tensor:
        return self.last_attn_norm_output_raw().float()

    def last_attn_norm_grad(self) -> torch.Tensor:
        return self.last_attn_norm_grad_raw().clone()
