"""The flat parameter arena that `vit_3d.ViT` and `temporal.TemporalHead` share.

Every nn.Parameter of a holder is a view of ONE contiguous fp32 tensor (`_arena`), every `.grad` a view of a second one
(`_grads`): the native kernels take two pointers instead of a parameter list, the fused AdamW steps a holder in one launch, and a
data-parallel all-reduce sends one message.  `FlatArena` is a base class, mixed into an nn.Module (ViT) or a plain object
(TemporalHead).  A holder defines `_build_arena()`, which hands its parameters and their layout to `_pack`, and `_packed()`, which
`_pack` calls last for what only that holder has.
"""
from __future__ import annotations

from typing import Callable, Iterable, List, Optional

import torch
from torch import nn


class FlatArena:
    operands = "bf16"          # operand format the process is set to before this holder's AdamW launch (what a 16-bit shadow holds)
    _phantom = ()              # [(offset, fp32 constant)]: arena slots that are no parameter (only a ViT without out-projection has any)
    _shadow = None             # 16-bit copy of the arena that the MFMA kernels read (only a ViT has one: the head computes in fp32)
    _direct_when_partly_frozen = True      # see _backward_to_grads

    def _init_arena(self):
        self._arena: Optional[torch.Tensor] = None      # flat fp32 master parameters
        self._grads: Optional[torch.Tensor] = None      # flat fp32 gradients (param.grad are views), allocated on first use
        self._plist: List[nn.Parameter] = []
        self._offsets: List[int] = []
        self._numels: List[int] = []
        self._param_generation = 0 # moves whenever the arena is rewritten through raw pointers (no tensor `_version` does then)

    # ------------------------------------------------------------------ packing and validating
    def _pack(self, plist, offsets, numels, total):
        """(Re)pack `plist` into one zeroed fp32 arena of `total` elements on the parameters' current device and make every
        nn.Parameter a view of it.  The gradient arena survives only on the same device."""
        dev = plist[0].device
        arena = torch.zeros(total, dtype=torch.float32, device=dev)
        with torch.no_grad():
            for p, o, n in zip(plist, offsets, numels):
                arena[o:o + n].copy_(p.detach().reshape(-1).float())
                p.data = arena[o:o + n].view(p.shape)
        if self._grads is not None and self._grads.device != dev:
            self._grads = None
        self._arena, self._plist, self._offsets, self._numels = arena, plist, offsets, numels
        self._packed()

    def _arena_ok(self) -> bool:
        if self._arena is None:
            return False
        base = self._arena.data_ptr()
        for p, o in zip(self._plist, self._offsets):
            if p.data_ptr() != base + 4 * o:
                return False
        return True

    def flat_parameters(self):
        """(arena fp32, 16-bit shadow or None) - the interface of the fused optimizer and the DP gradient all-reduce.  Packs lazily:
        after construction, after .to(device), after foreign code replaced a parameter's storage."""
        if not self._arena_ok():
            self._build_arena()
        return self._arena, self._shadow

    def arena_parameters(self) -> List[nn.Parameter]:
        """the parameters that are views of the (validated) arena, in arena order"""
        self.flat_parameters()
        return self._plist

    def gradient_arena(self) -> torch.Tensor:
        """the gradient arena, allocated on first use, WITHOUT validating the parameter arena (for a caller that just has)"""
        if self._grads is None:
            self._grads = torch.zeros_like(self._arena)
        return self._grads

    def flat_gradients(self) -> torch.Tensor:
        self.flat_parameters()
        return self.gradient_arena()

    def bump_generation(self):
        """the arena changed under derived copies (they key on `_param_generation`); nothing else moves"""
        self._param_generation += 1

    # ------------------------------------------------------------------ .grad as views of the gradient arena
    def _view_of(self, flat: torch.Tensor, i: int) -> torch.Tensor:
        o = self._offsets[i]
        return flat[o:o + self._numels[i]].view(self._plist[i].shape)

    def _grad_view(self, i: int) -> torch.Tensor:
        return self._view_of(self._grads, i)

    def install_grad_views(self, entries: Optional[Iterable[int]] = None):
        """.grad of `entries` (default: every parameter) = its view of the (allocated) gradient arena; valid while that arena lives"""
        for i in range(len(self._plist)) if entries is None else entries:
            self._plist[i].grad = self._grad_view(i)

    def ensure_grad_views(self):
        """install the views unless they are there: the arena paths set or clear every .grad together, so the first stands for all"""
        if self._plist[0].grad is None:
            self.install_grad_views()

    def grads_are_views(self, entries: Optional[Iterable[int]] = None) -> bool:
        """.grad of each of `entries` (default: every parameter) is set and is its view of the gradient arena"""
        if self._grads is None:
            return False
        for i in range(len(self._plist)) if entries is None else entries:
            g = self._plist[i].grad
            if g is None or g.data_ptr() != self._grad_view(i).data_ptr():
                return False
        return True

    def no_gradients(self) -> bool:
        """torch.optim.AdamW skips a parameter whose .grad is None (no weight decay, no moment decay, no step count): an arena none of
        whose parameters has a gradient - zero_grad(set_to_none=True) followed by step(), or a head no backward reached - is skipped
        as a whole by the fused step.  (A PARTIALLY populated arena is stepped with zeros for the missing gradients: gather_foreign_grads.)"""
        return all(p.grad is None for p in self._plist)

    def gather_foreign_grads(self):
        """Before a fused optimizer step: gradients that autograd produced outside the arena (the stock-module path of
        NeuroEncoder.forward) are moved into it; a parameter without a gradient contributes zeros - the fused step runs over the
        whole arena, so such a parameter still sees weight decay and moment decay where torch.optim.AdamW would skip it.  The
        optimizer skips the arena altogether when NO parameter has a gradient (`no_gradients`: the case torch skips entirely); a
        partially used head does not occur on the NeuroEncoder path (every parameter is on the forward path)."""
        grads = self.flat_gradients()
        for i, p in enumerate(self._plist):
            view = self._grad_view(i)
            if p.grad is None:
                view.zero_()
            elif p.grad.data_ptr() != view.data_ptr():
                view.copy_(p.grad)
                p.grad = view
        return grads

    def _backward_to_grads(self, run: Callable):
        """Where a backward pass puts its parameter gradients.  `run(target, accumulate, scratch)` computes them into the flat
        `target` (adding with `accumulate`) and its result is returned; `scratch`: `target` is a throw-away arena, not `_grads`.
          no trainable parameter has a .grad   -> the gradient arena is written and the views are installed
          every such .grad is its arena view   -> the gradient arena is accumulated into
          anything else (foreign .grad tensors) -> a scratch arena is written, then cloned from / added per parameter.
        A holder with `_direct_when_partly_frozen = False` also takes the third way whenever one of its parameters is frozen."""
        grads = self.flat_gradients()
        plist = self._plist
        trainable = [i for i, p in enumerate(plist) if p.requires_grad]
        direct = self._direct_when_partly_frozen or len(trainable) == len(plist)
        if direct and all(plist[i].grad is None for i in trainable):
            out = run(grads, False, False)
            self.install_grad_views(trainable)
        elif direct and self.grads_are_views(trainable):
            out = run(grads, True, False)
        else:
            scratch = torch.empty_like(grads)
            out = run(scratch, False, True)
            for i in trainable:
                p, g = plist[i], self._view_of(scratch, i)
                p.grad = g.clone() if p.grad is None else p.grad.add_(g)
        return out
