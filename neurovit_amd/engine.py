"""Python side of the native encoder engine (csrc/engine.hip): flat parameter arenas + workspace.

Memory design (MI355X-first, 288 GB HBM per GPU): all parameters of a ViT live in ONE contiguous fp32
arena (master weights), mirrored by a bf16 shadow arena of identical element offsets that the MFMA
kernels read, plus one gradient arena and (optimizer) m / v arenas.  nn.Parameters are VIEWS into the
arena, so the fused AdamW kernel, the bf16 refresh and the data-parallel gradient all-reduce all work
on a few large contiguous ranges instead of ~150 small tensors.
"""
from __future__ import annotations

import ctypes
import os
import weakref
from typing import Dict, List, Optional, Tuple

import torch

from . import _cabi, ops
from ._cabi import AttnExport, AttnGradExport, BackwardOpts, DropPath, TrainHparams, VitConfig, VitInput, check, lib

_BYTES = {torch.float32: 4, torch.bfloat16: 2, torch.float16: 2}


def make_config(*, image_size, image_patch_size, frames, frame_patch_size, num_classes, dim, depth, heads, mlp_dim,
                channels=3, dim_head=64, ln_eps=1e-5, pool='cls', image_width=0, patch_width=0, **_) -> VitConfig:
    """image_size / image_patch_size are the image / patch HEIGHT; image_width / patch_width (0 = same) the widths (vit_3d.py:80-81)."""
    if pool not in ('cls', 'mean'):
        raise ValueError("pool type must be either cls (cls token) or mean (mean pooling)")
    return VitConfig(image_size, image_patch_size, frames, frame_patch_size, channels, num_classes, dim, depth, heads,
                     dim_head, mlp_dim, ln_eps, int(pool == 'mean'), 0 if image_width == image_size else image_width,
                     0 if patch_width == image_patch_size else patch_width, int(heads == 1 and dim_head == dim))


def image_hw(cfg: VitConfig):
    """(image height, image width, patch height, patch width)"""
    return cfg.image_size, cfg.image_width or cfg.image_size, cfg.image_patch_size, cfg.patch_width or cfg.image_patch_size


def param_layout(cfg: VitConfig) -> Tuple[List[int], List[int], int]:
    """(offsets, numels, total) of the arena, in the reference's ViT.state_dict() order."""
    total = lib.nv_vit_param_count(ctypes.byref(cfg))
    if total < 0:
        check(-1, "nv_vit_param_count")
    cap = 8 + 11 * cfg.depth + 4 + 8
    off = (ctypes.c_long * cap)()
    num = (ctypes.c_long * cap)()
    cnt = lib.nv_vit_param_table(ctypes.byref(cfg), off, num, cap)
    if cnt < 0:
        check(cnt, "nv_vit_param_table")
    return list(off[:cnt]), list(num[:cnt]), int(total)


def flops_forward(cfg: VitConfig) -> float:
    """Algorithmic FLOPs per volume of one ViT forward (2 x MAC of the patch embedding, the four linears and the two
    attention products of every block, and the head; LayerNorm / softmax / GELU / bias excluded) - SURVEY.md 8(d).
    A train step counts 3 x this (backward = 2 x forward)."""
    H, Wd, p1, p2 = image_hw(cfg)
    N = (cfg.frames // cfg.frame_patch_size) * (H // p1) * (Wd // p2)
    n = N + 1
    P = cfg.channels * p1 * p2 * cfg.frame_patch_size
    d, inner, m = cfg.dim, cfg.heads * cfg.dim_head, cfg.mlp_dim
    per_layer = 2 * n * d * 3 * inner + 2 * n * n * inner + 2 * n * n * inner + 2 * n * inner * d + 4 * n * d * m
    return 2.0 * N * P * d + cfg.depth * per_layer + 2 * d * cfg.num_classes


def _inp_ptr(inp):
    """the optional nv_vit_input argument of the forwards and the train step (`inp` must outlive the call)"""
    return None if inp is None else ctypes.cast(ctypes.pointer(inp), ctypes.c_void_p)


def _drop(dropout):
    """(p of the blocks, p of the embedding, seed) as the C arguments"""
    return float(dropout[0]), float(dropout[1]), int(dropout[2])


class _Pass:
    """One forward and what a backward of it, or a tap into its workspace, needs: batch, layout (0 inference, 1 training, 2 fp32), workspace,
    input (the backward re-gathers the patches), input form `keep` = (vol_sigma, nv_vit_input), form of the last block, dropout draw,
    stochastic-depth table `drop_path` (device fp32 [depth, 2, B], or None: the backward of the pass must be given the same factors).
    `done`: a whole backward has run - the workspace may be refilled.  `grad_ready`: a backward has left the hook gradient in the workspace."""
    __slots__ = ("B", "layout", "ws", "video", "keep", "rows_form", "dropout", "drop_path", "dlogits", "dtokens", "done", "grad_ready", "_claim", "__weakref__")

    class _Claim:
        __slots__ = ("__weakref__",)

    def __init__(self, B, layout, ws, video, keep=(None, None), rows_form=0, dropout=(0.0, 0.0, 0), done=False, drop_path=None):
        self.B, self.layout, self.ws, self.video, self.keep, self.rows_form, self.dropout = B, int(layout), ws, video, keep, rows_form, dropout
        self.drop_path = drop_path
        self.dlogits, self.dtokens, self.done, self.grad_ready, self._claim = None, None, done, done, None

    def claim(self):
        """A token for whoever needs this pass's activations later (an autograd node keeps it on its ctx): the pass is held while it is alive."""
        token = _Pass._Claim()
        self._claim = weakref.ref(token)
        return token

    def finish(self) -> None:
        """nothing more of this pass will run: the workspace may be refilled by the next training forward, the hook gradient is in it"""
        self.done = self.grad_ready = True

    @property
    def held(self) -> bool:
        return self._claim is not None and self._claim() is not None


class PassLedger:
    """Which forward filled which workspace, and may it be overwritten.  Workspaces are cached per (B, layout, device); the training
    layout hands them out per pass: a pass that is claimed and whose backward has not run keeps its workspace, and the next training
    forward takes another one - as many live sets of activations as the caller's graph holds, the reference's autograd semantics
    (siamese / two-forward losses); the usual forward-backward loop never needs a second.  `nbytes(B, layout)` sizes a workspace."""

    def __init__(self, nbytes):
        self._nbytes = nbytes
        self._ws: Dict[Tuple[int, int, str], List[torch.Tensor]] = {}   # [primary, further training workspaces for overlapping passes ...]
        self._holder = {}   # workspace address -> weakref of the _Pass that filled it last
        self.last: Optional[_Pass] = None      # the most recent forward of any layout (taps, Grad-CAM)
        self.current: Optional[_Pass] = None   # the most recent training-layout pass: what a backward() that names none runs against

    def _workspaces(self, B: int, layout, device, more: bool = False) -> List[torch.Tensor]:
        sets = self._ws.setdefault((B, int(layout), str(device)), [])
        if more or not sets:
            nbytes = self._nbytes(B, int(layout))
            ws = torch.empty(nbytes + 256, dtype=torch.uint8, device=device)
            pad = (-ws.data_ptr()) % 256
            sets.append(ws[pad:pad + nbytes])
        return sets

    def workspace(self, B: int, training, device) -> torch.Tensor:
        """The primary workspace.  training: False / True, or 2 for the fp32 inference layout."""
        return self._workspaces(B, training, device)[0]

    def extra_workspaces(self, B: int, device) -> int:
        """how many training workspaces beyond the primary one overlapping passes have needed so far"""
        return max(len(self._ws.get((B, 1, str(device)), ())) - 1, 0)

    def acquire(self, B: int, layout, device) -> torch.Tensor:
        """The workspace of the next forward: the primary one, or in the training layout the first whose last pass is gone, done or not held."""
        if int(layout) != 1:
            return self.workspace(B, layout, device)
        for ws in self._workspaces(B, 1, device):
            ref = self._holder.get(ws.data_ptr())
            rec = ref() if ref is not None else None
            if rec is None or rec.done or not rec.held:
                return ws
        return self._workspaces(B, 1, device, more=True)[-1]

    def open(self, rec: _Pass) -> _Pass:
        """`rec` has just filled its workspace (whatever pass filled it before is stale now): it is the last pass, and the current one if it can be differentiated"""
        self._holder[rec.ws.data_ptr()] = weakref.ref(rec)
        self.last = rec
        if rec.layout == 1:
            self.current = rec
        return rec

    def pass_is_live(self, rec: _Pass) -> bool:
        """the workspace still holds THIS pass's activations (no later forward or train step has refilled it)"""
        ref = self._holder.get(rec.ws.data_ptr())
        return ref is not None and ref() is rec

    def backward_pass(self, of: Optional[_Pass] = None) -> _Pass:
        """the pass a backward runs against: `of`, or the most recent training pass - whose activations must still be in its workspace"""
        rec = self.current if of is None else of
        assert rec is not None, "backward needs a preceding forward(training=True)"
        if not self.pass_is_live(rec):
            raise RuntimeError("neurovit_amd: backward() of a forward pass whose activations have been overwritten - a later forward or train step "
                               "has refilled its workspace (a pass keeps its workspace only until a whole backward of it has run)")
        return rec

    def note_step_replayed(self, rec: _Pass) -> _Pass:
        """A captured train step (trainer.py) has been replayed: the workspace of the pass its capture opened holds ITS activations and gradient taps again."""
        return self.open(rec)


class VitRuntime(PassLedger):
    """Executes ViT forward / backward through the native engine on caller-provided arenas; its PassLedger keeps the passes' workspaces."""

    def __init__(self, cfg: VitConfig):
        super().__init__(self._workspace_bytes)
        self.cfg = cfg
        self._aux = {}      # device -> auxiliary stream for the weight-gradient GEMMs
        self.use_aux_stream = os.environ.get("NEUROVIT_AUX_STREAM", "1") != "0"
        # last block under pool='cls': 0 = the library's process default (cls rows), 1 = every row (A/B runs, debugging)
        self.rows_form = 1 if os.environ.get("NEUROVIT_CLS_TAIL") == "0" else 0
        self.operands = "bf16"       # 16-bit operand format of this runtime's calls (ViT.set_operands); set in the library before each of them

    def _workspace_bytes(self, B: int, layout: int) -> int:
        nbytes = lib.nv_vit_workspace_bytes(ctypes.byref(self.cfg), B, layout)
        if nbytes < 0:
            check(-1, "nv_vit_workspace_bytes")
        return nbytes

    def _forward(self, entry: str, video, layout, weights, mid=(), after=(), *, vol_sigma=None, time_points: int = 0, rows_form=None,
                 attn_export=None, dropout=(0.0, 0.0, 0), operands: bool = True, step: bool = False, drop_path=None,
                 path_arg: bool = False):
        """What every forward shares: checks, input form, workspace and logits, the C call
        `entry`(cfg, B, video, shape, strides, input, *weights, workspace, bytes, *mid, logits, *after, stream[, aux stream][, drop path]), the pass record.
        drop_path: the stochastic-depth table of an *_sd entry (checked here), kept with the pass for its backward.
        path_arg: the entry takes the drop-path argument even without a table (NULL then).
        step: the one-call train step - the primary training workspace (a pending pass in it goes stale), the auxiliary stream, a done pass.
        Returns (pass, logits)."""
        rows_form = self.rows_form if rows_form is None else int(rows_form)
        if operands:
            _cabi.set_operand_format(self.operands)
        B, inp = self._input_form(video, vol_sigma, time_points, rows_form, attn_export)
        dev = video.device
        sd = self._path_struct(drop_path, B, dev)
        ws = self.workspace(B, True, dev) if step else self.acquire(B, layout, dev)
        logits = torch.empty((B, self.cfg.num_classes), dtype=torch.float32, device=dev)
        check(getattr(lib, entry)(ctypes.byref(self.cfg), B, video.data_ptr(), ops.shape5(video), ops.strides5(video), _inp_ptr(inp), *weights,
                                  ws.data_ptr(), ws.numel(), *mid, logits.data_ptr(), *after, torch.cuda.current_stream().cuda_stream,
                                  *((self._aux_stream(dev),) if step else ()), *((ctypes.byref(sd),) if sd is not None else ((None,) if path_arg else ()))), entry)
        # a backward re-gathers the same (raw) input and takes the same form of the last block - and the same stochastic-depth factors
        return self.open(_Pass(B, layout, ws, video, (vol_sigma, inp), rows_form, dropout, done=step, drop_path=drop_path)), logits

    def _path_struct(self, drop_path, B: int, device) -> Optional[DropPath]:
        """nv_vit_drop_path of a stochastic-depth table (None: none) after checking it: contiguous fp32 [depth, 2, B] on the input's device.
        The struct holds a raw pointer: the table is kept alive by the pass record."""
        if drop_path is None:
            return None
        want = (self.cfg.depth, 2, B)
        if not (torch.is_tensor(drop_path) and drop_path.is_cuda and drop_path.device == device and drop_path.dtype == torch.float32
                and tuple(drop_path.shape) == want and drop_path.is_contiguous()):
            raise ValueError(f"neurovit_amd: drop_path must be a contiguous fp32 device tensor [depth, 2, B] = {list(want)} on {device}, got "
                             f"{tuple(drop_path.shape) if torch.is_tensor(drop_path) else type(drop_path).__name__}")
        return DropPath(ctypes.sizeof(DropPath), drop_path.data_ptr())

    def _input_form(self, video: torch.Tensor, vol_sigma, time_points: int, rows_form: int = 0, attn_export: Optional[AttnExport] = None):
        """(B, nv_vit_input or None) after checking the extents: plain [B, C, F, H, W] view, or (time_points > 0) a contiguous
        4D batch [B / T, H, W, D, T]; vol_sigma marks RAW volumes (z-score folded into the patch LayerNorm).
        attn_export (make_attn_export): the attention probabilities this forward writes behind each attention launch."""
        if not video.is_cuda:
            raise RuntimeError("neurovit_amd: ViT forward needs a CUDA/HIP tensor on MI355X - there is no CPU fallback")
        assert video.dtype == torch.float32 and video.dim() == 5
        c = self.cfg
        if time_points:
            want = (c.image_size, c.image_width or c.image_size, c.frames, time_points)
            if tuple(video.shape[1:]) != want or not video.is_contiguous() or time_points % 4 or c.channels != 1:
                raise ValueError(f"neurovit_amd: 4D batch of shape {tuple(video.shape)} (contiguous: {video.is_contiguous()}) does not match "
                                 f"[B, H, W, D, T] = [B, {', '.join(map(str, want))}] with T % 4 == 0")
            B = video.shape[0] * time_points
        else:
            want = (c.channels, c.frames, c.image_size, c.image_width or c.image_size)
            if tuple(video.shape[1:]) != want:
                raise ValueError(f"neurovit_amd: video of shape {tuple(video.shape)} does not match the model's "
                                 f"[B, channels, frames, height, width] = [B, {', '.join(map(str, want))}]")
            B = video.shape[0]
        if vol_sigma is None and not time_points and not rows_form and attn_export is None:
            return B, None
        if vol_sigma is not None:
            assert vol_sigma.is_cuda and vol_sigma.dtype == torch.float32 and vol_sigma.numel() == video.shape[0] and vol_sigma.is_contiguous()
        return B, VitInput(None if vol_sigma is None else vol_sigma.data_ptr(), int(time_points), int(rows_form),
                           None if attn_export is None else ctypes.cast(ctypes.pointer(attn_export), ctypes.c_void_p))

    def make_attn_export(self, B: int, layers, head_fusion: Optional[str], rows: str, device):
        """(nv_vit_attn_export, {layer: fp32 map}) for a forward of B volumes: per head [B, heads, R, n] or head-fused [B, R, n],
        R = n (rows "all") or 1 (rows "cls").  The struct holds raw pointers: keep the maps (and the struct) alive across the call."""
        c = self.cfg
        H, Wd, p1, p2 = image_hw(c)
        n = (c.frames // c.frame_patch_size) * (H // p1) * (Wd // p2) + 1
        R = 1 if rows == "cls" else n
        shape = (B, c.heads, R, n) if head_fusion is None else (B, R, n)
        maps = {int(l): torch.empty(shape, dtype=torch.float32, device=device) for l in layers}
        ptrs = (ctypes.c_void_p * c.depth)(*[maps[l].data_ptr() if l in maps else None for l in range(c.depth)])
        ex = AttnExport(ctypes.sizeof(AttnExport), ctypes.cast(ptrs, ctypes.c_void_p), _cabi.ATTN_FUSIONS[head_fusion], _cabi.ATTN_ROWS[rows])
        ex._ptrs = ptrs                                   # the host pointer array lives as long as the struct
        return ex, maps

    def make_attn_grad_export(self, B: int, layers, form: str, device):
        """(nv_vit_attn_grad_export, {layer: fp32 map}) for a backward of B volumes: form "per_head" [B, heads, n, n] = the gradient
        w.r.t. the output of the block's `attend`, or "relevance" [B, n, n] = mean_h relu(dP_h * P_h).  The struct holds raw pointers:
        keep the maps (and the struct) alive across the call."""
        c = self.cfg
        H, Wd, p1, p2 = image_hw(c)
        n = (c.frames // c.frame_patch_size) * (H // p1) * (Wd // p2) + 1
        shape = (B, c.heads, n, n) if form == "per_head" else (B, n, n)
        maps = {int(l): torch.empty(shape, dtype=torch.float32, device=device) for l in layers}
        ptrs = (ctypes.c_void_p * c.depth)(*[maps[l].data_ptr() if l in maps else None for l in range(c.depth)])
        ex = AttnGradExport(ctypes.sizeof(AttnGradExport), ctypes.cast(ptrs, ctypes.c_void_p), _cabi.ATTN_GRAD_FORMS[form])
        ex._ptrs = ptrs                                   # the host pointer array lives as long as the struct
        return ex, maps

    def forward(self, video: torch.Tensor, params: torch.Tensor, params16: torch.Tensor, training: bool,
                dropout: Tuple[float, float, int] = (0.0, 0.0, 0), vol_sigma=None, time_points: int = 0, rows_form: Optional[int] = None,
                attn_export: Optional[AttnExport] = None, drop_path: Optional[torch.Tensor] = None) -> torch.Tensor:
        """video: [B, C, F, H, W] fp32 view (any strides).  Returns logits [B, num_classes] fp32.
        drop_path: None, or the stochastic-depth factors of this forward, fp32 [depth, 2, B] on the device (0 or 1 / (1 - q) per block,
        branch and sample; ops.drop_path_draw) - training forwards only, not the fused 4D form (nv_vit_forward_sd).  The pass keeps the
        table: backward() hands the same factors to the engine.
        dropout = (p of the blocks, p of the embedding, seed) - (0, 0, *) in eval mode.
        vol_sigma / time_points: the optional input forms of nv_vit_forward_in (raw volumes; contiguous 4D batch).
        rows_form: 1 = the last block on every row (as the reference computes it), 2 = on the cls rows when eligible,
        None = this runtime's default (`self.rows_form`: the process default unless NEUROVIT_CLS_TAIL=0)."""
        if drop_path is not None and (not training or time_points):
            raise ValueError("neurovit_amd: drop_path belongs to training forwards (training=True) of the plain input form (no time_points)")
        return self._forward("nv_vit_forward_in" if drop_path is None else "nv_vit_forward_sd", video, training, (params.data_ptr(), params16.data_ptr()),
                             (int(training),) + _drop(dropout), vol_sigma=vol_sigma, time_points=time_points, rows_form=rows_form, attn_export=attn_export,
                             dropout=dropout, drop_path=drop_path)[1]

    # ------------------------------------------------------------------ inference forward with the LayerNorms folded into the GEMMs around them
    def lnfold_prepare(self, params: torch.Tensor, reuse=None):
        """W_qkv diag(gamma1) / W_1 diag(gamma2) of every block in the operand format (an arena with the parameter arena's element offsets), their
        column sums and the folded biases (nv_vit_lnfold_prepare).  reuse: a dict this function returned earlier - overwritten in place."""
        _cabi.set_operand_format(self.operands)
        n32 = lib.nv_vit_lnfold_floats(ctypes.byref(self.cfg))
        if n32 < 0:
            check(-1, "nv_vit_lnfold_floats")
        dt = torch.float16 if self.operands == "fp16" else torch.bfloat16
        if reuse is not None and reuse["fold16"].numel() == params.numel() and reuse["fold16"].dtype == dt and reuse["fold16"].device == params.device:
            f16, f32 = reuse["fold16"], reuse["fold32"]
        else:
            f16 = torch.zeros(params.numel(), dtype=dt, device=params.device)
            f32 = torch.empty(n32, dtype=torch.float32, device=params.device)
        check(lib.nv_vit_lnfold_prepare(ctypes.byref(self.cfg), params.data_ptr(), f16.data_ptr(), f32.data_ptr(), torch.cuda.current_stream().cuda_stream),
              "nv_vit_lnfold_prepare")
        return dict(fold16=f16, fold32=f32)

    def forward_lnfold(self, video: torch.Tensor, params: torch.Tensor, params16: torch.Tensor, fold, vol_sigma=None, time_points: int = 0,
                       rows_form: Optional[int] = None, attn_export: Optional[AttnExport] = None) -> torch.Tensor:
        """Inference forward (no dropout) whose blocks run without LayerNorm launches: nv_vit_forward_lnfold."""
        return self._forward("nv_vit_forward_lnfold", video, 0, (params.data_ptr(), params16.data_ptr(), fold["fold16"].data_ptr(), fold["fold32"].data_ptr()),
                             vol_sigma=vol_sigma, time_points=time_points, rows_form=rows_form, attn_export=attn_export)[1]

    # ------------------------------------------------------------------ fp32 inference (the reference's fp32 validate, Trainer.py:101-118)
    def forward_f32(self, video: torch.Tensor, params: torch.Tensor, vol_sigma=None, time_points: int = 0,
                    attn_export: Optional[AttnExport] = None, rows_form: Optional[int] = None) -> torch.Tensor:
        """Inference forward with every operand in fp32 (weights straight from the fp32 arena, contractions on the fp32 MFMA):
        logits within 1e-5 of the reference's CPU fp32 forward instead of the bf16 path's 1e-3 ... 7e-3.  Eval mode only."""
        return self._forward("nv_vit_forward_f32", video, 2, (params.data_ptr(),), vol_sigma=vol_sigma, time_points=time_points, rows_form=rows_form,
                             attn_export=attn_export, operands=False)[1]     # (no 16-bit operand anywhere: the format is left as it is)

    # ------------------------------------------------------------------ fp8 inference (BASELINE.json configs[4])
    def calibrate_fp8(self, video: torch.Tensor, params: torch.Tensor, params16: torch.Tensor, headroom: float = 2.0, out_proj: bool = True):
        """One bf16 forward of `video` with every layer's activations kept; returns the per-layer activation scales
        [depth][4] = 448 / (headroom * amax) of the LN1 output, the LN2 output, the GELU output and the attention output.  e4m3 is a floating
        format: headroom costs no relative precision, it only moves the subnormal floor."""
        self.forward(video, params, params16, training=True, rows_form=1)    # the fp8 forward quantises every row of every block: calibrate on every row
        B = video.shape[0]
        H, Wd, p1, p2 = image_hw(self.cfg)
        n = (self.cfg.frames // self.cfg.frame_patch_size) * (H // p1) * (Wd // p2) + 1
        scales = []
        for l in range(self.cfg.depth):
            row = []
            for name, width in (("xn1", self.cfg.dim), ("xn2", self.cfg.dim), ("h", self.cfg.mlp_dim), ("ao", self.cfg.heads * self.cfg.dim_head)):
                amax = float(self.tap(name, l, (B * n, width), torch.bfloat16).abs().max())     # calibration only: off the hot path
                row.append(448.0 / (headroom * max(amax, 1e-6)))
            if not out_proj:
                row[3] = 0.0          # the out-projection stays on bf16 operands (measured: fp8 there buys 1-2 % and adds ~15 % to the logits' error)
            scales.append(row)
        return scales

    def quantize_fp8(self, params: torch.Tensor, act_scales, reuse=None):
        """fp8 weight arena (bytes at the parameter arena's element offsets) + column scales for the given activation scales.
        reuse: a dict this function returned earlier - its device buffers are overwritten in place (the per-step re-quantisation of
        an fp8 training run must not allocate and clear a parameter-sized arena every step)."""
        cnt = lib.nv_vit_fp8_scale_count(ctypes.byref(self.cfg))
        if cnt < 0:
            check(-1, "nv_vit_fp8_scale_count")
        flat = [float(v) for row in act_scales for v in row]
        host = (ctypes.c_float * len(flat))(*flat)
        if reuse is not None and reuse["params8"].numel() == params.numel() and reuse["params8"].device == params.device:
            p8, cs = reuse["params8"], reuse["colscales"]
        else:
            p8 = torch.zeros(params.numel(), dtype=torch.uint8, device=params.device)
            cs = torch.empty(cnt, dtype=torch.float32, device=params.device)
        check(lib.nv_vit_quantize_fp8(ctypes.byref(self.cfg), params.data_ptr(), ctypes.cast(host, ctypes.c_void_p), p8.data_ptr(), cs.data_ptr(),
                                      torch.cuda.current_stream().cuda_stream), "nv_vit_quantize_fp8")
        return dict(params8=p8, colscales=cs, act_scales=host, act_list=act_scales)

    def forward_fp8_train(self, video: torch.Tensor, params: torch.Tensor, params16: torch.Tensor, f8, dropout: Tuple[float, float, int] = (0.0, 0.0, 0),
                          vol_sigma=None, rows_form: Optional[int] = None) -> torch.Tensor:
        """TRAINING forward with qkv / FC1 / FC2 of every block on e4m3 operands (nv_vit_forward_fp8_train): fills the training
        workspace exactly as forward(training=True) does, so backward() follows as usual (on bf16 operands); dropout as in forward()."""
        return self._forward("nv_vit_forward_fp8_train", video, 1, self._fp8_weights(params, params16, f8), _drop(dropout), vol_sigma=vol_sigma,
                             rows_form=rows_form, dropout=dropout)[1]

    def forward_fp8(self, video: torch.Tensor, params: torch.Tensor, params16: torch.Tensor, f8, vol_sigma=None, time_points: int = 0) -> torch.Tensor:
        return self._forward("nv_vit_forward_fp8", video, 0, self._fp8_weights(params, params16, f8), vol_sigma=vol_sigma, time_points=time_points)[1]

    @staticmethod
    def _fp8_weights(params, params16, f8):
        return (params.data_ptr(), params16.data_ptr(), f8["params8"].data_ptr(), f8["colscales"].data_ptr(), ctypes.cast(f8["act_scales"], ctypes.c_void_p))

    def backward(self, dlogits: Optional[torch.Tensor], params: torch.Tensor, params16: torch.Tensor, grads: Optional[torch.Tensor],
                 accumulate: bool, stages: Optional[Tuple[int, int]] = None, join_aux: bool = True,
                 grads16: Optional[torch.Tensor] = None, dvideo: Optional[torch.Tensor] = None, weight_grads: bool = True,
                 attn_grad: Optional[AttnGradExport] = None, *, of: Optional[_Pass] = None, final: bool = False,
                 dtokens: Optional[torch.Tensor] = None, drop_path: Optional[torch.Tensor] = None) -> None:
        """Whole backward, or only stages [first, last] (0 = head, 1+k = layer depth-1-k, depth+1 = embedding).
        of: the pass to run against (several may be pending: siamese / two-forward losses), by default the most recent training forward.
        final: nothing more of this pass will run although the stages stop short of the embedding - like a whole backward, the call
        then marks the pass done (its workspace may be refilled) and its hook gradient ready.
        join_aux=False (only for ranges before the last stage): the current stream is not made to wait for the auxiliary
        stream - order the consumer of the range's gradients after `aux_stream_object()` as well.
        dvideo: fp32 tensor of the forward input's shape (any strides) that receives d loss / d video; written by the call whose
        stages contain the embedding.  weight_grads=False: the data-only backward - no parameter gradient is produced, `grads`
        and `grads16` must be None (nv_vit_backward_ex).
        attn_grad (make_attn_grad_export): the gradients w.r.t. the attention probabilities, written behind the attention backward of
        every exported layer inside the stage range (nv_vit_backward_attn); needs a forward without block dropout.
        dtokens (instead of dlogits, which is then None): fp32 [B, n, dim] or [B n, dim], the gradient w.r.t. the last block's output, cls rows
        included - the backward of a loss on the tokens (nv_vit_backward_tokens).  The head takes no part: its gradient range is zeroed
        (left alone when accumulating).  The forward must have run with rows_form=1; no attention-gradient export in this form.
        drop_path: the stochastic-depth factors of the forward; None = the table the pass kept (forward(drop_path=...)), which is what a
        backward must be given (nv_vit_backward_sd).  Not with dtokens."""
        if (dlogits is None) == (dtokens is None):
            raise ValueError("neurovit_amd: backward() takes dlogits or dtokens, not both and not neither")
        rec = self.backward_pass(of)
        B, ws, video = rec.B, rec.ws, rec.video
        drop_path = rec.drop_path if drop_path is None else drop_path
        if drop_path is not None and dtokens is not None:
            raise NotImplementedError("neurovit_amd: backward(dtokens=...) of a forward under stochastic depth - the token-level backward carries no path factors")
        sd = self._path_struct(drop_path, B, video.device)
        if rec.keep[1] is not None and rec.keep[1].time_points:
            raise NotImplementedError("neurovit_amd: the fused 4D input form is forward-only (the 4D model's encoder is frozen, NeuroEncoder.py:34-36)")
        first, last = (0, self.cfg.depth + 1) if stages is None else stages
        _cabi.set_operand_format(self.operands)
        if dtokens is not None:
            return self._backward_tokens(rec, dtokens, params, params16, grads, accumulate, first, last, join_aux, grads16, dvideo, weight_grads, attn_grad, final)
        if first == 0:
            rec.dlogits = dlogits.contiguous().float()
        if attn_grad is not None and rec.dropout[0] > 0:
            raise NotImplementedError("neurovit_amd: no attention gradients of a forward with attention dropout (the mask is not replayed "
                                      "into the gradient of the probabilities) - run the attribution in eval mode")
        if dvideo is not None:
            if rec.keep[0] is not None:
                raise NotImplementedError("neurovit_amd: no input gradient of a forward on RAW volumes (vol_sigma): the folded z-score "
                                          "treats sigma as a constant, so the gradient w.r.t. the raw volume would be wrong")
            assert dvideo.is_cuda and dvideo.dtype == torch.float32 and dvideo.shape == video.shape and dvideo.device == video.device
        if not weight_grads:
            assert grads is None and grads16 is None, "the data-only backward writes no gradient arena"
        opts = None          # nv_vit_backward_opts: only for the input gradient or the data-only form
        if dvideo is not None or not weight_grads:
            dstrides = None if dvideo is None else ops.strides5(dvideo)      # (kept alive across the call)
            opts = BackwardOpts(ctypes.sizeof(BackwardOpts), None if dvideo is None else dvideo.data_ptr(),
                                None if dstrides is None else ctypes.cast(dstrides, ctypes.c_void_p), int(bool(weight_grads)))
        # grads16: bf16 arena (element offsets of `grads`) that also receives the Linear weight gradients, rounded, straight from
        # their GEMMs - the data-parallel message buffer (mirrored_ranges() lists what lands there)
        entry = "nv_vit_backward_attn" if sd is None else "nv_vit_backward_sd"
        check(getattr(lib, entry)(ctypes.byref(self.cfg), B, video.data_ptr(), ops.strides5(video), params.data_ptr(),
                                  params16.data_ptr(), ws.data_ptr(), ws.numel(), rec.dlogits.data_ptr(),
                                  None if grads is None else grads.data_ptr(), None if grads16 is None else grads16.data_ptr(),
                                  int(accumulate), first, last, float(rec.dropout[0]), float(rec.dropout[1]), int(rec.dropout[2]),
                                  torch.cuda.current_stream().cuda_stream, self._aux_stream(video.device) if weight_grads else None,
                                  int(join_aux), int(rec.rows_form), None if opts is None else ctypes.byref(opts),
                                  None if attn_grad is None else ctypes.byref(attn_grad), *(() if sd is None else (ctypes.byref(sd),))),
              entry)
        if final or last == self.cfg.depth + 1:
            rec.finish()

    def _backward_tokens(self, rec, dtokens, params, params16, grads, accumulate, first, last, join_aux, grads16, dvideo, weight_grads, attn_grad, final) -> None:
        """backward(dtokens=...): the checks that belong to this form, then nv_vit_backward_tokens"""
        B, ws, video, c = rec.B, rec.ws, rec.video, self.cfg
        if attn_grad is not None:
            raise NotImplementedError("neurovit_amd: backward(dtokens=...) exports no attention gradients")
        if rec.rows_form != 1:
            raise ValueError("neurovit_amd: backward(dtokens=...) needs a forward whose last block ran on every row - forward(..., rows_form=1)")
        H, Wd, p1, p2 = image_hw(c)
        n = (c.frames // c.frame_patch_size) * (H // p1) * (Wd // p2) + 1
        if not dtokens.is_cuda or dtokens.numel() != B * n * c.dim or dtokens.shape[-1] != c.dim:
            raise ValueError(f"neurovit_amd: dtokens of shape {tuple(dtokens.shape)} on {dtokens.device}, expected a device tensor [{B}, {n}, {c.dim}]")
        if dvideo is not None:
            if rec.keep[0] is not None:
                raise NotImplementedError("neurovit_amd: no input gradient of a forward on RAW volumes (vol_sigma)")
            assert dvideo.is_cuda and dvideo.dtype == torch.float32 and dvideo.shape == video.shape and dvideo.device == video.device
        if not weight_grads:
            assert grads is None and grads16 is None, "the data-only backward writes no gradient arena"
        if first == 0:
            rec.dtokens = dtokens.contiguous().float()      # (kept with the pass: a staged backward's later calls pass the same pointer)
        elif rec.dtokens is None:
            raise RuntimeError("neurovit_amd: backward(dtokens=...) of stages that start behind stage 0, whose seeding launch has not run for this pass")
        opts = None
        if dvideo is not None or not weight_grads:
            dstrides = None if dvideo is None else ops.strides5(dvideo)
            opts = BackwardOpts(ctypes.sizeof(BackwardOpts), None if dvideo is None else dvideo.data_ptr(),
                                None if dstrides is None else ctypes.cast(dstrides, ctypes.c_void_p), int(bool(weight_grads)))
        check(lib.nv_vit_backward_tokens(ctypes.byref(c), B, video.data_ptr(), ops.strides5(video), params.data_ptr(), params16.data_ptr(), ws.data_ptr(),
                                         ws.numel(), rec.dtokens.data_ptr(), None if grads is None else grads.data_ptr(),
                                         None if grads16 is None else grads16.data_ptr(), int(accumulate), first, last, float(rec.dropout[0]),
                                         float(rec.dropout[1]), int(rec.dropout[2]), torch.cuda.current_stream().cuda_stream,
                                         self._aux_stream(video.device) if weight_grads else None, int(join_aux), int(rec.rows_form),
                                         None if opts is None else ctypes.byref(opts)), "nv_vit_backward_tokens")
        if final or last == self.cfg.depth + 1:
            rec.finish()

    def train_step(self, video: torch.Tensor, labels: torch.Tensor, params: torch.Tensor, params16: torch.Tensor, grads: torch.Tensor,
                   adam_m: torch.Tensor, adam_v: torch.Tensor, *, step: int, lr: float, betas, eps: float, weight_decay: float,
                   grad_scale: float = 1.0, accumulate: bool = False, update: bool = True, fuse_update: int = 0,
                   dropout: Tuple[float, float, int] = (0.0, 0.0, 0), vol_sigma=None, rows_form: Optional[int] = None,
                   loss_scale: float = 0.0, loss_scale_state: Optional[torch.Tensor] = None, dp=None, loss_opts=None,
                   drop_path: Optional[torch.Tensor] = None, reg_opts=None):
        """The reference's whole train step (Trainer.py:65-79) as ONE native call (nv_vit_train_step): forward, CrossEntropyLoss,
        backward of every stage, AdamW over the arena + bf16 shadow refresh.  Returns (loss [1], logits [B, C]) on the device.
        Same launches, streams and arithmetic as forward() + ops.ce_loss + backward() + ops.adamw_step.
        fuse_update (only with update and not accumulate): 1 = the transformer layers' Linear weights are updated by their
        weight-gradient GEMMs (their gradients are then not left in `grads`), 2 = the same but they are; same bits either way.
        loss_scale: static factor on d(loss)/d(logits), divided out again by the update; loss_scale_state: the device block of a
        dynamic loss scale (optim.LossScaler) - GradScaler semantics on the device, needs fuse_update = 0.
        loss_opts: None, or a _cabi.LossOpts (ops.loss_opts: label smoothing, class weights, a mix table) - the step then goes
        through nv_vit_train_step_ex; the tensors it points to are the caller's to keep alive.
        drop_path: None, or the step's stochastic-depth factors fp32 [depth, 2, B] on the device (nv_vit_train_step_sd; every form above).
        reg_opts: None, or a _cabi.RegOpts (ops.reg_opts) - the regression objective (nv_vit_train_step_reg; every form above): `labels` are
          then the targets, fp32 [B, num_classes] on the device, and loss_opts must be None."""
        B, dev = video.shape[0], video.device
        loss = torch.empty(1, dtype=torch.float32, device=dev)
        dlogits = torch.empty((B, self.cfg.num_classes), dtype=torch.float32, device=dev)
        if reg_opts is not None:
            assert loss_opts is None, "the regression objective has options of its own (reg_opts)"
            assert labels.is_cuda and labels.dtype == torch.float32 and tuple(labels.shape) == (B, self.cfg.num_classes) and labels.is_contiguous()
        else:
            assert labels.is_cuda and labels.dtype == torch.int64 and labels.numel() == B and labels.is_contiguous()
        hp = TrainHparams(ctypes.sizeof(TrainHparams), int(step), float(lr), float(betas[0]), float(betas[1]), float(eps), float(weight_decay),
                          float(grad_scale), int(bool(accumulate)), int(bool(update)), int(fuse_update), float(loss_scale),
                          None if dp is None else ctypes.cast(ctypes.pointer(dp), ctypes.c_void_p),      # _cabi.DpPlan (kept alive by the caller)
                          None if loss_scale_state is None else loss_scale_state.data_ptr())
        extra = () if loss_opts is None else (ctypes.byref(loss_opts),)
        entry = "nv_vit_train_step_ex" if extra else "nv_vit_train_step"
        if drop_path is not None:
            entry, extra = "nv_vit_train_step_sd", extra or (None,)
        if reg_opts is not None:
            entry, extra = "nv_vit_train_step_reg", (ctypes.byref(reg_opts),)
        rec, logits = self._forward(entry, video, 1,
                                    (params.data_ptr(), params16.data_ptr(), grads.data_ptr(), adam_m.data_ptr(), adam_v.data_ptr()), (labels.data_ptr(),),
                                    (loss.data_ptr(), dlogits.data_ptr(), ctypes.byref(hp)) + extra + _drop(dropout),
                                    vol_sigma=vol_sigma, rows_form=rows_form, dropout=dropout, step=True, drop_path=drop_path,
                                    path_arg=reg_opts is not None)
        rec.dlogits = dlogits
        return loss, logits

    def aux_stream_object(self, device) -> Optional[torch.cuda.Stream]:
        """The torch stream object behind the engine's auxiliary stream (None when the engine runs single-stream)."""
        return self._aux.get(str(device)) if self.use_aux_stream else None

    def _aux_stream(self, device):
        if not self.use_aux_stream:
            return None
        st = self._aux.get(str(device))
        if st is None:
            from .parallel import independent_stream     # a stream that does not share the current stream's hardware queue
            st = self._aux[str(device)] = independent_stream(device, [torch.cuda.current_stream(device)])
        return st.cuda_stream

    def stage_range(self, first: int, last: int) -> Tuple[int, int]:
        """Arena element range [begin, end) that is final after backward stages first..last have run."""
        lo, hi = None, None
        b, e = ctypes.c_long(), ctypes.c_long()
        for s in range(first, last + 1):
            check(lib.nv_vit_stage_param_range(ctypes.byref(self.cfg), s, ctypes.byref(b), ctypes.byref(e)), "nv_vit_stage_param_range")
            lo = b.value if lo is None else min(lo, b.value)
            hi = e.value if hi is None else max(hi, e.value)
        return lo, hi

    def tap(self, name: str, layer: int, shape, dtype) -> torch.Tensor:
        """View of a named activation inside the last forward's workspace (tests, Grad-CAM hooks)."""
        B, layout, ws = self.last.B, self.last.layout, self.last.ws
        off = lib.nv_vit_workspace_offset(ctypes.byref(self.cfg), B, layout, name.encode(), layer)
        if off < 0:
            raise KeyError(f"no workspace buffer {name!r} (layer {layer})")
        n = 1
        for s in shape:
            n *= s
        return ws[off:off + n * _BYTES[dtype]].view(dtype).view(*shape)
