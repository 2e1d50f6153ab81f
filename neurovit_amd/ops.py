"""Thin functional wrappers over the C-ABI (one Python function per kernel entry point).

PyTorch is plumbing only: it owns the device buffers and the stream; every FLOP below runs in
libneurovit_hip.so.  No fallbacks: CPU tensors raise.
"""
from __future__ import annotations

import ctypes
from typing import Optional, Tuple

import torch

from . import _cabi
from ._cabi import check, lib


def op16() -> torch.dtype:
    """torch dtype of the 16-bit operand buffers under the current operand format (_cabi.set_operand_format): bfloat16 or float16"""
    return torch.float16 if _cabi.operand_format() == "fp16" else torch.bfloat16


NT, NN, TN = 0, 1, 2
EPI_STORE_BF16, EPI_STORE_F32, EPI_BIAS_F32, EPI_BIAS_GELU, EPI_BIAS_RESID, EPI_DGELU, EPI_DGELU_COLSUM = 0, 1, 2, 3, 4, 5, 6


def _stream() -> int:
    return torch.cuda.current_stream().cuda_stream


def _p(t: Optional[torch.Tensor]):
    return None if t is None else t.data_ptr()


def _need_cuda(*ts):
    for t in ts:
        if t is not None and not t.is_cuda:
            raise RuntimeError("neurovit_amd ops run on MI355X only (got a CPU tensor); there is no CPU fallback")


def _i32(t: Optional[torch.Tensor], n: int, what: str) -> Optional[torch.Tensor]:
    if t is None:
        return None
    _need_cuda(t)
    if t.dtype != torch.int32 or t.dim() != 1 or t.numel() != n or not t.is_contiguous():
        raise ValueError(f"{what} must be a contiguous int32 [{n}] tensor on the device")
    return t


def _f32(t: Optional[torch.Tensor], n: int, what: str) -> Optional[torch.Tensor]:
    if t is None:
        return None
    _need_cuda(t)
    if t.dtype != torch.float32 or t.numel() != n or not t.is_contiguous():
        raise ValueError(f"{what} must be a contiguous float32 tensor of {n} elements on the device")
    return t


def _rows2d(X, what: str, exc=ValueError):
    """the shape (N, w) of X, which must be float32 [N, w] on the device with N >= 1 and unit column stride (a row-strided view passes its
    leading dimension); anything else raises `exc` - the type that the call site has always raised"""
    if not torch.is_tensor(X) or X.dtype != torch.float32 or X.dim() != 2 or X.stride(1) != 1 or X.shape[0] < 1 or not X.is_cuda:
        raise exc(f"{what}: float32 [N, w] on the device with N >= 1 and unit column stride expected, got "
                  f"{(tuple(X.shape), X.dtype, X.device.type) if torch.is_tensor(X) else type(X).__name__}")
    return X.shape


def shape5(video: torch.Tensor):
    assert video.dim() == 5
    return (ctypes.c_long * 5)(*video.shape)


def cast_ranges_bf16(src: torch.Tensor, dst: torch.Tensor, ranges) -> None:
    """dst[b:e] = bf16(src[b:e]) for the element ranges [(b, e), ...] of two flat arenas (fp32 -> bf16), one launch per 48 ranges."""
    _need_cuda(src, dst)
    assert src.dtype == torch.float32 and dst.dtype == op16() and src.dim() == 1 and dst.numel() >= src.numel()
    ranges = [(int(b), int(e)) for b, e in ranges if e > b]
    if not ranges:
        return
    begins = (ctypes.c_long * len(ranges))(*[b for b, _ in ranges])
    lens = (ctypes.c_long * len(ranges))(*[e - b for b, e in ranges])
    check(lib.nv_cast_ranges_bf16(_p(src), _p(dst), begins, lens, len(ranges), _stream()), "nv_cast_ranges_bf16")


NO_PATH = object()      # `path` of the wrappers below: not given - the symbol without a factor table; None or a tensor - the *_path symbol (None = NULL)


def _path_call(name: str, path, path_rows: int):
    """(C function, trailing arguments) of a kernel-level call: `name`, or `name`_path with (path, path_rows) - path = the fp32 [samples]
    stochastic-depth factors of one site, path_rows = token rows per sample"""
    if path is NO_PATH:
        return getattr(lib, name), ()
    return getattr(lib, name + "_path"), (_p(path), int(path_rows))


def skinny_nt(epi: int, A: torch.Tensor, W: torch.Tensor, bias: torch.Tensor, out: torch.Tensor, resid: Optional[torch.Tensor] = None,
              u_out: Optional[torch.Tensor] = None, drop_seed: int = 0, drop_p: float = 0.0, path=NO_PATH, path_rows: int = 0) -> torch.Tensor:
    """out[r] = epilogue(A[r] @ W.T) on a few rows; A / resid / out / u_out may be row-strided 2-D views (e.g. x[::n]).
    epi 0: out f32 = resid + (bias + A W^T) * mask; epi 1: u = bias + A W^T (bf16, optional), out bf16 = gelu(u) * mask.
    mask: nn.Dropout of the dense tensor `out` is a view of (element offsets are hashed), drop_p = 0: none."""
    _need_cuda(A, W)
    R, K = A.shape
    N = W.shape[0]
    fn, tail = _path_call("nv_skinny_nt", path, path_rows)
    check(fn(epi, R, N, K, _p(A), A.stride(0), _p(W), W.stride(0), _p(bias), _p(resid), 0 if resid is None else resid.stride(0),
             _p(out), out.stride(0), _p(u_out), 0 if u_out is None else u_out.stride(0), int(drop_seed), float(drop_p), _stream(), *tail), "nv_skinny_nt")
    return out


def skinny_nn(epi: int, A: torch.Tensor, W: torch.Tensor, out: torch.Tensor, u: Optional[torch.Tensor] = None,
              dcol: Optional[torch.Tensor] = None, accumulate: bool = False, drop_seed: int = 0, drop_p: float = 0.0) -> torch.Tensor:
    """out[r] = epilogue(A[r] @ W) on a few rows (W [K, N]); epi 0: bf16 (A W * mask) * gelu'(u) (+ column sums into dcol), 1: f32, 2: bf16."""
    _need_cuda(A, W)
    R, K = A.shape
    N = W.shape[1]
    check(lib.nv_skinny_nn(epi, R, N, K, _p(A), A.stride(0), _p(W), W.stride(0), _p(u), 0 if u is None else u.stride(0), _p(out), out.stride(0),
                           _p(dcol), int(accumulate), int(drop_seed), float(drop_p), _stream()), "nv_skinny_nn")
    return out


def strides5(video: torch.Tensor):
    assert video.dim() == 5
    return (ctypes.c_long * 5)(*video.stride())


def gemm(layout: int, epi: int, A: torch.Tensor, B: torch.Tensor, *, out: Optional[torch.Tensor] = None, bias=None,
         aux_in=None, aux_out=None, accumulate: bool = False, alpha: float = 1.0, drop_seed: int = 0, drop_p: float = 0.0,
         path=NO_PATH, path_rows: int = 0) -> torch.Tensor:
    """C = op(A) op(B) with a fused epilogue; A, B bf16 2-D row-major (last stride 1).  path / path_rows: nv_gemm_bf16_path (epilogue 4)."""
    _need_cuda(A, B)
    assert A.dtype == op16() and B.dtype == op16() and A.stride(1) == 1 and B.stride(1) == 1
    if layout == NT:
        M, K = A.shape; N = B.shape[0]; assert B.shape[1] == K
    elif layout == NN:
        M, K = A.shape; N = B.shape[1]; assert B.shape[0] == K
    else:
        K, M = A.shape; N = B.shape[1]; assert B.shape[0] == K
    odt = op16() if epi in (EPI_STORE_BF16, EPI_BIAS_GELU, EPI_DGELU, EPI_DGELU_COLSUM) else torch.float32
    if out is None:
        out = torch.empty((M, N), dtype=odt, device=A.device)
    assert out.dtype == odt and out.shape == (M, N) and out.stride(1) == 1
    fn, tail = _path_call("nv_gemm_bf16", path, path_rows)
    check(fn(layout, epi, M, N, K, _p(A), A.stride(0), _p(B), B.stride(0), _p(out), out.stride(0), _p(bias),
             _p(aux_in), 0 if aux_in is None else aux_in.stride(0), _p(aux_out),
             0 if aux_out is None else aux_out.stride(0), int(accumulate), float(alpha), drop_seed, drop_p, _stream(), *tail), "nv_gemm_bf16")
    return out


EPI_F32_STORE, EPI_F32_BIAS, EPI_F32_BIAS_GELU, EPI_F32_BIAS_RESID = 0, 2, 3, 4


def gemm_f32(epi: int, A: torch.Tensor, W: torch.Tensor, *, bias=None, resid=None, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """fp32 inference path: out[M, N] = epi(A[M, K] @ W[N, K].T), every operand fp32, contraction on the fp32 MFMA.
    A / resid / out may be row-strided 2-D views (last stride 1)."""
    _need_cuda(A, W)
    assert A.dtype == torch.float32 and W.dtype == torch.float32 and A.stride(1) == 1 and W.stride(1) == 1
    M, K = A.shape
    N = W.shape[0]
    assert W.shape[1] == K
    if out is None:
        out = torch.empty((M, N), dtype=torch.float32, device=A.device)
    assert out.dtype == torch.float32 and out.shape == (M, N) and out.stride(1) == 1
    check(lib.nv_gemm_f32(epi, M, N, K, _p(A), A.stride(0), _p(W), W.stride(0), _p(out), out.stride(0), _p(bias), _p(resid),
                          0 if resid is None else resid.stride(0), _stream()), "nv_gemm_f32")
    return out


def attn_fwd_f32(qkv: torch.Tensor, B: int, n: int, heads: int, dim_head: int = 64, *, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """qkv f32 [B*n, 3*inner] -> out f32 [B*n, inner] (softmax(q k^T / sqrt(dh)) v per head, fp32 MFMA); out: a row-strided view to write."""
    _need_cuda(qkv)
    assert qkv.dtype == torch.float32 and qkv.stride(1) == 1
    inner = heads * dim_head
    out = _out2d(out, B * n, inner, torch.float32, qkv)
    check(lib.nv_attn_fwd_f32(_p(qkv), qkv.stride(0), B, n, heads, dim_head, dim_head ** -0.5, _p(out), out.stride(0), _stream()), "nv_attn_fwd_f32")
    return out


def ln_fwd_f32(x: torch.Tensor, gamma, beta, eps: float = 1e-5, *, y: Optional[torch.Tensor] = None, st=None) -> torch.Tensor:
    """y: a row-strided view to write; st: (mean, rstd) f32 [M] each, written when given"""
    _need_cuda(x)
    M, d = x.shape
    y = _out2d(y, M, d, torch.float32, x)
    mean, rstd = (None, None) if st is None else (st[0], st[1])
    check(lib.nv_ln_fwd_f32(_p(x), x.stride(0), M, d, _p(gamma), _p(beta), eps, _p(y), y.stride(0), _p(mean), _p(rstd), _stream()), "nv_ln_fwd_f32")
    return y


def patch_ln_fwd_f32(video: torch.Tensor, p1: int, p2: int, pf: int, gamma, beta, eps: float = 1e-5, vol_sigma=None, *, out=None, st=None):
    """As patch_ln_fwd with fp32 tokens [B*N, P] (fp32 inference path)."""
    _need_cuda(video)
    B, C, F, H, W = video.shape
    P = C * p1 * p2 * pf
    N = (F // pf) * (H // p1) * (W // p2)
    out = _out2d(out, B * N, P, torch.float32, video)
    st = torch.empty((2, B * N), dtype=torch.float32, device=video.device) if st is None else st
    check(lib.nv_patch_ln_fwd_f32(_p(video), strides5(video), B, C, F, H, W, p1, p2, pf, _p(gamma), _p(beta), eps, _p(out), out.stride(0), _p(st[0]),
                                  _p(st[1]), _p(vol_sigma), _stream()), "nv_patch_ln_fwd_f32")
    return out, st


class GemmProblem(ctypes.Structure):          # include/neurovit_hip.h::nv_gemm_problem
    _fields_ = [("M", ctypes.c_int), ("N", ctypes.c_int), ("K", ctypes.c_int), ("A", ctypes.c_void_p), ("lda", ctypes.c_long),
                ("B", ctypes.c_void_p), ("ldb", ctypes.c_long), ("C", ctypes.c_void_p), ("ldc", ctypes.c_long), ("accumulate", ctypes.c_int),
                ("C16", ctypes.c_void_p), ("ldc16", ctypes.c_long)]


def gemm_tn_grouped(problems) -> None:
    """problems: up to four (A[K, M] bf16, B[K, N] bf16, C[M, N] f32, accumulate[, C16[M, N] bf16 mirror]) - C (+)= A^T B, one launch."""
    arr = (GemmProblem * len(problems))()
    for i, pr in enumerate(problems):
        A, B, C, acc = pr[:4]
        C16 = pr[4] if len(pr) > 4 else None
        _need_cuda(A)
        K, M = A.shape
        N = B.shape[1]
        assert B.shape[0] == K and C.shape == (M, N) and C.dtype == torch.float32
        assert C16 is None or (C16.shape == (M, N) and C16.dtype == op16())
        arr[i] = GemmProblem(M, N, K, A.data_ptr(), A.stride(0), B.data_ptr(), B.stride(0), C.data_ptr(), C.stride(0), int(acc),
                             _p(C16), 0 if C16 is None else C16.stride(0))
    check(lib.nv_gemm_bf16_grouped(TN, EPI_STORE_F32, len(problems), ctypes.cast(arr, ctypes.c_void_p), _stream()), "nv_gemm_bf16_grouped")


def adamw_arena(params, grads, adam_m, adam_v, params16, step, lr, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, grad_scale=1.0, keep_grads=False):
    """struct nv_adamw_arena over five flat tensors that share element offsets (fp32 x 4, bf16 shadow)."""
    from ._cabi import AdamwArena
    n = params.numel()
    assert all(t.is_cuda and t.is_contiguous() and t.numel() == n for t in (params, grads, adam_m, adam_v, params16))
    assert params16.dtype == op16() and all(t.dtype == torch.float32 for t in (params, grads, adam_m, adam_v))
    return AdamwArena(ctypes.sizeof(AdamwArena), int(step), float(lr), float(betas[0]), float(betas[1]), float(eps), float(weight_decay), float(grad_scale),
                      int(bool(keep_grads)), params.data_ptr(), grads.data_ptr(), adam_m.data_ptr(), adam_v.data_ptr(), params16.data_ptr())


def gemm_tn_grouped_adamw(problems, opt) -> None:
    """problems: up to four (A[K, M] bf16, B[K, N] bf16, C[M, N] f32 VIEW INTO opt's gradient arena): the gradient C = A^T B is consumed by
    the AdamW update of the parameters at the same arena offsets inside the GEMM's epilogue (nv_gemm_bf16_grouped_adamw)."""
    arr = (GemmProblem * len(problems))()
    for i, pr in enumerate(problems):
        A, B, C = pr[:3]
        _need_cuda(A)
        K, M = A.shape
        N = B.shape[1]
        assert B.shape[0] == K and C.shape == (M, N) and C.dtype == torch.float32
        arr[i] = GemmProblem(M, N, K, A.data_ptr(), A.stride(0), B.data_ptr(), B.stride(0), C.data_ptr(), C.stride(0), 0, None, 0)
    check(lib.nv_gemm_bf16_grouped_adamw(len(problems), ctypes.cast(arr, ctypes.c_void_p), ctypes.byref(opt), _stream()), "nv_gemm_bf16_grouped_adamw")


def adamw_ranges(opt, ranges) -> None:
    """AdamW (nv_adamw_step arithmetic) over [(begin, len)] element ranges of opt's arenas, one launch."""
    n = len(ranges)
    b = (ctypes.c_long * max(n, 1))(*[int(r[0]) for r in ranges])
    l = (ctypes.c_long * max(n, 1))(*[int(r[1]) for r in ranges])
    check(lib.nv_adamw_ranges(ctypes.byref(opt), b, l, n, _stream()), "nv_adamw_ranges")


def ln_fwd(x: torch.Tensor, gamma, beta, eps: float = 1e-5, *, y: Optional[torch.Tensor] = None, st=None):
    """y: a row-strided 16-bit view to write (its leading dimension is passed on); st: [2, M], or a pair of f32 [M] (mean, rstd)"""
    _need_cuda(x)
    M, d = x.shape
    y = _out2d(y, M, d, op16(), x)
    st = torch.empty((2, M), dtype=torch.float32, device=x.device) if st is None else st
    check(lib.nv_ln_fwd(_p(x), x.stride(0), M, d, _p(gamma), _p(beta), eps, _p(y), y.stride(0), _p(st[0]), _p(st[1]), _stream()), "nv_ln_fwd")
    return y, st


def ln_bwd(dy, x, st, gamma, g_in=None, want_g16=True, accumulate=False, dgamma=None, dbeta=None, dcolsum=None, drop_seed=0, drop_p=0.0,
           path=NO_PATH, path_rows: int = 0, *, g_out: Optional[torch.Tensor] = None, g16: Optional[torch.Tensor] = None):
    """g_out / g16: row-strided views to write (ldg / ldg16 = their .stride(0); g_in, read through ldg, must share g_out's).  Not given:
    g_out is g_in (in place) or a fresh dense tensor, g16 a fresh dense tensor when want_g16."""
    _need_cuda(dy, x)
    M, d = x.shape
    if g_out is None:
        g_out = torch.empty((M, d), dtype=torch.float32, device=x.device) if g_in is None else g_in
    assert g_out.dtype == torch.float32 and g_out.shape == (M, d) and g_out.stride(1) == 1
    assert g_in is None or (g_in.shape == (M, d) and g_in.stride(1) == 1 and (M == 1 or g_in.stride(0) == g_out.stride(0))), "g_in and g_out share ldg"
    if g16 is None:
        g16 = torch.empty((M, d), dtype=op16(), device=x.device) if want_g16 else None
    assert g16 is None or (g16.dtype == op16() and g16.shape == (M, d) and g16.stride(1) == 1)
    dgamma = torch.empty(d, device=x.device) if dgamma is None else dgamma
    dbeta = torch.empty(d, device=x.device) if dbeta is None else dbeta
    dcolsum = torch.empty(d, device=x.device) if dcolsum is None else dcolsum
    nb = lib.nv_ln_bwd_workspace_bytes(M, d)
    ws = torch.empty(nb, dtype=torch.uint8, device=x.device)
    fn, tail = _path_call("nv_ln_bwd", path, path_rows)
    check(fn(_p(dy), dy.stride(0), _p(x), x.stride(0), _p(st[0]), _p(st[1]), _p(gamma), M, d, _p(g_in), _p(g_out), g_out.stride(0),
             _p(g16), d if g16 is None else g16.stride(0), _p(dgamma), _p(dbeta), _p(dcolsum), int(accumulate), _p(ws), nb, drop_seed, drop_p, _stream(), None, *tail), "nv_ln_bwd")
    return g_out, g16, dgamma, dbeta, dcolsum


def patch_ln_fwd(video: torch.Tensor, p1: int, p2: int, pf: int, gamma, beta, eps: float = 1e-5, ldo: Optional[int] = None, vol_sigma=None, *,
                 out: Optional[torch.Tensor] = None, st=None):
    """video [B,C,F,H,W] (any strides, e.g. the permuted view of a [B,H,W,D] volume).  out: a 16-bit [B*N, >= P] view to write - its
    .stride(0) is ldo, and the kernel writes zeros in the columns P .. ldo-1 of every row, whatever the view's width."""
    _need_cuda(video)
    B, C, F, H, W = video.shape
    P = C * p1 * p2 * pf
    N = (F // pf) * (H // p1) * (W // p2)
    if out is None:
        ldo = (P + 7) // 8 * 8 if ldo is None else ldo
        out = torch.empty((B * N, ldo), dtype=op16(), device=video.device)
    else:
        assert out.dtype == op16() and out.shape[0] == B * N and out.shape[1] >= P and out.stride(1) == 1
        ldo = out.stride(0)
    st = torch.empty((2, B * N), dtype=torch.float32, device=video.device) if st is None else st
    check(lib.nv_patch_ln_fwd(_p(video), strides5(video), B, C, F, H, W, p1, p2, pf, _p(gamma), _p(beta), eps, _p(out), ldo, _p(st[0]),
                              _p(st[1]), _p(vol_sigma), _stream()), "nv_patch_ln_fwd")
    return out, st


def patch_ln_bwd(video, p1, p2, pf, dxp, st, accumulate=False, *, dgamma=None, dbeta=None):
    """dxp f32 [B*N, >= P] with any row stride (ldd = dxp.stride(0)); dgamma / dbeta: f32 [P] to write (or add to, accumulate)"""
    B, C, F, H, W = video.shape
    P = C * p1 * p2 * pf
    T = dxp.shape[0]
    dg = torch.empty(P, device=video.device) if dgamma is None else dgamma
    db = torch.empty(P, device=video.device) if dbeta is None else dbeta
    nb = lib.nv_patch_ln_bwd_workspace_bytes(T, P)
    ws = torch.empty(nb, dtype=torch.uint8, device=video.device)
    check(lib.nv_patch_ln_bwd(_p(video), strides5(video), B, C, F, H, W, p1, p2, pf, _p(dxp), dxp.stride(0), _p(st[0]), _p(st[1]), _p(dg),
                              _p(db), int(accumulate), _p(ws), nb, _stream()), "nv_patch_ln_bwd")
    return dg, db


def patch_ln_dx(video, p1, p2, pf, dxp, st, gamma, *, dvideo: Optional[torch.Tensor] = None):
    """d loss / d video (f32, the geometry of `video`; dvideo: a [B,C,F,H,W] tensor of any strides to write) from dxp f32 [B*N, >= P] with any
    row stride (ldd = dxp.stride(0); columns P .. ldd-1 are not read), the forward's token statistics and gamma: nv_patch_ln_dx."""
    _need_cuda(video, dxp)
    B, C, F, H, W = video.shape
    dvideo = torch.empty(video.shape, dtype=torch.float32, device=video.device) if dvideo is None else dvideo
    assert dvideo.shape == video.shape and dvideo.dtype == torch.float32 and dxp.dtype == torch.float32 and dxp.stride(1) == 1
    check(lib.nv_patch_ln_dx(_p(video), strides5(video), B, C, F, H, W, p1, p2, pf, _p(dxp), dxp.stride(0), _p(st[0]), _p(st[1]), _p(gamma),
                             _p(dvideo), strides5(dvideo), _stream()), "nv_patch_ln_dx")
    return dvideo


def embed_finish_fwd(t, B, N, gamma, beta, pos, cls, eps=1e-5, drop_seed=0, drop_p=0.0, *, x: Optional[torch.Tensor] = None, st=None):
    """x: an f32 [B * (N + 1), d] row-strided view to write (ldx = its .stride(0)) instead of a fresh dense [B, N + 1, d]"""
    d = t.shape[1]
    ldx = d
    if x is None:
        x = torch.empty((B, N + 1, d), dtype=torch.float32, device=t.device)
    else:
        assert x.dtype == torch.float32 and x.shape == (B * (N + 1), d) and x.stride(1) == 1
        ldx = x.stride(0)
    st = torch.empty((2, B * N), dtype=torch.float32, device=t.device) if st is None else st
    check(lib.nv_embed_finish_fwd(_p(t), t.stride(0), B, N, d, _p(gamma), _p(beta), eps, _p(pos), _p(cls), _p(x), ldx, _p(st[0]), _p(st[1]),
                                  drop_seed, drop_p, _stream()), "nv_embed_finish_fwd")
    return x, st


def embed_finish_bwd(g, t, st, gamma, B, N, drop_seed=0, drop_p=0.0, *, dt: Optional[torch.Tensor] = None, dt16: Optional[torch.Tensor] = None,
                     params=None, data_only: bool = False):
    """g: f32 [B, N + 1, d] dense, or a 2-D [B * (N + 1), d] row-strided view (ldg = its .stride(0)).  dt / dt16: [B * N, d] row-strided
    views to write.  params: (dgamma, dbeta, dbias, dpos, dcls) to write; data_only: all five NULL - only dt / dt16 are produced."""
    d = t.shape[1]
    dev = t.device
    dt = _out2d(dt, B * N, d, torch.float32, t)
    dt16 = _out2d(dt16, B * N, d, op16(), t)
    if data_only:
        assert params is None
        dgamma = dbeta = dbias = dpos = dcls = None
    elif params is not None:
        dgamma, dbeta, dbias, dpos, dcls = params
    else:
        dgamma, dbeta, dbias = (torch.empty(d, device=dev) for _ in range(3))
        dpos = torch.empty((N + 1, d), device=dev); dcls = torch.empty(d, device=dev)
    nb = lib.nv_embed_finish_bwd_workspace_bytes(B, N, d)
    ws = torch.empty(nb, dtype=torch.uint8, device=dev)
    g2 = g.reshape(B * (N + 1), d) if g.dim() == 3 else g
    assert g2.shape == (B * (N + 1), d) and g2.stride(1) == 1
    check(lib.nv_embed_finish_bwd(_p(g2), g2.stride(0), _p(t), t.stride(0), _p(st[0]), _p(st[1]), _p(gamma), B, N, d, _p(dt), dt.stride(0), _p(dt16),
                                  dt16.stride(0), _p(dgamma), _p(dbeta), _p(dbias), _p(dpos), _p(dcls), 0, _p(ws), nb, drop_seed, drop_p, _stream()),
          "nv_embed_finish_bwd")
    return dt, dt16, dgamma, dbeta, dbias, dpos, dcls


def attn_fwd(qkv: torch.Tensor, B: int, n: int, heads: int, dim_head: int = 64, drop_seed=0, drop_p=0.0, *, out: Optional[torch.Tensor] = None,
             lse: Optional[torch.Tensor] = None):
    """qkv bf16 [B*n, 3*inner] -> (out bf16 [B*n, inner], lse f32 [B, heads, n]).  out: a row-strided view to write (ld_out = its .stride(0));
    lse: contiguous f32 of B * heads * n cells to write."""
    _need_cuda(qkv)
    inner = heads * dim_head
    out = _out2d(out, B * n, inner, op16(), qkv)
    lse = torch.empty((B, heads, n), dtype=torch.float32, device=qkv.device) if lse is None else lse
    assert lse.dtype == torch.float32 and lse.numel() == B * heads * n and lse.is_contiguous()
    check(lib.nv_attn_fwd(_p(qkv), qkv.stride(0), B, n, heads, dim_head, dim_head ** -0.5, _p(out), out.stride(0), _p(lse), drop_seed, drop_p, _stream()), "nv_attn_fwd")
    return out, lse


def attn_fwd_o8(qkv: torch.Tensor, B: int, n: int, heads: int, out_scale: float, dim_head: int = 64) -> torch.Tensor:
    """Attention forward with the output as OCP e4m3 bytes of (value * out_scale): uint8 [B*n, heads*dim_head] (fp8 inference path)."""
    _need_cuda(qkv)
    inner = heads * dim_head
    out = torch.empty((B * n, inner), dtype=torch.uint8, device=qkv.device)
    check(lib.nv_attn_fwd_o8(_p(qkv), qkv.stride(0), B, n, heads, dim_head, dim_head ** -0.5, _p(out), inner, float(out_scale), _stream()), "nv_attn_fwd_o8")
    return out


def attn_probs(qkv: torch.Tensor, B: int, n: int, heads: int, dim_head: int = 64, head_fusion: Optional[str] = None, rows: str = "all",
               out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """softmax(q k^T / sqrt(dh)) of a qkv buffer [B*n, 3*inner] (the operand format, or fp32) -> fp32 [B, heads, R, n] (head_fusion None)
    or [B, R, n] (head_fusion "mean" / "max" / "min"), R = n (rows "all") or 1 (rows "cls"): nv_attn_probs."""
    _need_cuda(qkv)
    assert qkv.stride(1) == 1 and qkv.dtype in (torch.float32, op16())
    fusion, form = _cabi.ATTN_FUSIONS[head_fusion], _cabi.ATTN_ROWS[rows]
    R = 1 if rows == "cls" else n
    shape = (B, heads, R, n) if head_fusion is None else (B, R, n)
    if out is None:
        out = torch.empty(shape, dtype=torch.float32, device=qkv.device)
    assert out.shape == shape and out.dtype == torch.float32 and out.is_contiguous()
    check(lib.nv_attn_probs(int(qkv.dtype == torch.float32), _p(qkv), qkv.stride(0), B, n, heads, dim_head, dim_head ** -0.5, fusion, form,
                            _p(out), _stream()), "nv_attn_probs")
    return out


def attn_rollout(maps, start_mean: bool = False) -> torch.Tensor:
    """Attention rollout over head-fused all-rows maps [B, n, n] (layer 0 first): [B, n - 1] = the patch-token entries of
    u A^_{L-1} ... A^_0, A^ = (A + I) / (rowsum(A) + 1); u = the cls row, or the mean of the rows (start_mean): nv_attn_rollout."""
    _need_cuda(*maps)
    B, n, _ = maps[0].shape
    for m in maps:
        assert m.shape == (B, n, n) and m.dtype == torch.float32 and m.is_contiguous()
    ptrs = (ctypes.c_void_p * len(maps))(*[m.data_ptr() for m in maps])
    nb = lib.nv_attn_rollout_workspace_bytes(B, n)
    ws = torch.empty(nb // 4, dtype=torch.float32, device=maps[0].device)
    out = torch.empty((B, n - 1), dtype=torch.float32, device=maps[0].device)
    check(lib.nv_attn_rollout(ctypes.cast(ptrs, ctypes.c_void_p), len(maps), B, n, int(bool(start_mean)), _p(out), _p(ws), nb, _stream()),
          "nv_attn_rollout")
    return out


def attn_grad(qkv: torch.Tensor, dout: torch.Tensor, B: int, n: int, heads: int, dim_head: int = 64, form: str = "per_head",
              out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Gradient w.r.t. the attention probabilities from a layer's qkv [B*n, 3*inner] and the gradient of its attention output dout
    [B*n, inner] (both in the operand format): fp32 [B, heads, n, n] = dO_h V_h^T (form "per_head") or [B, n, n] =
    mean_h relu(dP_h * P_h) (form "relevance", P = softmax(q k^T / sqrt(dh)) with the bits of attn_probs): nv_attn_grad."""
    _need_cuda(qkv, dout)
    assert qkv.stride(1) == 1 and dout.stride(1) == 1 and qkv.dtype == op16() and dout.dtype == op16()
    shape = (B, heads, n, n) if form == "per_head" else (B, n, n)
    if out is None:
        out = torch.empty(shape, dtype=torch.float32, device=qkv.device)
    assert out.shape == shape and out.dtype == torch.float32 and out.is_contiguous()
    check(lib.nv_attn_grad(_p(qkv), qkv.stride(0), _p(dout), dout.stride(0), B, n, heads, dim_head, dim_head ** -0.5,
                           _cabi.ATTN_GRAD_FORMS[form], _p(out), _stream()), "nv_attn_grad")
    return out


def attn_relevance(maps, start_mean: bool = False) -> torch.Tensor:
    """Class-specific token relevance over relevance-form maps [B, n, n] (layer 0 first): [B, n - 1] = the patch-token entries of
    u (I + A_{L-1}) ... (I + A_0); u = the cls row, or the mean of the rows (start_mean): nv_attn_relevance."""
    _need_cuda(*maps)
    B, n, _ = maps[0].shape
    for m in maps:
        assert m.shape == (B, n, n) and m.dtype == torch.float32 and m.is_contiguous()
    ptrs = (ctypes.c_void_p * len(maps))(*[m.data_ptr() for m in maps])
    nb = lib.nv_attn_relevance_workspace_bytes(B, n)
    ws = torch.empty(nb // 4, dtype=torch.float32, device=maps[0].device)
    out = torch.empty((B, n - 1), dtype=torch.float32, device=maps[0].device)
    check(lib.nv_attn_relevance(ctypes.cast(ptrs, ctypes.c_void_p), len(maps), B, n, int(bool(start_mean)), _p(out), _p(ws), nb, _stream()),
          "nv_attn_relevance")
    return out


def attn_bwd(qkv, out, dout, lse, B, n, heads, dim_head=64, drop_seed=0, drop_p=0.0, *, dqkv: Optional[torch.Tensor] = None,
             delta: Optional[torch.Tensor] = None):
    """out / dout: [B*n, inner] views that share one row stride (the C call has a single ld_out for both); dqkv: a row-strided view to
    write (ld_dqkv = its .stride(0)); delta: contiguous f32 of B * heads * n cells to write."""
    inner = heads * dim_head
    assert out.shape == (B * n, inner) and dout.shape == (B * n, inner) and out.stride(1) == 1 and dout.stride(1) == 1
    assert out.stride(0) == dout.stride(0), "out and dout share ld_out"
    dqkv = _out2d(dqkv, B * n, 3 * inner, op16(), qkv)
    delta = torch.empty((B, heads, n), dtype=torch.float32, device=qkv.device) if delta is None else delta
    assert delta.dtype == torch.float32 and delta.numel() == B * heads * n and delta.is_contiguous()
    check(lib.nv_attn_bwd(_p(qkv), qkv.stride(0), _p(out), _p(dout), out.stride(0), _p(lse), B, n, heads, dim_head, dim_head ** -0.5, _p(delta),
                          _p(dqkv), dqkv.stride(0), drop_seed, drop_p, _stream()), "nv_attn_bwd")
    return dqkv, delta


def head_fwd(x: torch.Tensor, gamma, beta, W, bias, eps=1e-5):
    """x f32 [B, n, d] -> logits [B, C] from the cls row (pool='cls')."""
    B, n, d = x.shape
    C = W.shape[0]
    xh = torch.empty((B, d), device=x.device); st = torch.empty((B, 2), device=x.device)
    logits = torch.empty((B, C), device=x.device)
    check(lib.nv_head_fwd(_p(x), n * d, B, d, _p(gamma), _p(beta), eps, _p(W), _p(bias), C, _p(xh), _p(st), _p(logits), _stream()), "nv_head_fwd")
    return logits, xh, st


def head_bwd(dlogits, W, x, st, xh, gamma, drop_seed=0, drop_p=0.0, path=NO_PATH, path_rows: int = 0):
    B, n, d = x.shape
    C = W.shape[0]
    dev = x.device
    g = torch.empty((B, n, d), device=dev); g16 = torch.empty((B, n, d), dtype=op16(), device=dev)
    dgamma, dbeta, dcol = (torch.empty(d, device=dev) for _ in range(3))
    dW = torch.empty((C, d), device=dev); db = torch.empty(C, device=dev)
    nb = lib.nv_head_bwd_workspace_bytes(B, d)
    ws = torch.empty(nb, dtype=torch.uint8, device=dev)
    fn, tail = _path_call("nv_head_bwd", path, path_rows)
    check(fn(_p(dlogits), B, C, _p(W), _p(x), n * d, _p(st), _p(xh), _p(gamma), d, n, _p(g), d, _p(g16), d, _p(dgamma), _p(dbeta),
             _p(dW), _p(db), _p(dcol), 0, _p(ws), nb, drop_seed, drop_p, 0, _stream(), *tail), "nv_head_bwd")
    return g, g16, dgamma, dbeta, dW, db, dcol


def _head_step_outputs(B, n, d, C, dev):
    """what a head step writes, in the order it is returned, and its workspace: (logits, xh, st, loss, dlogits, g, g16, dgamma, dbeta, dW,
    db, dcol), ws.  g / g16 start as NaN: the step must write every row."""
    logits, xh, st = torch.empty((B, C), device=dev), torch.empty((B, d), device=dev), torch.empty((B, 2), device=dev)
    loss, dl = torch.empty(1, device=dev), torch.empty((B, C), device=dev)
    g = torch.full((B, n, d), float("nan"), device=dev)
    g16 = torch.full((B, n, d), float("nan"), dtype=op16(), device=dev)
    dgamma, dbeta, dcol = (torch.empty(d, device=dev) for _ in range(3))
    dW, db = torch.empty((C, d), device=dev), torch.empty(C, device=dev)
    ws = torch.empty(lib.nv_head_step_workspace_bytes(B, d), dtype=torch.uint8, device=dev)
    return (logits, xh, st, loss, dl, g, g16, dgamma, dbeta, dW, db, dcol), ws


def head_step(x, gamma, beta, W, bias, labels, eps=1e-5, drop_seed=0, drop_p=0.0, path=NO_PATH, path_rows: int = 0, scale_state=None, opts=None):
    """nv_head_step: head forward + CrossEntropyLoss + head backward in two launches.  Returns what head_fwd, ce_loss and head_bwd return together:
    (logits, xh, st, loss, dlogits, g, g16, dgamma, dbeta, dW, db, dcol).  path given (None = NULL): nv_head_step_path, which also takes the
    scale_state / opts of nv_head_step_scaled / _soft."""
    B, n, d = x.shape
    C = W.shape[0]
    outs, ws = _head_step_outputs(B, n, d, C, x.device)
    logits, xh, st, loss, dl, g, g16, dgamma, dbeta, dW, db, dcol = outs
    if path is not NO_PATH:
        check(lib.nv_head_step_path(_p(x), n * d, B, d, _p(gamma), _p(beta), eps, _p(W), _p(bias), C, _p(labels), 1.0, _p(scale_state),
                                    None if opts is None else ctypes.byref(opts), _p(xh), _p(st), _p(logits), _p(loss), _p(dl), n, _p(g), d, _p(g16), d,
                                    _p(dgamma), _p(dbeta), _p(dW), _p(db), _p(dcol), 0, _p(ws), ws.numel(), drop_seed, drop_p, _stream(), _p(path), int(path_rows)),
              "nv_head_step_path")
        return outs
    check(lib.nv_head_step(_p(x), n * d, B, d, _p(gamma), _p(beta), eps, _p(W), _p(bias), C, _p(labels), 1.0, _p(xh), _p(st), _p(logits), _p(loss), _p(dl),
                           n, _p(g), d, _p(g16), d, _p(dgamma), _p(dbeta), _p(dW), _p(db), _p(dcol), 0, _p(ws), ws.numel(), drop_seed, drop_p, _stream()),
          "nv_head_step")
    return outs


def colsum_bf16(X: torch.Tensor, accumulate=False, out=None):
    M, N = X.shape
    out = torch.empty(N, device=X.device) if out is None else out
    nb = lib.nv_colsum_workspace_bytes(M, N)
    ws = torch.empty(nb, dtype=torch.uint8, device=X.device)
    check(lib.nv_colsum_bf16(_p(X), X.stride(0), M, N, _p(out), int(accumulate), _p(ws), nb, _stream()), "nv_colsum_bf16")
    return out


def ce_loss(logits: torch.Tensor, target: torch.Tensor, grad_scale: float = 1.0, want_grad=True, scale_state=None):
    B, C = logits.shape
    loss = torch.empty(1, device=logits.device)
    dl = torch.empty_like(logits) if want_grad else None
    check(lib.nv_ce_loss_scaled(_p(logits), _p(target), B, C, grad_scale, _p(scale_state), _p(loss), _p(dl), _stream()), "nv_ce_loss")
    return loss, dl


def loss_opts(label_smoothing: float = 0.0, class_weight: Optional[torch.Tensor] = None, mix: Optional[torch.Tensor] = None, B: Optional[int] = None,
              C: Optional[int] = None, device=None):
    """_cabi.LossOpts for the soft-target cross-entropy, or None when every option is off (the callers then make the calls they
    make without one).  class_weight: float32 [C] on the device; mix: int32 [B, 12] on the device (rows of nv_mix_params).  The
    tensors must outlive the call that reads them (the struct holds their addresses)."""
    from ._cabi import LossOpts, MIX_COLS
    if isinstance(label_smoothing, bool) or not isinstance(label_smoothing, (int, float)):
        raise TypeError(f"label_smoothing must be a number, got {label_smoothing!r}")
    if not (0.0 <= float(label_smoothing) < 1.0):
        raise ValueError(f"label_smoothing {label_smoothing} outside [0, 1)")
    if class_weight is not None:
        if not (torch.is_tensor(class_weight) and class_weight.dtype == torch.float32 and class_weight.dim() == 1 and class_weight.is_contiguous()):
            raise ValueError("class_weight must be a dense float32 vector [C]")
        if C is not None and class_weight.numel() != C:
            raise ValueError(f"class_weight has {class_weight.numel()} entries for {C} classes")
        if not class_weight.is_cuda or (device is not None and class_weight.device != torch.device(device)):
            raise RuntimeError("class_weight must live on the logits' MI355X (cuda) device - there is no CPU fallback")
    if mix is not None:
        if not (torch.is_tensor(mix) and mix.dtype == torch.int32 and mix.dim() == 2 and mix.shape[1] == MIX_COLS and mix.is_contiguous()):
            raise ValueError(f"mix must be a dense int32 [B, {MIX_COLS}] table (VolumeMix.params / last_mix)")
        if B is not None and mix.shape[0] != B:
            raise ValueError(f"mix has {mix.shape[0]} rows for a batch of {B}")
        if not mix.is_cuda or (device is not None and mix.device != torch.device(device)):
            raise RuntimeError("mix must live on the logits' MI355X (cuda) device - there is no CPU fallback")
    if float(label_smoothing) == 0.0 and class_weight is None and mix is None:
        return None
    return LossOpts(ctypes.sizeof(LossOpts), float(label_smoothing), _p(class_weight), _p(mix))


def ce_loss_soft(logits: torch.Tensor, target: torch.Tensor, label_smoothing: float = 0.0, class_weight: Optional[torch.Tensor] = None,
                 mix: Optional[torch.Tensor] = None, grad_scale: float = 1.0, want_grad=True, scale_state=None):
    """nv_ce_loss_soft: cross-entropy with label smoothing, class weights and a mixed target (the definition is in the header).
    With every option off it is ce_loss, bit for bit (the library hands the call over)."""
    B, C = logits.shape
    lo = loss_opts(label_smoothing, class_weight, mix, B, C, logits.device)
    loss = torch.empty(1, device=logits.device)
    dl = torch.empty_like(logits) if want_grad else None
    check(lib.nv_ce_loss_soft(_p(logits), _p(target), B, C, grad_scale, _p(scale_state), None if lo is None else ctypes.byref(lo), _p(loss), _p(dl),
                              _stream()), "nv_ce_loss_soft")
    return loss, dl


def reg_opts(kind: str = "mse", delta: float = 1.0, mean: Optional[torch.Tensor] = None, std: Optional[torch.Tensor] = None,
             weight: Optional[torch.Tensor] = None, mix: Optional[torch.Tensor] = None, B: Optional[int] = None, K: Optional[int] = None, device=None):
    """_cabi.RegOpts for the regression loss (the definition is in the header).  kind: "mse", "l1" or "huber" (delta > 0); mean / std / weight:
    float32 [K] on the device or None (0 / 1 / ones); mix: int32 [B, 12] on the device (rows of nv_mix_params).  The tensors must outlive the
    call that reads them (the struct holds their addresses)."""
    from ._cabi import REG_KINDS, MIX_COLS, RegOpts
    if kind not in REG_KINDS:
        raise ValueError(f"regression loss must be one of {sorted(REG_KINDS)}, got {kind!r}")
    if isinstance(delta, bool) or not isinstance(delta, (int, float)):
        raise TypeError(f"huber delta must be a number, got {delta!r}")
    if kind == "huber" and not float(delta) > 0.0:
        raise ValueError(f"huber delta must be > 0, got {delta}")
    for name, t in (("target_mean", mean), ("target_std", std), ("target_weight", weight)):
        if t is None:
            continue
        if not (torch.is_tensor(t) and t.dtype == torch.float32 and t.dim() == 1 and t.is_contiguous()):
            raise ValueError(f"{name} must be a dense float32 vector [K]")
        if K is not None and t.numel() != K:
            raise ValueError(f"{name} has {t.numel()} entries for {K} targets")
        if not t.is_cuda or (device is not None and t.device != torch.device(device)):
            raise RuntimeError(f"{name} must live on the predictions' MI355X (cuda) device - there is no CPU fallback")
    if mix is not None:
        if not (torch.is_tensor(mix) and mix.dtype == torch.int32 and mix.dim() == 2 and mix.shape[1] == MIX_COLS and mix.is_contiguous()):
            raise ValueError(f"mix must be a dense int32 [B, {MIX_COLS}] table (VolumeMix.params / last_mix)")
        if B is not None and mix.shape[0] != B:
            raise ValueError(f"mix has {mix.shape[0]} rows for a batch of {B}")
        if not mix.is_cuda or (device is not None and mix.device != torch.device(device)):
            raise RuntimeError("mix must live on the predictions' MI355X (cuda) device - there is no CPU fallback")
    return RegOpts(ctypes.sizeof(RegOpts), REG_KINDS[kind], float(delta), _p(mean), _p(std), _p(weight), _p(mix))


def reg_targets(target: torch.Tensor, B: int, K: int) -> torch.Tensor:
    """targets as the kernels read them: dense float32 [B, K] ([B] is [B, 1]); any real dtype is cast"""
    if not torch.is_tensor(target) or target.is_complex() or target.dtype == torch.bool:
        raise TypeError("regression targets must be a real-valued tensor")
    if target.dim() == 1 and K == 1:
        target = target.unsqueeze(1)
    if tuple(target.shape) != (B, K):
        raise ValueError(f"regression targets have shape {tuple(target.shape)}, the predictions are [{B}, {K}]")
    return target.to(torch.float32).contiguous()


def reg_loss(pred: torch.Tensor, target: torch.Tensor, opts=None, grad_scale: float = 1.0, want_grad=True, scale_state=None):
    """nv_reg_loss: the regression loss of a _cabi.RegOpts (reg_opts(...); None = plain mse) over pred / target float32 [B, K].
    Returns (loss [1], dpred or None)."""
    B, K = pred.shape
    ro = reg_opts() if opts is None else opts
    loss = torch.empty(1, device=pred.device)
    dp = torch.empty_like(pred) if want_grad else None
    check(lib.nv_reg_loss(_p(pred), _p(target), B, K, grad_scale, _p(scale_state), ctypes.byref(ro), _p(loss), _p(dp), _stream()), "nv_reg_loss")
    return loss, dp


def head_step_reg(x, gamma, beta, W, bias, targets, opts=None, eps=1e-5, grad_scale=1.0, scale_state=None, drop_seed=0, drop_p=0.0, path=None, path_rows: int = 0):
    """nv_head_step_reg: head_step with the regression loss over targets float32 [B, K].  Returns what head_step returns."""
    B, n, d = x.shape
    K = W.shape[0]
    ro = reg_opts() if opts is None else opts
    outs, ws = _head_step_outputs(B, n, d, K, x.device)
    logits, xh, st, loss, dl, g, g16, dgamma, dbeta, dW, db, dcol = outs
    check(lib.nv_head_step_reg(_p(x), n * d, B, d, _p(gamma), _p(beta), eps, _p(W), _p(bias), K, _p(targets), grad_scale, _p(scale_state), ctypes.byref(ro),
                               _p(xh), _p(st), _p(logits), _p(loss), _p(dl), n, _p(g), d, _p(g16), d, _p(dgamma), _p(dbeta), _p(dW), _p(db), _p(dcol), 0,
                               _p(ws), ws.numel(), drop_seed, drop_p, _stream(), _p(path), int(path_rows)), "nv_head_step_reg")
    return outs


class RegressionMetrics:
    """Validation metrics of a regression model on the RAW scale, accumulated on the device (nv_reg_metrics_*): update() makes one launch and
    no host read, compute() one launch and one read.  pred: the head's output [B, K] on the standardised scale (de-standardised with mean /
    std here); target: raw values, NaN = missing.  compute() -> {"n", "mae", "rmse", "bias", "r", "r2"}: float32 [K] tensors on the host."""

    def __init__(self, K: int, mean: Optional[torch.Tensor] = None, std: Optional[torch.Tensor] = None, device="cuda"):
        from ._cabi import REG_METRIC_SLOTS
        self.K, self.device = int(K), torch.device(device)
        if self.K < 1:
            raise ValueError(f"RegressionMetrics: K = {K}")
        if self.device.type != "cuda":
            raise RuntimeError("RegressionMetrics runs on the MI355X (cuda) device - there is no CPU fallback")

        def vec(t, name):
            if t is None:
                return None
            t = torch.as_tensor(t, dtype=torch.float32).reshape(-1).to(self.device).contiguous()
            if t.numel() != self.K:
                raise ValueError(f"RegressionMetrics: {name} has {t.numel()} entries for {self.K} targets")
            return t
        self.mean, self.std = vec(mean, "mean"), vec(std, "std")
        self.state = torch.zeros((self.K, REG_METRIC_SLOTS), dtype=torch.float64, device=self.device)

    def reset(self) -> None:
        self.state.zero_()

    def update(self, pred: torch.Tensor, target: torch.Tensor) -> None:
        if pred.dim() != 2 or pred.shape[1] != self.K or pred.dtype != torch.float32 or not pred.is_cuda:
            raise ValueError(f"RegressionMetrics.update: pred must be float32 [B, {self.K}] on the device")
        B = pred.shape[0]
        target = reg_targets(target, B, self.K).to(pred.device)
        check(lib.nv_reg_metrics_update(_p(pred.contiguous()), _p(target), B, self.K, _p(self.mean), _p(self.std), _p(self.state), _stream()), "nv_reg_metrics_update")

    def compute_device(self) -> torch.Tensor:
        """float32 [K, 6] on the device (n, MAE, RMSE, bias, r, R^2): no host read"""
        out = torch.empty((self.K, 6), device=self.device)
        check(lib.nv_reg_metrics_finish(_p(self.state), self.K, _p(out), _stream()), "nv_reg_metrics_finish")
        return out

    def compute(self) -> dict:
        from ._cabi import REG_METRIC_NAMES
        out = self.compute_device().cpu()          # the one host read
        return {name: out[:, i].clone() for i, name in enumerate(REG_METRIC_NAMES)}


def head_step_soft(x, gamma, beta, W, bias, labels, label_smoothing=0.0, class_weight=None, mix=None, eps=1e-5, grad_scale=1.0, scale_state=None):
    """nv_head_step_soft: head_step with the soft-target cross-entropy.  Returns what head_step returns."""
    B, n, d = x.shape
    C = W.shape[0]
    lo = loss_opts(label_smoothing, class_weight, mix, B, C, x.device)
    outs, ws = _head_step_outputs(B, n, d, C, x.device)
    logits, xh, st, loss, dl, g, g16, dgamma, dbeta, dW, db, dcol = outs
    check(lib.nv_head_step_soft(_p(x), n * d, B, d, _p(gamma), _p(beta), eps, _p(W), _p(bias), C, _p(labels), grad_scale, _p(scale_state),
                                None if lo is None else ctypes.byref(lo), _p(xh), _p(st), _p(logits), _p(loss), _p(dl), n, _p(g), d, _p(g16), d, _p(dgamma),
                                _p(dbeta), _p(dW), _p(db), _p(dcol), 0, _p(ws), ws.numel(), 0, 0.0, _stream()), "nv_head_step_soft")
    return outs


def adamw_step(p, grad, m, v, p16, step, lr, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, grad_scale=1.0, max_blocks=0, scale_state=None,
               clip_state=None):
    """grad may be fp32 or the 16-bit operand format (same numel as p).  scale_state: device block of a dynamic loss scale
    (optim.LossScaler.state) - the launch then does nothing when that step is skipped, un-scales the gradients and takes the step
    count / bias corrections from the block (`step` is ignored).  clip_state: device block of optim.GradClipper - the gradients are
    also multiplied by the clipping coefficient it holds (nv_adamw_step_clipped)."""
    assert grad.dtype in (torch.float32, op16()) and grad.numel() == p.numel()
    if clip_state is None:
        check(lib.nv_adamw_step_scaled(_p(p), _p(grad), int(grad.dtype == op16()), _p(m), _p(v), _p(p16), p.numel(), max(int(step), 1), lr, betas[0], betas[1],
                                       eps, weight_decay, grad_scale, int(max_blocks), _p(scale_state), _stream()), "nv_adamw_step")
    else:
        check(lib.nv_adamw_step_clipped(_p(p), _p(grad), int(grad.dtype == op16()), _p(m), _p(v), _p(p16), p.numel(), max(int(step), 1), lr, betas[0], betas[1],
                                        eps, weight_decay, grad_scale, int(max_blocks), _p(scale_state), _p(clip_state), _stream()), "nv_adamw_step_clipped")


class AdamwSegments:
    """The static half of nv_adamw_step_grouped's table, on the device: segment s covers the arena elements [ends[s-1], ends[s]) and
    belongs to group groups[s].  The library validates the lists (RuntimeError for anything it refuses) and uploads them once, here;
    `table` is the device buffer, owned by this object and forgotten by the library when it goes."""

    def __init__(self, ends, groups, n_groups: int, count: int, device):
        ends, groups = [int(e) for e in ends], [int(g) for g in groups]
        if len(ends) != len(groups):
            raise ValueError(f"AdamwSegments: {len(ends)} ends, {len(groups)} group indices")
        self.n_segments, self.n_groups, self.count = len(ends), int(n_groups), int(count)
        nbytes = lib.nv_adamw_segments_bytes(self.n_segments)
        self.table = torch.empty(max(int(nbytes), 16), dtype=torch.uint8, device=device)
        e = (ctypes.c_long * max(self.n_segments, 1))(*ends)
        g = (ctypes.c_int * max(self.n_segments, 1))(*groups)
        check(lib.nv_adamw_segments_build(self.table.data_ptr(), self.table.numel(), e, g, self.n_segments, self.n_groups, self.count, _stream()),
              "nv_adamw_segments_build")

    def __del__(self):
        try:
            lib.nv_adamw_segments_release(self.table.data_ptr())
        except Exception:
            pass


def adamw_step_grouped(p, grad, m, v, p16, step, segments: AdamwSegments, lrs, weight_decays, betas=(0.9, 0.999), eps=1e-8, grad_scale=1.0, max_blocks=0,
                       scale_state=None, clip_state=None):
    """adamw_step whose lr and weight_decay come per parameter group (nv_adamw_step_grouped): element i of segment s is updated with
    lrs[g], weight_decays[g], g = the segment's group - the bits adamw_step gives it when called with that pair.  Every other
    argument as in adamw_step; `segments` is the AdamwSegments of this arena."""
    from ._cabi import AdamwGroups
    _need_cuda(p, grad, m, v, p16, scale_state, clip_state)
    assert grad.dtype in (torch.float32, op16()) and grad.numel() == p.numel()
    if len(lrs) != len(weight_decays) or not 1 <= len(lrs) <= len(AdamwGroups().lr):
        raise ValueError(f"adamw_step_grouped: {len(lrs)} learning rates and {len(weight_decays)} weight decays, 1 .. {len(AdamwGroups().lr)} pairs are supported")
    tab = AdamwGroups(ctypes.sizeof(AdamwGroups), len(lrs), segments.table.data_ptr())
    for i, (lr, wd) in enumerate(zip(lrs, weight_decays)):
        tab.lr[i], tab.weight_decay[i] = float(lr), float(wd)
    check(lib.nv_adamw_step_grouped(_p(p), _p(grad), int(grad.dtype == op16()), _p(m), _p(v), _p(p16), p.numel(), max(int(step), 1), ctypes.byref(tab),
                                    betas[0], betas[1], eps, float(grad_scale), int(max_blocks), _p(scale_state), _p(clip_state), _stream()),
          "nv_adamw_step_grouped")


def ema_update(ema: torch.Tensor, p: torch.Tensor, weight: float, max_blocks: int = 0) -> None:
    """ema = ema + (p - ema) * weight in place, each fp32 operation rounded on its own (nv_ema_update): bit-equal to that torch expression
    on the CPU, and p == ema is an exact fixed point.  Both flat fp32, contiguous, the same numel (a multiple of 4) and 16-byte aligned;
    0 <= weight <= 1 - the library refuses anything else before the launch.  `p` is only read."""
    _need_cuda(ema, p)
    assert ema.dtype == torch.float32 and p.dtype == torch.float32 and ema.is_contiguous() and p.is_contiguous() and ema.numel() == p.numel()
    check(lib.nv_ema_update(_p(ema), _p(p), ema.numel(), float(weight), int(max_blocks), _stream()), "nv_ema_update")


GRAD_CLIP_FLOATS = (64 + 8 * 2048) // 4     # NV_GRAD_CLIP_BYTES / 4 (include/neurovit_hip.h)
GC_TOTAL_NORM, GC_COEF = 2, 3                # float indices into that block (csrc/common.h GC_*)


def grad_sumsq(grad: torch.Tensor, clip_state: torch.Tensor, scale_state: Optional[torch.Tensor] = None, max_blocks: int = 0) -> None:
    """clip_state's running sum of squares += sum of grad ** 2, summed in double (nv_grad_sumsq).  grad: contiguous, fp32 or the
    16-bit operand format, any element alignment.  scale_state: found_inf is raised when the sum is not finite."""
    _need_cuda(grad, clip_state, scale_state)
    assert grad.dtype in (torch.float32, op16()) and grad.is_contiguous()
    assert clip_state.dtype == torch.float32 and clip_state.numel() >= GRAD_CLIP_FLOATS and clip_state.is_contiguous()
    if grad.numel():
        check(lib.nv_grad_sumsq(_p(grad), int(grad.dtype != torch.float32), grad.numel(), _p(clip_state), _p(scale_state), int(max_blocks), _stream()),
              "nv_grad_sumsq")


def grad_clip_finish(clip_state: torch.Tensor, max_norm: float, grad_scale: float = 1.0, scale_state: Optional[torch.Tensor] = None) -> None:
    """total_norm and coef of the gradients summed since the last call (nv_grad_clip_finish); clears the running sum."""
    _need_cuda(clip_state, scale_state)
    check(lib.nv_grad_clip_finish(_p(clip_state), float(max_norm), float(grad_scale), _p(scale_state), _stream()), "nv_grad_clip_finish")


def loss_scale_init(state: torch.Tensor, init_scale=65536.0, growth_factor=2.0, backoff_factor=0.5, growth_interval=2000, start_step=0) -> None:
    assert state.is_cuda and state.dtype == torch.float32 and state.numel() >= 16 and state.is_contiguous()
    check(lib.nv_loss_scale_init(_p(state), float(init_scale), float(growth_factor), float(backoff_factor), int(growth_interval), int(start_step), _stream()),
          "nv_loss_scale_init")


def loss_scale_check(grads: torch.Tensor, state: torch.Tensor) -> None:
    """state[found_inf] |= any inf / NaN in the fp32 tensor `grads` (contiguous)."""
    assert grads.is_cuda and grads.dtype == torch.float32 and grads.is_contiguous()
    if grads.numel():
        check(lib.nv_loss_scale_check(_p(grads), grads.numel(), _p(state), _stream()), "nv_loss_scale_check")


def loss_scale_update(state: torch.Tensor, lr: float, betas) -> None:
    check(lib.nv_loss_scale_update(_p(state), float(lr), float(betas[0]), float(betas[1]), _stream()), "nv_loss_scale_update")


def cast_bf16(src: torch.Tensor, ld_dst: Optional[int] = None, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """fp32 [rows, cols] -> bf16 [rows, ld_dst] (zero padded columns)."""
    _need_cuda(src)
    rows, cols = src.shape
    if out is not None:
        ld_dst = out.stride(0) if rows > 1 else out.shape[1]
    ld_dst = (cols + 3) // 4 * 4 if ld_dst is None else ld_dst
    dst = torch.empty((rows, ld_dst), dtype=op16(), device=src.device) if out is None else out
    check(lib.nv_cast_bf16_2d(_p(src), src.stride(0), rows, cols, _p(dst), ld_dst, _stream()), "nv_cast_bf16_2d")
    return dst


def copy_2d_f32(src: torch.Tensor, dst: torch.Tensor, accumulate: bool = False) -> torch.Tensor:
    """dst[rows, cols] (+)= src[rows, cols], both f32 and row-strided (nv_copy_2d_f32)."""
    _need_cuda(src, dst)
    assert src.dtype == torch.float32 and dst.dtype == torch.float32 and src.shape == dst.shape and src.stride(1) == 1 and dst.stride(1) == 1
    rows, cols = src.shape
    check(lib.nv_copy_2d_f32(_p(src), src.stride(0), rows, cols, _p(dst), dst.stride(0), int(bool(accumulate)), _stream()), "nv_copy_2d_f32")
    return dst


def gradcam_reduce(act: torch.Tensor, grad: torch.Tensor):
    """act bf16 [B, n, d], grad f32 [B, n, d] (device) -> (cam f32 [B, n-1] min-max normalised, minmax f32 [2]); one launch."""
    _need_cuda(act, grad)
    assert act.dtype == op16() and grad.dtype == torch.float32 and act.shape == grad.shape and act.is_contiguous() and grad.is_contiguous()
    B, n, d = act.shape
    cam = torch.empty((B, n - 1), dtype=torch.float32, device=act.device)
    mm = torch.empty(2, dtype=torch.float32, device=act.device)
    nb = lib.nv_gradcam_workspace_bytes(B, n)
    ws = torch.empty(nb, dtype=torch.uint8, device=act.device)
    check(lib.nv_gradcam_reduce(_p(act), _p(grad), B, n, d, _p(cam), _p(mm), _p(ws), nb, _stream()), "nv_gradcam_reduce")
    return cam, mm


def gradcam_reduce_per_volume(act: torch.Tensor, grad: torch.Tensor):
    """gradcam_reduce with every volume normalised over its own cells: act 16-bit [B, n, d], grad f32 [B, n, d] (device) ->
    (cam f32 [B, n-1], minmax f32 [B, 2]); volume b has the bits of gradcam_reduce on that volume alone.  One launch."""
    _need_cuda(act, grad)
    assert act.dtype == op16() and grad.dtype == torch.float32 and act.shape == grad.shape and act.is_contiguous() and grad.is_contiguous()
    B, n, d = act.shape
    cam = torch.empty((B, n - 1), dtype=torch.float32, device=act.device)
    mm = torch.empty((B, 2), dtype=torch.float32, device=act.device)
    nb = lib.nv_gradcam_per_volume_workspace_bytes(B, n)
    ws = torch.empty(max(nb, 16), dtype=torch.uint8, device=act.device)
    check(lib.nv_gradcam_reduce_per_volume(_p(act), _p(grad), B, n, d, _p(cam), _p(mm), _p(ws), nb, _stream()), "nv_gradcam_reduce_per_volume")
    return cam, mm


def _int3_ptr(t):
    """three C ints for a `const int*` argument: (the array, which the caller holds for the duration of the call, a void pointer to it)"""
    a = (ctypes.c_int * 3)(*t)
    return a, ctypes.cast(a, ctypes.c_void_p)


def _triple(v, what):
    t = (int(v),) * 3 if isinstance(v, int) else tuple(int(e) for e in v)
    if len(t) != 3:
        raise ValueError(f"neurovit_amd: {what} must be an int or three ints, got {v!r}")
    return t


def token_maps_to_volumes(maps: torch.Tensor, grid, size, normalize: bool = True, keep_percent: float = 100.0, return_maps: bool = False,
                          out: Optional[torch.Tensor] = None):
    """maps f32 [B, G0*G1*G2] (device, token order) -> volumes f32 [B, S0, S1, S2]; grid / size: an int (cubic) or three.  Per volume:
    min-max normalisation (normalize), the keep_percent % largest cells kept by torch.quantile's linear rule, trilinear upsampling
    (align_corners=False): nv_token_map_to_volume, two launches.  return_maps: also (normalised maps [B, N], thresholded maps [B, N],
    cuts [B]) - views of the call's workspace."""
    _need_cuda(maps)
    grid, size = _triple(grid, "grid"), _triple(size, "size")
    N = grid[0] * grid[1] * grid[2]
    assert maps.dim() == 2 and maps.shape[1] == N and maps.dtype == torch.float32 and maps.is_contiguous()
    B = maps.shape[0]
    (g3, g3p), (s3, s3p) = _int3_ptr(grid), _int3_ptr(size)
    nb = lib.nv_token_map_to_volume_workspace_bytes(B, g3p)
    if nb < 0:
        raise ValueError(f"neurovit_amd: token_maps_to_volumes needs a non-empty batch and a positive grid, got B = {B}, grid = {grid}")
    ws = torch.empty(nb // 4, dtype=torch.float32, device=maps.device)
    if out is None:
        out = torch.empty((B,) + size, dtype=torch.float32, device=maps.device)
    assert out.shape == (B,) + size and out.dtype == torch.float32 and out.is_contiguous() and out.device == maps.device
    check(lib.nv_token_map_to_volume(_p(maps), B, g3p, s3p, int(bool(normalize)), float(keep_percent), _p(out), _p(ws), nb, _stream()),
          "nv_token_map_to_volume")
    if not return_maps:
        return out
    return out, (ws[:B * N].view(B, N), ws[B * N:2 * B * N].view(B, N), ws[2 * B * N:])


SERIES_SCOPES = {"series": 0, "volume": 1}      # NV_SERIES_SCOPE_SERIES / NV_SERIES_SCOPE_VOLUME
SERIES_LAYOUTS = {"series": 0, "frames": 1}     # NV_SERIES_LAYOUT_SERIES / NV_SERIES_LAYOUT_FRAMES
SERIES_MAX_TIMEPOINTS = 64                      # csrc/series_attr.hip: SS_MAX_T
SERIES_MAX_CELLS = 32768                        # SS_MAX_CELLS: T * N cells of one sample under scope "series"


def gradcam_reduce_grouped(act: torch.Tensor, grad: torch.Tensor, group: int):
    """gradcam_reduce with the min-max taken over every `group` consecutive volumes (a sample's T timepoints): act 16-bit [V, n, d],
    grad f32 [V, n, d] (device) -> (cam f32 [V, n-1], minmax f32 [V / group, 2]).  group = 1 has the bits of gradcam_reduce_per_volume,
    group = V those of gradcam_reduce.  nv_gradcam_reduce_grouped, one launch."""
    _need_cuda(act, grad)
    assert act.dtype == op16() and grad.dtype == torch.float32 and act.shape == grad.shape and act.is_contiguous() and grad.is_contiguous()
    V, n, d = act.shape
    nb = lib.nv_gradcam_grouped_workspace_bytes(V, n, int(group))
    if nb < 0:
        raise ValueError(f"neurovit_amd: gradcam_reduce_grouped: {V} volumes are no whole number of groups of {group}")
    cam = torch.empty((V, n - 1), dtype=torch.float32, device=act.device)
    mm = torch.empty((V // int(group), 2), dtype=torch.float32, device=act.device)
    ws = torch.empty(max(nb, 16), dtype=torch.uint8, device=act.device)
    check(lib.nv_gradcam_reduce_grouped(_p(act), _p(grad), V, n, d, int(group), _p(cam), _p(mm), _p(ws), nb, _stream()), "nv_gradcam_reduce_grouped")
    return cam, mm


def series_maps_to_volumes(maps: torch.Tensor, grid, size, normalize: bool = True, scope: str = "series", keep_percent: float = 100.0,
                           layout: str = "series", return_maps: bool = False, out: Optional[torch.Tensor] = None):
    """maps f32 [B, T, G0*G1*G2] (device, token order per timepoint) -> volumes f32 [B, S0, S1, S2, T] (layout "series": time innermost, as
    the model's input) or [B, T, S0, S1, S2] (layout "frames"); grid / size: an int (cubic) or three.  token_maps_to_volumes with the
    normalisation and the percentile cut taken over the sample's T N cells jointly (scope "series": one min, max and cut per sample) or
    over every volume on its own (scope "volume").  nv_series_map_to_volumes, two launches.  return_maps: also (normalised maps [B, T, N],
    thresholded maps [B, T, N], cuts [B] or [B, T]) - views of the call's workspace."""
    _need_cuda(maps)
    if scope not in SERIES_SCOPES or layout not in SERIES_LAYOUTS:
        raise ValueError(f"neurovit_amd: series_maps_to_volumes: scope must be 'series' or 'volume' and layout 'series' or 'frames', got {scope!r}, {layout!r}")
    grid, size = _triple(grid, "grid"), _triple(size, "size")
    N = grid[0] * grid[1] * grid[2]
    assert maps.dim() == 3 and maps.shape[2] == N and maps.dtype == torch.float32 and maps.is_contiguous()
    B, T = maps.shape[:2]
    (g3, g3p), (s3, s3p) = _int3_ptr(grid), _int3_ptr(size)
    nb = lib.nv_series_map_to_volumes_workspace_bytes(B, T, g3p, SERIES_SCOPES[scope])
    if nb < 0:
        raise ValueError(f"neurovit_amd: series_maps_to_volumes needs a non-empty batch, 1 .. {SERIES_MAX_TIMEPOINTS} timepoints and a positive grid, "
                         f"got B = {B}, T = {T}, grid = {grid}")
    ws = torch.empty(nb // 4, dtype=torch.float32, device=maps.device)
    shape = (B,) + size + (T,) if layout == "series" else (B, T) + size
    if out is None:
        out = torch.empty(shape, dtype=torch.float32, device=maps.device)
    assert out.shape == shape and out.dtype == torch.float32 and out.is_contiguous() and out.device == maps.device
    check(lib.nv_series_map_to_volumes(_p(maps), B, T, g3p, s3p, int(bool(normalize)), SERIES_SCOPES[scope], float(keep_percent), SERIES_LAYOUTS[layout],
                                       _p(out), _p(ws), nb, _stream()), "nv_series_map_to_volumes")
    if not return_maps:
        return out
    V = B * T
    return out, (ws[:V * N].view(B, T, N), ws[V * N:2 * V * N].view(B, T, N), ws[2 * V * N:] if scope == "series" else ws[2 * V * N:].view(B, T))


def series_leave_one_out(z: torch.Tensor, z_base: torch.Tensor) -> torch.Tensor:
    """z f32 [B, T, 2], z_base f32 [2] (device) -> f32 [B (T + 1), T, 2]: row b (T + 1) is z[b], row b (T + 1) + 1 + t is z[b] with timepoint t
    replaced by z_base - the sequences of temporal occlusion, a pure select.  nv_series_leave_one_out, one launch."""
    _need_cuda(z, z_base)
    assert z.dim() == 3 and z.shape[2] == 2 and z.dtype == torch.float32 and z.is_contiguous()
    assert z_base.shape == (2,) and z_base.dtype == torch.float32 and z_base.is_contiguous()
    B, T, _ = z.shape
    out = torch.empty((B * (T + 1), T, 2), dtype=torch.float32, device=z.device)
    check(lib.nv_series_leave_one_out(_p(z), _p(z_base), B, T, _p(out), _stream()), "nv_series_leave_one_out")
    return out


def temporal_grad_x_input(dx: torch.Tensor, z: torch.Tensor) -> torch.Tensor:
    """dx, z f32 [B, T, 2] (device) -> f32 [B, T] = sum_c dx[b, t, c] z[b, t, c], every product and the sum rounded on its own: the bits of
    (dx * z).sum(-1).  nv_temporal_grad_x_input, one launch."""
    _need_cuda(dx, z)
    assert z.dim() == 3 and z.shape[2] == 2 and dx.shape == z.shape and dx.dtype == z.dtype == torch.float32 and dx.is_contiguous() and z.is_contiguous()
    B, T, _ = z.shape
    out = torch.empty((B, T), dtype=torch.float32, device=z.device)
    check(lib.nv_temporal_grad_x_input(_p(dx), _p(z), B, T, _p(out), _stream()), "nv_temporal_grad_x_input")
    return out


SCORE_KINDS = {"prob": 0, "logit": 1}      # NV_SCORE_PROB / NV_SCORE_LOGIT


def token_ranks(maps: torch.Tensor) -> torch.Tensor:
    """maps f32 [B, N] (device, finite, N <= 4096) -> ranks int32 [B, N]: the position of every token in the descending order of its
    volume's map, ties to the lower token index (-0.0 == +0.0) - the inverse of torch.sort(descending=True, stable=True).indices.  One launch."""
    _need_cuda(maps)
    assert maps.dim() == 2 and maps.dtype == torch.float32 and maps.is_contiguous()
    B, N = maps.shape
    ranks = torch.empty((B, N), dtype=torch.int32, device=maps.device)
    check(lib.nv_token_ranks(_p(maps), B, N, _p(ranks), _stream()), "nv_token_ranks")
    return ranks


def mask_patches(x: torch.Tensor, labels: torch.Tensor, jobs: torch.Tensor, patch, baseline=0.0, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """x f32 [B, S0, S1, S2] (NeuroEncoder.forward's layout), labels int32 [B, N], jobs int32 [J, 3] of rows (b, lo, hi), all on the device
    -> f32 [J, S0, S1, S2]: copy j is x[b] with every patch whose label lies in [lo, hi) replaced by the baseline - a float, or a tensor of
    x's shape (one volume per source volume) or [1, S0, S1, S2] (shared).  patch: an int or three.  Tokens are numbered as the engine's
    patch gather numbers them.  A pure select (bits pass through); a job with b outside [0, B) leaves its slot of `out` as it was.
    nv_mask_patches, one launch."""
    _need_cuda(x, labels, jobs, out, baseline if torch.is_tensor(baseline) else None)
    patch = _triple(patch, "patch")
    assert x.dim() == 4 and x.dtype == torch.float32 and x.is_contiguous()
    B, size = x.shape[0], tuple(x.shape[1:])
    if any(s % p for s, p in zip(size, patch)):
        raise ValueError(f"neurovit_amd: mask_patches: volume {size} is not a whole number of {patch} patches")
    N = (size[0] // patch[0]) * (size[1] // patch[1]) * (size[2] // patch[2])
    assert labels.shape == (B, N) and labels.dtype == torch.int32 and labels.is_contiguous()
    assert jobs.dim() == 2 and jobs.shape[1] == 3 and jobs.dtype == torch.int32 and jobs.is_contiguous()
    J = jobs.shape[0]
    value, base, stride = _path_baseline("mask_patches", baseline, x.shape)
    if out is None:
        out = torch.empty((J,) + size, dtype=torch.float32, device=x.device)
    assert out.shape == (J,) + size and out.dtype == torch.float32 and out.is_contiguous() and out.device == x.device
    (s3, s3p), (p3, p3p) = _int3_ptr(size), _int3_ptr(patch)
    check(lib.nv_mask_patches(_p(x), B, s3p, p3p, _p(labels), _p(jobs), J, value, _p(base), stride, _p(out), _stream()), "nv_mask_patches")
    return out


def class_scores(logits: torch.Tensor, jobs: torch.Tensor, cls: torch.Tensor, kind: str = "prob") -> torch.Tensor:
    """logits f32 [J, C], jobs int32 [J, 3] (column 0: the source volume b_j), cls int64 [B] -> f32 [J]: the score of class cls[b_j] in row
    j - "logit": the logit itself, bit for bit; "prob": its softmax probability in fp32.  nv_class_scores, one launch."""
    _need_cuda(logits, jobs, cls)
    if kind not in SCORE_KINDS:
        raise ValueError(f"neurovit_amd: class_scores: kind must be 'prob' or 'logit', got {kind!r}")
    assert logits.dim() == 2 and logits.dtype == torch.float32 and logits.is_contiguous()
    J, C = logits.shape
    assert jobs.shape == (J, 3) and jobs.dtype == torch.int32 and jobs.is_contiguous()
    assert cls.dim() == 1 and cls.dtype == torch.int64 and cls.is_contiguous()
    scores = torch.empty(J, dtype=torch.float32, device=logits.device)
    check(lib.nv_class_scores(_p(logits), J, C, _p(jobs), _p(cls), cls.shape[0], SCORE_KINDS[kind], _p(scores), _stream()), "nv_class_scores")
    return scores


def curve_auc(scores: torch.Tensor) -> torch.Tensor:
    """scores f32 [B, K] (rows may be strided, K >= 2) -> f32 [B]: the trapezoid area under each curve on the uniform grid k / (K - 1),
    summed in double.  nv_curve_auc, one launch."""
    _need_cuda(scores)
    assert scores.dim() == 2 and scores.dtype == torch.float32 and scores.stride(1) == 1
    B, K = scores.shape
    auc = torch.empty(B, dtype=torch.float32, device=scores.device)
    check(lib.nv_curve_auc(_p(scores), B, K, scores.stride(0) if B > 1 else K, _p(auc), _stream()), "nv_curve_auc")
    return auc


def occlusion_gather(ref: torch.Tensor, scores: torch.Tensor, labels: torch.Tensor) -> torch.Tensor:
    """ref f32 [B], scores f32 [B, NB], labels int32 [B, N] -> f32 [B, N]: ref[b] - scores[b, labels[b, t]].  nv_occlusion_gather, one launch."""
    _need_cuda(ref, scores, labels)
    B, NB = scores.shape
    assert ref.shape == (B,) and labels.dim() == 2 and labels.shape[0] == B and labels.dtype == torch.int32
    assert ref.dtype == torch.float32 and scores.dtype == torch.float32 and ref.is_contiguous() and scores.is_contiguous() and labels.is_contiguous()
    maps = torch.empty(labels.shape, dtype=torch.float32, device=scores.device)
    check(lib.nv_occlusion_gather(_p(ref), _p(scores), _p(labels), B, labels.shape[1], NB, _p(maps), _stream()), "nv_occlusion_gather")
    return maps


SHAPLEY_MAX_PLAYERS = 4096


def mask_patches_rows(x: torch.Tensor, labels: torch.Tensor, jobs: torch.Tensor, patch, baseline=0.0, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """mask_patches with labels int32 [Rows, N] and jobs int32 [J, 4] of rows (b, row, lo, hi): copy j is x[b] with every patch whose label
    in row `row` lies in [lo, hi) replaced by the baseline - many labellings of one volume in one call.  A job with b outside [0, B) or row
    outside [0, Rows) leaves its slot of `out` as it was.  nv_mask_patches_rows (the kernel body of nv_mask_patches), one launch."""
    _need_cuda(x, labels, jobs, out, baseline if torch.is_tensor(baseline) else None)
    patch = _triple(patch, "patch")
    assert x.dim() == 4 and x.dtype == torch.float32 and x.is_contiguous()
    B, size = x.shape[0], tuple(x.shape[1:])
    if any(s % p for s, p in zip(size, patch)):
        raise ValueError(f"neurovit_amd: mask_patches_rows: volume {size} is not a whole number of {patch} patches")
    N = (size[0] // patch[0]) * (size[1] // patch[1]) * (size[2] // patch[2])
    assert labels.dim() == 2 and labels.shape[1] == N and labels.dtype == torch.int32 and labels.is_contiguous()
    assert jobs.dim() == 2 and jobs.shape[1] == 4 and jobs.dtype == torch.int32 and jobs.is_contiguous()
    J = jobs.shape[0]
    value, base, stride = _path_baseline("mask_patches_rows", baseline, x.shape)
    if out is None:
        out = torch.empty((J,) + size, dtype=torch.float32, device=x.device)
    assert out.shape == (J,) + size and out.dtype == torch.float32 and out.is_contiguous() and out.device == x.device
    (s3, s3p), (p3, p3p) = _int3_ptr(size), _int3_ptr(patch)
    check(lib.nv_mask_patches_rows(_p(x), B, s3p, p3p, _p(labels), labels.shape[0], _p(jobs), J, value, _p(base), stride, _p(out), _stream()),
          "nv_mask_patches_rows")
    return out


def shapley_ranks(U: int, R: int, B: int, F: int, seed: int = 0, first_unit: int = 0, device="cuda", out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """-> ranks int32 [U R, B, F] on the device: for each of the units first_unit .. first_unit + U - 1 and each sample a random permutation
    of the F players (row u R of the unit; the draw rule is in the header, tests/shapley_ref.py restates it) and, with R = 2, its
    antithetic permutation F - 1 - rank behind it.  nv_shapley_ranks, one launch; nothing is read back."""
    if R not in (1, 2) or not 2 <= F <= SHAPLEY_MAX_PLAYERS or U < 1 or B < 1:
        raise ValueError(f"neurovit_amd: shapley_ranks: needs U, B >= 1, R in (1, 2) and 2 <= F <= {SHAPLEY_MAX_PLAYERS}, got U {U}, R {R}, B {B}, F {F}")
    if out is None:
        out = torch.empty((U * R, B, F), dtype=torch.int32, device=device)
    _need_cuda(out)
    assert out.shape == (U * R, B, F) and out.dtype == torch.int32 and out.is_contiguous()
    check(lib.nv_shapley_ranks(int(seed) & (2 ** 64 - 1), int(first_unit), U, R, B, F, _p(out), _stream()), "nv_shapley_ranks")
    return out


def shapley_labels(ranks: torch.Tensor, features: torch.Tensor) -> torch.Tensor:
    """ranks int32 [Q, B, F] (or [Q B, F]: row q of volume q mod B), features int32 [B, N] of player ids (outside [0, F), by convention -1: no
    player) -> labels int32 [Q B, N]: the rank of every patch's player in that row, F for a patch of no player.  nv_shapley_labels, one launch."""
    _need_cuda(ranks, features)
    assert features.dim() == 2 and features.dtype == torch.int32 and features.is_contiguous()
    B, N = features.shape
    assert ranks.dtype == torch.int32 and ranks.is_contiguous() and ranks.dim() in (2, 3)
    F = ranks.shape[-1]
    rows = ranks.numel() // F
    assert rows % B == 0 and (ranks.dim() == 2 or ranks.shape[1] == B)
    labels = torch.empty((rows, N), dtype=torch.int32, device=ranks.device)
    check(lib.nv_shapley_labels(_p(ranks), _p(features), rows, B, F, N, _p(labels), _stream()), "nv_shapley_labels")
    return labels


def shapley_accumulate(interior: torch.Tensor, ends: torch.Tensor, ranks: torch.Tensor, R: int = 1):
    """interior f32 [U R, B, F - 1] (the score with the k = 1 .. F - 1 first-ranked players of each permutation present), ends f32 [B, 2]
    (nothing present, everything present), ranks int32 [U R, B, F] -> (values f32 [B, F], stderr f32 [B, F], delta f32 [B], sums f64
    [B, F, 2]): the mean over the U units of every player's marginal contribution (a unit: one permutation, or the mean of an antithetic
    pair), its standard error (NaN for U = 1), the efficiency residual sum_f value_f - (full - empty), and the double sums behind them.
    nv_shapley_accumulate; nothing is read back."""
    _need_cuda(interior, ends, ranks)
    assert ranks.dim() == 3 and ranks.dtype == torch.int32 and ranks.is_contiguous() and R in (1, 2)
    Q, B, F = ranks.shape
    assert Q % R == 0 and F >= 2
    assert interior.shape == (Q, B, F - 1) and interior.dtype == torch.float32 and interior.is_contiguous()
    assert ends.shape == (B, 2) and ends.dtype == torch.float32 and ends.is_contiguous()
    dev = ranks.device
    values, err = torch.empty((B, F), dtype=torch.float32, device=dev), torch.empty((B, F), dtype=torch.float32, device=dev)
    delta, sums = torch.empty(B, dtype=torch.float32, device=dev), torch.empty((B, F, 2), dtype=torch.float64, device=dev)
    check(lib.nv_shapley_accumulate(_p(interior), _p(ends), _p(ranks), Q // R, R, B, F, _p(values), _p(err), _p(delta), _p(sums), _stream()),
          "nv_shapley_accumulate")
    return values, err, delta, sums


def shapley_token_maps(values: torch.Tensor, features: torch.Tensor) -> torch.Tensor:
    """values f32 [B, F], features int32 [B, N] -> maps f32 [B, N]: a patch of player f gets values[b, f] / (patches of f in volume b), a patch
    of no player 0 - the map sums to the values; what token_maps_to_volumes and perturbation_curves take.  nv_shapley_token_maps, one launch."""
    _need_cuda(values, features)
    assert values.dim() == 2 and values.dtype == torch.float32 and values.is_contiguous()
    B, F = values.shape
    assert features.dim() == 2 and features.shape[0] == B and features.dtype == torch.int32 and features.is_contiguous()
    maps = torch.empty(features.shape, dtype=torch.float32, device=values.device)
    check(lib.nv_shapley_token_maps(_p(values), _p(features), B, F, features.shape[1], _p(maps), _stream()), "nv_shapley_token_maps")
    return maps


def _rows(t: torch.Tensor, rows: Optional[int] = None, V: Optional[int] = None) -> bool:
    """t is a dense fp32 [rows, V] device buffer (one row after the other)"""
    return (t.dim() == 2 and t.dtype == torch.float32 and t.stride(1) == 1 and (t.shape[0] == 1 or t.stride(0) == t.shape[1])
            and (rows is None or t.shape[0] == rows) and (V is None or t.shape[1] == V))


def check_baseline(what: str, baseline, shape):
    """A baseline is a float, or a tensor of `shape` (one per sample) or of (1,) + shape[1:] (shared): returns the float or the tensor,
    ValueError for a tensor of any other shape."""
    if not torch.is_tensor(baseline):
        return float(baseline)
    full, shared = tuple(shape), (1,) + tuple(shape[1:])
    if tuple(baseline.shape) not in (full, shared):
        raise ValueError(f"{what}: baseline of shape {tuple(baseline.shape)}, expected {full} or {shared}")
    return baseline


def _path_baseline(what: str, baseline, shape):
    """(value, base tensor or None, stride in elements) for the kernels that take a baseline (check_baseline) of dense fp32 samples"""
    baseline = check_baseline(f"neurovit_amd: {what}", baseline, shape)
    if not torch.is_tensor(baseline):
        return baseline, None, 0
    assert baseline.dtype == torch.float32 and baseline.is_contiguous()
    B = shape[0]
    return 0.0, baseline, (baseline[0].numel() if baseline.shape[0] == B and B > 1 else 0)


def path_points(x: torch.Tensor, jobs: torch.Tensor, alphas: torch.Tensor, baseline=0.0, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """x f32 [B, V] (every sample as V dense floats), jobs int32 [J, 2] of rows (b, k), alphas f32 [K], all on the device -> f32 [J, V]:
    point j is bl + alphas[k] * (x[b] - bl), three separately rounded fp32 operations (the bits of that torch expression on the CPU).
    baseline: a float, or a tensor [B, V] (one per source volume) or [1, V] (shared).  A job with b or k out of range leaves its row of
    `out` as it was.  nv_path_points, one launch."""
    _need_cuda(x, jobs, alphas, out, baseline if torch.is_tensor(baseline) else None)
    assert _rows(x) and jobs.dim() == 2 and jobs.shape[1] == 2 and jobs.dtype == torch.int32 and jobs.is_contiguous()
    assert alphas.dim() == 1 and alphas.dtype == torch.float32 and alphas.is_contiguous()
    (B, V), J = x.shape, jobs.shape[0]
    value, base, stride = _path_baseline("path_points", baseline, x.shape)
    if out is None:
        out = torch.empty((J, V), dtype=torch.float32, device=x.device)
    assert _rows(out, J, V) and out.device == x.device
    check(lib.nv_path_points(_p(x), B, V, _p(jobs), J, _p(alphas), alphas.shape[0], value, _p(base), stride, _p(out), _stream()), "nv_path_points")
    return out


def class_score_grads(logits: torch.Tensor, jobs: torch.Tensor, cls: torch.Tensor, kind: str = "logit") -> torch.Tensor:
    """logits f32 [J, C], jobs int32 [J, 2] (column 0: the source volume b_j), cls int64 [B] -> f32 [J, C]: the gradient of the score of
    class cls[b_j] w.r.t. row j - "logit": its one-hot; "prob": p_c (delta_ci - p_i) with the fp32 softmax of class_scores.  A class out of
    range gives a row of NaN.  nv_class_score_grads, one launch."""
    _need_cuda(logits, jobs, cls)
    if kind not in SCORE_KINDS:
        raise ValueError(f"neurovit_amd: class_score_grads: kind must be 'prob' or 'logit', got {kind!r}")
    assert logits.dim() == 2 and logits.dtype == torch.float32 and logits.is_contiguous()
    J, C = logits.shape
    assert jobs.shape == (J, 2) and jobs.dtype == torch.int32 and jobs.is_contiguous()
    assert cls.dim() == 1 and cls.dtype == torch.int64 and cls.is_contiguous()
    dlogits = torch.empty((J, C), dtype=torch.float32, device=logits.device)
    check(lib.nv_class_score_grads(_p(logits), J, C, _p(jobs), _p(cls), cls.shape[0], SCORE_KINDS[kind], _p(dlogits), _stream()),
          "nv_class_score_grads")
    return dlogits


def path_accumulate(g: torch.Tensor, jobs: torch.Tensor, weights: torch.Tensor, acc: torch.Tensor) -> torch.Tensor:
    """g f32 [J, V], jobs int32 [J, 2] of rows (b, k), weights f32 [K], acc f32 [B, V]: acc[b] += weights[k] * g[j] over the jobs of
    volume b in job order (a rounded product, then a rounded sum); volumes absent from `jobs` keep their bits.  In place; at most 1024
    jobs.  nv_path_accumulate, one launch."""
    _need_cuda(g, jobs, weights, acc)
    assert _rows(g) and _rows(acc, None, g.shape[1]) and g.device == acc.device
    J, V = g.shape
    assert jobs.shape == (J, 2) and jobs.dtype == torch.int32 and jobs.is_contiguous()
    assert weights.dim() == 1 and weights.dtype == torch.float32 and weights.is_contiguous()
    check(lib.nv_path_accumulate(_p(g), _p(jobs), J, _p(weights), weights.shape[0], _p(acc), acc.shape[0], V, _stream()), "nv_path_accumulate")
    return acc


def path_finish(acc: torch.Tensor, x: torch.Tensor, baseline=0.0, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """acc, x f32 [B, V] -> f32 [B, V]: (x - bl) * acc, a rounded difference then a rounded product; baseline as path_points.
    nv_path_finish, one launch."""
    _need_cuda(acc, x, out, baseline if torch.is_tensor(baseline) else None)
    assert _rows(x) and _rows(acc, *x.shape) and acc.device == x.device
    B, V = x.shape
    value, base, stride = _path_baseline("path_finish", baseline, x.shape)
    if out is None:
        out = torch.empty((B, V), dtype=torch.float32, device=x.device)
    assert _rows(out, B, V) and out.device == x.device
    check(lib.nv_path_finish(_p(acc), _p(x), B, V, value, _p(base), stride, _p(out), _stream()), "nv_path_finish")
    return out


def attr_token_sums(attr: torch.Tensor, patch) -> torch.Tensor:
    """attr f32 [B, S0, S1, S2] (NeuroEncoder.forward's layout, device), patch: an int or three -> f32 [B, N, 2]: per patch token (numbered
    as the engine's patch gather numbers them) the sum and the sum of absolute values of its voxels, accumulated in double in a fixed
    order.  nv_attr_token_sums, one launch."""
    _need_cuda(attr)
    patch = _triple(patch, "patch")
    assert attr.dim() == 4 and attr.dtype == torch.float32 and attr.is_contiguous()
    B, size = attr.shape[0], tuple(attr.shape[1:])
    if any(s % p for s, p in zip(size, patch)):
        raise ValueError(f"neurovit_amd: attr_token_sums: volume {size} is not a whole number of {patch} patches")
    N = (size[0] // patch[0]) * (size[1] // patch[1]) * (size[2] // patch[2])
    sums = torch.empty((B, N, 2), dtype=torch.float32, device=attr.device)
    (s3, s3p), (p3, p3p) = _int3_ptr(size), _int3_ptr(patch)
    check(lib.nv_attr_token_sums(_p(attr), B, s3p, p3p, _p(sums), _stream()), "nv_attr_token_sums")
    return sums


def dropout_apply(x: torch.Tensor, drop_seed: int = 0, drop_p: float = 0.0, want16: bool = True, want32: bool = False, *,
                  o16: Optional[torch.Tensor] = None, o32: Optional[torch.Tensor] = None):
    """x f32 [M, N] times the dropout mask of one site -> (bf16 copy or None, f32 copy or None).  o16 / o32: row-strided views to write."""
    _need_cuda(x)
    M, N = x.shape
    o16 = _out2d(o16, M, N, op16(), x) if (want16 or o16 is not None) else None
    o32 = _out2d(o32, M, N, torch.float32, x) if (want32 or o32 is not None) else None
    check(lib.nv_dropout_apply(_p(x), x.stride(0), M, N, drop_seed, drop_p, _p(o16), N if o16 is None else o16.stride(0), _p(o32),
                               N if o32 is None else o32.stride(0), _stream()), "nv_dropout_apply")
    return o16, o32


class ReduceJob(ctypes.Structure):            # include/neurovit_hip.h::nv_reduce_job
    _fields_ = [("partials", ctypes.c_void_p), ("rows", ctypes.c_int), ("width", ctypes.c_int), ("nseg", ctypes.c_int),
                ("out", ctypes.c_void_p * 3), ("accumulate", ctypes.c_int)]


def reduce_multi(jobs) -> None:
    """jobs: [(partials f32 [rows, nseg*width], width, [out tensors or None] (nseg of them), accumulate)] - one launch."""
    arr = (ReduceJob * len(jobs))()
    for i, (part, width, outs, acc) in enumerate(jobs):
        _need_cuda(part)
        rows, tot = part.shape
        nseg = tot // width
        assert nseg * width == tot and len(outs) == nseg and part.is_contiguous()
        o = (ctypes.c_void_p * 3)(*[(_p(t) if t is not None else None) for t in list(outs) + [None] * (3 - nseg)])
        arr[i] = ReduceJob(part.data_ptr(), rows, width, nseg, o, int(acc))
    check(lib.nv_reduce_multi(ctypes.cast(arr, ctypes.c_void_p), len(jobs), _stream()), "nv_reduce_multi")


def gemm_dgelu_colsum(A: torch.Tensor, B: torch.Tensor, u: torch.Tensor, drop_seed: int = 0, drop_p: float = 0.0):
    """dU = (A B) * gelu'(u) (bf16) with the fused column-sum epilogue -> (dU, partial column sums f32 [tile rows, N]);
    raises when the shape has no large-tile kernel (use EPI_DGELU + colsum_bf16 then)."""
    M, K = A.shape
    N = B.shape[1]
    rows = lib.nv_gemm_tile_rows(NN, M, N, K, A.stride(0), B.stride(0))
    if rows == 0:
        raise RuntimeError("neurovit_amd: fused column-sum epilogue not available for this shape")
    part = torch.empty(((M + rows - 1) // rows, N), dtype=torch.float32, device=A.device)
    out = gemm(NN, EPI_DGELU_COLSUM, A, B, aux_in=u, aux_out=part, drop_seed=drop_seed, drop_p=drop_p)
    return out, part


EPI_BIAS_GELU_F8, EPI_BIAS_GELU_F8T = 7, 8


def _out2d(out: Optional[torch.Tensor], rows: int, cols: int, dtype: torch.dtype, like: torch.Tensor) -> torch.Tensor:
    """A preallocated 2-D output (any row stride: a column slice of a wider buffer passes its own leading dimension) or a fresh dense one."""
    if out is None:
        return torch.empty((rows, cols), dtype=dtype, device=like.device)
    _need_cuda(out)
    assert out.dtype == dtype and out.shape == (rows, cols) and out.stride(1) == 1
    return out


def quant_rows_f8(W: torch.Tensor, act_scale: float, *, out: Optional[torch.Tensor] = None, colscale: Optional[torch.Tensor] = None):
    """fp32 [rows, cols] -> (e4m3 bytes uint8 [rows, cols], colscale f32 [rows] = 1 / (act_scale * row scale))."""
    _need_cuda(W)
    rows, cols = W.shape
    assert W.dtype == torch.float32 and W.stride(1) == 1
    out = _out2d(out, rows, cols, torch.uint8, W)
    cs = torch.empty(rows, dtype=torch.float32, device=W.device) if colscale is None else colscale
    assert cs.dtype == torch.float32 and cs.shape == (rows,) and cs.is_contiguous()
    check(lib.nv_quant_rows_f8(_p(W), W.stride(0), rows, cols, _p(out), out.stride(0), float(act_scale), _p(cs), _stream()), "nv_quant_rows_f8")
    return out, cs


def ln_fwd_f8(x: torch.Tensor, gamma, beta, out_scale: float, eps: float = 1e-5, *, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    _need_cuda(x)
    M, d = x.shape
    assert x.dtype == torch.float32 and x.stride(1) == 1
    y = _out2d(out, M, d, torch.uint8, x)
    check(lib.nv_ln_fwd_f8(_p(x), x.stride(0), M, d, _p(gamma), _p(beta), eps, float(out_scale), _p(y), y.stride(0), _stream()), "nv_ln_fwd_f8")
    return y


def ln_fwd_f8_train(x: torch.Tensor, gamma, beta, out_scale: float, eps: float = 1e-5, *, y8: Optional[torch.Tensor] = None,
                    y16: Optional[torch.Tensor] = None, st: Optional[torch.Tensor] = None):
    """LayerNorm of a training forward on fp8 operands -> (y8 e4m3 bytes as ln_fwd_f8, y16 bf16 and st = (mean, rstd) f32 [2, M] as ln_fwd)."""
    _need_cuda(x)
    M, d = x.shape
    assert x.dtype == torch.float32 and x.stride(1) == 1
    y8 = _out2d(y8, M, d, torch.uint8, x)
    y16 = _out2d(y16, M, d, torch.bfloat16, x)
    st = torch.empty((2, M), dtype=torch.float32, device=x.device) if st is None else st
    assert st.dtype == torch.float32 and st.shape == (2, M) and st.stride(1) == 1
    check(lib.nv_ln_fwd_f8_train(_p(x), x.stride(0), M, d, _p(gamma), _p(beta), eps, float(out_scale), _p(y8), y8.stride(0), _p(y16), y16.stride(0),
                                 _p(st[0]), _p(st[1]), _stream()), "nv_ln_fwd_f8_train")
    return y8, y16, st


def _f8_operands(A8: torch.Tensor, B8: torch.Tensor):
    _need_cuda(A8, B8)
    assert A8.dtype == torch.uint8 and B8.dtype == torch.uint8 and A8.stride(1) == 1 and B8.stride(1) == 1 and A8.shape[1] == B8.shape[1]
    return A8.shape[0], B8.shape[0], A8.shape[1]


def gemm_f8(epi: int, A8: torch.Tensor, B8: torch.Tensor, colscale: torch.Tensor, *, bias=None, aux_in=None, out_scale: float = 1.0, out=None):
    """C = epi((A8 B8^T) * colscale[n]); A8 [M, K], B8 [N, K] e4m3 bytes (uint8 tensors, row-strided views allowed)."""
    M, N, K = _f8_operands(A8, B8)
    odt = {EPI_STORE_BF16: op16(), EPI_STORE_F32: torch.float32, EPI_BIAS_RESID: torch.float32, EPI_BIAS_GELU_F8: torch.uint8}[epi]
    out = _out2d(out, M, N, odt, A8)
    check(lib.nv_gemm_f8(epi, M, N, K, _p(A8), A8.stride(0), _p(B8), B8.stride(0), _p(out), out.stride(0), _p(colscale), _p(bias), _p(aux_in),
                         0 if aux_in is None else aux_in.stride(0), float(out_scale), _stream()), "nv_gemm_f8")
    return out


def gemm_f8_gelu_train(A8: torch.Tensor, B8: torch.Tensor, colscale: torch.Tensor, bias: torch.Tensor, out_scale: float, *,
                       h8: Optional[torch.Tensor] = None, h16: Optional[torch.Tensor] = None, u16=None, drop_seed: int = 0, drop_p: float = 0.0):
    """FC1 of a training forward on fp8 operands (epilogue EPI_BIAS_GELU_F8T): u = (A8 B8^T) * colscale[n] + bias[n] ->
    (h8 e4m3 = sat(gelu(u) * mask * out_scale), h16 bf16 = gelu(u) * mask, u16 bf16 = u).  Every output: None allocates it, a tensor is
    written in place; u16=False skips the store of u (the third result is None then)."""
    M, N, K = _f8_operands(A8, B8)
    h8 = _out2d(h8, M, N, torch.uint8, A8)
    h16 = _out2d(h16, M, N, torch.bfloat16, A8)
    u16 = None if u16 is False else _out2d(u16, M, N, torch.bfloat16, A8)
    check(lib.nv_gemm_f8_gelu_train(M, N, K, _p(A8), A8.stride(0), _p(B8), B8.stride(0), _p(colscale), _p(bias), float(out_scale), _p(h8), h8.stride(0),
                                    _p(h16), h16.stride(0), _p(u16), 0 if u16 is None else u16.stride(0), int(drop_seed), float(drop_p), _stream()),
          "nv_gemm_f8_gelu_train")
    return h8, h16, u16


def gemm_f8_resid_drop(A8: torch.Tensor, B8: torch.Tensor, colscale: torch.Tensor, bias: torch.Tensor, aux_in: torch.Tensor, *,
                       out: Optional[torch.Tensor] = None, drop_seed: int = 0, drop_p: float = 0.0) -> torch.Tensor:
    """FC2 of a training forward on fp8 operands: f32 = aux_in + ((A8 B8^T) * colscale[n] + bias[n]) * mask (the mask of gemm(NT, EPI_BIAS_RESID))."""
    M, N, K = _f8_operands(A8, B8)
    out = _out2d(out, M, N, torch.float32, A8)
    check(lib.nv_gemm_f8_resid_drop(M, N, K, _p(A8), A8.stride(0), _p(B8), B8.stride(0), _p(out), out.stride(0), _p(colscale), _p(bias), _p(aux_in),
                                    aux_in.stride(0), int(drop_seed), float(drop_p), _stream()), "nv_gemm_f8_resid_drop")
    return out


def patch_ln_fwd_4d(x: torch.Tensor, p1: int, p2: int, pf: int, gamma, beta, eps: float = 1e-5, vol_sigma=None, *, out=None, st=None, f32: bool = False):
    """x f32 contiguous [Bo, H, W, D, T] -> tokens bf16 [Bo*T*N, P] of the T volumes of every sample (row (bo*T + t)*N + n)."""
    _need_cuda(x)
    assert x.dim() == 5 and x.is_contiguous() and x.dtype == torch.float32
    Bo, H, W, D, T = x.shape
    P = p1 * p2 * pf
    N = (D // pf) * (H // p1) * (W // p2)
    out = _out2d(out, Bo * T * N, P, torch.float32 if f32 else op16(), x)        # out: a row-strided view to write; f32: nv_patch_ln_fwd_4d_f32
    st = torch.empty((2, Bo * T * N), dtype=torch.float32, device=x.device) if st is None else st
    fn = lib.nv_patch_ln_fwd_4d_f32 if f32 else lib.nv_patch_ln_fwd_4d
    check(fn(_p(x), Bo, H, W, D, T, p1, p2, pf, _p(gamma), _p(beta), eps, _p(out), out.stride(0), _p(st[0]), _p(st[1]), _p(vol_sigma), _stream()),
          "nv_patch_ln_fwd_4d")
    return out, st


def temporal_head_param_count(ff: int) -> int:
    return int(lib.nv_temporal_head_param_count(int(ff)))


def temporal_head_fwd(x: torch.Tensor, params: torch.Tensor, ff: int, eps: float = 1e-5, drop_seed: int = 0, drop_p: float = 0.0) -> torch.Tensor:
    """The 4D model's temporal head (NeuroEncoder.py:60-66): x f32 [B, T, 2] -> encoder layer -> mean over T -> Linear(2, 2) -> [B, 2]."""
    _need_cuda(x, params)
    assert x.dtype == torch.float32 and x.dim() == 3 and x.shape[2] == 2 and x.is_contiguous() and params.dtype == torch.float32
    assert params.is_contiguous() and params.numel() == temporal_head_param_count(ff)
    B, T, _ = x.shape
    out = torch.empty((B, 2), dtype=torch.float32, device=x.device)
    check(lib.nv_temporal_head_fwd(_p(x), B, T, int(ff), _p(params), eps, int(drop_seed), float(drop_p), _p(out), _stream()), "nv_temporal_head_fwd")
    return out


def temporal_head_bwd(x: torch.Tensor, params: torch.Tensor, ff: int, dout: torch.Tensor, grads: torch.Tensor, accumulate: bool = False,
                      want_dx: bool = False, eps: float = 1e-5, drop_seed: int = 0, drop_p: float = 0.0):
    """Gradients of temporal_head_fwd (forward recomputed from x, same seed / p): parameter gradients into the flat arena `grads`
    (added when accumulate), returns dx [B, T, 2] when want_dx."""
    _need_cuda(x, params, dout, grads)
    assert x.dtype == torch.float32 and x.dim() == 3 and x.shape[2] == 2 and x.is_contiguous()
    assert dout.dtype == torch.float32 and dout.shape == (x.shape[0], 2) and dout.is_contiguous()
    assert grads.dtype == torch.float32 and grads.is_contiguous() and grads.numel() == params.numel() == temporal_head_param_count(ff)
    B, T, _ = x.shape
    dx = torch.empty_like(x) if want_dx else None
    check(lib.nv_temporal_head_bwd(_p(x), B, T, int(ff), _p(params), eps, int(drop_seed), float(drop_p), _p(dout), _p(grads), int(bool(accumulate)),
                                   _p(dx), _stream()), "nv_temporal_head_bwd")
    return dx


def ln_fold_weight(W: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor, bias: Optional[torch.Tensor] = None):
    """(Wg16 = op16(W diag(gamma)), colsum of the rounded Wg16 rows, folded bias W beta (+ bias)): the Linear behind a LayerNorm, folded (nv_ln_fold_weight)."""
    _need_cuda(W)
    N, K = W.shape
    Wg = torch.empty((N, K), dtype=op16(), device=W.device)
    cs = torch.empty(N, dtype=torch.float32, device=W.device)
    fb = torch.empty(N, dtype=torch.float32, device=W.device)
    check(lib.nv_ln_fold_weight(_p(W), W.stride(0), N, K, _p(gamma), _p(beta), _p(bias), _p(Wg), Wg.stride(0), _p(cs), _p(fb), _stream()), "nv_ln_fold_weight")
    return Wg, cs, fb


def gemm_resid_ln(A: torch.Tensor, W: torch.Tensor, bias: torch.Tensor, resid: torch.Tensor, *, out=None, out16=None, stats=None):
    """x = resid + (A W^T + bias) as f32, the same rows in the operand format, and the per-tile row statistics (nv_gemm_resid_ln)."""
    _need_cuda(A, W)
    M, K = A.shape
    N = W.shape[0]
    out = _out2d(out, M, N, torch.float32, A)
    out16 = _out2d(out16, M, N, op16(), A)
    stats = torch.empty(lib.nv_ln_fold_stats_floats(M, N), dtype=torch.float32, device=A.device) if stats is None else stats
    assert stats.dtype == torch.float32 and stats.numel() == lib.nv_ln_fold_stats_floats(M, N) and stats.is_contiguous()
    check(lib.nv_gemm_resid_ln(M, N, K, _p(A), A.stride(0), _p(W), W.stride(0), _p(bias), _p(resid), resid.stride(0), _p(out), out.stride(0), _p(out16), out16.stride(0),
                               _p(stats), _stream()), "nv_gemm_resid_ln")
    return out, out16, stats


def gemm_lnfold(X16: torch.Tensor, Wg16: torch.Tensor, stats: torch.Tensor, colsum: torch.Tensor, fbias: torch.Tensor, gelu: bool = False, eps: float = 1e-5, *, out=None):
    """(gelu)(LayerNorm(x) W^T + b) from the un-normalised rows X16, their statistics and the folded weight (nv_gemm_lnfold)."""
    _need_cuda(X16, Wg16)
    M, K = X16.shape
    N = Wg16.shape[0]
    out = _out2d(out, M, N, op16(), X16)
    check(lib.nv_gemm_lnfold(int(gelu), M, N, K, _p(X16), X16.stride(0), _p(Wg16), Wg16.stride(0), _p(stats), _p(colsum), _p(fbias), float(eps), _p(out), out.stride(0),
                             _stream()), "nv_gemm_lnfold")
    return out


# ---- masked-volume pretraining (csrc/pretrain.hip)
RECON_KINDS = {"l1": 0, "l2": 1}        # NV_RECON_L1 / NV_RECON_L2


def mim_masked_count(grid, unit: int, ratio: float) -> int:
    """Patches per volume that nv_mim_labels' tables mask for (grid, unit, ratio): clamp(floor(ratio U + 0.5), 1, U - 1) u^3 with U the number
    of mask units.  A host-side function of the library (nv_mim_masked_count); ValueError for a unit that does not divide the grid or a
    ratio outside (0, 1)."""
    (g3, g3p) = _int3_ptr(_triple(grid, "grid"))
    m = lib.nv_mim_masked_count(g3p, int(unit), float(ratio))
    if m < 0:
        raise ValueError(f"neurovit_amd: mim_masked_count: {_cabi.last_error()}")
    return m


def mim_labels(B: int, grid, unit: int, seed: int, step: int, rank: int = 0, device="cuda", out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """int32 [B, N] label tables of a fresh random mask per sample, drawn and ranked on the device from (seed, rank, step, sample, unit):
    label < mim_masked_count(grid, unit, ratio) means masked, so mask_patches with the jobs (b, 0, m) writes the masked batch.
    nv_mim_labels, one launch; nothing is read back."""
    grid = _triple(grid, "grid")
    N = grid[0] * grid[1] * grid[2]
    if out is None:
        out = torch.empty((B, N), dtype=torch.int32, device=device)
    _need_cuda(out)
    assert out.shape == (B, N) and out.dtype == torch.int32 and out.is_contiguous()
    (g3, g3p) = _int3_ptr(grid)
    check(lib.nv_mim_labels(int(seed), int(step), int(rank), B, g3p, int(unit), _p(out), _stream()), "nv_mim_labels")
    return out


def recon_loss(pred: torch.Tensor, x: torch.Tensor, labels: torch.Tensor, m: int, patch, kind: str = "l1", norm_pix: bool = True,
               loss_scale: float = 1.0, dpred: Optional[torch.Tensor] = None):
    """pred f32 [B n, >= P8] (row-strided 2-D view, n = N + 1 rows per volume, the cls row first), the ORIGINAL volumes x f32 [B, S0, S1, S2],
    labels int32 [B, N] (mim_labels) and the masked-patch count m -> (loss f32 [1], dpred [B n, ldd] in the operand format, partials f64 [B n]):
    the L1 / L2 reconstruction loss over the masked patches (norm_pix: targets standardised per patch, MAE's rule) and its gradient times
    loss_scale; every cell of dpred outside the masked rows' first P columns is written as zero.  nv_recon_loss, two launches."""
    _need_cuda(pred, x, labels, dpred)
    patch = _triple(patch, "patch")
    assert x.dim() == 4 and x.dtype == torch.float32 and x.is_contiguous()
    B, size = x.shape[0], tuple(x.shape[1:])
    if any(s % p for s, p in zip(size, patch)):
        raise ValueError(f"neurovit_amd: recon_loss: volume {size} is not a whole number of {patch} patches")
    N = (size[0] // patch[0]) * (size[1] // patch[1]) * (size[2] // patch[2])
    P = patch[0] * patch[1] * patch[2]
    P8 = (P + 7) // 8 * 8
    rows = B * (N + 1)
    assert pred.dim() == 2 and pred.dtype == torch.float32 and pred.shape[0] == rows and pred.shape[1] >= P8 and pred.stride(1) == 1
    assert labels.shape == (B, N) and labels.dtype == torch.int32 and labels.is_contiguous()
    if dpred is None:
        dpred = torch.empty((rows, P8), dtype=op16(), device=x.device)
    assert dpred.dim() == 2 and dpred.dtype == op16() and dpred.shape[0] == rows and dpred.shape[1] >= P8 and dpred.stride(1) == 1 and dpred.stride(0) == dpred.shape[1]
    partials = torch.empty(rows, dtype=torch.float64, device=x.device)
    loss = torch.empty(1, dtype=torch.float32, device=x.device)
    (s3, s3p), (p3, p3p) = _int3_ptr(size), _int3_ptr(patch)
    check(lib.nv_recon_loss(_p(pred), pred.stride(0), _p(x), B, s3p, p3p, _p(labels), int(m), RECON_KINDS[kind], int(bool(norm_pix)), float(loss_scale),
                            _p(dpred), dpred.stride(0), _p(partials), _p(loss), _stream()), "nv_recon_loss")
    return loss, dpred, partials


def token_grad_seed(dtokens: torch.Tensor, drop_seed: int = 0, drop_p: float = 0.0):
    """dtokens f32 [M, d] -> (g f32 = dtokens, g16 = cvt(dtokens * mask), colsum f32 [d] of dtokens * mask): what nv_vit_backward_tokens
    queues in the head's place (nv_token_grad_seed + nv_reduce_multi)."""
    _need_cuda(dtokens)
    assert dtokens.dim() == 2 and dtokens.dtype == torch.float32 and dtokens.is_contiguous()
    M, d = dtokens.shape
    g = torch.empty_like(dtokens)
    g16 = torch.empty((M, d), dtype=op16(), device=dtokens.device)
    nb = lib.nv_token_grad_seed_workspace_bytes(M, d)
    part = torch.empty((lib.nv_token_grad_seed_rows(M), d), dtype=torch.float32, device=dtokens.device)
    assert part.numel() * 4 == nb
    check(lib.nv_token_grad_seed(_p(dtokens), M, d, _p(g), _p(g16), _p(part), nb, int(drop_seed), float(drop_p), _stream()), "nv_token_grad_seed")
    colsum = torch.empty(d, dtype=torch.float32, device=dtokens.device)
    reduce_multi([(part, d, (colsum,), False)])
    return g, g16, colsum


def check_drop_path(rate, schedule) -> None:
    """ValueError for a stochastic-depth rate outside [0, 1) or a schedule that is not 'linear' / 'constant' (no device work)"""
    if isinstance(rate, bool) or not isinstance(rate, (int, float)) or not 0.0 <= float(rate) < 1.0:
        raise ValueError(f"neurovit_amd: drop_path_rate must be a number in [0, 1), got {rate!r}")
    if schedule not in _cabi.DROP_PATH_SCHEDULES:
        raise ValueError(f"neurovit_amd: drop_path_schedule must be 'linear' or 'constant', got {schedule!r}")


def drop_path_draw(seed: int, B: int, depth: int, rate: float, schedule: str = "linear", device="cuda", out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """fp32 [depth, 2, B] stochastic-depth factors (0 or 1 / (1 - q_l) per block, branch and sample), drawn on the device from the seed:
    schedule "linear" q_l = rate * l / (depth - 1) (timm's linspace), "constant" q_l = rate.  nv_drop_path_draw, one launch; nothing is
    read back.  The table VitRuntime.forward / backward / train_step take as drop_path=."""
    check_drop_path(rate, schedule)
    if out is None:
        out = torch.empty((depth, 2, B), dtype=torch.float32, device=device)
    _need_cuda(out)
    assert out.shape == (depth, 2, B) and out.dtype == torch.float32 and out.is_contiguous()
    check(lib.nv_drop_path_draw(int(seed), int(B), int(depth), float(rate), _cabi.DROP_PATH_SCHEDULES[schedule], _p(out), _stream()), "nv_drop_path_draw")
    return out


# ---- the evaluation of a frozen encoder.  Frozen features (features.hip): pooled features, the fused similarity + top-k search, the kNN vote;
# segments of rows (segments.hip)
def pool_features(tokens: torch.Tensor, mode, normalize: bool = False, *, out: Optional[torch.Tensor] = None, row0: int = 0) -> torch.Tensor:
    """nv_pool_features: tokens f32 [B, n, d] (any batch / row stride, last stride 1) -> rows row0 .. row0 + B of `out` f32 [*, d] (any row
    stride; a fresh [B, d] when None).  mode "cls" | "mean" | "patch_mean" (or 0 / 1 / 2).  Returns the B rows written."""
    _need_cuda(tokens)
    assert tokens.dtype == torch.float32 and tokens.dim() == 3 and tokens.stride(2) == 1
    B, n, d = tokens.shape
    if out is None:
        out, row0 = torch.empty((B, d), dtype=torch.float32, device=tokens.device), 0
    _need_cuda(out)
    assert out.dtype == torch.float32 and out.dim() == 2 and out.shape[1] == d and out.stride(1) == 1
    if row0 < 0 or row0 + B > out.shape[0]:
        raise ValueError(f"pool_features: rows {row0} .. {row0 + B} do not fit an output of {out.shape[0]} rows")
    mode = _cabi.POOL_MODES[mode] if isinstance(mode, str) else int(mode)
    check(lib.nv_pool_features(_p(tokens), tokens.stride(0), tokens.stride(1), B, n, d, mode, int(bool(normalize)), _p(out), out.stride(0), int(row0),
                               _stream()), "nv_pool_features")
    return out[row0:row0 + B]


def knn_topk(Q: torch.Tensor, bank: torch.Tensor, k: int, q_group: Optional[torch.Tensor] = None, b_group: Optional[torch.Tensor] = None, splits: int = 0):
    """nv_knn_topk: the k rows of bank f32 [Nb, d] with the largest dot product for every row of Q f32 [Nq, d] (row-strided views pass their
    leading dimension; d and both strides multiples of 4).  Larger sim first, equal sim to the lower bank index; bank row j is skipped for
    query q when q_group[q] >= 0 and q_group[q] == b_group[j] (int32, both or neither); unfilled slots are (-1, -inf).  splits: 0 = automatic.
    Returns (idx int32 [Nq, k], sim f32 [Nq, k])."""
    _need_cuda(Q, bank)
    (Nq, d), Nb = _rows2d(Q, "knn_topk: Q", AssertionError), _rows2d(bank, "knn_topk: bank", AssertionError)[0]
    if bank.shape[1] != d:
        raise ValueError(f"knn_topk: the queries have {d} columns, the bank {bank.shape[1]}")
    if (q_group is None) != (b_group is None):
        raise ValueError("knn_topk: q_group and b_group are given together or not at all")
    q_group, b_group = _i32(q_group, Nq, "q_group"), _i32(b_group, Nb, "b_group")
    idx = torch.empty((Nq, k), dtype=torch.int32, device=Q.device)
    sim = torch.empty((Nq, k), dtype=torch.float32, device=Q.device)
    nb = lib.nv_knn_topk_workspace_bytes(Nq, Nb, int(k), int(splits))
    ws = torch.empty(nb, dtype=torch.uint8, device=Q.device) if nb else None
    check(lib.nv_knn_topk(_p(Q), Q.stride(0), Nq, _p(bank), bank.stride(0), Nb, d, int(k), _p(q_group), _p(b_group), int(splits), _p(idx), _p(sim),
                          _p(ws), nb, _stream()), "nv_knn_topk")
    return idx, sim


def knn_vote(idx: torch.Tensor, sim: torch.Tensor, k: int, *, labels: Optional[torch.Tensor] = None, num_classes: int = 0,
             targets: Optional[torch.Tensor] = None, weights: str = "softmax", temperature: float = 0.07):
    """nv_knn_vote over the first k slots of idx / sim [Nq, kmax].  labels int32 [Nb] + num_classes -> (scores f32 [Nq, C], pred int32 [Nq]);
    targets f32 [Nb, K] -> pred f32 [Nq, K] (neighbours with a NaN target are left out per column)."""
    _need_cuda(idx, sim)
    assert idx.dtype == torch.int32 and sim.dtype == torch.float32 and idx.shape == sim.shape and idx.is_contiguous() and sim.is_contiguous()
    Nq, kmax = idx.shape
    if weights not in _cabi.KNN_WEIGHTS:
        raise ValueError(f"knn_vote: weights must be 'softmax' or 'uniform', got {weights!r}")
    w = _cabi.KNN_WEIGHTS[weights]
    if (labels is None) == (targets is None):
        raise ValueError("knn_vote: give labels (classification) or targets (regression), one of the two")
    if labels is not None:
        labels = _i32(labels, labels.numel(), "labels")
        scores = torch.empty((Nq, int(num_classes)), dtype=torch.float32, device=idx.device)
        pred = torch.empty(Nq, dtype=torch.int32, device=idx.device)
        check(lib.nv_knn_vote(_p(idx), _p(sim), Nq, kmax, int(k), w, float(temperature), labels.numel(), _p(labels), int(num_classes), _p(scores), _p(pred),
                              None, 0, None, _stream()), "nv_knn_vote")
        return scores, pred
    _need_cuda(targets)
    assert targets.dtype == torch.float32 and targets.dim() == 2 and targets.is_contiguous()
    Nb, K = targets.shape
    pred = torch.empty((Nq, K), dtype=torch.float32, device=idx.device)
    check(lib.nv_knn_vote(_p(idx), _p(sim), Nq, kmax, int(k), w, float(temperature), Nb, None, 0, None, None, _p(targets), K, _p(pred), _stream()), "nv_knn_vote")
    return pred


def host_ids(values, n: int, what: str) -> torch.Tensor:
    """integer ids or labels [n] as an int32 HOST tensor (subject ids are host data: the CSR of a segment mean is built from them without a
    device read)"""
    g = torch.as_tensor(values)
    if g.is_floating_point() or g.is_complex() or g.dtype == torch.bool or g.numel() != n:
        raise ValueError(f"{what}: {n} integer ids expected, got {tuple(g.shape)} {g.dtype}")
    return g.detach().reshape(-1).to("cpu", torch.int32)


def _segment_csr_host(groups, num_segments: Optional[int] = None):
    g = torch.as_tensor(groups).detach().to("cpu", torch.int64).reshape(-1)
    N = g.numel()
    G = int(num_segments) if num_segments is not None else (int(g.max().item()) + 1 if N else 0)
    if N < 1 or G < 1 or int(g.max().item()) >= G:
        raise ValueError(f"segment_csr: {N} rows, {G} segments, largest id {int(g.max().item()) if N else None}")
    keep = torch.nonzero(g >= 0).reshape(-1)
    srt = torch.sort(g[keep], stable=True)
    order = torch.zeros(N, dtype=torch.int32)
    order[:keep.numel()] = keep[srt.indices].to(torch.int32)
    offsets = torch.zeros(G + 1, dtype=torch.int32)
    offsets[1:] = torch.cumsum(torch.bincount(srt.values, minlength=G), 0).to(torch.int32)
    check(lib.nv_segment_csr_check(order.data_ptr(), offsets.data_ptr(), N, G), "nv_segment_csr_check")
    return order, offsets


def segment_csr(groups, num_segments: Optional[int] = None):
    """Host CSR of integer segment ids (a sequence or a tensor; a negative id = in no segment), validated by nv_segment_csr_check and uploaded:
    (order int32 [N], offsets int32 [G + 1]) on the current device.  The rows of a segment keep their ascending order."""
    order, offsets = _segment_csr_host(groups, num_segments)
    return order.cuda(), offsets.cuda()


def segment_mean(src: torch.Tensor, order: torch.Tensor, offsets: torch.Tensor, *, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """nv_segment_mean: out[g] = mean of the rows src[order[offsets[g] : offsets[g + 1]]] of src f32 [N, w] (a row-strided view passes its leading
    dimension), summed in double in that order; an empty segment gives zeros.  order / offsets: device int32, from segment_csr."""
    _need_cuda(src, order, offsets)
    N, w = _rows2d(src, "segment_mean: src", AssertionError)
    G = offsets.numel() - 1
    order, offsets = _i32(order, N, "order"), _i32(offsets, G + 1, "offsets")
    out = _out2d(out, G, w, torch.float32, src)
    check(lib.nv_segment_mean(_p(src), src.stride(0), N, w, _p(order), _p(offsets), G, _p(out), out.stride(0), _stream()), "nv_segment_mean")
    return out


def segment_labels(labels: torch.Tensor, order: torch.Tensor, offsets: torch.Tensor):
    """nv_segment_labels: (the label of each segment's first row int32 [G] - an empty segment gets -1 -, mixed int32 [1] = the number of
    segments that hold another valid label), device tensors; order / offsets from segment_csr."""
    _need_cuda(labels, order, offsets)
    N, G = labels.numel(), offsets.numel() - 1
    labels, order, offsets = _i32(labels, N, "segment_labels: labels"), _i32(order, N, "order"), _i32(offsets, G + 1, "offsets")
    out = torch.empty(G, dtype=torch.int32, device=labels.device)
    mixed = torch.empty(1, dtype=torch.int32, device=labels.device)
    check(lib.nv_segment_labels(_p(labels), N, _p(order), _p(offsets), G, _p(out), _p(mixed), _stream()), "nv_segment_labels")
    return out, mixed


class Segments:
    """The segments (subjects) of N rows from their host ids [N] (a negative id = in no segment; num_segments: default the largest id + 1),
    and what is computed per segment.  `ids` int32 [N], `sizes` int64 [G] (the rows of each segment) and `G` are host data and settled by the
    constructor without touching the device; `order` / `offsets` are segment_csr's device tensors, uploaded at their first use."""

    def __init__(self, ids, num_segments: Optional[int] = None, what: str = "segment ids"):
        self.ids = host_ids(ids, torch.as_tensor(ids).numel(), what)
        self._host_csr = _segment_csr_host(self.ids, num_segments)
        self.sizes = (self._host_csr[1][1:] - self._host_csr[1][:-1]).long()
        self.N, self.G, self._csr = self.ids.numel(), self.sizes.numel(), None

    def _device_csr(self):
        if self._csr is None:
            self._csr = tuple(t.cuda() for t in self._host_csr)
        return self._csr

    order = property(lambda self: self._device_csr()[0])
    offsets = property(lambda self: self._device_csr()[1])

    def mean(self, src: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """segment_mean of src f32 [N, w]: f32 [G, w], zeros for an empty segment"""
        return segment_mean(src, self.order, self.offsets, out=out)

    def nanmean(self, values: torch.Tensor) -> torch.Tensor:
        """per-segment mean over the cells that are not NaN (NaN where a segment has none): two nv_segment_mean calls, on the values with
        zeros for the missing cells and on the observed-cell mask"""
        seen = ~torch.isnan(values)
        total, share = self.mean(torch.where(seen, values, torch.zeros_like(values))), self.mean(seen.float())
        return torch.where(share > 0, total / share.clamp(min=1e-30), torch.full_like(total, float("nan")))

    def labels(self, device_labels: torch.Tensor):
        """segment_labels of device labels int32 [N]: (the label of each segment's first row int32 [G], -1 for an empty segment; mixed int32
        [1], the segments that hold another valid label) - device tensors, no host read"""
        return segment_labels(device_labels, self.order, self.offsets)

    def host_first_labels(self, host_labels: torch.Tensor):
        """The same rule on the host, for labels that are host data: (the label of each segment's first row [G], -1 for an empty segment;
        the number of segments that hold another valid label).  No device work."""
        order, offsets = (t.long() for t in self._host_csr)
        filled = self.sizes > 0
        first = torch.where(filled, host_labels[order[offsets[:-1].clamp(max=self.N - 1)]], torch.full((self.G,), -1, dtype=host_labels.dtype))
        rows = order[:int(offsets[-1])]
        segment = self.ids[rows].long()
        differ = (host_labels[rows] >= 0) & (host_labels[rows] != first[segment])
        return first, int(torch.unique(segment[differ]).numel())


# ---- classification metrics over scores and, with a bank, exact AUC and subject pooling (cls_metrics.hip)
def cls_auc(probs: torch.Tensor, labels: torch.Tensor, splits: int = 0) -> torch.Tensor:
    """nv_cls_auc: the exact one-vs-rest ROC-AUC per class of probs f32 [N, C] (a row-strided view passes its leading dimension) under labels
    int32 [N] (a label outside [0, C) = the row is not used), by counting pairs, ties as a half.  Returns float64 [C, 5] on the device:
    auc (NaN where a class has no positive or no negative row), n_pos, n_neg, gt, eq (_cabi.CLS_AUC_NAMES); no host read."""
    _need_cuda(probs, labels)
    N, C = _rows2d(probs, "cls_auc: probs")
    labels = _i32(labels, N, "cls_auc: labels")
    nb = lib.nv_cls_auc_workspace_bytes(N, C, int(splits))
    ws = torch.empty(max(nb, 8), dtype=torch.uint8, device=probs.device)
    out = torch.empty((C, len(_cabi.CLS_AUC_NAMES)), dtype=torch.float64, device=probs.device)
    check(lib.nv_cls_auc(_p(probs), probs.stride(0), _p(labels), N, C, int(splits), _p(out), _p(ws), nb, _stream()), "nv_cls_auc")
    return out


class ClassificationMetrics:
    """Validation metrics of a classifier, accumulated on the device (nv_cls_metrics_*, nv_cls_auc, nv_segment_labels): update() makes one
    launch and no host read, compute() one host read.  scores: logits (kind "logits") or probabilities (kind "probs", e.g. what
    LinearProbe.predict / knn_predict return) float32 [B, C]; labels: integers [B]; a row whose label lies outside [0, C) or that holds a
    non-finite score is counted in "skipped" and nowhere else.
    compute() -> {"n", "skipped", "accuracy", "balanced_accuracy", "macro_f1", "nll", "val_loss" (the mean over the updates of their mean
    nll: the reference's validation loss), "brier", "ece": floats; "class_support", "class_recall", "class_precision", "class_f1": float32 [C];
    "confusion": int64 [C, C], true x predicted}.  Undefined quantities are NaN.  With capacity > 0 update() also files the rows'
    probabilities and labels in a preallocated bank, and compute() adds "macro_auc" and "class_auc" (exact one-vs-rest ROC-AUC, ties as a
    half); with `groups` (host subject ids per row, as FeatureBank takes them) the same set once more under "subject_*" keys - the bank's
    probabilities averaged per subject, the subject's label from its first row - and "subject_mixed_labels", the number of subjects that hold
    another valid label.  With two classes also "sensitivity" (recall of class 1), "specificity" (recall of class 0) and "auc" (class 1's)."""

    def __init__(self, num_classes: int, capacity: int = 0, bins: int = 15, device="cuda"):
        self.C, self.capacity, self.bins, self.device = int(num_classes), int(capacity), int(bins), torch.device(device)
        if not 2 <= self.C <= _cabi.CLS_MAX_C or not 1 <= self.bins <= _cabi.CLS_MAX_BINS or self.capacity < 0:
            raise ValueError(f"ClassificationMetrics: num_classes = {num_classes} in [2, {_cabi.CLS_MAX_C}], bins = {bins} in [1, {_cabi.CLS_MAX_BINS}] and "
                             f"capacity = {capacity} >= 0 expected")
        if self.capacity > _cabi.CLS_AUC_MAX_N:
            raise ValueError(f"ClassificationMetrics: capacity = {capacity} above {_cabi.CLS_AUC_MAX_N} rows (nv_cls_auc)")
        if self.device.type != "cuda":
            raise RuntimeError("ClassificationMetrics runs on the MI355X (cuda) device - there is no CPU fallback")
        self.state = torch.zeros(lib.nv_cls_metrics_state_doubles(self.C, self.bins), dtype=torch.float64, device=self.device)
        self.bank_probs = torch.zeros((self.capacity, self.C), dtype=torch.float32, device=self.device) if self.capacity else None
        self.bank_labels = torch.full((self.capacity,), -1, dtype=torch.int32, device=self.device) if self.capacity else None
        self._host_groups = torch.full((self.capacity,), -1, dtype=torch.int32)
        self.size, self.has_groups = 0, False

    def reset(self) -> None:
        self.state.zero_()
        self._host_groups.fill_(-1)
        self.size, self.has_groups = 0, False

    def update(self, scores: torch.Tensor, labels: torch.Tensor, groups=None, kind: str = "logits") -> None:
        if kind not in _cabi.CLS_KINDS:
            raise ValueError(f"ClassificationMetrics.update: kind must be 'logits' or 'probs', got {kind!r}")
        if (not torch.is_tensor(scores) or scores.dim() != 2 or scores.shape[1] != self.C or scores.shape[0] < 1 or scores.dtype != torch.float32
                or not scores.is_cuda or scores.stride(1) != 1):
            raise ValueError(f"ClassificationMetrics.update: scores must be float32 [B, {self.C}] on the device (B >= 1, unit column stride)")
        B = scores.shape[0]
        labels = torch.as_tensor(labels)
        if labels.is_floating_point() or labels.is_complex() or labels.dtype == torch.bool or labels.numel() != B:
            raise ValueError(f"ClassificationMetrics.update: {B} integer labels expected, got {tuple(labels.shape)} {labels.dtype}")
        labels = labels.reshape(-1).to(scores.device, torch.int32).contiguous()
        host_groups = None
        if groups is not None:
            if not self.capacity:
                raise ValueError("ClassificationMetrics.update: groups need the bank - construct with capacity > 0")
            host_groups = host_ids(groups, B, "ClassificationMetrics.update: groups")
        if self.capacity and self.size + B > self.capacity:
            raise ValueError(f"ClassificationMetrics.update: {self.size} + {B} rows exceed the capacity {self.capacity}")
        check(lib.nv_cls_metrics_update(_p(scores), scores.stride(0), _p(labels), B, self.C, self.bins, _cabi.CLS_KINDS[kind], _p(self.state),
                                        _p(self.bank_probs), self.C, _p(self.bank_labels), self.size, self.capacity, _stream()), "nv_cls_metrics_update")
        if self.capacity:
            if host_groups is not None:
                self._host_groups[self.size:self.size + B] = host_groups
                self.has_groups = True
            self.size += B

    def state_parts(self, state: Optional[torch.Tensor] = None) -> dict:
        """views of the double state (no host read): "head" [6] (_cabi.CLS_STATE_NAMES), "confusion" [C, C], "bin_count" / "bin_conf" /
        "bin_correct" [bins]"""
        s = self.state if state is None else state
        h, cc, nb = _cabi.CLS_STATE_HEAD, self.C * self.C, self.bins
        return {"head": s[:h], "confusion": s[h:h + cc].view(self.C, self.C), "bin_count": s[h + cc:h + cc + nb],
                "bin_conf": s[h + cc + nb:h + cc + 2 * nb], "bin_correct": s[h + cc + 2 * nb:h + cc + 3 * nb]}

    def _finish(self, state, auc) -> torch.Tensor:
        out = torch.empty(lib.nv_cls_metrics_table_floats(self.C), dtype=torch.float32, device=self.device)
        check(lib.nv_cls_metrics_finish(_p(state), self.C, self.bins, _p(auc), _p(out), _stream()), "nv_cls_metrics_finish")
        return out

    def compute_device(self) -> dict:
        """Device tensors, no host read: "table" float32 [10 + 5 C + C C] as nv_cls_metrics_finish writes it, "auc" float64 [C, 5] (nv_cls_auc;
        with a bank), and with groups "subject_table", "subject_auc", "subject_labels" int32 [G], "subject_probs" float32 [G, C],
        "subject_state" and "subject_mixed" int32 [1]."""
        out = {}
        filled = self.capacity and self.size > 0
        if filled:
            out["auc"] = cls_auc(self.bank_probs[:self.size], self.bank_labels[:self.size])
        out["table"] = self._finish(self.state, out.get("auc"))
        if filled and self.has_groups and int(self._host_groups[:self.size].max()) >= 0:
            subjects = Segments(self._host_groups[:self.size])
            pooled = subjects.mean(self.bank_probs[:self.size])
            subject_labels, mixed = subjects.labels(self.bank_labels[:self.size])
            state = torch.zeros_like(self.state)
            check(lib.nv_cls_metrics_update(_p(pooled), pooled.stride(0), _p(subject_labels), subjects.G, self.C, self.bins, _cabi.CLS_KINDS["probs"], _p(state),
                                            None, 0, None, 0, 0, _stream()), "nv_cls_metrics_update")
            out["subject_auc"] = cls_auc(pooled, subject_labels)
            out["subject_table"] = self._finish(state, out["subject_auc"])
            out.update(subject_labels=subject_labels, subject_probs=pooled, subject_state=state, subject_mixed=mixed)
        return out

    def _named(self, table: torch.Tensor, prefix: str, with_auc: bool) -> dict:
        C, ns, nc = self.C, len(_cabi.CLS_METRIC_NAMES), len(_cabi.CLS_CLASS_METRIC_NAMES)
        got = {prefix + name: float(table[i]) for i, name in enumerate(_cabi.CLS_METRIC_NAMES)}
        per_class = table[ns:ns + C * nc].reshape(C, nc)
        for j, name in enumerate(_cabi.CLS_CLASS_METRIC_NAMES):
            got[f"{prefix}class_{name}"] = per_class[:, j].clone()
        got[prefix + "confusion"] = table[ns + C * nc:ns + C * nc + C * C].reshape(C, C).to(torch.int64)
        if not with_auc:
            del got[prefix + "macro_auc"], got[prefix + "class_auc"]
        if C == 2:
            got[prefix + "sensitivity"], got[prefix + "specificity"] = float(per_class[1, 1]), float(per_class[0, 1])
            if with_auc:
                got[prefix + "auc"] = float(per_class[1, 4])
        return got

    def compute(self) -> dict:
        dev = self.compute_device()
        parts = [dev["table"]]
        if "subject_table" in dev:
            parts += [dev["subject_table"], dev["subject_mixed"].to(torch.float32)]
        host = torch.cat(parts).cpu()              # the one host read
        T = dev["table"].numel()
        got = self._named(host[:T], "", bool(self.capacity))
        if "subject_table" in dev:
            got.update(self._named(host[T:2 * T], "subject_", True))
            got["subject_mixed_labels"] = int(host[2 * T])
        return got


# ---- the linear probe over a feature bank (probe.hip): column statistics, the fused loss + gradient pass, the Adam step, the prediction
def probe_heads(H: int, C: int, l2=None, step=None) -> "_cabi.ProbeHeads":
    """A _cabi.ProbeHeads: H heads of C columns (H * C <= 32), l2 and step per head (one value for all, a sequence, or None for zeros)."""
    H, C = int(H), int(C)
    if H < 1 or C < 1 or H * C > _cabi.PROBE_MAX_M:
        raise ValueError(f"probe_heads: H = {H} heads of C = {C} columns: H * C must lie in [1, {_cabi.PROBE_MAX_M}]")
    hd = _cabi.ProbeHeads(ctypes.sizeof(_cabi.ProbeHeads), H, C)
    for name, vals in (("l2", l2), ("step", step)):
        vals = [0.0] * H if vals is None else ([float(vals)] * H if isinstance(vals, (int, float)) else [float(v) for v in vals])
        if len(vals) != H:
            raise ValueError(f"probe_heads: {len(vals)} values of {name} for {H} heads")
        if name == "l2" and any(not v >= 0 for v in vals):
            raise ValueError(f"probe_heads: l2 must be >= 0, got {vals}")
        for h, v in enumerate(vals):
            getattr(hd, name)[h] = v
    return hd


def probe_stats(X: Optional[torch.Tensor] = None, *, skip_nan: bool = False, eps: float = 1e-12, labels: Optional[torch.Tensor] = None, num_classes: int = 0,
                class_weight: Optional[torch.Tensor] = None) -> dict:
    """nv_probe_stats.  X f32 [N, d] (a row-strided view passes its leading dimension) -> "mean", "rstd" = 1 / sqrt(var + eps) (0 where the
    variance is exactly 0), "std" (f32 [d]) and "count" (f64 [d], the observed cells; skip_nan leaves NaN cells out); labels int32 [N] +
    num_classes (+ class_weight f32 [C]) -> "denom" f64 [1], the class-weighted count of the rows whose label lies in [0, C).  Fixed
    256-row chunks, fp64, ascending order: the bits do not depend on the device."""
    if X is None and labels is None:
        raise ValueError("probe_stats: give X, labels or both")
    _need_cuda(X)
    out, dev = {}, (X if X is not None else labels).device
    N, d = (labels.numel(), 0) if X is None else _rows2d(X, "probe_stats: X")
    if X is not None:
        out = dict(mean=torch.empty(d, device=dev), rstd=torch.empty(d, device=dev), std=torch.empty(d, device=dev), count=torch.empty(d, dtype=torch.float64, device=dev))
    if labels is not None:
        labels = _i32(labels, N, "labels")
        class_weight = _f32(class_weight, int(num_classes), "class_weight")
        out["denom"] = torch.empty(1, dtype=torch.float64, device=dev)
    nb = lib.nv_probe_stats_workspace_bytes(N, d)
    ws = torch.empty(max(nb, 8), dtype=torch.uint8, device=dev)
    check(lib.nv_probe_stats(_p(X), X.stride(0) if X is not None else 0, N, d, int(bool(skip_nan)), float(eps), _p(out.get("mean")), _p(out.get("rstd")),
                             _p(out.get("std")), _p(out.get("count")), _p(labels), int(num_classes), _p(class_weight), _p(out.get("denom")), _p(ws), nb,
                             _stream()), "nv_probe_stats")
    return out


def probe_grad_workspace_bytes(N: int, d: int, M: int) -> int:
    """nv_probe_grad_workspace_bytes: the chunk partials of nv_probe_grad (0 for a shape it refuses)"""
    return int(lib.nv_probe_grad_workspace_bytes(int(N), int(d), int(M)))


def probe_grad(X: torch.Tensor, W: torch.Tensor, b: torch.Tensor, heads, denom: torch.Tensor, *, labels: Optional[torch.Tensor] = None,
               targets: Optional[torch.Tensor] = None, mean: Optional[torch.Tensor] = None, rstd: Optional[torch.Tensor] = None,
               class_weight: Optional[torch.Tensor] = None, target_mean: Optional[torch.Tensor] = None, target_std: Optional[torch.Tensor] = None,
               max_blocks: int = 0, out=None, workspace: Optional[torch.Tensor] = None):
    """nv_probe_grad: loss and gradient of the H heads of `heads` (probe_heads) over X f32 [N, d] in one pass: W f32 [M, d], b f32 [M], M = H C;
    labels int32 [N] (classification; outside [0, C) = unlabelled) or targets f32 [N, C] (regression; NaN = missing); denom f64 [1] / [C] from
    probe_stats.  Returns (dW f32 [M, d], db f32 [M], loss f32 [H]) - `out` = such a triple to write into (loss may be a row of a history)."""
    _need_cuda(X, W, b, denom)
    N, d = _rows2d(X, "probe_grad: X")
    H, C = heads.H, heads.C
    M = H * C
    if d % 4 or d > _cabi.PROBE_MAX_D:
        raise ValueError(f"probe_grad: d = {d} must be a multiple of 4 up to {_cabi.PROBE_MAX_D}")
    if (labels is None) == (targets is None):
        raise ValueError("probe_grad: give labels (classification) or targets (regression), one of the two")
    if (mean is None) != (rstd is None):
        raise ValueError("probe_grad: mean and rstd are given together or not at all")
    if W.dtype != torch.float32 or tuple(W.shape) != (M, d) or not W.is_contiguous():
        raise ValueError(f"probe_grad: W must be a contiguous float32 [{M}, {d}], got {tuple(W.shape)} {W.dtype}")
    b, mean, rstd = _f32(b, M, "b"), _f32(mean, d, "mean"), _f32(rstd, d, "rstd")
    if denom.dtype != torch.float64 or denom.numel() != (1 if labels is not None else C) or not denom.is_contiguous():
        raise ValueError(f"probe_grad: denom must be float64 [{1 if labels is not None else C}]")
    if labels is not None:
        if target_mean is not None or target_std is not None:
            raise ValueError("probe_grad: target_mean / target_std belong to regression")
        labels, class_weight, task = _i32(labels, N, "labels"), _f32(class_weight, C, "class_weight"), 0
    else:
        if class_weight is not None:
            raise ValueError("probe_grad: class_weight belongs to classification")
        targets, task = _f32(targets, N * C, "targets"), 1
        target_mean, target_std = _f32(target_mean, C, "target_mean"), _f32(target_std, C, "target_std")
    dW, db, loss = out if out is not None else (torch.empty_like(W), torch.empty_like(b), torch.empty(H, device=W.device))
    _f32(dW, M * d, "dW"), _f32(db, M, "db"), _f32(loss, H, "loss")
    nb = probe_grad_workspace_bytes(N, d, M)
    ws = workspace if workspace is not None else torch.empty(nb, dtype=torch.uint8, device=X.device)
    check(lib.nv_probe_grad(_p(X), X.stride(0), N, d, _p(mean), _p(rstd), _p(W), _p(b), ctypes.byref(heads), task, _p(labels), _p(class_weight), _p(targets),
                            _p(target_mean), _p(target_std), _p(denom), _p(dW), _p(db), _p(loss), int(max_blocks), _p(ws), ws.numel(), _stream()), "nv_probe_grad")
    return dW, db, loss


def probe_adam_constants(step: int, lrs, betas=(0.9, 0.999)):
    """what the host forms for step `step` (1-based) of nv_probe_step, in double: (lr_h / (1 - beta1^t) per head, sqrt(1 - beta2^t))"""
    bc1, bc2 = 1.0 - betas[0] ** step, 1.0 - betas[1] ** step
    return [float(lr) / bc1 for lr in lrs], bc2 ** 0.5


def probe_step(W, b, dW, db, mW, vW, mb, vb, heads, step: int, betas=(0.9, 0.999), eps: float = 1e-8) -> None:
    """nv_probe_step: one Adam step on W [M, d], b [M] and their moments from dW / db, in place; heads.step holds lr_h / (1 - beta1^t)
    (probe_adam_constants); every fp32 operation rounded on its own - the bits of the same torch fp32 expressions."""
    M, d = W.shape
    _need_cuda(W)
    for t, n, name in ((W, M * d, "W"), (dW, M * d, "dW"), (mW, M * d, "mW"), (vW, M * d, "vW"), (b, M, "b"), (db, M, "db"), (mb, M, "mb"), (vb, M, "vb")):
        _f32(t, n, name)
    if M != heads.H * heads.C:
        raise ValueError(f"probe_step: W has {M} rows, the heads {heads.H} x {heads.C}")
    check(lib.nv_probe_step(_p(W), _p(b), _p(dW), _p(db), _p(mW), _p(vW), _p(mb), _p(vb), d, ctypes.byref(heads), betas[0], betas[1], 1.0 - betas[0], 1.0 - betas[1],
                            (1.0 - betas[1] ** int(step)) ** 0.5, eps, _stream()), "nv_probe_step")


def probe_predict(Q: torch.Tensor, W: torch.Tensor, b: torch.Tensor, H: int, C: int, *, mean=None, rstd=None, want_probs: bool = False, logits=None, probs=None):
    """nv_probe_predict: queries f32 [Nq, d] -> logits f32 [Nq, M] under mean / rstd (M = H C <= 32), and with want_probs the fp32 softmax over
    each head's own C columns.  logits / probs: column windows of wider arrays to write into (their row stride is passed).  Returns (logits, probs or None)."""
    _need_cuda(Q, W, b)
    Nq, d = _rows2d(Q, "probe_predict: Q")
    M = int(H) * int(C)
    if d % 4 or d > _cabi.PROBE_MAX_D:
        raise ValueError(f"probe_predict: d = {d} must be a multiple of 4 up to {_cabi.PROBE_MAX_D}")
    if (mean is None) != (rstd is None):
        raise ValueError("probe_predict: mean and rstd are given together or not at all")
    if W.dtype != torch.float32 or tuple(W.shape) != (M, d) or not W.is_contiguous():
        raise ValueError(f"probe_predict: W must be a contiguous float32 [{M}, {d}], got {tuple(W.shape)} {W.dtype}")
    b, mean, rstd = _f32(b, M, "b"), _f32(mean, d, "mean"), _f32(rstd, d, "rstd")
    if logits is None:
        logits = torch.empty((Nq, M), device=Q.device)
    if probs is None and want_probs:
        probs = torch.empty((Nq, M), device=Q.device)
    for t in (logits, probs):
        if t is not None and (t.dtype != torch.float32 or tuple(t.shape) != (Nq, M) or t.stride(1) != 1 or not t.is_cuda):
            raise ValueError(f"probe_predict: logits / probs must be float32 [{Nq}, {M}] windows with unit column stride on the device")
    check(lib.nv_probe_predict(_p(Q), Q.stride(0), Nq, d, _p(mean), _p(rstd), _p(W), _p(b), int(H), int(C), _p(logits), logits.stride(0), _p(probs),
                               probs.stride(0) if probs is not None else 0, _stream()), "nv_probe_predict")
    return logits, probs
