"""Dropout-mask read-out: inputs under which a kernel's output IS the dropout mask it applied, and the proof - on the CPU oracle - that they work.

Every kernel of the train step regenerates its nn.Dropout mask from (seed, element index) (csrc/common.h: nv_hash64, drop_factor4,
drop_factor; the dK/dV pass of csrc/attention.hip has a hand-rolled form, drop_factor_rows4), forward and again backward; nothing is stored.
oracle/ref_cpu.py restates the mask bit for bit (drop_mask, drop_mask_at, attn_drop_mask, site_seed).  The builders below feed constants
so that every mask cell lands in one output element, exactly:

attention, Q = 0 (every score 0, P = 1 / n whatever K holds; lse = log n), dh columns of the mask per pass t:
  forward   V[key, c] = [key == dh t + c]                               ->  out[q, c] = r16(r16(P f[q, dh t + c]) / l) = f / n
  dK / dV   out = 0 (delta = 0), dO[q, c] = [q == dh t + c], any V      ->  dV[key, c] = r16(P f[dh t + c, key])
  dQ        out = 0, dO[:, 0] = 1, V[:, 0] = 1 (dP = 1), K[key, c] = [key == dh t + c]
                                                                        ->  dQ[q, c] = r16(scale r16(P f[q, dh t + c]))
  f = 0 or fl32(1 / (1 - p)); r16 = round to nearest even to the 16-bit operand format.
GEMM epilogues: A = 0, bias = 1, residual = 0 -> bias + residual returns f itself (fp32, bit exact), bias + GELU returns r16(gelu(1) f);
  A = ones[M, 8], B = ones[8, N], u = 0 -> dGELU returns r16(8 f gelu'(0)) = r16(4 f).

Gates (none of them measured on the code under test):
  zero pattern   exact: (output != 0) == (oracle mask != 0), every cell; columns of a pass beyond n exactly zero.
  kept values    fp32 outputs bit exact.  16-bit outputs within ONE step of the operand format of the stated value (ulp_steps: the two
                 16-bit words are equal or neighbours): the kernels reach the value through fp32 intermediates (1 / n by exp2 and a
                 reciprocal, gelu by a polynomial: a few fp32 ulp, 2^-23 relative) and, in the forward, through a second 16-bit rounding
                 (r16(P f) first, the division by l afterwards), so a value near a rounding boundary of the 16-bit format (2^-9 / 2^-12
                 relative) may fall to the other side of it - by one step, never by two.
This file runs the builders through ref_cpu._AttnEmu (the kernels' cast points on the CPU) and plain torch arithmetic: decoding the passes
returns the oracle's mask exactly and the oracle itself stays inside the value gate.  tests/test_dropout_masks_gpu.py runs the same builders
through the HIP kernels."""
import functools
import math
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from oracle import ref_cpu

SEED = ref_cpu.site_seed(123456789, 5)          # above 2^32: a seed truncated to 32 bits anywhere on the way gives another mask
assert SEED > 1 << 32
PS = (0.1, 0.5)                                 # 0.1: p * 65536 is not an integer (the threshold is its floor); 0.5: 1 / (1 - p) is exact
FORMATS = {"bf16": torch.bfloat16, "fp16": torch.float16}


# --------------------------------------------------------------------------------------------- expected values and the one-step gate
def drop_scale(p):
    """fl32(1 / (1 - p)) as csrc/common.h::make_drop forms it"""
    return float(np.float32(1.0) / (np.float32(1.0) - np.float32(p)))


def r16(value, dtype):
    """a Python float rounded to the 16-bit format, as fp32"""
    return torch.tensor(value, dtype=torch.float64).to(torch.float32).to(dtype).float()


def ulp_steps(got, want, dtype):
    """Distance in representable values of `dtype` between two tensors of positive finite values (fp32 storage, both representable):
    the difference of their 16-bit words, which are monotonic in the value."""
    a = got.to(dtype).contiguous().view(torch.int16).to(torch.int32)
    b = torch.as_tensor(want).to(dtype).contiguous().view(torch.int16).to(torch.int32)
    return (a - b).abs()


@functools.lru_cache(maxsize=None)
def attn_mask(p, B, heads, n):
    """the oracle's attention mask, computed once per shape and shared (read only)"""
    return ref_cpu.attn_drop_mask(SEED, p, B, heads, n)


def check_readout(seen, mask, want, dtype, what):
    """seen: the decoded factors-times-constant (fp32, shape of mask).  Zero pattern exact, every kept value within one step of `want`.
    Returns (cells compared, mismatching cells) for the report."""
    seen = seen.detach().float().cpu()
    bad = int(((seen != 0) != (mask != 0)).sum())
    assert torch.equal(seen != 0, mask != 0), f"{what}: {bad} of {mask.numel()} mask cells differ from the oracle's mask"
    kept = seen[mask != 0]
    steps = ulp_steps(kept, want, dtype)
    assert int(steps.max()) <= 1, f"{what}: kept value {kept[steps.argmax()].item():.9g}, expected {float(want):.9g} within one step of the 16-bit format ({int(steps.max())} steps)"
    return mask.numel(), bad


# --------------------------------------------------------------------------------------------- attention read-out builders
def n_passes(n, dh):
    return (n + dh - 1) // dh


def qkv_forward_pass(B, heads, n, dh, t, dtype, device="cpu"):
    """qkv [B * n, 3 * inner]: Q = K = 0, V[key, c] = 1 iff key == dh t + c (keys beyond n do not exist: those columns stay 0)"""
    qkv = torch.zeros((B, n, 3, heads, dh), dtype=dtype, device=device)
    keys = torch.arange(dh * t, min(dh * t + dh, n), device=device)
    qkv[:, keys, 2, :, keys - dh * t] = 1
    return qkv.reshape(B * n, 3 * heads * dh)


def any_v(n, dh, dtype, device="cpu"):
    """a V that is neither zero nor constant, exact in both formats"""
    key, c = torch.arange(n, device=device)[:, None], torch.arange(dh, device=device)[None, :]
    return (((key * 7 + c * 3) % 5 - 2) * 0.25).to(dtype)


def dkv_pass(B, heads, n, dh, t, dtype, device="cpu"):
    """(qkv, dout): Q = K = 0, V = any_v; dO[q, c] = 1 iff q == dh t + c"""
    qkv = torch.zeros((B, n, 3, heads, dh), dtype=dtype, device=device)
    qkv[:, :, 2] = any_v(n, dh, dtype, device)[None, :, None, :]
    dout = torch.zeros((B, n, heads, dh), dtype=dtype, device=device)
    rows = torch.arange(dh * t, min(dh * t + dh, n), device=device)
    dout[:, rows, :, rows - dh * t] = 1
    return qkv.reshape(B * n, 3 * heads * dh), dout.reshape(B * n, heads * dh)


def dq_pass(B, heads, n, dh, t, dtype, device="cpu"):
    """(qkv, dout): Q = 0, V[:, 0] = 1, K[key, c] = 1 iff key == dh t + c; dO[:, 0] = 1 - so dP = dO V^T = 1 everywhere"""
    qkv = torch.zeros((B, n, 3, heads, dh), dtype=dtype, device=device)
    qkv[:, :, 2, :, 0] = 1
    keys = torch.arange(dh * t, min(dh * t + dh, n), device=device)
    qkv[:, keys, 1, :, keys - dh * t] = 1
    dout = torch.zeros((B, n, heads, dh), dtype=dtype, device=device)
    dout[..., 0] = 1
    return qkv.reshape(B * n, 3 * heads * dh), dout.reshape(B * n, heads * dh)


def _width(n, dh, t):
    return min(dh, n - dh * t)


def decode_forward(seen, out, B, heads, n, dh, t):
    """out [B * n, inner] of pass t -> seen[b, h, q, dh t + c]; the columns of keys beyond n must be exactly zero"""
    o = out.reshape(B, n, heads, dh).permute(0, 2, 1, 3).float()
    w = _width(n, dh, t)
    assert not o[..., w:].any(), f"pass {t}: columns of keys beyond n are not zero"
    seen[:, :, :, dh * t:dh * t + w] = o[..., :w]


def decode_dkv(seen, dqkv, B, heads, n, dh, t):
    """dV (third of dqkv [B * n, 3 * inner]) of pass t: dV[key, c] -> seen[b, h, dh t + c, key]; dK must be exactly zero (Q = 0)"""
    d = dqkv.reshape(B, n, 3, heads, dh).float()
    w = _width(n, dh, t)
    assert not d[:, :, 1].any(), f"pass {t}: dK is not zero although Q = 0"
    dv = d[:, :, 2].permute(0, 2, 3, 1)                     # [B, heads, c, key]
    assert not dv[:, :, w:].any(), f"pass {t}: columns of query rows beyond n are not zero"
    seen[:, :, dh * t:dh * t + w, :] = dv[:, :, :w]


def decode_dq(seen, dqkv, B, heads, n, dh, t):
    """dQ (first third of dqkv) of pass t: dQ[q, c] -> seen[b, h, q, dh t + c]"""
    dq = dqkv.reshape(B, n, 3, heads, dh)[:, :, 0].permute(0, 2, 1, 3).float()
    w = _width(n, dh, t)
    assert not dq[..., w:].any(), f"pass {t}: columns of keys beyond n are not zero"
    seen[:, :, :, dh * t:dh * t + w] = dq[..., :w]


def want_forward(p, n, dtype):
    return r16(drop_scale(p) / n, dtype)


def want_dv(p, n, dtype):
    return r16(drop_scale(p) / n, dtype)


def want_dq(p, n, dh, dtype):
    """scale * r16(P f), rounded once more on the way out; dh ** -0.5 in fp32 as the caller passes it"""
    return r16(float(np.float32(dh ** -0.5)) * float(r16(drop_scale(p) / n, dtype)), dtype)


# --------------------------------------------------------------------------------------------- the oracle through the builders
def _split(qkv, B, heads, n, dh):
    return (x.reshape(B, n, heads, dh).permute(0, 2, 1, 3).float() for x in qkv.chunk(3, dim=-1))


def _emu_backward(qkv, dout, mask, B, heads, n, dh):
    """ref_cpu._AttnEmu.backward on the builders' inputs with the kernels' saved tensors: out = 0 and lse = log n"""
    q, k, v = _split(qkv, B, heads, n, dh)
    lse = torch.full((B, heads, n, 1), float(np.float32(math.log(n))))
    ctx = SimpleNamespace(saved_tensors=(q, k, v, torch.zeros_like(q), lse), scale=dh ** -0.5, mask=mask)
    do = dout.reshape(B, n, heads, dh).permute(0, 2, 1, 3).float()
    dq, dk, dv, _, _ = ref_cpu._AttnEmu.backward(ctx, do)
    return torch.cat([x.permute(0, 2, 1, 3).reshape(B * n, heads * dh) for x in (dq, dk, dv)], dim=-1)


@pytest.mark.parametrize("p", PS)
@pytest.mark.parametrize("fmt", list(FORMATS))
@pytest.mark.parametrize("B,heads,n", [(2, 2, 65), (1, 2, 130)])
def test_attention_readout_recovers_the_oracle_mask_on_the_oracle(B, heads, n, fmt, p):
    """The three read-outs through ref_cpu._AttnEmu (the kernels' cast points): decoding the passes gives attn_drop_mask != 0 for every
    (b, h, q, key) - the builders see every cell - and the kept values stay inside the one-step gate the GPU tests apply."""
    dh, dtype = 64, FORMATS[fmt]
    mask = attn_mask(p, B, heads, n)
    seen_f, seen_v, seen_q = (torch.full((B, heads, n, n), float("nan")) for _ in range(3))
    with ref_cpu.operand_format(fmt):
        for t in range(n_passes(n, dh)):
            q, k, v = _split(qkv_forward_pass(B, heads, n, dh, t, dtype), B, heads, n, dh)
            out = ref_cpu._AttnEmu.apply(q, k, v, dh ** -0.5, mask)
            decode_forward(seen_f, out.permute(0, 2, 1, 3).reshape(B * n, heads * dh), B, heads, n, dh, t)
            decode_dkv(seen_v, _emu_backward(*dkv_pass(B, heads, n, dh, t, dtype), mask, B, heads, n, dh), B, heads, n, dh, t)
            decode_dq(seen_q, _emu_backward(*dq_pass(B, heads, n, dh, t, dtype), mask, B, heads, n, dh), B, heads, n, dh, t)
    for seen in (seen_f, seen_v, seen_q):
        assert not torch.isnan(seen).any()                    # every cell was written by some pass
    check_readout(seen_f, mask, want_forward(p, n, dtype), dtype, "oracle forward")
    check_readout(seen_v, mask, want_dv(p, n, dtype), dtype, "oracle dV")
    check_readout(seen_q, mask, want_dq(p, n, dh, dtype), dtype, "oracle dQ")
    assert 0 < int((mask == 0).sum()) < mask.numel()          # a mask with both kinds of cells


@pytest.mark.parametrize("p", PS)
@pytest.mark.parametrize("fmt", list(FORMATS))
def test_the_double_rounding_of_the_forward_stays_inside_one_step(fmt, p):
    """The forward rounds P f to 16 bits before the division by l: r16(r16(f) / n) against the stated r16(f / n) for every n the GPU
    tests use - and for every n up to 4097 - differs by at most one step (here by arithmetic alone, no kernel involved)."""
    dtype = FORMATS[fmt]
    n = torch.arange(1, 4098, dtype=torch.float64)
    f = drop_scale(p)
    twice = (float(r16(f, dtype)) / n).float().to(dtype).float()
    once = (f / n).float().to(dtype).float()
    assert int(ulp_steps(twice, once, dtype).max()) <= 1


def test_gemm_constants_return_the_mask():
    """The GEMM read-outs with plain fp32 torch arithmetic in the epilogues' order (csrc/gemm_common.h::epilogue4): (0 + bias) * f + 0 is f,
    bit for bit; gelu(1) * f and (8 * f) * gelu'(0) land within one step of the stated r16(gelu(1) f) and r16(4 f) in both formats."""
    M, N = 130, 136
    for p in PS:
        f = ref_cpu.drop_mask(SEED, p, (M, N))
        acc, bias, resid = torch.zeros(M, N), torch.ones(N), torch.zeros(M, N)
        assert torch.equal((acc + bias) * f + resid, f)
        for dtype in FORMATS.values():
            h = (torch.nn.functional.gelu(acc + bias) * f).to(dtype).float()
            check_readout(h, f, want_gelu(p, dtype), dtype, "gelu constants")
            du = (torch.full((M, N), 8.0) * f * ref_cpu._gelu_grad(torch.zeros(M, N))).to(dtype).float()
            check_readout(du, f, want_dgelu(p, dtype), dtype, "dgelu constants")


def want_gelu(p, dtype):
    return r16(0.5 * (1.0 + math.erf(2.0 ** -0.5)) * drop_scale(p), dtype)


def want_dgelu(p, dtype):
    return r16(4.0 * drop_scale(p), dtype)
