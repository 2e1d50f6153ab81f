"""Every dropout mask of the HIP path read back exactly, kernel by kernel, against the oracle's restatement (ref_cpu.drop_mask /
drop_mask_at / attn_drop_mask).  The inputs (tests/test_dropout_masks_cpu.py, where the oracle proves them) make a kernel's output
its mask: zero patterns are compared with torch.equal over every cell, fp32 outputs bit for bit, 16-bit outputs within the one step
of the operand format derived there.  No cell is excluded and nothing is statistical.

  attention, dh = 64   streaming / resident / resident with partner waves / wide forward; streaming / resident / merged resident / wide
                       backward (dQ pass: drop_factor4, dK / dV pass: drop_factor_rows4), bf16 and fp16 instantiations, ragged tiles,
                       npad != n, several (batch, head) slices, a seed above 2^32; one case whose element index passes 2^32
  attention, dh != 64  attention_generic.hip, the same three read-outs
  GEMM epilogues       bias + residual, bias + GELU, dGELU, dGELU + column sums in every tile family; the skinny cls-row kernels
  row kernels          nv_dropout_apply, nv_ln_bwd, nv_embed_finish_fwd / _bwd, nv_head_bwd (both pools), nv_head_step
One report line per kernel family: mask cells compared, cells that differed."""
import contextlib
import functools
import math

import pytest
import torch
import torch.nn.functional as F

from conftest import rel_err, report
from oracle import ref_cpu
from test_dropout_masks_cpu import (FORMATS, PS, SEED, attn_mask, check_readout, decode_dkv, decode_dq, decode_forward, dkv_pass, dq_pass,
                                    n_passes, qkv_forward_pass, want_dgelu, want_dq, want_dv, want_forward, want_gelu)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ops():
    from neurovit_amd import ops as _ops
    from neurovit_amd._cabi import require_gpu
    require_gpu()
    return _ops


@pytest.fixture(scope="module")
def tally():
    """{kernel family: [mask cells compared, cells that differed from the oracle]} - one report line each when the module is done"""
    counts = {}
    yield counts
    for family, (cells, bad) in counts.items():
        report(f"dropout mask read-out, {family}: {cells} mask cells compared with the oracle, {bad} mismatches")


def gate(tally, family, seen, mask, want, dtype, what):
    """count, then assert (check_readout: zero pattern exact, kept values within one step of `want`)"""
    seen = seen.detach().float().cpu()
    c = tally.setdefault(family, [0, 0])
    c[0] += mask.numel()
    c[1] += int(((seen != 0) != (mask != 0)).sum())
    check_readout(seen, mask, want, dtype, f"{family}, {what}")


def gate_exact(tally, family, got, want, what):
    """fp32 / already rounded outputs: bit for bit"""
    got = got.detach().cpu()
    c = tally.setdefault(family, [0, 0])
    c[0] += want.numel()
    bad = int(((got != 0) != (want != 0)).sum())
    c[1] += bad
    assert torch.equal(got != 0, want != 0), f"{family}, {what}: {bad} of {want.numel()} mask cells differ from the oracle's mask"
    assert torch.equal(got, want), f"{family}, {what}: values differ, max {float((got.double() - want.double()).abs().max()):.3e}"


@contextlib.contextmanager
def operands(fmt):
    from neurovit_amd import _cabi
    _cabi.set_operand_format(fmt)
    try:
        yield FORMATS[fmt]
    finally:
        _cabi.set_operand_format("bf16")


@contextlib.contextmanager
def attn_mode(mode):
    from neurovit_amd._cabi import lib
    lib.nv_attn_set_mode(mode)
    try:
        yield
    finally:
        lib.nv_attn_set_mode(0)


def close32(a, b, what, rel=1e-5):
    e = rel_err(a, b)
    assert e <= rel, f"{what}: rel err {e:.3e} > {rel}"


# ------------------------------------------------------------------------------------------------------------ attention
ATTN_SHAPES = [(2, 2, 65), (1, 3, 130), (2, 2, 513), (1, 2, 577), (1, 2, 1001)]       # npad != n (all), one-row ragged tile (513), first n past the
                                                                                      # resident limit (577), the reference geometry (1001)
GENERIC = [(1, 2, 70, 32), (1, 1, 130, 128)]
FWD_NAMES = {0: "generic", 1: "streaming", 2: "resident", 22: "resident, partner waves", 3: "wide"}
BWD_NAMES = {0: "generic", 1: "streaming", 2: "resident", 102: "resident, merged launch", 3: "wide"}


def resident(n):
    """csrc/attention.hip::attn_resident: the LDS-resident kernels take at most RES_MAX_TILES = 9 key tiles of 64 (n <= 576); beyond, a resident
    mode runs the kernels another mode already names, so those combinations are not listed"""
    return (n + 63) // 64 <= 9


FWD_CASES = [(B, h, n, 64, m) for (B, h, n) in ATTN_SHAPES for m in (1, 2, 22, 3) if m in (1, 3) or resident(n)] + [s + (0,) for s in GENERIC]
BWD_CASES = [(B, h, n, 64, m) for (B, h, n) in ATTN_SHAPES for m in (1, 2, 102, 3) if m in (1, 3) or resident(n)] + [s + (0,) for s in GENERIC]


@pytest.mark.parametrize("p", PS)
@pytest.mark.parametrize("fmt", list(FORMATS))
@pytest.mark.parametrize("B,heads,n,dh,mode", FWD_CASES)
def test_attention_forward_applies_the_oracle_mask(ops, tally, B, heads, n, dh, mode, fmt, p):
    """out[q, c] = f[q, dh t + c] / n over the passes t: the factor of every (b, h, q, key) the forward kernel applied."""
    mask = attn_mask(p, B, heads, n)
    seen = torch.full((B, heads, n, n), float("nan"), device="cuda")
    with operands(fmt) as dtype, attn_mode(mode):
        for t in range(n_passes(n, dh)):
            out, lse = ops.attn_fwd(qkv_forward_pass(B, heads, n, dh, t, dtype, "cuda"), B, n, heads, dh, drop_seed=SEED, drop_p=p)
            decode_forward(seen, out, B, heads, n, dh, t)
            close32(lse, torch.full((B, heads, n), math.log(n), dtype=torch.float64), f"lse, pass {t}", 1e-6)      # dropout leaves the normaliser alone
    assert not torch.isnan(seen).any()
    gate(tally, f"attention forward, dh = {dh}, {FWD_NAMES[mode]}", seen, mask, want_forward(p, n, dtype), dtype, f"B {B} heads {heads} n {n} {fmt} p {p}")


@pytest.mark.parametrize("p", PS)
@pytest.mark.parametrize("fmt", list(FORMATS))
@pytest.mark.parametrize("B,heads,n,dh,mode", BWD_CASES)
def test_attention_backward_applies_the_oracle_mask(ops, tally, B, heads, n, dh, mode, fmt, p):
    """dV[key, c] = r16(P f[dh t + c, key]) (the dK / dV pass: drop_factor_rows4 in the MFMA kernels) and dQ[q, c] = scale r16(P f[q, dh t + c])
    (the dQ pass) over the passes t, with out = 0 (delta = 0) and lse = log n."""
    mask = attn_mask(p, B, heads, n)
    seen_v, seen_q = (torch.full((B, heads, n, n), float("nan"), device="cuda") for _ in range(2))
    lse = torch.full((B, heads, n), math.log(n), device="cuda")
    with operands(fmt) as dtype, attn_mode(mode):
        zero_out = torch.zeros((B * n, heads * dh), dtype=dtype, device="cuda")
        for t in range(n_passes(n, dh)):
            qkv, dout = dkv_pass(B, heads, n, dh, t, dtype, "cuda")
            dqkv, delta = ops.attn_bwd(qkv, zero_out, dout, lse, B, n, heads, dh, drop_seed=SEED, drop_p=p)
            assert not delta.any()
            decode_dkv(seen_v, dqkv, B, heads, n, dh, t)
            qkv, dout = dq_pass(B, heads, n, dh, t, dtype, "cuda")
            dqkv, _ = ops.attn_bwd(qkv, zero_out, dout, lse, B, n, heads, dh, drop_seed=SEED, drop_p=p)
            decode_dq(seen_q, dqkv, B, heads, n, dh, t)
    assert not torch.isnan(seen_v).any() and not torch.isnan(seen_q).any()
    what = f"B {B} heads {heads} n {n} {fmt} p {p}"
    gate(tally, f"attention dK/dV pass, dh = {dh}, {BWD_NAMES[mode]}", seen_v, mask, want_dv(p, n, dtype), dtype, what)
    gate(tally, f"attention dQ pass, dh = {dh}, {BWD_NAMES[mode]}", seen_q, mask, want_dq(p, n, dh, dtype), dtype, what)


def test_attention_mask_index_beyond_2_to_the_32(ops, tally):
    """B * heads = 264 at n = 4097: the element index (bh n + q) npad + key of the last two (batch, head) slices lies beyond 2^32.  One
    read-out pass - the last key tile, which holds key 4096 alone; for the dK / dV pass the last query tile - through the wide and
    the streaming forward and the default backward (the wide kernels at this size); the last two slices against ref_cpu.drop_mask_at."""
    B, heads, n, dh, p, dtype = 264, 1, 4097, 64, 0.1, torch.bfloat16
    npad, t = (n + 3) // 4 * 4, 4096 // 64
    first = (B - 2) * n * npad
    assert first > 1 << 32
    mask = ref_cpu.drop_mask_at(SEED, p, first, 2 * n * npad).reshape(2, n, npad)[:, :, :n]
    col, row = mask[:, :, 4096].contiguous(), mask[:, 4096, :].contiguous()           # f[q, 4096] and f[4096, key] of the two slices
    qkv = qkv_forward_pass(B, heads, n, dh, t, dtype, "cuda")
    for mode in (3, 1):
        with attn_mode(mode):
            out, lse = ops.attn_fwd(qkv, B, n, heads, dh, drop_seed=SEED, drop_p=p)
        o = out.reshape(B, n, dh)[-2:].float()
        assert not o[..., 1:].any()
        gate(tally, f"attention forward, index beyond 2^32, {FWD_NAMES[mode]}", o[..., 0], col, want_forward(p, n, dtype), dtype, "n 4097")
        close32(lse[-2:], torch.full((2, heads, n), math.log(n), dtype=torch.float64), "lse", 1e-6)
        del out, lse, o
    del qkv
    lse = torch.full((B, heads, n), math.log(n), device="cuda")
    zero_out = torch.zeros((B * n, dh), dtype=dtype, device="cuda")
    qkv, dout = dkv_pass(B, heads, n, dh, t, dtype, "cuda")
    dqkv, _ = ops.attn_bwd(qkv, zero_out, dout, lse, B, n, heads, dh, drop_seed=SEED, drop_p=p)
    dv = dqkv.reshape(B, n, 3, dh)[-2:, :, 2].float()
    assert not dv[..., 1:].any()
    gate(tally, "attention dK/dV pass, index beyond 2^32, default (wide)", dv[..., 0], row, want_dv(p, n, dtype), dtype, "n 4097")
    del qkv, dout, dqkv, dv
    qkv, dout = dq_pass(B, heads, n, dh, t, dtype, "cuda")
    dqkv, _ = ops.attn_bwd(qkv, zero_out, dout, lse, B, n, heads, dh, drop_seed=SEED, drop_p=p)
    dq = dqkv.reshape(B, n, 3, dh)[-2:, :, 0].float()
    assert not dq[..., 1:].any()
    gate(tally, "attention dQ pass, index beyond 2^32, default (wide)", dq[..., 0], col, want_dq(p, n, dh, dtype), dtype, "n 4097")


# ------------------------------------------------------------------------------------------------------------ GEMM epilogues
@functools.lru_cache(maxsize=None)
def dense_mask(p, M, N):
    return ref_cpu.drop_mask(SEED, p, (M, N))


TILES = [(0, 0), (1, 0), (3, 0), (4, 0), (9, 0), (11, 1)]      # heuristic, 128 x 128, 64 x 128, 256 x 128 ping-pong, 256 x 256; ping-pong NT on the 32 x 32 x 16 MFMA
TILE_NAMES = {0: "heuristic", 1: "128 x 128", 3: "64 x 128", 4: "256 x 128", 9: "256 x 256", 11: "256 x 128, 32 x 32 x 16 MFMA"}


@pytest.mark.parametrize("M,N", [(257, 264), (130, 136), (300, 8), (2052, 768)])
@pytest.mark.parametrize("tile", TILES)
def test_gemm_epilogues_apply_the_oracle_mask(ops, tally, tile, M, N):
    """A = 0, bias = 1, residual = 0: bias + residual returns the factor of element m N + n itself; bias + GELU returns r16(gelu(1) f) beside an
    unmasked u = 1; dGELU (A = ones[M, 8], B = ones[8, N], u = 0) returns r16(4 f), its fused column sums count the kept cells.
    K = 8 reaches the small-tile kernel only, whatever tile is forced (csrc/gemm.hip::plan_gemm: the large-tile families take whole 64-deep K
    tiles of K-contiguous operands), so the forced tiles run the same operands as [., 64] with the columns beyond the eighth zero: the same
    accumulators, in the kernel family the tile names.  The heuristic runs both."""
    from neurovit_amd._cabi import lib
    dtype = torch.bfloat16
    family = f"GEMM epilogues, tile {TILE_NAMES[tile[0]]}"
    bias, resid = torch.ones(N, device="cuda"), torch.zeros((M, N), device="cuda")
    u0 = torch.zeros((M, N), dtype=dtype, device="cuda")
    if tile[0] == 11:
        lib.nv_gemm_set_tile(4, 0)
    lib.nv_gemm_set_tile(*tile)
    try:
        for p, K in [(p, K) for p in PS for K in ((8, 64) if tile[0] == 0 else (64,))]:
            A0, B0 = torch.zeros((M, K), dtype=dtype, device="cuda"), torch.zeros((N, K), dtype=dtype, device="cuda")
            A1, B1 = torch.zeros((M, K), dtype=dtype, device="cuda"), torch.ones((K, N), dtype=dtype, device="cuda")
            A1[:, :8] = 1
            mask = dense_mask(p, M, N)
            out = ops.gemm(ops.NT, ops.EPI_BIAS_RESID, A0, B0, bias=bias, aux_in=resid, drop_seed=SEED, drop_p=p)
            gate_exact(tally, family, out, mask, f"bias + residual [{M}, {N}] p {p}")
            u = torch.empty((M, N), dtype=dtype, device="cuda")
            h = ops.gemm(ops.NT, ops.EPI_BIAS_GELU, A0, B0, bias=bias, aux_out=u, drop_seed=SEED, drop_p=p)
            assert bool((u == 1).all()), "the pre-activation is not masked"
            gate(tally, family, h, mask, want_gelu(p, dtype), dtype, f"bias + GELU [{M}, {N}] p {p}")
            if tile[0] == 11:          # the switch concerns the NT problems only
                continue
            du = ops.gemm(ops.NN, ops.EPI_DGELU, A1, B1, aux_in=u0, drop_seed=SEED, drop_p=p)
            gate(tally, family, du, mask, want_dgelu(p, dtype), dtype, f"dGELU [{M}, {N}] p {p}")
            if lib.nv_gemm_tile_rows(ops.NN, M, N, K, A1.stride(0), B1.stride(0)):      # 0: this shape has no kernel with the fused column sums
                fused, part = ops.gemm_dgelu_colsum(A1, B1, u0, drop_seed=SEED, drop_p=p)
                gate(tally, family, fused, mask, want_dgelu(p, dtype), dtype, f"dGELU + column sums [{M}, {N}] p {p}")
                assert torch.equal(fused, du)
                # count x value: every partial sum is a small integer times one 8-bit significand - exact in fp32 in any order
                assert torch.equal(part.double().sum(0).cpu(), (mask != 0).sum(0).double() * float(du.float().max()))
    finally:
        if tile[0] == 11:
            lib.nv_gemm_set_tile(11, 0)
        lib.nv_gemm_set_tile(0, 0)


def test_skinny_kernels_apply_the_oracle_mask_of_the_dense_tensor(ops, tally):
    """nv_skinny_nt (epilogues 0, 1) / nv_skinny_nn (epilogue 0) on every 513th row of dense [2052, .] tensors: the factors are those of
    the dense tensor's elements at these rows, as the oracle gives them."""
    R, n, K, dtype = 4, 513, 8, torch.bfloat16
    M = R * n
    family = "skinny cls-row kernels"
    for p in PS:
        N = 768                                                                    # out-projection / FC2: f32 = resid + (bias + A W^T) f
        rows = dense_mask(p, M, N)[::n]
        y = torch.full((M, N), 3.0, device="cuda")
        ops.skinny_nt(0, torch.zeros((M, K), dtype=dtype, device="cuda")[::n], torch.zeros((N, K), dtype=dtype, device="cuda"), torch.ones(N, device="cuda"),
                      y[::n], resid=torch.zeros((M, N), device="cuda")[::n], drop_seed=SEED, drop_p=p)
        gate_exact(tally, family, y[::n], rows, f"nt epilogue 0 p {p}")
        keep = torch.ones(M, dtype=torch.bool); keep[::n] = False
        assert bool((y.cpu()[keep] == 3.0).all())
        N = 3072                                                                   # FC1: bf16 = gelu(bias + A W^T) f, u unmasked
        rows = dense_mask(p, M, N)[::n]
        h, u = (torch.zeros((M, N), dtype=dtype, device="cuda") for _ in range(2))
        ops.skinny_nt(1, torch.zeros((M, K), dtype=dtype, device="cuda")[::n], torch.zeros((N, K), dtype=dtype, device="cuda"), torch.ones(N, device="cuda"),
                      h[::n], u_out=u[::n], drop_seed=SEED, drop_p=p)
        assert bool((u[::n] == 1).all())
        gate(tally, family, h[::n], rows, want_gelu(p, dtype), dtype, f"nt epilogue 1 p {p}")
        du, dcol = torch.zeros((M, N), dtype=dtype, device="cuda"), torch.zeros(N, device="cuda")      # dU = (A W f) gelu'(u)
        ops.skinny_nn(0, torch.ones((M, K), dtype=dtype, device="cuda")[::n], torch.ones((K, N), dtype=dtype, device="cuda"), du[::n],
                      u=torch.zeros((M, N), dtype=dtype, device="cuda")[::n], dcol=dcol, drop_seed=SEED, drop_p=p)
        gate(tally, family, du[::n], rows, want_dgelu(p, dtype), dtype, f"nn epilogue 0 p {p}")
        assert torch.equal(dcol.double().cpu(), (rows != 0).sum(0).double() * float(du.float().max()))


# ------------------------------------------------------------------------------------------------------------ row kernels
def rnd(*shape, seed=0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


ROW_SHAPES = [(65, 192), (2052, 768)]


@pytest.mark.parametrize("fmt", list(FORMATS))
@pytest.mark.parametrize("M,N", ROW_SHAPES)
def test_dropout_apply_writes_the_oracle_mask(tally, ops, M, N, fmt):
    """nv_dropout_apply on ones: the fp32 output is the mask of element m N + n, the 16-bit output its rounding - through leading dimensions
    wider than N on the input and on both outputs (the index must not follow them); the padding columns stay untouched."""
    from neurovit_amd._cabi import check, lib
    for p in PS:
        mask = dense_mask(p, M, N)
        with operands(fmt) as dtype:
            x = torch.ones((M, N + 8), device="cuda")
            o16 = torch.full((M, N + 16), 7.0, dtype=dtype, device="cuda")
            o32 = torch.full((M, N + 4), 7.0, device="cuda")
            check(lib.nv_dropout_apply(x.data_ptr(), N + 8, M, N, SEED, p, o16.data_ptr(), N + 16, o32.data_ptr(), N + 4, torch.cuda.current_stream().cuda_stream),
                  "nv_dropout_apply")
            gate_exact(tally, "nv_dropout_apply", o32[:, :N], mask, f"f32 [{M}, {N}] {fmt} p {p}")
            gate_exact(tally, "nv_dropout_apply", o16[:, :N].float(), mask.to(dtype).float(), f"16-bit [{M}, {N}] {fmt} p {p}")
            assert bool((o16[:, N:] == 7).all()) and bool((o32[:, N:] == 7).all())


@pytest.mark.parametrize("M,d", ROW_SHAPES)
def test_ln_bwd_masks_its_16_bit_gradient_with_the_oracle_mask(ops, tally, M, d):
    """nv_ln_bwd: g_out = g_in + dLN(dy) leaves unmasked (fp64 restatement); g16 = r16(g_out f) with f of element row d + c - one fp32 multiply
    of a value the kernel also stores, so bit for bit; the column sums are those of g_out f."""
    x, gamma, beta = rnd(M, d, seed=1) * 2 + 0.3, 1 + 0.1 * rnd(d, seed=2), 0.1 * rnd(d, seed=3)
    dy, g_in = rnd(M, d, seed=4), rnd(M, d, seed=5)
    _, st = ops.ln_fwd(x.cuda(), gamma.cuda(), beta.cuda())
    xd = x.double().requires_grad_(True)
    F.layer_norm(xd, (d,), gamma.double(), beta.double(), 1e-5).backward(dy.double())
    want = xd.grad + g_in.double()
    for p in PS:
        mask = dense_mask(p, M, d)
        g_out, g16, dg, db, dc = ops.ln_bwd(dy.cuda(), x.cuda(), st, gamma.cuda(), g_in=g_in.clone().cuda(), drop_seed=SEED, drop_p=p)
        close32(g_out, want, "ln_bwd.g_out")
        g = g_out.cpu()
        assert bool((g != 0).all())
        gate_exact(tally, "nv_ln_bwd", g16.float(), (g * mask).to(torch.bfloat16).float(), f"g16 [{M}, {d}] p {p}")
        assert torch.equal(g16.cpu() != 0, mask != 0)
        close32(dc, (want * mask.double()).sum(0), "ln_bwd.colsum")


def test_embed_finish_applies_the_oracle_mask(ops, tally):
    """nv_embed_finish_fwd masks x [B (N + 1), d] at element r d + c: with gamma = 0, beta = 1, pos = 0, cls = 1 the output is the mask itself, bit for
    bit, cls rows included; with ordinary parameters it is the fp64 restatement times the mask.  nv_embed_finish_bwd masks the incoming gradient in
    place: a gradient of ones comes back as the mask, and with gamma = 1 everything behind it is the fp64 backward of the masked gradient."""
    B, N, d = 2, 64, 192
    t, pos, cls = rnd(B * N, d, seed=1), rnd(N + 1, d, seed=4), rnd(d, seed=5)
    gamma, beta = 1 + 0.1 * rnd(d, seed=2), 0.1 * rnd(d, seed=3)
    one, zero = torch.ones(d, device="cuda"), torch.zeros(d, device="cuda")
    for p in PS:
        mask = dense_mask(p, B * (N + 1), d)
        x, _ = ops.embed_finish_fwd(t.cuda(), B, N, zero, one, torch.zeros((N + 1, d), device="cuda"), one, drop_seed=SEED, drop_p=p)
        gate_exact(tally, "nv_embed_finish_fwd", x.reshape(B * (N + 1), d), mask, f"constants p {p}")
        x, st = ops.embed_finish_fwd(t.cuda(), B, N, gamma.cuda(), beta.cuda(), pos.cuda(), cls.cuda(), drop_seed=SEED, drop_p=p)
        ref = torch.cat((cls.double().expand(B, 1, d), F.layer_norm(t.double(), (d,), gamma.double(), beta.double(), 1e-5).reshape(B, N, d)), dim=1) + pos.double()
        assert torch.equal(x.cpu().reshape(-1, d) != 0, mask != 0)
        close32(x, ref * mask.double().reshape(B, N + 1, d), "embed_finish_fwd")
        # backward: g = ones, gamma = 1
        g = torch.ones((B, N + 1, d), device="cuda")
        dt, dt16, dg, db, dbias, dpos, dcls = ops.embed_finish_bwd(g, t.cuda(), st, one, B, N, drop_seed=SEED, drop_p=p)
        gate_exact(tally, "nv_embed_finish_bwd", g.reshape(B * (N + 1), d), mask, f"gradient of ones p {p}")
        td = t.double().requires_grad_(True)
        gd, bd = torch.ones(d, dtype=torch.float64, requires_grad=True), torch.zeros(d, dtype=torch.float64, requires_grad=True)
        pd, cd = pos.double().requires_grad_(True), cls.double().requires_grad_(True)
        r = torch.cat((cd.expand(B, 1, d), F.layer_norm(td, (d,), gd, bd, 1e-5).reshape(B, N, d)), dim=1) + pd
        r.backward(mask.double().reshape(B, N + 1, d))
        for name, got, want in (("dt", dt, td.grad), ("dgamma", dg, gd.grad), ("dbeta", db, bd.grad), ("dbias", dbias, td.grad.sum(0)), ("dpos", dpos, pd.grad),
                                ("dcls", dcls, cd.grad)):
            close32(got, want, f"embed_finish_bwd.{name}")


def _head_inputs():
    B, n, d, C = 3, 9, 192, 5
    x, gamma, beta = rnd(B, n, d, seed=1), 1 + 0.1 * rnd(d, seed=2), 0.1 * rnd(d, seed=3)
    Wt, bias = rnd(C, d, seed=4) * d ** -0.5, 0.1 * rnd(C, seed=5)
    return B, n, d, C, x, gamma, beta, Wt, bias


def _head_grad(row, gamma, beta, Wt, bias, dl=None, labels=None):
    """fp64 gradient of the head w.r.t. the row it normalises: from a given d(loss)/d(logits), or from the mean cross entropy"""
    rd = row.double().requires_grad_(True)
    logits = F.linear(F.layer_norm(rd, (row.shape[-1],), gamma.double(), beta.double(), 1e-5), Wt.double(), bias.double())
    if dl is None:
        F.cross_entropy(logits, labels).backward()
    else:
        logits.backward(dl.double())
    return rd.grad


@pytest.mark.parametrize("pool_mean", [0, 1])
def test_head_bwd_masks_its_16_bit_gradient_with_the_oracle_mask(ops, tally, pool_mean):
    """nv_head_bwd: g (fp32) is the unmasked gradient - on the cls rows, or dx / n on every token row under pool = 'mean' - and
    g16 = r16(g f) with f of element (b n + t) d + c of the [B, n, d] residual stream, bit for bit; the column sums are those of g f."""
    from neurovit_amd._cabi import check, lib
    B, n, d, C, x, gamma, beta, Wt, bias = _head_inputs()
    dl = rnd(B, C, seed=6)
    pooled = x.mean(1) if pool_mean else x[:, 0]
    row_grad = _head_grad(pooled, gamma, beta, Wt, bias, dl=dl)
    want = torch.zeros((B, n, d), dtype=torch.float64)
    if pool_mean:
        want[:] = (row_grad / n)[:, None, :]
    else:
        want[:, 0] = row_grad
    xin = pooled.reshape(B, 1, d).contiguous().cuda() if pool_mean else x.cuda()
    _, xh, st = ops.head_fwd(xin, gamma.cuda(), beta.cuda(), Wt.cuda(), bias.cuda())
    family = f"nv_head_bwd, pool = {'mean' if pool_mean else 'cls'}"
    for p in PS:
        mask = ref_cpu.drop_mask(SEED, p, (B, n, d))
        if not pool_mean:
            g, g16, _, _, _, _, dcol = ops.head_bwd(dl.cuda(), Wt.cuda(), xin, st, xh, gamma.cuda(), drop_seed=SEED, drop_p=p)
        else:
            g = torch.full((B, n, d), float("nan"), device="cuda"); g16 = torch.full((B, n, d), float("nan"), dtype=torch.bfloat16, device="cuda")
            dgm, dbt, dcol = (torch.empty(d, device="cuda") for _ in range(3))
            dW, dbs = torch.empty((C, d), device="cuda"), torch.empty(C, device="cuda")
            nb = lib.nv_head_bwd_workspace_bytes(B, d)
            ws = torch.empty(nb, dtype=torch.uint8, device="cuda")
            gm, Wd, dld = gamma.cuda(), Wt.cuda(), dl.cuda()
            check(lib.nv_head_bwd(dld.data_ptr(), B, C, Wd.data_ptr(), xin.data_ptr(), d, st.data_ptr(), xh.data_ptr(), gm.data_ptr(), d, n, g.data_ptr(), d,
                                  g16.data_ptr(), d, dgm.data_ptr(), dbt.data_ptr(), dW.data_ptr(), dbs.data_ptr(), dcol.data_ptr(), 0, ws.data_ptr(), nb, SEED, p, 1,
                                  torch.cuda.current_stream().cuda_stream), "nv_head_bwd")
        close32(g, want, "head_bwd.g")
        gc = g.cpu()
        live = slice(None) if pool_mean else slice(0, 1)
        assert bool((gc[:, live] != 0).all())
        gate_exact(tally, family, g16[:, live].float(), (gc * mask)[:, live].to(torch.bfloat16).float(), f"g16 p {p}")
        assert torch.equal(g16.cpu()[:, live] != 0, mask[:, live] != 0)
        if not pool_mean:
            assert not gc[:, 1:].any() and not g16[:, 1:].any()
        close32(dcol, (want * mask.double()).sum((0, 1)), "head_bwd.colsum")


def test_head_step_masks_its_16_bit_gradient_with_the_oracle_mask(ops, tally):
    """nv_head_step (forward + CrossEntropyLoss + backward, pool = 'cls'): as nv_head_bwd, against the fp64 gradient of the mean cross entropy."""
    B, n, d, C, x, gamma, beta, Wt, bias = _head_inputs()
    labels = torch.tensor([i % C for i in range(B)])
    want = torch.zeros((B, n, d), dtype=torch.float64)
    want[:, 0] = _head_grad(x[:, 0], gamma, beta, Wt, bias, labels=labels)
    for p in PS:
        mask = ref_cpu.drop_mask(SEED, p, (B, n, d))
        outs = ops.head_step(x.cuda(), gamma.cuda(), beta.cuda(), Wt.cuda(), bias.cuda(), labels.cuda(), drop_seed=SEED, drop_p=p)
        g, g16, dcol = outs[5], outs[6], outs[11]
        close32(g, want, "head_step.g")
        gc = g.cpu()
        assert bool((gc[:, 0] != 0).all()) and not gc[:, 1:].any() and not g16[:, 1:].any()
        gate_exact(tally, "nv_head_step", g16[:, 0].float(), (gc * mask)[:, 0].to(torch.bfloat16).float(), f"g16 p {p}")
        assert torch.equal(g16.cpu()[:, 0] != 0, mask[:, 0] != 0)
        close32(dcol, (want * mask.double()).sum((0, 1)), "head_step.colsum")
