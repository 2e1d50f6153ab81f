"""The 16-bit kernels against float64 on the value ranges of a trained model (tests/hard_values.py: inputs, references, units and every K;
tests/test_hard_values_cpu.py proves them).  Every gate is per element: |kernel - float64| <= K x unit, the unit a first-order rounding bound
from the reference's own intermediates, K twice what a faithful fp32 / 16-bit restatement of the kernel needs.  Each test reports its largest
ratio (in units) through conftest.report."""
import math

import pytest
import torch

import hard_values as hv
from conftest import report

pytestmark = pytest.mark.gpu
FMTS = ("bf16", "fp16")


@pytest.fixture(scope="module")
def ops():
    from neurovit_amd import ops as _ops
    from neurovit_amd._cabi import require_gpu
    require_gpu()
    return _ops


@pytest.fixture
def operands():
    """operands("fp16") switches the 16-bit operand format (as tests/test_fp16_gpu.py does) until the test ends"""
    from neurovit_amd import _cabi

    def use(fmt):
        _cabi.set_operand_format(fmt)
        return hv.FMT[fmt]["dtype"]
    yield use
    _cabi.set_operand_format("bf16")


def dev(t):
    return t.cuda()


def gate(what, r, k):
    """r: per-element ratios (units); reports the largest and holds it to K"""
    worst = float(r.max())
    report(f"hard values, {what}: {worst:.2f} units (K = {k})")
    assert worst <= k, f"{what}: {worst:.2f} units > K = {k} at element {int(r.argmax())} of {tuple(r.shape)}"
    return worst


# ------------------------------------------------------------------------------------------ A. GELU and its derivative
# nv_gemm_set_tile families of the existing tests; None: the dispatcher's own choice (K = 8: the small-tile kernel).  The forced families need whole 64-deep
# K tiles - with K = 8 the dispatcher would quietly fall back to the small-tile kernel - so they run K = 64.
GELU_SITES = [None, (1, 0), (3, 0), (4, 0), (9, 0), (11, 1), "skinny", "lnfold"]


def _set_tile(lib, tile):
    if tile == (11, 1):
        assert lib.nv_gemm_set_tile(4, 0) == 0
    assert lib.nv_gemm_set_tile(*tile) == 0


def _reset_tile(lib):
    lib.nv_gemm_set_tile(11, 0)
    lib.nv_gemm_set_tile(0, 0)


@pytest.mark.parametrize("site", GELU_SITES, ids=str)
@pytest.mark.parametrize("fmt", FMTS)
def test_gelu_epilogue_on_every_16_bit_code(ops, operands, fmt, site):
    """The pre-activation is driven through the bias (A = 0), so u[m, n] = bias[n] without a rounding: every finite bf16 and fp16 code, the bf16 midpoints in
    [-16, 16], NaN and both infinities.  Every row agrees bit for bit, the stored pre-activation is the rounded value, NaN / +inf survive, -inf is what
    torch's fp32 GELU makes of it, and every finite value is within K["gelu"] units of float64."""
    from neurovit_amd._cabi import lib
    dt = operands(fmt)
    vals = hv.gelu_values()
    N = vals.numel()
    bias = dev(vals)
    u = None
    if site == "skinny":
        R, K = 5, 8
        h = torch.empty((R, N), dtype=dt, device="cuda")
        u = torch.empty((R, N), dtype=dt, device="cuda")
        ops.skinny_nt(1, torch.zeros((R, K), dtype=dt, device="cuda"), torch.ones((N, K), dtype=dt, device="cuda"), bias, h, u_out=u)
    elif site == "lnfold":
        M, K = 64, 64
        assert lib.nv_gemm_lnfold_supported(M, N, K)
        stats = torch.tensor([0.0, float(K)], device="cuda").repeat(M)                  # one tile of (sum, sum of squares) per row: mean 0, variance 1; eps = 0: rstd = 1
        h = ops.gemm_lnfold(torch.zeros((M, K), dtype=dt, device="cuda"), torch.ones((N, K), dtype=dt, device="cuda"), stats, torch.zeros(N, device="cuda"), bias,
                            gelu=True, eps=0.0)
    else:
        M, K = 16, (8 if site is None else 64)
        A, B = torch.zeros((M, K), dtype=dt, device="cuda"), torch.ones((N, K), dtype=dt, device="cuda")
        u = torch.empty((M, N), dtype=dt, device="cuda")
        try:
            if site is not None:
                _set_tile(lib, site)
            h = ops.gemm(ops.NT, ops.EPI_BIAS_GELU, A, B, bias=bias, aux_out=u)
        finally:
            _reset_tile(lib)
    torch.cuda.synchronize()
    h, u = h.cpu(), None if u is None else u.cpu()
    assert h.dtype == dt
    for m in range(1, h.shape[0]):
        assert hv.same_values(h[m], h[0]), f"row {m} differs from row 0"
    if u is not None:
        assert hv.same_values(u, hv.to16(vals, fmt).expand_as(u)), "stored pre-activation is not the rounded value"
    h0 = h[0].float()
    nan, pinf, ninf = (vals != vals), vals == float("inf"), vals == float("-inf")
    assert bool(torch.isnan(h0[nan]).all()) and bool((h0[pinf] == float("inf")).all())
    assert hv.same_values(h0[ninf], torch.nn.functional.gelu(torch.tensor([float("-inf")])).expand(int(ninf.sum())))
    fin = torch.isfinite(vals)
    gate(f"GELU epilogue {fmt} site {site}", hv.gelu_ratio(h0[fin], vals[fin], fmt), hv.K["gelu"])


@pytest.mark.parametrize("site", ["gemm", "colsum", "skinny"])
@pytest.mark.parametrize("fmt", FMTS)
def test_gelu_derivative_on_every_16_bit_code(ops, operands, fmt, site):
    """EPI_DGELU with A B = 1 exactly (one unit entry per row of A against rows of ones): the output is gelu'(u) on every finite code of the format"""
    from neurovit_amd._cabi import lib
    dt = operands(fmt)
    uv = hv.dgelu_values(fmt)
    u = dev(uv.to(dt))
    K = 64 if site == "colsum" else 8
    A = torch.zeros((256, K), dtype=dt)
    A[torch.arange(256), torch.arange(256) % K] = 1.0
    A, B = dev(A), torch.ones((K, 256), dtype=dt, device="cuda")
    if site == "gemm":
        out = ops.gemm(ops.NN, ops.EPI_DGELU, A, B, aux_in=u)
    elif site == "colsum":
        try:
            assert lib.nv_gemm_set_tile(9, 0) == 0
            out, part = ops.gemm_dgelu_colsum(A, B, u)
        finally:
            _reset_tile(lib)
        colsum = out.double().sum(0).cpu()
        assert float(((part.double().sum(0).cpu() - colsum).abs() / (hv.U24 * out.double().abs().sum(0).cpu())).max()) <= 4.0       # 256 stored values per column, summed in fp32
    else:
        out = torch.empty((256, 256), dtype=dt, device="cuda")
        ops.skinny_nn(0, A, B, out, u=u)
    gate(f"GELU derivative {fmt} site {site}", hv.gelu_ratio(out.float().cpu(), uv, fmt, grad=True), hv.K[f"dgelu.{fmt}"])


# ------------------------------------------------------------------------------------------ B. attention
def _attention(ops, qkv, do, n, fmt, dh, mode):
    from neurovit_amd._cabi import lib
    dt = hv.FMT[fmt]["dtype"]
    q16, do16 = dev(qkv.to(dt)), dev(do.to(dt))
    try:
        lib.nv_attn_set_mode(mode)
        out, lse = ops.attn_fwd(q16, hv.ATTN_B, n, hv.ATTN_HEADS, dh)
        dqkv, delta = ops.attn_bwd(q16, out, do16, lse, hv.ATTN_B, n, hv.ATTN_HEADS, dh)
    finally:
        lib.nv_attn_set_mode(0)
    return out, lse, dqkv, delta


def _attention_gates(what, res, ref, n, fmt, dh):
    out, lse, dqkv, _ = res
    inner = hv.ATTN_HEADS * dh
    assert bool(torch.isfinite(out.float()).all()) and bool(torch.isfinite(dqkv.float()).all())
    gate(f"{what} out", hv.ratio(out.float(), ref["out"], ref["u_out"]), hv.K["attn.out"])
    d = (lse.reshape(ref["lse"].shape).cpu().double() - ref["lse"]).abs()
    assert bool((d <= 1e-4 * ref["lse"].abs().clamp_min(1.0)).all()), f"{what} lse: {float(d.max()):.3e}"           # the 1e-4 gate, per row
    for i, name in enumerate(("dq", "dk", "dv")):
        gate(f"{what} {name}", hv.ratio(dqkv[:, i * inner:(i + 1) * inner].float(), ref[name], ref["u_" + name]), hv.K["attn." + name])


@pytest.mark.parametrize("n", hv.ATTN_SHAPES)
@pytest.mark.parametrize("family", hv.ATTN_FAMILIES)
def test_attention_on_structured_scores(ops, operands, family, n):
    """Streaming kernels (nv_attn_set_mode(1)) forward and backward against the per-element bounds; the LDS-resident forms (2, 22, 102) bit-equal to them on these
    inputs too; fp16 operands through the streaming kernels."""
    operands("bf16")
    qkv, do = hv.attn_qkv(family, n, "bf16"), hv.attn_dout(n, "bf16")
    res = _attention(ops, qkv, do, n, "bf16", 64, 1)
    _attention_gates(f"attention {family} n={n} bf16 streaming", res, hv.attn64(qkv, do, n, "bf16"), n, "bf16", 64)
    for mode in (2, 22, 102):
        other = _attention(ops, qkv, do, n, "bf16", 64, mode)
        for a, b, name in zip(res, other, ("out", "lse", "dqkv", "delta")):
            assert torch.equal(a, b), (mode, name)
    operands("fp16")
    qkv, do = hv.attn_qkv(family, n, "fp16"), hv.attn_dout(n, "fp16")
    _attention_gates(f"attention {family} n={n} fp16 streaming", _attention(ops, qkv, do, n, "fp16", 64, 1), hv.attn64(qkv, do, n, "fp16"), n, "fp16", 64)


@pytest.mark.parametrize("family", hv.ATTN_FAMILIES)
def test_attention_wide_kernels_on_structured_scores(ops, operands, family):
    """The wide kernels (mode 3) at n = 129: the forward inside the one-ulp allowance documented by test_attention_wide_forward_equals_streaming, the backward
    bit-equal to streaming"""
    from neurovit_amd._cabi import lib
    operands("bf16")
    n = 129
    qkv, do = hv.attn_qkv(family, n, "bf16"), hv.attn_dout(n, "bf16")
    out1, lse1, d1, delta1 = _attention(ops, qkv, do, n, "bf16", 64, 1)
    _attention_gates(f"attention {family} n={n} bf16 streaming", (out1, lse1, d1, delta1), hv.attn64(qkv, do, n, "bf16"), n, "bf16", 64)
    q16, do16 = dev(qkv.bfloat16()), dev(do.bfloat16())
    try:
        lib.nv_attn_set_mode(3)
        out3, lse3 = ops.attn_fwd(q16, hv.ATTN_B, n, hv.ATTN_HEADS)
        d3, delta3 = ops.attn_bwd(q16, out1, do16, lse1, hv.ATTN_B, n, hv.ATTN_HEADS)
    finally:
        lib.nv_attn_set_mode(0)
    assert bool(((lse1 - lse3).abs().cpu().double() <= hv.ulp32(lse1.cpu())).all())
    diff = (out1.float() - out3.float()).abs()
    assert (diff > 0).float().mean().item() <= 2e-5 and bool((diff <= out1.float().abs() * 2 ** -7 + 1e-30).all())
    assert torch.equal(d1, d3) and torch.equal(delta1, delta3)


@pytest.mark.parametrize("n,dh", [(65, 32), (130, 128)])
@pytest.mark.parametrize("family", hv.ATTN_FAMILIES)
def test_attention_generic_kernels_on_structured_scores(ops, operands, family, n, dh):
    operands("bf16")
    qkv, do = hv.attn_qkv(family, n, "bf16", dh), hv.attn_dout(n, "bf16", dh)
    _attention_gates(f"attention {family} n={n} dim_head {dh}", _attention(ops, qkv, do, n, "bf16", dh, 0), hv.attn64(qkv, do, n, "bf16", dh), n, "bf16", dh)


@pytest.mark.parametrize("n", hv.ATTN_SHAPES)
@pytest.mark.parametrize("family", hv.ATTN_FAMILIES)
def test_attention_f32_on_structured_scores_per_row(ops, family, n):
    """attn_fwd_f32 at its existing tolerance (tests/test_precise_gpu.py KERNEL_TOL = 1e-5 of the maximum), taken per row and head.  The `cancel` rows are what
    the kernel's float64 accumulation of P V is for: as an fp32 chain it sat at 8.3e-6 / 1.33e-5 / 1.95e-5 there (n = 65 / 130 / 200), now 3.4e-6 ... 4.2e-6."""
    qkv = hv.attn_qkv(family, n, "bf16")
    out = ops.attn_fwd_f32(dev(qkv), hv.ATTN_B, n, hv.ATTN_HEADS, 64).cpu().double()
    ref = hv.attn64(qkv, hv.attn_dout(n, "bf16"), n, "bf16")["out"]
    rows = lambda t: t.reshape(hv.ATTN_B * n, hv.ATTN_HEADS, 64)
    e = (rows(out) - rows(ref)).abs().amax(-1) / rows(ref).abs().amax(-1)
    report(f"hard values, attn_f32 {family} n={n}: per-row rel {float(e.max()):.2e}")
    assert float(e.max()) < 1e-5


# ------------------------------------------------------------------------------------------ C. LayerNorm family
M_ROWS = 13          # ln_bwd_kernel at d <= 1024: 2 workgroups x 4 waves x 2 rows - rows 8 .. 12 are the second slot, 13 .. 15 its ragged end; at 2048 the waves loop


def _ln_out_gates(what, y16, y32, st, ref, fmt):
    gate(f"{what} mean", hv.ratio(st[0], ref["mean"], ref["u_mean"]), hv.K["ln.mean"])
    gate(f"{what} rstd", hv.ratio(st[1], ref["rstd"], ref["u_rstd"]), hv.K["ln.rstd"])
    if y32 is not None:
        gate(f"{what} f32 out", hv.ratio(y32, ref["y"], ref["u_y"]), hv.K["ln.out"])
    if y16 is not None:
        gate(f"{what} {fmt} out", hv.ratio(y16.float(), ref["y"], ref["u_y"], fmt), hv.K["ln.out"])


@pytest.mark.parametrize("d", [192, 768, 2048])
@pytest.mark.parametrize("family", hv.ROW_FAMILIES)
@pytest.mark.parametrize("fmt", FMTS)
def test_layernorm_rows_with_offsets_and_outliers(ops, operands, fmt, family, d):
    operands(fmt)
    x, dy = hv.ln_rows(family, M_ROWS, d), hv.ln_rows("benign", M_ROWS, d, seed=9)
    gamma, beta = hv.ln_params(d)
    ref = hv.ln64(x, gamma, beta, dy=dy)
    y, st = ops.ln_fwd(dev(x), dev(gamma), dev(beta))
    y32 = ops.ln_fwd_f32(dev(x), dev(gamma), dev(beta))
    what = f"LayerNorm {family} d={d}"
    _ln_out_gates(what, y, y32, st, ref, fmt)
    if family == "constant":
        assert torch.equal(y32.cpu(), beta.expand(M_ROWS, d)) and torch.equal(y.cpu(), beta.to(y.dtype).expand(M_ROWS, d))      # exactly beta
    dx, g16, dg, db, dc = ops.ln_bwd(dev(dy), dev(x), st, dev(gamma))
    assert all(bool(torch.isfinite(t.float()).all()) for t in (dx, g16, dg, db, dc))
    gate(f"{what} dx", hv.ratio(dx, ref["dx"], ref["u_dx"]), hv.K["ln.dx"])
    gate(f"{what} {fmt} dx", hv.ratio(g16.float(), ref["dx"], ref["u_dx"], fmt), hv.K["ln.dx"])
    gate(f"{what} dgamma", hv.ratio(dg, ref["dgamma"], ref["u_dgamma"]), hv.K["ln.dgamma"])
    gate(f"{what} dbeta", hv.ratio(db, ref["dbeta"], ref["u_dbeta"]), hv.K["ln.dbeta"])
    gate(f"{what} column sums", hv.ratio(dc, ref["colsum"], ref["u_colsum"]), hv.K["ln.colsum"])


@pytest.mark.parametrize("family", hv.ROW_FAMILIES)
def test_embedding_and_head_layernorm_on_hard_rows(ops, operands, family):
    """embed_finish_fwd / _bwd (pos = 0: the token rows are the LayerNorm output itself) and head_fwd / head_bwd (one class, dlogits = 1: dy is the weight row) on the
    same rows, at the LayerNorm family's K"""
    operands("bf16")
    B, N, d = 2, 7, 192
    t = hv.ln_rows(family, B * N, d)
    gamma, beta = hv.ln_params(d)
    g = hv.ln_rows("benign", B * (N + 1), d, seed=9).reshape(B, N + 1, d)
    ref = hv.ln64(t, gamma, beta, dy=g[:, 1:].reshape(B * N, d))
    x, st = ops.embed_finish_fwd(dev(t), B, N, dev(gamma), dev(beta), dev(torch.zeros(N + 1, d)), dev(torch.zeros(d)))
    what = f"embed_finish {family}"
    _ln_out_gates(what, None, x[:, 1:].reshape(B * N, d), st, ref, None)
    dt, dt16, dg, db, dbias, dpos, dcls = ops.embed_finish_bwd(dev(g.clone()), dev(t), st, dev(gamma), B, N)
    gate(f"{what} dt", hv.ratio(dt, ref["dx"], ref["u_dx"]), hv.K["ln.dx"])
    gate(f"{what} bf16 dt", hv.ratio(dt16.float(), ref["dx"], ref["u_dx"], "bf16"), hv.K["ln.dx"])
    gate(f"{what} dgamma", hv.ratio(dg, ref["dgamma"], ref["u_dgamma"]), hv.K["ln.dgamma"])
    gate(f"{what} dbeta", hv.ratio(db, ref["dbeta"], ref["u_dbeta"]), hv.K["ln.dbeta"])
    gate(f"{what} dbias", hv.ratio(dbias, ref["colsum"], ref["u_colsum"]), hv.K["ln.colsum"])
    # the head: the cls rows of [B, n, d] are the hard rows
    Bh, n = 5, 3
    xs = torch.zeros(Bh, n, d)
    xs[:, 0] = hv.ln_rows(family, Bh, d, seed=3)
    W = hv.ln_rows("benign", 1, d, seed=4)
    href = hv.ln64(xs[:, 0], gamma, beta, dy=W.expand(Bh, d))
    logits, xh, hst = ops.head_fwd(dev(xs), dev(gamma), dev(beta), dev(W), dev(torch.zeros(1)))
    what = f"head {family}"
    _ln_out_gates(what, None, xh, hst.t(), href, None)
    gh = ops.head_bwd(dev(torch.ones(Bh, 1)), dev(W), dev(xs), hst, xh, dev(gamma))[0]
    assert bool(torch.isfinite(gh).all())
    gate(f"{what} dx", hv.ratio(gh[:, 0], href["dx"], href["u_dx"]), hv.K["ln.dx"])


@pytest.mark.parametrize("p,S,mode", [(8, 16, 0), (9, 18, 0), (8, 16, 2)], ids=["vector", "scalar", "slabs"])
@pytest.mark.parametrize("fmt", FMTS)
def test_patch_layernorm_on_brain_edge_volumes(ops, operands, fmt, p, S, mode):
    """patch_ln_fwd / patch_ln_fwd_f32 through the vector path (p = 8), the scalar path (p = 9) and the LDS-staged slabs (nv_patch_set_mode(2)) on volumes whose
    patches start in the background, sit on an offset, or are tiny / huge"""
    from neurovit_amd._cabi import lib
    from oracle import ref_cpu
    operands(fmt)
    vols = hv.volumes(S)
    P = p ** 3
    gamma, beta = hv.ln_params(P)
    ref = hv.ln64(hv.tokens_of(vols, p), gamma, beta)
    video = ref_cpu.fmri_to_video(dev(vols))
    try:
        lib.nv_patch_set_mode(mode)
        y, st = ops.patch_ln_fwd(video, p, p, p, dev(gamma), dev(beta))
        y32, st32 = ops.patch_ln_fwd_f32(video, p, p, p, dev(gamma), dev(beta))
    finally:
        lib.nv_patch_set_mode(0)
    assert torch.equal(st, st32) and torch.count_nonzero(y[:, P:]) == 0
    _ln_out_gates(f"patch LayerNorm p={p} mode {mode}", y[:, :P], y32, st, ref, fmt)


@pytest.mark.parametrize("sigma", [False, True], ids=["", "vol_sigma"])
@pytest.mark.parametrize("S,p,T", hv.SERIES_SHAPES)
def test_patch_4d_statistics_on_the_pivot_cases(ops, operands, S, p, T, sigma):
    """patch_ln_fwd_4d and its f32 form where voxel 0 of every patch is a background voxel in front of tissue (raw and z-scored) or an outlier: mean and rstd at
    the K of the per-volume gather, the tokens at the output unit.  (The kernel used to shift its one-pass sums by voxel 0 and lost 3e-4 of rstd here.)"""
    from neurovit_amd._cabi import check, lib
    operands("bf16")
    x = hv.series(S, p, T)
    P, N = p ** 3, (S // p) ** 3
    gamma, beta = hv.ln_params(P)
    sg = hv.SERIES_SIGMA if sigma else None
    ref = hv.ln64(hv.series_tokens(x, p), gamma, beta, eps=hv.series_eps(sg, T, N)[0])
    vs = None if sg is None else dev(sg)
    xd, gd, bd = dev(x), dev(gamma), dev(beta)
    tok, st = ops.patch_ln_fwd_4d(xd, p, p, p, gd, bd, vol_sigma=vs)
    tok32 = torch.empty((3 * T * N, P), device="cuda")
    st32 = torch.empty((2, 3 * T * N), device="cuda")
    check(lib.nv_patch_ln_fwd_4d_f32(xd.data_ptr(), 3, S, S, S, T, p, p, p, gd.data_ptr(), bd.data_ptr(), 1e-5, tok32.data_ptr(), P, st32[0].data_ptr(),
                                     st32[1].data_ptr(), None if vs is None else vs.data_ptr(), torch.cuda.current_stream().cuda_stream), "nv_patch_ln_fwd_4d_f32")
    torch.cuda.synchronize()
    assert torch.equal(st, st32)
    what = f"4D patch LayerNorm S={S} T={T}{' vol_sigma' if sigma else ''}"
    gate(f"{what} mean", hv.ratio(st[0], ref["mean"], ref["u_mean"]), hv.K["series.mean"])
    gate(f"{what} rstd", hv.ratio(st[1], ref["rstd"], ref["u_rstd"]), hv.K["series.rstd"])
    gate(f"{what} f32 tokens", hv.ratio(tok32, ref["y"], ref["u_y"]), hv.K["ln.out"])
    gate(f"{what} bf16 tokens", hv.ratio(tok.float(), ref["y"], ref["u_y"], "bf16"), hv.K["ln.out"])


# ------------------------------------------------------------------------------------------ D. AdamW
def _adam_step(ops, path, fmt, state, g, step, wd, gs, blocks):
    p, m, v, p16 = state
    n = p.numel()
    if path == "ranges":
        cut = (n // 2) // 4 * 4
        opt = ops.adamw_arena(p, g, m, v, p16, step=step, lr=hv.ADAM["lr"], betas=hv.ADAM["betas"], eps=hv.ADAM["eps"], weight_decay=wd, grad_scale=gs)
        ops.adamw_ranges(opt, [(0, cut), (cut, n - cut)] if cut else [(0, n)])
        return
    scale_state = None
    if path == "scale_state":                      # the constants of this step, as nv_loss_scale_update leaves them in the device block (csrc/common.h LS_*)
        b1, b2 = hv.ADAM["betas"]
        blk = torch.zeros(16)
        blk[1], blk[6], blk[7] = 1.0, hv.ADAM["lr"] / (1.0 - b1 ** step), math.sqrt(1.0 - b2 ** step)
        scale_state, step = dev(blk), 1
    ops.adamw_step(p, g, m, v, p16, step, hv.ADAM["lr"], betas=hv.ADAM["betas"], eps=hv.ADAM["eps"], weight_decay=wd, grad_scale=gs, max_blocks=blocks,
                   scale_state=scale_state)


@pytest.mark.parametrize("path", ["step", "ranges", "scale_state"])
def test_adamw_at_the_level_of_the_update(ops, operands, path):
    """Three consecutive steps from step 1, 1000 and 100000, every count (a capped grid at the largest), weight decay 0 / 1e-2, gradient scale 1 / 2^-16: after each
    step |p - float64| <= 2 ulp + K 2^-24 |update|, m and v relative at K 2^-24, the 16-bit shadow the rounded p.  The float64 step starts from the state the
    kernel itself left, so the bound is that of ONE step."""
    operands("bf16")
    worst = [0.0, 0.0, 0.0]
    for n in hv.ADAM_COUNTS:
        for start in hv.ADAM_STARTS:
            p0, grads, m0, v0 = hv.adam_inputs(n, start)
            for wd in hv.ADAM_DECAYS:
                for gs in hv.ADAM_SCALES:
                    for blocks in ((0, 3) if (n == hv.ADAM_COUNTS[-1] and path == "step") else (0,)):
                        state = (dev(p0.clone()), dev(m0.clone()), dev(v0.clone()), torch.empty(n, dtype=torch.bfloat16, device="cuda"))
                        for s, g in enumerate(grads):
                            before = [t.cpu() for t in state[:3]]
                            ref = hv.adam64(before[0], g, before[1], before[2], start + s, wd, gs)
                            _adam_step(ops, path, "bf16", state, dev(g), start + s, wd, gs, blocks)
                            worst = [max(a, b) for a, b in zip(worst, hv.adam_ratios(state[0], state[1], state[2], ref))]
                            assert torch.equal(state[3].cpu(), state[0].cpu().bfloat16())
    for name, w in zip(("adam.p", "adam.m", "adam.v"), worst):
        report(f"hard values, AdamW {path} {name}: {w:.2f} units (K = {hv.K[name]})")
        assert w <= hv.K[name], (path, name, w)
