"""Every fp8 (OCP e4m3) kernel and GEMM epilogue against the e4m3 reference of tests/fp8_ref.py, on a real MI355X.

  GEMM            nv_gemm_f8 epilogues 0, 1, 4, 7, nv_gemm_f8_gelu_train (with and without u16) and nv_gemm_f8_resid_drop in BOTH tile families -
                  256 x 128 ping-pong (launch_pp_f8) and 256 x 256 (launch_pq_f8, the two-pass epilogue), each forced - against the fp64 product
                  of the dequantised bytes the device holds; the training entry points against the inference ones byte for byte; family
                  against family; run against run.
  dropout         the two training epilogues' masks read back cell by cell against ref_cpu.drop_mask (A8 = 0, bias = 1, residual = 0).
  leading dims    every operand and output as a column slice of a wider buffer filled with a sentinel: same bits inside, sentinel outside.
  row kernels     nv_ln_fwd_f8 / nv_ln_fwd_f8_train (against nv_ln_fwd bit for bit) and nv_quant_rows_f8 at ragged shapes.
  format edges    saturation (0x7E / 0xFE exactly, never a NaN code for finite input), subnormals, NaN propagation.

Gates: fp32 outputs 1e-4 of max |reference| (the K = 128 MFMA keeps fewer guard bits than an fma chain: tests/test_kernels_gpu.py), bf16 outputs
assert_close_bf16, e4m3 outputs fp8_ref.check_e4m3 - reference code or a neighbour, a capped share differing (tests/test_fp8_ref_cpu.py shows the
reference itself stays below half of each cap), NaN and saturated cells exact.  Two tile families run the same MFMA over the same K order,
but nothing here relies on it: across families fp32 outputs agree to the same 1e-4, rounded outputs to that plus one step of their format.
One report line per family: cells compared with a reference or a twin - every gate below counts, the comparison of the two families
under a name of its own - and the cells that differed (e4m3: from the reference code; bit comparisons: at all; fp32 / bf16: beyond the gate)."""
import contextlib

import pytest
import torch

import fp8_ref as R
from conftest import rel_err, report
from ld_windows import SENTINEL, guards_intact, into_padded, padded         # noqa: F401  (shared with tests/test_ld_windows_gpu.py)
from oracle import ref_cpu
from test_dropout_masks_cpu import PS, SEED, check_readout, drop_scale, want_gelu

pytestmark = pytest.mark.gpu

FAMILIES = {"256 x 128": (0, 0), "256 x 256": (9, 0)}      # nv_gemm_set_tile: at these sizes the heuristic is the ping-pong family


@pytest.fixture(scope="module")
def ops():
    from neurovit_amd import ops as _ops
    from neurovit_amd._cabi import require_gpu
    require_gpu()
    return _ops


@pytest.fixture(scope="module")
def tally():
    """{family: [cells compared, cells that differed]} - one report line each when the module is done"""
    counts = {}
    yield counts
    for family, (cells, bad) in counts.items():
        report(f"fp8 kernels, {family}: {cells} cells compared, {bad} differing")


def count(tally, family, cells, bad):
    c = tally.setdefault(family, [0, 0])
    c[0] += cells
    c[1] += bad


def same_bits(tally, family, a, b, what):
    """two device outputs bit for bit (NaN cells included: the words compare)"""
    assert a.shape == b.shape and a.dtype == b.dtype, f"{family}, {what}: shape / dtype"
    wa, wb = (t.contiguous().view(torch.uint8).reshape(t.numel(), -1) for t in (a, b))
    bad = int((wa != wb).any(1).sum())
    count(tally, family, a.numel(), bad)
    assert bad == 0, f"{family}, {what}: {bad} of {a.numel()} cells differ"


def gate8(tally, family, got, want, cap, what):
    cells, differ = R.check_e4m3(got, want, cap, f"{family}, {what}")
    print(f"{family}, {what}: {differ} of {cells} codes differ from the reference")
    count(tally, family, cells, differ)


def gate32(tally, family, got, want, what, rel=1e-4):
    """fp32 output: max |got - want| <= rel * max |want| (tests/test_kernels_gpu.py::assert_close_f32); counts the cells beyond that bound"""
    got, want = got.detach().cpu().double(), want.detach().cpu().double()
    e = rel_err(got, want)
    print(f"{family}, {what}: rel err {e:.3e}")
    count(tally, family, want.numel(), int(((got - want).abs() > rel * want.abs().max()).sum()))
    assert e <= rel, f"{family}, {what}: rel err {e:.3e} > {rel}"


def gate16(tally, family, got, want, what, rel=1e-3):
    """bf16 output: |got - want| <= rel * max |want| + one bf16 ulp of |want| (tests/test_kernels_gpu.py::assert_close_bf16); counts the cells beyond"""
    a, b = got.detach().float().cpu().double(), want.detach().float().cpu().double()
    ulp = 2.0 ** (torch.floor(torch.log2(b.abs().clamp_min(1e-30))) - 7)
    bad = (a - b).abs() > rel * b.abs().max() + ulp
    count(tally, family, b.numel(), int(bad.sum()))
    assert not bad.any(), f"{family}, {what}: {int(bad.sum())} / {bad.numel()} outside tol, max diff {(a - b).abs().max():.3e}, max ref {b.abs().max():.3e}"


@contextlib.contextmanager
def forced(family):
    from neurovit_amd._cabi import lib
    assert lib.nv_gemm_set_tile(*FAMILIES[family]) == 0
    try:
        yield
    finally:
        lib.nv_gemm_set_tile(0, 0)


# ------------------------------------------------------------------------------------------------------------ GEMM: both families, every epilogue
@pytest.fixture(scope="module")
def gemm_case(ops):
    """(M, N, K) -> device operands (w8 / colscale from nv_quant_rows_f8, a8 from the CPU conversion) and the fp64 reference of what the device
    holds; computed once per shape, shared read only, released with the module"""
    cases = {}

    def get(M, N, K):
        if (M, N, K) not in cases:
            x, W, sa, bias, resid = R.gemm_inputs(M, N, K)
            w8, cs = ops.quant_rows_f8(W.cuda(), sa)
            a8, adq = R.e4m3(x * sa)
            acc = R.gemm_ref(adq, R.decode(w8.cpu()), cs.cpu(), torch.float64)
            cases[M, N, K] = a8.cuda(), w8, cs, bias.cuda(), resid.cuda(), acc
        return cases[M, N, K]
    yield get
    cases.clear()


def run_family(ops, A8, w8, cs, bias, resid, out_scale):
    """every fp8 GEMM entry point once: {name: output}"""
    o = {"f32": ops.gemm_f8(ops.EPI_STORE_F32, A8, w8, cs), "bf16": ops.gemm_f8(ops.EPI_STORE_BF16, A8, w8, cs),
         "resid": ops.gemm_f8(ops.EPI_BIAS_RESID, A8, w8, cs, bias=bias, aux_in=resid),
         "h8": ops.gemm_f8(ops.EPI_BIAS_GELU_F8, A8, w8, cs, bias=bias, out_scale=out_scale)}
    o["t.h8"], o["t.h16"], o["t.u16"] = ops.gemm_f8_gelu_train(A8, w8, cs, bias, out_scale)
    o["t0.h8"], o["t0.h16"], none = ops.gemm_f8_gelu_train(A8, w8, cs, bias, out_scale, u16=False)
    assert none is None
    o["resid_drop"] = ops.gemm_f8_resid_drop(A8, w8, cs, bias, resid)
    torch.cuda.synchronize()
    return o


@pytest.mark.parametrize("M,N,K", R.GEMM_SHAPES)
def test_gemm_f8_every_epilogue_in_both_families(ops, tally, gemm_case, M, N, K):
    A8, w8, cs, bias, resid, acc = gemm_case(M, N, K)
    u, h, h_scaled = R.gelu_ref(acc, bias.cpu(), R.GELU_SCALE, torch.float64)
    outs = {}
    for family in FAMILIES:
        with forced(family):
            o = outs[family] = run_family(ops, A8, w8, cs, bias, resid, R.GELU_SCALE)
            again = run_family(ops, A8, w8, cs, bias, resid, R.GELU_SCALE)
        gate32(tally, family, o["f32"], acc, "epilogue 1 (fp32 store)")
        gate16(tally, family, o["bf16"], acc, "epilogue 0 (bf16 store)")
        gate32(tally, family, o["resid"], acc + bias.cpu().double() + resid.cpu().double(), "epilogue 4 (bias + residual)")
        gate8(tally, family, o["h8"], h_scaled, R.CAP_GELU, "epilogue 7 (GELU -> e4m3)")
        gate16(tally, family, o["t.u16"], u, "training GELU u16")
        gate16(tally, family, o["t.h16"], h, "training GELU h16")
        same_bits(tally, family, o["t.h8"], o["h8"], "training GELU h8 against epilogue 7")
        same_bits(tally, family, o["t0.h8"], o["t.h8"], "training GELU without u16, h8")
        same_bits(tally, family, o["t0.h16"], o["t.h16"], "training GELU without u16, h16")
        same_bits(tally, family, o["resid_drop"], o["resid"], "residual epilogue with p = 0 against epilogue 4")
        for name in o:
            same_bits(tally, family, again[name], o[name], f"{name}, second run")
    a, b = (outs[f] for f in FAMILIES)
    across = "256 x 128 against 256 x 256"
    for name in ("f32", "resid", "resid_drop"):
        gate32(tally, across, a[name], b[name], name, 1e-4)
    for name in ("bf16", "t.u16", "t.h16", "t0.h16"):
        gate16(tally, across, a[name], b[name], name, 1e-4)
    for name in ("h8", "t.h8", "t0.h8"):
        av, bv = R.decode(a[name].cpu()).double(), R.decode(b[name].cpu()).double()
        far = (av - bv).abs() > R.e4m3_step(torch.minimum(av.abs(), bv.abs()))
        count(tally, across, av.numel(), int((av != bv).sum()))
        print(f"{across}, {name}: {int((av != bv).sum())} of {av.numel()} codes differ")
        assert not far.any(), f"{across}, {name}: {int(far.sum())} cells more than one code apart"


# ------------------------------------------------------------------------------------------------------------ dropout masks of the training epilogues
@pytest.mark.parametrize("M,N", [(257, 264), (300, 8)])
@pytest.mark.parametrize("family", list(FAMILIES))
def test_training_epilogues_apply_the_oracle_mask(ops, tally, family, M, N):
    """A8 = 0, bias = 1, residual = 0 (tests/test_dropout_masks_gpu.py's read-out): FC2's epilogue returns the factor of element m N + n itself;
    FC1's returns gelu(1) f in h16 and sat(gelu(1) f out_scale) in h8 beside an unmasked u16 = 1 - and h16 is, bit for bit, what the bf16
    GEMM's bias + GELU epilogue writes for the same seed and p."""
    K, out_scale, dtype = 128, 16.0, torch.bfloat16
    A8, B8 = torch.zeros((M, K), dtype=torch.uint8, device="cuda"), torch.zeros((N, K), dtype=torch.uint8, device="cuda")
    A16, B16 = torch.zeros((M, 64), dtype=dtype, device="cuda"), torch.zeros((N, 64), dtype=dtype, device="cuda")
    cs, bias, resid = torch.ones(N, device="cuda"), torch.ones(N, device="cuda"), torch.zeros((M, N), device="cuda")
    name = f"{family}, dropout read-out"
    for p in PS:
        mask = ref_cpu.drop_mask(SEED, p, (M, N))
        twin = ops.gemm(ops.NT, ops.EPI_BIAS_GELU, A16, B16, bias=bias, drop_seed=SEED, drop_p=p)
        with forced(family):
            out = ops.gemm_f8_resid_drop(A8, B8, cs, bias, resid, drop_seed=SEED, drop_p=p)
            h8, h16, u16 = ops.gemm_f8_gelu_train(A8, B8, cs, bias, out_scale, drop_seed=SEED, drop_p=p)
        what = f"[{M}, {N}] p {p}"
        bad = int(((out.cpu() != 0) != (mask != 0)).sum())
        count(tally, name, mask.numel(), bad)
        assert torch.equal(out.cpu() != 0, mask != 0), f"{name}, bias + residual {what}: {bad} of {mask.numel()} mask cells differ from the oracle's mask"
        assert torch.equal(out.cpu(), mask), f"{name}, bias + residual {what}: kept values differ"
        assert bool((u16 == 1).all()), "the pre-activation is not masked"
        count(tally, name, mask.numel(), int(((h16.float().cpu() != 0) != (mask != 0)).sum()))
        check_readout(h16, mask, want_gelu(p, dtype), dtype, f"{name}, h16 {what}")
        z8 = R.decode(h8.cpu()) != 0
        count(tally, name, mask.numel(), int((z8 != (h16.float().cpu() != 0)).sum()))
        assert torch.equal(z8, h16.float().cpu() != 0), f"{name}, {what}: h8 and h16 carry different masks"
        kept = mask != 0
        want8 = torch.full((int(kept.sum()),), float(R.gelu(torch.tensor(1.0, dtype=torch.float64))) * drop_scale(p) * out_scale, dtype=torch.float64)
        R.check_e4m3(h8.cpu()[kept], want8, 1.0, f"{name}, kept h8 {what}")      # one value in every kept cell: within one step, no share to cap
        same_bits(tally, name, h16, twin, f"h16 against the bf16 GEMM's bias + GELU epilogue {what}")


# ------------------------------------------------------------------------------------------------------------ leading dimensions and guards
# (padded, into_padded, guards_intact: tests/ld_windows.py)
@pytest.mark.parametrize("family", list(FAMILIES))
def test_gemm_f8_honours_every_leading_dimension(ops, tally, gemm_case, family):
    """A8, B8, the residual and every output as column slices of wider buffers: same bits as the dense run inside, sentinel outside."""
    M, N, K = R.GEMM_LD_SHAPE
    A8, w8, cs, bias, resid, _ = gemm_case(M, N, K)
    Ap, Bp, Rp = into_padded(A8, 16), into_padded(w8, 32), into_padded(resid, 8)
    assert Ap.stride(0) == K + 16 and Bp.stride(0) == K + 32 and Rp.stride(0) == N + 8
    bf = torch.bfloat16
    with forced(family):
        dense = run_family(ops, A8, w8, cs, bias, resid, R.GELU_SCALE)
        got, bufs = {}, {}
        for name, dtype in (("f32", torch.float32), ("bf16", bf), ("resid", torch.float32), ("h8", torch.uint8), ("t.h8", torch.uint8), ("t.h16", bf),
                            ("t.u16", bf), ("t0.h8", torch.uint8), ("t0.h16", bf), ("resid_drop", torch.float32)):
            got[name], bufs[name] = padded(M, N, dtype)
            assert got[name].stride(0) == N + 8
        ops.gemm_f8(ops.EPI_STORE_F32, Ap, Bp, cs, out=got["f32"])
        ops.gemm_f8(ops.EPI_STORE_BF16, Ap, Bp, cs, out=got["bf16"])
        ops.gemm_f8(ops.EPI_BIAS_RESID, Ap, Bp, cs, bias=bias, aux_in=Rp, out=got["resid"])
        ops.gemm_f8(ops.EPI_BIAS_GELU_F8, Ap, Bp, cs, bias=bias, out_scale=R.GELU_SCALE, out=got["h8"])
        ops.gemm_f8_gelu_train(Ap, Bp, cs, bias, R.GELU_SCALE, h8=got["t.h8"], h16=got["t.h16"], u16=got["t.u16"])
        ops.gemm_f8_gelu_train(Ap, Bp, cs, bias, R.GELU_SCALE, h8=got["t0.h8"], h16=got["t0.h16"], u16=False)
        ops.gemm_f8_resid_drop(Ap, Bp, cs, bias, Rp, out=got["resid_drop"])
        torch.cuda.synchronize()
    for name in got:
        same_bits(tally, family, got[name], dense[name], f"{name} with padded leading dimensions")
        assert guards_intact(got[name], bufs[name]), f"{family}, {name}: wrote outside its [M, N] view"


# ------------------------------------------------------------------------------------------------------------ LayerNorm -> e4m3
def check_ln(ops, tally, x, gamma, beta, scale, y8, y16, st, what):
    """the training kernel's three outputs against nv_ln_fwd_f8 / nv_ln_fwd on the same device input, byte for byte"""
    name = "LayerNorm -> e4m3"
    same_bits(tally, name, y8, ops.ln_fwd_f8(x, gamma, beta, scale), f"{what}: y8 against nv_ln_fwd_f8")
    r16, rst = ops.ln_fwd(x, gamma, beta)
    same_bits(tally, name, y16, r16, f"{what}: y16 against nv_ln_fwd")
    same_bits(tally, name, st, rst, f"{what}: mean / rstd against nv_ln_fwd")


@pytest.mark.parametrize("M,d", R.LN_SHAPES)
def test_ln_fwd_f8_train(ops, tally, M, d):
    x, gamma, beta = R.ln_inputs(M, d)
    xd, gd, bd = x.cuda(), gamma.cuda(), beta.cuda()
    y8, y16, st = ops.ln_fwd_f8_train(xd, gd, bd, R.LN_SCALE)
    check_ln(ops, tally, xd, gd, bd, R.LN_SCALE, y8, y16, st, f"[{M}, {d}]")
    ref = R.ln_ref(x, gamma, beta, 1.0, torch.float64)
    gate8(tally, "LayerNorm -> e4m3", y8, ref * R.LN_SCALE, R.CAP_LN, f"[{M}, {d}] y8")
    gate16(tally, "LayerNorm -> e4m3", y16, ref, f"[{M}, {d}] y16")
    gate32(tally, "LayerNorm -> e4m3", st[0], x.double().mean(1), f"[{M}, {d}] mean", 1e-5)
    gate32(tally, "LayerNorm -> e4m3", st[1], 1 / torch.sqrt(x.double().var(1, unbiased=False) + 1e-5), f"[{M}, {d}] rstd", 1e-5)
    # the same rows out of / into wider buffers
    xp = into_padded(xd, 8)
    (p8, b8), (p16, b16) = padded(M, d, torch.uint8), padded(M, d, torch.bfloat16)
    assert xp.stride(0) == d + 8 and p8.stride(0) == d + 8 and p16.stride(0) == d + 8
    _, _, pst = ops.ln_fwd_f8_train(xp, gd, bd, R.LN_SCALE, y8=p8, y16=p16)
    (q8, c8) = padded(M, d, torch.uint8)
    ops.ln_fwd_f8(xp, gd, bd, R.LN_SCALE, out=q8)
    for got, want, buf, what in ((p8, y8, b8, "y8"), (p16, y16, b16, "y16"), (q8, y8, c8, "nv_ln_fwd_f8 y8")):
        same_bits(tally, "LayerNorm -> e4m3", got, want, f"[{M}, {d}] {what} with padded leading dimensions")
        assert guards_intact(got, buf), f"{what}: wrote outside its [M, d] view"
    same_bits(tally, "LayerNorm -> e4m3", pst, st, "statistics with padded leading dimensions")


def test_ln_fwd_f8_rejects_widths_it_has_no_kernel_for(ops):
    g, b = torch.ones(2052, device="cuda"), torch.zeros(2052, device="cuda")
    for x in (torch.zeros((8, 8), device="cuda")[:, :6], torch.zeros((4, 2052), device="cuda")):      # d = 6: no multiple of 4 (ldx = 8 is); d = 2052 > 2048
        with pytest.raises(RuntimeError):
            ops.ln_fwd_f8_train(x, g, b, 1.0)
        with pytest.raises(RuntimeError):
            ops.ln_fwd_f8(x, g, b, 1.0)
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------------------ row quantisation
@pytest.mark.parametrize("rows,cols", R.QUANT_SHAPES)
def test_quant_rows_f8(ops, tally, rows, cols):
    W = R.quant_inputs(rows, cols)
    w8, cs = ops.quant_rows_f8(W.cuda(), R.QUANT_ACT_SCALE)
    want, want_cs = R.quant_ref(W, torch.float64)
    gate8(tally, "row quantisation", w8, want, R.CAP_QUANT, f"[{rows}, {cols}]")
    gate32(tally, "row quantisation", cs, want_cs, f"[{rows}, {cols}] colscale", 1e-6)
    assert not w8[1].any() and cs[1].item() == (torch.tensor(1.0) / torch.tensor(R.QUANT_ACT_SCALE)).item()      # the zero row: bytes 0, row scale 1, fp32 1 / act_scale
    top = R.decode(w8.cpu())
    live = torch.ones(rows, dtype=torch.bool)
    live[1] = False
    assert bool((top.abs().amax(1)[live] == 448.0).all()) and top[2].min() == -448.0 and top[2].max() <= 0      # row 2's largest element is -448
    at = W.abs().argmax(1)
    assert bool((top[torch.arange(rows), at][live].abs() == 448.0).all())
    Wp = into_padded(W.cuda(), 8)
    p8, buf = padded(rows, cols, torch.uint8)
    _, pcs = ops.quant_rows_f8(Wp, R.QUANT_ACT_SCALE, out=p8)
    same_bits(tally, "row quantisation", p8, w8, "bytes with padded leading dimensions")
    same_bits(tally, "row quantisation", pcs, cs, "colscale with padded leading dimensions")
    assert guards_intact(p8, buf), "wrote outside its [rows, cols] view"


# ------------------------------------------------------------------------------------------------------------ the edges of the format
@pytest.mark.parametrize("kind", ["saturate", "saturate_inf", "subnormal", "nan"])
def test_ln_fwd_f8_at_the_edges_of_the_format(ops, tally, kind):
    """Saturation: cells beyond +-480 are 0x7E / 0xFE exactly and finite input never gives a NaN code; an infinity in beta saturates its column,
    one in the input makes its row NaN (inf - mean) as in the reference.  Subnormals: every cell within one 2^-9 step.  NaN: one NaN in a row
    makes that row's y8 the NaN code beside a NaN y16, and leaves every other row as it was."""
    x, gamma, beta, scale = R.ln_edge_inputs(kind)
    xd, gd, bd = x.cuda(), gamma.cuda(), beta.cuda()
    ref = R.ln_ref(x, gamma, beta, scale, torch.float64)
    name = f"format edges, {kind}"
    y8 = ops.ln_fwd_f8(xd, gd, bd, scale)
    t8, t16, _ = ops.ln_fwd_f8_train(xd, gd, bd, scale)
    same_bits(tally, name, t8, y8, "LayerNorm: training y8 against nv_ln_fwd_f8")
    gate8(tally, name, y8, ref, R.CAP_LN, "LayerNorm y8")
    codes = y8.cpu()
    if kind == "saturate":
        assert not bool(((codes & 0x7F) == 0x7F).any()), "a NaN code for finite input"
        assert (codes == 0x7E).any() and (codes == 0xFE).any()
    if kind == "nan":
        r = R.LN_NAN_CELL[0]
        assert bool(((codes[r] & 0x7F) == 0x7F).all()) and bool(torch.isnan(t16[r].float()).all())
        x0, g0, b0, _ = R.ln_edge_inputs("saturate")                       # the same rows without the NaN
        clean = ops.ln_fwd_f8(x0.cuda(), g0.cuda(), b0.cuda(), scale).cpu()
        others = torch.arange(x.shape[0]) != r
        assert torch.equal(codes[others], clean[others]), "a NaN row changed other rows"
        assert bool(torch.isfinite(t16.float().cpu()[others]).all())


@pytest.mark.parametrize("family", list(FAMILIES))
@pytest.mark.parametrize("kind", ["saturate", "saturate_inf", "subnormal", "nan"])
def test_gelu_epilogues_at_the_edges_of_the_format(ops, tally, gemm_case, kind, family):
    """Epilogue 7 and the training GELU.  Saturation: 0x7E beyond 480, no NaN code for finite input, bias = +inf gives 448 (bias = -inf gives
    gelu(-inf) = -inf * 0, a NaN, in the reference and on the device).  Subnormals: within one 2^-9 step.  NaN: one NaN in the bias makes that
    output column NaN in h8, h16 and u16 and leaves the others as they were."""
    M, N, K = R.GEMM_EDGE_SHAPE
    A8, w8, cs, bias0, _, acc = gemm_case(M, N, K)
    bias, scale = R.gemm_edge_bias(kind, bias0.cpu())
    u, h, h_scaled = R.gelu_ref(acc, bias, scale, torch.float64)
    name = f"format edges, {kind}"
    with forced(family):
        h8 = ops.gemm_f8(ops.EPI_BIAS_GELU_F8, A8, w8, cs, bias=bias.cuda(), out_scale=scale)
        t8, t16, u16 = ops.gemm_f8_gelu_train(A8, w8, cs, bias.cuda(), scale)
        clean8 = ops.gemm_f8(ops.EPI_BIAS_GELU_F8, A8, w8, cs, bias=bias0, out_scale=scale) if kind == "nan" else None
        torch.cuda.synchronize()
    same_bits(tally, name, t8, h8, f"{family}: training h8 against epilogue 7")
    gate8(tally, name, h8, h_scaled, R.CAP_GELU, f"{family}, epilogue 7")
    codes = h8.cpu()
    if kind == "saturate":
        assert not bool(((codes & 0x7F) == 0x7F).any()), "a NaN code for finite input"
        assert (codes == 0x7E).any()
    if kind == "saturate_inf":
        (cp, _), (cn, _) = R.GEMM_INF_BIAS
        assert bool((codes[:, cp] == 0x7E).all()) and bool(torch.isinf(t16[:, cp].float()).all()) and bool((u16[:, cn].float() == -float("inf")).all())
    if kind == "nan":
        c = R.GEMM_NAN_COL
        for t, what in ((R.decode(codes), "h8"), (t16.float().cpu(), "h16"), (u16.float().cpu(), "u16")):
            nan = torch.isnan(t)
            assert bool(nan[:, c].all()) and int(nan.sum()) == M, f"{family}, {what}: NaN in {int(nan.sum())} cells, {int(nan[:, c].sum())} of them in column {c}"
        others = torch.arange(N) != c
        assert torch.equal(codes[:, others], clean8.cpu()[:, others]), "a NaN column changed other columns"
