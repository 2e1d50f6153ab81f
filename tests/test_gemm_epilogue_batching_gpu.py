"""The LDS epilogues of the large-tile GEMMs request their global operands once per tile, ahead of the arithmetic (csrc/gemm_common.h:
epilogue_lds_request / epilogue_lds_finish).  What that structure can get wrong, at the smallest shapes that reach it: tile rows and tile
columns with a single valid row / column group (the hoisted loads are clamped there and their values must not be used), a single K tile
(nothing covers the loads), row-strided and in-place residuals, the optional second output of the GELU epilogue, the accumulating fp32
store that reads its own output, the dropout masks' element indexing, and run-to-run bit equality (the loads are issued while the operand
ring is still in use).  Tolerances and the fp64 reference are those of tests/test_kernels_gpu.py."""
import pytest
import torch
import torch.nn.functional as F

from conftest import rel_err
from oracle import ref_cpu

pytestmark = pytest.mark.gpu
REL = 1e-3

PP = (4, 0)                          # nv_gemm_set_tile: the 256 x 128 ping-pong kernel
WS = [(3, 0), (3, 3)]                # the 64 x 128 warp-specialised kernel, 64-deep and 128-deep ring
PP_SHAPES = [(257, 136, 64), (300, 8, 128), (256, 128, 192)]
WS_SHAPES = [(65, 136, 128), (64, 128, 256)]
CASES = [(PP, s) for s in PP_SHAPES] + [(t, s) for t in WS for s in WS_SHAPES]
DROP_CASES = [(PP, PP_SHAPES[0])] + [(t, WS_SHAPES[0]) for t in WS]
IDS = lambda v: "x".join(str(i) for i in v)      # noqa: E731


@pytest.fixture(scope="module")
def ops():
    from neurovit_amd import ops as _ops
    from neurovit_amd._cabi import require_gpu
    require_gpu()
    return _ops


def bf(t):
    return t.to(torch.bfloat16)


def rnd(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g) * scale


def assert_close_bf16(a, b, what=""):
    a, b = a.detach().float().cpu().double(), b.detach().float().cpu().double()
    ulp = 2.0 ** (torch.floor(torch.log2(b.abs().clamp_min(1e-30))) - 7)
    tol = REL * b.abs().max() + ulp
    bad = ((a - b).abs() > tol)
    assert not bad.any(), f"{what}: {int(bad.sum())} / {bad.numel()} outside tol, max diff {(a - b).abs().max():.3e}, max ref {b.abs().max():.3e}"


def assert_close_f32(a, b, what="", rel=1e-5):
    e = rel_err(a, b)
    assert e <= rel, f"{what}: rel err {e:.3e} > {rel}"


_inputs = {}


def inputs(M, N, K):
    """Operands and fp64 references of one shape: computed once, shared by every kernel and test, never modified."""
    if (M, N, K) not in _inputs:
        A, B, Bt = bf(rnd(M, K, seed=1)), bf(rnd(N, K, seed=2, scale=K ** -0.5)), bf(rnd(K, N, seed=7, scale=K ** -0.5))
        bias, resid, u, c0 = rnd(N, seed=3), rnd(M, N, seed=4), bf(rnd(M, N, seed=8)), rnd(M, N, seed=5)
        d = dict(A=A.cuda(), B=B.cuda(), Bt=Bt.cuda(), bias=bias.cuda(), resid=resid.cuda(), u=u.cuda(), c0=c0.cuda(),
                 nt=A.double() @ B.double().T, nn=A.double() @ Bt.double(), bias64=bias.double(), resid64=resid.double(), u64=u.double(), c064=c0.double())
        _inputs[(M, N, K)] = d
    return _inputs[(M, N, K)]


def five_times(fn):
    """fn() -> tensor or tuple of tensors; five more launches must reproduce the first bit for bit."""
    first = fn()
    for _ in range(5):
        again = fn()
        for a, b in zip(first if isinstance(first, tuple) else (first,), again if isinstance(again, tuple) else (again,)):
            assert torch.equal(a, b)
    return first


@pytest.mark.parametrize("tile,shape", CASES, ids=IDS)
def test_batched_epilogues_against_fp64(ops, tile, shape):
    from neurovit_amd._cabi import lib
    M, N, K = shape
    d = inputs(M, N, K)
    A, B, Bt, bias = d["A"], d["B"], d["Bt"], d["bias"]
    lib.nv_gemm_set_tile(*tile)
    try:
        out = five_times(lambda: ops.gemm(ops.NT, ops.EPI_BIAS_F32, A, B, bias=bias))
        assert_close_f32(out, d["nt"] + d["bias64"], "bias_f32")

        # residual as a row-strided view (leading dimension > N), then in place (out = aux_in)
        wide = torch.full((M, N + 24), float("nan"), device="cuda")
        wide[:, 8:8 + N] = d["resid"]
        view = wide[:, 8:8 + N]
        want = d["nt"] + d["bias64"] + d["resid64"]
        out = five_times(lambda: ops.gemm(ops.NT, ops.EPI_BIAS_RESID, A, B, bias=bias, aux_in=view))
        assert_close_f32(out, want, "bias_resid strided")
        inplace = d["resid"].clone()
        ops.gemm(ops.NT, ops.EPI_BIAS_RESID, A, B, bias=bias, aux_in=inplace, out=inplace)
        assert torch.equal(inplace, out)
        wide_io = wide.clone()
        ops.gemm(ops.NT, ops.EPI_BIAS_RESID, A, B, bias=bias, aux_in=wide_io[:, 8:8 + N], out=wide_io[:, 8:8 + N])
        assert torch.equal(wide_io[:, 8:8 + N], out) and torch.isnan(wide_io[:, :8]).all() and torch.isnan(wide_io[:, 8 + N:]).all()

        # GELU with and without the pre-activation output
        uref = d["nt"] + d["bias64"]

        def gelu_u():
            u = torch.zeros((M, N), dtype=torch.bfloat16, device="cuda")
            return ops.gemm(ops.NT, ops.EPI_BIAS_GELU, A, B, bias=bias, aux_out=u), u
        h, u = five_times(gelu_u)
        assert_close_bf16(u, uref, "gelu.u")
        assert_close_bf16(h, F.gelu(uref), "gelu.h")
        h0 = five_times(lambda: ops.gemm(ops.NT, ops.EPI_BIAS_GELU, A, B, bias=bias))
        assert torch.equal(h0, h)

        du = five_times(lambda: ops.gemm(ops.NN, ops.EPI_DGELU, A, Bt, aux_in=d["u"]))
        assert_close_bf16(du, d["nn"] * ref_cpu._gelu_grad(d["u64"]), "dgelu")

        fused, part = five_times(lambda: ops.gemm_dgelu_colsum(A, Bt, d["u"]))
        assert torch.equal(fused, du)
        rows = lib.nv_gemm_tile_rows(ops.NN, M, N, K, A.stride(0), Bt.stride(0))
        assert rows == (256 if tile == PP else 64) and part.shape == ((M + rows - 1) // rows, N)
        for t in range(part.shape[0]):
            assert_close_f32(part[t], fused[t * rows:(t + 1) * rows].double().sum(0), f"colsum tile row {t}")

        def accumulate():
            c = d["c0"].clone()
            ops.gemm(ops.NT, ops.EPI_STORE_F32, A, B, out=c, accumulate=True)
            return c
        assert_close_f32(five_times(accumulate), d["nt"] + d["c064"], "accumulate")
    finally:
        lib.nv_gemm_set_tile(0, 0)


@pytest.mark.parametrize("tile,shape", DROP_CASES, ids=IDS)
def test_batched_epilogues_keep_the_dropout_masks(ops, tile, shape):
    """drop_p = 0.25: the mask of element (m, n) is a function of (seed, m * N + n) alone - two launches agree bit for bit, and the kept /
    zeroed positions are those ops.dropout_apply gives on the dense [M, N] tensor."""
    from neurovit_amd._cabi import lib
    M, N, K = shape
    d = inputs(M, N, K)
    A, B, Bt, bias = d["A"], d["B"], d["Bt"], d["bias"]
    seed, p = 1234, 0.25
    _, factor = ops.dropout_apply(torch.ones((M, N), device="cuda"), drop_seed=seed, drop_p=p, want16=False, want32=True)
    kept = factor != 0
    assert 0.15 < 1.0 - float(kept.float().mean()) < 0.35 and float((factor[kept] - 1.0 / (1.0 - p)).abs().max()) < 1e-6
    f64 = factor.double().cpu()
    lib.nv_gemm_set_tile(*tile)
    try:
        zero = torch.zeros((M, N), device="cuda")
        y = five_times(lambda: ops.gemm(ops.NT, ops.EPI_BIAS_RESID, A, B, bias=bias, aux_in=zero, drop_seed=seed, drop_p=p))
        assert torch.equal(y != 0, kept)
        assert_close_f32(y, (d["nt"] + d["bias64"]) * f64, "resid.drop")
        y = ops.gemm(ops.NT, ops.EPI_BIAS_RESID, A, B, bias=bias, aux_in=d["resid"], drop_seed=seed, drop_p=p)
        assert torch.equal(y == d["resid"], ~kept)
        assert_close_f32(y, (d["nt"] + d["bias64"]) * f64 + d["resid64"], "resid.drop + residual")

        def gelu_u():
            u = torch.zeros((M, N), dtype=torch.bfloat16, device="cuda")
            return ops.gemm(ops.NT, ops.EPI_BIAS_GELU, A, B, bias=bias, aux_out=u, drop_seed=seed, drop_p=p), u
        h, u = five_times(gelu_u)
        # (in fp32 erf(x) is exactly -1 below x = -4, so gelu(u) and gelu'(u) are exact zeros for u < -5.6 whatever the mask says: look where |u| < 4)
        sel = ((d["nt"] + d["bias64"]).abs() < 4.0).cuda()
        assert torch.equal((h != 0)[sel], kept[sel])
        assert_close_bf16(u, d["nt"] + d["bias64"], "gelu.u under dropout")
        assert_close_bf16(h, F.gelu(d["nt"] + d["bias64"]) * f64, "gelu.h under dropout")

        du = five_times(lambda: ops.gemm(ops.NN, ops.EPI_DGELU, A, Bt, aux_in=d["u"], drop_seed=seed, drop_p=p))
        sel = (d["u64"].abs() < 4.0).cuda()
        assert torch.equal((du != 0)[sel], kept[sel])
        assert_close_bf16(du, d["nn"] * f64 * ref_cpu._gelu_grad(d["u64"]), "dgelu under dropout")
        fused, part = five_times(lambda: ops.gemm_dgelu_colsum(A, Bt, d["u"], drop_seed=seed, drop_p=p))
        assert torch.equal(fused, du)
        assert_close_f32(part.sum(0), fused.double().sum(0), "colsum under dropout")
    finally:
        lib.nv_gemm_set_tile(0, 0)
