"""CPU reference of the fp8 (OCP e4m3) kernels: the conversion, the exact code spacing, the gate every e4m3 output is held to, and the inputs
of tests/test_fp8_kernels_gpu.py.  tests/test_fp8_ref_cpu.py proves the helper against the 254 finite codes and shows that every input,
evaluated in fp32 and in fp64, gives the same e4m3 codes on all but a share of cells below half of the cap the GPU test applies - so the
reference alone never uses up the allowance.

e4m3: 1 sign, 4 exponent (bias 7), 3 mantissa bits; no infinities; 0x7F / 0xFF are the NaN; the largest finite value is 448 (0x7E / 0xFE).
Subnormals are the multiples of 2^-9 below 2^-6.  The kernels saturate: everything beyond +-448, infinities included, becomes +-448.  A value
of 464 or more would round to the next code if there were one, so a cell whose reference lies beyond +-480 - a whole code step past 448 -
is saturated whatever the last bits of the fp32 arithmetic in front of it."""
import functools
import math

import torch

E4M3_MAX = 448.0
SAT_FROM = 480.0                  # |reference| >= this: the byte is 0x7E / 0xFE exactly
CAP_LN, CAP_GELU, CAP_QUANT = 1e-2, 2e-2, 1e-3      # share of cells that may differ from the reference code (tests/test_kernels_gpu.py's figures)


def rnd(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g) * scale


def e4m3(t):
    """fp32 / fp64 -> OCP e4m3, round to nearest even, saturating (+-inf -> +-448), a NaN stays a NaN: (bytes uint8, dequantised fp32)"""
    q = t.float().clamp(-E4M3_MAX, E4M3_MAX).to(torch.float8_e4m3fn)
    return q.view(torch.uint8), q.float()


def decode(b):
    """e4m3 bytes (uint8) -> fp32"""
    return b.contiguous().view(torch.float8_e4m3fn).float()


def e4m3_step(v):
    """the spacing of the e4m3 codes at |v| (towards larger magnitudes): 2^-9 below 2^-6, 2^(floor(log2 |v|) - 3) from there on"""
    a = torch.as_tensor(v).double().abs()
    _, e = torch.frexp(a)                                # a = m 2^e with m in [0.5, 1): floor(log2 a) = e - 1, exactly
    return torch.where(a < 2.0 ** -6, torch.tensor(2.0 ** -9, dtype=torch.float64), torch.ldexp(torch.ones_like(a), e - 4))


def check_e4m3(got_bytes, want_f32, cap, what):
    """got_bytes: the kernel's uint8 output; want_f32: the reference value in front of the conversion (any float dtype, already scaled).
    Asserts, against the reference code e4m3(want_f32):
      * a NaN exactly where the reference has one;
      * |reference| >= 480 (infinities included): the byte is exactly 0x7E / 0xFE, by sign;
      * every other cell is the reference code or one of its two neighbours - the difference of the decoded values is at most the code
        spacing at the smaller of the two magnitudes (values compare, so -0 == +0);
      * at most `cap` of the cells differ from the reference code at all.
    Returns (cells compared, cells that differ) for the report."""
    got_bytes = got_bytes.detach().cpu().contiguous()
    want = torch.as_tensor(want_f32).detach().cpu()
    assert got_bytes.dtype == torch.uint8 and got_bytes.shape == want.shape, f"{what}: shape / dtype"
    _, ref = e4m3(want)
    got = decode(got_bytes)
    nan_ref, nan_got = torch.isnan(ref), torch.isnan(got)
    assert torch.equal(nan_got, nan_ref), f"{what}: NaN codes in {int(nan_got.sum())} cells, the reference has {int(nan_ref.sum())} ({int((nan_got != nan_ref).sum())} cells differ)"
    sat = (want.double().abs() >= SAT_FROM) & ~nan_ref
    sat_want = torch.where(want < 0, 0xFE, 0x7E).to(torch.uint8)
    bad_sat = sat & (got_bytes != sat_want)
    assert not bad_sat.any(), f"{what}: {int(bad_sat.sum())} of {int(sat.sum())} cells beyond +-{SAT_FROM:g} are not 0x7E / 0xFE"
    fin = ~nan_ref
    g, r = got[fin].double(), ref[fin].double()
    diff = (g - r).abs()
    step = e4m3_step(torch.minimum(g.abs(), r.abs()))
    worst = (diff - step).max().item() if diff.numel() else 0.0
    assert worst <= 0.0, f"{what}: {int((diff > step).sum())} of {diff.numel()} cells more than one code from the reference (worst by {worst:.3e})"
    differ = int((diff != 0).sum())
    share = differ / max(diff.numel(), 1)
    assert share <= cap, f"{what}: {differ} of {diff.numel()} cells ({share:.3e}) differ from the reference code, cap {cap:g}"
    return diff.numel(), differ


def code_disagreement(a, b):
    """share of cells on which two evaluations of one reference land on different e4m3 codes (values compare: -0 == +0; NaN == NaN)"""
    _, qa = e4m3(a)
    _, qb = e4m3(b)
    same = (qa == qb) | (torch.isnan(qa) & torch.isnan(qb))
    return 1.0 - same.double().mean().item()


def gelu(u):
    """exact-erf GELU in the dtype of u, written out: +inf stays +inf and -inf gives NaN (-inf * 0) in fp32 and fp64 alike"""
    return 0.5 * u * (1.0 + torch.erf(u * (2.0 ** -0.5)))


def layer_norm(x, gamma, beta, eps=1e-5):
    """nn.LayerNorm in the dtype of x, written out (two-pass statistics, biased variance, eps inside the root)"""
    mean = x.mean(1, keepdim=True)
    var = ((x - mean) ** 2).mean(1, keepdim=True)
    return (x - mean) / torch.sqrt(var + eps) * gamma + beta


# --------------------------------------------------------------------------------------------------------------------------- LayerNorm
LN_SHAPES = [(9, 4), (65, 192), (130, 260), (33, 2048), (258, 1024)]
LN_SCALE = 32.0
LN_EDGE_SHAPE = (65, 192)
LN_SAT_SCALE = 256.0              # |y| > 1.875 saturates: about 6 % of a unit normal
SUBNORMAL_SCALE = 2.0 ** -9       # |y| < 8 lands below 2^-6; |y| < 0.5 rounds to zero
LN_NAN_CELL = (7, 100)            # one NaN in the input: row 7 of every output is NaN
LN_INF_CELLS = ((3, 5, math.inf), (12, 77, -math.inf))      # in the INPUT: inf - mean = NaN, the row's statistics and the whole row are NaN
LN_INF_BETA = ((20, math.inf), (41, -math.inf))             # in beta: y = finite + inf, the column saturates to +-448


@functools.lru_cache(maxsize=None)
def ln_inputs(M, d):
    """rows with a DC offset (tests/test_kernels_gpu.py::test_ln_fwd_fp8); shared and read only"""
    return rnd(M, d, seed=1) * 2 + 0.3, 1 + 0.1 * rnd(d, seed=2), 0.1 * rnd(d, seed=3)


@functools.lru_cache(maxsize=None)
def ln_edge_inputs(kind):
    """(x, gamma, beta, out_scale) of the format-edge cases: 'saturate', 'saturate_inf', 'subnormal', 'nan'"""
    x, gamma, beta = (t.clone() for t in ln_inputs(*LN_EDGE_SHAPE))
    scale = {"saturate": LN_SAT_SCALE, "saturate_inf": LN_SAT_SCALE, "subnormal": SUBNORMAL_SCALE, "nan": LN_SCALE}[kind]
    if kind == "saturate_inf":
        for r, c, v in LN_INF_CELLS:
            x[r, c] = v
        for c, v in LN_INF_BETA:
            beta[c] = v
    if kind == "nan":
        x[LN_NAN_CELL] = math.nan
    return x, gamma, beta, scale


def ln_ref(x, gamma, beta, out_scale, dtype):
    """LayerNorm * out_scale, every operation in `dtype`: what goes into the e4m3 conversion"""
    return layer_norm(x.to(dtype), gamma.to(dtype), beta.to(dtype)) * out_scale


# --------------------------------------------------------------------------------------------------------------------------- row quantisation
QUANT_SHAPES = [(5, 4), (7, 260), (130, 1024)]
QUANT_ACT_SCALE = 3.0


@functools.lru_cache(maxsize=None)
def quant_inputs(rows, cols):
    """fp32 [rows, cols]: row 1 all zero, row 2 all negative (its maximum too), the rest normal"""
    W = rnd(rows, cols, seed=5, scale=cols ** -0.5)
    W[1] = 0
    W[2] = -W[2].abs() - 1e-3
    return W


def quant_ref(W, dtype):
    """(W * sw in `dtype` - what goes into the conversion -, colscale fp64); sw = 448 / max |row|, 1 for a zero row"""
    amax = W.abs().amax(1, keepdim=True).to(dtype)
    sw = torch.where(amax > 0, E4M3_MAX / amax.clamp_min(1e-37), torch.ones_like(amax))
    return W.to(dtype) * sw, (1.0 / (QUANT_ACT_SCALE * sw.double())).reshape(-1)


# --------------------------------------------------------------------------------------------------------------------------- GEMM
GEMM_SHAPES = [(256, 256, 128), (257, 136, 128), (300, 8, 256), (520, 392, 1024)]
GEMM_LD_SHAPE = (257, 136, 128)
GEMM_EDGE_SHAPE = (257, 136, 128)
GELU_SCALE = 16.0
GELU_SAT_SCALE = 512.0            # gelu(u) > 0.9375 saturates: about a quarter of u ~ N(0, 2)
GEMM_NAN_COL = 21                 # a NaN in bias[21]: column 21 of h8, h16 and u16 is NaN
GEMM_INF_BIAS = ((9, math.inf), (100, -math.inf))      # u = +-inf: gelu(+inf) = +inf saturates to 448; gelu(-inf) = -inf * 0 is a NaN


@functools.lru_cache(maxsize=None)
def gemm_inputs(M, N, K):
    """(x [M, K], W [N, K], activation scale, bias [N], residual [M, N]) as tests/test_kernels_gpu.py::test_gemm_fp8_kernel draws them"""
    x, W = rnd(M, K, seed=1), rnd(N, K, seed=2, scale=K ** -0.5)
    return x, W, 448.0 / float(x.abs().max()) * 0.5, rnd(N, seed=3), rnd(M, N, seed=4)


def gemm_edge_bias(kind, bias):
    """(bias, out_scale) of the format-edge cases of epilogue 7 / the training GELU"""
    bias = bias.clone()
    if kind == "saturate_inf":
        for c, v in GEMM_INF_BIAS:
            bias[c] = v
    if kind == "nan":
        bias[GEMM_NAN_COL] = math.nan
    return bias, {"saturate": GELU_SAT_SCALE, "saturate_inf": GELU_SAT_SCALE, "subnormal": SUBNORMAL_SCALE, "nan": GELU_SCALE}[kind]


def gemm_operands_cpu(x, W, sa):
    """the CPU's own quantisation of the operands: (a8 bytes, dequantised A, w8 bytes, dequantised W, colscale fp32).  The GPU test takes w8 and
    colscale from nv_quant_rows_f8 instead (at most one code apart on < 1e-3 of the cells) and multiplies what the device holds."""
    a8, adq = e4m3(x * sa)
    sw = E4M3_MAX / W.abs().amax(dim=1, keepdim=True)
    w8, wdq = e4m3(W * sw)
    return a8, adq, w8, wdq, (1.0 / (sa * sw)).reshape(-1)


def gemm_ref(adq, wdq, cs, dtype):
    """(A . W^T) * colscale[n] of the dequantised operands in `dtype`"""
    return (adq.to(dtype) @ wdq.to(dtype).T) * cs.to(dtype)


def gelu_ref(acc, bias, out_scale, dtype):
    """(u, gelu(u), gelu(u) * out_scale) in `dtype`: the last is what goes into the e4m3 conversion"""
    u = acc.to(dtype) + bias.to(dtype)
    h = gelu(u)
    return u, h, h * out_scale
