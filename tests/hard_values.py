"""Hard VALUES for the 16-bit kernels: input builders, float64 references, per-element bounds and the constants K of
tests/test_hard_values_gpu.py.  tests/test_hard_values_cpu.py proves every bound on the CPU: a faithful fp32 / 16-bit restatement of each
kernel stays within K / 2 of float64 over all of these inputs, and every planted defect lands outside K on at least one of them.

One method for every gate.  The reference is float64 on the same (16-bit representable, where the kernel reads 16 bits) inputs.  The
tolerance is per element: K times a UNIT, the unit being a first-order rounding bound evaluated in float64 from the reference's own
intermediates.  K = 2 x (the restatement's largest distance in units), rounded up to the next half: the factor of two is for what the
device may legitimately do differently - summation order, fused multiply-adds, and 1-ulp v_exp_f32 / v_rcp_f32 / v_rsq_f32 class
instructions, which move isolated 16-bit roundings by one code.  MEASURED below is what test_hard_values_cpu.py measures (it asserts that
no figure has grown past its record); K follows from it by k_from().

No pytest in this file: the GPU job scripts import it too."""
import math
import os
import sys

import numpy as np
import torch

_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if _ROOT not in sys.path:                # the oracle package, when a job script imports this file without pytest's conftest
    sys.path.insert(0, _ROOT)

U24 = 2.0 ** -24                      # half an ulp of fp32 at 1: the unit of every fp32 rounding
FMT = {"bf16": dict(dtype=torch.bfloat16, mant=8, emin=-126, u=2.0 ** -9, max=float(torch.finfo(torch.bfloat16).max)),
       "fp16": dict(dtype=torch.float16, mant=11, emin=-14, u=2.0 ** -12, max=65504.0)}


def k_from(measured):
    """K of a family: twice the restatement's maximum, rounded up to the next half"""
    return math.ceil(4.0 * measured) / 2.0


# ---- what tests/test_hard_values_cpu.py measures: the restatement's largest distance from float64 in units, over every hard input of the family (rounded up
# in the last digit; the CPU test asserts that no figure has grown past its record) - and the K that follows from it
MEASURED = {
    "gelu": 2.60,            # gelu_f in fp32 (in front of the 16-bit conversion) over every code of both formats and the bf16 midpoints in [-16, 16]: 1.55e-7 max(1, |u|)
    "dgelu.bf16": 4.65,      # gelu_grad_f in fp32 over every finite bf16 code: 2.8e-7
    "dgelu.fp16": 4.79,      # ... over every finite fp16 code: 2.9e-7
    "attn.out": 1.48,        # ref_cpu._AttnEmu, both formats, every family, n = 65 / 129 / 130 / 200 at dim_head 64, n = 65 at 32, n = 130 at 128
    "attn.dv": 1.93,
    "attn.dq": 0.85,
    "attn.dk": 0.90,
    "ln.mean": 1.00,         # row_stats / ln_fwd_kernel / ln_bwd_kernel restated in fp32: the six row families at d = 192 / 768 / 2048, the six volume families
    "ln.rstd": 2.83,         # through the vector (p = 8) and the scalar (p = 9) patch gather, and the rows of the 4D pivot cases
    "ln.out": 7.10,          # (`huge` rows at d = 2048: the mean's own rounding, 2^-24 rms, against a unit that only has |mean| / std)
    "ln.dx": 3.57, 
    "ln.dgamma": 1.64,
    "ln.dbeta": 2.90,
    "ln.colsum": 1.20,
    "series.mean": 0.43,     # patch_ln_fwd_t_kernel's own statistics restated in fp32 on the pivot cases: inside the row kernels' figures (held to K["ln.mean"] / K["ln.rstd"])
    "series.rstd": 2.65,
    "adam.p": 5.51,          # oracle/train_step.py AdamW in fp32: every count, start step, weight decay and gradient scale, three steps each
    "adam.m": 1.96,
    "adam.v": 2.70,
}
K = {name: k_from(v) for name, v in MEASURED.items()}
K["series.mean"], K["series.rstd"] = K["ln.mean"], K["ln.rstd"]        # the 4D gather is held to the per-volume gather's K


# ======================================================================================================================================
# A. GELU and its derivative
# ======================================================================================================================================
def finite_codes(fmt):
    """every finite code of the format as fp32 values (both zeros included), ascending bit pattern"""
    t = torch.arange(65536, dtype=torch.int32).to(torch.int16).view(FMT[fmt]["dtype"]).float()
    return t[torch.isfinite(t)]


def gelu_values():
    """fp32 pre-activations: every finite bf16 code, every finite fp16 code, for each bf16 code in [-16, 16] the midpoint to the next code up
    (fp32 pre-activations are not 16-bit codes), and NaN, +inf, -inf at the end; padded with zeros to a multiple of 8 (the GEMM's N)."""
    b = finite_codes("bf16")
    inner = torch.sort(b[(b >= -16) & (b <= 16)]).values.unique()
    mid = ((inner[:-1].double() + inner[1:].double()) / 2).float()           # exact: neighbours differ in the last of 8 bits
    v = torch.cat([b, finite_codes("fp16"), mid, torch.tensor([float("nan"), float("inf"), float("-inf")])])
    return torch.cat([v, torch.zeros(-v.numel() % 8)])


def dgelu_values(fmt):
    """every finite code of the format, padded with zeros to the [256, 256] tensor the derivative reads as `u`"""
    c = finite_codes(fmt)
    return torch.cat([c, torch.zeros(65536 - c.numel())]).reshape(256, 256)


def phi64(u):
    """Phi(u) as 0.5 erfc(-u / sqrt 2): 1 + erf cancels in the negative tail"""
    return 0.5 * torch.special.erfc(-u.double() / math.sqrt(2.0))


def gelu64(u):
    u = u.double()
    return torch.where(u == 0, u, u * phi64(u))                  # (0 * Phi is 0 anyway; keeps -inf * 0 out of the finite cells' way)


def dgelu64(u):
    u = u.double()
    return phi64(u) + u * torch.exp(-0.5 * u * u) / math.sqrt(2.0 * math.pi)


def ulp16(x, fmt):
    """spacing of the format's codes at |x| (float64); below the normal range the subnormal spacing"""
    f = FMT[fmt]
    _, e = torch.frexp(x.double().abs())                          # |x| = m 2^e, m in [0.5, 1): floor(log2 |x|) = e - 1
    e = torch.clamp(e - 1, min=f["emin"])
    return torch.ldexp(torch.ones_like(x, dtype=torch.float64), e - (f["mant"] - 1))


def ulp32(x):
    _, e = torch.frexp(x.double().abs())
    return torch.ldexp(torch.ones_like(x, dtype=torch.float64), torch.clamp(e - 1, min=-126) - 23)


def gelu_ratio(h, u, fmt, grad=False):
    """per element: (|h - ref| - half an ulp of the output format at ref) / (2^-24 max(1, |u|)) [derivative: / 2^-24], floored at 0 -
    the number K bounds.  fmt None: h is the fp32 value in front of the conversion (no half ulp).  Only finite u; where the reference
    reaches the format's largest finite value the conversion may give it or infinity: such a cell counts 0 when h is that infinity."""
    u64, h64 = u.double(), h.double()
    ref = dgelu64(u64) if grad else gelu64(u64)
    unit = U24 * (torch.ones_like(u64) if grad else u64.abs().clamp_min(1.0))
    half = 0.5 * ulp16(ref, fmt) if fmt else torch.zeros_like(ref)
    r = ((h64 - ref).abs() - half).clamp_min(0.0) / unit
    if fmt:
        over = ref.abs() >= FMT[fmt]["max"]
        r = torch.where(over & torch.isinf(h64) & (torch.sign(h64) == torch.sign(ref)), torch.zeros_like(r), r)
    return r


A5, A4, A3, A2, A1, AP = 1.061405429, -1.453152027, 1.421413741, -0.284496736, 0.254829592, 0.3275911      # Abramowitz-Stegun 7.1.26


def erf_parts32(u, a1=A1, ap=AP, gauss_of_x=False):
    """csrc/common.h erf_parts in numpy float32, operation by operation (a correctly rounded 1 / x and exp in place of v_rcp_f32 and
    v_exp_f32, no fused multiply-adds).  a1 / ap / gauss_of_x plant the defects of the issue."""
    f = np.float32
    u = np.asarray(u, dtype=f)
    with np.errstate(over="ignore", invalid="ignore"):
        x = np.abs(u) * f(0.70710678118654752440)
        t = f(1.0) / (f(1.0) + f(ap) * x)
        gauss = np.exp(-x if gauss_of_x else -x * x).astype(f)
        poly = ((((f(A5) * t + f(A4)) * t + f(A3)) * t + f(A2)) * t + f(a1)) * t
        erf = np.copysign(f(1.0) - poly * gauss, u).astype(f)
    return erf, gauss


def gelu32(u, **defect):
    f = np.float32
    u = np.asarray(u, dtype=f)
    e, _ = erf_parts32(u, **defect)
    with np.errstate(over="ignore", invalid="ignore"):
        return torch.from_numpy((f(0.5) * u * (f(1.0) + e)).astype(f))


def dgelu32(u, **defect):
    f = np.float32
    u = np.asarray(u, dtype=f)
    e, g = erf_parts32(u, **defect)
    with np.errstate(over="ignore", invalid="ignore"):
        return torch.from_numpy((f(0.5) * (f(1.0) + e) + u * g * f(0.39894228040143267794)).astype(f))


GELU_DEFECTS = {"a1 = 0.254929592 (4th digit)": dict(a1=0.254929592), "p = 0.3276911 (4th digit)": dict(ap=0.3276911),
                "gauss = exp(-x)": dict(gauss_of_x=True)}


def to16(t, fmt):
    """round to nearest even to the format, fp32 storage"""
    return t.to(FMT[fmt]["dtype"]).float()


def same_values(a, b):
    """equal as values, NaN in the same places (torch.equal calls NaN != NaN)"""
    a, b = a.detach().cpu().float(), b.detach().cpu().float()
    return a.shape == b.shape and bool(torch.equal(torch.isnan(a), torch.isnan(b))) and bool(torch.equal(torch.nan_to_num(a, nan=0.0), torch.nan_to_num(b, nan=0.0)))


# ======================================================================================================================================
# C. The LayerNorm family
# ======================================================================================================================================
LN_EPS = 1e-5
ROW_FAMILIES = ("offset", "outlier", "constant", "tiny", "huge", "benign")


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def ln_rows(family, M, d, seed=0):
    """fp32 rows [M, d] of one family.  `constant` rows hold multiples of 1/4 so that their fp32 sums are exact in any order: the mean IS the
    value, xhat is exactly 0 and y exactly beta."""
    g = _gen(1000 + seed)
    r = torch.randn(M, d, generator=g)
    if family == "offset":
        return 100.0 + r
    if family == "outlier":
        r[torch.arange(M), (torch.arange(M) * 37 + 5) % d] = 300.0
        return r
    if family == "constant":
        return ((torch.arange(M) % 9 - 3).float() * 2.75).reshape(M, 1).expand(M, d).contiguous()
    if family == "tiny":
        return r * 1e-4
    if family == "huge":
        return r * 1e3
    assert family == "benign"
    return r * 2.0 + 0.3


def ln_params(d, seed=0):
    g = _gen(2000 + seed)
    return 1 + 0.1 * torch.randn(d, generator=g), 0.1 * torch.randn(d, generator=g)


def ln64(x, gamma, beta, eps=LN_EPS, dy=None):
    """float64 LayerNorm over the last dimension with every intermediate the units need; with dy also the backward"""
    x, gamma, beta = x.double(), gamma.double(), beta.double()
    eps = torch.as_tensor(eps, dtype=torch.float64)
    if eps.dim():
        eps = eps.reshape(-1, 1)
    mean = x.mean(1, keepdim=True)
    var = ((x - mean) ** 2).mean(1, keepdim=True)
    rstd = 1.0 / torch.sqrt(var + eps)
    xh = (x - mean) * rstd
    y = xh * gamma + beta
    rms = torch.sqrt((x * x).mean(1, keepdim=True))
    r = dict(mean=mean[:, 0], rstd=rstd[:, 0], xh=xh, y=y,
             u_mean=U24 * (mean.abs() + rms)[:, 0], u_rstd=U24 * rstd[:, 0],
             u_xh=U24 * (mean.abs() * rstd + xh.abs()))                    # what the fp32 statistics do to xhat: the |mean| / std + |xhat| of the output unit
    r["u_y"] = gamma.abs() * r["u_xh"] + U24 * y.abs()
    if dy is not None:
        dy = dy.double()
        dyg = dy * gamma
        c1, c2 = dyg.mean(1, keepdim=True), (dyg * xh).mean(1, keepdim=True)
        r["dx"] = rstd * (dyg - c1 - xh * c2)
        # 2^-24 rstd (|dy gamma| + |c1| + |xhat c2|) with two first-order terms written out.  (1) c1 and c2 are SUMS: their rounding is 2^-24 of the mean of the
        # |terms| (as for the column sums), not of the result - rows whose dy gamma average out to c1 = 0 still carry it, and `constant` / `tiny` rows multiply it by
        # rstd = 316.  (2) xhat inherits u_xh from the fp32 statistics where it enters: xhat c2 here, dy xhat in dgamma; without it the `offset` rows
        # (|mean| / std = 100) alone would set K a hundred times above what every other family needs.  It enters twice: directly, and through c2 = mean(dy gamma xhat).
        a1, a2 = dyg.abs().mean(1, keepdim=True), (dyg * xh).abs().mean(1, keepdim=True)
        r["u_dx"] = U24 * rstd * (dyg.abs() + a1 + xh.abs() * a2) + rstd * (c2.abs() * r["u_xh"] + xh.abs() * (dyg.abs() * r["u_xh"]).mean(1, keepdim=True))
        r["dgamma"], r["dbeta"] = (dy * xh).sum(0), dy.sum(0)
        r["u_dgamma"] = U24 * (dy * xh).abs().sum(0) + (dy.abs() * r["u_xh"]).sum(0)
        r["u_dbeta"] = U24 * dy.abs().sum(0)
        r["colsum"] = r["dx"].sum(0)
        r["u_colsum"] = U24 * r["dx"].abs().sum(0) + r["u_dx"].sum(0)
    return r


def ratio(got, ref, unit, fmt=None):
    """per element (|got - ref| - half an ulp of the 16-bit output at ref) / unit, floored at 0; a zero unit with a zero difference counts 0"""
    got, ref, unit = got.detach().cpu().double(), ref.double(), unit.double()
    d = (got - ref).abs()
    if fmt:
        d = (d - 0.5 * ulp16(ref, fmt)).clamp_min(0.0)
    return torch.where(d == 0, torch.zeros_like(d), d / unit.clamp_min(1e-300))


def _butterfly32(s):
    """wave_sum (csrc/common.h): v += shfl_xor(v, o) for o = 32 .. 1, on fp32 [M, 64]"""
    lanes = np.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        s = (s + s[:, lanes ^ o]).astype(np.float32)
    return s[:, 0]


def _rowsum32(t, d, vec=True):
    """the row reduction of the wave-per-row kernels in fp32: a lane adds its float4 #(lane + 64 v) [vec] or its element lane + 64 v, v ascending, then wave_sum"""
    M = t.shape[0]
    nv = -(-d // (256 if vec else 64))
    pad = np.zeros((M, nv * (256 if vec else 64)), dtype=np.float32)
    pad[:, :d] = t
    if vec:
        r = pad.reshape(M, nv, 64, 4)
        part = ((r[..., 0] + r[..., 1]) + (r[..., 2] + r[..., 3])).astype(np.float32)
    else:
        part = pad.reshape(M, nv, 64)
    s = np.zeros((M, 64), dtype=np.float32)
    for v in range(nv):
        s = (s + part[:, v]).astype(np.float32)
    return _butterfly32(s)


def ln32(x, gamma, beta, eps=LN_EPS, dy=None, vec=True):
    """csrc/norm.hip row_stats / ln_fwd_kernel / ln_bwd_kernel (and the scalar patch path, vec=False) in numpy float32, operation by operation"""
    f = np.float32
    x, gamma, beta = (np.asarray(t, dtype=f) for t in (x, gamma, beta))
    M, d = x.shape
    eps = np.broadcast_to(np.asarray(eps, dtype=f), (M,))
    mean = (_rowsum32(x, d, vec) / f(d)).astype(f)
    t = (x - mean[:, None]).astype(f)
    rstd = (f(1.0) / np.sqrt((_rowsum32((t * t).astype(f), d, vec) / f(d) + eps).astype(f))).astype(f)
    r = dict(mean=mean, rstd=rstd, y=((t * rstd[:, None]).astype(f) * gamma + beta).astype(f))
    if dy is not None:
        dy = np.asarray(dy, dtype=f)
        xh = (t * rstd[:, None]).astype(f)
        dyg = (dy * gamma).astype(f)
        c1 = (_rowsum32(dyg, d) / f(d)).astype(f)
        c2 = (_rowsum32((dyg * xh).astype(f), d) / f(d)).astype(f)
        r["dx"] = (((dyg - c1[:, None]).astype(f) - (xh * c2[:, None]).astype(f)).astype(f) * rstd[:, None]).astype(f)
        ag, ab, ac = np.zeros(d, dtype=f), np.zeros(d, dtype=f), np.zeros(d, dtype=f)
        for m in range(M):                                    # the column accumulators, rows in order
            ag, ab, ac = (ag + (dy[m] * xh[m]).astype(f)).astype(f), (ab + dy[m]).astype(f), (ac + r["dx"][m]).astype(f)
        r["dgamma"], r["dbeta"], r["colsum"] = ag, ab, ac
    return {k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in r.items()}


# ---- volumes whose patches are the hard rows: one family per sample ------------------------------------------------------------------
VOLUME_FAMILIES = ("edge", "zscored_edge", "offset", "tiny", "huge", "benign")


def volumes(S, seed=0):
    """[6, S, S, S] fp32.  `edge`: raw scanner values, tissue 8000 +- 20 with the background (0) filling the first three planes of every axis - every patch
    starts in the background; `zscored_edge`: the same after a z-score (-2.5 against 0.6 +- 0.05)."""
    g = _gen(3000 + seed)
    r = torch.randn(len(VOLUME_FAMILIES), S, S, S, generator=g)
    v = torch.empty_like(r)
    v[0] = 8000.0 + 20.0 * r[0]
    v[1] = 0.6 + 0.05 * r[1]
    for b, bg in ((0, 0.0), (1, -2.5)):
        v[b, :3], v[b, :, :3], v[b, :, :, :3] = bg, bg, bg
    v[2], v[3], v[4], v[5] = 100.0 + r[2], 1e-4 * r[3], 1e3 * r[4], 2.0 * r[5] + 0.3
    return v


def tokens_of(vols, p):
    """[B, H, W, D] volumes -> the [B * N, p^3] patch rows the gather kernels normalise (the oracle's index map), same dtype"""
    from oracle import ref_cpu
    return ref_cpu.patchify(ref_cpu.fmri_to_video(vols), p, p, p).reshape(-1, p ** 3)


SERIES_SHAPES = ((16, 8, 4), (32, 8, 8))          # (S, p, T): 256 and 128 voxels per round
SERIES_SIGMA = torch.tensor([0.7, 1.9, 1.3])      # vol_sigma of the three samples


def series_eps(sigma, T, N):
    """eps per token row (float64 tensor or the plain eps, and the fp32 the kernel forms: eps * sg * sg)"""
    if sigma is None:
        return LN_EPS, LN_EPS
    e32 = (np.float32(LN_EPS) * (sigma * sigma).numpy()).astype(np.float32)
    return (LN_EPS * sigma.double() ** 2).repeat_interleave(T * N), e32.repeat(T * N)


def series(S, p, T, seed=0):
    """[3, S, S, S, T] fp32 4D samples, one pivot case per sample.  Voxel 0 of every patch (the old kernel's pivot) is (0) a raw background 0 in front of tissue
    8000 +- 20, (1) a z-scored background -2.5 in front of 0.6 +- 0.05, (2) an outlier 1000 in front of N(0.3, 1.5); the timepoints differ in level and
    flatness (the flatter the patch, the larger the old loss)."""
    g = _gen(4000 + seed + S + T)
    r = torch.randn(3, S, S, S, T, generator=g)
    flat = 1.0 / (1.0 + torch.arange(T).float())               # timepoint t: spread / (1 + t)
    x = torch.empty_like(r)
    x[0] = 8000.0 + 20.0 * r[0] * flat
    x[1] = 0.6 + 0.05 * r[1] * flat
    x[2] = 0.3 + 1.5 * r[2] * flat
    for b, piv in enumerate((0.0, -2.5, 1000.0)):
        x[b, ::p, ::p, ::p, :] = piv
    return x.contiguous()


def series_tokens(x, p):
    """[Bo, H, W, D, T] -> rows (bo T + t) N + n of the regrouped volumes (NeuroEncoder.py:54-56), [Bo T N, p^3]"""
    Bo, H, W, D, T = x.shape
    return tokens_of(x.permute(0, 4, 1, 2, 3).reshape(Bo * T, H, W, D), p)


def series_kr(T):
    """voxels per round of patch_ln_fwd_t_kernel (csrc/norm.hip patch_ln_fwd_4d_launch)"""
    tg = T // 4
    nact = (256 // tg) * tg
    nact -= (nact // tg % 4) * tg
    return nact // tg


def series_stats32(rows, T, eps=LN_EPS, old=False):
    """The statistics of patch_ln_fwd_t_kernel on rows [R, P] (any timepoint: they do not mix) in numpy float32.  A thread sums voxels kk, kk + KR, ...; one thread
    per timepoint adds the KR partials in four interleaved chains.  old=True: the kernel before the fix - one sweep of sums shifted by voxel 0 and
    var = q / P - ms^2, the partials added in one chain."""
    f = np.float32
    x = np.asarray(rows, dtype=f)
    R, P = x.shape
    KR = series_kr(T)
    eps = np.broadcast_to(np.asarray(eps, dtype=f), (R,))

    def sweep(pivot, squares):
        d = (x - pivot[:, None]).astype(f)
        nj = -(-P // KR)
        pad = np.zeros((R, nj * KR), dtype=f)
        pad[:, :P] = d
        pad = pad.reshape(R, nj, KR)
        s1, s2 = np.zeros((R, KR), dtype=f), np.zeros((R, KR), dtype=f)
        for j in range(nj):
            s1 = (s1 + pad[:, j]).astype(f)
            if squares:
                s2 = (s2 + (pad[:, j] * pad[:, j]).astype(f)).astype(f)
        return s1, s2

    def chains(s, kahan):
        acc, c = np.zeros(R, dtype=f), np.zeros(R, dtype=f)
        for j in range(KR):
            if kahan:
                y = (s[:, j] - c).astype(f)
                t = (acc + y).astype(f)
                c = ((t - acc).astype(f) - y).astype(f)
                acc = t
            else:
                acc = (acc + s[:, j]).astype(f)
        return acc

    if old:
        pivot = x[:, 0].copy()
        s1, s2 = sweep(pivot, True)
        a, q = chains(s1, False), chains(s2, False)
    else:
        s1, _ = sweep(x[:, 0].copy(), False)
        pivot = (x[:, 0] + (chains(s1, False) / f(P)).astype(f)).astype(f)
        s1, s2 = sweep(pivot, True)
        a, q = chains(s1, True), chains(s2, True)
    ms = (a / f(P)).astype(f)
    var = np.maximum(((q / f(P)).astype(f) - (ms * ms).astype(f)).astype(f), f(0))
    mean = (pivot + ms).astype(f)
    rstd = (f(1.0) / np.sqrt((var + eps).astype(f))).astype(f)
    return torch.from_numpy(mean), torch.from_numpy(rstd)


# ======================================================================================================================================
# D. AdamW at the level of the update
# ======================================================================================================================================
ADAM = dict(lr=1e-3, betas=(0.9, 0.999), eps=1e-8)
ADAM_COUNTS = (4, 2044, 2052, 4104)
ADAM_STARTS = (1, 1000, 100000)
ADAM_DECAYS = (0.0, 1e-2)
ADAM_SCALES = (1.0, 2.0 ** -16)


def adam_inputs(n, start, seed=0):
    """p0, three gradients, m0, v0 (fp32, [n]).  |p| spans 1e-4 .. 10 (log-uniform); |g| cycles through 0, 1e-12, 1e-8 (= eps) and log-uniform 1e-4 .. 10, the sign of
    an element's gradient the same in all three steps (m never cancels: its relative gate stays meaningful).  start = 1: zero moments; later starts: moments of a run
    in progress."""
    g = _gen(5000 + seed + n + start)
    sign = torch.where(torch.rand(n, generator=g) < 0.5, -1.0, 1.0)
    p0 = torch.where(torch.rand(n, generator=g) < 0.5, -1.0, 1.0) * 10.0 ** (torch.rand(n, generator=g) * 5 - 4)
    grads = []
    for s in range(3):
        mag = 10.0 ** (torch.rand(n, generator=g) * 5 - 4)
        kind = (torch.arange(n) + s) % 8
        mag = torch.where(kind == 0, torch.zeros(n), mag)
        mag = torch.where(kind == 1, torch.full((n,), 1e-12), mag)
        mag = torch.where(kind == 2, torch.full((n,), 1e-8), mag)
        grads.append((sign * mag).float())
    if start == 1:
        m0, v0 = torch.zeros(n), torch.zeros(n)
    else:
        mag = 10.0 ** (torch.rand(n, generator=g) * 5 - 4)
        m0, v0 = (sign * mag * 0.5).float(), (mag * mag * 0.7).float()
    return p0.float(), grads, m0, v0


def adam64(p, g, m, v, step, weight_decay, grad_scale, lr=ADAM["lr"], betas=ADAM["betas"], eps=ADAM["eps"]):
    """one float64 torch.optim.AdamW step from the fp32 state (p, m, v) and the fp32 gradient: (p, m, v, |p - p_before| = the update)"""
    p, g, m, v = p.double(), g.double() * grad_scale, m.double(), v.double()
    b1, b2 = betas
    pn = p * (1.0 - lr * weight_decay)
    m = m + (g - m) * (1.0 - b1)
    v = v * b2 + (1.0 - b2) * g * g
    pn = pn - (lr / (1.0 - b1 ** step)) * m / (v.sqrt() / math.sqrt(1.0 - b2 ** step) + eps)
    return pn, m, v, (pn - p).abs()


def adam32(p, g, m, v, step, weight_decay, grad_scale):
    """the oracle's AdamW (oracle/train_step.py) in float32 on the same state: the restatement"""
    from oracle import train_step
    params = {"w": p.clone()}
    opt = train_step.AdamW(params, lr=ADAM["lr"], betas=ADAM["betas"], eps=ADAM["eps"], weight_decay=weight_decay)
    opt.t, opt.m["w"], opt.v["w"] = step - 1, m.clone(), v.clone()
    opt.step({"w": g * torch.tensor(grad_scale, dtype=torch.float32)})
    return params["w"], opt.m["w"], opt.v["w"]


def adam_ratios(p, m, v, ref):
    """(p, m, v) of one step against adam64's result: the largest of (|p - ref| - 2 ulp32(ref)) / (2^-24 |update|) and of the relative errors of m and v / 2^-24"""
    pr, mr, vr, upd = ref
    rp = ((p.detach().cpu().double() - pr).abs() - 2.0 * ulp32(pr)).clamp_min(0.0)
    rp = torch.where(rp == 0, torch.zeros_like(rp), rp / (U24 * upd).clamp_min(1e-300))
    return float(rp.max()), float(ratio(m, mr, U24 * mr.abs()).max()), float(ratio(v, vr, U24 * vr.abs()).max())


# ======================================================================================================================================
# B. Attention on structured scores
# ======================================================================================================================================
ATTN_FAMILIES = ("peaked", "late_max", "sink", "ties", "cancel", "benign")
ATTN_SHAPES = (65, 130, 200)           # one tile + 1; two tiles + 2 (both half-range states live); four tiles.  n = 129 for the wide kernel
ATTN_B, ATTN_HEADS = 2, 2


def attn_qkv(family, n, fmt, dh=64, seed=0):
    """[B n, 3 heads dh] fp32 holding values of the 16-bit format"""
    B, heads = ATTN_B, ATTN_HEADS
    g = _gen(6000 + seed + n + dh)
    q, k, v = (torch.randn(B, n, heads, dh, generator=g) for _ in range(3))
    pat = torch.where(torch.arange(dh) % 2 == 0, 1.0, -1.0)             # a direction every query shares
    if family == "peaked":
        q, k = q * 3.5, k * 3.5                                          # scores N(0, 12^2): mean row maximum of P about 0.85
    elif family == "late_max":
        q = 0.5 * q + 0.75 * pat                                         # q . k_last / sqrt(dh) = 0.75 sqrt(dh): the LAST key dominates every row
        k = 0.5 * k
        k[:, n - 1] = pat
    elif family == "sink":
        q = 0.5 * q + 0.75 * pat
        k = 0.5 * k
        k[:, 0] = pat                                                    # key 0 (cls) takes most of the mass ...
        v[:, 0] = 50.0 * v[:, 0]                                         # ... and its value row is 50 times the others
    elif family == "ties":
        k = k[:, :1].expand(B, n, heads, dh).clone()                     # all keys identical: P = 1 / n
    elif family == "cancel":
        q, k = 0.3 * q, 0.3 * k                                          # nearly flat softmax over value rows that cancel
        v = 8.0 * torch.where(torch.arange(n) % 2 == 0, 1.0, -1.0).reshape(1, n, 1, 1) + 0.05 * v
    else:
        assert family == "benign"
    return to16(torch.cat([t.reshape(B * n, heads * dh) for t in (q, k, v)], dim=1), fmt)


def attn_dout(n, fmt, dh=64, seed=0):
    return to16(torch.randn(ATTN_B * n, ATTN_HEADS * dh, generator=_gen(7000 + seed + n + dh)), fmt)


def split_heads(t, n, dh=64):
    """[B n, heads dh] -> [B, heads, n, dh]"""
    return t.reshape(ATTN_B, n, ATTN_HEADS, dh).permute(0, 2, 1, 3)


def merge_heads(t):
    B, h, n, dh = t.shape
    return t.permute(0, 2, 1, 3).reshape(B * n, h * dh)


def attn64(qkv, dout, n, fmt, dh=64, out16=None):
    """float64 attention forward and backward on [B n, 3 inner] / [B n, inner], every result as [B n, inner] (lse [B, heads, n]), with the units.
    out16: the 16-bit forward output delta = rowsum(dO O) was formed from (the kernel's own); the units allow for its rounding either way."""
    u, scale = FMT[fmt]["u"], dh ** -0.5
    q, k, v = (split_heads(t, n, dh).double() for t in qkv.chunk(3, dim=1))
    do = split_heads(dout, n, dh).double()
    s = q @ k.transpose(-1, -2) * scale
    p = torch.softmax(s, dim=-1)
    o = p @ v
    dv = p.transpose(-1, -2) @ do
    dp = do @ v.transpose(-1, -2)
    delta = (do * o).sum(-1, keepdim=True)
    ds = p * (dp - delta)
    dq, dk = ds @ k * scale, ds.transpose(-1, -2) @ q * scale
    a = 2 * u * ds.abs() + p * u * (do.abs() * o.abs()).sum(-1, keepdim=True)
    floor = n * 2.0 ** -25 if fmt == "fp16" else 0.0            # fp16: P and dS below 2^-14 are subnormal codes (spacing 2^-24): half of it per key
    r = dict(out=o, dv=dv, dq=dq, dk=dk, lse=torch.logsumexp(s, dim=-1),
             u_out=u * (p @ v.abs() + o.abs()) + floor * v.abs().max(),
             u_dv=u * (p.transpose(-1, -2) @ do.abs() + dv.abs()) + floor * do.abs().max(),
             u_dq=scale * (a @ k.abs()) + u * dq.abs() + floor * scale * k.abs().max(),
             u_dk=scale * (a.transpose(-1, -2) @ q.abs()) + u * dk.abs() + floor * scale * q.abs().max())
    return {key: (val if key == "lse" else merge_heads(val)) for key, val in r.items()}


def attn_emu(qkv, dout, n, fmt, dh=64):
    """the oracle's restatement of the kernels (ref_cpu._AttnEmu: 64-key tiles, two half-range states, the 16-bit cast points), backward from its own output"""
    from oracle import ref_cpu
    with ref_cpu.operand_format(fmt):
        q, k, v = (split_heads(t, n, dh).clone().requires_grad_(True) for t in qkv.chunk(3, dim=1))
        o = ref_cpu._AttnEmu.apply(q, k, v, dh ** -0.5)
        o.backward(split_heads(dout, n, dh))
    return dict(out=merge_heads(o.detach()), dq=merge_heads(q.grad), dk=merge_heads(k.grad), dv=merge_heads(v.grad))


ATTN_DEFECTS = ("padded key in the normaliser", "last key dropped", "rescale skipped in the last tile")


def attn64_defect(qkv, n, defect, dh=64):
    """float64 forward output [B n, inner] of an attention with one planted defect"""
    scale = dh ** -0.5
    q, k, v = (split_heads(t, n, dh).double() for t in qkv.chunk(3, dim=1))
    s = q @ k.transpose(-1, -2) * scale
    if defect == ATTN_DEFECTS[0]:                    # one zero-score key of the ragged tile's padding counted in the row sum
        m = s.amax(-1, keepdim=True).clamp_min(0.0)
        e = torch.exp(s - m)
        return merge_heads(e @ v / (e.sum(-1, keepdim=True) + torch.exp(-m)))
    if defect == ATTN_DEFECTS[1]:
        return merge_heads(torch.softmax(s[..., :-1], dim=-1) @ v[..., :-1, :])
    assert defect == ATTN_DEFECTS[2]                 # online softmax over 64-key tiles; o and l keep their old scale when the maximum moves in the last tile
    m = torch.full(s.shape[:-1] + (1,), float("-inf"), dtype=torch.float64)
    l, o = torch.zeros_like(m), torch.zeros_like(q)
    tiles = list(range(0, n, 64))
    for k0 in tiles:
        st = s[..., k0:k0 + 64]
        mnew = torch.maximum(m, st.amax(-1, keepdim=True))
        alpha = torch.exp(m - mnew)
        if k0 == tiles[-1]:
            alpha = torch.ones_like(alpha)
        pt = torch.exp(st - mnew)
        l, o, m = l * alpha + pt.sum(-1, keepdim=True), o * alpha + pt @ v[..., k0:k0 + 64, :], mnew
    return merge_heads(o / l)
