"""The e4m3 reference of the fp8 kernel tests (tests/fp8_ref.py), proved without a GPU: the code spacing against all 254 finite codes, the
conversion's round trip, ties and saturation, the gate itself on planted errors - and every input tests/test_fp8_kernels_gpu.py uses,
evaluated in fp32 and in fp64: the two land on different e4m3 codes on at most HALF of the share the GPU test allows a kernel (1e-2 behind a
LayerNorm, 2e-2 behind a GELU, 1e-3 for the row quantisation), so the reference's own rounding never uses up the allowance.  The edge inputs
hold what they are for: saturating cells, subnormal cells with some rounding to zero, exactly the planted non-finite cells."""
import math

import pytest
import torch

import fp8_ref as R

FINITE = torch.tensor([b for b in range(256) if b & 0x7F != 0x7F], dtype=torch.uint8)


def test_there_are_254_finite_codes_and_two_nan():
    v = R.decode(torch.arange(256, dtype=torch.int16).to(torch.uint8))
    assert FINITE.numel() == 254 and torch.isfinite(R.decode(FINITE)).all()
    assert torch.isnan(v[0x7F]) and torch.isnan(v[0xFF]) and int(torch.isnan(v).sum()) == 2
    assert v[0x7E] == 448.0 and v[0xFE] == -448.0 and v[0x01] == 2.0 ** -9 and v[0x08] == 2.0 ** -6
    assert v[0x00] == 0 and v[0x80] == 0 and math.copysign(1.0, v[0x80].item()) == -1.0


def test_step_is_the_distance_to_the_neighbouring_code_for_every_finite_code():
    mags = R.decode(torch.arange(0x7F, dtype=torch.int16).to(torch.uint8)).double()        # 0 .. 448, ascending with the code
    assert bool((mags[1:] > mags[:-1]).all())
    up = mags[1:] - mags[:-1]                                                              # distance to the next code of larger magnitude
    step = R.e4m3_step(R.decode(FINITE))
    for sign_codes in (FINITE[FINITE < 0x80], FINITE[FINITE >= 0x80]):
        s = R.e4m3_step(R.decode(sign_codes))
        assert torch.equal(s[:-1], up)                                                     # every code below the largest: the way up
        assert s[-1] == mags[-1] - mags[-2] == 32.0                                        # 448: the way down (there is no code above)
    assert step.numel() == 254 and step.min() == 2.0 ** -9
    # between two codes the spacing is that of the code below
    mid = (mags[1:] + mags[:-1]) / 2
    assert torch.equal(R.e4m3_step(mid), up) and torch.equal(R.e4m3_step(-mid), up)


def test_round_trip_of_every_code_is_the_identity():
    b, v = R.e4m3(R.decode(FINITE))
    assert torch.equal(b, FINITE) and torch.equal(v, R.decode(FINITE))
    b, v = R.e4m3(R.decode(torch.tensor([0x7F, 0xFF], dtype=torch.uint8)))
    assert torch.isnan(v).all() and bool(((b & 0x7F) == 0x7F).all())


def test_ties_round_to_even_and_the_conversion_saturates():
    mags = R.decode(torch.arange(0x7F, dtype=torch.int16).to(torch.uint8))
    mid = (mags[1:].double() + mags[:-1].double()) / 2                                     # exact in fp32: one more mantissa bit
    b, _ = R.e4m3(mid.float())
    lo = torch.arange(0x7E, dtype=torch.int16)
    assert torch.equal(b.to(torch.int16), lo + (lo & 1))                                   # the even one of codes lo, lo + 1
    b, _ = R.e4m3(-mid.float())
    assert torch.equal(b.to(torch.int16), (lo + (lo & 1)) | 0x80)
    b, v = R.e4m3(torch.tensor([463.9, 464.0, 480.0, 1e30, math.inf, -464.0, -math.inf, math.nan]))
    assert b.tolist()[:7] == [0x7E] * 5 + [0xFE] * 2 and math.isnan(v[7].item()) and b[7] & 0x7F == 0x7F
    assert R.e4m3(torch.tensor([2.0 ** -10, 2.0 ** -10 * 1.001, 3 * 2.0 ** -10]))[0].tolist() == [0, 1, 2]      # tie to even among the subnormals


def test_the_gate_passes_neighbours_and_catches_everything_else():
    want = torch.tensor([1.0, 1.9, 2.0, -2.0 ** -9, 0.0, 500.0, -math.inf, math.nan, 2.0 ** -6])
    ref, _ = R.e4m3(want)
    assert ref.tolist()[:7] == [0x38, 0x3F, 0x40, 0x81, 0x00, 0x7E, 0xFE]
    assert R.check_e4m3(ref, want, 0.0, "same") == (8, 0)
    ok = ref.clone()
    ok[0], ok[2], ok[3], ok[4], ok[8] = 0x39, 0x3F, 0x80, 0x80, 0x07      # one code up, one down across a binade, -2^-9 -> -0, +0 -> -0, 2^-6 -> the largest subnormal
    assert R.check_e4m3(ok, want, 0.5, "neighbours") == (8, 4)            # (-0 for +0 is no difference)
    with pytest.raises(AssertionError, match="cap"):
        R.check_e4m3(ok, want, 0.49, "neighbours")
    for cell, byte, msg in ((0, 0x3A, "more than one code"), (2, 0x3E, "more than one code"), (3, 0x01, "more than one code"), (2, 0x42, "more than one code"),
                            (5, 0x7D, "0x7E"), (6, 0x7E, "0x7E"), (5, 0x7F, "NaN"), (7, 0x7E, "NaN"), (1, 0xFF, "NaN")):
        bad = ref.clone()
        bad[cell] = byte
        with pytest.raises(AssertionError, match=msg):
            R.check_e4m3(bad, want, 1.0, "planted")


# ------------------------------------------------------------------------------------------------ the inputs of the GPU tests, twice
def non_finite_cells(t):
    return {tuple(i) for i in (~torch.isfinite(t)).nonzero().tolist()}


@pytest.mark.parametrize("M,d", R.LN_SHAPES)
def test_layernorm_inputs_fp32_and_fp64_agree_on_the_codes(M, d):
    x, gamma, beta = R.ln_inputs(M, d)
    a, b = R.ln_ref(x, gamma, beta, R.LN_SCALE, torch.float32), R.ln_ref(x, gamma, beta, R.LN_SCALE, torch.float64)
    assert torch.isfinite(b).all() and b.abs().max() < 448
    assert R.code_disagreement(a, b) <= R.CAP_LN / 2


@pytest.mark.parametrize("kind", ["saturate", "saturate_inf", "subnormal", "nan"])
def test_layernorm_edge_inputs_hold_what_they_are_for(kind):
    x, gamma, beta, scale = R.ln_edge_inputs(kind)
    M, d = R.LN_EDGE_SHAPE
    a, b = R.ln_ref(x, gamma, beta, scale, torch.float32), R.ln_ref(x, gamma, beta, scale, torch.float64)
    assert R.code_disagreement(a, b) <= R.CAP_LN / 2
    assert torch.equal(torch.isnan(a), torch.isnan(b)) and torch.equal(torch.isinf(a), torch.isinf(b))
    if kind.startswith("saturate"):
        assert (b[torch.isfinite(b)].abs() >= R.SAT_FROM).double().mean().item() >= 0.02
        assert bool((b[torch.isfinite(b)] >= R.SAT_FROM).any()) and bool((b[torch.isfinite(b)] <= -R.SAT_FROM).any())      # both signs
    if kind == "saturate":
        assert torch.isfinite(b).all()
    if kind == "saturate_inf":
        # an infinity in the input makes its row's mean infinite and inf - inf a NaN: the whole row is NaN in fp32 and fp64 alike.  One in beta
        # reaches the output as itself: those columns are +-inf in every other row, and the conversion saturates them.
        nan_rows = {r for r, _, _ in R.LN_INF_CELLS}
        assert non_finite_cells(x) == {(r, c) for r, c, _ in R.LN_INF_CELLS}
        want = {(r, c) for r in range(M) for c in range(d) if r in nan_rows or c in {c for c, _ in R.LN_INF_BETA}}
        assert non_finite_cells(b) == want
        for c, v in R.LN_INF_BETA:
            rows = [r for r in range(M) if r not in nan_rows]
            assert bool((b[rows, c] == v).all())
        assert bool(torch.isnan(b[sorted(nan_rows)]).all())
    if kind == "subnormal":
        assert (b.abs() < 2.0 ** -6).double().mean().item() >= 0.10 and b.abs().max() < 2.0 ** -6
        q = R.e4m3(b)[1]
        assert bool(((q == 0) & (b != 0)).any()) and bool((q != 0).any())
    if kind == "nan":
        assert non_finite_cells(x) == {R.LN_NAN_CELL}
        assert non_finite_cells(b) == {(R.LN_NAN_CELL[0], c) for c in range(d)} and bool(torch.isnan(b[R.LN_NAN_CELL[0]]).all())


@pytest.mark.parametrize("rows,cols", R.QUANT_SHAPES)
def test_quantisation_inputs_fp32_and_fp64_agree_on_the_codes(rows, cols):
    W = R.quant_inputs(rows, cols)
    (a, _), (b, cs) = R.quant_ref(W, torch.float32), R.quant_ref(W, torch.float64)
    assert R.code_disagreement(a, b) <= R.CAP_QUANT / 2
    assert not W[1].any() and cs[1] == 1.0 / R.QUANT_ACT_SCALE and not R.e4m3(a)[0][1].any()
    assert bool((W[2] < 0).all()) and R.e4m3(a)[1][2].min() == -448.0
    q = R.e4m3(a)[1]
    live = torch.ones(rows, dtype=torch.bool)
    live[1] = False
    assert bool((q.abs().amax(1)[live] == 448.0).all())


@pytest.mark.parametrize("M,N,K", R.GEMM_SHAPES)
def test_gemm_inputs_fp32_and_fp64_agree_on_the_codes(M, N, K):
    x, W, sa, bias, _ = R.gemm_inputs(M, N, K)
    _, adq, _, wdq, cs = R.gemm_operands_cpu(x, W, sa)
    res = [R.gelu_ref(R.gemm_ref(adq, wdq, cs, dt), bias, R.GELU_SCALE, dt)[2] for dt in (torch.float32, torch.float64)]
    assert torch.isfinite(res[1]).all() and res[1].abs().max() < 448
    assert R.code_disagreement(*res) <= R.CAP_GELU / 2


@pytest.mark.parametrize("kind", ["saturate", "saturate_inf", "subnormal", "nan"])
def test_gemm_edge_inputs_hold_what_they_are_for(kind):
    M, N, K = R.GEMM_EDGE_SHAPE
    x, W, sa, bias0, _ = R.gemm_inputs(M, N, K)
    _, adq, _, wdq, cs = R.gemm_operands_cpu(x, W, sa)
    bias, scale = R.gemm_edge_bias(kind, bias0)
    (u32, h32, a), (u, h, b) = (R.gelu_ref(R.gemm_ref(adq, wdq, cs, dt), bias, scale, dt) for dt in (torch.float32, torch.float64))
    assert R.code_disagreement(a, b) <= R.CAP_GELU / 2
    assert torch.equal(torch.isnan(a), torch.isnan(b)) and torch.equal(torch.isinf(a), torch.isinf(b))
    if kind.startswith("saturate"):
        assert (b[torch.isfinite(b)] >= R.SAT_FROM).double().mean().item() >= 0.02           # (a GELU has no large negative values)
    if kind == "saturate":
        assert torch.isfinite(b).all()
    if kind == "saturate_inf":
        assert non_finite_cells(bias) == {(c,) for c, _ in R.GEMM_INF_BIAS}
        assert non_finite_cells(b) == {(r, c) for r in range(M) for c, _ in R.GEMM_INF_BIAS}
        (cp, _), (cn, _) = R.GEMM_INF_BIAS
        assert bool((b[:, cp] == math.inf).all()) and bool((u[:, cn] == -math.inf).all()) and bool(torch.isnan(b[:, cn]).all())
    if kind == "subnormal":
        assert (b.abs() < 2.0 ** -6).double().mean().item() >= 0.10 and b.abs().max() < 2.0 ** -6
        q = R.e4m3(b)[1]
        assert bool(((q == 0) & (b != 0)).any()) and bool((q != 0).any())
    if kind == "nan":
        assert non_finite_cells(bias) == {(R.GEMM_NAN_COL,)}
        want = {(r, R.GEMM_NAN_COL) for r in range(M)}
        assert non_finite_cells(b) == want and non_finite_cells(u) == want and non_finite_cells(h) == want and bool(torch.isnan(b[:, R.GEMM_NAN_COL]).all())
