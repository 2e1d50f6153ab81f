"""Leading dimensions and write windows of the 16-bit training kernels and the fp32 inference kernels, on a real MI355X.

tests/test_kernels_gpu.py hands every 2-D kernel dense operands (ld == width) and lets it write into torch.empty((M, N)): a K used where
lda was meant, an N used for ldc in one epilogue's second output, or a ragged last tile that stores a few cells past the window changes
nothing such a test looks at.  Inside the engine every buffer is a slice of one workspace arena, where such a store lands in the
neighbouring activation and such a read takes whatever the neighbour holds.  Here every case runs the same five steps (run_windows):

  (a) dense      the kernel on dense operands, gated against a float64 restatement at the tolerance tests/test_kernels_gpu.py uses for
                 that kernel and output type (assert_close_f32 at 1e-5, assert_close_bf16, assert_close_stat) - no new tolerances
  (b) padded     every operand an into_padded view, every output a padded view (tests/ld_windows.py), each ld padded differently from its
                 neighbours of the same width; strides asserted; outputs word for word those of (a) - an ld does not change the order
                 of the arithmetic when the same kernel runs.  Where a launcher picks another kernel BECAUSE of the ld the case says so,
                 cites the line, and holds (b) to (a)'s float64 gate instead
  (c) guards     no byte outside any output's window changed: second outputs, per-row statistics and column sums (1-D, guarded) included
  (d) poisoned   once more with the inputs' spare rows and pad columns as NaN (byte 0xFF): outputs word for word those of (b), no NaN
  (e) no skips   each section starts with the table of its cases; a case is left out only where an argument check or the plan refuses
                 it - the table cites the line and the test asserts the refusal

Pads (elements): lda + 8, ldb + 16; f32 outputs + 4, 16-bit outputs + 8; ld_aux_in + 4, ld_aux_out + 8 - and + 12 / + 16 where that
would give two [M, N] operands of one call the same pad (epilogue 4: C f32 + 4, so the residual takes + 12; epilogue 3: h 16-bit + 8,
so u takes + 16; epilogue 6: C 16-bit + 8, the f32 partial rows + 12), so that two swapped lds never cancel; ld_qkv + 8, ld_out + 8,
ld_dqkv + 4; LayerNorm ldx + 4, ldy + 8, lddy + 8, ldg + 12, ldg16 + 16.
One report line per test: family, cases run, cases refused by design - the counts are asserted against the tables."""
import contextlib

import pytest
import torch
import torch.nn.functional as F

from conftest import rel_l2, report
from ld_windows import guarded, guards_intact, into_padded, into_poisoned, padded, same_window_bits
from oracle import ref_cpu
from test_kernels_gpu import assert_close_bf16, assert_close_f32, assert_close_stat, bf, dev, rnd

pytestmark = pytest.mark.gpu
SEED = ref_cpu.site_seed(123456789, 5)          # above 2^32, as tests/test_dropout_masks_cpu.py


@pytest.fixture(scope="module")
def ops():
    from neurovit_amd import ops as _ops
    from neurovit_amd._cabi import require_gpu
    require_gpu()
    return _ops


@pytest.fixture(scope="module")
def lib():
    from neurovit_amd._cabi import lib as _lib
    return _lib


class Tally:
    """cases run / refused by design of one test; done() checks them against the section's table and writes the report line"""

    def __init__(self, family):
        self.family, self.ran, self.refused = family, 0, 0

    def done(self, ran, refused):
        assert (self.ran, self.refused) == (ran, refused), f"{self.family}: {self.ran} cases run, {self.refused} refused; the table says {ran} and {refused}"
        report(f"ld windows, {self.family}: {self.ran} cases run, {self.refused} refused by design")


def refused(tl, what, fn):
    """a combination the argument checks refuse: the call raises, nothing is skipped"""
    with pytest.raises(RuntimeError):
        fn()
    torch.cuda.synchronize()
    tl.refused += 1


# ------------------------------------------------------------------------------------------------------------ the five steps
def _outputs(outs, windows):
    """outs: {name: (shape, dtype, pad_cols, init)} -> ({name: tensor}, {name: guard buffer}); shape 2-D: padded, 1-D: guarded (f32);
    init (a dense device tensor, or None): what the output holds before the call (accumulation, in-place updates)"""
    o, bufs = {}, {}
    for name, (shape, dtype, pad, init) in outs.items():
        if not windows:
            o[name] = torch.empty(shape, dtype=dtype, device="cuda") if init is None else init.clone()
            continue
        if len(shape) == 1:
            o[name], bufs[name] = guarded(shape[0], dtype)
        else:
            o[name], bufs[name] = padded(shape[0], shape[1], dtype, pad)
            assert o[name].stride(0) == shape[1] + pad and o[name].data_ptr() % 16 == 0, name
        if init is not None:
            o[name].copy_(init)
    return o, bufs


def _inputs(ins, wrap):
    """ins: {name: (dense device tensor, pad_cols or None)}; None: handed over as it is (vectors, tables)"""
    i = {}
    for name, (t, pad) in ins.items():
        if pad is None or wrap is None:
            i[name] = t
        else:
            i[name] = wrap(t, pad)
            assert i[name].stride(0) == t.shape[1] + pad and i[name].data_ptr() % 16 == 0, name
    return i


def run_windows(tl, what, call, ins, outs, gate, same_kernel=True):
    """steps (a) - (d) of the module docstring for one case.  call(i, o) launches the kernel on the inputs i, writing the outputs o;
    gate(o) holds dense-shaped outputs to float64.  same_kernel=False: the launcher takes another kernel for a padded ld (the caller
    cites the line), so (b) is held to gate instead of to (a)'s bits."""
    d, _ = _outputs(outs, False)
    call(_inputs(ins, None), d)
    torch.cuda.synchronize()
    gate(d)                                                                                              # (a)
    p, pbuf = _outputs(outs, True)
    call(_inputs(ins, into_padded), p)
    torch.cuda.synchronize()
    for name in outs:                                                                                    # (b), (c)
        if same_kernel:
            bad = same_window_bits(p[name], d[name])
            assert bad == 0, f"{tl.family}, {what}: {name}: {bad} of {d[name].numel()} cells differ from the dense run under padded leading dimensions"
        assert guards_intact(p[name], pbuf[name]), f"{tl.family}, {what}: {name}: wrote outside its window"
    if not same_kernel:
        gate({name: t.contiguous() for name, t in p.items()})
    x, xbuf = _outputs(outs, True)
    call(_inputs(ins, into_poisoned), x)
    torch.cuda.synchronize()
    for name in outs:                                                                                    # (d)
        nan = int(torch.isnan(x[name].float()).sum())
        assert nan == 0, f"{tl.family}, {what}: {name}: {nan} NaN cells - a pad cell of an input reached a stored output"
        bad = same_window_bits(x[name], p[name])
        assert bad == 0, f"{tl.family}, {what}: {name}: {bad} of {p[name].numel()} cells change with what the inputs' pad cells hold"
        assert guards_intact(x[name], xbuf[name]), f"{tl.family}, {what}: {name}: wrote outside its window (poisoned run)"
    tl.ran += 1
    return d


# ------------------------------------------------------------------------------------------------------------ GEMM (nv_gemm_bf16)
# Cases of ONE tile family, (M, N, K) = (264, 136, 128) - M ragged for 64-, 128- and 256-row tiles (the last by 8 rows), N for 128- and
# 256-wide tiles, K two 64-deep steps or one 128-deep step - and TN over 200 token rows (ragged for every K tile) with Mo = 264:
#
#   layout  epilogue                                   outputs under guard
#   NT      0 store 16-bit                             C
#   NT      1 store f32                                C
#   NT      1 store f32 + 16-bit mirror                C, aux_out
#   NT      2 bias f32                                 C
#   NT      3 bias + GELU, no aux_out                  C
#   NT      3 bias + GELU, aux_out = u                 C, aux_out
#   NT      4 bias + residual                          C
#   NN      0 store 16-bit                             C
#   NN      1 store f32                                C
#   NN      5 dGELU                                    C
#   NN      6 dGELU + column sums                      C, aux_out (partial rows sized by nv_gemm_tile_rows with the PADDED lda / ldb)
#   TN      1 store f32                                C
#   TN      1 accumulate                               C
#
# = 13 cases per family.  The three small-tile families also run the ten NT / NN cases other than epilogue 6 at K = 72, the ragged K
# plan_gemm sends to them (gemm.hip: k_ok) = 23 - 1: epilogue 6 has no small-tile kernel (gemm.hip, launch_fmt: "the fused column-sum
# epilogue needs a large-tile kernel"), at either K the call is refused: 22 run, 2 refused.  The six large-tile families are refused
# K = 72 by the plan (k_ok is false: nv_gemm_tile_rows answers 0 and the launch would go to a small-tile kernel, which the small-tile
# families cover): 13 run, 1 refused.  Under (11, 1) only the NT problems change kernel (gemm_pp.hip, launch_pp: g_pp_w32); its NN and
# TN cases rerun the (4, 0) kernels and are kept so that every family has one table.
M_G, N_G, K_G, K_RAGGED, K_TN = 264, 136, 128, 72, 200
TILES = {"small 64 x 64": ((64, 64),), "small 64 x 128": ((64, 128),), "small 128 x 128": ((128, 128),),
         "warp-specialised 128 x 128, 3 x 64": ((1, 1),), "warp-specialised 64 x 128, 3 x 64": ((3, 1),), "warp-specialised 64 x 128, 3 x 128": ((3, 3),),
         "ping-pong 256 x 128": ((4, 0),), "ping-pong 256 x 128 on 32 x 32 x 16": ((4, 0), (11, 1)), "256 x 256": ((9, 0),)}
TILE_ROWS = {"warp-specialised 128 x 128, 3 x 64": 128, "warp-specialised 64 x 128, 3 x 64": 64, "warp-specialised 64 x 128, 3 x 128": 64,
             "ping-pong 256 x 128": 256, "ping-pong 256 x 128 on 32 x 32 x 16": 256, "256 x 256": 128}         # plan_gemm's bm; small tiles: 0
PAD_A, PAD_B, PAD_F32, PAD_16 = 8, 16, 4, 8


@contextlib.contextmanager
def forced(lib, family):
    try:
        for bm, bn in TILES[family]:
            assert lib.nv_gemm_set_tile(bm, bn) == 0
        yield
    finally:
        lib.nv_gemm_set_tile(11, 0)
        lib.nv_gemm_set_tile(0, 0)


@pytest.fixture(scope="module")
def gemm_data():
    """layout / K -> device operands and the float64 product, computed once and shared read only"""
    cache = {}

    def get(layout, K):
        if (layout, K) not in cache:
            M, N = M_G, N_G
            if layout == "NT":
                A, B = bf(rnd(M, K, seed=1)), bf(rnd(N, K, seed=2, scale=K ** -0.5))
                ref = A.double() @ B.double().T
            elif layout == "NN":
                A, B = bf(rnd(M, K, seed=6)), bf(rnd(K, N, seed=7, scale=K ** -0.5))
                ref = A.double() @ B.double()
            else:
                A, B = bf(rnd(K, M, seed=9)), bf(rnd(K, N, seed=10, scale=K ** -0.5))
                ref = A.double().T @ B.double()
            cache[layout, K] = dev(A), dev(B), ref
        return cache[layout, K]
    extra = dict(bias=rnd(N_G, seed=3), resid=rnd(M_G, N_G, seed=4), u=bf(rnd(M_G, N_G, seed=8)), c0=rnd(M_G, N_G, seed=5))
    yield get, extra
    cache.clear()


def tile_rows(lib, layout, K, padded_lds, opsmod):
    """nv_gemm_tile_rows for the dense or the padded leading dimensions of a (264, 136, K) problem"""
    code = {"NT": opsmod.NT, "NN": opsmod.NN, "TN": opsmod.TN}[layout]
    wa, wb = {"NT": (K, K), "NN": (K, N_G), "TN": (M_G, N_G)}[layout]
    return lib.nv_gemm_tile_rows(code, M_G, N_G, K, wa + (PAD_A if padded_lds else 0), wb + (PAD_B if padded_lds else 0))


def gemm_cases(ops, lib, tl, get, extra, layouts, K, same_rows):
    """the table's cases of `layouts` at one K, under whatever tile is forced"""
    M, N = M_G, N_G
    f32, t16 = torch.float32, torch.bfloat16
    bias, resid, u, c0 = (extra[k] for k in ("bias", "resid", "u", "c0"))
    bd, rd, ud, c0d = dev(bias), dev(resid), dev(u), dev(c0)
    for layout in layouts:
        A, B, ref = get(layout, K)
        code = {"NT": ops.NT, "NN": ops.NN, "TN": ops.TN}[layout]
        rows_dense, rows_padded = tile_rows(lib, layout, K, False, ops), tile_rows(lib, layout, K, True, ops)
        assert rows_dense == rows_padded == same_rows, f"{tl.family}, {layout} K = {K}: the plan gives {rows_dense} tile rows for dense and {rows_padded} for padded lds, {same_rows} expected"
        ab = {"A": (A, PAD_A), "B": (B, PAD_B)}

        def case(name, epi, outs, gate, more=None, **kw):
            ins = dict(ab, **(more or {}))

            def call(i, o):
                ops.gemm(code, epi, i["A"], i["B"], out=o["C"], aux_in=i.get("aux_in"), aux_out=o.get("aux_out"), **kw)
            run_windows(tl, f"{layout} K = {K}, {name}", call, ins, outs, gate)

        if layout == "NT":
            uref = ref + bias.double()
            case("epilogue 0", ops.EPI_STORE_BF16, {"C": ((M, N), t16, PAD_16, None)}, lambda o: assert_close_bf16(o["C"], ref, "store_bf16"))
            case("epilogue 1", ops.EPI_STORE_F32, {"C": ((M, N), f32, PAD_F32, None)}, lambda o: assert_close_f32(o["C"], ref, "store_f32", 1e-5))

            def mirror(o):
                assert_close_f32(o["C"], ref, "store_f32", 1e-5)
                assert torch.equal(o["aux_out"], o["C"].to(t16)), "the 16-bit mirror is not the rounded fp32 store"
            case("epilogue 1 + mirror", ops.EPI_STORE_F32, {"C": ((M, N), f32, PAD_F32, None), "aux_out": ((M, N), t16, PAD_16, None)}, mirror)
            case("epilogue 2", ops.EPI_BIAS_F32, {"C": ((M, N), f32, PAD_F32, None)}, lambda o: assert_close_f32(o["C"], uref, "bias_f32", 1e-5), bias=bd)
            case("epilogue 3", ops.EPI_BIAS_GELU, {"C": ((M, N), t16, PAD_16, None)}, lambda o: assert_close_bf16(o["C"], F.gelu(uref), "gelu.h"), bias=bd)

            def gelu_u(o):
                assert_close_bf16(o["C"], F.gelu(uref), "gelu.h")
                assert_close_bf16(o["aux_out"], uref, "gelu.u")
            case("epilogue 3 + u", ops.EPI_BIAS_GELU, {"C": ((M, N), t16, PAD_16, None), "aux_out": ((M, N), t16, 16, None)}, gelu_u, bias=bd)
            case("epilogue 4", ops.EPI_BIAS_RESID, {"C": ((M, N), f32, PAD_F32, None)},
                 lambda o: assert_close_f32(o["C"], uref + resid.double(), "bias_resid", 1e-5), more={"aux_in": (rd, 12)}, bias=bd)
        elif layout == "NN":
            dref = ref * ref_cpu._gelu_grad(u.double())
            case("epilogue 0", ops.EPI_STORE_BF16, {"C": ((M, N), t16, PAD_16, None)}, lambda o: assert_close_bf16(o["C"], ref, "nn_bf16"))
            case("epilogue 1", ops.EPI_STORE_F32, {"C": ((M, N), f32, PAD_F32, None)}, lambda o: assert_close_f32(o["C"], ref, "nn_f32", 1e-5))
            case("epilogue 5", ops.EPI_DGELU, {"C": ((M, N), t16, PAD_16, None)}, lambda o: assert_close_bf16(o["C"], dref, "dgelu"), more={"aux_in": (ud, 4)})
            if same_rows == 0:
                part = torch.empty((M, N), device="cuda")
                refused(tl, "epilogue 6", lambda: ops.gemm(code, ops.EPI_DGELU_COLSUM, A, B, aux_in=ud, aux_out=part))
            else:
                def colsum(o):
                    assert_close_bf16(o["C"], dref, "dgelu")
                    assert_close_f32(o["aux_out"].sum(0), o["C"].double().sum(0), "colsum", 1e-5)
                prows = (M + rows_padded - 1) // rows_padded
                case("epilogue 6", ops.EPI_DGELU_COLSUM, {"C": ((M, N), t16, PAD_16, None), "aux_out": ((prows, N), f32, 12, None)}, colsum, more={"aux_in": (ud, 4)})
        else:
            case("epilogue 1", ops.EPI_STORE_F32, {"C": ((M, N), f32, PAD_F32, None)}, lambda o: assert_close_f32(o["C"], ref, "tn_f32", 1e-5))
            case("epilogue 1, accumulate", ops.EPI_STORE_F32, {"C": ((M, N), f32, PAD_F32, c0d)},
                 lambda o: assert_close_f32(o["C"], ref + c0.double(), "tn accumulate", 1e-5), accumulate=True)


@pytest.mark.parametrize("family", list(TILES))
def test_gemm_honours_every_leading_dimension(ops, lib, gemm_data, family):
    get, extra = gemm_data
    tl = Tally(f"nv_gemm_bf16, {family}")
    small = family.startswith("small")
    with forced(lib, family):
        gemm_cases(ops, lib, tl, get, extra, ("NT", "NN"), K_G, 0 if small else TILE_ROWS[family])
        gemm_cases(ops, lib, tl, get, extra, ("TN",), K_TN, 0 if small else TILE_ROWS[family])
        if small:
            gemm_cases(ops, lib, tl, get, extra, ("NT", "NN"), K_RAGGED, 0)
        else:                       # gemm.hip, plan_gemm: k_ok = (K % BK == 0) || (A_T && B_T) - no large tile takes a ragged K of K-contiguous operands
            for layout in ("NT", "NN"):
                assert tile_rows(lib, layout, K_RAGGED, False, ops) == 0 and tile_rows(lib, layout, K_RAGGED, True, ops) == 0
            tl.refused += 1
    tl.done(*((22, 2) if small else (13, 1)))


# grouped weight gradients, stochastic depth, LayerNorm folded into the GEMMs
#
#   nv_gemm_bf16_grouped   two TN problems in one launch - (Mo, N, K) = (264, 136, 200) stored with a 16-bit mirror, (72, 264, 200)
#                          accumulated - lda, ldb, ldc, ldc16 padded; on the ping-pong tiles (default) and the warp-specialised ones
#                          ((3, 1): gemm.hip, grouped_tn_impl)                                                        2 cases
#   nv_gemm_bf16_path      NT epilogue 4 with factors (1, 0, 1.25, 0.5) over 66-row samples, every tile family        9 cases
#   nv_gemm_resid_ln,      (M, d) = (449, 768): the fewest rows nv_gemm_lnfold_supported admits at the model width without a forced tile
#   nv_gemm_lnfold         (gemm.hip, plan_gemm: 48 tiles of 64 x 128; 448 rows are refused, asserted) - heuristic, (1, 1), (3, 1), (3, 3),
#                          (4, 0); (9, 0) is refused: gemm.hip, launch_fold_fmt has no 256 x 256 kernel.  Three launches each
#                          (producer, consumer, consumer + GELU): 15 run, 3 refused (the small-tile and 256 x 256 plans)
def test_grouped_gemm_honours_every_leading_dimension(ops, lib):
    tl = Tally("nv_gemm_bf16_grouped")
    K = K_TN
    shapes = [(M_G, N_G), (72, M_G)]
    A = [dev(bf(rnd(K, mo, seed=20 + i))) for i, (mo, n) in enumerate(shapes)]
    B = [dev(bf(rnd(K, n, seed=30 + i, scale=K ** -0.5))) for i, (mo, n) in enumerate(shapes)]
    c1 = dev(rnd(*shapes[1], seed=41))
    refs = [A[0].cpu().double().T @ B[0].cpu().double(), A[1].cpu().double().T @ B[1].cpu().double() + c1.cpu().double()]
    ins = {"A0": (A[0], 8), "B0": (B[0], 16), "A1": (A[1], 16), "B1": (B[1], 8)}
    outs = {"C0": (shapes[0], torch.float32, 4, None), "C16": (shapes[0], torch.bfloat16, 8, None), "C1": (shapes[1], torch.float32, 12, c1)}

    def call(i, o):
        ops.gemm_tn_grouped([(i["A0"], i["B0"], o["C0"], False, o["C16"]), (i["A1"], i["B1"], o["C1"], True)])

    def gate(o):
        assert_close_f32(o["C0"], refs[0], "grouped store", 1e-5)
        assert_close_f32(o["C1"], refs[1], "grouped accumulate", 1e-5)
        assert torch.equal(o["C16"], o["C0"].to(torch.bfloat16))
    for family in ("ping-pong 256 x 128", "warp-specialised 64 x 128, 3 x 64"):
        with forced(lib, family):
            run_windows(tl, family, call, ins, outs, gate)
    tl.done(2, 0)


def test_gemm_path_epilogue_honours_every_leading_dimension(ops, lib, gemm_data):
    get, extra = gemm_data
    tl = Tally("nv_gemm_bf16_path")
    A, B, ref = get("NT", K_G)
    table, rows = torch.tensor([1.0, 0.0, 1.25, 0.5]), 66
    want = extra["resid"].double() + (ref + extra["bias"].double()) * table.double()[torch.arange(M_G) // rows][:, None]
    bd, td = dev(extra["bias"]), dev(table)

    def call(i, o):
        ops.gemm(ops.NT, ops.EPI_BIAS_RESID, i["A"], i["B"], out=o["C"], bias=bd, aux_in=i["aux_in"], path=td, path_rows=rows)
    for family in TILES:
        with forced(lib, family):
            run_windows(tl, family, call, {"A": (A, PAD_A), "B": (B, PAD_B), "aux_in": (dev(extra["resid"]), 12)}, {"C": ((M_G, N_G), torch.float32, PAD_F32, None)},
                        lambda o: assert_close_f32(o["C"], want, "path", 1e-5))
    tl.done(len(TILES), 0)


FOLD_M, FOLD_D, FOLD_K, FOLD_N = 449, 768, 128, 648


def test_folded_layernorm_gemms_honour_every_leading_dimension(ops, lib):
    from test_kernels_gpu import _fold_reference
    tl = Tally("nv_gemm_resid_ln / nv_gemm_lnfold")
    M, d, K, N = FOLD_M, FOLD_D, FOLD_K, FOLD_N
    assert lib.nv_gemm_lnfold_supported(M, d, K) == 1 and lib.nv_gemm_lnfold_supported(M, N, d) == 1
    assert lib.nv_gemm_lnfold_supported(M - 1, d, K) == 0                    # one row fewer: 7 x 6 tiles of 64 x 128, below plan_gemm's 48
    A, Wp, bp = dev(bf(rnd(M, K, seed=1))), dev(bf(rnd(d, K, seed=2, scale=K ** -0.5))), rnd(d, seed=3)
    resid = rnd(M, d, seed=4) * 2 + 0.5 * rnd(M, 1, seed=5)
    x = resid.double() + A.cpu().double() @ Wp.cpu().double().T + bp.double()
    gamma, beta = 1 + 0.1 * rnd(d, seed=6), 0.1 * rnd(d, seed=7)
    Wc, bc = rnd(N, d, seed=8, scale=d ** -0.5), 0.1 * rnd(N, seed=9)
    bpd, nstat = dev(bp), lib.nv_ln_fold_stats_floats(M, d)
    folded = {gelu: ops.ln_fold_weight(dev(Wc), dev(gamma), dev(beta), dev(bc) if gelu else None) for gelu in (False, True)}
    for family in (None, "warp-specialised 128 x 128, 3 x 64", "warp-specialised 64 x 128, 3 x 64", "warp-specialised 64 x 128, 3 x 128", "ping-pong 256 x 128",
                   "256 x 256", "small 64 x 64", "small 128 x 128"):
        with (forced(lib, family) if family else contextlib.nullcontext()):
            name = family or "heuristic"
            if family in ("256 x 256", "small 64 x 64", "small 128 x 128"):
                assert lib.nv_gemm_lnfold_supported(M, d, K) == 0
                refused(tl, name, lambda: ops.gemm_resid_ln(A, Wp, bpd, dev(resid)))
                continue

            def produce(i, o):
                ops.gemm_resid_ln(i["A"], i["W"], bpd, i["resid"], out=o["out"], out16=o["out16"], stats=o["stats"])

            def gate(o):
                assert_close_f32(o["out"], x, "resid_ln.out", 1e-5)
                assert torch.equal(o["out16"], o["out"].to(torch.bfloat16))
            prod = run_windows(tl, f"{name}, producer", produce, {"A": (A, 8), "W": (Wp, 16), "resid": (dev(resid), 12)},
                               {"out": ((M, d), torch.float32, 4, None), "out16": ((M, d), torch.bfloat16, 8, None), "stats": ((nstat,), torch.float32, 0, None)}, gate)
            for gelu in (False, True):
                Wg, cs, fb = folded[gelu]
                want = _fold_reference(prod["out"].cpu(), gamma, beta, Wc, bc if gelu else None, gelu)

                def consume(i, o):
                    ops.gemm_lnfold(i["X"], i["Wg"], prod["stats"], cs, fb, gelu=gelu, out=o["y"])

                def gate_y(o):          # the gate of test_layernorm_folded_into_the_gemms_around_it
                    assert rel_l2(o["y"].float(), want) <= 4e-3 and float((o["y"].float().cpu().double() - want).abs().max() / want.abs().max()) <= 2.0 ** -6
                run_windows(tl, f"{name}, consumer{' + GELU' if gelu else ''}", consume, {"X": (prod["out16"], 8), "Wg": (Wg, 16)},
                            {"y": ((M, N), torch.bfloat16, 8, None)}, gate_y)
    tl.done(15, 3)


# ------------------------------------------------------------------------------------------------------------ LayerNorm
# nv_ln_fwd, nv_ln_bwd, nv_ln_bwd_path at (M, d) in LN_SHAPES; ldx + 4, ldy + 8, lddy + 8, ldg + 12, ldg16 + 16.  Per shape:
#
#   nv_ln_fwd                                        y, mean, rstd                                     run
#   nv_ln_bwd   g_in given, g_out another buffer     g_out, g16, dgamma, dbeta, dcolsum                run
#   nv_ln_bwd   g_in null                            g_out, g16, dgamma, dbeta, dcolsum                run
#   nv_ln_bwd   in place (g_out is g_in)             g, g16, dgamma, dbeta, dcolsum                    run
#   nv_ln_bwd   dropout 0.25, ldg = 2 d              rows [::2] of a dense [2 M, d] g; g16 padded      run   (against rows [::2] of the dense [2 M, d] run)
#   nv_ln_bwd_path  dropout 0.25 + factors, ldg = 2 d   the same                                       run
#   nv_ln_bwd   dropout, ldg = d + 12                refused: norm.hip, ln_bwd_launch, "with dropout g must be a (row-strided) view of a dense [*, d] tensor"
#   nv_ln_bwd_path  ldg = d + 12                     refused: norm.hip, ln_bwd_launch, "nv_ln_bwd_path: ... (ldg a multiple of d)"
#
# = 6 run, 2 refused per shape.  d <= 1024 and d = 2048 are the two instantiations of ln_bwd_kernel.
LN_SHAPES = [(65, 192), (130, 128), (67, 768), (9, 1024), (33, 2048)]
LN_P = 0.25


def ln_reference(x, gamma, beta, dy, g_in):
    """float64: (y, mean, rstd, dx + g_in, dgamma, dbeta)"""
    d = x.shape[1]
    xd = x.double().requires_grad_(True)
    gd, bd = gamma.double().requires_grad_(True), beta.double().requires_grad_(True)
    y = F.layer_norm(xd, (d,), gd, bd, 1e-5)
    y.backward(dy.double())
    return y.detach(), x.double().mean(1), 1 / torch.sqrt(x.double().var(1, unbiased=False) + 1e-5), xd.grad + g_in.double(), gd.grad, bd.grad


def ln_forward_case(ops, tl, x, gamma, beta, what=""):
    M, d = x.shape
    want = ln_reference(x, gamma, beta, torch.zeros_like(x), torch.zeros_like(x))
    gm, bt = dev(gamma), dev(beta)

    def gate(o):
        assert_close_bf16(o["y"], want[0], "ln_fwd")
        assert_close_f32(o["mean"], want[1], "mean", 1e-5)
        assert_close_f32(o["rstd"], want[2], "rstd", 1e-5)
    run_windows(tl, f"nv_ln_fwd [{M}, {d}]{what}", lambda i, o: ops.ln_fwd(i["x"], gm, bt, y=o["y"], st=(o["mean"], o["rstd"])), {"x": (dev(x), 4)},
                {"y": ((M, d), ops.op16(), 8, None), "mean": ((M,), torch.float32, 0, None), "rstd": ((M,), torch.float32, 0, None)}, gate)


def ln_backward_cases(ops, tl, x, gamma, beta, dy, g_in, forms=("given", "null", "in place")):
    M, d = x.shape
    f32 = torch.float32
    gm = dev(gamma)
    _, st = ops.ln_fwd(dev(x), gm, dev(beta))
    ins = {"dy": (dev(dy), 8), "x": (dev(x), 4)}
    vec = {k: ((d,), f32, 0, None) for k in ("dgamma", "dbeta", "dcolsum")}
    for form in forms:
        base = g_in if form != "null" else torch.zeros_like(g_in)
        _, _, _, g_want, dg_want, db_want = ln_reference(x, gamma, beta, dy, base)

        def gate(o):
            assert_close_f32(o["g"], g_want, "ln_bwd.dx", 1e-5)
            assert_close_bf16(o["g16"], g_want, "ln_bwd.g16")
            assert_close_f32(o["dgamma"], dg_want, "ln_bwd.dgamma", 1e-5)
            assert_close_f32(o["dbeta"], db_want, "ln_bwd.dbeta", 1e-5)
            assert_close_f32(o["dcolsum"], g_want.sum(0), "ln_bwd.colsum", 1e-5)

        def call(i, o):
            g_arg = {"given": i.get("g_in"), "null": None, "in place": o["g"]}[form]
            ops.ln_bwd(i["dy"], i["x"], st, gm, g_in=g_arg, g_out=o["g"], g16=o["g16"], dgamma=o["dgamma"], dbeta=o["dbeta"], dcolsum=o["dcolsum"])
        more = {"g_in": (dev(g_in), 12)} if form == "given" else {}
        outs = dict({"g": ((M, d), f32, 12, dev(g_in) if form == "in place" else None), "g16": ((M, d), ops.op16(), 16, None)}, **vec)
        run_windows(tl, f"nv_ln_bwd [{M}, {d}], g_in {form}", call, dict(ins, **more), outs, gate)


def ln_strided_case(ops, tl, M, d, with_path):
    """rows [::2] of a dense [2 M, d] problem (ldg = 2 d) under dropout (and stochastic-depth factors): the launch rows take the masks and
    factors of the dense rows, so g and g16 must be rows [::2] of the dense [2 M, d] run, word for word; the rows in between stay as they were"""
    M2, f32 = 2 * M, torch.float32
    x, gamma, beta = rnd(M2, d, seed=11) * 2 + 0.3, 1 + 0.1 * rnd(d, seed=12), 0.1 * rnd(d, seed=13)
    dy, g_in = rnd(M2, d, seed=14), rnd(M2, d, seed=15)
    rows = 9
    table = torch.tensor([1.0, 1.25, 0.0, 1.75, 0.5])[torch.arange((M2 + rows - 1) // rows) % 5]
    kw = dict(drop_seed=SEED, drop_p=LN_P, **(dict(path=dev(table), path_rows=rows) if with_path else {}))
    gm = dev(gamma)
    _, st = ops.ln_fwd(dev(x), gm, dev(beta))
    dense_g, dense_g16, _, _, _ = ops.ln_bwd(dev(dy), dev(x), st, gm, g_in=dev(g_in), **kw)
    torch.cuda.synchronize()
    _, _, _, g_want, _, _ = ln_reference(x, gamma, beta, dy, g_in)
    factor = ref_cpu.drop_mask(SEED, LN_P, (M2, d)).double() * (table.double()[torch.arange(M2) // rows][:, None] if with_path else 1.0)
    assert_close_f32(dense_g, g_want, "ln_bwd.dx", 1e-5)                                                 # (a)
    assert_close_bf16(dense_g16, g_want * factor, "ln_bwd.g16")
    xs, dys, sts = x[::2], dy[::2], st[:, ::2].contiguous()
    _, _, _, _, dg_want, db_want = ln_reference(xs, gamma, beta, dys, g_in[::2])
    name = f"{'nv_ln_bwd_path' if with_path else 'nv_ln_bwd'} [{M}, {d}], dropout, ldg = 2 d"
    got = {}
    for wrap in (into_padded, into_poisoned):
        g = dev(g_in)
        if wrap is into_poisoned:
            g[1::2] = float("nan")
        before = g.clone()
        (g16, b16), vecs = padded(M, d, ops.op16(), 16), [guarded(d) for _ in range(3)]
        i_dy, i_x = wrap(dev(dys.contiguous()), 8), wrap(dev(xs.contiguous()), 4)
        assert g[::2].stride(0) == 2 * d and g16.stride(0) == d + 16 and i_dy.stride(0) == d + 8 and i_x.stride(0) == d + 4
        ops.ln_bwd(i_dy, i_x, sts, gm, g_in=g[::2], g16=g16, dgamma=vecs[0][0], dbeta=vecs[1][0], dcolsum=vecs[2][0], **kw)
        torch.cuda.synchronize()
        assert same_window_bits(g[::2], dense_g[::2]) == 0, f"{name}: g differs from rows [::2] of the dense run"            # (b)
        assert same_window_bits(g16, dense_g16[::2]) == 0, f"{name}: g16 differs from rows [::2] of the dense run"
        assert same_window_bits(g[1::2], before[1::2]) == 0, f"{name}: wrote the rows between its rows"                       # (c)
        assert guards_intact(g16, b16) and all(guards_intact(v, b) for v, b in vecs), f"{name}: wrote outside a window"
        assert_close_f32(vecs[0][0], dg_want, "ln_bwd.dgamma", 1e-5)
        assert_close_f32(vecs[1][0], db_want, "ln_bwd.dbeta", 1e-5)
        got[wrap] = [v.clone() for v, _ in vecs]
    for a, b in zip(got[into_padded], got[into_poisoned]):                                               # (d)
        assert same_window_bits(a, b) == 0 and not torch.isnan(b).any(), f"{name}: the column sums change with what the inputs' pad cells hold"
    tl.ran += 1
    # a padded ldg is no view of a dense [*, d] tensor: the launcher refuses it
    xs_d, dys_d = dev(xs.contiguous()), dev(dys.contiguous())
    gp = into_padded(dev(g_in[::2].contiguous()), 12)
    refused(tl, name, lambda: ops.ln_bwd(dys_d, xs_d, sts, gm, g_in=gp, **(dict(path=dev(table), path_rows=rows) if with_path else dict(drop_seed=SEED, drop_p=LN_P))))


@pytest.mark.parametrize("M,d", LN_SHAPES)
def test_layernorm_honours_every_leading_dimension(ops, M, d):
    tl = Tally(f"nv_ln_fwd / nv_ln_bwd / nv_ln_bwd_path [{M}, {d}]")
    x, gamma, beta = rnd(M, d, seed=1) * 2 + 0.3, 1 + 0.1 * rnd(d, seed=2), 0.1 * rnd(d, seed=3)
    dy, g_in = rnd(M, d, seed=4), rnd(M, d, seed=5)
    ln_forward_case(ops, tl, x, gamma, beta)
    ln_backward_cases(ops, tl, x, gamma, beta, dy, g_in)
    ln_strided_case(ops, tl, M, d, with_path=False)
    ln_strided_case(ops, tl, M, d, with_path=True)
    tl.done(6, 2)


# ------------------------------------------------------------------------------------------------------------ attention
# nv_attn_fwd, nv_attn_bwd; qkv ld + 8, out / dout ld + 8 (one ld_out for both: include/neurovit_hip.h), dqkv ld + 4, lse and delta
# guarded.  dim_head 64: nv_attn_set_mode 1 (streaming), 2 (LDS-resident), 3 (wide streaming), 22 (resident forward, two partner
# waves), 102 (resident backward as one launch) x (B, n, heads) in (2, 65, 2), (2, 130, 1) x dropout 0, 0.1 x (forward, backward)
# = 40 cases; B = 2 because the keys past n in the first sample's last tile are the second sample's rows.  The generic kernels
# (attention_generic.hip) at dim_head 32 and 128, (1, 37, 2), dropout 0 and 0.1, forward and backward = 8 cases.  None refused.
# Reference: the oracle's flash restatement with the kernels' cast points (ref_cpu._AttnEmu) at assert_close_stat for dim_head 64 and
# the fp64 softmax at rel_l2 4e-3 / 6e-3 for the generic kernels - what tests/test_kernels_gpu.py holds these kernels to.
ATTN_MODES = (1, 2, 3, 22, 102)
ATTN_SHAPES = [(2, 65, 2), (2, 130, 1)]
ATTN_DROPS = (0.0, 0.1)


@pytest.fixture(scope="module")
def attn_data():
    """(B, n, heads, dh, drop, fmt) -> inputs and references, computed once and shared read only"""
    cache = {}

    def get(B, n, heads, dh, drop, fmt="bf16"):
        key = (B, n, heads, dh, drop, fmt)
        if key not in cache:
            t16 = {"bf16": torch.bfloat16, "fp16": torch.float16}[fmt]
            inner = heads * dh
            qkv = rnd(B * n, 3 * inner, seed=n + dh).to(t16).float()
            do = rnd(B * n, inner, seed=7).to(t16).float()
            mask = ref_cpu.attn_drop_mask(SEED, drop, B, heads, n) if drop else None
            split = lambda t: t.reshape(B, n, heads, dh).permute(0, 2, 1, 3)
            join = lambda t: t.permute(0, 2, 1, 3).reshape(B * n, inner)
            if dh == 64:
                q, k, v = (split(t).clone().requires_grad_(True) for t in qkv.chunk(3, dim=-1))
                with ref_cpu.operand_format(fmt):
                    ref = ref_cpu._AttnEmu.apply(q, k, v, dh ** -0.5, mask)
                    ref.backward(split(do))
                out_ref = join(ref.detach())
                out_fed = out_ref.to(t16)                    # the backward reads the oracle's own 16-bit output: both sides form the same delta
            else:
                q, k, v = (split(t).double().clone().requires_grad_(True) for t in qkv.chunk(3, dim=-1))
                pr = torch.softmax(torch.matmul(q, k.transpose(-1, -2)) * dh ** -0.5, dim=-1)
                ref = torch.matmul(pr if mask is None else pr * mask.double(), v)
                out_ref = join(ref.detach())
                out_fed = out_ref.to(t16)
                # the kernel's delta is formed from the 16-bit output it is given: restate the backward with that delta
                dO = split(do).double()
                delta = (dO * split(out_fed.float()).double()).sum(-1, keepdim=True)
                mk = 1.0 if mask is None else mask.double()
                dv = torch.matmul((pr * mk).transpose(-1, -2), dO)
                ds = pr * (torch.matmul(dO, v.transpose(-1, -2)) * mk - delta)
                q.grad, k.grad, v.grad = torch.matmul(ds, k) * dh ** -0.5, torch.matmul(ds.transpose(-1, -2), q) * dh ** -0.5, dv
            s = torch.matmul(q.detach().double(), k.detach().double().transpose(-1, -2)) * dh ** -0.5
            cache[key] = dict(qkv=dev(qkv.to(t16)), do=dev(do.to(t16)), out_fed=dev(out_fed), out_ref=out_ref, lse_ref=torch.logsumexp(s, dim=-1).reshape(-1),
                              dqkv_ref=torch.cat([join(t.grad.detach()) for t in (q, k, v)], dim=-1),
                              delta_ref=(split(do).double() * split(out_fed.float()).double()).sum(-1).reshape(-1))
        return cache[key]
    yield get
    cache.clear()


def attention_cases(ops, tl, D, B, n, heads, dh, drop, what):
    inner, f32 = heads * dh, torch.float32
    kw = dict(drop_seed=SEED if drop else 0, drop_p=drop)

    def gate_fwd(o):
        if dh == 64:
            assert_close_stat(o["out"], D["out_ref"], "attn.out")
        else:
            assert rel_l2(o["out"].float(), D["out_ref"]) < 4e-3
        assert_close_f32(o["lse"], D["lse_ref"], "attn.lse", 1e-4)
    fwd = run_windows(tl, f"nv_attn_fwd {what}", lambda i, o: ops.attn_fwd(i["qkv"], B, n, heads, dh, out=o["out"], lse=o["lse"], **kw), {"qkv": (D["qkv"], 8)},
                      {"out": ((B * n, inner), ops.op16(), 8, None), "lse": ((B * heads * n,), f32, 0, None)}, gate_fwd)

    def gate_bwd(o):
        if dh == 64:
            assert_close_stat(o["dqkv"], D["dqkv_ref"], "attn.dqkv")
        else:
            for lo in (0, inner, 2 * inner):
                assert rel_l2(o["dqkv"][:, lo:lo + inner].float(), D["dqkv_ref"][:, lo:lo + inner]) < 6e-3
        assert_close_f32(o["delta"], D["delta_ref"], "attn.delta", 1e-4)
    lse = fwd["lse"]
    run_windows(tl, f"nv_attn_bwd {what}", lambda i, o: ops.attn_bwd(i["qkv"], i["out"], i["dout"], lse, B, n, heads, dh, dqkv=o["dqkv"], delta=o["delta"], **kw),
                {"qkv": (D["qkv"], 8), "out": (D["out_fed"], 8), "dout": (D["do"], 8)},
                {"dqkv": ((B * n, 3 * inner), ops.op16(), 4, None), "delta": ((B * heads * n,), f32, 0, None)}, gate_bwd)


@pytest.mark.parametrize("mode", ATTN_MODES)
def test_attention_honours_every_leading_dimension(ops, lib, attn_data, mode):
    tl = Tally(f"nv_attn_fwd / nv_attn_bwd, dim_head 64, mode {mode}")
    try:
        assert lib.nv_attn_set_mode(mode) == 0
        for B, n, heads in ATTN_SHAPES:
            for drop in ATTN_DROPS:
                attention_cases(ops, tl, attn_data(B, n, heads, 64, drop), B, n, heads, 64, drop, f"({B}, {n}, {heads}) dropout {drop}")
    finally:
        lib.nv_attn_set_mode(0)
    tl.done(8, 0)


@pytest.mark.parametrize("dh", [32, 128])
def test_generic_attention_honours_every_leading_dimension(ops, attn_data, dh):
    tl = Tally(f"nv_attn_fwd / nv_attn_bwd, dim_head {dh}")
    B, n, heads = 1, 37, 2
    for drop in ATTN_DROPS:
        attention_cases(ops, tl, attn_data(B, n, heads, dh, drop), B, n, heads, dh, drop, f"({B}, {n}, {heads}) dropout {drop}")
    tl.done(4, 0)


# ------------------------------------------------------------------------------------------------------------ front end and embed
# S, p = 32, 8 (P = 512 = Ppad, 64 tokens per volume, B = 2); the volume itself is a strided view: the [B, S, S, S] corner of a
# [B, S + 1, S + 1, S + 4] buffer whose other cells are the sentinel, then NaN.
#
#   nv_patch_ln_fwd      gather (nv_patch_set_mode 0), ldo = Ppad + 8      another kernel: norm.hip, patch_vec_ok needs ldo == P, so a padded
#   nv_patch_ln_fwd      slabs  (nv_patch_set_mode 2), ldo = Ppad + 8      ldo takes the scalar gather in BOTH modes (the slabs need `vec` too:
#   nv_patch_ln_fwd_f32  gather, ldo = P + 4                               patch_ln_fwd_launch) - held to the float64 gate.  Columns P .. ldo-1
#   nv_patch_ln_fwd_f32  slabs,  ldo = P + 4                               are WRITTEN AS ZERO (the comment above patch_ln_fwd_launch); rows above / below untouched
#   nv_patch_ln_fwd_4d       ldo = P + 8    [1, 16, 16, 16, 4], p = 8: the same kernel for every ldo - bits of the dense run; columns P .. ldo-1
#   nv_patch_ln_fwd_4d_f32   ldo = P + 4    are left as they were (include/neurovit_hip.h says so now).  x is contiguous by contract: no pad cells to poison
#   nv_patch_ln_bwd      ldd = P + 8, NaN in the pad columns of dxp          dgamma, dbeta guarded
#   nv_patch_ln_dx       ldd = P + 8, NaN in the pad columns of dxp          dvideo a strided view of a sentinel buffer
#   nv_embed_finish_fwd  ldt + 8, ldx + 4; dropout 0 and 0.25                x, mean, rstd
#   nv_embed_finish_bwd  ldg + 12, ldt + 8, lddt + 4, lddt16 + 8: full and data-only (the five parameter gradients NULL), dropout 0
#   nv_embed_finish_bwd  dropout 0.25: ldg == d, everything else padded, full and data-only
#   nv_embed_finish_bwd  dropout 0.25, ldg = d + 12                          refused: norm.hip, "nv_embed_finish_bwd: dropout needs a dense g"
#
# = 8 run (patch), 6 run + 1 refused (embed).
def volume_views(vol):
    """the dense device volume, and the same cells as a corner of a larger sentinel / NaN buffer (its strides stay multiples of four floats)"""
    B, S = vol.shape[0], vol.shape[1]
    views = {"dense": dev(vol)}
    for name, byte in (("padded", 0xA5), ("poisoned", 0xFF)):
        big = torch.full((B, S + 1, S + 1, (S + 4) * 4), byte, dtype=torch.uint8, device="cuda").view(torch.float32)
        assert big.shape == (B, S + 1, S + 1, S + 4) and bool(torch.isnan(big).all()) == (byte == 0xFF)
        big[:, :S, :S, :S] = dev(vol)
        views[name] = big[:, :S, :S, :S]
    return views


def test_patch_front_end_honours_every_leading_dimension(ops, lib):
    tl = Tally("nv_patch_ln_fwd / _f32 / _4d / _4d_f32 / nv_patch_ln_bwd / nv_patch_ln_dx")
    S, p, B = 32, 8, 2
    P, f32 = p ** 3, torch.float32
    g = torch.Generator().manual_seed(S + p)
    vol = torch.randn(B, S, S, S, generator=g) * 3.0 + 1.5
    gamma, beta = 1 + 0.1 * rnd(P, seed=1), 0.1 * rnd(P, seed=2)
    gm, bt = dev(gamma), dev(beta)
    vols = volume_views(vol)
    video = {k: ref_cpu.fmri_to_video(v) for k, v in vols.items()}
    tok = ref_cpu.patchify(ref_cpu.fmri_to_video(vol), p, p, p).reshape(-1, P).double()
    rows = tok.shape[0]
    want = F.layer_norm(tok, (P,), gamma.double(), beta.double(), 1e-5)
    mean_want, rstd_want = tok.mean(1), 1 / torch.sqrt(tok.var(1, unbiased=False) + 1e-5)

    def gate_tokens(out, st, is32):
        (assert_close_f32(out, want, "patch_ln", 1e-5) if is32 else assert_close_bf16(out, want, "patch_ln"))
        assert_close_f32(st[0], mean_want, "patch_ln.mean", 1e-5)
        assert_close_f32(st[1], rstd_want, "patch_ln.rstd", 1e-5)
    for is32, pad in ((False, 8), (True, 4)):
        fwd = ops.patch_ln_fwd_f32 if is32 else ops.patch_ln_fwd
        odt = f32 if is32 else ops.op16()
        for mode in (0, 2):
            lib.nv_patch_set_mode(mode)
            try:
                out, st = fwd(video["dense"], p, p, p, gm, bt)
                torch.cuda.synchronize()
                gate_tokens(out[:, :P], st, is32)                                                    # (a): the vector gather (mode 0) / the slabs (mode 2)
                got = {}
                for which in ("padded", "poisoned"):
                    (win, buf), (mean, bm), (rstd, br) = padded(rows, P + pad, odt, 0), guarded(rows), guarded(rows)
                    assert win.stride(0) == P + pad and video[which].stride() != video["dense"].stride()
                    fwd(video[which], p, p, p, gm, bt, out=win[:, :P] if is32 else win, st=(mean, rstd))        # ldo = the view's row stride
                    torch.cuda.synchronize()
                    gate_tokens(win[:, :P].contiguous(), (mean, rstd), is32)                         # (b): the scalar gather - float64 gate
                    assert torch.count_nonzero(win[:, P:]) == 0, "columns P .. ldo-1 are documented to be written as zero"
                    assert guards_intact(win, buf) and guards_intact(mean, bm) and guards_intact(rstd, br)          # (c)
                    got[which] = (win.clone(), mean.clone(), rstd.clone())
                for a, b in zip(got["padded"], got["poisoned"]):                                     # (d)
                    assert same_window_bits(a, b) == 0 and not torch.isnan(b.float()).any()
            finally:
                lib.nv_patch_set_mode(0)
            tl.ran += 1
    # ---- 4D: every ldo runs the one kernel
    S4, T4 = 16, 4
    x4 = torch.randn(1, S4, S4, S4, T4, generator=g) * 1.5 + 0.3
    tok4 = ref_cpu.patchify(ref_cpu.fmri_to_video(x4.permute(0, 4, 1, 2, 3).reshape(T4, S4, S4, S4)), p, p, p).reshape(-1, P).double()
    want4 = F.layer_norm(tok4, (P,), gamma.double(), beta.double(), 1e-5)
    rows4 = tok4.shape[0]
    for is32, pad in ((False, 8), (True, 4)):
        odt = f32 if is32 else ops.op16()
        dense, st = ops.patch_ln_fwd_4d(dev(x4), p, p, p, gm, bt, f32=is32)
        torch.cuda.synchronize()
        (assert_close_f32(dense, want4, "patch_ln_4d", 1e-5) if is32 else assert_close_bf16(dense, want4, "patch_ln_4d"))
        assert_close_f32(st[0], tok4.mean(1), "patch_ln_4d.mean", 1e-5)
        assert_close_f32(st[1], 1 / torch.sqrt(tok4.var(1, unbiased=False) + 1e-5), "patch_ln_4d.rstd", 1e-5)
        (win, buf), (mean, bm), (rstd, br) = padded(rows4, P, odt, pad), guarded(rows4), guarded(rows4)
        assert win.stride(0) == P + pad
        ops.patch_ln_fwd_4d(dev(x4), p, p, p, gm, bt, out=win, st=(mean, rstd), f32=is32)
        torch.cuda.synchronize()
        assert same_window_bits(win, dense) == 0 and same_window_bits(mean, st[0]) == 0 and same_window_bits(rstd, st[1]) == 0
        assert guards_intact(win, buf), "nv_patch_ln_fwd_4d leaves the columns P .. ldo-1 and the rows around its window as they were"
        assert guards_intact(mean, bm) and guards_intact(rstd, br)
        tl.ran += 1
    # ---- backward: parameter gradients and the gradient with respect to the volume, dxp with NaN pad columns
    _, st = ops.patch_ln_fwd(video["dense"], p, p, p, gm, bt)
    dxp = rnd(rows, P, seed=4)
    vd = vol.double().requires_grad_(True)
    gd, bd = gamma.double().requires_grad_(True), beta.double().requires_grad_(True)
    F.layer_norm(ref_cpu.patchify(ref_cpu.fmri_to_video(vd), p, p, p).reshape(-1, P), (P,), gd, bd, 1e-5).backward(dxp.double())
    dg, db = ops.patch_ln_bwd(video["dense"], p, p, p, dev(dxp), st)
    dvol = torch.empty((B, S, S, S), device="cuda")           # in the volume's own layout, as the padded runs: the launcher takes its float4 kernel only
    ops.patch_ln_dx(video["dense"], p, p, p, dev(dxp), st, gm, dvideo=ref_cpu.fmri_to_video(dvol))      # when BOTH views have contiguous frames (norm.hip, nv_patch_ln_dx: vec)
    torch.cuda.synchronize()
    assert_close_f32(dg, gd.grad, "patch_ln.dgamma", 1e-4)                                          # tests/test_kernels_gpu.py::test_patch_ln_fwd_bwd_general
    assert_close_f32(db, bd.grad, "patch_ln.dbeta", 1e-4)
    assert_close_f32(dvol, vd.grad, "patch_ln.dvideo", 1e-5)
    got = {}
    for which, wrap in (("padded", into_padded), ("poisoned", into_poisoned)):
        dx_in = wrap(dev(dxp), 8)
        (dgw, b0), (dbw, b1) = guarded(P), guarded(P)
        assert dx_in.stride(0) == P + 8
        ops.patch_ln_bwd(video[which], p, p, p, dx_in, st, dgamma=dgw, dbeta=dbw)
        big = torch.full((B, S + 1, S + 1, S + 4, 4), 0xA5, dtype=torch.uint8, device="cuda")
        dwin = big.view(torch.float32).reshape(B, S + 1, S + 1, S + 4)[:, :S, :S, :S]
        ops.patch_ln_dx(video[which], p, p, p, dx_in, st, gm, dvideo=ref_cpu.fmri_to_video(dwin))
        torch.cuda.synchronize()
        assert same_window_bits(dgw, dg) == 0 and same_window_bits(dbw, db) == 0 and same_window_bits(dwin, dvol) == 0, which
        assert guards_intact(dgw, b0) and guards_intact(dbw, b1)
        outside = big.clone()
        outside[:, :S, :S, :S] = 0xA5
        assert bool((outside == 0xA5).all()), "nv_patch_ln_dx wrote outside the volume's cells"
        got[which] = (dgw.clone(), dbw.clone(), dwin.clone())
    for a, b in zip(got["padded"], got["poisoned"]):
        assert same_window_bits(a, b) == 0 and not torch.isnan(b).any()
    tl.ran += 2
    tl.done(8, 0)


def test_embed_finish_honours_every_leading_dimension(ops):
    tl = Tally("nv_embed_finish_fwd / nv_embed_finish_bwd")
    B, N, d, f32, p = 2, 64, 192, torch.float32, 0.25
    t, gamma, beta = rnd(B * N, d, seed=1), 1 + 0.1 * rnd(d, seed=2), 0.1 * rnd(d, seed=3)
    pos, cls, g = rnd(N + 1, d, seed=4), rnd(d, seed=5), rnd(B * (N + 1), d, seed=6)
    gm, bt, ps, cl = dev(gamma), dev(beta), dev(pos), dev(cls)
    R = B * (N + 1)
    for drop in (0.0, p):
        mask = ref_cpu.drop_mask(SEED, drop, (R, d)).double()
        kw = dict(drop_seed=SEED if drop else 0, drop_p=drop)
        td = t.double().requires_grad_(True)
        gd, bd, pd, cd = (v.double().requires_grad_(True) for v in (gamma, beta, pos, cls))
        ref = (torch.cat((cd.expand(B, 1, d), F.layer_norm(td, (d,), gd, bd, 1e-5).reshape(B, N, d)), dim=1) + pd).reshape(R, d) * mask
        ref.backward(g.double())

        def gate_fwd(o):
            assert_close_f32(o["x"], ref.detach(), "embed_finish", 1e-5)
            assert_close_f32(o["mean"], t.double().mean(1), "embed_finish.mean", 1e-5)
            assert_close_f32(o["rstd"], 1 / torch.sqrt(t.double().var(1, unbiased=False) + 1e-5), "embed_finish.rstd", 1e-5)

        res = run_windows(tl, f"nv_embed_finish_fwd dropout {drop}",
                          lambda i, o: ops.embed_finish_fwd(i["t"], B, N, gm, bt, ps, cl, x=o["x"], st=(o["mean"], o["rstd"]), **kw), {"t": (dev(t), 8)},
                          {"x": ((R, d), f32, 4, None), "mean": ((B * N,), f32, 0, None), "rstd": ((B * N,), f32, 0, None)}, gate_fwd)
        st = (res["mean"], res["rstd"])
        vec = {"dgamma": ((d,), f32, 0, None), "dbeta": ((d,), f32, 0, None), "dbias": ((d,), f32, 0, None), "dpos": (((N + 1) * d,), f32, 0, None),
               "dcls": ((d,), f32, 0, None)}
        for data_only in (False, True):
            def gate_bwd(o):
                assert_close_f32(o["dt"], td.grad, "dt", 1e-5)
                assert_close_bf16(o["dt16"], td.grad, "dt16")
                if not data_only:
                    for name, w in (("dgamma", gd.grad), ("dbeta", bd.grad), ("dbias", td.grad.sum(0)), ("dpos", pd.grad.reshape(-1)), ("dcls", cd.grad)):
                        assert_close_f32(o[name], w, name, 1e-5)

            def bwd(i, o):
                params = None if data_only else (o["dgamma"], o["dbeta"], o["dbias"], o["dpos"].view(N + 1, d), o["dcls"])
                g_arg = i["g"].clone() if drop else i["g"]            # under dropout the kernel masks the incoming gradient in place: a dense copy per launch
                ops.embed_finish_bwd(g_arg, i["t"], st, gm, B, N, dt=o["dt"], dt16=o["dt16"], params=params, data_only=data_only, **kw)
            outs = dict({"dt": ((B * N, d), f32, 4, None), "dt16": ((B * N, d), ops.op16(), 8, None)}, **({} if data_only else vec))
            run_windows(tl, f"nv_embed_finish_bwd dropout {drop}{', data only' if data_only else ''}", bwd,
                        {"g": (dev(g), None if drop else 12), "t": (dev(t), 8)}, outs, gate_bwd)
    gp = into_padded(dev(g), 12)
    refused(tl, "dropout with a padded g", lambda: ops.embed_finish_bwd(gp, dev(t), st, gm, B, N, drop_seed=SEED, drop_p=p))
    tl.done(6, 1)


# ------------------------------------------------------------------------------------------------------------ small 2-D movers
# (rows, cols) = (37, 136), one case each, none refused:
#
#   nv_cast_bf16_2d     ld_src + 4, ld_dst = cols + 8: the columns cols .. ld_dst-1 are WRITTEN AS ZERO (optim.hip: "0 for cols <= c < ld_dst"),
#                       so the window is [rows, ld_dst]; rows above / below untouched
#   nv_copy_2d_f32      store: ld_src + 8, ld_dst + 4
#   nv_copy_2d_f32      accumulate: the same
#   nv_dropout_apply    ldx + 12, ld16 + 8, ld32 + 4, dropout 0.25
#   nv_colsum_bf16      ld + 8, the [cols] sums guarded
def test_small_movers_honour_every_leading_dimension(ops):
    tl = Tally("nv_cast_bf16_2d / nv_copy_2d_f32 / nv_dropout_apply / nv_colsum_bf16")
    rows, cols, f32, t16 = 37, 136, torch.float32, ops.op16()
    x, y0 = rnd(rows, cols, seed=1), rnd(rows, cols, seed=2)
    # cast: dense = ld_dst == cols (the same kernel); padded: the zero columns belong to the destination
    dense = ops.cast_bf16(dev(x), ld_dst=cols)
    torch.cuda.synchronize()
    assert torch.equal(dense.cpu(), x.to(t16)), "nv_cast_bf16_2d is not round-to-nearest-even of the fp32 value"
    got = {}
    for wrap in (into_padded, into_poisoned):
        win, buf = padded(rows, cols + 8, t16, 0)
        src = wrap(dev(x), 4)
        assert src.stride(0) == cols + 4 and win.stride(0) == cols + 8
        ops.cast_bf16(src, out=win)
        torch.cuda.synchronize()
        assert same_window_bits(win[:, :cols], dense) == 0 and torch.count_nonzero(win[:, cols:]) == 0 and guards_intact(win, buf)
        got[wrap] = win.clone()
    assert same_window_bits(got[into_padded], got[into_poisoned]) == 0 and not torch.isnan(got[into_poisoned].float()).any()
    tl.ran += 1
    for acc in (False, True):
        want = (y0 + x) if acc else x                                           # one fp32 addition per cell: exact against torch's
        run_windows(tl, f"nv_copy_2d_f32 accumulate {acc}", lambda i, o: ops.copy_2d_f32(i["src"], o["dst"], accumulate=acc), {"src": (dev(x), 8)},
                    {"dst": ((rows, cols), f32, 4, dev(y0) if acc else None)}, lambda o: assert_close_f32(o["dst"], want.double(), "copy_2d", 1e-5))
    mask = ref_cpu.drop_mask(SEED, 0.25, (rows, cols)).double()

    def gate_drop(o):
        assert_close_f32(o["o32"], x.double() * mask, "dropout_apply.f32", 1e-5)
        assert_close_bf16(o["o16"], x.double() * mask, "dropout_apply.16")
    run_windows(tl, "nv_dropout_apply", lambda i, o: ops.dropout_apply(i["x"], SEED, 0.25, o16=o["o16"], o32=o["o32"]), {"x": (dev(x), 12)},
                {"o16": ((rows, cols), t16, 8, None), "o32": ((rows, cols), f32, 4, None)}, gate_drop)
    x16 = x.to(t16)
    run_windows(tl, "nv_colsum_bf16", lambda i, o: ops.colsum_bf16(i["X"], out=o["sum"]), {"X": (dev(x16), 8)}, {"sum": ((cols,), f32, 0, None)},
                lambda o: assert_close_f32(o["sum"], x16.double().sum(0), "colsum", 1e-5))
    tl.done(5, 0)


# ------------------------------------------------------------------------------------------------------------ fp32 inference kernels
#   nv_gemm_f32      (M, N, K) = (130, 136, 72), epilogues 0, 2, 3, 4: lda + 8, ldb + 16, ldc + 4, ldr + 12        4 cases
#   nv_ln_fwd_f32    (65, 192): ldx + 4, ldy + 8, mean / rstd guarded                                              1 case
#   nv_attn_fwd_f32  (B, n, heads) = (2, 65, 2), dim_head 64: ld_qkv + 8, ld_out + 4                               1 case
def test_fp32_kernels_honour_every_leading_dimension(ops):
    tl = Tally("nv_gemm_f32 / nv_ln_fwd_f32 / nv_attn_fwd_f32")
    f32 = torch.float32
    M, N, K = 130, 136, 72
    A, W, bias, resid = rnd(M, K, seed=1), rnd(N, K, seed=2, scale=K ** -0.5), rnd(N, seed=3), rnd(M, N, seed=4)
    ref = A.double() @ W.double().T
    bd = dev(bias)
    wants = {ops.EPI_F32_STORE: ref, ops.EPI_F32_BIAS: ref + bias.double(), ops.EPI_F32_BIAS_GELU: F.gelu(ref + bias.double()),
             ops.EPI_F32_BIAS_RESID: ref + bias.double() + resid.double()}
    for epi, want in wants.items():
        ins = {"A": (dev(A), 8), "W": (dev(W), 16)}
        if epi == ops.EPI_F32_BIAS_RESID:
            ins["resid"] = (dev(resid), 12)
        run_windows(tl, f"nv_gemm_f32 epilogue {epi}", lambda i, o: ops.gemm_f32(epi, i["A"], i["W"], bias=bd if epi else None, resid=i.get("resid"), out=o["C"]),
                    ins, {"C": ((M, N), f32, 4, None)}, lambda o: assert_close_f32(o["C"], want, f"gemm_f32 epilogue {epi}", 1e-5))
    M, d = 65, 192
    x, gamma, beta = rnd(M, d, seed=1) * 2 + 0.3, 1 + 0.1 * rnd(d, seed=2), 0.1 * rnd(d, seed=3)
    y_want, mean_want, rstd_want, _, _, _ = ln_reference(x, gamma, beta, torch.zeros_like(x), torch.zeros_like(x))
    gm, bt = dev(gamma), dev(beta)

    def gate_ln(o):
        assert_close_f32(o["y"], y_want, "ln_fwd_f32", 1e-5)
        assert_close_f32(o["mean"], mean_want, "mean", 1e-5)
        assert_close_f32(o["rstd"], rstd_want, "rstd", 1e-5)
    run_windows(tl, "nv_ln_fwd_f32", lambda i, o: ops.ln_fwd_f32(i["x"], gm, bt, y=o["y"], st=(o["mean"], o["rstd"])), {"x": (dev(x), 4)},
                {"y": ((M, d), f32, 8, None), "mean": ((M,), f32, 0, None), "rstd": ((M,), f32, 0, None)}, gate_ln)
    B, n, heads, dh = 2, 65, 2, 64
    inner = heads * dh
    qkv = rnd(B * n, 3 * inner, seed=n)
    q, k, v = (t.reshape(B, n, heads, dh).permute(0, 2, 1, 3).double() for t in qkv.chunk(3, dim=-1))
    want = (torch.softmax(q @ k.transpose(-1, -2) * dh ** -0.5, dim=-1) @ v).permute(0, 2, 1, 3).reshape(B * n, inner)
    run_windows(tl, "nv_attn_fwd_f32", lambda i, o: ops.attn_fwd_f32(i["qkv"], B, n, heads, dh, out=o["out"]), {"qkv": (dev(qkv), 8)},
                {"out": ((B * n, inner), f32, 4, None)}, lambda o: assert_close_f32(o["out"], want, "attn_fwd_f32", 1e-5))
    tl.done(6, 0)


# ------------------------------------------------------------------------------------------------------------ fp16 operand format
# The second instantiation of every 16-bit kernel (nv_set_operand_format(NV_OPERAND_FP16), as tests/test_fp16_gpu.py switches it):
#
#   nv_gemm_bf16     NT epilogue 4 at (264, 136, 128), every tile family                                   9 cases
#   nv_ln_fwd / nv_ln_bwd   (65, 192): forward and the three g_in forms                                    4 cases
#   nv_attn_fwd / nv_attn_bwd   (2, 65, 2), mode 2, dropout 0 and 0.1                                      4 cases
@contextlib.contextmanager
def fp16_operands():
    from neurovit_amd import _cabi
    _cabi.set_operand_format("fp16")
    try:
        with ref_cpu.operand_format("fp16"):
            yield
    finally:
        _cabi.set_operand_format("bf16")


def test_fp16_operands_honour_every_leading_dimension(ops, lib, attn_data):
    tl = Tally("fp16 operands: nv_gemm_bf16 NT epilogue 4, LayerNorm [65, 192], attention (2, 65, 2) mode 2")
    M, N, K = M_G, N_G, K_G
    A, B = rnd(M, K, seed=1).half(), rnd(N, K, seed=2, scale=K ** -0.5).half()
    bias, resid = rnd(N, seed=3), rnd(M, N, seed=4)
    want = A.double() @ B.double().T + bias.double() + resid.double()
    bd = dev(bias)
    with fp16_operands():
        assert ops.op16() == torch.float16
        for family in TILES:
            with forced(lib, family):
                run_windows(tl, f"NT epilogue 4, {family}", lambda i, o: ops.gemm(ops.NT, ops.EPI_BIAS_RESID, i["A"], i["B"], out=o["C"], bias=bd, aux_in=i["aux_in"]),
                            {"A": (dev(A), PAD_A), "B": (dev(B), PAD_B), "aux_in": (dev(resid), 12)}, {"C": ((M, N), torch.float32, PAD_F32, None)},
                            lambda o: assert_close_f32(o["C"], want, "fp16 bias_resid", 1e-5))
        Ml, d = 65, 192
        x, gamma, beta = rnd(Ml, d, seed=1) * 2 + 0.3, 1 + 0.1 * rnd(d, seed=2), 0.1 * rnd(d, seed=3)
        ln_forward_case(ops, tl, x, gamma, beta, " fp16")
        ln_backward_cases(ops, tl, x, gamma, beta, rnd(Ml, d, seed=4), rnd(Ml, d, seed=5))
        try:
            assert lib.nv_attn_set_mode(2) == 0
            for drop in ATTN_DROPS:
                attention_cases(ops, tl, attn_data(2, 65, 2, 64, drop, "fp16"), 2, 65, 2, 64, drop, f"fp16 (2, 65, 2) dropout {drop}")
        finally:
            lib.nv_attn_set_mode(0)
    tl.done(len(TILES) + 4 + 4, 0)
