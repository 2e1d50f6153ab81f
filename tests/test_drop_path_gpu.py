"""Stochastic depth on the MI355X: the draw kernel bit for bit against its restatement, the four path-aware kernel sites read back
exactly (inputs that make a kernel's output its combined factor k = e * f, the idiom of tests/test_dropout_masks_gpu.py), and the engine,
the one-call train step and the module over hand-made and drawn tables.  tests/drop_path_ref.py is the CPU restatement."""
import contextlib

import pytest
import torch
import torch.nn.functional as F

import drop_path_ref as dpr
import weights as W
from conftest import rel_err, rel_l2, report
from oracle import ref_cpu, train_step
from test_dropout_masks_cpu import FORMATS, SEED
from test_dropout_masks_gpu import ROW_SHAPES, TILES, _head_grad, _head_inputs, close32, dense_mask, operands, rnd
from test_engine_gpu import GRAD_REL, RATIO, REL, SLACK
from test_gemm_epilogue_batching_gpu import PP, WS
from test_gemm_epilogue_batching_gpu import REL as GEMM_REL

pytestmark = pytest.mark.gpu
P = 0.25                                    # element dropout of the kernel-level read-outs: e = 4 / 3, not a power of two


@pytest.fixture(scope="module")
def ops():
    from neurovit_amd import ops as _ops
    from neurovit_amd._cabi import require_gpu
    require_gpu()
    return _ops


def site_table(samples):
    """fp32 [samples] of distinct factors 1, 1.25, 0, 1.75, 2, 2.25, ... (the zero third, so that a one-sample table is not all zeros);
    every product with e = fp32(4 / 3) is one fp32 multiply"""
    t = 0.25 * (torch.arange(samples, dtype=torch.float32) + 4)
    if samples > 2:
        t[2] = 0.0
    return t


def per_row(table, M, rows, step=1):
    """the factor of launch row r = table[r * step // rows], fp32 [M, 1]"""
    return table[(torch.arange(M) * step) // rows][:, None]


# ------------------------------------------------------------------------------------------------------------ the draw
@pytest.mark.parametrize("rate", [0.0, 0.1, 0.5])
@pytest.mark.parametrize("kind", [dpr.LINEAR, dpr.CONSTANT])
@pytest.mark.parametrize("B,depth", [(1, 1), (3, 2), (5, 12), (4096, 12)])
def test_draw_equals_the_restatement(ops, B, depth, kind, rate):
    for seed in (1234, (1 << 63) + 5):
        got = ops.drop_path_draw(seed, B, depth, rate, kind).cpu()
        assert torch.equal(got, dpr.draw_table(seed, B, depth, rate, kind)), (seed, B, depth, kind, rate)
        if rate == 0.0:
            assert bool((got == 1.0).all())


# ------------------------------------------------------------------------------------------------------------ GEMM residual epilogue
@pytest.mark.parametrize("fmt", list(FORMATS))
@pytest.mark.parametrize("M,N", [(257, 264), (130, 136), (300, 8)])
@pytest.mark.parametrize("tile", TILES)
def test_gemm_residual_epilogue_applies_the_row_factor(ops, tile, M, N, fmt):
    """A = 0, bias = 1, residual = 0: the output IS the combined factor of its element - table[m / rows] without dropout, fp32(e * f) with it.
    rows = 1 catches any lane or row mix-up; 9 and 65 put sample boundaries inside a 16-row fragment and inside every tile height.
    (K as in test_gemm_epilogues_apply_the_oracle_mask: 8 reaches the small-tile kernel only, the forced tiles run [., 64].)"""
    from neurovit_amd._cabi import lib
    bias, resid = torch.ones(N, device="cuda"), torch.zeros((M, N), device="cuda")
    if tile[0] == 11:
        lib.nv_gemm_set_tile(4, 0)
    lib.nv_gemm_set_tile(*tile)
    try:
        with operands(fmt) as dtype:
            for K in ((8, 64) if tile[0] == 0 else (64,)):
                A0, B0 = torch.zeros((M, K), dtype=dtype, device="cuda"), torch.zeros((N, K), dtype=dtype, device="cuda")
                for rows in (1, 9, 65, M):
                    table = site_table((M + rows - 1) // rows)
                    f = per_row(table, M, rows)
                    out = ops.gemm(ops.NT, ops.EPI_BIAS_RESID, A0, B0, bias=bias, aux_in=resid, path=table.cuda(), path_rows=rows)
                    assert torch.equal(out.cpu(), f.expand(M, N)), (tile, M, N, K, rows, "p = 0")
                    out = ops.gemm(ops.NT, ops.EPI_BIAS_RESID, A0, B0, bias=bias, aux_in=resid, drop_seed=SEED, drop_p=P, path=table.cuda(), path_rows=rows)
                    assert torch.equal(out.cpu(), dense_mask(P, M, N) * f), (tile, M, N, K, rows, "p = 0.25")
            # random operands and residual against float64; and without a table the call IS nv_gemm_bf16
            K, rows = 64, 9
            A, Bm = rnd(M, K, seed=1).to(dtype), rnd(N, K, seed=2).to(dtype)
            b, r = rnd(N, seed=3), rnd(M, N, seed=4)
            table = site_table((M + rows - 1) // rows)
            k = dense_mask(P, M, N).double() * per_row(table, M, rows).double()
            want = r.double() + (A.double() @ Bm.double().t() + b.double()) * k
            out = ops.gemm(ops.NT, ops.EPI_BIAS_RESID, A.cuda(), Bm.cuda(), bias=b.cuda(), aux_in=r.cuda(), drop_seed=SEED, drop_p=P, path=table.cuda(), path_rows=rows)
            assert rel_err(out, want) <= GEMM_REL, (tile, M, N, rel_err(out, want))
            plain = ops.gemm(ops.NT, ops.EPI_BIAS_RESID, A.cuda(), Bm.cuda(), bias=b.cuda(), aux_in=r.cuda(), drop_seed=SEED, drop_p=P)
            null = ops.gemm(ops.NT, ops.EPI_BIAS_RESID, A.cuda(), Bm.cuda(), bias=b.cuda(), aux_in=r.cuda(), drop_seed=SEED, drop_p=P, path=None, path_rows=rows)
            ones = ops.gemm(ops.NT, ops.EPI_BIAS_RESID, A.cuda(), Bm.cuda(), bias=b.cuda(), aux_in=r.cuda(), drop_seed=SEED, drop_p=P,
                            path=torch.ones_like(table).cuda(), path_rows=rows)
            assert torch.equal(null, plain) and torch.equal(ones, plain), (tile, M, N, "NULL table / all-ones table")
    finally:
        if tile[0] == 11:
            lib.nv_gemm_set_tile(11, 0)
        lib.nv_gemm_set_tile(0, 0)


@pytest.mark.parametrize("fmt", list(FORMATS))
def test_skinny_nt_applies_the_factor_of_the_dense_row(ops, fmt):
    """R = 3 rows strided by n = 9 of a dense [27, 64] tensor: strided row r is dense row 9 r, so with 9 rows per sample its sample is r."""
    R, n, N, K = 3, 9, 64, 64
    M = R * n
    table = site_table(R)
    f = table[:, None]
    with operands(fmt) as dtype:
        zA, zW = torch.zeros((M, K), dtype=dtype, device="cuda"), torch.zeros((N, K), dtype=dtype, device="cuda")
        for p in (0.0, P):
            y = torch.full((M, N), 3.0, device="cuda")
            ops.skinny_nt(0, zA[::n], zW, torch.ones(N, device="cuda"), y[::n], resid=torch.zeros((M, N), device="cuda")[::n], drop_seed=SEED, drop_p=p,
                          path=table.cuda(), path_rows=n)
            assert torch.equal(y[::n].cpu(), dense_mask(p, M, N)[::n] * f), (fmt, p)
            keep = torch.ones(M, dtype=torch.bool); keep[::n] = False
            assert bool((y.cpu()[keep] == 3.0).all())
        A, Wm, b, r = rnd(M, K, seed=1).to(dtype), rnd(N, K, seed=2).to(dtype), rnd(N, seed=3), rnd(M, N, seed=4)
        want = r.double()[::n] + (A.double()[::n] @ Wm.double().t() + b.double()) * (dense_mask(P, M, N)[::n].double() * f.double())

        def run(**kw):
            y = torch.zeros((M, N), device="cuda")
            ops.skinny_nt(0, A.cuda()[::n], Wm.cuda(), b.cuda(), y[::n], resid=r.cuda()[::n], drop_seed=SEED, drop_p=P, **kw)
            return y[::n].clone()
        assert rel_err(run(path=table.cuda(), path_rows=n), want) <= GEMM_REL
        plain = run()
        assert torch.equal(run(path=None, path_rows=n), plain) and torch.equal(run(path=torch.ones(R).cuda(), path_rows=n), plain)


# ------------------------------------------------------------------------------------------------------------ LayerNorm backward
def _ln_inputs(M, d):
    x, gamma, beta = rnd(M, d, seed=1) * 2 + 0.3, 1 + 0.1 * rnd(d, seed=2), 0.1 * rnd(d, seed=3)
    return x, gamma, beta, rnd(M, d, seed=4), rnd(M, d, seed=5)


@pytest.mark.parametrize("fmt", list(FORMATS))
@pytest.mark.parametrize("rows", [1, 9])
@pytest.mark.parametrize("M,d", ROW_SHAPES)
def test_ln_bwd_scales_its_16_bit_gradient_by_the_combined_factor(ops, M, d, rows, fmt):
    """nv_ln_bwd_path: the fp32 g_out is the call without a table, bit for bit; g16 = cvt16(g_out * fp32(e * f)) from the kernel's own g_out;
    the column sums are those of g_out e f."""
    x, gamma, beta, dy, g_in = _ln_inputs(M, d)
    table = site_table((M + rows - 1) // rows) % 8.0            # (2052 samples at rows = 1: keep the factors small; neighbours still differ)
    f = per_row(table, M, rows)
    with operands(fmt) as dtype:
        _, st = ops.ln_fwd(x.cuda(), gamma.cuda(), beta.cuda())
        for p in (0.0, P):
            base = ops.ln_bwd(dy.cuda(), x.cuda(), st, gamma.cuda(), g_in=g_in.clone().cuda(), drop_seed=SEED, drop_p=p)
            g_out, g16, dg, db, dc = ops.ln_bwd(dy.cuda(), x.cuda(), st, gamma.cuda(), g_in=g_in.clone().cuda(), drop_seed=SEED, drop_p=p, path=table.cuda(), path_rows=rows)
            assert torch.equal(g_out, base[0]) and torch.equal(dg, base[2]) and torch.equal(db, base[3]), (M, d, rows, p)
            k = dense_mask(p, M, d) * f
            g = g_out.cpu()
            assert torch.equal(g16.float().cpu(), (g * k).to(dtype).float()), (M, d, rows, p, fmt)
            close32(dc, (g.double() * k.double()).sum(0), "ln_bwd_path.colsum")
            for alt in (dict(path=None, path_rows=rows), dict(path=torch.ones_like(table).cuda(), path_rows=rows)):
                same = ops.ln_bwd(dy.cuda(), x.cuda(), st, gamma.cuda(), g_in=g_in.clone().cuda(), drop_seed=SEED, drop_p=p, **alt)
                assert all(torch.equal(a, b) for a, b in zip(same, base)), (M, d, rows, p, "NULL / all-ones table")


def test_ln_bwd_row_strided_call_takes_the_dense_rows_sample(ops):
    """M = 3 rows of a dense [27, 192] gradient, ldg = 9 d (the cls rows of three samples of 9 tokens): launch row r is sample r."""
    from neurovit_amd._cabi import check, lib
    R, n, d, dtype = 3, 9, 192, torch.bfloat16
    M = R * n
    x, gamma, beta, dy, g_in = _ln_inputs(M, d)
    table = torch.tensor([2.0, 0.0, 1.25])
    _, st = ops.ln_fwd(x.cuda()[::n].contiguous(), gamma.cuda(), beta.cuda())
    xs, dys, gm, tb = x.cuda(), dy.cuda(), gamma.cuda(), table.cuda()
    nb = lib.nv_ln_bwd_workspace_bytes(R, d)
    outs = {}
    for name, path in (("plain", None), ("path", tb)):
        g = g_in.clone().cuda()
        g16 = torch.full((M, d), 7.0, dtype=dtype, device="cuda")
        dg, db, dc = (torch.empty(d, device="cuda") for _ in range(3))
        ws = torch.empty(nb, dtype=torch.uint8, device="cuda")
        check(lib.nv_ln_bwd_path(dys.data_ptr(), n * d, xs.data_ptr(), n * d, st[0].data_ptr(), st[1].data_ptr(), gm.data_ptr(), R, d, g.data_ptr(), g.data_ptr(), n * d,
                                 g16.data_ptr(), n * d, dg.data_ptr(), db.data_ptr(), dc.data_ptr(), 0, ws.data_ptr(), nb, SEED, P, torch.cuda.current_stream().cuda_stream,
                                 None, None if path is None else path.data_ptr(), n), "nv_ln_bwd_path")
        outs[name] = (g.cpu(), g16.cpu(), dc.cpu())
    assert torch.equal(outs["path"][0], outs["plain"][0])
    g = outs["path"][0][::n]
    k = dense_mask(P, M, d)[::n] * table[:, None]
    assert torch.equal(outs["path"][1][::n].float(), (g * k).to(dtype).float())
    keep = torch.ones(M, dtype=torch.bool); keep[::n] = False
    assert bool((outs["path"][1][keep] == 7).all())
    close32(outs["path"][2], (g.double() * k.double()).sum(0), "ln_bwd_path.colsum, strided")


# ------------------------------------------------------------------------------------------------------------ the head's backward
def _check_head(g, g16, dcol, want, table, p, pool_mean, dtype, what):
    B, n, d = want.shape
    close32(g, want, f"{what}.g")
    gc = g.cpu()
    k = ref_cpu.drop_mask(SEED, p, (B, n, d)) * table[:, None, None]
    live = slice(None) if pool_mean else slice(0, 1)
    assert torch.equal(g16[:, live].float().cpu(), (gc * k)[:, live].to(dtype).float()), (what, p)
    if not pool_mean:
        assert not gc[:, 1:].any() and not g16[:, 1:].any()
    close32(dcol, (want * k.double()).sum((0, 1)), f"{what}.colsum")


@pytest.mark.parametrize("fmt", list(FORMATS))
@pytest.mark.parametrize("pool_mean", [0, 1])
def test_head_bwd_scales_its_16_bit_gradient_by_the_samples_factor(ops, pool_mean, fmt):
    from neurovit_amd._cabi import check, lib
    B, n, d, C, x, gamma, beta, Wt, bias = _head_inputs()
    dl = rnd(B, C, seed=6)
    table = torch.tensor([1.25, 0.0, 2.0])
    pooled = x.mean(1) if pool_mean else x[:, 0]
    row_grad = _head_grad(pooled, gamma, beta, Wt, bias, dl=dl)
    want = torch.zeros((B, n, d), dtype=torch.float64)
    if pool_mean:
        want[:] = (row_grad / n)[:, None, :]
    else:
        want[:, 0] = row_grad
    with operands(fmt) as dtype:
        xin = pooled.reshape(B, 1, d).contiguous().cuda() if pool_mean else x.cuda()
        _, xh, st = ops.head_fwd(xin, gamma.cuda(), beta.cuda(), Wt.cuda(), bias.cuda())
        for p in (0.0, P):
            res = {}
            for name, path in (("plain", None), ("ones", torch.ones(B).cuda()), ("path", table.cuda())):
                if not pool_mean:
                    g, g16, _, _, _, _, dcol = ops.head_bwd(dl.cuda(), Wt.cuda(), xin, st, xh, gamma.cuda(), drop_seed=SEED, drop_p=p, path=path, path_rows=n)
                else:
                    g = torch.full((B, n, d), float("nan"), device="cuda"); g16 = torch.full((B, n, d), float("nan"), dtype=dtype, device="cuda")
                    dgm, dbt, dcol = (torch.empty(d, device="cuda") for _ in range(3))
                    dW, dbs = torch.empty((C, d), device="cuda"), torch.empty(C, device="cuda")
                    nb = lib.nv_head_bwd_workspace_bytes(B, d)
                    ws = torch.empty(nb, dtype=torch.uint8, device="cuda")
                    gm, Wd, dld = gamma.cuda(), Wt.cuda(), dl.cuda()
                    check(lib.nv_head_bwd_path(dld.data_ptr(), B, C, Wd.data_ptr(), xin.data_ptr(), d, st.data_ptr(), xh.data_ptr(), gm.data_ptr(), d, n, g.data_ptr(), d,
                                               g16.data_ptr(), d, dgm.data_ptr(), dbt.data_ptr(), dW.data_ptr(), dbs.data_ptr(), dcol.data_ptr(), 0, ws.data_ptr(), nb, SEED, p, 1,
                                               torch.cuda.current_stream().cuda_stream, None if path is None else path.data_ptr(), n), "nv_head_bwd_path")
                res[name] = (g, g16, dcol)
            _check_head(*res["path"], want, table, p, pool_mean, dtype, f"head_bwd_path pool_mean {pool_mean}")
            assert torch.equal(res["path"][0], res["plain"][0])                                   # the fp32 g is not scaled
            assert all(torch.equal(a, b) for a, b in zip(res["ones"], res["plain"]))
            if not pool_mean:
                base = ops.head_bwd(dl.cuda(), Wt.cuda(), xin, st, xh, gamma.cuda(), drop_seed=SEED, drop_p=p)      # the existing symbol
                assert torch.equal(base[0], res["plain"][0]) and torch.equal(base[1], res["plain"][1]) and torch.equal(base[6], res["plain"][2])


@pytest.mark.parametrize("soft", [False, True])
def test_head_step_path_form_serves_the_plain_and_the_soft_variants(ops, soft):
    B, n, d, C, x, gamma, beta, Wt, bias = _head_inputs()
    labels = torch.tensor([i % C for i in range(B)])
    table = torch.tensor([0.0, 2.0, 1.25])
    opts = ops.loss_opts(0.1, None, None, B, C, "cuda") if soft else None
    target = F.one_hot(labels, C).double() * 0.9 + 0.1 / C if soft else None
    rd = x[:, 0].double().requires_grad_(True)
    logits = F.linear(F.layer_norm(rd, (d,), gamma.double(), beta.double(), 1e-5), Wt.double(), bias.double())
    (-(target * F.log_softmax(logits, -1)).sum(-1).mean() if soft else F.cross_entropy(logits, labels)).backward()
    want = torch.zeros((B, n, d), dtype=torch.float64)
    want[:, 0] = rd.grad
    args = (x.cuda(), gamma.cuda(), beta.cuda(), Wt.cuda(), bias.cuda(), labels.cuda())
    for p in (0.0, P):
        outs = ops.head_step(*args, drop_seed=SEED, drop_p=p, path=table.cuda(), path_rows=n, opts=opts)
        _check_head(outs[5], outs[6], outs[11], want, table, p, 0, torch.bfloat16, f"head_step_path soft {soft}")
        null = ops.head_step(*args, drop_seed=SEED, drop_p=p, path=None, path_rows=n, opts=opts)
        ones = ops.head_step(*args, drop_seed=SEED, drop_p=p, path=torch.ones(B).cuda(), path_rows=n, opts=opts)
        assert all(torch.equal(a, b) for a, b in zip(ones, null))
        assert torch.equal(outs[0], null[0]) and torch.equal(outs[3], null[3]) and torch.equal(outs[5], null[5])      # logits, loss and the fp32 g: no factor
        if not soft:
            base = ops.head_step(*args, drop_seed=SEED, drop_p=p)                                                      # nv_head_step itself
            assert all(torch.equal(a, b) for a, b in zip(base, null))


# ------------------------------------------------------------------------------------------------------------ the engine
DROPOUT = (0.1, 0.2, 0x1234567)
CASES = {"micro": (W.MICRO, 3), "noproj": (W.NOPROJ, 5)}


class Net:
    """A ViT on the device with the golden weights: its runtime, arenas and parameter table drive the engine directly."""

    def __init__(self, cfgdict, B, fmt="bf16"):
        from neurovit_amd.vit_3d import ViT
        self.cfgdict, self.B = cfgdict, B
        self.sd = W.make_tensors(W.vit_param_spec(**cfgdict), 1)
        self.m = ViT(**cfgdict).cuda()
        self.m.load_state_dict(self.sd, strict=True)
        self.m.set_operands(fmt)
        self.params, self.params16 = self.m.flat_parameters()
        self.m._refresh_shadow()
        S = cfgdict["image_size"]
        self.fmri = W.make_volume((B, S, S, S), 2)
        self.video = ref_cpu.fmri_to_video(self.fmri.cuda())
        self.rt = self.m._rt
        self.depth, self.n, self.d = cfgdict["depth"], self.m.pos_embedding.shape[1], cfgdict["dim"]
        self.dlogits = rnd(B, cfgdict["num_classes"], seed=9).cuda()
        self.labels = torch.tensor([i % cfgdict["num_classes"] for i in range(B)], device="cuda")

    def ones(self):
        return torch.ones((self.depth, 2, self.B), device="cuda")

    def forms(self):
        return (1, 2) if self.B <= 4 and self.cfgdict["pool"] == "cls" else (1,)

    def pass_(self, table, dropout, rows_form, dlogits=None):
        """forward + backward; every tap cloned.  In the cls-rows form only the cls rows of the last block's x1 / x2 are produced."""
        B, n, d, rt = self.B, self.n, self.d, self.rt
        out = {"logits": rt.forward(self.video, self.params, self.params16, training=True, dropout=dropout, rows_form=rows_form, drop_path=table).clone()}
        out["x0"] = rt.tap("x0", -1, (B, n, d), torch.float32).clone()
        for l in range(self.depth):
            rows = slice(0, 1) if (rows_form == 2 and l == self.depth - 1) else slice(None)
            for name in ("x1", "x2"):
                out[f"{name}.{l}"] = rt.tap(name, l, (B, n, d), torch.float32)[:, rows].clone()
        grads, dvideo = torch.zeros_like(self.params), torch.empty_like(self.video)
        rt.backward(self.dlogits if dlogits is None else dlogits, self.params, self.params16, grads, accumulate=False, dvideo=dvideo)
        out["grads"], out["dvideo"] = grads, dvideo
        return out

    def step(self, table, dropout, rows_form, fuse):
        p, p16 = self.params.clone(), self.params16.clone()
        g, am, av = (torch.zeros_like(p) for _ in range(3))
        loss, logits = self.rt.train_step(self.video, self.labels, p, p16, g, am, av, step=1, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2,
                                          fuse_update=fuse, dropout=dropout, rows_form=rows_form, drop_path=table)
        return dict(loss=loss.clone(), logits=logits.clone(), params=p, params16=p16, grads=g, adam_m=am, adam_v=av)


def same(a, b, what):
    for k in a:
        assert torch.equal(a[k], b[k]), (what, k)


def check_all_ones_is_nothing(net, dropouts=((0.0, 0.0, 0), DROPOUT)):
    for dropout in dropouts:
        for rf in net.forms():
            same(net.pass_(net.ones(), dropout, rf), net.pass_(None, dropout, rf), ("forward + backward", dropout, rf))
            for fuse in (0, 1, 2, 3):
                same(net.step(net.ones(), dropout, rf, fuse), net.step(None, dropout, rf, fuse), ("train step", dropout, rf, fuse))


def check_dropped_sample_passes_through(net, dropouts=((0.0, 0.0, 0), DROPOUT)):
    L = net.depth
    table = net.ones()
    table[:, :, 1] = 0
    others = [b for b in range(net.B) if b != 1]
    for dropout in dropouts:
        for rf in net.forms():
            got, ref = net.pass_(table, dropout, rf), net.pass_(net.ones(), dropout, rf)
            rows = slice(0, 1) if rf == 2 else slice(None)
            assert torch.equal(got[f"x2.{L - 1}"][1], got["x0"][1, rows]), (dropout, rf)
            for k in ref:
                if k not in ("grads", "dvideo"):
                    assert torch.equal(got[k][others], ref[k][others]), (k, dropout, rf)
            dv = got["dvideo"]
            assert not dv[1].any(), (dropout, rf)
            assert bool(torch.isfinite(dv).all()) and all(bool(dv[b].any()) for b in others)
            assert torch.equal(dv[others], ref["dvideo"][others])


@pytest.mark.parametrize("case", list(CASES))
def test_all_ones_table_is_nothing(ops, case):
    check_all_ones_is_nothing(Net(*CASES[case]))


@pytest.mark.parametrize("case", list(CASES))
def test_dropped_sample_passes_through(ops, case):
    check_dropped_sample_passes_through(Net(*CASES[case]))


def test_fp16_operands(ops):
    net = Net(W.MICRO, 3, "fp16")
    try:
        check_all_ones_is_nothing(net, (DROPOUT,))
        check_dropped_sample_passes_through(net, (DROPOUT,))
    finally:
        from neurovit_amd import _cabi
        _cabi.set_operand_format("bf16")


@contextlib.contextmanager
def forced_tile(tile):
    from neurovit_amd._cabi import lib
    lib.nv_gemm_set_tile(*tile)
    try:
        yield
    finally:
        lib.nv_gemm_set_tile(0, 0)


@pytest.mark.parametrize("tile", [PP] + WS, ids=lambda t: "x".join(map(str, t)))
def test_forced_tile_families_through_the_engine(ops, tile):
    net = Net(W.MICRO, 3)
    with forced_tile(tile):
        check_all_ones_is_nothing(net, (DROPOUT,))
        check_dropped_sample_passes_through(net, (DROPOUT,))


def general_table(B, depth):
    """the drawn factors at rate 0.5, constant schedule (about half of the sites dropped, kept ones 2.0) plus one hand-set power of two per
    layer: a wrong site or layer index is an O(1) error"""
    table = dpr.draw_table(0xD1CE, B, depth, 0.5, dpr.CONSTANT)
    for l in range(depth):
        table[l, l % 2, l % B] = 4.0 if l % 2 == 0 else 0.5
    assert bool((table == 0).any()) and bool((table == 2.0).any())
    return table


@pytest.mark.parametrize("case,dropout", [("micro", (0.0, 0.0, 0)), ("micro", DROPOUT), ("noproj", (0.0, 0.0, 0)), ("mean", (0.0, 0.0, 0))])
def test_general_factors_three_way(ops, case, dropout):
    """Forward stages, logits and every parameter gradient against vit_forward_sd with and without the emulation of the 16-bit cast points:
    the gate and the constants of tests/test_engine_gpu.py::_run_case_full_rows (every-row form)."""
    cfgdict, B = (dict(W.MICRO, pool="mean"), 3) if case == "mean" else CASES[case]
    net = Net(cfgdict, B)
    table = general_table(B, net.depth)
    ocfg = ref_cpu.ViTCfg(**cfgdict)
    video = ref_cpu.fmri_to_video(net.fmri)

    def oracle(emulate):
        leaves = {k: v.clone().requires_grad_(True) for k, v in net.sd.items()}
        taps = {}
        return leaves, taps, dpr.vit_forward_sd(leaves, ocfg, video, table, emulate_bf16=emulate, dropout=dropout, taps=taps)
    leaves, taps, ref_logits = oracle(True)
    leaves32, taps32, logits32 = oracle(False)
    labels = net.labels.cpu()
    names = list(leaves)
    ref_grads = dict(zip(names, torch.autograd.grad(train_step.cross_entropy(ref_logits, labels), [leaves[k] for k in names])))
    grads32 = dict(zip(names, torch.autograd.grad(train_step.cross_entropy(logits32, labels), [leaves32[k] for k in names])))
    ld = ref_logits.detach().clone().requires_grad_(True)          # dlogits from the oracle's logits: the backward comparison is not polluted by the forward difference
    (dlogits,) = torch.autograd.grad(train_step.cross_entropy(ld, labels), ld)
    got = net.pass_(table.cuda(), dropout, 1, dlogits.cuda())
    fails = []

    def three_way(kind, name, hip, emu, f32, limit):
        e_he, e_h32, e_e32 = rel_l2(hip, emu), rel_l2(hip, f32), rel_l2(emu, f32)
        report(f"drop path {case} {kind} {name}: hip-emu {e_he:.3e}  hip-fp32 {e_h32:.3e}  emu-fp32 {e_e32:.3e}")
        if not (e_h32 <= RATIO * e_e32 + SLACK and e_he <= limit):
            fails.append((kind, name, e_he, e_h32, e_e32))
    three_way("fwd", "A5", got["x0"], taps["A5"], taps32["A5"], REL)
    for i in range(net.depth):
        three_way("fwd", f"block{i}", got[f"x2.{i}"], taps[f"block{i}"], taps32[f"block{i}"], REL)
    three_way("fwd", "logits", got["logits"], ref_logits, logits32, 2 * REL)
    off, num, _ = net.m._layout
    assert [k for k, _ in net.m.named_parameters()] == names
    gcpu = got["grads"].cpu()
    for k, o, nn in zip(names, off, num):
        three_way("grad", k, gcpu[o:o + nn].reshape(ref_grads[k].shape), ref_grads[k], grads32[k], GRAD_REL)
    assert not fails, fails


# ------------------------------------------------------------------------------------------------------------ the module
SIZE = dict(TRAINING_VIT_DIM=128, TRAINING_VIT_DEPTH=2, TRAINING_VIT_HEADS=2, TRAINING_VIT_MLP_DIM=256)


def _model(rate, dropout=0.0, **extra):
    from neurovit_amd.NeuroEncoder import NeuroEncoder
    cfg = W.neuro_config(32, 8, DEVICE="cuda", TRAINING_DROPOUT=dropout, TRAINING_DROP_PATH=rate, TRAINING_LEARNING_RATE=1e-3, TRAINING_WEIGHT_DECAY=1e-2, **SIZE, **extra)
    model = NeuroEncoder(cfg)
    model.load_state_dict(W.make_tensors(W.vit_param_spec(**W.MICRO), 1, prefix="volume_encoder.vit3d."), strict=True)
    return model


def test_module_draws_one_table_per_training_forward(ops):
    x = W.make_volume((3, 32, 32, 32), 2).cuda()
    model = _model(0.2)
    vit = model.volume_encoder.vit3d
    model.train()
    for grad in (True, False):
        torch.manual_seed(21 + grad)
        seed = int(torch.randint(0, 2 ** 62, (1,)).item())          # what draw_dropout draws first
        torch.manual_seed(21 + grad)
        with torch.enable_grad() if grad else torch.no_grad():
            out = model(x)
        assert torch.equal(vit.last_drop_path.cpu(), dpr.draw_table(seed, 3, 2, 0.2))
        assert tuple(vit.last_drop_path.shape) == (2, 2, 3) and vit._rt.last.drop_path is vit.last_drop_path
        if grad:
            out.sum().backward()                                      # the backward takes the pass's table
            assert all(p.grad is not None and bool(torch.isfinite(p.grad).all()) for p in vit.parameters())
    # eval mode: untouched by the rate
    model.eval()
    with torch.no_grad():
        with_rate = model(x).clone()
        vit.drop_path_rate = 0.0
        assert torch.equal(model(x), with_rate)


@pytest.mark.parametrize("case", ["plain", "accumulate2", "dropout"])
def test_native_step_equals_the_general_path_under_drop_path(ops, case):
    """As tests/test_modules_gpu.py::test_native_train_step_equals_the_general_path_bitwise, with TRAINING_DROP_PATH = 0.2: both paths draw
    their seeds from torch's generator, one per (micro-)step, and their tables from those seeds."""
    from neurovit_amd.trainer import TrainStep
    acc = 2 if case == "accumulate2" else 1
    x = W.make_volume((3, 32, 32, 32), 2).cuda()
    y = torch.tensor([1, 0, 1], device="cuda")
    runs = []
    for native in (True, False):
        model = _model(0.2, 0.1 if case == "dropout" else 0.0)
        model.train()
        step = TrainStep(model, accumulation_steps=acc)
        if not native:
            step._native = False
        torch.manual_seed(11)
        losses = [step(x, y).clone() for _ in range(2 * acc)]
        assert step._native == native and step.last_path == ("native" if native else "general")
        vit = model.volume_encoder.vit3d
        assert not step._plan(3 * 65, vit._dropout_p != (0.0, 0.0) or vit.drop_path_rate > 0, False).graph_ok
        runs.append((torch.stack(losses), step.last_outputs.clone(), vit.flat_gradients().clone(), vit.flat_parameters()[0].clone(), vit.flat_parameters()[1].clone(),
                     vit.last_drop_path.clone()))
    for i, name in enumerate(("losses", "logits", "gradient arena", "parameters", "16-bit shadow", "last table")):
        assert torch.equal(runs[0][i], runs[1][i]), f"{case}: {name} differ between the native call and the general path"
    # and the rate matters: the same seeds at rate 0 give other parameters
    model = _model(0.0, 0.1 if case == "dropout" else 0.0)
    model.train()
    step = TrainStep(model, accumulation_steps=acc)
    torch.manual_seed(11)
    for _ in range(2 * acc):
        step(x, y)
    assert not torch.equal(model.volume_encoder.vit3d.flat_parameters()[0], runs[0][3])


def test_refusals_at_the_point_of_use(ops):
    from neurovit_amd.pretrain import MaskedPretrainStep
    x = W.make_volume((2, 32, 32, 32), 2).cuda()
    model = _model(0.2)
    vit = model.volume_encoder.vit3d
    model.train()
    video = x.permute(0, 3, 1, 2).unsqueeze(1)
    with pytest.raises(NotImplementedError, match="drop_path_rate"):
        vit.forward_tokens(video)
    with pytest.raises(NotImplementedError, match="drop_path_rate"):
        MaskedPretrainStep(model)
    with pytest.raises(NotImplementedError, match="drop_path_rate"):
        vit.enable_fp8(video, training=True)
    with pytest.raises(NotImplementedError, match="on its own"):
        vit.transformer(torch.zeros(2, 65, 128, device="cuda"))
    vit.drop_path_rate = 0.0
    pre = MaskedPretrainStep(model)
    vit.drop_path_rate = 0.2                                           # set after the step was built: refused at the call
    with pytest.raises(NotImplementedError, match="drop_path_rate"):
        pre(x)
    vit.drop_path_rate = 0.0
    vit.enable_fp8(video, training=True)
    vit.drop_path_rate = 0.2                                           # ... and after fp8 training was switched on: refused at the forward
    with pytest.raises(NotImplementedError, match="fp8"):
        model(x)
    vit.disable_fp8()
    # the runtime: tables of another shape or dtype, a table without a training forward, a token-level backward of a pass under a table
    rt, (params, params16) = vit._rt, vit.flat_parameters()
    for bad in (torch.ones(2, 2, 3, device="cuda"), torch.ones(2, 2, 2, device="cuda", dtype=torch.float64), torch.ones(2, 2, 2)):
        with pytest.raises(ValueError):
            rt.forward(video, params, params16, training=True, drop_path=bad)
    good = torch.ones(2, 2, 2, device="cuda")
    with pytest.raises(ValueError):
        rt.forward(video, params, params16, training=False, drop_path=good)
    rt.forward(video, params, params16, training=True, rows_form=1, drop_path=good)
    with pytest.raises(NotImplementedError, match="token"):
        rt.backward(None, params, params16, torch.zeros_like(params), accumulate=False, dtokens=torch.zeros(2, 65, 128, device="cuda"))
