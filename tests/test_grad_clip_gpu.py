"""Device-side gradient-norm clipping on MI355X: the squared-norm reduction (csrc/grad_clip.hip), the coefficient, the fused AdamW that
reads it, and TrainStep(max_grad_norm=...) on the native, general, 4D and data-parallel paths.  Expectations come from the host: the
restatement of clip_grad_norm_ pinned to torch in tests/test_grad_clip_cpu.py and the oracle's AdamW."""
import os

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import weights as W
from conftest import rel_err
from oracle import train_step
from test_grad_clip_cpu import norm_and_coef

pytestmark = pytest.mark.gpu
SIZE = dict(TRAINING_VIT_DIM=128, TRAINING_VIT_DEPTH=2, TRAINING_VIT_HEADS=2, TRAINING_VIT_MLP_DIM=256)
LR, WD = 1e-3, 1e-2
LS_UNSCALE, LS_FOUND_INF, LS_SKIP = 1, 2, 3


@pytest.fixture(scope="module")
def ops():
    from neurovit_amd import ops as _ops
    from neurovit_amd._cabi import require_gpu
    require_gpu()
    return _ops


@pytest.fixture(autouse=True)
def _bf16_format_afterwards():
    yield
    from neurovit_amd import _cabi
    _cabi.set_operand_format("bf16")


def rnd(*shape, seed=0, scale=1.0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale


def close(a, b, rel):
    a, b = float(a), float(b)
    return abs(a - b) <= rel * abs(b)


def host_norm(*xs):
    return float(sum((x.double().cpu() ** 2).sum() for x in xs).sqrt())


def offset_view(x, off):
    """a copy of x that starts `off` elements into an aligned allocation"""
    base = torch.zeros(x.numel() + off + 8, dtype=x.dtype, device="cuda")
    base[off:off + x.numel()].copy_(x)
    return base[off:off + x.numel()]


def device_norm(ops, bufs, ls=None, max_blocks=0, state=None):
    st = torch.zeros(ops.GRAD_CLIP_FLOATS, device="cuda") if state is None else state
    for b in bufs:
        ops.grad_sumsq(b, st, ls, max_blocks)
    sumsq = st[:2].clone().view(torch.float64)          # the running double, before finish clears it
    ops.grad_clip_finish(st, 1.0, 1.0, None)
    return st[ops.GC_TOTAL_NORM].clone(), sumsq


def loss_scale_state():
    from neurovit_amd.optim import LossScaler
    return LossScaler("cuda", init_scale=2.0 ** 10)


# ------------------------------------------------------------------------------------------ 1. the reduction
COUNTS = (1, 3, 4, 5, 255, 1024, 2049)
STRIDED = 20001          # with max_blocks = 2: 5000 16-byte pieces, 2048 per grid pass = three passes


def test_sumsq_fp32_every_count_and_alignment(ops):
    for count, blocks in [(c, 0) for c in COUNTS] + [(STRIDED, 2)]:
        x = rnd(count, seed=count)
        for off in range(4):
            got, _ = device_norm(ops, [offset_view(x.cuda(), off)], max_blocks=blocks)
            assert close(got, host_norm(x), 1e-6), (count, off, float(got), host_norm(x))


@pytest.mark.parametrize("fmt", ["bf16", "fp16"])
def test_sumsq_16bit_every_count_and_alignment(ops, fmt):
    from neurovit_amd import _cabi
    _cabi.set_operand_format(fmt)
    for count, blocks in [(c, 0) for c in COUNTS] + [(STRIDED, 2)]:
        x = rnd(count, seed=count).to(ops.op16())
        for off in range(8):
            got, _ = device_norm(ops, [offset_view(x.cuda(), off)], max_blocks=blocks)
            assert close(got, host_norm(x), 1e-6), (fmt, count, off, float(got), host_norm(x))


def test_sumsq_is_bit_reproducible_and_accumulates_over_buffers(ops):
    x = rnd(300001, seed=1).cuda()                       # 74 workgroups
    (n1, s1), (n2, s2) = device_norm(ops, [x]), device_norm(ops, [x])
    assert torch.equal(s1.view(torch.int64), s2.view(torch.int64)) and torch.equal(n1, n2)
    (_, s3), (_, s4) = device_norm(ops, [x], max_blocks=5), device_norm(ops, [x], max_blocks=5)
    assert torch.equal(s3.view(torch.int64), s4.view(torch.int64))
    assert close(s1, host_norm(x) ** 2, 1e-12) and close(s3, host_norm(x) ** 2, 1e-12)      # the double itself: ~n 2^-53
    a, b, c = rnd(2049, seed=2).cuda(), rnd(5, seed=3).cuda(), rnd(70001, seed=4).cuda()
    three, _ = device_norm(ops, [a, b, c])
    one, _ = device_norm(ops, [torch.cat([a, b, c])])
    assert close(three, one, 1e-6) and close(three, host_norm(a, b, c), 1e-6)
    # finish cleared the running sum: the same block is ready for the next step
    st = torch.zeros(ops.GRAD_CLIP_FLOATS, device="cuda")
    device_norm(ops, [a], state=st)
    again, _ = device_norm(ops, [b], state=st)
    assert close(again, host_norm(b), 1e-6)


def test_sumsq_of_finite_fp32_gradients_is_finite(ops):
    """values whose squares (1e30) or whose sum of squares (1000 x 9e36) overflow fp32"""
    sc = loss_scale_state()
    got, _ = device_norm(ops, [torch.full((1000,), 3e18, device="cuda")], ls=sc.state)
    assert close(got, host_norm(torch.full((1000,), 3e18)), 1e-6)
    one = torch.zeros(777, device="cuda")
    one[333] = 1e30
    got1, _ = device_norm(ops, [one], ls=sc.state)
    assert close(got1, 1e30, 1e-6)
    assert float(sc.state[LS_FOUND_INF]) == 0.0


@pytest.mark.parametrize("bad", [float("inf"), float("-inf"), float("nan")])
def test_sumsq_raises_found_inf_wherever_the_element_sits(ops, bad):
    from neurovit_amd import _cabi
    count = 1030                     # one element into an aligned allocation: 3 head elements, 256 pieces, 3 tail elements
    for where in (1, 500, count - 1):
        x = rnd(count, seed=9)
        x[where] = bad
        sc = loss_scale_state()
        got, _ = device_norm(ops, [offset_view(x.cuda(), 1)], ls=sc.state)
        assert not torch.isfinite(got).item() and float(sc.state[LS_FOUND_INF]) == 1.0, where
    # a flag that is already up stays up after a clean buffer
    device_norm(ops, [rnd(64, seed=1).cuda()], ls=sc.state)
    assert float(sc.state[LS_FOUND_INF]) == 1.0
    _cabi.set_operand_format("fp16")
    count = 1037                     # 1038 16-bit elements, three elements in: 5 head elements, 129 pieces, 1 tail element
    for where in (2, 600, count):
        x = rnd(count + 1, seed=10).half()
        x[where] = bad
        sc = loss_scale_state()
        got, _ = device_norm(ops, [offset_view(x.cuda(), 3)], ls=sc.state)
        assert not torch.isfinite(got).item() and float(sc.state[LS_FOUND_INF]) == 1.0, where


def test_nothing_outside_the_clip_block_is_written(ops):
    guard, n = 64, ops.GRAD_CLIP_FLOATS
    area = torch.full((guard + n + guard,), -12345.0, device="cuda")
    st = area[guard:guard + n]
    st.zero_()
    big = rnd(2048 * 4096 + 4099, seed=5).cuda()       # the largest grid: every partial slot is written
    keep = big.clone()
    for x in (big[:1], big[:2049], big[3:], big):
        ops.grad_sumsq(x, st, None, 0)
    ops.grad_clip_finish(st, 1.0, 1.0, None)
    assert close(st[ops.GC_TOTAL_NORM], host_norm(big[:1], big[:2049], big[3:], big), 1e-6)
    assert (area[:guard] == -12345.0).all().item() and (area[guard + n:] == -12345.0).all().item()
    assert torch.equal(big, keep)


# ------------------------------------------------------------------------------------------ 2. the coefficient
def test_coefficient_cases(ops):
    x = torch.tensor([3.0, 0.0, -4.0], device="cuda")                  # norm 5
    st = torch.zeros(ops.GRAD_CLIP_FLOATS, device="cuda")
    for max_norm, grad_scale in ((2.5, 1.0), (10.0, 1.0), (5.0, 1.0), (2.5, -0.25), (1.0, 1e-3)):
        ops.grad_sumsq(x, st)
        ops.grad_clip_finish(st, max_norm, grad_scale)
        want_t, want_c = norm_and_coef([x], max_norm, grad_scale)
        assert close(st[ops.GC_TOTAL_NORM], want_t, 1e-6) and close(st[ops.GC_COEF], want_c, 1e-6)
        if max_norm / (float(want_t) + 1e-6) >= 1:
            assert float(st[ops.GC_COEF]) == 1.0                        # exactly
        else:
            assert float(st[ops.GC_COEF]) < 1.0
        assert float(st[:2].view(torch.float64)) == 0.0                 # the running sum is cleared
    x[1] = float("inf")
    ops.grad_sumsq(x, st)
    ops.grad_clip_finish(st, 2.5, 1.0)
    assert torch.isinf(st[ops.GC_TOTAL_NORM]).item() and float(st[ops.GC_COEF]) == 0.0
    x[1] = float("nan")
    ops.grad_sumsq(x, st)
    ops.grad_clip_finish(st, 2.5, 1.0)
    assert torch.isnan(st[ops.GC_TOTAL_NORM]).item() and torch.isnan(st[ops.GC_COEF]).item()


def test_coefficient_unscales_by_what_the_update_wrote(ops):
    """growth_interval 1: the update that follows the sum doubles LS_SCALE, so 1 / LS_SCALE is NOT the factor of these gradients"""
    from neurovit_amd.optim import LossScaler
    sc = LossScaler("cuda", init_scale=1024.0, growth_interval=1)
    st = torch.zeros(ops.GRAD_CLIP_FLOATS, device="cuda")
    x = torch.tensor([3.0, 4.0], device="cuda") * 1024.0
    ops.grad_sumsq(x, st, sc.state)
    sc.update(LR, (0.9, 0.999))
    assert float(sc.state[0]) == 2048.0 and float(sc.state[LS_UNSCALE]) == 1.0 / 1024.0
    ops.grad_clip_finish(st, 2.5, 0.5, sc.state)
    want_t, want_c = norm_and_coef([x], 2.5, 0.5 / 1024.0)
    assert close(want_t, 2.5, 1e-6)
    assert close(st[ops.GC_TOTAL_NORM], want_t, 1e-6) and close(st[ops.GC_COEF], want_c, 1e-6)


# ------------------------------------------------------------------------------------------ 3. AdamW with the coefficient
def test_clipped_adamw_matches_the_oracle_fed_clipped_gradients(ops):
    """coefficients 0.5, 1, 0.7 on consecutive steps (Adam is invariant to a UNIFORM gradient scale: a constant coefficient would
    move the parameters below the gate - the moments, gated here at every step, are what cannot hide it)"""
    n = 4096 + 8
    p0 = rnd(n, seed=1)
    params = {"w": p0.clone()}
    opt = train_step.AdamW(params, lr=LR, weight_decay=WD)
    p, m, v = p0.clone().cuda(), torch.zeros(n, device="cuda"), torch.zeros(n, device="cuda")
    p16 = torch.empty(n, dtype=torch.bfloat16, device="cuda")
    st = torch.zeros(ops.GRAD_CLIP_FLOATS, device="cuda")
    for step, target in enumerate((0.5, 2.0, 0.7), start=1):
        g = rnd(n, seed=10 + step, scale=0.1)
        max_norm = target * host_norm(g)
        want_t, want_c = norm_and_coef([g], max_norm)
        assert close(want_c, min(target, 1.0), 1e-4)
        opt.step({"w": g * want_c})
        ops.grad_sumsq(g.cuda(), st)
        ops.grad_clip_finish(st, max_norm)
        ops.adamw_step(p, g.cuda(), m, v, p16, step, LR, weight_decay=WD, clip_state=st)
        assert close(st[ops.GC_COEF], want_c, 1e-6)
        for name, got, want in (("p", p, params["w"]), ("m", m, opt.m["w"]), ("v", v, opt.v["w"])):
            assert rel_err(got, want) <= 1e-6, (name, step, rel_err(got, want))
        assert torch.equal(p16.cpu(), p.cpu().to(torch.bfloat16))


def test_clipped_adamw_reads_16bit_gradients_and_a_capped_grid_bit_for_bit(ops):
    n = 8192 + 16
    p0 = rnd(n, seed=4)
    g = rnd(n, seed=5, scale=0.1).to(torch.bfloat16).float()        # fp32 storage, bf16-representable values
    st = torch.zeros(ops.GRAD_CLIP_FLOATS, device="cuda")
    ops.grad_sumsq(g.cuda(), st)
    ops.grad_clip_finish(st, 0.3 * host_norm(g), 0.5)                # norm of 0.5 g: coefficient 0.6
    assert close(st[ops.GC_COEF], 0.6, 1e-4)
    outs = []
    for grad, blocks in ((g.cuda(), 0), (g.cuda().bfloat16(), 0), (g.cuda().bfloat16(), 3), (g.cuda(), 3)):
        p, m, v = p0.clone().cuda(), torch.zeros(n, device="cuda"), torch.zeros(n, device="cuda")
        p16 = torch.empty(n, dtype=torch.bfloat16, device="cuda")
        ops.adamw_step(p, grad, m, v, p16, 1, LR, weight_decay=WD, grad_scale=0.5, max_blocks=blocks, clip_state=st)
        outs.append((p, m, v, p16))
    for other in outs[1:]:
        for a, b in zip(outs[0], other):
            assert torch.equal(a, b)
    # and it is the coefficient that was applied: m = (1 - beta1) * 0.5 * coef * g
    assert rel_err(outs[0][1], 0.1 * 0.5 * float(st[ops.GC_COEF]) * g) <= 1e-6


# ------------------------------------------------------------------------------------------ TrainStep
def _model(fmt="bf16"):
    import neurovit_amd.NeuroEncoder as ne
    cfg = W.neuro_config(32, 8, DEVICE="cuda", TRAINING_LEARNING_RATE=LR, TRAINING_WEIGHT_DECAY=WD, TRAINING_VIT_OPERANDS=fmt, **SIZE)
    model = ne.NeuroEncoder(cfg)
    model.load_state_dict(W.make_tensors(W.vit_param_spec(**W.MICRO), 1, prefix="volume_encoder.vit3d."), strict=True)
    model.train()
    return model


def _data(seed, B=2):
    return W.make_volume((B, 32, 32, 32), seed).cuda(), (torch.arange(B) % 2).cuda()


def _make_step(model, fmt, **kw):
    from neurovit_amd.optim import LossScaler
    from neurovit_amd.trainer import TrainStep
    step = TrainStep(model, **kw)
    if fmt == "fp16":
        assert step.scaler is not None
        step.scaler = LossScaler("cuda", init_scale=2.0 ** 10)      # (the default 65536 may skip the first steps: GradScaler's own behaviour)
    return step


@pytest.fixture
def path(request, monkeypatch):
    monkeypatch.setenv("NEUROVIT_NATIVE_STEP", "1" if request.param == "native" else "0")
    return request.param


BOTH_PATHS = pytest.mark.parametrize("path", ["native", "general"], indirect=True)


# ------------------------------------------------------------------------------------------ 4. a clip that does not bind
@BOTH_PATHS
@pytest.mark.parametrize("fmt", ["bf16", "fp16"])
def test_clip_that_does_not_bind_changes_no_bit(path, fmt):
    outs = []
    for kw in (dict(fuse_update=0), dict(max_grad_norm=1e9)):
        model = _model(fmt)
        vit = model.volume_encoder.vit3d
        step = _make_step(model, fmt, **kw)
        for seed in (7, 8, 9):
            step(*_data(seed))
        assert step.last_path == path
        m, v = step.optimizer.arena_state(vit)
        outs.append((vit.flat_parameters()[0].clone(), m.clone(), v.clone(), step))
    for a, b in zip(outs[0][:3], outs[1][:3]):
        assert torch.equal(a, b)
    clipped = outs[1][3]
    assert float(clipped.last_clip_coef) == 1.0 and 0.0 < float(clipped.last_grad_norm) < 1e9
    if fmt == "fp16":
        assert clipped.scaler.steps_applied() == outs[0][3].scaler.steps_applied() == 3


# ------------------------------------------------------------------------------------------ 5. a clip that binds
def _first_norm(make_model, fmt, batches, **kw):
    """norm of the first optimizer step, measured by a throw-away run with a bound that cannot bind"""
    step = _make_step(make_model(), fmt, max_grad_norm=1e9, **kw)
    for b in batches:
        step(*b)
    return float(step.last_grad_norm)


def _replicate(step, holder, windows, factor_of, lr=LR, expect_binding_first=True):
    """Run `windows` (lists of micro-batches, one optimizer step each); after each, rebuild the update on the host from the step's OWN
    raw gradient arena: norm and coefficient by the restatement, AdamW by the oracle on g * factor * coef."""
    opt = step.optimizer
    applied = 0
    for w, batches in enumerate(windows):
        arena = holder.flat_parameters()[0]
        m, v = opt.arena_state(holder)
        p0, m0, v0 = arena.detach().cpu().clone(), m.cpu().clone(), v.cpu().clone()
        for b in batches:
            step(*b)
        g = holder.flat_gradients().detach().cpu().clone()
        factor = factor_of(step)
        want_t, want_c = norm_and_coef([g], step.max_grad_norm, factor)
        assert close(step.last_grad_norm, want_t, 1e-6), (w, float(step.last_grad_norm), float(want_t))
        assert close(step.last_clip_coef, want_c, 1e-6), (w, float(step.last_clip_coef), float(want_c))
        if w == 0 and expect_binding_first:
            assert float(step.last_clip_coef) < 1.0
        ref = train_step.AdamW({"w": p0}, lr=lr, weight_decay=WD)
        ref.m["w"], ref.v["w"], ref.t = m0, v0, applied
        ref.step({"w": g * factor * want_c})
        applied += 1
        for name, got, want in (("p", arena, ref.params["w"]), ("m", m, ref.m["w"]), ("v", v, ref.v["w"])):
            assert rel_err(got, want) <= 2e-6, (name, w, rel_err(got, want))
    return applied


@BOTH_PATHS
@pytest.mark.parametrize("case", ["bf16", "fp16-dynamic", "static-scale", "accumulate-2"])
def test_binding_clip_replicated_from_the_raw_gradients(path, case):
    fmt = "fp16" if case == "fp16-dynamic" else "bf16"
    kw = dict(loss_scale=1024.0) if case == "static-scale" else dict(accumulation_steps=2) if case == "accumulate-2" else {}
    per = 2 if case == "accumulate-2" else 1
    windows = [[_data(20 + per * w + i) for i in range(per)] for w in range(3)]
    max_norm = 0.5 * _first_norm(lambda: _model(fmt), fmt, windows[0], **kw)
    model = _model(fmt)
    vit = model.volume_encoder.vit3d
    step = _make_step(model, fmt, max_grad_norm=max_norm, **kw)

    def factor_of(s):
        if s.scaler is not None:
            return float(s.scaler.state[LS_UNSCALE])            # 1 / (the scale these gradients carry), as the update wrote it
        return 1.0 / s.static_scale if s.static_scale > 0 else 1.0

    _replicate(step, vit, windows, factor_of)
    assert step.last_path == path
    assert step.optimizer._steps == 3
    if case == "static-scale":
        assert close(host_norm(vit.flat_gradients()), 1024.0 * float(step.last_grad_norm), 1e-5)      # the arena keeps the raw, still scaled gradients
    if case != "fp16-dynamic":
        return
    # an inf in the gradient arena: the summing pass is the overflow check - the update is skipped, the scale backed off
    assert step.scaler.steps_applied() == 3 and step.scaler.steps_skipped() == 0
    arena = vit.flat_parameters()[0]
    m, v = step.optimizer.arena_state(vit)
    before = (arena.clone(), m.clone(), v.clone())
    scale = step.scaler.get_scale()
    vit._grad_view(10).view(-1)[5] = float("inf")                            # (inside a parameter: the next backward pass overwrites it)
    step.optimizer.step(grad_scale=1.0, scaler=step.scaler, clip=step.clipper)
    assert step.scaler.last_step_skipped() and step.scaler.get_scale() == 0.5 * scale
    assert step.scaler.steps_applied() == 3 and step.scaler.steps_skipped() == 1
    assert not torch.isfinite(step.last_grad_norm).item()
    for a, b in zip(before, (arena, m, v)):
        assert torch.equal(a, b)
    step(*_data(31))                                                         # and the next step is applied again
    assert not step.scaler.last_step_skipped() and torch.isfinite(step.last_grad_norm).item()
    assert not torch.equal(before[0], arena)


# ------------------------------------------------------------------------------------------ 6. the 4D model: only the temporal head's arena is live
def test_binding_clip_on_the_4d_models_temporal_head():
    import test_dp_gpu as tdp

    def batch(seed):
        return W.make_volume((2, 32, 32, 32, 4), seed).cuda(), torch.tensor([0, 1], device="cuda")

    windows = [[batch(7)], [batch(8)]]
    max_norm = 0.5 * _first_norm(tdp._model4d, "bf16", windows[0])
    model = tdp._model4d()
    step = _make_step(model, "bf16", max_grad_norm=max_norm)
    _replicate(step, model._temporal_head, windows, lambda s: 1.0, lr=1e-2)
    assert step.last_path == "general"


def test_norm_counts_parameters_only_on_a_vit_without_projection():
    """heads == 1 with dim_head == dim: the engine's to_out slots are constants outside the optimizer, and what the backward pass
    writes into their gradient slots is no gradient of the model - clip_grad_norm_(m.parameters()) does not see it"""
    from neurovit_amd.optim import FusedAdamW, GradClipper
    from neurovit_amd.vit_3d import ViT
    from oracle import ref_cpu
    m = ViT(**W.NOPROJ).cuda()
    m.load_state_dict(W.make_tensors(W.vit_param_spec(**W.NOPROJ), 71), strict=True)
    m.train()
    S = W.NOPROJ["image_size"]
    video = ref_cpu.fmri_to_video(W.make_volume((3, S, S, S), 72)).cuda()
    opt = FusedAdamW(m.parameters(), lr=LR, weight_decay=WD, model=m)
    torch.nn.functional.cross_entropy(m(video), torch.tensor([0, 1, 0], device="cuda")).backward()
    grads = [q.grad.detach().cpu().clone() for q in m.parameters()]
    assert m._phantom
    clip = GradClipper("cuda", 0.5 * host_norm(*grads))
    opt.step(clip=clip)
    want_t, want_c = norm_and_coef(grads, clip.max_norm)
    assert close(clip.total_norm, want_t, 1e-6) and close(clip.coef, want_c, 1e-6) and float(clip.coef) < 1.0
    arena = m.flat_parameters()[0]
    for o, const in m._phantom:                                   # and the constants survive the clipped step
        assert torch.equal(arena[o:o + const.numel()], const)


# ------------------------------------------------------------------------------------------ 7. data parallel
def _dp_run(max_norm, comm):
    model = _model()
    step = _make_step(model, "bf16", max_grad_norm=max_norm, n_buckets=3, grad_comm_dtype=comm)
    out = []
    for seed in (7, 8):
        step(*_data(seed))
        out.append((float(step.last_grad_norm), float(step.last_clip_coef)))
    torch.cuda.synchronize()
    red = None
    if step.sync is not None and not step.sync.write_back:
        red = step.sync.reduced_buffer().float().cpu().numpy()
    return model.volume_encoder.vit3d.flat_parameters()[0].detach().cpu().numpy(), out, red, step.last_path


def _worker(rank, world, port, max_norm, q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        torch.cuda.set_device(0)
        q.put((rank, _dp_run(max_norm, torch.float32), _dp_run(max_norm, torch.bfloat16)))      # by value (numpy / floats)
    finally:
        dist.destroy_process_group()


def test_dp2_clipped_replicas_equal_each_other_and_the_single_process_run():
    """same batch on both ranks: (g + g) * 0.5 == g and sqrt(4 s) * 0.5 == sqrt(s) exactly, so with fp32 messages norm, coefficient and
    parameters equal the single-process clipped run bit for bit; with 16-bit messages the replicas equal each other and the norm is
    that of the reduced 16-bit buffer"""
    single = _dp_run(1e9, torch.float32)
    max_norm = 0.5 * single[1][0][0]
    single = _dp_run(max_norm, torch.float32)
    assert single[1][0][1] < 1.0 and single[3] == "native"
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = 29600 + (os.getpid() % 1000)
    procs = [ctx.Process(target=_worker, args=(r, 2, port, max_norm, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = {rank: (f32, b16) for rank, f32, b16 in (q.get(timeout=240) for _ in procs)}
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    (p0, n0, _, path0), (p1, n1, _, _) = res[0][0], res[1][0]
    assert path0 == "general"                                   # no native data-parallel plan under clipping
    assert (p0 == p1).all() and n0 == n1
    assert (p0 == single[0]).all() and n0 == single[1]
    (q0, m0, red0, _), (q1, m1, red1, _) = res[0][1], res[1][1]
    assert (q0 == q1).all() and m0 == m1 and (red0 == red1).all()
    want_t, want_c = norm_and_coef([torch.from_numpy(red0)], max_norm, 0.5)
    assert close(m0[-1][0], want_t, 1e-6) and close(m0[-1][1], want_c, 1e-6)
    assert m0[0][1] < 1.0


# ------------------------------------------------------------------------------------------ 8. refusals
def test_refusals():
    from neurovit_amd.trainer import TrainStep
    model = _model()
    with pytest.raises(AssertionError):
        TrainStep(model, max_grad_norm=1.0, overlap_optimizer=True)
    for bad in (0.0, -1.0, float("inf"), float("nan")):
        with pytest.raises(ValueError):
            TrainStep(model, max_grad_norm=bad)
