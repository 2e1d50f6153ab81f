"""Parameter groups and the learning-rate schedule on MI355X: nv_adamw_step_grouped against the per-group composition of the launch
WITHOUT groups (tests/param_groups_ref.py) bit for bit, FusedAdamW with param_groups against torch.optim.AdamW, and TrainStep with
groups / a schedule on the native, general, graph-replayed, resumed and data-parallel paths."""
import ctypes
import io
import os

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import param_groups_ref as R
import weights as W
from conftest import rel_err

pytestmark = pytest.mark.gpu
SIZE = dict(TRAINING_VIT_DIM=128, TRAINING_VIT_DEPTH=2, TRAINING_VIT_HEADS=2, TRAINING_VIT_MLP_DIM=256)
LR, WD = 1e-3, 0.1
LS_FOUND_INF, LS_SKIP, LS_STEPS = 2, 3, 5
BETAS = (0.9, 0.999)
# a span of the kernel is 2048 elements: boundaries inside a span, exactly on a span edge, several segments in one span
ALIGNED = (8, 2040, 2048, 8, 2056, 4104, 16)
# the same total, ends at offsets 1, 2 and 3 mod 4 (the temporal head's arena is packed like this: 12, 6, 4, 2, ...)
RAGGED = (12, 6, 4, 2, 2041, 2046, 9, 2051, 4093, 16)
LAYOUTS = {"aligned": ALIGNED, "ragged": RAGGED}
LRS, WDS = (1e-3, 2e-3, 4e-3), (0.0, 0.1, 0.1)          # a wrong group is a factor 2 in lr or the whole weight decay away


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


def layout(lens, n_groups=3):
    ends = [sum(lens[:i + 1]) for i in range(len(lens))]
    index = [i % n_groups for i in range(len(lens))]
    assert ends[-1] == 10280
    return ends, index


def same(a, b):
    return a.dtype == b.dtype and torch.equal(a.view(torch.int32 if a.element_size() == 4 else torch.int16), b.view(torch.int32 if b.element_size() == 4 else torch.int16))


def state_of(n, in_progress, seed):
    p = rnd(n, seed=seed).cuda()
    if not in_progress:
        return p, torch.zeros(n, device="cuda"), torch.zeros(n, device="cuda"), 1
    return p, rnd(n, seed=seed + 1, scale=0.05).cuda(), (rnd(n, seed=seed + 2, scale=0.05) ** 2).cuda(), 5


def assert_same_state(got, want, what):
    for name, a, b in zip("pmvs", got, want):
        if a is not None:
            assert same(a, b), (what, name, int((a != b).sum()))


# ------------------------------------------------------------------------------------------ 1. grouped == composed, bit for bit
@pytest.mark.parametrize("fmt", ["bf16", "fp16"])
@pytest.mark.parametrize("name", list(LAYOUTS))
def test_grouped_equals_the_composition_bit_for_bit(ops, name, fmt):
    from neurovit_amd import _cabi
    _cabi.set_operand_format(fmt)
    ends, index = layout(LAYOUTS[name])
    n = ends[-1]
    eg = R.element_groups(ends, index)
    seg = ops.AdamwSegments(ends, index, 3, n, "cuda")
    for g16 in (False, True):
        for shadow in (True, False):
            for blocks in (0, 3):
                for in_progress in (False, True):
                    p, m, v, step0 = state_of(n, in_progress, seed=3)
                    p16 = torch.zeros(n, dtype=ops.op16(), device="cuda") if shadow else None
                    for k in range(3):
                        grad = rnd(n, seed=20 + k, scale=0.1).cuda()
                        grad = grad.to(ops.op16()) if g16 else grad
                        want = R.compose_device(ops, p, grad, m, v, p16, step0 + k, eg, LRS, WDS, BETAS, 1e-8, 0.5, blocks)
                        ops.adamw_step_grouped(p, grad, m, v, p16, step0 + k, seg, LRS, WDS, BETAS, 1e-8, 0.5, blocks)
                        assert_same_state((p, m, v, p16), want, (name, fmt, g16, shadow, blocks, in_progress, k))
    # the groups are what moved the parameters: group 0's pair everywhere is far away
    p, m, v, _ = state_of(n, False, seed=3)
    q = p.clone()
    grad = rnd(n, seed=20, scale=0.1).cuda()
    ops.adamw_step_grouped(p, grad, m, v, None, 1, seg, LRS, WDS)
    ops.adamw_step(q, grad, torch.zeros_like(q), torch.zeros_like(q), None, 1, LRS[0], BETAS, 1e-8, WDS[0])
    for g in (1, 2):
        assert rel_err(p[eg.cuda() == g], q[eg.cuda() == g]) > 1e-4


# ------------------------------------------------------------------------------------------ 2. one group, one segment
def test_one_group_equals_the_launch_without_groups(ops):
    n = 10280
    seg = ops.AdamwSegments([n], [0], 1, n, "cuda")
    for g16, blocks in ((False, 0), (True, 0), (False, 3)):
        p, m, v, step0 = state_of(n, True, seed=7)
        q, mq, vq = p.clone(), m.clone(), v.clone()
        p16, q16 = torch.zeros(n, dtype=torch.bfloat16, device="cuda"), torch.zeros(n, dtype=torch.bfloat16, device="cuda")
        grad = rnd(n, seed=8, scale=0.1).cuda()
        grad = grad.bfloat16() if g16 else grad
        ops.adamw_step_grouped(p, grad, m, v, p16, step0, seg, [LR], [WD], BETAS, 1e-8, 1.0, blocks)
        ops.adamw_step(q, grad, mq, vq, q16, step0, LR, BETAS, 1e-8, WD, 1.0, blocks)
        assert_same_state((p, m, v, p16), (q, mq, vq, q16), (g16, blocks))


# ------------------------------------------------------------------------------------------ 3. a dynamic loss scale
@pytest.mark.parametrize("name", list(LAYOUTS))
def test_with_a_loss_scale_block_skipped_steps_change_nothing_and_applied_ones_equal_the_composition(ops, name):
    from neurovit_amd.optim import LossScaler
    ends, index = layout(LAYOUTS[name])
    n = ends[-1]
    eg = R.element_groups(ends, index)
    seg = ops.AdamwSegments(ends, index, 3, n, "cuda")
    sc = LossScaler("cuda", init_scale=1024.0)
    p, m, v, _ = state_of(n, False, seed=11)
    p16 = torch.zeros(n, dtype=torch.bfloat16, device="cuda")
    for k, overflow in enumerate((True, False, True, False, False)):       # (the very first step is skipped: the block's step count is 0 then)
        grad = (rnd(n, seed=30 + k, scale=0.1) * 1024.0).cuda()
        if overflow:
            sc.state[LS_FOUND_INF] = 1.0
        before = sc.state.clone()
        want = (p.clone(), m.clone(), v.clone(), p16.clone()) if overflow else \
            R.compose_device(ops, p, grad, m, v, p16, 99, eg, LRS, WDS, BETAS, 1e-8, 1.0, 0, scale_state=before)
        sc.update(LRS[0], BETAS)                                             # group 0's lr, as FusedAdamW passes it
        ops.adamw_step_grouped(p, grad, m, v, p16, 99, seg, LRS, WDS, BETAS, 1e-8, 1.0, 0, scale_state=sc.state)
        assert float(sc.state[LS_SKIP]) == float(overflow)
        assert_same_state((p, m, v, p16), want, (name, k, overflow))
    assert sc.steps_applied() == 3 and sc.steps_skipped() == 2


# ------------------------------------------------------------------------------------------ 4. a clipping coefficient that binds
@pytest.mark.parametrize("g16", [False, True])
def test_with_a_binding_clip_coefficient_equals_the_composition(ops, g16):
    ends, index = layout(RAGGED)
    n = ends[-1]
    eg = R.element_groups(ends, index)
    seg = ops.AdamwSegments(ends, index, 3, n, "cuda")
    p, m, v, step0 = state_of(n, True, seed=13)
    p16 = torch.zeros(n, dtype=torch.bfloat16, device="cuda")
    grad = rnd(n, seed=14, scale=0.1).cuda()
    st = torch.zeros(ops.GRAD_CLIP_FLOATS, device="cuda")
    ops.grad_sumsq(grad, st)
    ops.grad_clip_finish(st, 0.5 * float(grad.double().norm()))
    assert 0.49 < float(st[ops.GC_COEF]) < 0.51
    grad = grad.bfloat16() if g16 else grad
    want = R.compose_device(ops, p, grad, m, v, p16, step0, eg, LRS, WDS, BETAS, 1e-8, 1.0, 0, clip_state=st)
    unclipped = R.compose_device(ops, p, grad, m, v, p16, step0, eg, LRS, WDS, BETAS, 1e-8, 1.0, 0)
    ops.adamw_step_grouped(p, grad, m, v, p16, step0, seg, LRS, WDS, BETAS, 1e-8, 1.0, 0, clip_state=st)
    assert_same_state((p, m, v, p16), want, g16)
    assert not same(m, unclipped[1])


# ------------------------------------------------------------------------------------------ 5. nothing outside [0, count) is written
def test_guard_cells_tables_and_blocks_are_left_alone(ops):
    from neurovit_amd.optim import LossScaler
    ends, index = layout(RAGGED)
    n, pad, guard = ends[-1], 64, -12345.0
    seg = ops.AdamwSegments(ends, index, 3, n, "cuda")
    table = seg.table.clone()
    bufs = [torch.full((n + 2 * pad,), guard, device="cuda") for _ in range(4)]
    b16 = torch.full((n + 2 * pad,), guard, dtype=torch.bfloat16, device="cuda")
    p, grad, m, v = (b[pad:pad + n] for b in bufs)
    p16 = b16[pad:pad + n]
    p.copy_(rnd(n, seed=1)); grad.copy_(rnd(n, seed=2, scale=0.1)); m.zero_(); v.zero_()
    keep = grad.clone()
    clip = torch.zeros(ops.GRAD_CLIP_FLOATS, device="cuda")
    ops.grad_sumsq(grad, clip)
    ops.grad_clip_finish(clip, 1e9)
    clip0 = clip.clone()
    for blocks in (0, 3):
        ops.adamw_step_grouped(p, grad, m, v, p16, 1, seg, LRS, WDS, max_blocks=blocks, clip_state=clip)
    assert torch.equal(seg.table, table) and torch.equal(clip, clip0) and torch.equal(grad, keep)
    sc = LossScaler("cuda", init_scale=1.0)
    sc.update(LRS[0], BETAS)
    block = sc.state.clone()
    ops.adamw_step_grouped(p, grad, m, v, p16, 1, seg, LRS, WDS, scale_state=sc.state)
    assert torch.equal(sc.state, block)
    nseg = 12 * len(ends)
    assert torch.equal(seg.table[:nseg], table[:nseg])             # (behind the segments: the step sizes the launch formed for this step)
    for b in bufs + [b16]:
        assert (b[:pad] == guard).all().item() and (b[pad + n:] == guard).all().item()
    assert torch.equal(p16, p.bfloat16())


# ------------------------------------------------------------------------------------------ 6. a no-decay segment at rest stays put
def test_a_no_decay_segment_with_zero_gradients_and_moments_is_unchanged(ops):
    ends, index = layout(RAGGED)
    n = ends[-1]
    eg = R.element_groups(ends, index).cuda()
    seg = ops.AdamwSegments(ends, index, 3, n, "cuda")
    p = rnd(n, seed=5).cuda()
    start = p.clone()
    grad = torch.zeros(n, device="cuda")
    m, v = torch.zeros(n, device="cuda"), torch.zeros(n, device="cuda")
    for step in (1, 2):
        ops.adamw_step_grouped(p, grad, m, v, None, step, seg, LRS, WDS)
    assert same(p[eg == 0], start[eg == 0])                        # weight decay 0: bit for bit
    for g in (1, 2):                                               # weight decay 0.1: every element moved (towards zero)
        assert bool((p[eg == g].abs() < start[eg == g].abs()).all())
    assert not m.any().item() and not v.any().item()


# ------------------------------------------------------------------------------------------ 7. refusals
def test_every_refusal_returns_its_error_and_touches_nothing(ops):
    from neurovit_amd import _cabi
    lib = _cabi.lib
    ends, index = layout(ALIGNED)
    n = ends[-1]
    for bad_ends, bad_index, G, count in (([], [], 1, n), (list(range(4, 4 * 1026, 4)), [0] * 1025, 1, 4 * 1025), (ends, index, 0, n), (ends, index, 65, n),
                                          ([8, 8, n], [0, 1, 0], 3, n), ([16, 8, n], [0, 1, 0], 3, n), ([0, n], [0, 1], 3, n), (ends[:-1] + [n - 4], index, 3, n),
                                          (ends, index, 2, n), (ends, [-1] + index[1:], 3, n), ([5, 10], [0, 1], 2, 10)):
        with pytest.raises(RuntimeError, match="nv_adamw_segments_build"):
            ops.AdamwSegments(bad_ends, bad_index, G, count, "cuda")
    seg = ops.AdamwSegments(ends, index, 3, n, "cuda")
    big = [rnd(n + 8, seed=s).cuda() for s in range(4)]
    big[3].abs_()
    b16 = torch.zeros(n + 8, dtype=torch.bfloat16, device="cuda")
    keep = [b.clone() for b in big]
    p, grad, m, v = (b[:n] for b in big)
    p16 = b16[:n]

    def refused(*args, **kw):
        with pytest.raises(RuntimeError, match="nv_adamw_step_grouped"):
            ops.adamw_step_grouped(*args, **kw)

    refused(big[0][1:n + 1], grad, m, v, p16, 1, seg, LRS, WDS)                       # alignment of p, grad, m, v, the shadow
    refused(p, big[1][2:n + 2], m, v, p16, 1, seg, LRS, WDS)
    refused(p, grad, big[2][1:n + 1], v, p16, 1, seg, LRS, WDS)
    refused(p, grad, m, big[3][3:n + 3], p16, 1, seg, LRS, WDS)
    refused(p, grad, m, v, b16[1:n + 1], 1, seg, LRS, WDS)
    refused(p[:n - 2], grad[:n - 2], m[:n - 2], v[:n - 2], None, 1, seg, LRS, WDS)   # count no multiple of 4
    refused(p[:n - 4], grad[:n - 4], m[:n - 4], v[:n - 4], None, 1, seg, LRS, WDS)   # a table built for another count
    refused(p, grad, m, v, p16, 1, seg, LRS[:2], WDS[:2])                            # ... for another number of groups
    for bad in (-1e-3, float("nan"), float("inf")):
        refused(p, grad, m, v, p16, 1, seg, (LRS[0], bad, LRS[2]), WDS)
        refused(p, grad, m, v, p16, 1, seg, LRS, (WDS[0], WDS[1], bad))
    with pytest.raises(ValueError):
        ops.adamw_step_grouped(p, grad, m, v, p16, 1, seg, [LR] * 65, [WD] * 65)
    # a table the library did not build: a copy of a good one at another address
    class Copy:
        table = seg.table.clone()
    refused(p, grad, m, v, p16, 1, Copy, LRS, WDS)
    # through the C-ABI itself: null pointers, a wrong struct_size, G out of range, a released table
    tab = _cabi.AdamwGroups(ctypes.sizeof(_cabi.AdamwGroups), 3, seg.table.data_ptr())
    for i in range(3):
        tab.lr[i], tab.weight_decay[i] = LRS[i], WDS[i]
    stream = torch.cuda.current_stream().cuda_stream

    def call(pp=p.data_ptr(), gg=grad.data_ptr(), mm=m.data_ptr(), vv=v.data_ptr(), table=tab, step=1):
        return lib.nv_adamw_step_grouped(pp, gg, 0, mm, vv, p16.data_ptr(), n, step, None if table is None else ctypes.byref(table), 0.9, 0.999, 1e-8, 1.0, 0,
                                         None, None, stream)

    for kw in (dict(pp=None), dict(gg=None), dict(mm=None), dict(vv=None), dict(table=None), dict(step=0)):
        assert call(**kw) != 0 and "nv_adamw_step_grouped" in _cabi.last_error(), kw
    tab.struct_size -= 8
    assert call() != 0 and "struct_size" in _cabi.last_error()
    tab.struct_size += 8
    for G in (0, 65):
        tab.n_groups = G
        assert call() != 0
    tab.n_groups = 3
    tab.segments = None
    assert call() != 0
    tab.segments = seg.table.data_ptr()
    torch.cuda.synchronize()
    for b, k in zip(big, keep):
        assert torch.equal(b, k)
    assert not b16.any().item()
    assert call() == 0                                                               # and the same call with nothing wrong goes through
    assert lib.nv_adamw_segments_release(seg.table.data_ptr()) == 0
    assert call() != 0 and "nv_adamw_segments_build" in _cabi.last_error()
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------ models
def _model(fmt="bf16"):
    import neurovit_amd.NeuroEncoder as ne
    cfg = W.neuro_config(32, 8, DEVICE="cuda", TRAINING_LEARNING_RATE=LR, TRAINING_WEIGHT_DECAY=WD, TRAINING_VIT_OPERANDS=fmt, **SIZE)
    model = ne.NeuroEncoder(cfg)
    model.load_state_dict(W.make_tensors(W.vit_param_spec(**W.MICRO), 1, prefix="volume_encoder.vit3d."), strict=True)
    model.train()
    return model


def _vit(model):
    return model.volume_encoder.vit3d


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
RECIPE = dict(no_decay=True, layer_decay=0.5)


# ------------------------------------------------------------------------------------------ 8. FusedAdamW against the stock optimizer
def _against_stock(model, holder, batch, loss_of):
    """two steps of FusedAdamW on param_groups(model, 0.1, no_decay, layer_decay 0.5) against torch.optim.AdamW on the same groups, on
    a CPU copy fed the same gradients; the copy is resynchronised after each step (as test_fused_step_equals_stock_optimizer_step does)"""
    from neurovit_amd import param_groups, set_group_lrs
    from neurovit_amd.optim import FusedAdamW
    groups = param_groups(model, WD, no_decay=True, layer_decay=0.5)
    fused = FusedAdamW(groups, lr=LR, model=model)
    set_group_lrs(fused, LR)
    named = dict(model.named_parameters())
    copies = {n: torch.nn.Parameter(named[n].detach().cpu().clone()) for g in groups for n in g["names"]}
    stock = torch.optim.AdamW([{"params": [copies[n] for n in g["names"]], "lr": LR * g["lr_scale"], "weight_decay": g["weight_decay"]} for g in groups])
    assert fused.is_grouped(holder)
    worst = 0.0
    for _ in range(2):
        fused.zero_grad(set_to_none=True)
        loss_of(model, batch).backward()
        for n, c in copies.items():
            c.grad = named[n].grad.detach().cpu().clone()
        fused.step()
        stock.step()
        for n, c in copies.items():                       # per parameter: the small ones are not hidden behind the large
            err = rel_err(named[n], c)
            worst = max(worst, err)
            assert err <= 1e-6, (n, err)
        with torch.no_grad():
            for n, c in copies.items():
                c.copy_(named[n].detach().cpu())
    return worst


def test_fused_adamw_with_the_recipes_groups_equals_the_stock_optimizer():
    model = _model()
    x, y = _data(2)
    _against_stock(model, _vit(model), (x, y), lambda m, b: torch.nn.functional.cross_entropy(m(b[0]), b[1]))


def test_fused_adamw_with_groups_on_the_4d_models_temporal_head():
    import test_dp_gpu as tdp
    model = tdp._model4d()
    batch = (W.make_volume((2, 32, 32, 32, 4), 7).cuda(), torch.tensor([0, 1], device="cuda"))
    _against_stock(model, model._temporal_head, batch, lambda m, b: torch.nn.functional.cross_entropy(m(b[0]), b[1]))


# ------------------------------------------------------------------------------------------ 9. TrainStep with groups
def _replicate(ops, step, holder, batches):
    """one optimizer step per batch; after each, the update is rebuilt from the step's OWN raw gradient arena by the composition"""
    from neurovit_amd import _cabi
    opt = step.optimizer
    for k, batch in enumerate(batches):
        arena, shadow = holder.flat_parameters()
        m, v = opt.arena_state(holder)
        p0, m0, v0 = arena.detach().clone(), m.clone(), v.clone()
        s0 = None if shadow is None else shadow.clone()
        block = None if step.scaler is None else step.scaler.state.clone()      # (no overflow in these steps: as it is when the update reads it)
        step(*batch)
        grads = holder.flat_gradients().detach().clone()
        info = opt._arena_groups[id(holder)]
        eg = R.element_groups(info["ends"], info["index"], arena.numel())
        pairs = opt._arena_pairs(holder)[1]
        assert len(set(pairs)) > 1
        _cabi.set_operand_format(holder.operands)
        factor = 1.0 / step.static_scale if step.static_scale > 0 else 1.0
        want = R.compose_device(ops, p0, grads, m0, v0, s0, k + 1, eg, [a for a, _ in pairs], [b for _, b in pairs], BETAS, 1e-8, factor, 0,
                                scale_state=block, clip_state=None if step.clipper is None else step.clipper.state)
        assert_same_state((arena.detach(), m, v, shadow), want, k)
        if step.scaler is not None:
            assert not step.scaler.last_step_skipped()
        assert not same(arena.detach(), p0)


@BOTH_PATHS
@pytest.mark.parametrize("case", ["bf16", "fp16", "bf16-clip", "fp16-clip", "bf16-ema"])
def test_train_step_with_groups_replicated_from_the_raw_gradients(ops, path, case):
    fmt = case.split("-")[0]
    kw = dict(RECIPE)
    model = _model(fmt)
    if case.endswith("clip"):
        probe = _make_step(_model(fmt), fmt, max_grad_norm=1e9, **RECIPE)
        probe(*_data(20))
        kw["max_grad_norm"] = 0.5 * float(probe.last_grad_norm)
    if case.endswith("ema"):
        kw["ema_decay"] = 0.9
    step = _make_step(model, fmt, **kw)
    _replicate(ops, step, _vit(model), [_data(20), _data(21), _data(22)])
    assert step.last_fuse_update == 0 and step.last_path == path and step.optimizer._steps == 3
    assert step.last_lr == LR and len(step.optimizer.param_groups) == 8
    if case.endswith("clip"):
        assert float(step.last_clip_coef) <= 1.0
    if case.endswith("ema"):
        assert step.ema.num_updates == 3


def _run(batches, **kw):
    model = _model()
    step = _make_step(model, "bf16", **kw)
    for b in batches:
        step(*b)
    m, v = step.optimizer.arena_state(_vit(model))
    torch.cuda.synchronize()
    return _vit(model).flat_parameters()[0].detach().clone(), m.clone(), v.clone(), step


def test_groups_behind_the_graph_replayed_step_equal_the_eager_run(monkeypatch):
    monkeypatch.setenv("NEUROVIT_NATIVE_STEP", "1")
    batch = _data(9)
    eager = _run([batch] * 6, **RECIPE)
    monkeypatch.setenv("NEUROVIT_GRAPH_STEP", "1")
    graph = _run([batch] * 6, **RECIPE)
    assert len(graph[3]._graphs) == 1 and len(eager[3]._graphs) == 0
    for a, b in zip(eager[:3], graph[:3]):
        assert same(a, b)


# ------------------------------------------------------------------------------------------ 10. groups that are all alike change nothing
def test_groups_that_carry_one_pair_equal_the_default_step_bit_for_bit(monkeypatch):
    monkeypatch.setenv("NEUROVIT_NATIVE_STEP", "1")
    batches = [_data(7), _data(8), _data(9)]
    default = _run(batches)
    for kw in (dict(no_decay=False, layer_decay=None), dict(layer_decay=1.0)):
        other = _run(batches, **kw)
        assert other[3].last_fuse_update == default[3].last_fuse_update == 3 and other[3].last_path == "native"
        for a, b in zip(default[:3], other[:3]):
            assert same(a, b)
    assert len(other[3].optimizer.param_groups) == 4 and not other[3].optimizer.is_grouped()


# ------------------------------------------------------------------------------------------ 11. a schedule alone
def _schedule():
    from neurovit_amd import LRSchedule
    return LRSchedule(LR, 6, 2, "cosine", 1e-5)


def test_a_schedule_alone_equals_learning_rates_set_by_hand_and_keeps_every_mode(monkeypatch):
    monkeypatch.setenv("NEUROVIT_NATIVE_STEP", "1")
    batches = [_data(7), _data(8), _data(9), _data(10)]
    sched = _schedule()
    auto = _run(batches, lr_schedule=sched)
    assert auto[3].last_fuse_update == 3 and auto[3].last_path == "native" and auto[3].last_lr == sched.lr_at(4)
    model = _model()
    step = _make_step(model, "bf16")
    for k, b in enumerate(batches, start=1):
        for g in step.optimizer.param_groups:
            g["lr"] = sched.lr_at(k)
        step(*b)
        assert step.last_lr == sched.lr_at(k)
    m, v = step.optimizer.arena_state(_vit(model))
    for a, b in zip(auto[:3], (_vit(model).flat_parameters()[0].detach(), m, v)):
        assert same(a, b)
    constant = _run(batches)
    assert not same(auto[0], constant[0])


def _through_a_file(obj):
    buf = io.BytesIO()
    torch.save(obj, buf)
    buf.seek(0)
    return torch.load(buf, weights_only=True)


@BOTH_PATHS
@pytest.mark.parametrize("grouped", [False, True])
def test_a_resumed_scheduled_run_equals_the_straight_run(path, grouped):
    kw = dict(RECIPE) if grouped else {}
    batches = [_data(7), _data(8), _data(9), _data(10)]
    straight = _run(batches, lr_schedule=_schedule(), **kw)
    first = _run(batches[:2], lr_schedule=_schedule(), **kw)
    state = _through_a_file(first[3].state_dict())
    weights = _through_a_file(first[3].model.state_dict())
    assert ("groups" in state) == grouped
    model = _model()
    model.load_state_dict(weights, strict=True)
    step = _make_step(model, "bf16", lr_schedule=_schedule(), **kw)
    step.load_state_dict(state)
    for b in batches[2:]:
        step(*b)
    m, v = step.optimizer.arena_state(_vit(model))
    for a, b in zip(straight[:3], (_vit(model).flat_parameters()[0].detach(), m, v)):
        assert same(a, b)
    assert step.optimizer._steps == 4 and step.last_lr == _schedule().lr_at(4) and step.last_path == path
    assert step.last_fuse_update == (0 if grouped or path == "general" else 3)


# ------------------------------------------------------------------------------------------ 12. data parallel
def _dp_run():
    model = _model()
    step = _make_step(model, "bf16", n_buckets=3, lr_schedule=_schedule(), **RECIPE)
    for seed in (7, 8):
        step(*_data(seed))
    torch.cuda.synchronize()
    return _vit(model).flat_parameters()[0].detach().cpu().numpy(), step.last_path, step.last_lr


def _worker(rank, world, port, q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        torch.cuda.set_device(0)
        q.put((rank, _dp_run()))
    finally:
        dist.destroy_process_group()


def test_dp2_grouped_replicas_equal_each_other_and_the_single_process_run():
    """same batch on both ranks: (g + g) * 0.5 == g exactly, so the replicas equal the single-process grouped run bit for bit"""
    single = _dp_run()
    assert single[1] == "native"
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = 29600 + (os.getpid() % 1000)
    procs = [ctx.Process(target=_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = dict(q.get(timeout=240) for _ in procs)
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    assert res[0][1] == "general"                                # no native data-parallel plan with parameter groups
    assert (res[0][0] == res[1][0]).all() and (res[0][0] == single[0]).all()
    assert res[0][2] == res[1][2] == single[2]


# ------------------------------------------------------------------------------------------ 13. refusals
def test_refusals_on_the_device():
    from neurovit_amd import param_groups
    from neurovit_amd.optim import FusedAdamW
    from neurovit_amd.trainer import TrainStep
    model = _model()
    vit = _vit(model)
    start = vit.flat_parameters()[0].detach().clone()
    with pytest.raises(ValueError, match="overlap_optimizer"):
        TrainStep(model, overlap_optimizer=True, **RECIPE)
    groups = param_groups(model, WD)
    groups[1]["betas"] = (0.8, 0.999)
    with pytest.raises(ValueError, match="groups 0 and 1"):
        FusedAdamW(groups, lr=LR, model=model).step()
    groups = param_groups(model, WD)
    groups[0]["params"].append(groups[1]["params"][0])
    with pytest.raises(ValueError):
        FusedAdamW(groups, lr=LR, model=model)
    opt = FusedAdamW(param_groups(model, WD), lr=LR, model=model)
    opt.begin_step()
    with pytest.raises(ValueError, match="step_range"):
        opt.step_range(vit, 0, 64)
    grouped, plain = TrainStep(model, **RECIPE), TrainStep(_model())
    plain(*_data(3))
    m, v = plain.optimizer.arena_state(plain._vit)
    before = (m.clone(), v.clone(), plain.optimizer._steps)
    with pytest.raises(ValueError, match="parameter groups"):
        plain.load_state_dict(grouped.state_dict())
    assert same(m, before[0]) and same(v, before[1]) and plain.optimizer._steps == before[2]
    assert same(vit.flat_parameters()[0].detach(), start)
