"""Parameter groups and the learning-rate schedule without a GPU: the segment builder, param_groups, LRSchedule, the Trainer's config
parsing, the refusals that come before any device work, the C boundary, and the proof of the tests' own reference - the per-group
composition of tests/param_groups_ref.py against torch.optim.AdamW with real parameter groups."""
import math
import os
import tempfile

import pytest
import torch

import param_groups_ref as R
import weights as W
from conftest import rel_err

SIZE = dict(TRAINING_VIT_DIM=128, TRAINING_VIT_DEPTH=2, TRAINING_VIT_HEADS=2, TRAINING_VIT_MLP_DIM=256)
ENC = "volume_encoder.vit3d."


def rnd(*shape, seed=0, scale=1.0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale


def _cpu_model(**extra):
    import neurovit_amd.NeuroEncoder as ne
    return ne.NeuroEncoder(W.neuro_config(32, 8, DEVICE="cpu", **dict(SIZE, **extra)))


def _cpu_model4d():
    import neurovit_amd.NeuroEncoder as ne
    with tempfile.TemporaryDirectory() as td:
        torch.save(dict(W.make_tensors(W.vit_param_spec(**W.MICRO), 1, prefix=ENC)), os.path.join(td, "c.pth"))
        cfg = W.neuro_config(32, 8, dim=4, DEVICE="cpu", GLOBAL_BASE_PATH=td, BEST_MODEL_PATH="c.pth", **SIZE)
        return ne.NeuroEncoder(cfg)


# ------------------------------------------------------------------------------------------ 1. the reference of the GPU tests
def test_composition_equals_torch_adamw_with_parameter_groups():
    """three steps, three groups (lr a factor 2 apart, weight decay 0 / 0.1), ragged boundaries: compose_host against the stock
    optimizer at the gate of test_fused_step_equals_stock_optimizer_step"""
    lens, groups = (12, 6, 4, 2, 2041, 2047, 9), (0, 1, 2, 1, 0, 2, 1)
    lrs, wds = (1e-3, 2e-3, 4e-3), (0.1, 0.0, 0.1)
    ends = [sum(lens[:i + 1]) for i in range(len(lens))]
    eg = R.element_groups(ends, groups)
    n = ends[-1]
    start = rnd(n, seed=1)
    pieces = [torch.nn.Parameter(start[e - k:e].clone()) for e, k in zip(ends, lens)]
    stock = torch.optim.AdamW([{"params": [q for q, g in zip(pieces, groups) if g == k], "lr": lrs[k], "weight_decay": wds[k]} for k in range(3)])
    p, m, v = start.clone(), torch.zeros(n), torch.zeros(n)
    for t in range(3):
        grad = rnd(n, seed=10 + t, scale=0.1)
        for q, e, k in zip(pieces, ends, lens):
            q.grad = grad[e - k:e].clone()
        stock.step()
        p, m, v = R.compose_host(p, grad, m, v, t, eg, lrs, wds)
        want = torch.cat([q.detach() for q in pieces])
        want_m = torch.cat([stock.state[q]["exp_avg"] for q in pieces])
        want_v = torch.cat([stock.state[q]["exp_avg_sq"] for q in pieces])
        for name, got, ref in (("p", p, want), ("m", m, want_m), ("v", v, want_v)):
            assert rel_err(got, ref) <= 1e-6, (name, t, rel_err(got, ref))
        for g in range(3):                              # per group, so that no group hides behind another
            assert rel_err(p[eg == g], want[eg == g]) <= 1e-6, (g, t)
    # and the groups matter: group 0's pair everywhere is far outside the gate
    q, _, _ = R.compose_host(start, grad, torch.zeros(n), torch.zeros(n), 0, torch.zeros(n, dtype=torch.int64), lrs[:1], wds[:1])
    r, _, _ = R.compose_host(start, grad, torch.zeros(n), torch.zeros(n), 0, eg, lrs, wds)
    assert rel_err(q, r) > 1e-4


# ------------------------------------------------------------------------------------------ 2. the segment builder
def _check_cover(ends, index, total):
    assert ends[-1] == total and all(a < b for a, b in zip([0] + ends, ends))
    assert all(a != b for a, b in zip(index, index[1:]))            # adjacent equal groups are merged


def test_segments_plain_cases():
    from neurovit_amd.optim import arena_segments
    assert arena_segments([0, 8, 16], [8, 8, 8], 24, [0, 0, 0]) == ([24], [0])
    assert arena_segments([0, 8, 16], [8, 8, 8], 24, [0, 1, 0]) == ([8, 16, 24], [0, 1, 0])
    assert arena_segments([0, 8, 16], [5, 3, 8], 32, [0, 1, 1]) == ([8, 32], [0, 1])        # gaps join the entry in front of them
    assert arena_segments([8, 16], [8, 8], 24, [1, 0]) == ([16, 24], [1, 0])                # what lies in front of the first joins the first
    assert arena_segments([0, 12, 18, 22], [12, 6, 4, 2], 24, [0, 1, 0, 1]) == ([12, 18, 22, 24], [0, 1, 0, 1])
    assert arena_segments([0, 4, 4], [4, 0, 4], 8, [0, 1, 0]) == ([8], [0])                 # an empty entry leaves no segment
    for bad in (([], [], 0, []), ([0, 4], [8, 4], 12, [0, 1]), ([0], [8], 4, [0]), ([0, 8], [8], 16, [0, 1])):
        with pytest.raises(ValueError):
            arena_segments(*bad)


def _holder_segments(holder, by_entry):
    from neurovit_amd.optim import arena_segments
    holder.flat_parameters()
    total = holder._arena.numel()
    ends, index = arena_segments(holder._offsets, holder._numels, total, by_entry)
    _check_cover(ends, index, total)
    eg = R.element_groups(ends, index, total)
    for o, k, g in zip(holder._offsets, holder._numels, by_entry):
        assert (eg[o:o + k] == g).all()                            # every parameter lies in its own group, whole
    return ends, index, eg


def test_segments_of_the_micro_vit_the_vit_without_projection_and_the_temporal_head():
    from neurovit_amd.vit_3d import ViT
    vit = _cpu_model().volume_encoder.vit3d
    by_entry = [int(p.ndim <= 1) for p in vit.arena_parameters()]
    ends, index, eg = _holder_segments(vit, by_entry)
    assert len(ends) < len(by_entry)                               # bias + LayerNorm runs were merged
    assert all(o % 8 == 0 for o in vit._offsets)
    # alignment padding belongs to the entry in front of it
    for i, (o, k) in enumerate(zip(vit._offsets, vit._numels)):
        nxt = vit._offsets[i + 1] if i + 1 < len(vit._offsets) else vit._arena.numel()
        assert (eg[o + k:nxt] == by_entry[i]).all()
    # a ViT without output projection: the constant slots are no parameter and join the segment in front of them
    noproj = ViT(**W.NOPROJ)
    plist = noproj.arena_parameters()
    assert noproj._phantom
    by_entry = [i % 3 for i in range(len(plist))]
    _, _, eg = _holder_segments(noproj, by_entry)
    for o, const in noproj._phantom:
        before = max(i for i, po in enumerate(noproj._offsets) if po < o)
        assert (eg[o:o + const.numel()] == by_entry[before]).all()
    # the temporal head: densely packed, boundaries at any element
    head = _cpu_model4d()._temporal_head
    plist = head.arena_parameters()
    by_entry = [int(p.ndim <= 1) for p in plist]
    ends, index, _ = _holder_segments(head, by_entry)
    assert any(e % 4 for e in ends[:-1]) and head._arena.numel() % 4 == 0


# ------------------------------------------------------------------------------------------ 3. param_groups
def _names_by_param(model):
    return {id(p): n for n, p in model.named_parameters()}


def test_param_groups_cover_the_trainable_parameters_once_and_name_the_no_decay_set():
    from neurovit_amd import param_groups
    from neurovit_amd.optim import in_no_decay_set
    model = _cpu_model()
    names = _names_by_param(model)
    groups = param_groups(model, 0.1)
    assert len(groups) == 2
    seen = [id(p) for g in groups for p in g["params"]]
    assert len(seen) == len(set(seen)) and set(seen) == {id(p) for p in model.parameters() if p.requires_grad}
    no_decay = {names[id(p)] for g in groups if g["weight_decay"] == 0.0 for p in g["params"]}
    decay = {names[id(p)] for g in groups if g["weight_decay"] == 0.1 for p in g["params"]}
    assert ENC + "pos_embedding" in no_decay and ENC + "cls_token" in no_decay
    assert ENC + "to_patch_embedding.2.bias" in no_decay and ENC + "mlp_head.0.weight" in no_decay and ENC + "transformer.layers.1.0.norm.weight" in no_decay
    assert ENC + "to_patch_embedding.2.weight" in decay and ENC + "mlp_head.1.weight" in decay and ENC + "transformer.layers.0.0.to_qkv.weight" in decay
    for n, p in model.named_parameters():
        assert (n in no_decay) == in_no_decay_set(n, p) == (p.ndim <= 1 or n.endswith(("pos_embedding", "cls_token"))), n
    assert all(g["lr_scale"] == 1.0 and "lr" not in g for g in groups)
    assert [n for g in groups for n in g["names"]] == [names[i] for i in seen]
    # names matching extra_no_decay join the set
    extra = param_groups(model, 0.1, extra_no_decay=("to_qkv",))
    assert ENC + "transformer.layers.0.0.to_qkv.weight" in {names[id(p)] for g in extra if g["weight_decay"] == 0.0 for p in g["params"]}
    # both features off: one group
    one = param_groups(model, 0.1, no_decay=False)
    assert len(one) == 1 and one[0]["weight_decay"] == 0.1 and one[0]["lr_scale"] == 1.0 and len(one[0]["params"]) == len(seen)
    # any torch optimizer takes them
    torch.optim.AdamW(param_groups(model, 0.1, layer_decay=0.75), lr=1e-3)


def test_param_groups_layer_ids_and_scales():
    from neurovit_amd import param_groups
    from neurovit_amd.optim import encoder_depth, layer_id_of
    model = _cpu_model()
    L = encoder_depth(model)
    assert L == 2
    want = {ENC + "pos_embedding": 0, ENC + "cls_token": 0, ENC + "to_patch_embedding.1.weight": 0, ENC + "to_patch_embedding.2.bias": 0,
            ENC + "transformer.layers.0.0.to_qkv.weight": 1, ENC + "transformer.layers.0.1.net.1.bias": 1, ENC + "transformer.layers.1.0.norm.bias": 2,
            ENC + "transformer.norm.weight": 3, ENC + "mlp_head.0.weight": 3, ENC + "mlp_head.1.bias": 3,
            "temporal_transformer.transformer.layers.0.linear1.weight": 3, "projection_head.projection_head.bias": 3}
    present = dict(model.named_parameters())
    for n, i in want.items():
        assert layer_id_of(n, L) == i, n
        assert n in present or n.startswith(("temporal", "projection")) or n == ENC + "transformer.norm.weight", n      # (this ViT has no final norm)
    decay = 0.65
    names = _names_by_param(model)
    groups = param_groups(model, 0.05, no_decay=True, layer_decay=decay)
    assert len(groups) == 2 * (L + 2)                               # every layer id holds matrices and vectors
    for g in groups:
        ids = {layer_id_of(names[id(p)], L) for p in g["params"]}
        assert len(ids) == 1
        assert g["lr_scale"] == decay ** (L + 1 - ids.pop())        # in double, exactly
        assert g["weight_decay"] in (0.0, 0.05)
    assert max(g["lr_scale"] for g in groups) == 1.0 and min(g["lr_scale"] for g in groups) == decay ** 3
    seen = [id(p) for g in groups for p in g["params"]]
    assert len(seen) == len(set(seen)) == len(list(model.parameters()))
    # layer_decay alone: one group per id; 1.0 gives scales of exactly 1
    assert [g["lr_scale"] for g in param_groups(model, 0.05, no_decay=False, layer_decay=decay)] == [decay ** 3, decay ** 2, decay, 1.0]
    assert all(g["lr_scale"] == 1.0 and g["weight_decay"] == 0.05 for g in param_groups(model, 0.05, no_decay=False, layer_decay=1.0))
    for bad, err in (("0.5", TypeError), (True, TypeError), (0.0, ValueError), (1.5, ValueError), (float("nan"), ValueError)):
        with pytest.raises(err):
            param_groups(model, 0.05, layer_decay=bad)
    for bad, err in (("x", TypeError), (-1.0, ValueError), (float("inf"), ValueError)):
        with pytest.raises(err):
            param_groups(model, bad)


def test_param_groups_of_the_4d_model_leave_the_frozen_encoder_out():
    from neurovit_amd import param_groups
    model = _cpu_model4d()
    names = _names_by_param(model)
    groups = param_groups(model, 0.1, layer_decay=0.5)
    got = {names[id(p)] for g in groups for p in g["params"]}
    assert got == {n for n, p in model.named_parameters() if p.requires_grad}
    assert got and not any(n.startswith("volume_encoder.") for n in got)
    assert all(g["lr_scale"] == 1.0 for g in groups)               # temporal transformer and projection head: id L + 1
    assert len(groups) == 2
    no_decay = {names[id(p)] for g in groups if g["weight_decay"] == 0.0 for p in g["params"]}
    assert no_decay == {n for n in got if dict(model.named_parameters())[n].ndim <= 1}


# ------------------------------------------------------------------------------------------ 4. LRSchedule
def test_schedule_matches_the_closed_forms():
    from neurovit_amd import LRSchedule
    base, lo, total, warm = 3e-4, 1e-6, 50, 7
    cos, lin, con = (LRSchedule(base, total, warm, kind, lo) for kind in ("cosine", "linear", "constant"))
    for k in range(1, total + 20):
        if k <= warm:
            want = (base * k / warm,) * 3
        else:
            q = min(1.0, max(0.0, (k - warm) / max(1, total - warm)))
            want = (lo + (base - lo) * 0.5 * (1.0 + math.cos(math.pi * q)), base + (lo - base) * q, base)
            if q == 1.0:                                            # the end of the run is min_lr itself, not its rounded closed form
                want = (lo, lo, base)
        assert (cos.lr_at(k), lin.lr_at(k), con.lr_at(k)) == want, k
    ramp = [cos.lr_at(k) for k in range(1, warm + 1)]
    assert ramp[0] > 0.0 and all(a < b for a, b in zip(ramp, ramp[1:])) and ramp[-1] == base
    assert cos.lr_at(total) == lo and lin.lr_at(total) == lo
    assert all(s.lr_at(total + j) == s.lr_at(total) for s in (cos, lin, con) for j in (1, 5, 10 ** 6))
    assert all(a >= b for a, b in zip([cos.lr_at(k) for k in range(warm, total)], [cos.lr_at(k) for k in range(warm + 1, total + 1)]))
    # no warm-up: the first step runs at the base rate; one step in all; warm-up as long as the run
    assert LRSchedule(base, total).lr_at(1) < base and LRSchedule(base, total).lr_at(1) > 0.99 * base
    assert LRSchedule(base, 1).lr_at(1) == 0.0 + LRSchedule(base, 1, min_lr=0.0).lr_at(1)
    assert LRSchedule(base, 5, 5, "linear").lr_at(5) == base and LRSchedule(base, 5, 5, "linear").lr_at(6) == 0.0
    assert LRSchedule(base, total, kind="constant").lr_at(3) == base


def test_schedule_refusals():
    from neurovit_amd import LRSchedule
    for args, err in ((("1e-3", 10), TypeError), ((True, 10), TypeError), ((1e-3, 10.0), TypeError), ((1e-3, 10, 2.0), TypeError),
                      ((1e-3, 10, 0, 3), TypeError), ((1e-3, 10, 0, "cosine", "0"), TypeError), ((1e-3, True), TypeError),
                      ((0.0, 10), ValueError), ((-1e-3, 10), ValueError), ((float("nan"), 10), ValueError), ((float("inf"), 10), ValueError),
                      ((1e-3, 0), ValueError), ((1e-3, 10, -1), ValueError), ((1e-3, 10, 11), ValueError), ((1e-3, 10, 0, "step"), ValueError),
                      ((1e-3, 10, 0, "cosine", -1e-6), ValueError), ((1e-3, 10, 0, "cosine", 2e-3), ValueError)):
        with pytest.raises(err):
            LRSchedule(*args)
    s = LRSchedule(1e-3, 10)
    for k, err in ((0, ValueError), (-3, ValueError), (1.0, TypeError), (True, TypeError)):
        with pytest.raises(err):
            s.lr_at(k)


# ------------------------------------------------------------------------------------------ 5. the Trainer's config keys
def test_schedule_from_config():
    from neurovit_amd.optim import LRSchedule
    from neurovit_amd.trainer import Trainer
    parse = Trainer.schedule_from_config
    assert parse({}, 3, 10) == {}
    assert parse(dict(TRAINING_LR_SCHEDULE=None, TRAINING_LAYER_DECAY=None, TRAINING_NO_DECAY_NORM_BIAS=False), 3, 10) == {}
    out = parse(dict(TRAINING_LR_SCHEDULE="cosine", TRAINING_WARMUP_STEPS=4, TRAINING_MIN_LR=1e-6, TRAINING_LEARNING_RATE=2e-4, TRAINING_LAYER_DECAY=0.75,
                     TRAINING_NO_DECAY_NORM_BIAS=True), 3, 10)
    s = out.pop("lr_schedule")
    assert out == dict(layer_decay=0.75, no_decay=True)
    assert isinstance(s, LRSchedule) and (s.base_lr, s.total_steps, s.warmup_steps, s.kind, s.min_lr) == (2e-4, 30, 4, "cosine", 1e-6)
    # total_steps = epochs * ceil(batches / accumulation); the accumulation key counts only when accumulation is on
    acc = dict(TRAINING_LR_SCHEDULE="linear", USE_ACCUMULATION=True, TRAINING_ACCUMULATION_STEP=4)
    assert parse(acc, 3, 10)["lr_schedule"].total_steps == 9
    assert parse(dict(acc, USE_ACCUMULATION=False), 3, 10)["lr_schedule"].total_steps == 30
    assert parse(dict(TRAINING_LR_SCHEDULE="constant"), 2, 5)["lr_schedule"].base_lr == 1e-4          # the step's default learning rate
    for cfg, err in ((dict(TRAINING_LR_SCHEDULE="step"), ValueError), (dict(TRAINING_LR_SCHEDULE=3), TypeError),
                     (dict(TRAINING_WARMUP_STEPS=3), ValueError), (dict(TRAINING_MIN_LR=1e-6), ValueError),
                     (dict(TRAINING_LR_SCHEDULE="cosine", TRAINING_WARMUP_STEPS=31), ValueError),
                     (dict(TRAINING_LR_SCHEDULE="cosine", TRAINING_WARMUP_STEPS=2.5), TypeError),
                     (dict(TRAINING_LR_SCHEDULE="cosine", TRAINING_MIN_LR=1.0), ValueError),
                     (dict(TRAINING_LAYER_DECAY="0.75"), TypeError), (dict(TRAINING_LAYER_DECAY=True), TypeError), (dict(TRAINING_LAYER_DECAY=0.0), ValueError),
                     (dict(TRAINING_LAYER_DECAY=1.01), ValueError), (dict(TRAINING_NO_DECAY_NORM_BIAS="yes"), TypeError), (dict(TRAINING_NO_DECAY_NORM_BIAS=1), TypeError)):
        with pytest.raises(err):
            parse(cfg, 3, 10)


# ------------------------------------------------------------------------------------------ 6. the step's bookkeeping on a CPU-resident model
def test_train_step_builds_the_groups_and_sets_their_learning_rates():
    from neurovit_amd.optim import LRSchedule, set_group_lrs
    from neurovit_amd.trainer import TrainStep
    plain = TrainStep(_cpu_model(), lr=3e-4, weight_decay=0.05)
    assert len(plain.optimizer.param_groups) == 1 and plain.last_lr == 3e-4 and "groups" not in plain.state_dict()
    assert len(TrainStep(_cpu_model(), lr=3e-4, weight_decay=0.05, no_decay=False, layer_decay=None).optimizer.param_groups) == 1
    sched = LRSchedule(3e-4, 10, 2)
    step = TrainStep(_cpu_model(), lr=3e-4, weight_decay=0.05, no_decay=True, layer_decay=0.5, lr_schedule=sched)
    groups = step.optimizer.param_groups
    assert len(groups) == 8 and step.last_lr == sched.lr_at(1) == 1.5e-4
    assert all(g["lr"] == 1.5e-4 * g["lr_scale"] for g in groups) and {g["weight_decay"] for g in groups} == {0.0, 0.05}
    assert step.optimizer.is_grouped() and not plain.optimizer.is_grouped()
    assert not TrainStep(_cpu_model(), layer_decay=1.0).optimizer.is_grouped()
    set_group_lrs(step.optimizer, 1.0)
    assert [g["lr"] for g in groups] == [g["lr_scale"] for g in groups]
    # the state carries lr, lr_scale and weight_decay per group and restores them per group
    state = step.state_dict()
    assert state["groups"] == [dict(lr=g["lr"], lr_scale=g["lr_scale"], weight_decay=g["weight_decay"]) for g in groups]
    other = TrainStep(_cpu_model(), lr=1e-3, weight_decay=0.5, no_decay=True, layer_decay=0.9)
    other.load_state_dict(state)
    assert [(g["lr"], g["lr_scale"], g["weight_decay"]) for g in other.optimizer.param_groups] == [(g["lr"], g["lr_scale"], g["weight_decay"]) for g in groups]
    # a state whose group count differs is refused before anything is copied
    m, v = plain.optimizer.arena_state(plain._vit)
    m.fill_(1.0)
    plain.optimizer._steps = 5
    with pytest.raises(ValueError, match="parameter groups"):
        plain.load_state_dict(state)
    assert plain.optimizer._steps == 5 and bool((m == 1.0).all()) and plain.optimizer.param_groups[0]["lr"] == 3e-4
    # a state from before parameter groups (no such key) loads as it always did: group 0's hyper-parameters everywhere
    old = {k: val for k, val in state.items() if k != "groups"}
    other.load_state_dict(old)
    assert all(g["lr"] == state["hyper"]["lr"] and g["weight_decay"] == state["hyper"]["weight_decay"] for g in other.optimizer.param_groups)


def test_refusals_come_before_any_device_work():
    from neurovit_amd import param_groups
    from neurovit_amd.optim import FusedAdamW
    from neurovit_amd.trainer import TrainStep
    with pytest.raises(ValueError, match="overlap_optimizer"):
        TrainStep(_cpu_model(), no_decay=True, overlap_optimizer=True)
    with pytest.raises(TypeError):
        TrainStep(_cpu_model(), lr_schedule="cosine")
    with pytest.raises(TypeError):
        TrainStep(_cpu_model(), no_decay=1)
    model = _cpu_model()
    vit = model.volume_encoder.vit3d
    # betas / eps that differ between groups of one arena: named
    for key, value in (("betas", (0.8, 0.999)), ("eps", 1e-6)):
        groups = param_groups(model, 0.1)
        groups[1][key] = value
        opt = FusedAdamW(groups, lr=1e-3, model=model)
        with pytest.raises(ValueError, match="groups 0 and 1"):
            opt.arenas()
    # a parameter in two groups (torch's own constructor refuses it, with the same exception type)
    groups = param_groups(model, 0.1)
    groups[1]["params"].append(groups[0]["params"][0])
    with pytest.raises(ValueError, match="more than one parameter group"):
        FusedAdamW(groups, lr=1e-3, model=model)
    # more groups in one arena than the launch has pairs
    plist = vit.arena_parameters()
    assert len(plist) < 65
    big = _cpu_model(TRAINING_VIT_DEPTH=8)
    many = [{"params": [p], "weight_decay": 0.01 * i} for i, p in enumerate(big.parameters())]
    assert len(many) > 64
    with pytest.raises(ValueError, match="64"):
        FusedAdamW(many, lr=1e-3, model=big).arenas()
    # the per-bucket update of overlap_optimizer on a grouped arena
    opt = FusedAdamW(param_groups(model, 0.1), lr=1e-3, model=model)
    opt.begin_step()
    with pytest.raises(ValueError, match="step_range"):
        opt.step_range(vit, 0, 64)


# ------------------------------------------------------------------------------------------ 7. the boundary
def test_header_declares_and_library_exports_the_grouped_step():
    import ctypes
    from neurovit_amd import _cabi
    protos = _cabi.parse_header()
    for name in ("nv_adamw_step_grouped", "nv_adamw_segments_build", "nv_adamw_segments_bytes", "nv_adamw_segments_release"):
        assert name in protos, name
    clipped, grouped = protos["nv_adamw_step_clipped"][1], protos["nv_adamw_step_grouped"][1]
    # nv_adamw_step_clipped with (lr, weight_decay) replaced by one pointer to the table
    assert grouped[:8] == clipped[:8] and grouped[8] is ctypes.c_void_p and grouped[9:12] == clipped[9:12] and grouped[12:] == clipped[13:]
    assert protos["nv_adamw_segments_bytes"][0] is ctypes.c_long
    assert ctypes.sizeof(_cabi.AdamwGroups) == 16 + 2 * 8 * _cabi.ADAMW_MAX_GROUPS == 1040
    src = open(_cabi.HEADER).read()
    assert "#define NV_ADAMW_MAX_GROUPS 64" in src and "#define NV_ADAMW_MAX_SEGMENTS 1024" in src and "#define NV_ABI_VERSION 8" in src
    if os.path.exists(_cabi.LIB_PATH):
        dll = ctypes.CDLL(_cabi.LIB_PATH)
        assert all(hasattr(dll, n) for n in ("nv_adamw_step_grouped", "nv_adamw_segments_build", "nv_adamw_segments_bytes", "nv_adamw_segments_release"))
        dll.nv_adamw_segments_bytes.restype = ctypes.c_long
        assert dll.nv_adamw_segments_bytes(0) == 0 and dll.nv_adamw_segments_bytes(1025) == 0
        assert dll.nv_adamw_segments_bytes(150) == (150 * 12 + 15) // 16 * 16 + 256
