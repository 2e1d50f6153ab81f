"""The weight average and the resumable training state on MI355X: nv_ema_update bit for bit against tests/ema_ref.py, TrainStep(ema_decay=...)
replicated from parameter snapshots on every path that can end a step, the invariant that an average changes no bit of training, the
averaged model's derived copies (16-bit shadow, folded weights) after raw-pointer updates, the 4D model and the ViT without output
projection, TrainStep.state_dict / load_state_dict (a resumed run equals the straight one bit for bit) and the Trainer shell's keys.
The micro model, its path fixture and its fp16 scaler set-up are those of tests/test_grad_clip_gpu.py."""
import glob
import io
import os

import numpy as np
import pytest
import torch

import ema_ref as E
import weights as W
from test_grad_clip_gpu import LR, SIZE, WD, _data, _make_step, _model

pytestmark = pytest.mark.gpu


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


@pytest.fixture
def path(request, monkeypatch):
    monkeypatch.setenv("NEUROVIT_NATIVE_STEP", "1" if request.param == "native" else "0")
    return request.param


BOTH_PATHS = pytest.mark.parametrize("path", ["native", "general"], indirect=True)


def rnd(*shape, seed=0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


# ------------------------------------------------------------------------------------------ 1. the kernel
COUNTS = (4, 8, 1020, 2048, 2052, 4100)
STRIDED = 20004          # with max_blocks = 2: 5001 16-byte pieces, 1024 per grid pass = four full passes and a tail
WEIGHTS = (0.0, 1.0, float(np.float32(1e-4)), float(np.float32(0.1)))
SPECIALS = ((1e-42, -3e-45), (float("inf"), 1.0), (1.0, float("-inf")), (float("inf"), float("inf")), (float("nan"), 0.5), (0.5, float("nan")),
            (-1e-40, -1e-40), (float("-inf"), float("inf")))
GUARD, PAD = 7.5, 16     # 16 floats in front keep the range 16-byte aligned


def _operands(count):
    e, p = rnd(count, seed=count), rnd(count, seed=count + 1)
    e[1::5] = p[1::5]                                            # cells at the fixed point
    for i, (a, b) in enumerate(SPECIALS):                        # denormals, infinities, NaN
        if 2 + 3 * i < count:
            e[2 + 3 * i], p[2 + 3 * i] = a, b
    return e, p


@pytest.mark.parametrize("weight", WEIGHTS)
def test_kernel_equals_the_restatement_bit_for_bit(ops, weight):
    for count, blocks in [(c, 0) for c in COUNTS] + [(STRIDED, 2)]:
        e, p = _operands(count)
        buf = torch.full((count + 2 * PAD,), GUARD, device="cuda")
        ema = buf[PAD:PAD + count]
        ema.copy_(e)
        pd = p.cuda()
        ops.ema_update(ema, pd, weight, blocks)
        want = E.update(e, p, weight)
        got = ema.cpu()
        assert E.same_bits(got, want), (count, weight, int((got.view(torch.int32) != want.view(torch.int32)).sum()))
        assert E.same_bits(got, torch.from_numpy(E.update_np(e.numpy(), p.numpy(), weight)))
        fixed = torch.isfinite(e) & (e == p)
        assert torch.equal(got[fixed].view(torch.int32), e[fixed].view(torch.int32)), (count, weight)      # p == ema: not one bit moves
        assert bool((buf[:PAD] == GUARD).all()) and bool((buf[PAD + count:] == GUARD).all()), (count, weight)
        assert E.same_bits(pd, p), (count, weight)                                                         # p is only read


def test_kernel_refusals(ops):
    e, p = torch.zeros(16, device="cuda"), torch.ones(16, device="cuda")
    for ema, par, w in ((e[:6], p[:6], 0.1), (e[1:9], p[:8], 0.1), (e[:8], p[2:10], 0.1), (e, p, 1.5), (e, p, -0.5), (e, p, float("nan"))):
        with pytest.raises(RuntimeError, match="nv_ema_update"):
            ops.ema_update(ema, par, w)
    with pytest.raises(RuntimeError):
        ops.ema_update(e.cpu(), p.cpu(), 0.1)
    assert bool((e == 0).all()) and bool((p == 1).all())


# ------------------------------------------------------------------------------------------ 2. TrainStep, replicated from snapshots
def _vit(model):
    return model.volume_encoder.vit3d


def _replay_steps(step, holder, ema_holder, batches, decay, warmup=True, every=1):
    """Run `batches` (micro-batches); the average must equal the recurrence over the parameter arena as it stood after every
    optimizer step - and must not move on a micro-step that ends no window."""
    arena, avg = holder.flat_parameters()[0], ema_holder.flat_parameters()[0]
    start = arena.detach().cpu().clone()
    assert torch.equal(avg.cpu(), start) and avg.data_ptr() != arena.data_ptr()
    snaps = []
    for b in batches:
        before = avg.clone()
        step(*b)
        if step._micro == 0:
            snaps.append(arena.detach().cpu().clone())
        else:
            assert torch.equal(avg, before)
    want, t = E.replay(start, snaps, decay, warmup, every)
    assert step.ema.num_updates == t == len(snaps)
    assert torch.equal(avg.cpu(), want)
    assert not torch.equal(want, start) and not torch.equal(want, snaps[-1])
    return snaps


CASES = {
    "native-fuse0": ("native", "bf16", dict(fuse_update=0), {}),
    "native-fuse1": ("native", "bf16", dict(fuse_update=1), {}),
    "native-fuse3": ("native", "bf16", dict(fuse_update=3), {}),
    "general": ("general", "bf16", {}, {}),
    "native-accumulate-2": ("native", "bf16", dict(accumulation_steps=2), {}),
    "general-accumulate-2": ("general", "bf16", dict(accumulation_steps=2), {}),
    "native-clip": ("native", "bf16", dict(max_grad_norm=0.05), {}),
    "general-clip": ("general", "bf16", dict(max_grad_norm=0.05), {}),
    "native-static-scale": ("native", "bf16", dict(loss_scale=1024.0), {}),
    "general-overlap-optimizer": ("general", "bf16", dict(overlap_optimizer=True), {}),
    "general-side-stream": ("general", "bf16", {}, {"NEUROVIT_FORCE_COMPUTE_STREAM": "1"}),
    "native-update-every-2": ("native", "bf16", dict(ema_update_every=2, ema_warmup=False), {}),
    "general-no-warmup": ("general", "bf16", dict(ema_warmup=False), {}),
}


@pytest.mark.parametrize("case", list(CASES))
def test_average_replicated_from_parameter_snapshots(case, monkeypatch):
    want_path, fmt, kw, env = CASES[case]
    monkeypatch.setenv("NEUROVIT_NATIVE_STEP", "1" if want_path == "native" else "0")
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    model = _model(fmt)
    step = _make_step(model, fmt, ema_decay=0.9, **kw)
    per = kw.get("accumulation_steps", 1)
    steps = 4 if "ema_update_every" in kw else 3
    batches = [_data(50 + i) for i in range(per * steps)]
    _replay_steps(step, _vit(model), _vit(step.ema.module), batches, 0.9, kw.get("ema_warmup", True), kw.get("ema_update_every", 1))
    assert step.last_path == want_path
    if "fuse_update" in kw:
        assert step.last_fuse_update == kw["fuse_update"]
    if "side-stream" in case:
        assert step._compute_stream is not None
    assert step.optimizer._steps == steps


def test_average_behind_the_graph_replayed_step(monkeypatch):
    """three eager native steps, then the captured graph: the average follows the AdamW launch queued behind the replay"""
    monkeypatch.setenv("NEUROVIT_NATIVE_STEP", "1")
    monkeypatch.setenv("NEUROVIT_GRAPH_STEP", "1")
    model = _model()
    step = _make_step(model, "bf16", ema_decay=0.9)
    x, y = _data(60)
    _replay_steps(step, _vit(model), _vit(step.ema.module), [(x, y)] * 6, 0.9)
    assert len(step._graphs) == 1


@BOTH_PATHS
def test_a_skipped_step_is_still_averaged_and_counted(path):
    """fp16 operands, dynamic loss scale: an infinite voxel makes every gradient of the second step non-finite - the scaler's skip path.
    The parameters do not move, the average moves towards them once more, num_updates counts the call."""
    model = _model("fp16")
    step = _make_step(model, "fp16", ema_decay=0.9)
    bad_x, bad_y = _data(71)
    bad_x[0, 3, 4, 5] = float("inf")
    snaps = _replay_steps(step, _vit(model), _vit(step.ema.module), [_data(70), (bad_x, bad_y), _data(72)], 0.9)
    assert step.last_path == path
    assert torch.equal(snaps[0], snaps[1]) and not torch.equal(snaps[1], snaps[2])
    assert step.scaler.steps_applied() == 2 and step.scaler.steps_skipped() == 1 and step.ema.num_updates == 3
    assert bool(torch.isfinite(_vit(step.ema.module).flat_parameters()[0]).all())


def test_average_on_the_one_rank_native_data_parallel_plan(monkeypatch):
    """nv_dp_plan on a communicator of one rank (tests/test_dp_gpu.py): AdamW per bucket on the communication stream (1), on the auxiliary
    stream one bucket late (2) - the main stream has joined both when the call returns, so the average reads finished parameters."""
    monkeypatch.setenv("NEUROVIT_NATIVE_STEP", "1")
    for per_bucket in ("1", "2"):
        monkeypatch.setenv("NEUROVIT_DP_UPDATE_PER_BUCKET", per_bucket)
        model = _model()
        step = _make_step(model, "bf16", n_buckets=3, native_dp=True, ema_decay=0.9)
        _replay_steps(step, _vit(model), _vit(step.ema.module), [_data(80 + i) for i in range(3)], 0.9)
        assert step.last_path == "native-dp" and step.last_dp["update_per_bucket"] == int(per_bucket)


# ------------------------------------------------------------------------------------------ 3. an average changes no bit of training
@BOTH_PATHS
@pytest.mark.parametrize("fmt", ["bf16", "fp16"])
def test_average_changes_no_bit_of_training(path, fmt):
    outs = []
    for kw in ({}, dict(ema_decay=0.99)):
        model = _model(fmt)
        step = _make_step(model, fmt, **kw)
        losses = [step(*_data(seed)).clone() for seed in (7, 8, 9)]
        assert step.last_path == path and (step.ema is not None) == bool(kw)
        m, v = step.optimizer.arena_state(_vit(model))
        outs.append((torch.stack(losses), _vit(model).flat_parameters()[0].clone(), m.clone(), v.clone(), _vit(model).flat_gradients().clone(),
                     None if step.scaler is None else step.scaler.state.clone()))
    for a, b in zip(*outs):
        assert (a is None and b is None) or torch.equal(a, b)
    assert (outs[0][5] is not None) == (fmt == "fp16")


# ------------------------------------------------------------------------------------------ 4. the averaged model is never stale
@pytest.mark.parametrize("mode", ["fold", "plain", "fp32"])
def test_averaged_model_forward_follows_every_update(mode):
    def build():
        m = _model()
        _vit(m).fold_layernorm = mode != "plain"
        return m

    def forward(m):
        import contextlib
        with torch.no_grad(), (m.precision("fp32") if mode == "fp32" else contextlib.nullcontext()):
            return m(x).clone()
    model = build()
    step = _make_step(model, "bf16", ema_decay=0.5, ema_warmup=False)
    avg = step.ema.module
    assert not avg.training and not any(p.requires_grad for p in avg.parameters()) and _vit(avg).fold_layernorm == (mode != "plain")
    assert list(avg.state_dict()) == list(model.state_dict())
    x = _data(90)[0]
    outs = [forward(avg)]                                         # shadow and folded weights of the starting average now exist
    for seed in (91, 92):
        step(*_data(seed))
        outs.append(forward(avg))
        fresh = build()
        fresh.load_state_dict(step.ema.state_dict()["module"], strict=True)
        fresh.eval()
        assert torch.equal(outs[-1], forward(fresh)), (mode, seed)
    assert not torch.equal(outs[0], outs[1]) and not torch.equal(outs[1], outs[2])
    model.eval()
    assert not torch.equal(outs[2], forward(model))               # and it is not the raw model


def test_model_ema_state_round_trip_and_refusals():
    from neurovit_amd import ModelEma
    model = _model()
    ema = ModelEma(model, decay=0.5, warmup=False)
    with torch.no_grad():
        for p in model.parameters():
            p.add_(0.25)
    ema.update()
    ema.update(model)
    assert ema.num_updates == 2
    state = ema.state_dict()
    assert set(state) == {"module", "num_updates", "decay", "warmup", "update_every"} and state["num_updates"] == 2
    assert (state["decay"], state["warmup"], state["update_every"]) == (0.5, False, 1)
    other = ModelEma(_model(), decay=0.5, warmup=False)
    arena = _vit(other.module).flat_parameters()[0]
    ptr = arena.data_ptr()
    other.load_state_dict({k: (v if k != "module" else {n: t.cpu().clone() for n, t in v.items()}) for k, v in state.items()})
    assert _vit(other.module).flat_parameters()[0].data_ptr() == ptr and other.num_updates == 2
    assert torch.equal(arena, _vit(ema.module).flat_parameters()[0])
    # a model of another size: refused before any launch, nothing counted
    import neurovit_amd.NeuroEncoder as ne
    small = ne.NeuroEncoder(W.neuro_config(32, 8, DEVICE="cuda", **dict(SIZE, TRAINING_VIT_DEPTH=1)))
    before = arena.clone()
    with pytest.raises(ValueError, match="arena"):
        other.update(small)
    assert other.num_updates == 2 and torch.equal(arena, before)


# ------------------------------------------------------------------------------------------ 5. the 4D model; a ViT without output projection
def test_4d_model_averages_the_head_and_keeps_the_frozen_encoder():
    import test_dp_gpu as tdp
    model = tdp._model4d()                                        # (its encoder checkpoint is gone by now: the average must not read it again)
    step = _make_step(model, "bf16", ema_decay=0.9)
    avg = step.ema.module
    assert not any(p.requires_grad for p in avg.parameters()) and list(avg.state_dict()) == list(model.state_dict())
    batches = [(W.make_volume((2, 32, 32, 32, 4), s).cuda(), torch.tensor([0, 1], device="cuda")) for s in (7, 8, 9)]
    _replay_steps(step, model._temporal_head, avg._temporal_head, batches, 0.9)
    assert step.last_path == "general"
    assert torch.equal(_vit(avg).flat_parameters()[0], _vit(model).flat_parameters()[0])
    with torch.no_grad():
        avg(batches[0][0])                                        # the averaged 4D model runs


def test_constant_slots_of_a_vit_without_projection_stay_exact():
    import neurovit_amd.NeuroEncoder as ne
    size = dict(TRAINING_VIT_DIM=64, TRAINING_VIT_DEPTH=2, TRAINING_VIT_HEADS=1, TRAINING_VIT_DIM_HEAD=64, TRAINING_VIT_MLP_DIM=128)
    model = ne.NeuroEncoder(W.neuro_config(16, 8, DEVICE="cuda", TRAINING_LEARNING_RATE=LR, TRAINING_WEIGHT_DECAY=WD, **size))
    model.load_state_dict(W.make_tensors(W.vit_param_spec(**W.NOPROJ), 71, prefix="volume_encoder.vit3d."), strict=True)
    model.train()
    step = _make_step(model, "bf16", ema_decay=0.9)
    avg = _vit(step.ema.module)
    batches = [(W.make_volume((3, 16, 16, 16), s).cuda(), torch.tensor([0, 1, 0], device="cuda")) for s in (72, 73, 74)]
    _replay_steps(step, _vit(model), avg, batches, 0.9)
    assert _vit(model)._phantom and len(avg._phantom) == len(_vit(model)._phantom)
    arena = avg.flat_parameters()[0]
    for o, const in avg._phantom:
        assert torch.equal(arena[o:o + const.numel()].view(torch.int32), const.view(torch.int32))


# ------------------------------------------------------------------------------------------ 6. resume
def _through_a_file(obj):
    buf = io.BytesIO()
    torch.save(obj, buf)
    buf.seek(0)
    return torch.load(buf, map_location="cpu", weights_only=True)


def _everything(step, model):
    m, v = step.optimizer.arena_state(_vit(model))
    return dict(params=_vit(model).flat_parameters()[0].clone(), m=m.clone(), v=v.clone(), ema=_vit(step.ema.module).flat_parameters()[0].clone(),
                scaler=None if step.scaler is None else step.scaler.state.clone(), updates=step.ema.num_updates, steps=step.optimizer._steps)


RESUME = {"bf16-native": ("native", "bf16", {}), "bf16-general": ("general", "bf16", {}), "fp16-dynamic": ("native", "fp16", {}),
          "clip": ("native", "bf16", dict(max_grad_norm=0.05)), "clip-general-fp16": ("general", "fp16", dict(max_grad_norm=0.05))}


@pytest.mark.parametrize("case", list(RESUME))
def test_resumed_run_equals_the_straight_run(case, monkeypatch):
    want_path, fmt, kw = RESUME[case]
    monkeypatch.setenv("NEUROVIT_NATIVE_STEP", "1" if want_path == "native" else "0")
    kw = dict(kw, ema_decay=0.9)
    batches = [_data(100 + i) for i in range(4)]
    model = _model(fmt)
    step = _make_step(model, fmt, **kw)
    for b in batches:
        step(*b)
    straight = _everything(step, model)
    first = _model(fmt)
    step1 = _make_step(first, fmt, **kw)
    for b in batches[:2]:
        step1(*b)
    state, weights = _through_a_file(step1.state_dict()), _through_a_file(first.state_dict())
    del step1, first
    second = _model(fmt)
    second.load_state_dict(weights, strict=True)
    step2 = _make_step(second, fmt, **kw)
    ptrs = [t.data_ptr() for t in step2.optimizer.arena_state(_vit(second))] + [_vit(step2.ema.module).flat_parameters()[0].data_ptr()]
    step2.load_state_dict(state)
    assert ptrs == [t.data_ptr() for t in step2.optimizer.arena_state(_vit(second))] + [_vit(step2.ema.module).flat_parameters()[0].data_ptr()]
    assert step2.optimizer._steps == 2 and step2.ema.num_updates == 2
    for b in batches[2:]:
        step2(*b)
    assert step2.last_path == want_path
    resumed = _everything(step2, second)
    for name, a in straight.items():
        b = resumed[name]
        assert (torch.equal(a, b) if torch.is_tensor(a) else a == b), name
    assert straight["steps"] == 4 and straight["updates"] == 4


def test_state_refusals_on_the_device_change_nothing():
    import neurovit_amd.NeuroEncoder as ne
    model = _model()
    step = _make_step(model, "bf16", ema_decay=0.9, accumulation_steps=2)
    step(*_data(110))
    with pytest.raises(RuntimeError, match="window"):
        step.state_dict()
    step(*_data(111))
    good = step.state_dict()
    assert good["ema"]["num_updates"] == 1 and good["steps"] == 1 and good["scaler"] is None
    target_model = _model()
    target = _make_step(target_model, "bf16", ema_decay=0.9)
    target(*_data(112))
    before = _everything(target, target_model)
    small = ne.NeuroEncoder(W.neuro_config(32, 8, DEVICE="cuda", **dict(SIZE, TRAINING_VIT_DEPTH=1)))
    other_size = _make_step(small, "bf16", ema_decay=0.9).state_dict()
    fp16 = _make_step(_model("fp16"), "fp16", ema_decay=0.9).state_dict()
    scaled = _make_step(_model(), "bf16", ema_decay=0.9, loss_scale="dynamic").state_dict()
    assert scaled["operands"] == "bf16" and scaled["scaler"].numel() == 16
    plain = _make_step(_model(), "bf16").state_dict()
    for word, bad in (("arena", other_size), ("operands", fp16), ("loss scale", scaled), ("average", plain), ("version", dict(good, version=0))):
        with pytest.raises(ValueError, match=word):
            target.load_state_dict(bad)
        after = _everything(target, target_model)
        for name, a in before.items():
            assert (torch.equal(a, after[name]) if torch.is_tensor(a) else a == after[name]), (word, name)
    target.load_state_dict(good)                                  # and the good one still loads
    assert target.optimizer._steps == 1 and target.ema.num_updates == 1


# ------------------------------------------------------------------------------------------ 7. the Trainer shell
class Cubes(torch.utils.data.Dataset):
    """DatasetADNI's 7-tuples over the synthetic cube-localisation volumes (neurovit_amd.synthetic): 8 samples, 8 classes"""

    def __init__(self, seed):
        from neurovit_amd.synthetic import cube_volumes
        self.x, self.y, _ = cube_volumes(8, 32, 16, grid_noise=0.0, seed=seed)
        self.x = self.x + 0.05 * rnd(8, 32, 32, 32, seed=seed)

    def __len__(self):
        return 8

    def __getitem__(self, i):
        return f"s{i}", torch.tensor(0), self.x[i], torch.tensor(0), torch.tensor(1), torch.tensor(70), self.y[i]


def _trainer(tmp_path, epochs, **extra):
    from neurovit_amd.NeuroEncoder import NeuroEncoder
    from neurovit_amd.trainer import Trainer
    cfg = W.neuro_config(32, 8, dataset="gradcam", DEVICE="cuda", GRADCAM_CUBE_SIZE=16, TRAINING_LEARNING_RATE=1e-3, TRAINING_WEIGHT_DECAY=1e-2,
                         GLOBAL_OUTPUT_DIR=str(tmp_path / "runs"), TRAINING_EPOCHS=epochs, TRAINING_BATCH_SIZE=2, TRAINING_NUM_WORKERS=0, **SIZE, **extra)
    return Trainer(cfg, NeuroEncoder(cfg), Cubes(1), Cubes(2))


def _files(folder):
    return sorted(os.path.basename(f) for f in glob.glob(os.path.join(str(folder), "*")))


def test_trainer_validates_and_saves_the_average(tmp_path, monkeypatch, capsys):
    monkeypatch.chdir(tmp_path)
    torch.manual_seed(5)
    tr = _trainer(tmp_path, 1, TRAINING_EMA_DECAY=0.9, TRAINING_EMA_WARMUP=False, TRAINING_EMA_UPDATE_EVERY=2)
    ema = tr.step.ema
    assert (ema.decay, ema.warmup, ema.update_every) == (0.9, False, 2)
    logged = []
    tr._log = logged.append
    tr.run()
    assert ema.num_updates == 4 and tr.global_step == 4
    val = [p for p in logged if "val_loss" in p or "val_loss_ema" in p]
    assert [sorted(p) for p in val] == [["epoch", "val_accuracy", "val_loss"], ["epoch", "val_accuracy_ema", "val_loss_ema"]]
    assert tr.val_loss == val[0]["val_loss"] and tr.val_loss_ema == val[1]["val_loss_ema"] and tr.val_loss != tr.val_loss_ema
    out = capsys.readouterr().out
    lines = [l for l in out.splitlines() if l.startswith("[VALIDATION]")]
    assert len(lines) == 2 and "val_loss_ema" in lines[1] and "ema" not in lines[0]
    assert _files(tmp_path / "results") == ["last_model.pth", "last_model_ema.pth"]
    run_dir = glob.glob(str(tmp_path / "runs" / "*"))
    assert len(run_dir) == 1 and _files(run_dir[0]) == ["model-e0-ema.pth", "model-e0.pth"]
    saved = torch.load(os.path.join(run_dir[0], "model-e0-ema.pth"), weights_only=True)      # a plain state_dict
    assert list(saved) == list(tr.model.state_dict())
    for k, v in ema.module.state_dict().items():
        assert torch.equal(saved[k], v)
    # the second pass can be turned off
    tr.validate_ema = False
    logged.clear()
    tr.validate(1)
    assert len(logged) == 1 and "val_loss" in logged[0]


def test_trainer_without_the_keys_writes_and_prints_what_it_did(tmp_path, monkeypatch, capsys):
    monkeypatch.chdir(tmp_path)
    torch.manual_seed(5)
    tr = _trainer(tmp_path, 1)
    assert tr.step.ema is None and not tr.save_state and tr.resume_from is None
    logged = []
    tr._log = logged.append
    tr.run()
    assert not hasattr(tr, "val_loss_ema") and all("ema" not in k for p in logged for k in p)
    out = capsys.readouterr().out
    assert "ema" not in out
    lines = out.splitlines()
    assert sum(l.startswith("[VALIDATION] epoch 0\t| total_batch 3\t| val_loss ") for l in lines) == 1
    assert sum(l.startswith("MODEL SAVED to .") and l.endswith("/model-e0.pth") for l in lines) == 1
    assert sum(l.startswith("epoch 0\t| batch ") for l in lines) == 3 and lines[0].startswith("Model total parameters: ")
    assert len(lines) == 6
    assert _files(tmp_path / "results") == ["last_model.pth"]
    run_dir = glob.glob(str(tmp_path / "runs" / "*"))
    assert len(run_dir) == 1 and _files(run_dir[0]) == ["model-e0.pth"]


def test_trainer_resumes_a_run_bit_for_bit(tmp_path, monkeypatch):
    keys = dict(TRAINING_EMA_DECAY=0.9, TRAINING_SAVE_STATE=True)
    a_dir, b_dir = tmp_path / "a", tmp_path / "b"
    a_dir.mkdir()
    b_dir.mkdir()
    monkeypatch.chdir(a_dir)
    torch.manual_seed(5)
    straight = _trainer(a_dir, 2, **keys)
    straight.run()
    assert _files(a_dir / "results") == ["last_model.pth", "last_model_ema.pth", "last_state.pth"]
    assert {"model-e0.pth", "model-e1.pth", "state-e0.pth", "state-e1.pth", "model-e0-ema.pth", "model-e1-ema.pth"} == set(_files(glob.glob(str(a_dir / "runs" / "*"))[0]))
    monkeypatch.chdir(b_dir)
    torch.manual_seed(5)
    first = _trainer(b_dir, 1, **keys)
    first.run()
    state = torch.load("./results/last_state.pth", weights_only=True)
    assert set(state) == {"epoch", "global_step", "step", "torch_rng"} and state["epoch"] == 0 and state["global_step"] == 4
    torch.manual_seed(99)                                         # whatever happened to the generator in between
    second = _trainer(b_dir, 2, TRAINING_RESUME_FROM="./results/last_state.pth", **keys)
    assert second.start_epoch == 1 and second.global_step == 4 and second.step.optimizer._steps == 4 and second.step.ema.num_updates == 4
    seen = []
    train = second.train
    second.train = lambda epoch: (seen.append(epoch), train(epoch))[1]
    second.run()
    assert seen == [1] and second.global_step == 8 == straight.global_step
    assert any("model-e1.pth" in _files(d) for d in glob.glob(str(b_dir / "runs" / "*")))
    for got, want in ((second.model, straight.model), (second.step.ema.module, straight.step.ema.module)):
        assert torch.equal(_vit(got).flat_parameters()[0], _vit(want).flat_parameters()[0])
    assert second.step.ema.num_updates == straight.step.ema.num_updates == 8
    # the per-epoch state file pairs with the per-epoch model file
    run_dir = [d for d in glob.glob(str(b_dir / "runs" / "*")) if "state-e0.pth" in _files(d)][0]
    third = _trainer(b_dir, 2, TRAINING_RESUME_FROM=os.path.join(run_dir, "state-e0.pth"), **keys)
    assert third.start_epoch == 1 and third.global_step == 4
    assert torch.equal(_vit(third.model).flat_parameters()[0], _vit(first.model).flat_parameters()[0])
