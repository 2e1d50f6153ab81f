"""Gradient-norm clipping, the parts that need no GPU: the C-ABI additions, the restatement of clip_grad_norm_'s norm and
coefficient that the GPU tests use as their expectation (pinned to torch here), and the argument / config handling."""
import ctypes
import math
import re

import pytest
import torch

import weights as W

SIZE = dict(TRAINING_VIT_DIM=128, TRAINING_VIT_DEPTH=2, TRAINING_VIT_HEADS=2, TRAINING_VIT_MLP_DIM=256)


def norm_and_coef(tensors, max_norm, factor=1.0):
    """(total_norm, clip_coef_clamped) of torch.nn.utils.clip_grad_norm_(norm_type 2) for the gradients `factor * t`, as fp32 0-dim
    tensors: the squares are summed in double, the norm is rounded to fp32 once, the coefficient is formed in fp32 as torch does."""
    sumsq = 0.0
    for t in tensors:
        sumsq += float((t.detach().double().cpu() ** 2).sum())
    total = torch.tensor(math.sqrt(sumsq) * abs(factor), dtype=torch.float64).to(torch.float32)
    coef = torch.clamp(max_norm / (total + 1e-6), max=1.0)
    return total, coef


def _rnd(*shape, seed=0, scale=1.0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale


def _torch_clip(grads, max_norm):
    ps = [torch.nn.Parameter(torch.zeros_like(g)) for g in grads]
    for p, g in zip(ps, grads):
        p.grad = g.clone()
    total = torch.nn.utils.clip_grad_norm_(ps, max_norm)
    return total, [p.grad for p in ps]


@pytest.mark.parametrize("max_norm", [0.5, 1e9])
def test_restatement_matches_clip_grad_norm(max_norm):
    """a binding and a non-binding bound: norm, coefficient and clipped gradients against torch (fp32 vector_norm: a few 1e-7)"""
    grads = [_rnd(37, 5, seed=1), _rnd(1000, seed=2, scale=0.1), _rnd(3, seed=3)]
    total, clipped = _torch_clip(grads, max_norm)
    t, c = norm_and_coef(grads, max_norm)
    assert t.dtype == torch.float32 and c.dtype == torch.float32
    assert abs(float(t) - float(total)) <= 1e-6 * float(total)
    binding = max_norm < float(total)
    assert (float(c) < 1.0) == binding
    if not binding:
        assert float(c) == 1.0
    for g, want in zip(grads, clipped):
        assert ((g * c - want).abs().max() <= 1e-6 * want.abs().max()).item()
    # a gradient factor (1 / world, 1 / loss scale) scales the norm
    t2, _ = norm_and_coef([g * 8 for g in grads], max_norm, factor=0.125)
    assert abs(float(t2) - float(t)) <= 1e-6 * float(t)


def test_restatement_follows_torch_on_inf_and_nan():
    grads = [_rnd(64, seed=4), _rnd(9, seed=5)]
    grads[1][3] = float("inf")
    total, clipped = _torch_clip(grads, 1.0)
    t, c = norm_and_coef(grads, 1.0)
    assert math.isinf(float(total)) and math.isinf(float(t)) and float(c) == 0.0
    assert torch.equal(clipped[0], grads[0] * c)               # every finite gradient becomes 0
    grads[1][3] = float("nan")
    total, clipped = _torch_clip(grads, 1.0)
    t, c = norm_and_coef(grads, 1.0)
    assert math.isnan(float(total)) and math.isnan(float(t)) and math.isnan(float(c))
    assert torch.isnan(clipped[0]).all()


def test_header_declares_and_library_exports_the_new_symbols():
    from neurovit_amd import ops
    from neurovit_amd._cabi import HEADER, LIB_PATH, parse_header
    protos = parse_header()
    dll = ctypes.CDLL(LIB_PATH)
    for name in ("nv_grad_sumsq", "nv_grad_clip_finish", "nv_adamw_step_clipped"):
        assert name in protos, name
        assert hasattr(dll, name), name
    # the clipped step takes nv_adamw_step_scaled's arguments plus the clip block in front of the stream
    scaled, clipped = protos["nv_adamw_step_scaled"][1], protos["nv_adamw_step_clipped"][1]
    assert clipped == scaled[:-1] + [ctypes.c_void_p] + scaled[-1:]
    src = open(HEADER).read()
    assert re.search(r"#define\s+NV_ABI_VERSION\s+8\b", src)
    assert dll.nv_abi_version() == 8
    blocks = int(re.search(r"#define\s+NV_GRAD_CLIP_MAX_BLOCKS\s+(\d+)", src).group(1))
    m = re.search(r"#define\s+NV_GRAD_CLIP_BYTES\s+\((\d+)\s*\+\s*(\d+)\s*\*\s*NV_GRAD_CLIP_MAX_BLOCKS\)", src)
    assert m, "NV_GRAD_CLIP_BYTES"
    assert int(m.group(1)) + int(m.group(2)) * blocks == 4 * ops.GRAD_CLIP_FLOATS
    assert int(m.group(1)) == 4 * 16 and (ops.GC_TOTAL_NORM, ops.GC_COEF) == (2, 3)      # header of the block: common.h GC_*


def _cpu_model():
    import neurovit_amd.NeuroEncoder as ne
    return ne.NeuroEncoder(W.neuro_config(32, 8, DEVICE="cpu", **SIZE))


@pytest.mark.parametrize("bad", [0, 0.0, -1.0, float("inf"), float("nan"), "one", True])
def test_trainstep_refuses_a_max_grad_norm_that_is_not_finite_and_positive(bad):
    from neurovit_amd.trainer import TrainStep
    with pytest.raises(ValueError):
        TrainStep(_cpu_model(), max_grad_norm=bad)


def test_trainstep_arguments():
    from neurovit_amd.trainer import TrainStep
    model = _cpu_model()
    with pytest.raises(AssertionError):
        TrainStep(model, max_grad_norm=1.0, overlap_optimizer=True)
    off = TrainStep(model)
    assert off.max_grad_norm is None and off.clipper is None and off.last_grad_norm is None and off.last_clip_coef is None
    on = TrainStep(model, max_grad_norm=2)
    assert on.max_grad_norm == 2.0 and on.clipper.max_norm == 2.0
    for t in (on.last_grad_norm, on.last_clip_coef):
        assert t.dim() == 0 and t.dtype == torch.float32
    assert on.last_grad_norm.data_ptr() != on.last_clip_coef.data_ptr()
    assert on.last_grad_norm.untyped_storage().data_ptr() == on.clipper.state.untyped_storage().data_ptr()      # views, not copies


def test_trainer_reads_the_config_key():
    from neurovit_amd.trainer import Trainer
    read = Trainer.grad_clip_from_config
    assert read({}) is None and read({"TRAINING_GRAD_CLIP": None}) is None
    assert read({"TRAINING_GRAD_CLIP": 0}) is None and read({"TRAINING_GRAD_CLIP": 0.0}) is None
    assert read({"TRAINING_GRAD_CLIP": 1}) == 1.0 and read({"TRAINING_GRAD_CLIP": 0.25}) == 0.25
    for bad in (-1, float("inf"), float("nan"), "1.0x"):
        with pytest.raises(ValueError):
            read({"TRAINING_GRAD_CLIP": bad})


def test_trainer_hands_the_key_to_its_step():
    from neurovit_amd.trainer import Trainer
    ds = torch.utils.data.TensorDataset(torch.zeros(2, 1), torch.zeros(2, 1), torch.zeros(2, 32, 32, 32), torch.zeros(2, dtype=torch.long))
    base = dict(W.neuro_config(32, 8, DEVICE="cpu", **SIZE), GLOBAL_OUTPUT_DIR="unused", TRAINING_EPOCHS=1, TRAINING_BATCH_SIZE=2, TRAINING_NUM_WORKERS=0)
    for extra, want in (({}, None), ({"TRAINING_GRAD_CLIP": 0}, None), ({"TRAINING_GRAD_CLIP": 0.5}, 0.5)):
        cfg = dict(base, **extra)
        import neurovit_amd.NeuroEncoder as ne
        trainer = Trainer(cfg, ne.NeuroEncoder(cfg), ds, ds)
        assert trainer.step.max_grad_norm == want
