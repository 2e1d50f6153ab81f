"""The weight average and the resumable training state without a GPU: the restatement of the update (tests/ema_ref.py) against numpy and
torch, the exact fixed point, the decay rule, the C boundary (nv_ema_update), the Trainer's config helpers, and the layout and refusals
of TrainStep.state_dict / load_state_dict on a CPU-resident model (no device work is involved in either)."""
import ctypes
import re

import numpy as np
import pytest
import torch

import ema_ref as E
import weights as W

SIZE = dict(TRAINING_VIT_DIM=128, TRAINING_VIT_DEPTH=2, TRAINING_VIT_HEADS=2, TRAINING_VIT_MLP_DIM=256)


def rnd(*shape, seed=0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


# ------------------------------------------------------------------------------------------ 1. per-operation equality
@pytest.mark.parametrize("w", [0.0, 1.0, float(np.float32(1e-4)), float(np.float32(0.1)), float(E.weight32(0.9999))])
def test_update_is_the_per_operation_float32_evaluation(w):
    e, p = rnd(4099, seed=1), rnd(4099, seed=2)
    e[::7] = p[::7]                                              # cells at the fixed point
    e[5], p[6] = 1e-42, -3e-45                                   # denormals
    e[10], p[11], e[12], p[12] = float("inf"), float("-inf"), float("inf"), float("inf")
    e[20], p[21] = float("nan"), float("nan")
    got = E.update(e, p, w)
    assert E.same_bits(got, torch.from_numpy(E.update_np(e.numpy(), p.numpy(), w)))
    assert E.same_bits(got, e + (p - e) * w)                     # the expression of the issue, Python float w
    keep = torch.isfinite(e) & torch.isfinite(p) & (e == p)
    assert torch.equal(got[keep], e[keep])
    if w > 0:
        assert torch.isnan(got[12]) and torch.isnan(got[20]) and torch.isnan(got[21])      # inf - inf, NaN in either operand


def test_weight_is_one_rounding_of_the_double_difference():
    for d in (0.9999, 0.999, 0.0, 2.0 / 11.0, 0.9999 ** 4):
        from neurovit_amd.optim import ema_weight
        assert ema_weight(d) == float(E.weight32(d)) == float(np.float32(np.float64(1.0) - np.float64(d)))


# ------------------------------------------------------------------------------------------ 2. the exact fixed point
def test_fixed_point_is_exact_and_the_two_product_form_drifts():
    p = rnd(100000, seed=0)
    w = E.weight32(0.9999)
    e, q = p.clone(), p.clone()
    for _ in range(20000):
        e = E.update(e, p, w)
        q = E.two_product(q, p, 0.9999)
    assert torch.equal(e, p)
    assert not torch.equal(q, p)
    drift = float(((q - p).abs() / p.abs().clamp_min(1e-30)).max())
    assert drift > 1e-6, drift                                   # (1.7e-4 measured: the two rounded factors do not sum to one)


# ------------------------------------------------------------------------------------------ 3. the decay rule
def test_decay_rule():
    from neurovit_amd.optim import ema_decay_at
    want = {1: 2.0 / 11.0, 10: 11.0 / 20.0, 1000: 1001.0 / 1010.0, 10 ** 6: 0.9999}
    for t, d in want.items():
        assert E.decay_at(t, 0.9999) == d == ema_decay_at(t, 0.9999)
        assert E.decay_at(t, 0.9999, warmup=False) == 0.9999 == ema_decay_at(t, 0.9999, False)
        assert E.decay_at(t, 0.9999, update_every=4) == d ** 4 == ema_decay_at(t, 0.9999, True, 4)
        assert E.decay_at(t, 0.9999, warmup=False, update_every=4) == 0.9999 ** 4 == ema_decay_at(t, 0.9999, False, 4)
    assert E.decay_at(10 ** 6, 0.9999) < (1.0 + 10 ** 6) / (10.0 + 10 ** 6)


def test_replay_counts_every_call_and_averages_every_kth():
    start, snaps = rnd(64, seed=3), [rnd(64, seed=10 + i) for i in range(5)]
    e, t = E.replay(start, snaps, 0.99, warmup=True, update_every=2)
    assert t == 5
    want = E.update(start, snaps[1], E.weight32(E.decay_at(2, 0.99, True, 2)))
    want = E.update(want, snaps[3], E.weight32(E.decay_at(4, 0.99, True, 2)))
    assert torch.equal(e, want)


# ------------------------------------------------------------------------------------------ 4. the boundary
def test_header_declares_and_library_exports_nv_ema_update():
    from neurovit_amd._cabi import HEADER, LIB_PATH, parse_header
    protos = parse_header()
    assert "nv_ema_update" in protos
    restype, argtypes = protos["nv_ema_update"]
    assert restype is ctypes.c_int
    assert argtypes == [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_long, ctypes.c_float, ctypes.c_int, ctypes.c_void_p]
    dll = ctypes.CDLL(LIB_PATH)
    assert hasattr(dll, "nv_ema_update")
    assert re.search(r"#define\s+NV_ABI_VERSION\s+8\b", open(HEADER).read())
    assert dll.nv_abi_version() == 8


def test_library_refuses_bad_arguments_before_any_launch():
    """count, alignment and weight are checked on the host: the calls below never reach a device (there is none here)"""
    from neurovit_amd._cabi import last_error, lib
    a, b = 1 << 20, 2 << 20                                     # 16-byte aligned addresses that are never dereferenced
    call = lambda ema, p, count, weight: lib.nv_ema_update(ema, p, count, weight, 0, None)
    for args in ((a, b, 6, 0.1), (a, b, 0, 0.1), (a, b, -4, 0.1), (a + 4, b, 8, 0.1), (a, b + 8, 8, 0.1), (None, b, 8, 0.1), (a, None, 8, 0.1),
                 (a, b, 8, 1.5), (a, b, 8, -0.1), (a, b, 8, float("nan")), (a, b, 8, float("inf"))):
        assert call(*args) != 0, args
        assert "nv_ema_update" in last_error()


# ------------------------------------------------------------------------------------------ 5. config helpers
def test_trainer_reads_the_ema_keys():
    from neurovit_amd.trainer import Trainer
    read = Trainer.ema_from_config
    assert read({}) == {} and read({"TRAINING_EMA_DECAY": None}) == {}
    assert read({"TRAINING_EMA_WARMUP": False, "TRAINING_EMA_UPDATE_EVERY": 3}) == {}           # no decay: off, whatever else is set
    assert read({"TRAINING_EMA_DECAY": 0.999}) == dict(ema_decay=0.999, ema_warmup=True, ema_update_every=1)
    assert read({"TRAINING_EMA_DECAY": 0, "TRAINING_EMA_WARMUP": False, "TRAINING_EMA_UPDATE_EVERY": 4}) == dict(ema_decay=0.0, ema_warmup=False, ema_update_every=4)
    for bad in (1.0, 1.5, -0.1, float("nan")):
        with pytest.raises(ValueError):
            read({"TRAINING_EMA_DECAY": bad})
    for bad in ("0.99", True):
        with pytest.raises(TypeError):
            read({"TRAINING_EMA_DECAY": bad})
    for bad in (0, -2):
        with pytest.raises(ValueError):
            read({"TRAINING_EMA_DECAY": 0.9, "TRAINING_EMA_UPDATE_EVERY": bad})
    for bad in (1.5, "2", True):
        with pytest.raises(TypeError):
            read({"TRAINING_EMA_DECAY": 0.9, "TRAINING_EMA_UPDATE_EVERY": bad})
    for bad in (1, "yes", None):
        with pytest.raises(TypeError):
            read({"TRAINING_EMA_DECAY": 0.9, "TRAINING_EMA_WARMUP": bad})


def test_trainer_reads_the_state_keys():
    from neurovit_amd.trainer import Trainer
    read = Trainer.state_options_from_config
    assert read({}) == (False, None) and read({"TRAINING_SAVE_STATE": None, "TRAINING_RESUME_FROM": None}) == (False, None)
    assert read({"TRAINING_SAVE_STATE": True, "TRAINING_RESUME_FROM": "runs/x/state-e3.pth"}) == (True, "runs/x/state-e3.pth")
    for bad in (1, "true", 0.0):
        with pytest.raises(TypeError):
            read({"TRAINING_SAVE_STATE": bad})
    for bad in (3, "", True):
        with pytest.raises(TypeError):
            read({"TRAINING_RESUME_FROM": bad})
    pair = Trainer.model_file_of_state
    assert pair("runs/x/state-e3.pth") == "runs/x/model-e3.pth" and pair("./results/last_state.pth") == "./results/last_model.pth"
    assert pair("state-e12.pth") == "model-e12.pth"
    for bad in ("runs/x/model-e3.pth", "runs/x/state-e.pth", "runs/x/state-e3.pt", "runs/x/state-eN.pth"):
        with pytest.raises(ValueError):
            pair(bad)


def test_trainer_hands_the_keys_to_its_step_and_stays_plain_without_them():
    from neurovit_amd.trainer import Trainer
    import neurovit_amd.NeuroEncoder as ne
    ds = torch.utils.data.TensorDataset(torch.zeros(2, 1), torch.zeros(2, 1), torch.zeros(2, 32, 32, 32), torch.zeros(2, dtype=torch.long))
    cfg = dict(W.neuro_config(32, 8, DEVICE="cpu", **SIZE), GLOBAL_OUTPUT_DIR="unused", TRAINING_EPOCHS=1, TRAINING_BATCH_SIZE=2, TRAINING_NUM_WORKERS=0)
    trainer = Trainer(cfg, ne.NeuroEncoder(cfg), ds, ds)
    assert trainer.step.ema is None and trainer.save_state is False and trainer.resume_from is None and trainer.start_epoch == 0
    with pytest.raises(ValueError, match="cuda"):                # the key reaches TrainStep, which refuses a CPU-resident model
        Trainer(dict(cfg, TRAINING_EMA_DECAY=0.99), ne.NeuroEncoder(cfg), ds, ds)


# ------------------------------------------------------------------------------------------ 6. ModelEma / TrainStep: arguments, state layout, refusals
def _cpu_model(**extra):
    import neurovit_amd.NeuroEncoder as ne
    return ne.NeuroEncoder(W.neuro_config(32, 8, DEVICE="cpu", **SIZE, **extra))


def test_model_ema_refusals_come_before_any_device_work():
    from neurovit_amd import ModelEma
    from neurovit_amd.trainer import TrainStep
    model = _cpu_model()
    for bad in (1.0, -0.5, 2, float("nan")):
        with pytest.raises(ValueError):
            ModelEma(model, decay=bad)
        with pytest.raises(ValueError):
            TrainStep(model, ema_decay=bad)
    with pytest.raises(TypeError):
        ModelEma(model, decay="0.9")
    for bad in (0, -1):
        with pytest.raises(ValueError):
            ModelEma(model, update_every=bad)
        with pytest.raises(ValueError):
            TrainStep(model, ema_decay=0.9, ema_update_every=bad)
    with pytest.raises(TypeError):
        ModelEma(model, update_every=2.0)
    with pytest.raises(TypeError):
        ModelEma(torch.nn.Linear(2, 2))
    with pytest.raises(ValueError, match="cuda"):
        ModelEma(model)
    with pytest.raises(ValueError, match="cuda"):
        TrainStep(model, ema_decay=0.999)
    assert TrainStep(model).ema is None


def test_twin_has_the_models_keys_values_and_settings_and_leaves_model_and_generator_alone():
    from neurovit_amd.NeuroEncoder import NeuroEncoder, twin_of
    model = _cpu_model(TRAINING_VIT_OPERANDS="fp16", TRAINING_VIT_EVAL_PRECISION="fp32")
    model.volume_encoder.vit3d.fold_layernorm = False
    before = {k: v.clone() for k, v in model.state_dict().items()}
    rng = torch.get_rng_state()
    twin = twin_of(model)
    assert torch.equal(torch.get_rng_state(), rng)
    assert isinstance(twin, NeuroEncoder) and twin is not model
    sd = twin.state_dict()
    assert list(sd) == list(before)
    for k, v in model.state_dict().items():
        assert torch.equal(v, before[k]) and torch.equal(sd[k], v) and sd[k].data_ptr() != v.data_ptr(), k
    vit = twin.volume_encoder.vit3d
    assert (vit.operands, vit.eval_precision, vit.fold_layernorm) == ("fp16", "fp32", False)
    assert vit._rt is not model.volume_encoder.vit3d._rt


def test_mark_arena_rewritten_invalidates_the_shadow_and_moves_the_generation():
    vit = _cpu_model().volume_encoder.vit3d
    vit.flat_parameters()
    vit._shadow_key = tuple(p._version for p in vit._plist)
    key = vit._param_key()
    vit.mark_arena_rewritten()
    assert vit._shadow_key is None and vit._param_key() != key and vit._param_generation == key[0] + 1


STATE_KEYS = {"version", "operands", "steps", "hyper", "arenas", "rest", "scaler", "static_scale", "ema"}


def test_state_dict_layout():
    from neurovit_amd.trainer import TrainStep
    model = _cpu_model()
    step = TrainStep(model, lr=3e-4, weight_decay=0.05, loss_scale=128.0)
    step.optimizer._steps = 7
    vit = model.volume_encoder.vit3d
    m, v = step.optimizer.arena_state(vit)
    m.fill_(0.25)
    v.fill_(0.5)
    state = step.state_dict()
    assert set(state) == STATE_KEYS
    assert state["version"] == TrainStep.STATE_VERSION == 1 and state["operands"] == "bf16" and state["steps"] == 7
    assert state["hyper"] == dict(lr=3e-4, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.05)
    assert state["rest"] is None and state["scaler"] is None and state["ema"] is None and state["static_scale"] == 128.0
    n = vit.flat_parameters()[0].numel()
    assert len(state["arenas"]) == 1 and set(state["arenas"][0]) == {"numel", "exp_avg", "exp_avg_sq"} and state["arenas"][0]["numel"] == n
    assert torch.equal(state["arenas"][0]["exp_avg"], m) and torch.equal(state["arenas"][0]["exp_avg_sq"], v)
    assert state["arenas"][0]["exp_avg"].data_ptr() != m.data_ptr()          # clones: later steps do not change a saved state
    assert not any(k.startswith("volume_encoder") for k in state)            # the parameters are not part of it
    # a round trip through a file, into a fresh step: in place
    import io
    buf = io.BytesIO()
    torch.save(state, buf)
    buf.seek(0)
    loaded = torch.load(buf, weights_only=True)
    other = TrainStep(_cpu_model())
    m2, v2 = other.optimizer.arena_state(other._vit)
    ptrs = (m2.data_ptr(), v2.data_ptr())
    other.load_state_dict(loaded)
    m3, v3 = other.optimizer.arena_state(other._vit)
    assert (m3.data_ptr(), v3.data_ptr()) == ptrs and torch.equal(m3, m) and torch.equal(v3, v)
    g0 = other.optimizer.param_groups[0]
    assert other.optimizer._steps == 7 and other.static_scale == 128.0 and (g0["lr"], g0["weight_decay"], tuple(g0["betas"]), g0["eps"]) == (3e-4, 0.05, (0.9, 0.999), 1e-8)


def test_state_dict_refusals_change_nothing():
    from neurovit_amd.trainer import TrainStep
    step = TrainStep(_cpu_model(), accumulation_steps=2)
    step._micro = 1                                               # inside a window
    with pytest.raises(RuntimeError, match="window"):
        step.state_dict()
    step._micro = 0
    good = step.state_dict()
    target = TrainStep(_cpu_model())
    m, v = target.optimizer.arena_state(target._vit)
    m.fill_(1.0)
    v.fill_(2.0)
    target.optimizer._steps = 3
    small = dict(good, arenas=[dict(numel=good["arenas"][0]["numel"] - 4, exp_avg=good["arenas"][0]["exp_avg"][:-4], exp_avg_sq=good["arenas"][0]["exp_avg_sq"][:-4])])
    cases = {"version": dict(good, version=99), "operands": dict(good, operands="fp16"), "arena": small, "arenas": dict(good, arenas=[]),
             "loss scale": dict(good, scaler=torch.zeros(16)), "average": dict(good, ema={"module": {}, "num_updates": 0})}
    for word, bad in cases.items():
        with pytest.raises(ValueError, match=word):
            target.load_state_dict(bad)
        assert bool((m == 1.0).all()) and bool((v == 2.0).all()) and target.optimizer._steps == 3 and target.static_scale == 0.0, word
