"""Stochastic depth without a GPU: the restatement (tests/drop_path_ref.py) against torch and against the oracle, the statistics of the
draw rule, the published C-ABI, the argument checks that precede every launch, and the Python surface (ViT keywords, the config key,
TrainStep's plan, the refusals)."""
import ctypes
import math

import numpy as np
import pytest
import torch

import drop_path_ref as dpr
import weights as W
from oracle import ref_cpu

SEEDS = (1234, 20261020, 0x5EED)
NEW_SYMBOLS = ("nv_drop_path_draw", "nv_gemm_bf16_path", "nv_skinny_nt_path", "nv_ln_bwd_path", "nv_head_bwd_path", "nv_head_step_path",
               "nv_vit_forward_sd", "nv_vit_backward_sd", "nv_vit_train_step_sd")
SIZE = dict(TRAINING_VIT_DIM=64, TRAINING_VIT_DEPTH=2, TRAINING_VIT_HEADS=1, TRAINING_VIT_MLP_DIM=128)


# ------------------------------------------------------------------------------------------------ the restatement
@pytest.mark.parametrize("rate,depth", [(0.1, 12), (0.2, 12), (0.5, 2), (0.3, 7)])
def test_linear_schedule_is_torch_linspace(rate, depth):
    want = torch.linspace(0, float(np.float32(rate)), depth, dtype=torch.float64).numpy()
    assert np.abs(dpr.schedule(rate, depth) - want).max() <= 1e-15
    assert dpr.schedule(rate, 1).tolist() == [0.0]
    assert dpr.schedule(rate, depth, dpr.CONSTANT).tolist() == [float(np.float32(rate))] * depth


@pytest.mark.parametrize("seed", SEEDS)
def test_draw_statistics(seed):
    """rate 0.2, depth 12, B 4096: the dropped share of every site within 4 sigma of q_l (binomial), and the joint drops of the two
    branches of a layer and of the same branch of neighbouring layers within 4 sigma of independence.  Kept factors are 1 / (1 - q_l) in fp32."""
    depth, B, rate = 12, 4096, 0.2
    t = dpr.draw_table(seed, B, depth, rate).numpy()
    q = dpr.schedule(rate, depth)
    dropped = t == 0
    for l in range(depth):
        kept = np.float32(1.0) / (np.float32(1.0) - np.float32(q[l]))
        assert set(np.unique(t[l]).tolist()) <= {0.0, float(kept)}
        for c in range(2):
            n, sigma = int(dropped[l, c].sum()), math.sqrt(B * q[l] * (1 - q[l]))
            assert abs(n - B * q[l]) <= 4 * sigma, (l, c, n, B * q[l], sigma)
        pj = q[l] * q[l]
        assert abs(int((dropped[l, 0] & dropped[l, 1]).sum()) - B * pj) <= 4 * math.sqrt(B * pj * (1 - pj)), ("branches", l)
        if l + 1 < depth:
            pn = q[l] * q[l + 1]
            for c in range(2):
                assert abs(int((dropped[l, c] & dropped[l + 1, c]).sum()) - B * pn) <= 4 * math.sqrt(B * pn * (1 - pn)), ("layers", l, c)
    assert (t[0] == 1.0).all()                                                 # q_0 = 0: nothing hashed, nothing dropped
    assert not np.array_equal(t, dpr.draw_table(seed + 1, B, depth, rate).numpy())
    assert (dpr.draw_table(seed, 7, 3, 0.0).numpy() == 1.0).all()


def _micro(B=2):
    sd = W.make_tensors(W.vit_param_spec(**W.MICRO), 1)
    S = W.MICRO["image_size"]
    return sd, ref_cpu.ViTCfg(**W.MICRO), ref_cpu.fmri_to_video(W.make_volume((B, S, S, S), 2))


@pytest.mark.parametrize("dropout", [None, (0.1, 0.2, 77)])
@pytest.mark.parametrize("emulate", [False, True])
def test_an_all_ones_table_is_the_oracle_forward(emulate, dropout):
    sd, cfg, video = _micro()
    with torch.no_grad():
        want = ref_cpu.vit_forward(sd, cfg, video, emulate_bf16=emulate, dropout=dropout)
        got = dpr.vit_forward_sd(sd, cfg, video, torch.ones(cfg.depth, 2, 2), emulate_bf16=emulate, dropout=dropout)
    assert torch.equal(got, want)


def test_a_dropped_sample_passes_through_the_blocks():
    sd, cfg, video = _micro()
    table = torch.ones(cfg.depth, 2, 2)
    table[:, :, 1] = 0
    taps, plain = {}, {}
    with torch.no_grad():
        dpr.vit_forward_sd(sd, cfg, video, table, taps=taps)
        ref_cpu.vit_forward(sd, cfg, video, taps=plain)
    assert torch.equal(taps[f"block{cfg.depth - 1}"][1], taps["A5"][1])
    assert torch.equal(taps[f"block{cfg.depth - 1}"][0], plain[f"block{cfg.depth - 1}"][0])


def test_the_restatement_yields_gradients():
    sd, cfg, video = _micro()
    leaves = {k: v.clone().requires_grad_(True) for k, v in sd.items()}
    table = torch.ones(cfg.depth, 2, 2)
    table[1, 1, 0] = 0                     # sample 0 skips the last FeedForward: its FC2 weight sees sample 1 alone
    dpr.vit_forward_sd(leaves, cfg, video, table).sum().backward()
    g = leaves["transformer.layers.1.1.net.4.weight"].grad
    assert g is not None and torch.isfinite(g).all() and g.abs().sum() > 0


# ------------------------------------------------------------------------------------------------ header and binding
def test_header_and_binding_declare_the_new_entry_points():
    from neurovit_amd import _cabi
    dll = ctypes.CDLL(_cabi.LIB_PATH)
    for name in NEW_SYMBOLS:
        assert name in _cabi.lib.protos, name
        assert getattr(dll, name) is not None, name
    header = open(_cabi.HEADER).read()
    assert "#define NV_ABI_VERSION 8" in header and _cabi.ABI_VERSION == 8 and _cabi.lib.nv_abi_version() == 8
    assert "#define NV_DROP_PATH_LINEAR 0" in header and "#define NV_DROP_PATH_CONSTANT 1" in header
    assert "typedef struct nv_vit_drop_path" in header
    assert _cabi.DROP_PATH_SCHEDULES == {"linear": 0, "constant": 1}
    assert ctypes.sizeof(_cabi.DropPath) == 16 and [f[0] for f in _cabi.DropPath._fields_] == ["struct_size", "factors"]
    protos = _cabi.lib.protos
    # the existing argument lists plus (path, path_rows) / plus the table
    for name in ("nv_gemm_bf16", "nv_skinny_nt", "nv_ln_bwd", "nv_head_bwd"):
        assert protos[name + "_path"][1] == protos[name][1] + [ctypes.c_void_p, ctypes.c_int], name
    assert protos["nv_head_step_path"][1] == protos["nv_head_step_soft"][1] + [ctypes.c_void_p, ctypes.c_int]
    for name, base in (("nv_vit_forward_sd", "nv_vit_forward_in"), ("nv_vit_backward_sd", "nv_vit_backward_attn"), ("nv_vit_train_step_sd", "nv_vit_train_step_ex")):
        assert protos[name][1] == protos[base][1] + [ctypes.c_void_p], name


def test_entry_points_refuse_bad_arguments_before_any_launch():
    from neurovit_amd import _cabi, engine
    lib = _cabi.lib
    fake = 1 << 20                                                        # an aligned address nothing dereferences: every call below is refused first
    draw = lambda **kw: lib.nv_drop_path_draw(*[dict(dict(seed=1, B=4, depth=2, rate=0.1, schedule=0, factors=fake, stream=None), **kw)[k]
                                                for k in ("seed", "B", "depth", "rate", "schedule", "factors", "stream")])
    for bad in (dict(rate=-0.1), dict(rate=1.0), dict(rate=float("nan")), dict(schedule=2), dict(schedule=-1), dict(B=0), dict(depth=0), dict(factors=None)):
        assert draw(**bad) == -1, bad
    assert "rate" in (draw(rate=1.5), _cabi.last_error())[1]
    # kernel level: a table where no path-aware form exists
    assert lib.nv_gemm_bf16_path(0, 3, 64, 64, 64, fake, 64, fake, 64, fake, 64, fake, None, 0, None, 0, 0, 1.0, 0, 0.0, None, fake, 9) == -1 and "epilogue 4" in _cabi.last_error()
    assert lib.nv_gemm_bf16_path(1, 4, 64, 64, 64, fake, 64, fake, 64, fake, 64, fake, fake, 64, None, 0, 0, 1.0, 0, 0.0, None, fake, 9) == -1
    assert lib.nv_gemm_bf16_path(0, 4, 64, 64, 64, fake, 64, fake, 64, fake, 64, fake, fake, 64, None, 0, 0, 1.0, 0, 0.0, None, fake, 0) == -1 and "path_rows" in _cabi.last_error()
    assert lib.nv_skinny_nt_path(1, 3, 64, 64, fake, 64, fake, 64, fake, None, 0, fake, 64, None, 0, 0, 0.0, None, fake, 9) == -1 and "epilogue 0" in _cabi.last_error()
    assert lib.nv_skinny_nt_path(0, 3, 64, 64, fake, 64, fake, 64, fake, fake, 64, fake, 100, None, 0, 0, 0.0, None, fake, 9) == -1       # ldo no multiple of N
    assert lib.nv_ln_bwd_path(fake, 64, fake, 64, fake, fake, fake, 3, 64, fake, fake, 100, fake, 64, None, None, None, 0, fake, 1 << 30, 0, 0.0, None, None, fake, 9) == -1
    assert lib.nv_ln_bwd_path(fake, 64, fake, 64, fake, fake, fake, 3, 64, fake, fake, 64, fake, 64, None, None, None, 0, fake, 1 << 30, 0, 0.0, None, None, fake, 0) == -1
    assert lib.nv_head_bwd_path(fake, 3, 5, fake, fake, 9 * 192, fake, fake, fake, 192, 9, fake, 192, fake, 192, fake, fake, fake, fake, fake, 0, fake, 1 << 30, 0, 0.0, 0, None,
                                fake, 8) == -1 and "path_rows" in _cabi.last_error()
    # engine level: the struct, training forwards only, not the fused 4D form
    cfg = engine.make_config(**W.NOPROJ)
    shape, strides = (ctypes.c_long * 5)(2, 1, 16, 16, 16), (ctypes.c_long * 5)(4096, 4096, 256, 16, 1)
    good = _cabi.DropPath(ctypes.sizeof(_cabi.DropPath), fake)

    def fwd(sd, training=1, inp=None):
        return lib.nv_vit_forward_sd(ctypes.byref(cfg), 2, fake, shape, strides, inp, fake, fake, fake << 4, 1 << 40, training, 0.0, 0.0, 0, fake, None, ctypes.byref(sd))
    assert fwd(_cabi.DropPath(8, fake)) == -1 and "struct_size" in _cabi.last_error()
    assert fwd(_cabi.DropPath(ctypes.sizeof(_cabi.DropPath), None)) == -1 and "factors" in _cabi.last_error()
    assert fwd(good, training=0) == -1 and "training" in _cabi.last_error()
    four_d = _cabi.VitInput(None, 4, 0, None)
    assert fwd(good, inp=ctypes.byref(four_d)) == -1 and "4D" in _cabi.last_error()
    bwd = lambda sd: lib.nv_vit_backward_sd(ctypes.byref(cfg), 2, fake, strides, fake, fake, fake << 4, 1 << 40, fake, fake, None, 0, 0, 3, 0.0, 0.0, 0, None, None, 1, 1,
                                            None, None, ctypes.byref(sd))
    assert bwd(_cabi.DropPath(8, fake)) == -1 and "struct_size" in _cabi.last_error()
    assert bwd(_cabi.DropPath(ctypes.sizeof(_cabi.DropPath), None)) == -1 and "factors" in _cabi.last_error()
    hp = _cabi.TrainHparams(ctypes.sizeof(_cabi.TrainHparams), 1, 1e-3, 0.9, 0.999, 1e-8, 0.0, 1.0, 0, 1, 0, 0.0, None, None)
    step = lambda sd: lib.nv_vit_train_step_sd(ctypes.byref(cfg), 2, fake, shape, strides, None, fake, fake, fake, fake, fake, fake << 4, 1 << 40, fake, fake, fake, fake,
                                               ctypes.byref(hp), None, 0.0, 0.0, 0, None, None, ctypes.byref(sd))
    assert step(_cabi.DropPath(8, fake)) == -1 and "struct_size" in _cabi.last_error()
    assert step(_cabi.DropPath(ctypes.sizeof(_cabi.DropPath), None)) == -1 and "factors" in _cabi.last_error()


# ------------------------------------------------------------------------------------------------ the Python surface
def test_vit_keywords_are_plain_validated_attributes():
    from neurovit_amd.vit_3d import ViT
    m = ViT(**W.NOPROJ)
    assert m.drop_path_rate == 0.0 and m.drop_path_schedule == "linear" and m.last_drop_path is None
    m = ViT(**W.NOPROJ, drop_path_rate=0.1, drop_path_schedule="constant")
    assert m.drop_path_rate == 0.1 and m.drop_path_schedule == "constant"
    assert not [k for k in m.state_dict() if "drop_path" in k]                       # no parameter, no buffer: checkpoints are unchanged
    m.drop_path_rate, m.drop_path_schedule = 0.25, "linear"                           # settable on a built (or loaded) model
    assert m.drop_path_rate == 0.25 and m.transformer.drop_path_rate == 0.25
    for bad in (-0.1, 1.0, 1.5, "0.1", None, True):
        with pytest.raises(ValueError):
            m.drop_path_rate = bad
        with pytest.raises(ValueError):
            ViT(**W.NOPROJ, drop_path_rate=bad)
    with pytest.raises(ValueError):
        m.drop_path_schedule = "cosine"
    with pytest.raises(ValueError):
        ViT(**W.NOPROJ, drop_path_schedule="cosine")
    # the seed of the step: drawn in train mode once the rate is positive, even without dropout; the return shape stays
    m.train()
    p, pe, seed = m.draw_dropout()
    assert (p, pe) == (0.0, 0.0) and seed > 0
    m.eval()
    assert m.draw_dropout() == (0.0, 0.0, 0) and m.draw_drop_path(2, 5, "cpu") is None
    m.train()
    m.drop_path_rate = 0.0
    assert m.draw_dropout() == (0.0, 0.0, 0) and m.draw_drop_path(2, 5, "cpu") is None


def test_config_key_reaches_the_vit():
    import neurovit_amd.NeuroEncoder as ne
    model = ne.NeuroEncoder(W.neuro_config(16, 8, DEVICE="cpu", TRAINING_DROP_PATH=0.1, **SIZE))
    assert model.volume_encoder.vit3d.drop_path_rate == 0.1 and model.volume_encoder.vit3d.drop_path_schedule == "linear"
    plain = ne.NeuroEncoder(W.neuro_config(16, 8, DEVICE="cpu", **SIZE))
    assert plain.volume_encoder.vit3d.drop_path_rate == 0.0
    with pytest.raises(ValueError):
        ne.NeuroEncoder(W.neuro_config(16, 8, DEVICE="cpu", TRAINING_DROP_PATH=1.0, **SIZE))
    with pytest.raises(NotImplementedError, match="3D model"):
        ne.ViT3DEncoder(W.neuro_config(16, 8, dim=4, DEVICE="cpu", TRAINING_DROP_PATH=0.1, **SIZE))
    ne.ViT3DEncoder(W.neuro_config(16, 8, dim=4, DEVICE="cpu", TRAINING_DROP_PATH=0.0, **SIZE))      # rate 0: nothing changes


def test_refusals_that_need_no_device():
    import neurovit_amd.NeuroEncoder as ne
    from neurovit_amd.pretrain import MaskedPretrainStep
    from neurovit_amd.trainer import TrainStep
    model = ne.NeuroEncoder(W.neuro_config(16, 8, DEVICE="cpu", TRAINING_DROP_PATH=0.2, **SIZE))
    vit = model.volume_encoder.vit3d
    with pytest.raises(NotImplementedError, match="drop_path_rate"):
        MaskedPretrainStep(model)
    with pytest.raises(NotImplementedError, match="drop_path_rate"):
        vit.refuse_drop_path("forward_tokens")
    x = torch.zeros(2, 9, 64)
    model.train()
    with pytest.raises(NotImplementedError, match="on its own"):
        vit.transformer(x)
    # a positive rate counts as live dropout: no graph replay
    step = TrainStep(model)
    step._graphs_on = True
    rows = 2 * vit.pos_embedding.shape[1]
    assert not step._plan(rows, vit._dropout_p != (0.0, 0.0) or vit.drop_path_rate > 0, False).graph_ok
    vit.drop_path_rate = 0.0
    assert step._plan(rows, vit._dropout_p != (0.0, 0.0) or vit.drop_path_rate > 0, False).graph_ok
