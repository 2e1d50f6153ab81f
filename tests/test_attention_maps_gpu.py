"""Attention probabilities and attention rollout through the native ViT3D on MI355X (nv_attn_probs, nv_vit_attn_export, nv_attn_rollout;
hooks on every block's `attend`, ViT.attention_maps / attention_rollout, NeuroEncoder.get_attention_rollout).

Gates:
  hooks        a forward hook on each `attend` fires once per forward, in layer order, with the fp32 [B, heads, n, n] probabilities
               (the parent commit never called it: the fused kernels do not run that module);
  fixture      precision("fp32") maps against the imported reference's `attend` outputs (tests/golden/attention.npz): max |dP| <= 1e-5,
               rollout <= 1e-5 relative (max-norm);
  three-way    16-bit operands: max |P_hip - P_fp32| <= max(1.5 max |P_emul - P_fp32|, 1e-4), P_emul / P_fp32 = float64 softmax of the
               emulating / exact oracle's q, k taps; rows sum to 1 within 1e-5;
  forms        max / min head fusion bit-identical to torch's reduction of the per-head export, mean within 2e-7; cls rows bit-identical
               to row 0 of the all-rows form;
  bit-identity logits (plain, LN-folded, fp32, fused 4D, train mode with dropout) and the gradients of a following backward do not move
               when an export is requested.
"""
import pytest
import torch

import weights as W
from oracle import ref_cpu
from test_engine_gpu import report
from test_input_grad_gpu import make_input, make_model, oracle_cfg

pytestmark = pytest.mark.gpu
P729 = dict(W.MICRO, image_size=27, image_patch_size=9, frames=27, frame_patch_size=9)
REFGEO = dict(image_size=90, image_patch_size=9, frames=90, frame_patch_size=9, num_classes=2, dim=1024, depth=2, heads=8,
              mlp_dim=2048, channels=1, dim_head=64, pool="cls")          # the reference default geometry (n = 1001) at depth 2


@pytest.fixture(scope="module", autouse=True)
def gpu():
    from neurovit_amd._cabi import require_gpu
    require_gpu()


def maxabs(a, b):
    return (a.detach().double().cpu() - b.detach().double().cpu()).abs().max().item()


def oracle_probs(cfgdict, sd, video, emulate, dropout=None):
    """float64 softmax(q k^T * scale) of every block from the oracle's q / k taps (16-bit-rounded when emulating)"""
    taps = {}
    ref_cpu.vit_forward(sd, oracle_cfg(cfgdict), video, emulate_bf16=emulate, taps=taps, dropout=dropout)
    out = []
    for l in range(cfgdict["depth"]):
        q, k = taps[f"transformer.layers.{l}.0.q"].double(), taps[f"transformer.layers.{l}.0.k"].double()
        out.append(torch.softmax(q @ k.transpose(-1, -2) * cfgdict["dim_head"] ** -0.5, dim=-1))
    return out


def eval_model(cfgdict, seed):
    m = make_model(cfgdict, seed).eval()
    m.fold_layernorm = False
    return m


# ---------------------------------------------------------------------------------------------------------------- hooks

def test_attend_hooks_fire_once_per_forward_in_layer_order():
    cfg = dict(W.MICRO, depth=3)
    m = eval_model(cfg, 3)
    calls = []

    def hook(module, args, out):
        calls.append((module, args, out.shape, out.dtype, out.device.type))
    for attn, _ in m.transformer.layers:
        attn.attend.register_forward_hook(hook)
    x = make_input(cfg, 2, 4).cuda()
    with torch.no_grad():
        m(x)
    n = m.pos_embedding.shape[1]
    assert [c[0] for c in calls] == [attn.attend for attn, _ in m.transformer.layers]
    assert all(c[1] == () and c[2] == (2, cfg["heads"], n, n) and c[3] == torch.float32 and c[4] == "cuda" for c in calls)
    m.train()                                    # a training forward (graph recorded) fires them as well
    m(x).sum().backward()
    assert len(calls) == 6


def test_hook_on_some_layers_and_removal():
    m = eval_model(W.MICRO, 5)
    seen = []
    h = m.transformer.layers[1][0].attend.register_forward_hook(lambda mod, a, out: seen.append(out.clone()))
    x = make_input(W.MICRO, 2, 6).cuda()
    with torch.no_grad():
        m(x)
        logits_maps, maps = m.attention_maps(x, layers=[1])
    assert len(seen) == 2 and torch.equal(seen[0], maps[1]) and torch.equal(seen[1], maps[1])
    h.remove()
    with torch.no_grad():
        m(x)
    assert len(seen) == 2


def test_hook_returning_a_value_and_pre_hooks_raise():
    m = eval_model(W.MICRO, 7)
    x = make_input(W.MICRO, 1, 8).cuda()
    h = m.transformer.layers[0][0].attend.register_forward_hook(lambda mod, a, out: out * 2)
    with torch.no_grad(), pytest.raises(RuntimeError, match="returned a value"):
        m(x)
    h.remove()
    h = m.transformer.layers[0][0].attend.register_forward_pre_hook(lambda mod, a: None)
    with torch.no_grad(), pytest.raises(NotImplementedError):
        m(x)
    h.remove()


def test_standalone_attention_module_fires_attend_hooks():
    from neurovit_amd.vit_3d import Attention
    torch.manual_seed(0)
    a = Attention(128, heads=2, dim_head=64).cuda()
    got = []
    a.attend.register_forward_hook(lambda mod, args, out: got.append(out))
    x = torch.randn(2, 37, 128, device="cuda")
    a(x)
    assert len(got) == 1 and got[0].shape == (2, 2, 37, 37)
    # the same probabilities from float64 softmax of the bf16-rounded q, k (the module's LayerNorm -> bf16 to_qkv arithmetic)
    xn = torch.nn.functional.layer_norm(x.double(), (128,), a.norm.weight.double(), a.norm.bias.double(), 1e-5)
    qkv = (xn.bfloat16().double() @ a.to_qkv.weight.bfloat16().double().t()).bfloat16().double()
    q, k, _ = (t.reshape(2, 37, 2, 64).permute(0, 2, 1, 3) for t in qkv.chunk(3, dim=-1))
    ref = torch.softmax(q @ k.transpose(-1, -2) / 8.0, dim=-1)
    assert maxabs(got[0], ref) < 2e-3
    assert maxabs(got[0].sum(-1), torch.ones(2, 2, 37)) < 1e-5


# ---------------------------------------------------------------------------------------------------------------- reference fixture

VIT_CASES = [("micro", W.MICRO), ("p729", P729), ("rect", W.RECT), ("noproj", W.NOPROJ), ("mean", dict(W.MICRO, pool="mean"))]


@pytest.mark.parametrize("tag,cfg", VIT_CASES, ids=[c[0] for c in VIT_CASES])
def test_fp32_maps_and_rollout_against_the_reference(golden, tag, cfg):
    g = golden("attention.npz")
    sw, sx = (int(v) for v in g[f"{tag}.seeds"])
    m = eval_model(cfg, sw)
    video = W.make_volume(tuple(int(v) for v in g[f"{tag}.shape"]), sx).cuda()
    with torch.no_grad(), m.precision("fp32"):
        _, maps = m.attention_maps(video)
        _, roll = m.attention_rollout(video)
    err = max(maxabs(maps[l], torch.from_numpy(g[f"{tag}.P{l}"])) for l in range(cfg["depth"]))
    ref = torch.from_numpy(g[f"{tag}.rollout"])
    rerr = maxabs(roll, ref) / ref.abs().max().item()
    report(f"attention fixture {tag}: max|dP| {err:.2e}, rollout rel {rerr:.2e}")
    assert err <= 1e-5 and rerr <= 1e-5


def test_neuro3d_fp32_maps_and_rollout_against_the_reference(golden):
    from neurovit_amd.NeuroEncoder import NeuroEncoder
    g = golden("attention.npz")
    sw, sx = (int(v) for v in g["neuro3d.seeds"])
    B, S = int(g["neuro3d.shape"][0]), int(g["neuro3d.shape"][1])
    model = NeuroEncoder(W.neuro_config(S, 8, DEVICE="cuda:0"))
    vc = dict(image_size=S, image_patch_size=8, frames=S, frame_patch_size=8, num_classes=2, dim=1024, depth=6, heads=8, mlp_dim=2048,
              channels=1, dim_head=64)
    model.load_state_dict(W.make_tensors(W.vit_param_spec(**vc), sw, prefix="volume_encoder.vit3d."), strict=True)
    model.eval()
    x = W.make_volume((B, S, S, S), sx).cuda()
    vit = model.volume_encoder.vit3d
    with torch.no_grad(), vit.precision("fp32"):
        _, maps = vit.attention_maps(x.permute(0, 3, 1, 2).unsqueeze(1))
        _, roll = vit.attention_rollout(x.permute(0, 3, 1, 2).unsqueeze(1))
    err = max(maxabs(maps[l], torch.from_numpy(g[f"neuro3d.P{l}"])) for l in range(6))
    ref = torch.from_numpy(g["neuro3d.rollout"])
    assert err <= 1e-5 and maxabs(roll, ref) / ref.abs().max().item() <= 1e-5


# ---------------------------------------------------------------------------------------------------------------- 16-bit operands

# bf16 on every geometry; fp16 operands (the second instantiation of the kernel) on the two small ones
THREE_WAY = [("micro", W.MICRO, 2, "bf16"), ("tiny", W.TINY, 2, "bf16"), ("base", W.BASE, 1, "bf16"), ("refgeo", REFGEO, 1, "bf16"),
             ("micro", W.MICRO, 2, "fp16"), ("tiny", W.TINY, 2, "fp16")]


@pytest.mark.parametrize("tag,cfg,B,fmt", THREE_WAY, ids=[f"{c[0]}-{c[3]}" for c in THREE_WAY])
def test_16bit_maps_three_way(tag, cfg, B, fmt):
    m = eval_model(cfg, 21)
    m.set_operands(fmt)
    sd = {k: v.detach().cpu() for k, v in m.state_dict().items()}
    video = make_input(cfg, B, 22)
    with torch.no_grad():
        _, maps = m.attention_maps(video.cuda())
    f32 = oracle_probs(cfg, sd, video, emulate=False)
    with ref_cpu.operand_format(fmt):
        emu = oracle_probs(cfg, sd, video, emulate=True)
    for l in range(cfg["depth"]):
        e_h, e_e = maxabs(maps[l], f32[l]), maxabs(emu[l], f32[l])
        report(f"attention three-way {tag} {fmt} layer {l}: hip-fp32 {e_h:.2e}, emul-fp32 {e_e:.2e}")
        assert e_h <= max(1.5 * e_e, 1e-4), (l, e_h, e_e)
        assert maxabs(maps[l].sum(-1), torch.ones(maps[l].shape[:-1])) <= 1e-5


@pytest.mark.parametrize("cfg", [dict(W.MICRO, dim_head=40, heads=3), dict(W.MICRO, dim_head=96, heads=2), W.NOPROJ],
                         ids=["dh40", "dh96", "noproj"])
def test_other_head_dims_and_noproj_three_way(cfg):
    m = eval_model(cfg, 31)
    sd = {k: v.detach().cpu() for k, v in m.state_dict().items()}
    video = make_input(cfg, 2, 32)
    with torch.no_grad():
        _, maps = m.attention_maps(video.cuda())
        with m.precision("fp32"):
            _, maps32 = m.attention_maps(video.cuda())
    f32 = oracle_probs(cfg, sd, video, emulate=False)
    emu = oracle_probs(cfg, sd, video, emulate=True)
    for l in range(cfg["depth"]):
        assert maxabs(maps[l], f32[l]) <= max(1.5 * maxabs(emu[l], f32[l]), 1e-4)
        assert maxabs(maps32[l], f32[l]) <= 1e-5


# ---------------------------------------------------------------------------------------------------------------- forms

@pytest.mark.parametrize("precision", ["bf16", "fp32"])
@pytest.mark.parametrize("cfg", [W.MICRO, REFGEO], ids=["micro", "refgeo"])
def test_head_fusion_and_cls_rows(cfg, precision):
    m = eval_model(cfg, 41)
    x = make_input(cfg, 2, 42).cuda()
    with torch.no_grad(), m.precision(precision):
        _, per = m.attention_maps(x)
        fused = {f: m.attention_maps(x, head_fusion=f)[1] for f in ("mean", "max", "min")}
        _, cls = m.attention_maps(x, rows="cls")
        _, cls_mean = m.attention_maps(x, head_fusion="mean", rows="cls")
    for l in range(cfg["depth"]):
        assert torch.equal(fused["max"][l], per[l].amax(dim=1))
        assert torch.equal(fused["min"][l], per[l].amin(dim=1))
        assert maxabs(fused["mean"][l], per[l].mean(dim=1)) <= 2e-7
        assert torch.equal(cls[l], per[l][:, :, :1])
        assert torch.equal(cls_mean[l], fused["mean"][l][:, :1])


def test_rollout_equals_a_restatement_of_the_exported_maps():
    for cfg in (W.MICRO, dict(W.MICRO, pool="mean")):
        m = eval_model(cfg, 43)
        x = make_input(cfg, 2, 44).cuda()
        with torch.no_grad():
            for fusion in ("mean", "max", "min"):
                _, maps = m.attention_maps(x, head_fusion=fusion)
                _, roll = m.attention_rollout(x, head_fusion=fusion)
                n = maps[0].shape[-1]
                u = torch.full((2, n), 1.0 / n, dtype=torch.float64) if cfg["pool"] == "mean" else torch.eye(n, dtype=torch.float64)[0].repeat(2, 1)
                for l in reversed(range(cfg["depth"])):
                    A = maps[l].double().cpu()
                    u = torch.einsum("bi,bij->bj", u, (A + torch.eye(n, dtype=torch.float64)) / (A.sum(-1, keepdim=True) + 1))
                assert maxabs(roll, u[:, 1:]) / u[:, 1:].abs().max().item() <= 1e-5


# ---------------------------------------------------------------------------------------------------------------- bit-identity

def _logits_with_and_without(m, x, **kw):
    with torch.no_grad():
        a = m(x, **kw).clone()
        b, maps = m.attention_maps(x, **kw)
        c, _ = m.attention_maps(x, head_fusion="mean", rows="cls", **kw)
    return a, b, c


@pytest.mark.parametrize("form", ["plain", "lnfold", "fp32"])
def test_export_leaves_inference_logits_bit_identical(form):
    m = make_model(W.TINY, 51).eval()
    m.fold_layernorm = form == "lnfold"
    x = make_input(W.TINY, 2, 52).cuda()
    if form == "fp32":
        with m.precision("fp32"):
            a, b, c = _logits_with_and_without(m, x)
    else:
        a, b, c = _logits_with_and_without(m, x)
    assert torch.equal(a, b) and torch.equal(a, c)


def test_export_leaves_fused_4d_logits_bit_identical():
    m = eval_model(W.MICRO, 53)
    series = W.make_volume((2, 32, 32, 32, 4), 54).cuda().contiguous()
    a, b, _ = _logits_with_and_without(m, series, time_points=4)
    assert torch.equal(a, b)
    with torch.no_grad(), m.precision("fp32"):      # the B*T volumes the encoder sees, as the regroup path's (fp32: the two gathers agree to 1e-5)
        a32, b32, _ = _logits_with_and_without(m, series, time_points=4)
        _, maps4 = m.attention_maps(series, time_points=4, layers=[1])
        _, maps = m.attention_maps(series.movedim(-1, 1).flatten(0, 1).permute(0, 3, 1, 2).unsqueeze(1), layers=[1])
    assert torch.equal(a32, b32)
    assert maps4[1].shape[0] == 8 and maxabs(maps4[1], maps[1]) <= 1e-5


def test_train_mode_with_dropout_logits_and_gradients_bit_identical_and_hook_is_predropout():
    cfg = W.MICRO
    drop = (0.1, 0.1, 424242)
    x = make_input(cfg, 2, 56)
    runs = []
    for hooked in (False, True):
        m = make_model(cfg, 55, dropout=0.1)
        m.draw_dropout = lambda: drop
        seen = {}
        if hooked:
            for l, (attn, _) in enumerate(m.transformer.layers):
                attn.attend.register_forward_hook(lambda mod, a, out, l=l: seen.__setitem__(l, out.clone()))
        logits = m(x.cuda())
        logits[:, 0].sum().backward()
        runs.append((logits.detach().clone(), m.flat_gradients().clone(), seen))
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])
    sd = {k: v.detach().cpu() for k, v in make_model(cfg, 55).state_dict().items()}
    f32 = oracle_probs(cfg, sd, x, emulate=False, dropout=drop)
    emu = oracle_probs(cfg, sd, x, emulate=True, dropout=drop)
    seen = runs[1][2]
    assert sorted(seen) == list(range(cfg["depth"]))
    for l in range(cfg["depth"]):
        assert maxabs(seen[l], f32[l]) <= max(1.5 * maxabs(emu[l], f32[l]), 1e-4)
        assert maxabs(seen[l].sum(-1), torch.ones(seen[l].shape[:-1])) <= 1e-5        # pre-dropout: rows sum to 1


def test_lnfold_maps_gate():
    """The LN-folded forward computes the same softmax from a qkv whose LayerNorm is applied in the GEMM epilogue (rstd (x Wg^T) - rstd mu
    colsum(Wg) + folded bias): a different rounding of the same 16-bit arithmetic, so its distance to the fp32 maps is that of the plain path
    up to rounding noise - gated at 2x the plain path's measured distance (floor 1e-4)."""
    m = make_model(W.TINY, 57).eval()
    x = make_input(W.TINY, 2, 58).cuda()
    with torch.no_grad():
        m.fold_layernorm = False
        _, plain = m.attention_maps(x)
        m.fold_layernorm = True
        _, folded = m.attention_maps(x)
        with m.precision("fp32"):
            _, exact = m.attention_maps(x)
    for l in range(W.TINY["depth"]):
        d_plain, d_fold = maxabs(plain[l], exact[l]), maxabs(folded[l], exact[l])
        report(f"attention lnfold layer {l}: plain {d_plain:.2e}, folded {d_fold:.2e}")
        assert d_fold <= max(2 * d_plain, 1e-4)


# ---------------------------------------------------------------------------------------------------------------- NeuroEncoder, fp8

def test_neuro_get_attention_rollout_reference_geometry():
    from neurovit_amd.NeuroEncoder import NeuroEncoder
    cfg = W.neuro_config(90, 9, DEVICE="cuda:0", TRAINING_VIT_DIM=256, TRAINING_VIT_DEPTH=2, TRAINING_VIT_HEADS=4, TRAINING_VIT_MLP_DIM=512)
    torch.manual_seed(61)
    model = NeuroEncoder(cfg).eval()
    x = W.make_volume((1, 90, 90, 90), 62).cuda()
    cam, cls = model.get_attention_rollout(x)
    assert cam.shape == (90, 90, 90) and cam.device.type == "cpu" and torch.isfinite(cam).all()
    assert cam.min() >= 0 and cam.max() <= 1 and cls.shape == (1,)
    vit = model.volume_encoder.vit3d
    with torch.no_grad():
        logits, roll = vit.attention_rollout(x.permute(0, 3, 1, 2).unsqueeze(1))
    t = roll.cpu()
    t = (t - t.min()) / (t.max() - t.min() + 1e-8)
    assert torch.equal(cam, model._token_map_to_volume(t)) and torch.equal(cls, logits.argmax(dim=1))
    assert model.visualize_slice(cam, x.cpu()) is not None


def test_fp8_paths_raise():
    m = make_model(W.MICRO, 63).eval()
    x = make_input(W.MICRO, 2, 64).cuda()
    m.enable_fp8(x)
    with torch.no_grad(), pytest.raises(NotImplementedError):
        m.attention_maps(x)
    with torch.no_grad(), pytest.raises(NotImplementedError):
        m.attention_rollout(x)
    h = m.transformer.layers[0][0].attend.register_forward_hook(lambda *a: None)
    with torch.no_grad(), pytest.raises(NotImplementedError):
        m(x)
    h.remove()
    m.train()
    m.enable_fp8(x, training=True)
    with pytest.raises(NotImplementedError):
        m.attention_maps(x)
