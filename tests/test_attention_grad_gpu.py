"""Gradient w.r.t. the attention probabilities and class-specific attention relevance through the native ViT3D on MI355X (nv_attn_grad,
nv_attn_relevance, nv_vit_backward_attn; backward hooks on every block's `attend`, ViT.attention_gradients / attention_relevance,
NeuroEncoder.get_attention_relevance).

Gates (the constants of tests/test_engine_gpu.py; nothing restated):
  hooks        a full backward hook on each `attend` fires once per backward, in reverse layer order, as hook(attend, (None,), (dP,))
               with dP fp32 [B, heads, n, n] on the device (the parent commit accepted the hook and never called it);
  kernel       nv_attn_grad per head against the float64 product of the same 16-bit operands: |err| <= 2 dim_head 2^-24 (|dO| |V|^T)
               elementwise - both operands are exact, only the fp32 accumulation differs, and a sum of dim_head products of fp32 roundings
               is off by at most (dim_head - 1 + 1) ulp-halves of the running magnitude, i.e. dim_head 2^-24 sum |terms|; 2x headroom for
               the MFMA's internal order;  zero rows of dO give exact zero rows;
  three-way    dP_l: err(HIP, fp32 oracle) <= RATIO err(emulating oracle, fp32) + SLACK and err(HIP, emulating oracle) <= GRAD_REL
               (relative L2 per layer; fp16 operands: FP16_GRAD_REL);
  fixture      dP_l and the relevance against the imported reference's (tests/golden/attention_grad.npz): relative L2 <= GRAD_REL;
  forms        relevance form == mean_h relu(dP * P) of the per-head export and attention_maps' P within 2 (heads + 1) 2^-24 max|A|
               (heads additions, one product, one division, each <= 2^-24 relative - holds only because the kernel's P has the bits of
               the export); attention_relevance against a float64 restatement of the exported A_l: <= 1e-5 max-norm relative;
  bit-identity logits, parameter gradients, x.grad and the Grad-CAM hook gradient do not move when backward hooks are registered.
Measured errors go to the parity report of test_engine_gpu.report.
"""
import pytest
import torch

import weights as W
from conftest import rel_l2
from test_attention_grad_cpu import oracle_attention_grads
from test_engine_gpu import GRAD_REL, RATIO, SLACK, report
from test_input_grad_gpu import FP16_GRAD_REL, make_input, make_model

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


def eval_model(cfgdict, seed):
    return make_model(cfgdict, seed).eval()


# ---------------------------------------------------------------------------------------------------------------- 1. hooks

def test_backward_hooks_fire_once_per_backward_in_reverse_layer_order():
    cfg = dict(W.MICRO, depth=3)
    m = make_model(cfg, 3)                       # train mode, no dropout
    calls = []

    def hook(module, grad_input, grad_output):
        calls.append((module, grad_input, grad_output))
    for attn, _ in m.transformer.layers:
        attn.attend.register_full_backward_hook(hook)
    x = make_input(cfg, 2, 4).cuda()
    m(x)[:, 0].sum().backward()
    n = m.pos_embedding.shape[1]
    assert [c[0] for c in calls] == [attn.attend for attn, _ in reversed(list(m.transformer.layers))]
    for _, gin, gout in calls:
        assert gin == (None,) and isinstance(gout, tuple) and len(gout) == 1
        assert gout[0].shape == (2, cfg["heads"], n, n) and gout[0].dtype == torch.float32 and gout[0].device.type == "cuda"
        assert torch.isfinite(gout[0]).all() and gout[0].abs().sum().item() > 0
    m(x)[:, 0].sum().backward()
    assert len(calls) == 6
    with torch.no_grad():                        # no backward, no call
        m(x)
    assert len(calls) == 6


def test_hook_on_some_layers_removal_legacy_hook_and_equality_with_attention_gradients():
    m = eval_model(W.MICRO, 5)                   # eval mode, parameters trainable: a graph is recorded
    seen = []
    h = m.transformer.layers[1][0].attend.register_full_backward_hook(lambda mod, gi, go: seen.append((1, go[0].clone())))
    h0 = m.transformer.layers[0][0].attend.register_backward_hook(lambda mod, gi, go: seen.append((0, go[0].clone())))     # legacy form
    x = make_input(W.MICRO, 2, 6).cuda()
    m(x)[:, 1].sum().backward()
    assert [l for l, _ in seen] == [1, 0]
    _, maps = m.attention_gradients(x, target=1)
    assert torch.equal(seen[0][1], maps[1]) and torch.equal(seen[1][1], maps[0])       # bit for bit
    h0.remove()
    m(x)[:, 1].sum().backward()
    assert [l for l, _ in seen] == [1, 0, 1]
    h.remove()
    m(x)[:, 1].sum().backward()
    assert len(seen) == 3


def test_hook_returning_a_value_and_pre_hooks_raise():
    m = make_model(W.MICRO, 7)
    x = make_input(W.MICRO, 1, 8).cuda()
    h = m.transformer.layers[0][0].attend.register_full_backward_hook(lambda mod, gi, go: (go[0] * 2,))
    with pytest.raises(RuntimeError, match="returned a value"):
        m(x).sum().backward()
    h.remove()
    h = m.transformer.layers[0][0].attend.register_full_backward_pre_hook(lambda mod, go: None)
    with pytest.raises(NotImplementedError):
        m(x)
    h.remove()
    m(x).sum().backward()                        # and the model is usable again


def test_standalone_attention_module_fires_its_backward_hook():
    from neurovit_amd.vit_3d import Attention
    torch.manual_seed(0)
    a = Attention(128, heads=2, dim_head=64).cuda()
    got = []
    a.attend.register_full_backward_hook(lambda mod, gi, go: got.append((gi, go[0])))
    x = torch.randn(2, 37, 128, device="cuda")
    w = torch.randn(2, 37, 128, device="cuda")
    (a(x) * w).sum().backward()
    assert len(got) == 1 and got[0][0] == (None,) and got[0][1].shape == (2, 2, 37, 37)
    # float64 restatement with the module's cast points: dAO = bf16(bf16(dy) Wo16), V = the v third of the bf16 qkv
    xn = torch.nn.functional.layer_norm(x.double(), (128,), a.norm.weight.double(), a.norm.bias.double(), 1e-5)
    qkv = (xn.bfloat16().double() @ a.to_qkv.weight.bfloat16().double().t()).bfloat16().double()
    v = qkv.chunk(3, dim=-1)[2].reshape(2, 37, 2, 64).permute(0, 2, 1, 3)
    dao = (w.bfloat16().double() @ a.to_out[0].weight.bfloat16().double()).bfloat16().double().reshape(2, 37, 2, 64).permute(0, 2, 1, 3)
    ref = dao @ v.transpose(-1, -2)
    assert rel_l2(got[0][1], ref) <= GRAD_REL


# ---------------------------------------------------------------------------------------------------------------- 2. the kernel alone

@pytest.mark.parametrize("fmt", ["bf16", "fp16"])
@pytest.mark.parametrize("dh", [40, 64, 96])
@pytest.mark.parametrize("n", [28, 65, 132, 513, 1001])          # 132: several 64-key chunks on the float4 store path
def test_attn_grad_kernel_against_float64_product(n, dh, fmt):
    from neurovit_amd import _cabi, ops
    B, heads = 2, 2
    inner = heads * dh
    g = torch.Generator().manual_seed(1000 * n + dh)
    dt = torch.float16 if fmt == "fp16" else torch.bfloat16
    qkv = torch.randn(B * n, 3 * inner, generator=g).to(dt).cuda()
    dout = (0.05 * torch.randn(B * n, inner, generator=g)).to(dt).cuda()
    try:
        _cabi.set_operand_format(fmt)
        out = ops.attn_grad(qkv, dout, B, n, heads, dh)
        torch.cuda.synchronize()
    finally:
        _cabi.set_operand_format("bf16")
    dO = dout.double().reshape(B, n, heads, dh).permute(0, 2, 1, 3)
    V = qkv.double()[:, 2 * inner:].reshape(B, n, heads, dh).permute(0, 2, 1, 3)
    want = dO @ V.transpose(-1, -2)
    bound = 2.0 * dh * 2.0 ** -24 * (dO.abs() @ V.abs().transpose(-1, -2))
    err = (out.double() - want).abs()
    worst = (err / bound.clamp_min(1e-300)).max().item()
    report(f"nv_attn_grad per head n={n} dh={dh} {fmt}: max err / bound {worst:.3f}, max|err| {err.max().item():.3e}")
    assert out.shape == (B, heads, n, n) and torch.isfinite(out).all()
    assert (err <= bound).all(), worst


@pytest.mark.parametrize("form", ["per_head", "relevance"])
def test_zero_rows_of_dout_give_exact_zero_rows(form):
    from neurovit_amd import ops
    B, n, heads, dh = 2, 65, 2, 64
    g = torch.Generator().manual_seed(9)
    qkv = torch.randn(B * n, 3 * heads * dh, generator=g).bfloat16().cuda()
    dout = torch.zeros(B, n, heads * dh)
    dout[:, 0] = torch.randn(B, heads * dh, generator=g)            # only the cls rows carry a gradient (last block, pool='cls')
    out = ops.attn_grad(qkv, dout.reshape(B * n, -1).bfloat16().cuda(), B, n, heads, dh, form=form)
    rows = out if form == "relevance" else out.transpose(1, 2)      # [B, n, ...]
    assert (rows[:, 1:] == 0).all() and rows[:, 0].abs().sum().item() > 0


# ---------------------------------------------------------------------------------------------------------------- 3. whole model, three-way

THREE_WAY = [("micro", W.MICRO, 2, "bf16"), ("tiny", W.TINY, 2, "bf16"), ("p729", P729, 2, "bf16"), ("base", W.BASE, 1, "bf16"),
             ("refgeo", REFGEO, 1, "bf16"), ("micro", W.MICRO, 2, "fp16"), ("tiny", W.TINY, 2, "fp16")]


@pytest.mark.parametrize("tag,cfg,B,fmt", THREE_WAY, ids=[f"{c[0]}-{c[3]}" for c in THREE_WAY])
def test_attention_gradients_three_way(tag, cfg, B, fmt):
    from oracle import ref_cpu
    m = eval_model(cfg, 21).requires_grad_(False)
    m.set_operands(fmt)
    sd = {k: v.detach().cpu() for k, v in m.state_dict().items()}
    video = make_input(cfg, B, 22)
    target = torch.zeros(B, dtype=torch.long)
    try:
        with torch.no_grad():
            _, maps = m.attention_gradients(video.cuda(), target=0)
        maps = {l: t.cpu() for l, t in maps.items()}
    finally:
        from neurovit_amd import _cabi
        _cabi.set_operand_format("bf16")
    _, _, f32 = oracle_attention_grads(cfg, sd, video, target)
    with ref_cpu.operand_format(fmt):
        _, _, emu = oracle_attention_grads(cfg, sd, video, target, emulate=True)
    limit = FP16_GRAD_REL if fmt == "fp16" else GRAD_REL
    fails = []
    for l in range(cfg["depth"]):
        e_he, e_h32, e_e32 = rel_l2(maps[l], emu[l]), rel_l2(maps[l], f32[l]), rel_l2(emu[l], f32[l])
        report(f"attention-grad three-way {tag} {fmt} layer {l}: hip-emu {e_he:.3e}  hip-fp32 {e_h32:.3e}  emu-fp32 {e_e32:.3e}")
        print(f"{tag} {fmt} layer {l}: hip-emu {e_he:.3e}  hip-fp32 {e_h32:.3e}  emu-fp32 {e_e32:.3e}")
        if not (e_h32 <= RATIO * e_e32 + SLACK and e_he <= limit):
            fails.append((l, e_he, e_h32, e_e32))
    assert not fails, fails


# ---------------------------------------------------------------------------------------------------------------- 4. reference fixture

VIT_CASES = [("micro", W.MICRO), ("p729", P729), ("rect", W.RECT), ("noproj", W.NOPROJ), ("mean", dict(W.MICRO, pool="mean"))]


def _fixture_gate(tag, depth, g, maps, rel):
    for l in range(depth):
        err = rel_l2(maps[l], g[f"{tag}.dP{l}"])
        report(f"attention-grad {tag} layer {l} vs reference fixture: rel L2 {err:.3e}")
        print(f"{tag} layer {l} vs reference fixture: rel L2 {err:.3e}")
        assert err <= GRAD_REL, (tag, l, err)
    err = rel_l2(rel, g[f"{tag}.relevance"])
    report(f"attention relevance {tag} vs reference fixture: rel L2 {err:.3e}")
    print(f"{tag} relevance vs reference fixture: rel L2 {err:.3e}")
    assert err <= GRAD_REL, (tag, err)


@pytest.mark.parametrize("tag,cfg", VIT_CASES, ids=[c[0] for c in VIT_CASES])
def test_attention_gradients_and_relevance_against_the_reference(golden, tag, cfg):
    g = golden("attention_grad.npz")
    sw, sx = (int(v) for v in g[f"{tag}.seeds"])
    m = eval_model(cfg, sw)
    video = W.make_volume(tuple(int(v) for v in g[f"{tag}.shape"]), sx).cuda()
    target = torch.from_numpy(g[f"{tag}.target"]).cuda()           # the class the reference explained (its arg-max)
    with torch.no_grad():
        logits, maps = m.attention_gradients(video, target=target)
        _, rel = m.attention_relevance(video, target=target)
    assert rel.shape == (video.shape[0], m.pos_embedding.shape[1] - 1)
    _fixture_gate(tag, cfg["depth"], g, maps, rel)


def test_neuro3d_attention_gradients_and_relevance_against_the_reference(golden):
    from neurovit_amd.NeuroEncoder import NeuroEncoder
    g = golden("attention_grad.npz")
    sw, sx = (int(v) for v in g["neuro3d.seeds"])
    B, S = int(g["neuro3d.shape"][0]), int(g["neuro3d.shape"][1])
    model = NeuroEncoder(W.neuro_config(S, 8, DEVICE="cuda:0"))
    vc = dict(image_size=S, image_patch_size=8, frames=S, frame_patch_size=8, num_classes=2, dim=1024, depth=6, heads=8, mlp_dim=2048,
              channels=1, dim_head=64)
    model.load_state_dict(W.make_tensors(W.vit_param_spec(**vc), sw, prefix="volume_encoder.vit3d."), strict=True)
    model.eval()
    x = W.make_volume((B, S, S, S), sx).cuda()
    vit = model.volume_encoder.vit3d
    target = torch.from_numpy(g["neuro3d.target"]).cuda()
    video = x.permute(0, 3, 1, 2).unsqueeze(1)
    with torch.no_grad():
        _, maps = vit.attention_gradients(video, target=target)
        _, rel = vit.attention_relevance(video, target=target)
    _fixture_gate("neuro3d", 6, g, maps, rel)


# ---------------------------------------------------------------------------------------------------------------- 5. forms

@pytest.mark.parametrize("cfg", [W.MICRO, dict(W.MICRO, pool="mean"), W.TINY, REFGEO], ids=["micro", "mean", "tiny", "refgeo"])
def test_relevance_form_equals_the_per_head_export_times_the_exported_probabilities(cfg):
    m = eval_model(cfg, 41)
    m.fold_layernorm = False                     # attention_maps in the arithmetic of the graph-recording forward (same qkv bits)
    B = 1 if cfg is REFGEO else 2
    x = make_input(cfg, B, 42).cuda()
    with torch.no_grad():
        _, per = m.attention_gradients(x, target=1)
        _, rel = m.attention_gradients(x, target=1, form="relevance")
        _, P = m.attention_maps(x)
    heads = cfg["heads"]
    for l in range(cfg["depth"]):
        want = torch.relu(per[l] * P[l]).mean(dim=1)                # torch, fp32
        tol = 2 * (heads + 1) * 2.0 ** -24 * rel[l].abs().max().item()
        err = maxabs(rel[l], want)
        report(f"relevance form vs per-head x P, layer {l}: max|d| {err:.3e} (tol {tol:.3e})")
        assert err <= tol, (l, err, tol)
        assert (rel[l] >= 0).all()


@pytest.mark.parametrize("pool", ["cls", "mean"])
def test_attention_relevance_equals_a_float64_restatement_of_the_exported_terms(pool):
    cfg = dict(W.TINY, pool=pool)
    m = eval_model(cfg, 43)
    x = make_input(cfg, 2, 44).cuda()
    with torch.no_grad():
        logits, A = m.attention_gradients(x, form="relevance")
        logits2, rel = m.attention_relevance(x)
    assert torch.equal(logits, logits2)
    n = A[0].shape[-1]
    u = torch.full((2, n), 1.0 / n, dtype=torch.float64) if pool == "mean" else torch.eye(n, dtype=torch.float64)[0].repeat(2, 1)
    for l in reversed(range(cfg["depth"])):
        u = u + torch.einsum("bi,bij->bj", u, A[l].double().cpu())
    err = maxabs(rel, u[:, 1:]) / u[:, 1:].abs().max().item()
    report(f"attention_relevance pool={pool} vs float64 restatement: max-norm rel {err:.3e}")
    assert err <= 1e-5, err
    assert (rel >= 0).all() and rel.shape == (2, n - 1)


def test_target_forms_and_layer_subsets():
    m = eval_model(W.TINY, 45)
    x = make_input(W.TINY, 2, 46).cuda()
    with torch.no_grad():
        logits, all_maps = m.attention_gradients(x)
        _, by_tensor = m.attention_gradients(x, target=logits.argmax(dim=1))
        _, some = m.attention_gradients(x, layers=[2, 3])                 # the backward stops at layer 2
        _, other = m.attention_gradients(x, target=(1 - logits.argmax(dim=1)))
    assert sorted(some) == [2, 3]
    for l in range(W.TINY["depth"]):
        assert torch.equal(all_maps[l], by_tensor[l])
    assert torch.equal(some[2], all_maps[2]) and torch.equal(some[3], all_maps[3])
    assert not torch.equal(other[0], all_maps[0])
    with pytest.raises(ValueError):
        m.attention_gradients(x, form="mean")
    with pytest.raises(ValueError):
        m.attention_gradients(x, layers=[7])


# ---------------------------------------------------------------------------------------------------------------- 6. nothing else moves

def test_hooks_leave_logits_gradients_input_gradient_and_gradcam_hook_bit_identical():
    cfg = W.MICRO
    xin = make_input(cfg, 2, 52).contiguous()
    runs = []
    for hooked in (False, True):
        m = make_model(cfg, 51)
        seen = {}
        if hooked:
            for l, (attn, _) in enumerate(m.transformer.layers):
                attn.attend.register_full_backward_hook(lambda mod, gi, go, l=l: seen.__setitem__(l, go[0].clone()))
        x = xin.cuda().requires_grad_(True)
        logits = m(x)
        logits[:, 1].sum().backward()
        torch.cuda.synchronize()
        runs.append((logits.detach().clone(), m.flat_gradients().clone(), x.grad.clone(), m.last_attn_norm_grad(), seen))
    for a, b in zip(runs[0][:4], runs[1][:4]):
        assert torch.equal(a, b)
    assert sorted(runs[1][4]) == [0, 1]

    # the frozen model's data-only backward gives the same dP, and attention_gradients touches no p.grad
    f = make_model(cfg, 51).requires_grad_(False)
    with torch.no_grad():
        lg, maps = f.attention_gradients(xin.cuda(), target=1)
    assert torch.equal(lg, runs[0][0])
    for l in (0, 1):
        assert torch.equal(maps[l], runs[1][4][l])
    assert all(p.grad is None for p in f.parameters()) and f._grads is None
    assert torch.equal(f.last_attn_norm_grad(), runs[0][3])          # the hook gradient, as a normal backward leaves it
    t = make_model(cfg, 51)                                          # trainable, with gradients already in place
    t(xin.cuda())[:, 0].sum().backward()
    before = t.flat_gradients().clone()
    t.attention_gradients(xin.cuda(), target=1)
    assert torch.equal(t.flat_gradients(), before) and all(p.grad is not None for p in t.parameters())


# ---------------------------------------------------------------------------------------------------------------- 7. NeuroEncoder

def test_neuro_get_attention_relevance_reference_geometry():
    from neurovit_amd.NeuroEncoder import NeuroEncoder
    cfg = W.neuro_config(90, 9, DEVICE="cuda:0", TRAINING_VIT_DIM=256, TRAINING_VIT_DEPTH=2, TRAINING_VIT_HEADS=4, TRAINING_VIT_MLP_DIM=512)
    torch.manual_seed(61)
    model = NeuroEncoder(cfg).eval()
    x = W.make_volume((1, 90, 90, 90), 62).cuda()
    cam, cls = model.get_attention_relevance(x)
    assert cam.shape == (90, 90, 90) and cam.device.type == "cpu" and torch.isfinite(cam).all()
    assert cam.min() >= 0 and cam.max() <= 1 and cls.shape == (1,)
    vit = model.volume_encoder.vit3d
    with torch.no_grad():
        logits, rel = vit.attention_relevance(x.permute(0, 3, 1, 2).unsqueeze(1))
    t = rel.cpu()
    t = (t - t.min()) / (t.max() - t.min() + 1e-8)
    assert torch.equal(cam, model._token_map_to_volume(t)) and torch.equal(cls, logits.argmax(dim=1))
    other = 1 - int(cls.item())
    cam2, cls2 = model.get_attention_relevance(x, target=other)
    assert int(cls2.item()) == other and not torch.equal(cam2, cam)
    assert all(p.grad is None for p in model.parameters())
    assert model.visualize_slice(cam, x.cpu()) is not None


# ---------------------------------------------------------------------------------------------------------------- 8. what is refused

def test_refusals():
    from neurovit_amd.NeuroEncoder import NeuroEncoder
    from neurovit_amd.trainer import TrainStep
    x = make_input(W.MICRO, 2, 64).cuda()
    # attention dropout active
    d = make_model(W.MICRO, 63, dropout=0.1)
    with pytest.raises(NotImplementedError, match="dropout"):
        d.attention_gradients(x)
    with pytest.raises(NotImplementedError, match="dropout"):
        d.attention_relevance(x)
    h = d.transformer.layers[0][0].attend.register_full_backward_hook(lambda *a: None)
    with pytest.raises(NotImplementedError, match="dropout"):
        d(x).sum().backward()
    d.eval()                                     # eval mode: no dropout, everything works
    d.attention_gradients(x)
    d(x).sum().backward()
    h.remove()
    # the fused 4D input form
    m = make_model(W.MICRO, 63).eval()
    series = W.make_volume((1, 32, 32, 32, 4), 65).cuda().contiguous()
    with pytest.raises(NotImplementedError, match="time_points"):
        m.attention_gradients(series, time_points=4)
    # the fp8 training forward
    m.train()
    m.enable_fp8(x, training=True)
    with pytest.raises(NotImplementedError, match="fp8"):
        m.attention_gradients(x)
    with pytest.raises(NotImplementedError, match="fp8"):
        m.attention_relevance(x)
    h = m.transformer.layers[1][0].attend.register_full_backward_hook(lambda *a: None)
    with pytest.raises(NotImplementedError, match="fp8"):
        m(x)
    h.remove()
    m.disable_fp8()
    # TrainStep's native one-call step
    size = dict(TRAINING_VIT_DIM=128, TRAINING_VIT_DEPTH=2, TRAINING_VIT_HEADS=2, TRAINING_VIT_MLP_DIM=256)
    model = NeuroEncoder(W.neuro_config(32, 8, DEVICE="cuda", TRAINING_LEARNING_RATE=1e-3, TRAINING_WEIGHT_DECAY=1e-2, **size))
    model.train()
    step = TrainStep(model)
    fmri, labels = W.make_volume((2, 32, 32, 32), 66).cuda(), torch.tensor([0, 1], device="cuda")
    fired = []
    h = model.volume_encoder.vit3d.transformer.layers[0][0].attend.register_full_backward_hook(lambda mod, gi, go: fired.append(go[0].shape))
    with pytest.raises(NotImplementedError, match="native"):
        step._native_step(fmri, labels)
    step(fmri, labels)                           # TrainStep itself routes the hooked model to the general path, whose backward fires the hook
    assert len(fired) == 1 and not step._native_ok(fmri, labels)
    h.remove()
