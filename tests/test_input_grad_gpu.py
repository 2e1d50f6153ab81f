"""Gradient w.r.t. the input volume through the native ViT3D on MI355X (nv_patch_ln_dx, nv_vit_backward_ex, _ViTFunction's `video` slot).

Gates (the constants of tests/test_engine_gpu.py for parameter gradients):
  kernel       nv_patch_ln_dx against float64 autograd of F.layer_norm(patchify(video)): max-norm relative <= 1e-5;
  three-way    x.grad: err(HIP, fp32 oracle) <= RATIO err(emulating oracle, fp32) + SLACK and err(HIP, emulating oracle) <= GRAD_REL
               (relative L2; fp16 operands: test_fp16_gpu.py's 1.5e-3);
  reference    x.grad against the imported reference's input gradients (tests/golden/input_grad.npz) at GRAD_REL;
  bit-identity the parameter-gradient arena does not change when the input also wants a gradient; the frozen model's data-only x.grad
               and Grad-CAM hook gradient equal the trainable model's, and it leaves every p.grad None.
Measured errors go to the parity report of test_engine_gpu.report.
"""
import pytest
import torch
import torch.nn.functional as F

import weights as W
from conftest import rel_err, rel_l2
from oracle import ref_cpu
from test_engine_gpu import GRAD_REL, RATIO, SLACK, report

pytestmark = pytest.mark.gpu
FP16_GRAD_REL = 1.5e-3            # test_fp16_gpu.py's gradient gate
P729 = dict(W.MICRO, image_size=27, image_patch_size=9, frames=27, frame_patch_size=9)


@pytest.fixture(scope="module", autouse=True)
def gpu():
    from neurovit_amd._cabi import require_gpu
    require_gpu()


def oracle_cfg(cfgdict):
    v = dict(cfgdict)
    (H, Wd), (p1, p2) = (x if isinstance(x, tuple) else (x, x) for x in (v.pop("image_size"), v.pop("image_patch_size")))
    return ref_cpu.ViTCfg(image_size=H, image_patch_size=p1, image_width=Wd, patch_width=p2, **v)


def video_shape(cfgdict, B):
    H, Wd = cfgdict["image_size"] if isinstance(cfgdict["image_size"], tuple) else (cfgdict["image_size"],) * 2
    return (B, cfgdict.get("channels", 3), cfgdict["frames"], H, Wd)


def make_model(cfgdict, seed, dropout=0.0):
    from neurovit_amd.vit_3d import ViT
    m = ViT(**cfgdict, dropout=dropout, emb_dropout=dropout)
    m.load_state_dict(W.make_tensors(W.vit_param_spec(**cfgdict), seed), strict=True)
    return m.cuda().train()


def make_input(cfgdict, B, seed):
    """[B, C, F, H, W]: for one channel the [B, H, W, D] -> [B, 1, D, H, W] permute view ViT3DEncoder feeds (the float4 gather), else contiguous"""
    shape = video_shape(cfgdict, B)
    if shape[1] == 1 and shape[2] == shape[3] == shape[4]:
        return ref_cpu.fmri_to_video(W.make_volume((B, shape[3], shape[4], shape[2]), seed))
    return W.make_volume(shape, seed)


def hip_input_grad(model, video_cpu, c=0, scale=1.0):
    x = video_cpu.cuda().requires_grad_(True) if video_cpu.is_contiguous() else _leaf_view(video_cpu)
    logits = model(x)
    (logits[:, c].sum() * scale).backward()
    return x, logits


def _leaf_view(video_cpu):
    """a leaf tensor with the permute view's strides (torch.empty_strided + copy): what a caller's x.requires_grad_() gives"""
    x = torch.empty_strided(video_cpu.shape, video_cpu.stride(), device="cuda")
    x.copy_(video_cpu)
    return x.requires_grad_(True)


def oracle_input_grad(cfgdict, sd, video_cpu, emulate, dropout=None, c=0, scale=1.0):
    v = video_cpu.clone().requires_grad_(True)
    logits = ref_cpu.vit_forward(sd, oracle_cfg(cfgdict), v, emulate_bf16=emulate, dropout=dropout)
    (g,) = torch.autograd.grad(logits[:, c].sum() * scale, v)
    return g / scale


def three_way(tag, hip, emu, f32, limit=GRAD_REL):
    e_he, e_h32, e_e32 = rel_l2(hip, emu), rel_l2(hip, f32), rel_l2(emu, f32)
    report(f"input-grad {tag}: hip-emu {e_he:.3e}  hip-fp32 {e_h32:.3e}  emu-fp32 {e_e32:.3e}")
    assert e_h32 <= RATIO * e_e32 + SLACK and e_he <= limit, (tag, e_he, e_h32, e_e32)


# ------------------------------------------------------------------ 1. the kernel
def _patch_ln_dx(video, p, gamma, dxp, dvideo):
    from neurovit_amd import ops
    from neurovit_amd._cabi import check, lib
    B, C, Fr, H, Wd = video.shape
    p1, p2, pf = p
    P = C * p1 * p2 * pf
    tok = ref_cpu.patchify(video.double().cpu(), p1, p2, pf)
    mean = tok.mean(-1)
    rstd = 1.0 / torch.sqrt(((tok - mean[..., None]) ** 2).mean(-1) + 1e-5)
    m32, r32 = mean.float().reshape(-1).cuda(), rstd.float().reshape(-1).cuda()
    check(lib.nv_patch_ln_dx(video.data_ptr(), ops.strides5(video), B, C, Fr, H, Wd, p1, p2, pf, dxp.data_ptr(), dxp.stride(0),
                             m32.data_ptr(), r32.data_ptr(), gamma.data_ptr(), dvideo.data_ptr(), ops.strides5(dvideo),
                             torch.cuda.current_stream().cuda_stream), "nv_patch_ln_dx")
    torch.cuda.synchronize()
    # float64 autograd of the LayerNorm over the gathered patches, with the statistics the kernel was given
    v = video.double().cpu().requires_grad_(True)
    y = F.layer_norm(ref_cpu.patchify(v, p1, p2, pf), (P,), gamma.double().cpu(), None, 1e-5)
    (want,) = torch.autograd.grad(y, v, dxp[:, :P].double().cpu().reshape(y.shape))
    return want


@pytest.mark.parametrize("case", ["vec", "scalar729", "channels3", "strided", "nan_prefill"])
def test_patch_ln_dx_kernel_against_float64_autograd(case):
    g = torch.Generator().manual_seed(5)
    if case in ("vec", "nan_prefill"):        # [B, H, W, D] permute view, 8^3 patches: float4 runs
        video = ref_cpu.fmri_to_video(torch.randn(2, 32, 32, 32, generator=g)).cuda()
        p = (8, 8, 8)
    elif case == "scalar729":                 # the reference's 9^3 patches
        video = ref_cpu.fmri_to_video(torch.randn(2, 27, 27, 27, generator=g)).cuda()
        p = (9, 9, 9)
    elif case == "channels3":
        video = torch.randn(2, 3, 8, 16, 24, generator=g).cuda()
        p = (8, 4, 4)
    else:                                     # a non-dense view: every other volume of a batch, two axes transposed
        base = torch.randn(4, 1, 16, 24, 16, generator=g).cuda()
        video = base[::2].transpose(2, 4)     # [2, 1, 16, 24, 16] -> F = 16, H = 24, W = 16 with strides off the float4 path
        p = (8, 4, 8)
    B, C, Fr, H, Wd = video.shape
    P = C * p[0] * p[1] * p[2]
    N = (Fr // p[2]) * (H // p[0]) * (Wd // p[1])
    ldd = (P + 7) // 8 * 8
    dxp = torch.full((B * N, ldd), float("nan"), device="cuda")         # padding columns NaN: never read
    dxp[:, :P] = torch.randn(B * N, P, generator=g).cuda()
    gamma = (1 + 0.1 * torch.randn(P, generator=g)).cuda()
    if case == "strided":
        dvideo = torch.empty(video.shape, device="cuda")                 # contiguous, unlike the input
    else:
        dvideo = torch.empty_like(video, memory_format=torch.preserve_format)
    if case == "nan_prefill":
        dvideo.fill_(float("nan"))
    want = _patch_ln_dx(video, p, gamma, dxp, dvideo)
    got = dvideo.cpu()
    assert torch.isfinite(got).all(), "nv_patch_ln_dx left elements unwritten"
    err = rel_err(got, want)
    report(f"nv_patch_ln_dx {case}: max-norm rel {err:.3e}")
    assert err <= 1e-5, err


# ------------------------------------------------------------------ 2. three-way, through the module
CASES = {
    "micro": (W.MICRO, 2), "tiny": (W.TINY, 2), "p729": (P729, 2), "rect": (W.RECT, 2), "noproj": (W.NOPROJ, 2),
    "pool_mean": (dict(W.MICRO, pool="mean"), 2),
}


@pytest.mark.parametrize("tag", sorted(CASES))
def test_input_grad_three_way(tag):
    cfgdict, B = CASES[tag]
    model = make_model(cfgdict, 41)
    sd = W.make_tensors(W.vit_param_spec(**cfgdict), 41)
    video = make_input(cfgdict, B, 42)
    x, _ = hip_input_grad(model, video)
    assert x.grad is not None and x.grad.shape == x.shape and x.grad.stride() == x.stride()
    three_way(tag, x.grad.cpu(), oracle_input_grad(cfgdict, sd, video, True), oracle_input_grad(cfgdict, sd, video, False))


def test_input_grad_three_way_dropout_same_masks():
    cfgdict = W.MICRO
    model = make_model(cfgdict, 43, dropout=0.1)
    sd = W.make_tensors(W.vit_param_spec(**cfgdict), 43)
    video = make_input(cfgdict, 2, 44)
    torch.manual_seed(7)
    seed = int(torch.randint(0, 2 ** 62, (1,)).item())                 # what ViT.draw_dropout draws next
    torch.manual_seed(7)
    x, _ = hip_input_grad(model, video)
    drop = (0.1, 0.1, seed)
    three_way("dropout0.1", x.grad.cpu(), oracle_input_grad(cfgdict, sd, video, True, drop), oracle_input_grad(cfgdict, sd, video, False, drop))


def test_input_grad_three_way_base_one_volume():
    cfgdict = W.BASE
    model = make_model(cfgdict, 45).requires_grad_(False)
    sd = W.make_tensors(W.vit_param_spec(**cfgdict), 45)
    video = make_input(cfgdict, 1, 46)
    x, _ = hip_input_grad(model, video)
    three_way("base", x.grad.cpu(), oracle_input_grad(cfgdict, sd, video, True), oracle_input_grad(cfgdict, sd, video, False))


def test_input_grad_three_way_fp16_operands():
    cfgdict = W.TINY
    model = make_model(cfgdict, 47).set_operands("fp16")
    sd = W.make_tensors(W.vit_param_spec(**cfgdict), 47)
    video = make_input(cfgdict, 2, 48)
    LS = 1024.0                                                        # a power-of-two loss scale, as fp16 training uses
    try:
        x, _ = hip_input_grad(model, video, scale=LS)
        with ref_cpu.operand_format("fp16"):
            emu = oracle_input_grad(cfgdict, sd, video, True, scale=LS)
    finally:
        from neurovit_amd import _cabi
        _cabi.set_operand_format("bf16")
    three_way("tiny-fp16", x.grad.cpu() / LS, emu, oracle_input_grad(cfgdict, sd, video, False), FP16_GRAD_REL)


# ------------------------------------------------------------------ 3. against the imported reference
@pytest.mark.parametrize("tag", ["micro", "p729", "rect"])
def test_input_grad_against_reference_fixture(golden, tag):
    g = golden("input_grad.npz")
    cfgdict = {"micro": W.MICRO, "p729": P729, "rect": W.RECT}[tag]
    seed_w, seed_x = (int(v) for v in g[f"{tag}.seeds"])
    model = make_model(cfgdict, seed_w).requires_grad_(False)
    video = W.make_volume(tuple(int(v) for v in g[f"{tag}.shape"]), seed_x)
    x, _ = hip_input_grad(model, video)
    err = rel_l2(x.grad, g[f"{tag}.grad"])
    report(f"input-grad {tag} vs reference fixture: rel L2 {err:.3e}")
    assert err <= GRAD_REL, err


def test_neuro3d_input_grad_against_reference_fixture(golden):
    from neurovit_amd.NeuroEncoder import NeuroEncoder
    g = golden("input_grad.npz")
    B, S = int(g["neuro3d.shape"][0]), int(g["neuro3d.shape"][1])
    seed_w, seed_x = (int(v) for v in g["neuro3d.seeds"])
    model = NeuroEncoder(W.neuro_config(S, 8, DEVICE="cuda:0"))
    vc = dict(image_size=S, image_patch_size=8, frames=S, frame_patch_size=8, num_classes=2, dim=1024, depth=6, heads=8,
              mlp_dim=2048, channels=1, dim_head=64)
    model.load_state_dict(W.make_tensors(W.vit_param_spec(**vc), seed_w, prefix="volume_encoder.vit3d."), strict=True)
    model.train()
    x = W.make_volume((B, S, S, S), seed_x).cuda().requires_grad_(True)
    model(x)[:, 0].sum().backward()
    err = rel_l2(x.grad, g["neuro3d.grad"])
    report(f"input-grad neuro3d vs reference fixture: rel L2 {err:.3e}")
    assert err <= GRAD_REL, err


# ------------------------------------------------------------------ 4. bit-identity
def test_parameter_arena_unchanged_by_input_grad_and_frozen_equals_trainable():
    from neurovit_amd.NeuroEncoder import NeuroEncoder
    S = 32
    size = dict(TRAINING_VIT_DIM=128, TRAINING_VIT_DEPTH=2, TRAINING_VIT_HEADS=2, TRAINING_VIT_MLP_DIM=256)
    sd = W.make_tensors(W.vit_param_spec(**W.MICRO), 49, prefix="volume_encoder.vit3d.")
    fmri = W.make_volume((2, S, S, S), 50).cuda()

    def run(input_grad, frozen):
        model = NeuroEncoder(W.neuro_config(S, 8, DEVICE="cuda:0", **size))
        model.load_state_dict(sd, strict=True)
        model.train()
        if frozen:
            model.requires_grad_(False)
        x = fmri.clone().requires_grad_(input_grad)
        model(x)[:, 1].sum().backward()
        torch.cuda.synchronize()
        vit = model.volume_encoder.vit3d
        arena = None if frozen else vit.flat_gradients().clone()
        pgrads = [p.grad for p in vit.parameters()]
        return arena, (x.grad.clone() if input_grad else None), model.gradients.clone(), pgrads, vit

    arena_plain, _, hook_plain, _, _ = run(False, False)
    arena_x, dx_train, hook_train, _, _ = run(True, False)
    _, dx_frozen, hook_frozen, pgrads_frozen, vit_frozen = run(True, True)
    assert torch.equal(arena_plain, arena_x)                     # every parameter gradient bit for bit
    assert torch.equal(hook_plain, hook_train)
    assert torch.equal(dx_train, dx_frozen)                      # the data-only backward: the same data chain
    assert torch.equal(hook_train, hook_frozen)                  # Grad-CAM hook gradient of the frozen run
    assert all(g is None for g in pgrads_frozen)
    assert vit_frozen._grads is None                             # no parameter-sized gradient arena was allocated
    assert dx_frozen.abs().sum().item() > 0 and torch.isfinite(dx_frozen).all()


# ------------------------------------------------------------------ 5. autograd.grad and integrated gradients
def test_autograd_grad_and_integrated_gradients():
    cfgdict = W.MICRO
    model = make_model(cfgdict, 51)                              # trainable: autograd.grad must work here too
    sd = W.make_tensors(W.vit_param_spec(**cfgdict), 51)
    video = make_input(cfgdict, 1, 52).contiguous()
    x = video.cuda().requires_grad_(True)
    (gx,) = torch.autograd.grad(model(x)[:, 1].sum(), x)        # raised "not used in the graph" before
    assert gx.shape == x.shape and torch.isfinite(gx).all()

    # integrated gradients as captum computes them: zero baseline, 16 alphas batched, Riemann mean of the gradients along the path
    steps, c = 16, 1
    model.requires_grad_(False)
    alphas = (torch.arange(steps, dtype=torch.float32) + 0.5) / steps

    def ig(f, inp):
        path = (alphas.view(-1, 1, 1, 1, 1).to(inp.device) * inp).requires_grad_(True)
        (g,) = torch.autograd.grad(f(path)[:, c].sum(), path)
        return inp[0] * g.mean(0)

    ocfg = oracle_cfg(cfgdict)
    attr_hip = ig(model, x.detach()).cpu()
    attr_emu = ig(lambda v: ref_cpu.vit_forward(sd, ocfg, v, emulate_bf16=True), video)
    attr_f32 = ig(lambda v: ref_cpu.vit_forward(sd, ocfg, v), video)
    three_way("integrated-gradients", attr_hip, attr_emu, attr_f32)
    # completeness: sum(attr) ~ f(x) - f(0); the HIP path's error within RATIO x the fp32 oracle's own (16-step Riemann) error + SLACK
    with torch.no_grad():
        f_hip = model(torch.cat([x.detach(), torch.zeros_like(x)]))[:, c].cpu()
        f_32 = ref_cpu.vit_forward(sd, ocfg, torch.cat([video, torch.zeros_like(video)]))[:, c]
    err_hip = abs(attr_hip.sum().item() - (f_hip[0] - f_hip[1]).item())
    err_32 = abs(attr_f32.sum().item() - (f_32[0] - f_32[1]).item())
    report(f"integrated gradients completeness: hip {err_hip:.3e}  fp32 oracle {err_32:.3e}")
    assert err_hip <= RATIO * err_32 + SLACK, (err_hip, err_32)


# ------------------------------------------------------------------ 6. 4D: dL / d(fMRI series)
def test_neuro4d_series_gradient_against_oracle_composition(tmp_path):
    from neurovit_amd.NeuroEncoder import NeuroEncoder
    S, T, B = 16, 3, 1      # T % 4 != 0 and B * T <= 4: both runs take the regroup path and the same encoder form (see run())
    m3 = NeuroEncoder(W.neuro_config(S, 8, dim=3, TRAINING_VIT_DIM=128, TRAINING_VIT_DEPTH=2, TRAINING_VIT_HEADS=2, TRAINING_VIT_MLP_DIM=256))
    vc = dict(image_size=S, image_patch_size=8, frames=S, frame_patch_size=8, num_classes=2, dim=128, depth=2, heads=2, mlp_dim=256,
              channels=1, dim_head=64)
    m3.load_state_dict(W.make_tensors(W.vit_param_spec(**vc), 53, prefix="volume_encoder.vit3d."), strict=True)
    torch.save(m3.state_dict(), tmp_path / "c.pth")
    cfg4 = W.neuro_config(S, 8, dim=4, DEVICE="cuda:0", GLOBAL_BASE_PATH=str(tmp_path), BEST_MODEL_PATH="c.pth",
                          TRAINING_VIT_DIM=128, TRAINING_VIT_DEPTH=2, TRAINING_VIT_HEADS=2, TRAINING_VIT_MLP_DIM=256)
    torch.manual_seed(3)
    model = NeuroEncoder(cfg4)
    model.temporal_transformer.eval()                            # no dropout in the temporal head: the oracle composition has no masks
    series = W.make_volume((B, S, S, S, T), 54)

    # the run without an input gradient takes the no-grad inference forward: with the LayerNorms unfolded it is the training forward's
    # arithmetic bit for bit (test_engine_gpu.py::test_inference_mode_matches_training_forward)
    model.volume_encoder.vit3d.fold_layernorm = False

    def run(input_grad):
        s = series.cuda().requires_grad_(input_grad)
        model.zero_grad(set_to_none=True)
        out = model(s)
        out[:, 0].sum().backward()
        torch.cuda.synchronize()
        head = [p.grad.clone() for p in list(model.temporal_transformer.parameters()) + list(model.projection_head.parameters())]
        return (s.grad.cpu() if input_grad else None), head

    _, head_plain = run(False)
    dseries, head_x = run(True)
    assert all(torch.equal(a, b) for a, b in zip(head_plain, head_x))
    assert all(p.grad is None for p in model.volume_encoder.parameters())

    sd = {k: v.detach().cpu() for k, v in model.state_dict().items()}

    def oracle(emulate):
        f = series.clone().requires_grad_(True)
        cfg = ref_cpu.neuro_cfg(cfg4)
        vols = f.permute(0, 4, 1, 2, 3).reshape(B * T, S, S, S)
        enc = ref_cpu.vit_forward(ref_cpu.strip_prefix(sd, "volume_encoder.vit3d."), cfg, ref_cpu.fmri_to_video(vols), emulate).reshape(B, T, -1)
        (g,) = torch.autograd.grad(ref_cpu.temporal_head(sd, enc)[:, 0].sum(), f)
        return g

    three_way("neuro4d", dseries, oracle(True), oracle(False))


# ------------------------------------------------------------------ 7. what is refused
def test_input_grad_refused_where_it_would_be_wrong_or_is_not_built():
    from neurovit_amd.NeuroEncoder import NeuroEncoder
    size = dict(TRAINING_VIT_DIM=128, TRAINING_VIT_DEPTH=2, TRAINING_VIT_HEADS=2, TRAINING_VIT_MLP_DIM=256)
    model = NeuroEncoder(W.neuro_config(32, 8, DEVICE="cuda:0", **size)).requires_grad_(False)
    raw = (100 + 30 * W.make_volume((1, 33, 51, 33), 55)).cuda().requires_grad_(True)      # the dataset's crop -> 32^3
    with pytest.raises(NotImplementedError, match="RAW"):
        model.forward_raw(raw)
    vit = model.volume_encoder.vit3d
    series = W.make_volume((1, 32, 32, 32, 4), 56).cuda().requires_grad_(True)
    with pytest.raises(NotImplementedError, match="time_points"):
        vit(series, time_points=4)
    cal = ref_cpu.fmri_to_video(W.make_volume((1, 32, 32, 32), 57)).cuda()
    vit.enable_fp8(cal, training=True)
    x = cal.clone().requires_grad_(True)
    with pytest.raises(NotImplementedError, match="fp8"):
        vit(x)
    vit.disable_fp8()
    # without an input gradient, nothing changes: the frozen model records no graph
    y = vit(cal)
    assert not y.requires_grad
