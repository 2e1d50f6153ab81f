"""CPU restatements shared by the series-attribution tests (tests/test_series_attribution_cpu.py pins them, tests/test_series_attribution_gpu.py
measures the kernels of csrc/series_attr.hip and the 4D model's attribution_series / temporal_importance against them), and the micro
4D model both files build.  Everything here is plain torch on the CPU; the 3D restatement it extends is tests/test_attribution_volume_cpu.py's."""
import torch
import torch.nn.functional as F

import weights as W
from oracle import ref_cpu
from test_attribution_volume_cpu import minmax_reciprocal, quantile_cut, restate

MICRO_SIZE = dict(TRAINING_VIT_DIM=128, TRAINING_VIT_DEPTH=2, TRAINING_VIT_HEADS=2, TRAINING_VIT_MLP_DIM=256)
MICRO_VIT = dict(image_size=16, image_patch_size=8, frames=16, frame_patch_size=8, num_classes=2, dim=128, depth=2, heads=2, mlp_dim=256,
                 channels=1, dim_head=64)
S, PATCH = 16, 8
# (T, B, seed of the series, seed of torch.manual_seed for the temporal head): the module cases of the GPU tests.  The CPU file checks that
# every volume of every case has a raw Grad-CAM range above GRADCAM_RAW_FLOOR, so its normalised map r / (r + 1e-8) peaks above 0.9.
MODULE_CASES = [(3, 1, 54, 3), (4, 2, 71, 3)]
ENCODER_SEED = 53
GRADCAM_RAW_FLOOR = 1.5e-7


def restate_series(maps, grid, size, keep_percent, scope, normalize=True):
    """CPU restatement of nv_series_map_to_volumes: maps [B, T, N] fp32 -> (normalised maps [B, T, N], cuts [B] or [B, T], thresholded maps
    [B, T, N], volumes in layout "frames" [B, T, S0, S1, S2]).  Scope "volume": `restate` on each (b, t); scope "series": its normalisation
    and cut on the flattened [B, T N] map, the upsampling per (b, t)."""
    B, T, N = maps.shape
    if scope == "volume":
        flat = maps.reshape(B * T, N)
        norm = minmax_reciprocal(flat) if normalize else flat
        cuts, sparse, vols = restate(norm, grid, size, keep_percent)
        return norm.reshape(B, T, N), cuts.reshape(B, T), sparse.reshape(B, T, N), vols.reshape(B, T, *size)
    flat = maps.reshape(B, T * N)
    norm = minmax_reciprocal(flat) if normalize else flat
    cuts = torch.stack([quantile_cut(m, keep_percent) for m in norm])
    sparse = torch.where(norm >= cuts[:, None], norm, torch.zeros_like(norm))
    vols = F.interpolate(sparse.reshape(B * T, 1, *grid), size=tuple(size), mode='trilinear', align_corners=False)
    return norm.reshape(B, T, N), cuts, sparse.reshape(B, T, N), vols.reshape(B, T, *size)


def leave_one_out_table(z, z_base):
    """[B, T, 2], [2] -> [B (T + 1), T, 2]: row b (T + 1) is z[b], row b (T + 1) + 1 + t is z[b] with timepoint t replaced by z_base"""
    B, T, _ = z.shape
    rows = z[:, None].repeat(1, T + 1, 1, 1)
    for t in range(T):
        rows[:, 1 + t, t] = z_base
    return rows.reshape(B * (T + 1), T, 2)


def grad_x_input(dx, z):
    """[B, T]: sum_c dx[b, t, c] z[b, t, c] in fp32, every product and the sum rounded on its own"""
    return (dx * z).sum(-1)


def class_score(logits, cls, kind):
    rows = torch.arange(logits.shape[0])
    return (torch.softmax(logits, dim=1) if kind == "prob" else logits)[rows, cls]


def head_seed(sd, z, target=None, double=False):
    """(logits [B, 2], class_idx [B], dx [B, T, 2] = d logit_class / d z) of the oracle's temporal head by autograd; double: in float64
    (the two-feature LayerNorms cancel heavily in fp32 autograd: test_temporal_gpu.py measures the native backward against float64)"""
    if double:
        sd = {k: v.double() for k, v in sd.items() if k.startswith(("temporal_transformer.", "projection_head."))}
    leaf = (z.double() if double else z).detach().clone().requires_grad_(True)
    logits = ref_cpu.temporal_head(sd, leaf)
    cls = logits.argmax(dim=1) if target is None else target
    (dx,) = torch.autograd.grad(logits.gather(1, cls[:, None]).sum(), leaf)
    return logits.detach(), cls, dx


def temporal_occlusion(sd, z, z_base, cls, kind):
    """[B, T]: score(z) - score(z with timepoint t replaced), the sequences of leave_one_out_table through the oracle's head"""
    B, T, _ = z.shape
    with torch.no_grad():
        out = ref_cpu.temporal_head(sd, leave_one_out_table(z, z_base))
    scores = class_score(out, cls.repeat_interleave(T + 1), kind).reshape(B, T + 1)
    return scores[:, :1] - scores[:, 1:]


HEAD_LAYER = "temporal_transformer.transformer.layers.0."
ENCODER_LOGIT_SCALE = 1e-2


def encoder_state():
    """the micro encoder's weights, its classifier scaled by ENCODER_LOGIT_SCALE: volume logits of ~1e-2, so that the two-feature LayerNorms of
    the temporal head are not saturated by their own input (at logits of ~1 they pass ~1e-11 of a gradient, and every Grad-CAM map of
    the 4D model would sit below the 1e-8 of the reference's normalisation)"""
    sd = W.make_tensors(W.vit_param_spec(**MICRO_VIT), ENCODER_SEED, prefix="volume_encoder.vit3d.")
    for key in ("volume_encoder.vit3d.mlp_head.1.weight", "volume_encoder.vit3d.mlp_head.1.bias"):
        sd[key] = sd[key] * ENCODER_LOGIT_SCALE
    return sd


def soften_head(model):
    """the scaling tests/test_temporal_gpu.py calls `soft`: both LayerNorm inputs of the temporal head stay near the eps scale, so d logit /
    d volume_logits is ~0.1 and the raw Grad-CAM range of a volume ~1e-6, two decades above the 1e-8 of the normalisation"""
    params = dict(model.named_parameters())
    with torch.no_grad():
        params[HEAD_LAYER + "self_attn.out_proj.weight"].mul_(3e-3)
        params[HEAD_LAYER + "self_attn.out_proj.bias"].mul_(3e-2)
        params[HEAD_LAYER + "norm1.weight"].mul_(4e-3)
        params[HEAD_LAYER + "norm1.bias"].fill_(0.05)
        params[HEAD_LAYER + "linear2.weight"].mul_(2e-2)
        params[HEAD_LAYER + "linear2.bias"].mul_(3e-2)


def micro_4d_model(tmp_path, device, head_seed_value=3, **extra):
    """the micro 4D NeuroEncoder of test_neuro4d_series_gradient_against_oracle_composition (S 16, p 8, d 128, L 2) around a 3D checkpoint
    written to tmp_path (encoder_state), its head softened (soften_head), in eval mode -> (model, its config); extra: further config keys
    of the 4D model"""
    from neurovit_amd.NeuroEncoder import NeuroEncoder
    m3 = NeuroEncoder(W.neuro_config(S, PATCH, dim=3, **MICRO_SIZE))
    m3.load_state_dict(encoder_state(), strict=True)
    torch.save(m3.state_dict(), tmp_path / "c.pth")
    cfg4 = W.neuro_config(S, PATCH, dim=4, DEVICE=device, GLOBAL_BASE_PATH=str(tmp_path), BEST_MODEL_PATH="c.pth", **dict(MICRO_SIZE, **extra))
    torch.manual_seed(head_seed_value)
    model = NeuroEncoder(cfg4).eval()
    soften_head(model)
    return model, cfg4


def oracle_series(sd, cfg4, series, emulate, target=None, want=()):
    """The oracle composition ref_cpu.vit_forward -> ref_cpu.temporal_head -> autograd for a series [B, S, S, S, T] (CPU):
    a dict with z [B, T, 2], logits, cls, and on request ("hook") the activation and the gradient of the last block's attention-LN output
    [B T, n, d] for the class logit of the FINAL logits, ("dP") the per-layer d logit / d P_l [B T, heads, n, n]."""
    B, T = series.shape[0], series.shape[-1]
    cfg = ref_cpu.neuro_cfg(cfg4)
    vsd = ref_cpu.strip_prefix(sd, "volume_encoder.vit3d.")
    taps = {}
    vols = series.permute(0, 4, 1, 2, 3).reshape(B * T, S, S, S).clone().requires_grad_(True)
    z = ref_cpu.vit_forward(vsd, cfg, ref_cpu.fmri_to_video(vols), emulate, taps).reshape(B, T, -1)
    logits = ref_cpu.temporal_head(sd, z)
    cls = logits.argmax(dim=1) if target is None else target
    score = logits.gather(1, cls[:, None]).sum()
    out = {"z": z.detach(), "logits": logits.detach(), "cls": cls}
    if "hook" in want:
        act = taps[f"transformer.layers.{cfg.depth - 1}.0.norm.out"]
        (grad,) = torch.autograd.grad(score, act, retain_graph=True)
        out["act"], out["grad"] = act.detach(), grad
    if "dP" in want:
        outs = [taps[f"transformer.layers.{l}.0.attn.out"] for l in range(cfg.depth)]
        grads = torch.autograd.grad(score, outs, retain_graph=True)
        n = outs[0].shape[1]
        out["dP"] = []
        for l, g in enumerate(grads):
            dO = (ref_cpu._r(g) if emulate else g).reshape(B * T, n, cfg.heads, cfg.dim_head).permute(0, 2, 1, 3)
            out["dP"].append(dO @ taps[f"transformer.layers.{l}.0.v"].detach().transpose(-1, -2))
    return out


def gradcam_raw(act, grad):
    """[V, n, d] taps -> the un-normalised Grad-CAM rows [V, n - 1] in float64: relu(mean_d grad * sum_d act) of the patch tokens"""
    return torch.relu(grad.double().mean(dim=2) * act.double().sum(dim=2))[:, 1:]


def gradcam_normalised(act, grad, group):
    """float64 restatement of nv_gradcam_reduce_grouped: gradcam_raw, min-max normalised over every `group` consecutive volumes -> [V, n - 1]"""
    raw = gradcam_raw(act, grad)
    V, N = raw.shape
    rows = raw.reshape(V // group, group * N)
    lo, hi = rows.amin(1, keepdim=True), rows.amax(1, keepdim=True)
    return ((rows - lo) / (hi - lo + 1e-8)).reshape(V, N)
