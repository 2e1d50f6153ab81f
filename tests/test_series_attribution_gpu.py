"""Spatio-temporal attribution of the 4D model on MI355X (csrc/series_attr.hip: nv_gradcam_reduce_grouped, nv_series_map_to_volumes,
nv_series_leave_one_out, nv_temporal_grad_x_input; NeuroEncoder.attribution_series / temporal_importance; ViT score_grad / gradcam_taps).

Gates (the yardsticks are the CPU restatements of tests/series_attribution_ref.py, pinned by tests/test_series_attribution_cpu.py):
  selection     normalised maps, cuts and thresholded maps have the restatement's bits - ties (about half the cells are exact zeros) included;
                T = 1 has the bits of nv_token_map_to_volume;
  upsampling    layout SERIES equals layout FRAMES permuted, bit for bit (the two kernels run the same taps in the same operation order:
                attr_common.h's blend / plane_value); FRAMES with scope VOLUME equals nv_token_map_to_volume on the B T volumes, bit for bit;
                both within VOLUME_TOL of the restatement; `out` pre-filled with NaN comes back finite and the guard tail behind it stays NaN;
  Grad-CAM      group = 1 / group = V have the bits of nv_gradcam_reduce_per_volume / nv_gradcam_reduce; group = T against the float64 formula
                at the 2e-5 of test_modules_gpu.py::test_gradcam_reduce_kernel_matches_formula;
  module        the seed through the temporal head (hook gradient, per-head attention gradients) against the oracle composition
                ref_cpu.vit_forward -> ref_cpu.temporal_head -> autograd with the three-way gates of test_engine_gpu (GRAD_REL, RATIO, SLACK);
                token maps and volumes of all three methods against restatements from the device's own taps / exported terms.
A normalised map spans [0, r / (r + 1e-8)] of its raw range r - the reference's normalisation, which reaches 1 only for r >> 1e-8.  The test
models (series_attribution_ref.micro_4d_model) keep the temporal head's LayerNorms out of saturation, so r is ~1e-6 for Grad-CAM (pinned on
the CPU) and the group maxima are gated at > 0.9 (Grad-CAM), > 0.999 (rollout); every map and volume gate is relative to the largest cell.
Measured errors go to the parity report of test_engine_gpu.report.
"""
import pytest
import torch

import series_attribution_ref as R
import weights as W
from conftest import rel_l2
from test_attribution_volume_cpu import VOLUME_TOL, minmax_reciprocal, relu_maps
from test_engine_gpu import GRAD_REL, RATIO, SLACK, report
from test_input_grad_gpu import three_way

pytestmark = pytest.mark.gpu
KEEPS = sorted({5, W.neuro_config(32, 8)["GRADCAM_THRESHOLD"], 37.5, 100})
SELECTION = [(1, (4, 4, 4), (32,) * 3), (3, (2, 2, 2), (8,) * 3), (5, (4, 6, 5), (20, 36, 45)), (20, (10,) * 3, (20,) * 3), (8, (16,) * 3, (32,) * 3)]
UPSAMPLING = [(3, (4, 6, 5), (20, 36, 45)), (4, (2, 2, 2), (16,) * 3), (20, (4, 4, 4), (32,) * 3)]
GUARD = 64            # floats behind `out` that must stay untouched
METHODS = ("gradcam", "rollout", "relevance")


@pytest.fixture(scope="module", autouse=True)
def gpu():
    from neurovit_amd._cabi import require_gpu
    require_gpu()


def ident(case):
    T, grid, size = case
    return f"T{T}-{grid[0]}x{grid[1]}x{grid[2]}to{size[0]}"


def series_maps(B, T, N, seed):
    """[B, T, N] ReLU-of-normal maps whose timepoints and samples have different ranges"""
    raw = relu_maps(B * T, N, seed) * torch.linspace(0.05, 9.0, B * T)[:, None]
    return raw.reshape(B, T, N)


def run_kernel(maps_cpu, grid, size, keep, scope, layout, normalize=True):
    """(volumes, normalised maps, thresholded maps, cuts) of nv_series_map_to_volumes on the CPU; `out` pre-filled with NaN inside a larger
    NaN buffer whose tail must come back untouched"""
    from neurovit_amd import ops
    B, T = maps_cpu.shape[:2]
    shape = (B,) + tuple(size) + (T,) if layout == "series" else (B, T) + tuple(size)
    numel = B * T * size[0] * size[1] * size[2]
    buf = torch.full((numel + GUARD,), float("nan"), device="cuda")
    out = buf[:numel].view(shape)
    vols, (norm, sparse, cuts) = ops.series_maps_to_volumes(maps_cpu.cuda(), grid, size, normalize=normalize, scope=scope, keep_percent=keep,
                                                           layout=layout, return_maps=True, out=out)
    assert vols.data_ptr() == buf.data_ptr() and vols.shape == shape
    assert torch.isnan(buf[numel:]).all(), "the kernel wrote behind `out`"
    assert torch.isfinite(vols).all(), "NaN left in `out`"
    return vols.cpu(), norm.cpu(), sparse.cpu(), cuts.cpu()


# ---------------------------------------------------------------------------------------------------------------- kernels

@pytest.mark.parametrize("keep", KEEPS)
@pytest.mark.parametrize("case", SELECTION, ids=ident)
def test_selection_against_cpu_restatement(case, keep):
    from neurovit_amd import ops
    T, grid, size = case
    N = grid[0] * grid[1] * grid[2]
    raw = series_maps(2, T, N, 7 * N + T + int(keep))
    assert float((raw == 0).float().mean()) > 0.3                                    # ties are the normal case
    for scope in ("series", "volume"):
        vols, norm, sparse, cuts = run_kernel(raw, grid, size, keep, scope, "frames")
        want_norm, want_cuts, want_sparse, want_vols = R.restate_series(raw, grid, size, keep, scope)
        err = float((vols - want_vols).abs().max())
        report(f"series selection {ident(case)} keep {keep} scope {scope}: cut diff {float((cuts - want_cuts).abs().max()):.1e}, kept cells "
               f"{int((sparse > 0).sum())} (mismatches {int(((sparse > 0) != (want_sparse > 0)).sum())}), volume max |err| {err:.2e}")
        assert torch.equal(norm, want_norm), (scope, "normalised maps")
        assert torch.equal(cuts, want_cuts), (scope, cuts, want_cuts)
        kept = norm >= (cuts[:, None, None] if scope == "series" else cuts[:, :, None])
        want_kept = want_norm >= (want_cuts[:, None, None] if scope == "series" else want_cuts[:, :, None])
        assert torch.equal(kept, want_kept) and torch.equal(sparse, want_sparse), scope
        assert err <= VOLUME_TOL, (scope, err)
    # constant and all-zero samples: (c - c) * inv = 0 everywhere, the cut is 0, everything is kept
    flat = torch.stack([torch.full((T, N), 0.25), torch.zeros(T, N)])
    vols, norm, sparse, cuts = run_kernel(flat, grid, size, keep, "series", "frames")
    assert float(vols.abs().max()) == 0.0 and float(norm.abs().max()) == 0.0 and float(cuts.abs().max()) == 0.0
    if T == 1:                                                                       # one timepoint: nv_token_map_to_volume, bit for bit
        for scope in ("series", "volume"):
            for layout in ("series", "frames"):
                vols, norm, sparse, cuts = run_kernel(raw, grid, size, keep, scope, layout)
                want, (n3, s3, c3) = ops.token_maps_to_volumes(raw[:, 0].contiguous().cuda(), grid, size, normalize=True, keep_percent=keep, return_maps=True)
                assert torch.equal(vols.reshape(want.shape), want.cpu()), (scope, layout)
                assert torch.equal(norm[:, 0], n3.cpu()) and torch.equal(sparse[:, 0], s3.cpu()) and torch.equal(cuts.reshape(-1), c3.cpu())


@pytest.mark.parametrize("case", UPSAMPLING, ids=ident)
def test_upsampling_layouts(case):
    from neurovit_amd import ops
    T, grid, size = case
    N = grid[0] * grid[1] * grid[2]
    B = 2
    raw = series_maps(B, T, N, 3 * N + T)
    keep = 37.5
    for scope in ("series", "volume"):
        frames, norm_f, sparse_f, cuts_f = run_kernel(raw, grid, size, keep, scope, "frames")
        series, norm_s, sparse_s, cuts_s = run_kernel(raw, grid, size, keep, scope, "series")
        assert series.shape == (B,) + tuple(size) + (T,) and frames.shape == (B, T) + tuple(size)
        assert torch.equal(norm_s, norm_f) and torch.equal(sparse_s, sparse_f) and torch.equal(cuts_s, cuts_f)
        assert torch.equal(series, frames.permute(0, 2, 3, 4, 1)), (scope, float((series - frames.permute(0, 2, 3, 4, 1)).abs().max()))    # bit for bit
        want = R.restate_series(raw, grid, size, keep, scope)[3]
        err = float((frames - want).abs().max())
        report(f"series upsampling {ident(case)} scope {scope}: volume max |err| {err:.2e} (both layouts, bit-equal to each other)")
        assert err <= VOLUME_TOL, (scope, err)
        assert float(frames.max()) > 0.5                                              # (the gates above did not compare zeros)
        if scope == "volume":
            flat = raw.reshape(B * T, N).contiguous().cuda()
            per_volume = ops.token_maps_to_volumes(flat, grid, size, normalize=True, keep_percent=keep)
            assert torch.equal(frames.reshape(per_volume.shape), per_volume.cpu())    # bit for bit
    # keep everything: the dense case, no zeros from the threshold
    frames = run_kernel(raw, grid, size, 100, "series", "frames")[0]
    series = run_kernel(raw, grid, size, 100, "series", "series")[0]
    assert torch.equal(series, frames.permute(0, 2, 3, 4, 1))
    assert float((frames - R.restate_series(raw, grid, size, 100, "series")[3]).abs().max()) <= VOLUME_TOL


def test_batch_independence():
    from neurovit_amd import ops
    for T, grid, size in UPSAMPLING:
        N = grid[0] * grid[1] * grid[2]
        maps = series_maps(3, T, N, 41).cuda()
        for scope in ("series", "volume"):
            together, (norm, sparse, cuts) = ops.series_maps_to_volumes(maps, grid, size, scope=scope, keep_percent=5, return_maps=True)
            for b in range(3):
                alone, (n1, s1, c1) = ops.series_maps_to_volumes(maps[b:b + 1].contiguous(), grid, size, scope=scope, keep_percent=5, return_maps=True)
                assert torch.equal(together[b], alone[0]), (T, grid, scope, b)
                assert torch.equal(norm[b], n1[0]) and torch.equal(sparse[b], s1[0]) and torch.equal(cuts[b], c1[0])


@pytest.mark.parametrize("fmt", ["bf16", "fp16"])
@pytest.mark.parametrize("n", [9, 65])
def test_gradcam_reduce_grouped(fmt, n):
    from neurovit_amd import _cabi, ops
    before = _cabi.operand_format()
    _cabi.set_operand_format(fmt)
    try:
        V, T, d = 6, 3, 128
        g = torch.Generator().manual_seed(31 + n)
        act = torch.randn(V, n, d, generator=g).to(ops.op16()).cuda()
        grad = (1e-3 * torch.randn(V, n, d, generator=g) * torch.tensor([1.0, 25.0, 0.04, 3.0, 0.5, 8.0]).view(V, 1, 1)).cuda()
        one, mm_one = ops.gradcam_reduce_grouped(act, grad, 1)
        per_volume, mm_pv = ops.gradcam_reduce_per_volume(act, grad)
        assert torch.equal(one, per_volume) and torch.equal(mm_one, mm_pv)                       # bit for bit
        whole, mm_whole = ops.gradcam_reduce_grouped(act, grad, V)
        batch, mm_b = ops.gradcam_reduce(act, grad)
        assert torch.equal(whole, batch) and torch.equal(mm_whole.reshape(-1), mm_b.reshape(-1))
        cam, mm = ops.gradcam_reduce_grouped(act, grad, T)
        assert cam.shape == (V, n - 1) and mm.shape == (V // T, 2)
        raw = R.gradcam_raw(act.cpu(), grad.cpu()).reshape(V // T, T * (n - 1))
        lo, hi = raw.amin(1, keepdim=True), raw.amax(1, keepdim=True)
        want = ((raw - lo) / (hi - lo + 1e-8)).reshape(V, n - 1)
        err = float((cam.cpu().double() - want).abs().max())
        report(f"nv_gradcam_reduce_grouped {fmt} n={n} group={T}: max |err| vs float64 {err:.2e}")
        assert err < 2e-5, err
        for s in range(V // T):                                                                   # one min and one max per sample
            rows = cam[s * T:(s + 1) * T]
            assert float(rows.min()) == 0.0 and float(rows.max()) > 0.999
            alone, _ = ops.gradcam_reduce(act[s * T:(s + 1) * T].contiguous(), grad[s * T:(s + 1) * T].contiguous())
            assert torch.equal(rows, alone)                                                       # the sample alone, as one batch: the same bits
        again, _ = ops.gradcam_reduce_grouped(act, grad, T)                                       # the tickets reset
        assert torch.equal(again, cam)
    finally:
        _cabi.set_operand_format(before)


@pytest.mark.parametrize("B,T", [(1, 1), (2, 3), (5, 64), (300, 20)])
def test_leave_one_out_and_grad_x_input_against_torch(B, T):
    from neurovit_amd import ops
    g = torch.Generator().manual_seed(B + T)
    z, dx, z_base = torch.randn(B, T, 2, generator=g), torch.randn(B, T, 2, generator=g), torch.randn(2, generator=g)
    z[0, 0, 0], z_base[1] = float("inf"), -0.0                                                   # a pure select: every bit passes through
    table = ops.series_leave_one_out(z.cuda(), z_base.cuda()).cpu()
    want = R.leave_one_out_table(z, z_base)
    assert table.shape == (B * (T + 1), T, 2) and torch.equal(table.view(torch.int32), want.view(torch.int32))
    z[0, 0, 0] = 1.5
    got = ops.temporal_grad_x_input(dx.cuda(), z.cuda()).cpu()
    assert got.shape == (B, T) and torch.equal(got, R.grad_x_input(dx, z))                       # separately rounded: torch's bits on the CPU


# ---------------------------------------------------------------------------------------------------------------- module

def build(tmp_path, case, **extra):
    T, B, seed, head = case
    model, cfg4 = R.micro_4d_model(tmp_path, "cuda:0", head, **extra)
    return model, cfg4, W.make_volume((B, R.S, R.S, R.S, T), seed), T, B


def targets_of(B):
    return torch.tensor([0, 1][:B], dtype=torch.long) if B <= 2 else torch.arange(B) % 2


def as_video(series):
    """[B, S, S, S, T] -> the [B T, 1, D, H, W] view attribution_series feeds the encoder"""
    B, T = series.shape[0], series.shape[-1]
    return series.movedim(-1, 1).reshape(B * T, R.S, R.S, R.S).permute(0, 3, 1, 2).unsqueeze(1)


@pytest.mark.parametrize("chunk", ["whole", 2])
@pytest.mark.parametrize("case", R.MODULE_CASES, ids=lambda c: f"T{c[0]}B{c[1]}")
def test_seed_through_the_head_against_the_oracle_composition(tmp_path, case, chunk):
    model, cfg4, series, T, B = build(tmp_path, case)
    vit = model.volume_encoder.vit3d
    V = B * T
    chunk = V if chunk == "whole" else chunk
    target = targets_of(B)
    out = model.attribution_series(series.cuda(), method="gradcam", target=target.cuda(), chunk=chunk)
    hook = vit.last_attn_norm_grad_raw().cpu()                    # the last pass: every volume (one chunk), or the last `chunk` volumes
    first = V - hook.shape[0]
    assert hook.shape[0] == (V if chunk >= V else (V - 1) % chunk + 1)
    sd = {k: v.detach().cpu() for k, v in model.state_dict().items()}
    emu = R.oracle_series(sd, cfg4, series, True, target=target, want=("hook", "dP"))
    f32 = R.oracle_series(sd, cfg4, series, False, target=target, want=("hook", "dP"))
    tag = f"series-seed T{T} B{B} chunk {chunk}"
    three_way(tag + " hook gradient", hook, emu["grad"][first:], f32["grad"][first:])
    assert torch.equal(out["class_idx"].cpu(), target) and out["logits"].shape == (B, 2) and out["volume_logits"].shape == (B, T, 2)
    assert rel_l2(out["volume_logits"].cpu(), emu["z"]) <= GRAD_REL
    # the temporal key is grad x input of the same pass
    logits, cls, dx = model._head_seed(out["volume_logits"], target.cuda())
    assert torch.equal(logits, out["logits"]) and torch.equal(out["temporal"].cpu(), R.grad_x_input(dx.cpu(), out["volume_logits"].cpu()))
    _, _, dx_emu = R.head_seed(sd, emu["z"], target)
    report(f"{tag}: final logits vs emulating oracle rel L2 {rel_l2(out['logits'].cpu(), emu['logits']):.3e}, dx {rel_l2(dx.cpu(), dx_emu):.3e}")
    if chunk < V:
        return
    # per-head attention gradients seeded with dx: the gate of test_attention_gradients_three_way
    video = as_video(series.cuda())
    with torch.no_grad():
        _, maps = vit.attention_gradients(video, score_grad=dx.view(V, 2))
    fails = []
    for l in range(vit._cfg.depth):
        got = maps[l].cpu()
        e_he, e_h32, e_e32 = rel_l2(got, emu["dP"][l]), rel_l2(got, f32["dP"][l]), rel_l2(emu["dP"][l], f32["dP"][l])
        report(f"{tag} attention-grad layer {l}: hip-emu {e_he:.3e}  hip-fp32 {e_h32:.3e}  emu-fp32 {e_e32:.3e}")
        if not (e_h32 <= RATIO * e_e32 + SLACK and e_he <= GRAD_REL):
            fails.append((l, e_he, e_h32, e_e32))
    assert not fails, fails
    # the one-hot of c as score_grad has the bits of target = c; gradcam_taps leaves the hook gradient of the same backward
    for c in (0, 1):
        _, by_target = vit.attention_gradients(video, target=c)
        hook_c = vit.last_attn_norm_grad_raw().clone()
        onehot = torch.nn.functional.one_hot(torch.full((V,), c, device="cuda"), 2).float()
        logits_c, by_seed = vit.attention_gradients(video, score_grad=onehot)
        assert all(torch.equal(by_target[l], by_seed[l]) for l in by_target)
        assert torch.equal(vit.gradcam_taps(video, onehot), logits_c) and torch.equal(vit.last_attn_norm_grad_raw(), hook_c)
    with pytest.raises(ValueError, match="mutually exclusive"):
        vit.attention_gradients(video, target=0, score_grad=onehot)
    with pytest.raises(ValueError, match="score_grad must be"):
        vit.attention_gradients(video, score_grad=onehot[:1])


def check_volumes(tag, out, G, keep, scope, layout):
    """volumes and cuts of an attribution_series result against the restatement of its returned token maps (every gate of the kernel tests;
    VOLUME_TOL is for cells in [0, 1], so it is scaled by the largest cell of the maps: a small map cannot pass by being small)"""
    maps = out["token_maps"].cpu()
    B, T, N = maps.shape
    _, want_cuts, want_sparse, want_vols = R.restate_series(maps, (G,) * 3, (R.S,) * 3, keep, scope, normalize=False)
    vols = out["volumes"].cpu()
    frames = vols.permute(0, 4, 1, 2, 3) if layout == "series" else vols
    assert vols.shape == ((B, R.S, R.S, R.S, T) if layout == "series" else (B, T, R.S, R.S, R.S)) and vols.dtype == torch.float32
    top = float(maps.max())
    err = float((frames - want_vols).abs().max())
    report(f"attribution_series {tag} scope {scope} layout {layout}: volume max |err| {err:.2e} (largest cell {top:.3f})")
    assert top > 0 and float(want_vols.max()) > 0
    assert torch.equal(out["cuts"].cpu(), want_cuts), tag
    assert torch.isfinite(vols).all() and err <= VOLUME_TOL * top, (tag, err, top)


def replay_taps(model, series_gpu, seeds, chunk):
    """the Grad-CAM taps [B T, n, d] of every volume, chunk by chunk as attribution_series runs them (the same passes: the same bits)"""
    vit = model.volume_encoder.vit3d
    video = as_video(series_gpu)
    V = video.shape[0]
    acts, grads = [], []
    for first in range(0, V, chunk):
        vit.gradcam_taps(video[first:first + chunk], seeds[first:first + chunk].contiguous())
        acts.append(vit.last_attn_norm_output_raw().float().cpu())
        grads.append(vit.last_attn_norm_grad_raw().cpu())
    return torch.cat(acts), torch.cat(grads)


def check_gradcam_maps(tag, out, act, grad, scope):
    """Grad-CAM token maps against the float64 restatement of the device's taps of ALL volumes, relative to the largest cell of each
    normalisation group (2e-5 of test_modules_gpu.py::test_gradcam_reduce_kernel_matches_formula, whose maps peak at 1)"""
    B, T, N = out["token_maps"].shape
    group = T if scope == "series" else 1
    want = R.gradcam_normalised(act, grad, group).reshape(B * T // group, group * N)
    got = out["token_maps"].cpu().double().reshape(want.shape)
    top = want.amax(1, keepdim=True)
    err = ((got - want).abs() / top).max().item()
    report(f"attribution_series {tag} scope {scope}: Grad-CAM maps vs float64 of the device's taps, max |err| / group max {err:.2e} (group maxima {top.min().item():.3f} .. {top.max().item():.3f})")
    assert (top > 0.9).all(), top                                                  # (precondition, pinned on the CPU: raw ranges >> 1e-8)
    assert err < 2e-5, err
    assert (got.amin(1) == 0).all() and (got.amax(1) > 0.9).all()
    return got.reshape(B, T, N)


@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("case", R.MODULE_CASES, ids=lambda c: f"T{c[0]}B{c[1]}")
def test_token_maps_and_volumes_against_restatements(tmp_path, case, method):
    from neurovit_amd import ops
    model, cfg4, series, T, B = build(tmp_path, case)
    vit = model.volume_encoder.vit3d
    G, keep, V = R.S // R.PATCH, cfg4["GRADCAM_THRESHOLD"], B * T
    N = G ** 3
    x = series.cuda()
    target = targets_of(B).cuda()
    video = as_video(x)
    by_scope = {}
    for scope in ("series", "volume"):
        for layout in ("series", "frames"):
            out = model.attribution_series(x, method=method, target=target, scope=scope, layout=layout)
            assert all(v.is_cuda for v in out.values()) and out["token_maps"].shape == (B, T, N) and out["temporal"].shape == (B, T)
            check_volumes(f"{method} T{T} B{B}", out, G, keep, scope, layout)
        maps = out["token_maps"].cpu()
        group = maps.reshape(B, T * N) if scope == "series" else maps.reshape(V, N)
        if method == "gradcam":
            # the restatement from the device's own taps (the one pass of this call is still in the workspace), in float64
            act, grad = vit.last_attn_norm_output_raw().float().cpu(), vit.last_attn_norm_grad_raw().cpu()
            by_scope[scope] = check_gradcam_maps(f"gradcam T{T} B{B}", out, act, grad, scope)
        else:
            # the exported terms of the same passes: the raw maps of the ViT-level call, normalised by the restatement's rule, bit for bit
            _, _, dx = model._head_seed(out["volume_logits"], target)
            with torch.no_grad():
                raw = vit.attention_rollout(video)[1] if method == "rollout" else vit.attention_relevance(video, score_grad=dx.view(V, 2))[1]
            assert torch.equal(group, minmax_reciprocal(raw.cpu().reshape(group.shape))), (method, scope)
            by_scope[scope] = maps.double()
        # one minimum and one maximum per normalisation group: the sample (scope "series") or the volume; the maximum is r / (r + 1e-8) of the raw range r
        floor = {"rollout": 0.999, "gradcam": 0.9, "relevance": 0.0}[method]
        report(f"attribution_series {method} T{T} B{B} scope {scope}: group maxima {float(group.amax(1).min()):.6f} .. {float(group.amax(1).max()):.6f}")
        assert (group.amin(dim=1) == 0).all() and (group.amax(dim=1) > floor).all() and float(group.max()) <= 1.0
    # the scopes differ: jointly normalised, only the strongest timepoint of a sample reaches the top; per volume every timepoint does
    per_volume = {k: v.reshape(B, T, -1).amax(2) for k, v in by_scope.items()}
    assert (per_volume["volume"] > floor).all() and not torch.equal(by_scope["series"], by_scope["volume"])
    if method == "gradcam":                                       # (pinned on the CPU: the raw ranges of a sample's timepoints differ by more than 1.2)
        assert (per_volume["series"].amin(1) < 0.9 * per_volume["series"].amax(1)).all(), per_volume["series"]
        assert (by_scope["series"] <= by_scope["volume"] * (1 + 1e-4)).all()       # both subtract a minimum of 0; the joint range is the larger divisor
    # target None explains the arg-max of the FINAL logits
    free = model.attribution_series(x, method=method)
    same = model.attribution_series(x, method=method, target=target)
    assert torch.equal(free["class_idx"], free["logits"].argmax(dim=1)) and torch.equal(same["class_idx"], target)
    flipped = model.attribution_series(x, method=method, target=1 - target)
    if method == "rollout":                                       # class-agnostic: the maps do not depend on the target
        assert torch.equal(free["token_maps"], same["token_maps"]) and torch.equal(flipped["token_maps"], same["token_maps"])
    else:
        assert not torch.equal(flipped["token_maps"], same["token_maps"])


@pytest.mark.parametrize("case", R.MODULE_CASES, ids=lambda c: f"T{c[0]}B{c[1]}")
def test_scope_volume_rollout_equals_the_3d_path(tmp_path, case):
    from neurovit_amd.NeuroEncoder import NeuroEncoder
    model, cfg4, series, T, B = build(tmp_path, case)
    m3 = NeuroEncoder(W.neuro_config(R.S, R.PATCH, DEVICE="cuda:0", **R.MICRO_SIZE)).eval()
    m3.load_state_dict(R.encoder_state(), strict=True)
    x = series.cuda()
    out = model.attribution_series(x, method="rollout", scope="volume", layout="frames")
    volumes3 = x.movedim(-1, 1).reshape(B * T, R.S, R.S, R.S).contiguous()              # the same B T volumes, as a 3D batch
    vols3, _, maps3 = m3.attribution_volumes(volumes3, method="rollout", return_token_maps=True)
    assert torch.equal(out["token_maps"].reshape(maps3.shape), maps3)
    assert torch.equal(out["volumes"].reshape(vols3.shape), vols3)
    series_layout = model.attribution_series(x, method="rollout", scope="volume", layout="series")
    assert torch.equal(series_layout["volumes"], out["volumes"].permute(0, 2, 3, 4, 1))


@pytest.mark.parametrize("case", R.MODULE_CASES, ids=lambda c: f"T{c[0]}B{c[1]}")
def test_state_is_left_alone(tmp_path, case):
    model, cfg4, series, T, B = build(tmp_path, case)
    x = series.cuda()
    labels = targets_of(B).cuda()
    head = list(model.temporal_transformer.parameters()) + list(model.projection_head.parameters())

    def step():
        model.zero_grad(set_to_none=True)
        loss = torch.nn.functional.cross_entropy(model(x), labels)
        loss.backward()
        return loss.detach().clone(), [p.grad.clone() for p in head]
    loss_before, grads_before = step()
    kept = [p.grad for p in head]
    results = {}
    for method in METHODS:
        results[method] = model.attribution_series(x, method=method)
        assert all(p.grad is None for p in model.volume_encoder.parameters()), method
        assert all(p.grad is g and torch.equal(g, g0) for p, g, g0 in zip(head, kept, grads_before)), method       # the head's .grad: same tensors, same bits
        assert model.volume_encoder.vit3d._grads is None                                    # no parameter-sized gradient arena either
        with torch.no_grad():
            again = model.attribution_series(x, method=method)
        assert all(torch.equal(results[method][k], again[k]) for k in again), method
    importance = model.temporal_importance(x)
    assert all(p.grad is g and torch.equal(g, g0) for p, g, g0 in zip(head, kept, grads_before))
    assert x.grad is None and not x.requires_grad
    loss_after, grads_after = step()
    assert torch.equal(loss_after, loss_before) and all(torch.equal(a, b) for a, b in zip(grads_after, grads_before))
    assert importance["grad_x_input"].shape == (B, T)


@pytest.mark.parametrize("method", METHODS)
def test_chunked_passes(tmp_path, method):
    """chunk = 2 splits the B T = 8 volumes of the second case over four passes (and a sample over two): the gates of the unchunked route"""
    from neurovit_amd import ops
    case = R.MODULE_CASES[1]
    model, cfg4, series, T, B = build(tmp_path, case)
    vit = model.volume_encoder.vit3d
    G, keep, V = R.S // R.PATCH, cfg4["GRADCAM_THRESHOLD"], B * T
    x = series.cuda()
    target = targets_of(B).cuda()
    whole = model.attribution_series(x, method=method, target=target, chunk=V)
    for scope in ("series", "volume"):
        out = model.attribution_series(x, method=method, target=target, scope=scope, chunk=2)
        check_volumes(f"{method} chunk 2", out, G, keep, scope, "series")
        maps = out["token_maps"].cpu()
        group = maps.reshape(B, -1) if scope == "series" else maps.reshape(V, -1)
        assert (group.amin(dim=1) == 0).all() and (group.amax(dim=1) > 0).all()
        if method == "gradcam":
            # the taps of every volume, replayed chunk by chunk with the call's own seeds: the gather of the chunks, row by row
            _, _, dx = model._head_seed(out["volume_logits"], target)
            act, grad = replay_taps(model, x, dx.view(V, 2), 2)
            check_gradcam_maps("gradcam chunk 2", out, act, grad, scope)
        if method == "rollout":
            assert (group.amax(dim=1) > 0.999).all()
        # across the routes: the same maps to the precision of the passes
        same_scope = whole if scope == "series" else model.attribution_series(x, method=method, target=target, scope=scope, chunk=V)
        err = rel_l2(maps, same_scope["token_maps"].cpu())
        report(f"attribution_series {method} scope {scope}: chunk 2 against one pass, token maps rel L2 {err:.2e}")
        assert err <= GRAD_REL, (method, scope, err)
    # the two routes agree to the precision of the arithmetic (not bit for bit: GEMM plans may differ with the row count)
    assert torch.equal(out["class_idx"], whole["class_idx"])
    assert rel_l2(out["volume_logits"].cpu(), whole["volume_logits"].cpu()) <= GRAD_REL
    assert rel_l2(out["temporal"].cpu(), whole["temporal"].cpu()) <= GRAD_REL
    with pytest.raises(ValueError, match="chunk"):
        model.attribution_series(x, chunk=0)


@pytest.mark.parametrize("case", R.MODULE_CASES, ids=lambda c: f"T{c[0]}B{c[1]}")
def test_temporal_importance(tmp_path, case):
    from neurovit_amd import ops
    model, cfg4, series, T, B = build(tmp_path, case)
    x = series.cuda()
    target = targets_of(B).cuda()
    head = model._temporal_head
    for kind in ("logit", "prob"):
        out = model.temporal_importance(x, target=target, baseline=0.5, score=kind)
        z = out["volume_logits"]
        assert z.shape == (B, T, 2) and out["occlusion"].shape == (B, T) and out["scores"].shape == (B, T + 1)
        with torch.no_grad():
            assert torch.equal(z, model._volume_logits(x))                                   # the model's own forward: one encoder pass
            z_base = model.volume_encoder(torch.full((1, R.S, R.S, R.S), 0.5, device="cuda"))[0]
            assert torch.equal(out["logits"], head(z))
            for b in range(B):
                for t in range(T):                                                           # hand-built sequences through the head's own forward
                    seq = z[b:b + 1].clone()
                    seq[0, t] = z_base
                    full, cut = head(z[b:b + 1]), head(seq)
                    c = int(target[b])
                    if kind == "logit":
                        want = full[0, c] - cut[0, c]
                    else:
                        jobs = torch.zeros(1, 3, dtype=torch.int32, device="cuda")
                        want = ops.class_scores(full, jobs, target[b:b + 1], kind="prob")[0] - ops.class_scores(cut, jobs, target[b:b + 1], kind="prob")[0]
                        soft = torch.softmax(full, 1)[0, c] - torch.softmax(cut, 1)[0, c]
                        assert abs(float(want) - float(soft)) <= 1e-6
                    assert torch.equal(out["occlusion"][b, t], want), (kind, b, t)
        _, _, dx = model._head_seed(z, target)
        assert torch.equal(out["grad_x_input"].cpu(), R.grad_x_input(dx.cpu(), z.cpu()))
        sd = {k: v.detach().cpu() for k, v in model.state_dict().items()}
        _, _, dx64 = R.head_seed(sd, z.cpu(), target.cpu(), double=True)
        err = float((dx.cpu().double() - dx64).abs().max())
        report(f"temporal_importance T{T} B{B}: dx against the float64 oracle head, max |err| {err:.2e} (max |dx| {float(dx64.abs().max()):.2e})")
        assert err <= 2e-4 * float(dx64.abs().max()), err                 # the relative part of the dx gate of tests/test_temporal_gpu.py
        assert torch.equal(out["class_idx"], target)
    free = model.temporal_importance(x)
    assert torch.equal(free["class_idx"], free["logits"].argmax(dim=1))
    # a constant series occluded by the same constant: nothing changes, the occlusion is exactly 0
    const = torch.full((B, R.S, R.S, R.S, T), 0.25, device="cuda")
    for kind in ("logit", "prob"):
        out = model.temporal_importance(const, baseline=0.25, score=kind)
        print(f"temporal_importance T{T} B{B} {kind}: constant series, max |occlusion| {float(out['occlusion'].abs().max()):.3e}")
        assert (out["occlusion"] == 0).all(), out["occlusion"]


def test_refusals(tmp_path):
    from neurovit_amd.NeuroEncoder import NeuroEncoder
    model, cfg4, series, T, B = build(tmp_path, R.MODULE_CASES[0])
    x = series.cuda()
    vit = model.volume_encoder.vit3d
    for kw in (dict(method="lime"), dict(scope="batch"), dict(layout="nifti"), dict(chunk=0), dict(chunk=1.5), dict(chunk=-3)):
        with pytest.raises(ValueError, match=next(iter(kw))):
            model.attribution_series(x, **kw)
    with pytest.raises(ValueError, match="score"):
        model.temporal_importance(x, score="odds")
    with pytest.raises(ValueError, match="baseline"):
        model.temporal_importance(x, baseline=torch.zeros(1, R.S, R.S, R.S))
    with pytest.raises(ValueError, match="x must be"):
        model.attribution_series(x[..., 0])
    with pytest.raises(ValueError, match="target"):
        model.attribution_series(x, target=2)
    m3 = NeuroEncoder(W.neuro_config(R.S, R.PATCH, DEVICE="cuda:0", **R.MICRO_SIZE)).eval()
    for call in (m3.attribution_series, m3.temporal_importance):
        with pytest.raises(NotImplementedError, match="4D model only"):
            call(x)
    # the existing 3D-only refusals keep their words
    with pytest.raises(NotImplementedError, match="3D model only"):
        model.attribution_volumes(x[..., 0])
    # a head the native kernel does not compute
    layer = model.temporal_transformer.transformer.layers[0]
    layer.norm_first = True
    for call in (model.attribution_series, model.temporal_importance):
        with pytest.raises(NotImplementedError, match="TemporalHead.supported"):
            call(x)
    layer.norm_first = False
    with pytest.raises(NotImplementedError, match="TemporalHead.supported"):
        model.attribution_series(torch.zeros(1).expand(1, R.S, R.S, R.S, 65))             # more than 64 timepoints
    # dropout in train mode: the head (nn.TransformerEncoderLayer's default p = 0.1), the encoder
    model.temporal_transformer.train()
    for call in (model.attribution_series, model.temporal_importance):
        with pytest.raises(NotImplementedError, match="temporal head is in train mode"):
            call(x)
    model.temporal_transformer.eval()
    wet, _, _, _, _ = build(tmp_path, R.MODULE_CASES[0], TRAINING_DROPOUT=0.1)
    wet.volume_encoder.train()
    for call in (wet.attribution_series, wet.temporal_importance):
        with pytest.raises(NotImplementedError, match="encoder is in train mode"):
            call(x)
    wet.volume_encoder.eval()
    assert wet.attribution_series(x)["volumes"].shape == (B, R.S, R.S, R.S, T)             # eval mode: dropout does not matter
    # the fp8 forwards
    vit.enable_fp8(as_video(x)[:1])
    for call in (model.attribution_series, model.temporal_importance):
        with pytest.raises(NotImplementedError, match="fp8"):
            call(x)
    vit.disable_fp8()
    assert model.attribution_series(x)["volumes"].shape == (B, R.S, R.S, R.S, T)
    # T G^3 beyond one workgroup's LDS under scope "series": 9 timepoints of a 16^3 grid
    big3 = NeuroEncoder(W.neuro_config(128, 8, dim=3, **R.MICRO_SIZE))
    torch.save(big3.state_dict(), tmp_path / "big.pth")
    big = NeuroEncoder(W.neuro_config(128, 8, dim=4, DEVICE="cuda:0", GLOBAL_BASE_PATH=str(tmp_path), BEST_MODEL_PATH="big.pth", **R.MICRO_SIZE)).eval()
    with pytest.raises(NotImplementedError, match='scope="volume"'):
        big.attribution_series(torch.zeros(1).expand(1, 128, 128, 128, 9))


def test_4d_forward_with_patches_the_fused_gather_does_not_take(tmp_path):
    """9^3 patches (patch_dim % 4 != 0) with T % 4 == 0: the 4D forward regroups the volumes instead of calling the fused gather, which
    refuses them; the result is the head over the encoder's logits of the B T volumes"""
    from neurovit_amd.NeuroEncoder import NeuroEncoder
    S, p, T, B = 27, 9, 4, 2
    torch.manual_seed(5)
    torch.save(NeuroEncoder(W.neuro_config(S, p, dim=3, **R.MICRO_SIZE)).state_dict(), tmp_path / "p9.pth")
    model = NeuroEncoder(W.neuro_config(S, p, dim=4, DEVICE="cuda:0", GLOBAL_BASE_PATH=str(tmp_path), BEST_MODEL_PATH="p9.pth", **R.MICRO_SIZE)).eval()
    x = W.make_volume((B, S, S, S, T), 6).cuda()
    with torch.no_grad():
        out = model(x)
        z = model.volume_encoder(x.movedim(-1, 1).reshape(B * T, S, S, S)).view(B, T, 2)
        assert torch.equal(model._volume_logits(x), z) and torch.equal(out, model._temporal_head(z))
    assert out.shape == (B, 2) and torch.isfinite(out).all()
    assert model.temporal_importance(x)["occlusion"].shape == (B, T)
    assert model.attribution_series(x, method="rollout")["volumes"].shape == (B, S, S, S, T)
