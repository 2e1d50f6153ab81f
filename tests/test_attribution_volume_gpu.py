"""Batched device-side attribution volumes on MI355X (nv_gradcam_reduce_per_volume, nv_token_map_to_volume; ops.gradcam_reduce_per_volume,
ops.token_maps_to_volumes; NeuroEncoder.token_maps_to_volumes / attribution_volumes).

Gates (the yardstick is the CPU restatement of tests/test_attribution_volume_cpu.py, which that file pins to the shipped single-volume
NeuroEncoder._token_map_to_volume):
  kernel        per volume the normalised map and the cut have the restatement's bits, so the kept-cell set is identical - no exclusions;
                the volume is within 2e-6 absolute of the restatement (convex combinations of numbers in [0, 1] through seven fp32 lerps;
                the header's index rule against ATen is <= 6e-7 on the CPU, test_index_rule_against_aten); `out` is pre-filled with NaN
                and must come back finite;
  independence  volume b of a batched call is bit-identical to the call on that volume alone;
  Grad-CAM      nv_gradcam_reduce_per_volume: volume b bit-identical to nv_gradcam_reduce on the slice (both operand formats), and
                different from the batch-normalised nv_gradcam_reduce of the whole batch when the volumes' ranges differ;
  module        attribution_volumes of a batch = the restatement of its returned token maps (gates above); rollout / relevance token maps =
                ViT.attention_rollout / attention_relevance of the batch normalised per volume, bit for bit; B = 1 against
                get_attention_map / get_attention_rollout / get_attention_relevance: same class, same kept set, within 2e-6.
Measured errors go to the parity report of test_engine_gpu.report.
"""
import pytest
import torch

import weights as W
from test_attribution_volume_cpu import VOLUME_TOL, minmax_division, minmax_reciprocal, quantile_cut, relu_maps, restate
from test_engine_gpu import report

pytestmark = pytest.mark.gpu
GEOMETRIES = [((4,) * 3, (32,) * 3), ((10,) * 3, (90,) * 3), ((8,) * 3, (128,) * 3), ((16,) * 3, (128,) * 3), ((4, 6, 5), (20, 36, 45))]
KEEPS = sorted({5, W.neuro_config(32, 8)["GRADCAM_THRESHOLD"], 37.5, 100})
MICRO_SIZE = dict(TRAINING_VIT_DIM=128, TRAINING_VIT_DEPTH=2, TRAINING_VIT_HEADS=2, TRAINING_VIT_MLP_DIM=256)
METHODS = ("gradcam", "rollout", "relevance")


@pytest.fixture(scope="module", autouse=True)
def gpu():
    from neurovit_amd._cabi import require_gpu
    require_gpu()


def cells_of(grid):
    return grid[0] * grid[1] * grid[2]


def run_kernel(maps_cpu, grid, size, normalize, keep):
    """(volumes, normalised maps, thresholded maps, cuts) of the kernel, on the CPU; `out` pre-filled with NaN"""
    from neurovit_amd import ops
    out = torch.full((maps_cpu.shape[0],) + tuple(size), float("nan"), device="cuda")
    vols, (norm, sparse, cuts) = ops.token_maps_to_volumes(maps_cpu.cuda(), grid, size, normalize=normalize, keep_percent=keep, return_maps=True, out=out)
    assert vols.data_ptr() == out.data_ptr() and vols.is_cuda and vols.dtype == torch.float32
    return vols.cpu(), norm.cpu(), sparse.cpu(), cuts.cpu()


def check_against_restatement(tag, got, norm_want, grid, size, keep):
    """the gates of the kernel test; norm_want: the expected normalised maps [B, N] (CPU)"""
    vols, norm, sparse, cuts = got
    assert torch.isfinite(vols).all(), tag
    assert torch.equal(norm, norm_want), tag
    want_cuts, want_sparse, want_vols = restate(norm_want, grid, size, keep)
    err = float((vols - want_vols).abs().max())
    kept, want_kept = norm >= cuts[:, None], norm_want >= want_cuts[:, None]
    report(f"attribution volume {tag} grid {tuple(grid)} -> {tuple(size)} keep {keep}: cut diff {float((cuts - want_cuts).abs().max()):.1e}, "
           f"kept cells {int(kept.sum())} (mismatches {int((kept != want_kept).sum())}), volume max |err| {err:.2e}")
    assert torch.equal(cuts, want_cuts), (tag, cuts, want_cuts)
    assert torch.equal(kept, want_kept), tag                                 # every volume, every cell
    assert torch.equal(sparse, want_sparse), tag
    assert err <= VOLUME_TOL, (tag, err)
    return err


@pytest.mark.parametrize("keep", KEEPS)
@pytest.mark.parametrize("grid,size", GEOMETRIES, ids=[f"{g[0]}x{g[1]}x{g[2]}to{s[0]}" for g, s in GEOMETRIES])
def test_kernel_against_cpu_restatement(grid, size, keep):
    N = cells_of(grid)
    raw = relu_maps(3, N, 11 * N + int(keep)) * torch.tensor([[1.0], [7.5], [0.01]])          # three ranges: per-volume normalisation
    assert float((raw == 0).float().mean()) > 0.3
    check_against_restatement("relu normalize=1", run_kernel(raw, grid, size, True, keep), minmax_reciprocal(raw), grid, size, keep)
    pre = minmax_reciprocal(raw)                                                               # an already normalised map, taken as it is
    check_against_restatement("relu normalize=0", run_kernel(pre, grid, size, False, keep), pre, grid, size, keep)
    flat = torch.stack([torch.full((N,), 0.25), torch.zeros(N), relu_maps(1, N, 5)[0]])        # constant, all-zero, and a live neighbour
    got = run_kernel(flat, grid, size, True, keep)
    check_against_restatement("constant / zero", got, minmax_reciprocal(flat), grid, size, keep)
    assert float(got[0][:2].abs().max()) == 0.0                                               # (c - c) * inv = 0: both volumes are zero
    got = run_kernel(flat, grid, size, False, keep)
    check_against_restatement("constant / zero normalize=0", got, flat, grid, size, keep)
    assert float((got[0][0] - 0.25).abs().max()) <= VOLUME_TOL and float(got[0][1].abs().max()) == 0.0


def test_batch_independence():
    from neurovit_amd import ops
    for grid, size in GEOMETRIES:
        maps = (relu_maps(4, cells_of(grid), 21) * torch.tensor([[1.0], [3.0], [0.2], [40.0]])).cuda()
        together = ops.token_maps_to_volumes(maps, grid, size, normalize=True, keep_percent=5)
        for b in range(4):
            alone = ops.token_maps_to_volumes(maps[b:b + 1].contiguous(), grid, size, normalize=True, keep_percent=5)
            assert torch.equal(together[b], alone[0]), (grid, b)


@pytest.mark.parametrize("fmt", ["bf16", "fp16"])
@pytest.mark.parametrize("n,d", [(65, 128), (1001, 256), (513, 768)])
def test_gradcam_reduce_per_volume(fmt, n, d):
    from neurovit_amd import _cabi, ops
    before = _cabi.operand_format()
    _cabi.set_operand_format(fmt)
    try:
        g = torch.Generator().manual_seed(31 + n)
        act = torch.randn(3, n, d, generator=g).to(ops.op16()).cuda()
        grad = (torch.randn(3, n, d, generator=g) * torch.tensor([1.0, 25.0, 0.04]).view(3, 1, 1)).cuda()      # the volumes' ranges differ
        cam, mm = ops.gradcam_reduce_per_volume(act, grad)
        whole, _ = ops.gradcam_reduce(act, grad)
        assert cam.shape == (3, n - 1) and mm.shape == (3, 2) and torch.isfinite(cam).all()
        for b in range(3):
            alone, mm1 = ops.gradcam_reduce(act[b:b + 1].contiguous(), grad[b:b + 1].contiguous())
            assert torch.equal(cam[b], alone[0]), (fmt, n, b)                 # bit for bit
            assert torch.equal(mm[b], mm1)
            assert float(cam[b].max()) > 0.999 and float(cam[b].min()) == 0.0
        # why the entry point exists: normalised over the whole batch, the small-range volumes are squeezed towards zero
        assert not torch.equal(cam, whole)
        assert float(whole[2].max()) < 0.1 and float(cam[2].max()) > 0.999
        again, _ = ops.gradcam_reduce_per_volume(act, grad)                   # the tickets reset: a second call gives the same bits
        assert torch.equal(again, cam)
    finally:
        _cabi.set_operand_format(before)


# ---------------------------------------------------------------------------------------------------------------- module

def make_neuro(S, p, seed=61, frozen=False):
    from neurovit_amd.NeuroEncoder import NeuroEncoder
    torch.manual_seed(seed)
    model = NeuroEncoder(W.neuro_config(S, p, DEVICE="cuda:0", **MICRO_SIZE)).eval()
    return model.requires_grad_(False) if frozen else model


def vit_view(x):
    return x.permute(0, 3, 1, 2).unsqueeze(1)


@pytest.mark.parametrize("S,p", [(32, 8), (27, 9)])
@pytest.mark.parametrize("method", METHODS)
def test_module_batch_against_restatement(S, p, method):
    from neurovit_amd import ops
    model = make_neuro(S, p)
    vit = model.volume_encoder.vit3d
    G = S // p
    keep = model.config["GRADCAM_THRESHOLD"]
    x = W.make_volume((3, S, S, S), 62).cuda()
    vols, cls, maps = model.attribution_volumes(x, method=method, return_token_maps=True)
    assert vols.shape == (3, S, S, S) and vols.is_cuda and vols.dtype == torch.float32 and cls.shape == (3,) and cls.is_cuda
    assert maps.shape == (3, G ** 3) and maps.is_cuda
    assert len(model.attribution_volumes(x, method=method)) == 2
    # the volumes are the restatement of the returned maps: the same call on the maps gives the same bits and exposes the kept set
    again, (norm, sparse, cuts) = ops.token_maps_to_volumes(maps.clone(), G, S, normalize=False, keep_percent=keep, return_maps=True)
    assert torch.equal(again, vols)
    check_against_restatement(f"module {method} S{S}", (vols.cpu(), norm.cpu(), sparse.cpu(), cuts.cpu()), maps.cpu(), (G,) * 3, (S,) * 3, keep)
    assert torch.equal(model.token_maps_to_volumes(maps, normalize=False), vols)
    if method != "gradcam":
        if method == "rollout":
            with torch.no_grad():
                logits, raw = vit.attention_rollout(vit_view(x))
        else:
            logits, raw = vit.attention_relevance(vit_view(x))
        assert raw.shape == maps.shape
        assert torch.equal(maps.cpu(), minmax_reciprocal(raw.cpu()))           # normalised per volume, bit for bit
        assert torch.equal(model.token_maps_to_volumes(raw), vols)             # the public building block on the raw maps
        assert torch.equal(cls, logits.argmax(dim=1))
    # every volume is normalised on its own: min 0, max = r / (r + 1e-8) of ITS raw range r (an untrained model's Grad-CAM has r ~ 1e-7)
    assert (maps.amin(dim=1) == 0).all() and (maps.amax(dim=1) > 0).all() and float(maps.max()) <= 1.0


def single_volume_token_map(model, method, x1, target=None):
    """(volume, class, normalised token map) of the single-volume method, the map recomputed as the method forms it"""
    from neurovit_amd import ops
    vit = model.volume_encoder.vit3d
    if method == "gradcam":
        cam, cls = model.get_attention_map(x1)
        t = ops.gradcam_reduce(vit.last_attn_norm_output_raw(), vit.last_attn_norm_grad_raw())[0].cpu()
    elif method == "rollout":
        cam, cls = model.get_attention_rollout(x1)
        with torch.no_grad():
            t = minmax_division(vit.attention_rollout(vit_view(x1))[1].cpu())
    else:
        cam, cls = model.get_attention_relevance(x1, target=target)
        t = minmax_division(vit.attention_relevance(vit_view(x1), target=target)[1].cpu())
    assert torch.equal(cam, model._token_map_to_volume(t))                      # t is the map the method thresholded
    return cam, cls, t


@pytest.mark.parametrize("S,p", [(32, 8), (27, 9)])
@pytest.mark.parametrize("method", METHODS)
def test_module_single_volume_against_the_existing_methods(S, p, method):
    model = make_neuro(S, p)
    keep = model.config["GRADCAM_THRESHOLD"]
    x1 = W.make_volume((1, S, S, S), 63).cuda()
    cam, cls1, t = single_volume_token_map(model, method, x1)
    vols, cls, maps = model.attribution_volumes(x1, method=method, return_token_maps=True)
    assert torch.equal(cls.cpu(), cls1.cpu())
    kept_single = t[0] >= torch.quantile(t.double().flatten(), 1.0 - keep / 100.0).to(torch.float32)
    kept_batched = maps[0].cpu() >= quantile_cut(maps[0].cpu(), keep)
    err = float((vols[0].cpu() - cam).abs().max())
    report(f"attribution_volumes {method} S{S} B=1 vs the single-volume method: kept-set mismatches {int((kept_single != kept_batched).sum())}, "
           f"token map max |diff| {float((maps.cpu() - t).abs().max()):.2e}, volume max |err| {err:.2e}")
    assert torch.equal(kept_single, kept_batched)
    assert err <= VOLUME_TOL, err


def test_module_targets_and_frozen_model():
    S = 32
    model = make_neuro(S, 8, frozen=True)
    x = W.make_volume((3, S, S, S), 64).cuda()
    for method in METHODS:
        base, predicted = model.attribution_volumes(x, method=method)
        other = 1 - predicted
        as_tensor, cls_t = model.attribution_volumes(x, method=method, target=other)
        assert torch.equal(cls_t, predicted if method == "rollout" else other)
        as_one, cls_1 = model.attribution_volumes(x, method=method, target=1)
        as_zero, cls_0 = model.attribution_volumes(x, method=method, target=0)
        assert torch.equal(cls_1, predicted if method == "rollout" else torch.ones_like(predicted))
        assert torch.equal(cls_0, predicted if method == "rollout" else torch.zeros_like(predicted))
        if method == "rollout":
            assert torch.equal(as_tensor, base) and torch.equal(as_one, base) and torch.equal(as_zero, base)
        else:
            # volumes do not couple: row b is the map of ITS class, whatever the other rows explain
            assert not torch.equal(as_one, as_zero)
            assert torch.equal(as_tensor, torch.where((other == 1).view(3, 1, 1, 1), as_one, as_zero))
            assert torch.equal(base, torch.where((predicted == 1).view(3, 1, 1, 1), as_one, as_zero))
        assert all(q.grad is None for q in model.parameters()), method
    assert model.volume_encoder.vit3d._grads is None                             # no parameter-sized gradient arena either
    assert x.grad is None and not x.requires_grad
    # threshold: an explicit percentage overrides GRADCAM_THRESHOLD
    wide, _ = model.attribution_volumes(x, method="rollout", threshold=100)
    narrow, _ = model.attribution_volumes(x, method="rollout")
    assert int((wide > 0).sum()) > int((narrow > 0).sum())


def test_refusals(tmp_path):
    from neurovit_amd import ops
    from neurovit_amd.NeuroEncoder import NeuroEncoder
    S = 16
    m3 = NeuroEncoder(W.neuro_config(S, 8, dim=3, **MICRO_SIZE))
    torch.save(m3.state_dict(), tmp_path / "c.pth")
    model = NeuroEncoder(W.neuro_config(S, 8, dim=4, DEVICE="cuda:0", GLOBAL_BASE_PATH=str(tmp_path), BEST_MODEL_PATH="c.pth", **MICRO_SIZE))
    with pytest.raises(NotImplementedError, match="3D model only"):
        model.attribution_volumes(W.make_volume((1, S, S, S), 65).cuda())
    with pytest.raises(ValueError, match="method"):
        make_neuro(32, 8).attribution_volumes(W.make_volume((1, 32, 32, 32), 65).cuda(), method="lime")
    with pytest.raises(RuntimeError, match="at most 4096"):                       # one plane more than ViT3D-large's 16^3 grid
        ops.token_maps_to_volumes(torch.zeros(1, 17 * 16 * 16, device="cuda"), (17, 16, 16), 128)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.token_maps_to_volumes(torch.zeros(1, 64), 4, 32)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.gradcam_reduce_per_volume(torch.zeros(1, 9, 8, dtype=ops.op16()), torch.zeros(1, 9, 8))
