"""Path attribution on MI355X: the kernels of csrc/path_attr.hip against their CPU restatements (tests/path_attribution_ref.py), and
ViT.integrated_gradients / NeuroEncoder.integrated_gradients against the autograd loop of tests/test_input_grad_gpu.py and the oracles.

Gates:
  nv_path_points, nv_path_accumulate, nv_path_finish   bit-equal to the restatements (the same separately rounded fp32 operations; NaN at
                 the same positions) at V = 16^3 (every row 16-byte aligned) and 27^3 (every row start unaligned);
  nv_class_score_grads   logit: exactly the one-hot; prob: within 2e-6 absolute of float64 autograd of the softmax (nv_class_scores' bound);
  nv_attr_token_sums     |got - float64 restatement| <= P 2^-53 sum|.| (P voxels per patch: the double accumulation in another order) + 2^-24 |sum|
                 (the fp32 store); two runs bit-identical;
  end to end     W.MICRO, weights seed 51, input seed 52, class 1, zero baseline, riemann_middle, 16 steps, chunk 16, frozen model:
                 (a) against the autograd loop on the same model every element within 16 2^-23 sum_k |w_k g_k x| (both run the same
                 16-volume forward and backward; only the order of the fp32 sum over the steps differs); (b) three_way (GRAD_REL, RATIO,
                 SLACK) against the restated method on the emulating and the fp32 oracle; (c) |delta| <= RATIO |delta of the fp32 oracle
                 at the same rule| + SLACK; (d) the same with score "prob" and a per-volume tensor baseline on B = 2;
  side effects   a trainable model under no_grad: no p.grad, no gradient arena, parameters bit-unchanged, no backward hook fires;
  chunking       chunk 16 against chunk 5 within GRAD_REL (the batch composition changes the GEMM plan), one chunk size twice bit-identical.
Measured errors go to the parity report of test_engine_gpu.report.
"""
import pytest
import torch

import path_attribution_ref as R
import weights as W
from conftest import rel_l2
from oracle import ref_cpu
from test_engine_gpu import GRAD_REL, RATIO, SLACK, report
from test_input_grad_gpu import make_input, make_model, oracle_cfg, three_way

pytestmark = pytest.mark.gpu
MICRO_SIZE = dict(TRAINING_VIT_DIM=128, TRAINING_VIT_DEPTH=2, TRAINING_VIT_HEADS=2, TRAINING_VIT_MLP_DIM=256)
VOLUMES = {"aligned": 16 ** 3, "unaligned": 27 ** 3}
NAN = float("nan")


@pytest.fixture(scope="module", autouse=True)
def gpu():
    from neurovit_amd._cabi import require_gpu
    require_gpu()


def same_bits(got, want):
    """equal bit patterns wherever the value is a number, NaN at the same positions (the payload of a NaN is the processor's own)"""
    got, want = got.cpu(), want.cpu()
    nan = torch.isnan(want)
    return torch.equal(torch.isnan(got), nan) and torch.equal(got.view(torch.int32)[~nan], want.view(torch.int32)[~nan])


def baselines(B, V, g):
    return {"scalar": 0.25, "shared": torch.randn(1, V, generator=g), "per_volume": torch.randn(B, V, generator=g)}


def on_device(baseline):
    return baseline.cuda() if torch.is_tensor(baseline) else baseline


# ------------------------------------------------------------------ 1. kernels
@pytest.mark.parametrize("bad", ["b", "k"])
@pytest.mark.parametrize("kind", ["scalar", "shared", "per_volume"])
@pytest.mark.parametrize("vol", sorted(VOLUMES))
def test_path_points_bit_equal(vol, kind, bad):
    from neurovit_amd import ops
    B, V, K = 3, VOLUMES[vol], 4
    g = torch.Generator().manual_seed(V + len(kind))
    x = torch.randn(B, V, generator=g)
    baseline = baselines(B, V, g)[kind]
    x[0, 5], x[1, 7], x[2, 9], x[0, V - 1] = NAN, float("inf"), float("-inf"), float("inf")
    if torch.is_tensor(baseline):
        baseline[0, 7] = float("inf")                     # inf - inf at (1, 7) for the shared baseline
        baseline[-1, 11] = NAN
    alphas = torch.tensor([0.0, 0.3, 0.625, 1.0])
    # J = 7: mixed volumes, runs of one, two and three jobs of a volume, no multiple of the group, one job out of range
    jobs = torch.tensor([[0, 0], [0, 1], [0, 3], [2, 1], [B + 2, 0] if bad == "b" else [1, K], [1, 2], [1, 3]], dtype=torch.int32)
    prefill = torch.full((7, V), NAN)
    want = R.path_points_ref(x, jobs, alphas, baseline, out=prefill)
    got = ops.path_points(x.cuda(), jobs.cuda(), alphas.cuda(), on_device(baseline), out=prefill.cuda())
    assert same_bits(got, want)
    assert torch.isnan(got[4].cpu()).all()               # the job out of range left its row as it was


@pytest.mark.parametrize("C", [2, 5, 64, 65, 130])              # 65 and 130: the lane-strided loops take a second and a third turn
def test_class_score_grads(C):
    from neurovit_amd import ops
    B, J = 3, 9
    g = torch.Generator().manual_seed(C)
    logits = 3 * torch.randn(J, C, generator=g)
    jobs = torch.stack([torch.tensor([0, 0, 0, 1, 1, 2, 2, 2, 1]), torch.arange(J)], 1).to(torch.int32)
    cls = torch.tensor([1, 0, C - 1])
    onehot = torch.nn.functional.one_hot(cls[jobs[:, 0].long()], C).float()
    got = ops.class_score_grads(logits.cuda(), jobs.cuda(), cls.cuda(), kind="logit").cpu()
    assert torch.equal(got, onehot) and torch.equal(got, R.class_score_grads_ref(logits, jobs, cls, "logit"))
    l64 = logits.double().requires_grad_(True)
    (want,) = torch.autograd.grad((torch.softmax(l64, 1) * onehot.double()).sum(), l64)
    got = ops.class_score_grads(logits.cuda(), jobs.cuda(), cls.cuda(), kind="prob").cpu()
    err = (got.double() - want).abs().max().item()
    report(f"nv_class_score_grads C = {C}: max abs error vs float64 autograd {err:.3e}")
    assert err <= 2e-6, err
    assert (R.class_score_grads_ref(logits, jobs, cls, "prob").double() - want).abs().max().item() <= 2e-6
    # one softmax for the score and its gradient: d p_c / d l_c = p_c (1 - p_c) with the p_c of nv_class_scores, bit for bit
    jobs3 = torch.cat([jobs[:, :1], torch.zeros(J, 2, dtype=torch.int32)], 1)
    s = ops.class_scores(logits.cuda(), jobs3.cuda(), cls.cuda(), "prob").cpu()
    own = got[torch.arange(J), cls[jobs[:, 0].long()]]
    assert same_bits(own, s * (1 - s))
    bad = torch.tensor([1, C, -1])                          # volumes 1 and 2: a class outside [0, C)
    for kind in ("logit", "prob"):
        got = ops.class_score_grads(logits.cuda(), jobs.cuda(), bad.cuda(), kind=kind).cpu()
        rows = jobs[:, 0] > 0
        assert torch.isnan(got[rows]).all() and torch.isfinite(got[~rows]).all()
    with pytest.raises(ValueError):
        ops.class_score_grads(logits.cuda(), jobs.cuda(), cls.cuda(), kind="margin")


@pytest.mark.parametrize("vol", sorted(VOLUMES))
def test_path_accumulate_and_finish_bit_equal(vol):
    from neurovit_amd import ops
    B, V, K = 3, VOLUMES[vol], 4
    g = torch.Generator().manual_seed(V)
    weights = torch.tensor([0.125, 0.4, 0.3, 0.175])
    jobs = torch.stack([torch.arange(B).repeat_interleave(K), torch.arange(K).repeat(B)], 1).to(torch.int32)
    acc = torch.randn(B, V, generator=g)                     # (not zero: a volume absent from a call must keep these bits)
    acc_d = acc.cuda()
    for first in range(0, B * K, 5):                         # chunks of 5 jobs straddle the volume boundaries at 4 and 8
        part = jobs[first:first + 5]
        grads = torch.randn(part.shape[0], V, generator=g)
        before = acc_d.clone()
        want = R.path_accumulate_ref(grads, part, weights, acc)
        ops.path_accumulate(grads.cuda(), part.cuda(), weights.cuda(), acc_d)
        assert torch.equal(acc_d.cpu().view(torch.int32), want.view(torch.int32)), first
        absent = [b for b in range(B) if b not in part[:, 0].tolist()]
        assert absent
        for b in absent:
            assert torch.equal(acc_d[b], before[b])
        acc = want
    # a job with k out of range adds nothing
    odd = torch.tensor([[1, K], [B, 0], [2, -1]], dtype=torch.int32)
    before = acc_d.clone()
    ops.path_accumulate(torch.randn(3, V, generator=g).cuda(), odd.cuda(), weights.cuda(), acc_d)
    assert torch.equal(acc_d, before)
    x = torch.randn(B, V, generator=g)
    for kind, baseline in baselines(B, V, g).items():
        want = R.path_finish_ref(acc, x, baseline)
        got = ops.path_finish(acc_d, x.cuda(), on_device(baseline))
        assert torch.equal(got.cpu().view(torch.int32), want.view(torch.int32)), kind


@pytest.mark.parametrize("S,p", [(16, 8), (27, 9)])
def test_attr_token_sums(S, p):
    from neurovit_amd import ops
    g = torch.Generator().manual_seed(S)
    attr = torch.randn(3, S, S, S, generator=g) * torch.rand(3, S, S, S, generator=g).pow(4)      # magnitudes spread over decades
    want = R.token_sums_ref(attr, p)
    got = ops.attr_token_sums(attr.cuda(), p)
    again = ops.attr_token_sums(attr.cuda(), p)
    assert got.shape == (3, (S // p) ** 3, 2) and torch.equal(got, again)
    err = (got.cpu().double() - want).abs()
    bound = p ** 3 * 2.0 ** -53 * want[..., 1:] + 2.0 ** -24 * want.abs()
    report(f"nv_attr_token_sums {S}^3 / p{p}: max error / bound {(err / bound).max().item():.3f}")
    assert (err <= bound).all()
    assert (got[..., 1] >= got[..., 0].abs()).all()


# ------------------------------------------------------------------ 2. end to end, tied to the gate that already holds
STEPS, CLASS = 16, 1


def device_view(video_cpu):
    """the tensor on the device with the strides it has on the CPU (the permute view ViT3DEncoder.forward makes)"""
    x = torch.empty_strided(video_cpu.shape, video_cpu.stride(), device="cuda")
    x.copy_(video_cpu)
    return x


@pytest.fixture(scope="module")
def micro():
    model = make_model(W.MICRO, 51).requires_grad_(False)
    sd = W.make_tensors(W.vit_param_spec(**W.MICRO), 51)
    return model, sd, oracle_cfg(W.MICRO)


def oracle_runs(sd, ocfg, video, cls, alphas, weights, baseline, score):
    """(attributions, |delta|) of the restated method on the emulating and on the fp32 oracle"""
    out = []
    for emulate in (True, False):
        attr, delta, _, _ = R.integrated_gradients_ref(lambda v: ref_cpu.vit_forward(sd, ocfg, v, emulate_bf16=emulate), video, cls, alphas, weights,
                                                       baseline=baseline, score=score)
        out.append((attr, delta.abs()))
    return out


def test_integrated_gradients_against_the_autograd_loop_and_the_oracles(micro):
    from neurovit_amd.NeuroEncoder import path_quadrature
    model, sd, ocfg = micro
    video = make_input(W.MICRO, 1, 52).contiguous()
    x = video.cuda()
    out = model.integrated_gradients(x, target=CLASS, baseline=0.0, steps=STEPS, method="riemann_middle", score="logit", chunk=16)
    attr = out["attributions"]
    assert attr.shape == x.shape and attr.stride() == x.stride() and out["class_idx"].tolist() == [CLASS]
    alphas, weights = path_quadrature("riemann_middle", STEPS)
    assert torch.equal(out["alphas"].cpu(), alphas) and torch.equal(out["weights"].cpu(), weights)

    # (a) the loop of test_autograd_grad_and_integrated_gradients on the same model
    path = (alphas.view(-1, 1, 1, 1, 1).cuda() * x).requires_grad_(True)
    (g,) = torch.autograd.grad(model(path)[:, CLASS].sum(), path)
    loop = x[0] * g.mean(0)
    bound = 16 * 2.0 ** -23 * (weights.view(-1, 1, 1, 1, 1).cuda() * g * x).abs().sum(0)
    worst = ((attr[0] - loop).abs() / bound.clamp_min(1e-38)).max().item()
    report(f"integrated gradients native vs autograd loop: max error / bound {worst:.3e}")
    assert ((attr[0] - loop).abs() <= bound).all(), worst

    # (b), (c) the restated method on the oracles
    (emu, _), (f32, delta32) = oracle_runs(sd, ocfg, video, torch.tensor([CLASS]), alphas, weights, 0.0, "logit")
    three_way("integrated-gradients native", attr.cpu(), emu, f32)
    delta = out["delta"].abs().cpu()
    want = attr.double().sum().cpu() - (out["score_input"].double() - out["score_baseline"].double()).cpu()
    assert out["delta"].dtype == torch.float64 and torch.allclose(out["delta"].cpu(), want, rtol=0, atol=1e-9)
    report(f"integrated gradients native completeness (riemann_middle {STEPS}): |delta| {delta.item():.3e}  fp32 oracle {delta32.item():.3e}")
    assert delta.item() <= RATIO * delta32.item() + SLACK, (delta, delta32)


def test_integrated_gradients_prob_score_and_tensor_baseline(micro):
    from neurovit_amd.NeuroEncoder import path_quadrature
    model, sd, ocfg = micro
    video = make_input(W.MICRO, 2, 52)                       # the [B, H, W, D] -> [B, 1, D, H, W] permute view
    baseline = 0.25 * make_input(W.MICRO, 2, 53)
    x, bl = device_view(video), device_view(baseline)
    assert not x.is_contiguous()
    out = model.integrated_gradients(x, target=CLASS, baseline=bl, steps=STEPS, method="riemann_middle", score="prob", chunk=16)
    attr = out["attributions"]
    assert attr.shape == x.shape and attr.stride() == x.stride()
    alphas, weights = path_quadrature("riemann_middle", STEPS)
    (emu, _), (f32, delta32) = oracle_runs(sd, ocfg, video, torch.tensor([CLASS, CLASS]), alphas, weights, baseline, "prob")
    three_way("integrated-gradients native prob / tensor baseline", attr.cpu(), emu, f32)
    delta = out["delta"].abs().cpu()
    report(f"integrated gradients native completeness (prob, tensor baseline): |delta| {delta.tolist()}  fp32 oracle {delta32.tolist()}")
    assert (delta <= RATIO * delta32 + SLACK).all(), (delta, delta32)
    # target None: the arg-max class of the input
    with torch.no_grad():
        predicted = model(x).argmax(dim=1)
    again = model.integrated_gradients(x, baseline=bl, steps=4, method="gausslegendre")
    assert torch.equal(again["class_idx"], predicted)


def test_integrated_gradients_has_no_side_effects():
    model = make_model(W.MICRO, 51)                          # trainable, train mode (no dropout)
    x = make_input(W.MICRO, 1, 52).contiguous().cuda()
    fired = []
    handles = [attn.attend.register_full_backward_hook(lambda m, gi, go: fired.append(1)) for attn, _ in model.transformer.layers]
    with torch.no_grad():
        model(x)
        before = [p.detach().clone() for p in model.parameters()]
        out = model.integrated_gradients(x, target=CLASS, steps=4, method="riemann_middle")
    torch.cuda.synchronize()
    for h in handles:
        h.remove()
    assert torch.isfinite(out["attributions"]).all() and out["attributions"].abs().sum().item() > 0
    assert all(p.grad is None for p in model.parameters()) and model._grads is None
    assert all(torch.equal(a, p.detach()) for a, p in zip(before, model.parameters()))
    assert not fired
    assert not out["attributions"].requires_grad


def test_integrated_gradients_chunking(micro):
    model, _, _ = micro
    x = device_view(make_input(W.MICRO, 2, 52))
    kwargs = dict(target=CLASS, steps=STEPS, method="riemann_middle")
    whole = model.integrated_gradients(x, chunk=16, **kwargs)["attributions"]
    fives = model.integrated_gradients(x, chunk=5, **kwargs)["attributions"]
    err = rel_l2(fives, whole)
    report(f"integrated gradients chunk 5 vs chunk 16: rel L2 {err:.3e}")
    assert err <= GRAD_REL, err
    assert torch.equal(model.integrated_gradients(x, chunk=5, **kwargs)["attributions"], fives)
    assert torch.equal(model.integrated_gradients(x, chunk=16, **kwargs)["attributions"], whole)


def test_integrated_gradients_refusals(micro):
    model, _, _ = micro
    x = make_input(W.MICRO, 2, 52).contiguous().cuda()
    with pytest.raises(ValueError, match="dense"):
        model.integrated_gradients(torch.cat([x, x])[::2])                     # every other volume of a batch: not dense
    with pytest.raises(NotImplementedError, match="time_points"):
        model.integrated_gradients(x, time_points=4)
    with pytest.raises(NotImplementedError, match="RAW"):
        model.integrated_gradients(x, vol_sigma=torch.ones(2, device="cuda"))
    with pytest.raises(ValueError):
        model.integrated_gradients(x, target=2)


# ------------------------------------------------------------------ 3. NeuroEncoder
def test_neuro_encoder_integrated_gradients_and_its_consumers(tmp_path):
    from neurovit_amd import ops
    from neurovit_amd.NeuroEncoder import NeuroEncoder
    S, p = 32, 8
    model = NeuroEncoder(W.neuro_config(S, p, DEVICE="cuda:0", **MICRO_SIZE))
    model.load_state_dict(W.make_tensors(W.vit_param_spec(**W.MICRO), 51, prefix="volume_encoder.vit3d."), strict=True)
    model.eval()
    x = W.make_volume((2, S, S, S), 52).cuda()
    out = model.integrated_gradients(x, steps=8, method="riemann_middle", baseline=torch.zeros(1, S, S, S))
    attr, maps = out["attributions"], out["token_maps"]
    assert attr.shape == (2, S, S, S) and attr.is_contiguous() and maps.shape == out["token_abs"].shape == (2, (S // p) ** 3)
    want = R.token_sums_ref(attr.cpu(), p)
    bound = p ** 3 * 2.0 ** -53 * want[..., 1:] + 2.0 ** -24 * want.abs()
    got = torch.stack([maps, out["token_abs"]], -1).cpu().double()
    assert ((got - want).abs() <= bound).all()
    delta = maps.double().sum(1) - (out["score_input"].double() - out["score_baseline"].double())
    assert torch.equal(out["delta"], delta)
    # the ViT-level call on ViT3DEncoder.forward's view gives the same attributions
    vit = model.volume_encoder.vit3d
    direct = vit.integrated_gradients(x.permute(0, 3, 1, 2).unsqueeze(1), steps=8, method="riemann_middle")
    assert torch.equal(direct["attributions"].squeeze(1).permute(0, 2, 3, 1), attr) and torch.equal(direct["class_idx"], out["class_idx"])

    volumes, class_idx, normalised = model.attribution_volumes(x, method="integrated_gradients", return_token_maps=True)
    full = model.integrated_gradients(x)
    want_volumes, (want_maps, _, _) = ops.token_maps_to_volumes(
        torch.relu(full["token_maps"]), S // p, S, normalize=True, keep_percent=model.config["GRADCAM_THRESHOLD"], return_maps=True)
    assert torch.equal(volumes, want_volumes) and torch.equal(normalised, want_maps) and torch.equal(class_idx, full["class_idx"])
    assert torch.equal(model.attribution_volumes(x, method="integrated_gradients")[0], volumes)

    curves = model.perturbation_curves(x, maps, steps=4)
    assert all(torch.isfinite(curves[k]).all() for k in ("deletion", "insertion", "deletion_auc", "insertion_auc"))

    for kwargs in (dict(method="simpson"), dict(steps=0), dict(chunk=0)):
        with pytest.raises(ValueError):
            model.integrated_gradients(x, **kwargs)
    torch.save(model.state_dict(), tmp_path / "c.pth")
    four_d = NeuroEncoder(W.neuro_config(S, p, dim=4, DEVICE="cuda:0", GLOBAL_BASE_PATH=str(tmp_path), BEST_MODEL_PATH="c.pth", **MICRO_SIZE))
    with pytest.raises(NotImplementedError, match="3D model only"):
        four_d.integrated_gradients(x)
