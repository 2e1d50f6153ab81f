"""Masked-volume pretraining on MI355X: nv_mim_labels, nv_recon_loss, nv_vit_backward_tokens, ViT.forward_tokens and MaskedPretrainStep.

  labels        bit-equal to tests/mim_ref.py (pure integer Python), mask units of 1 and 2 patches;
  dpred         every masked cell within ONE code of the operand format of the float64 restatement's value, every other cell exactly zero,
                the cells behind the buffer untouched; for L1 only cells whose |pred - target| exceeds 2^-20 max(|pred|, |target|) are
                held to the value (the sign of a difference below fp32 resolution is not decided; the inputs leave < 1 % of them out);
  loss          within 1e-6 relative of the float64 sum;
  tokens        nv_vit_backward_tokens fed the residual gradient an ordinary backward's stage 0 left: every gradient of the later stages
                and the input gradient bit-equal to that ordinary backward, with dropout 0 and 0.1, full and data-only;
  whole models  three-way against the oracle's fp32 and 16-bit-emulating forms, err(HIP, fp32) <= 1.5 err(emulation, fp32) + 2e-4 (the
                gate of tests/test_engine_gpu.py), for a torch loss on ViT.forward_tokens and for one whole pretraining step;
  the loop      mlp_head bit-unchanged, two runs from one seed bit-equal, a run resumed after two of four steps bit-equal to the straight
                one, the validation loss falls on synthetic volumes, the encoder is adopted by a fresh NeuroEncoder, fp16 operands, and
                the Trainer shell under TRAINING_OBJECTIVE "mim".

Geometries: S = 16, p = 4 (N = 64, P = 64: 16-byte runs) and S = 12, p = 3 (P = 27 -> 32 columns: pad columns, 12-byte runs); depth 2,
dim 64, one head of 64; B = 3.  The volumes' voxel values encode their flat index (floor(value) = index), so any permutation of patch
or element order shows."""
import math

import pytest
import torch

import mim_ref as R
import weights as W
from conftest import rel_l2, report
from oracle import ref_cpu

pytestmark = pytest.mark.gpu

GEOMS = {"s16p4": (16, 4), "s12p3": (12, 3)}
B = 3
RATIO, SLACK = 1.5, 2e-4
DT16 = {"bf16": torch.bfloat16, "fp16": torch.float16}
SIG_BITS = {"bf16": 7, "fp16": 10}          # stored significand bits
MIN_EXP = {"bf16": -126, "fp16": -14}       # exponent of the smallest normal


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    from neurovit_amd._cabi import require_gpu, set_operand_format
    require_gpu()
    yield
    set_operand_format("bf16")


def index_volume(S, seed=0):
    """[B, S, S, S] fp32 whose floor is the voxel's flat index over the batch; the fraction (below 0.5) makes every patch's statistics its own"""
    n = B * S ** 3
    frac = torch.rand(n, generator=torch.Generator().manual_seed(seed)) * 0.5
    return (torch.arange(n, dtype=torch.float32) + frac).reshape(B, S, S, S)


def code_of(v, fmt):
    """the spacing of the operand format's codes at |v| (float64 tensor)"""
    e = torch.floor(torch.log2(v.abs().clamp_min(1e-300))).clamp_min(MIN_EXP[fmt])
    return torch.pow(torch.tensor(2.0, dtype=torch.float64), e - SIG_BITS[fmt])


# ------------------------------------------------------------------------------------------------ nv_mim_labels
@pytest.mark.parametrize("unit", [1, 2])
def test_labels_bit_equal_to_the_restatement(unit):
    from neurovit_amd import ops
    grid = (4, 4, 4)
    for seed, step, rank in ((0, 0, 0), (1234567, 3, 1), (2 ** 63 + 5, 2 ** 33 + 1, 7)):
        got = ops.mim_labels(B, grid, unit, seed, step, rank).cpu()
        want = R.labels_ref(B, grid, unit, seed, step, rank)
        assert torch.equal(got, want), (unit, seed, step, rank)
        assert all(sorted(row.tolist()) == list(range(64)) for row in got)
    assert ops.mim_masked_count(grid, unit, 0.6) == R.masked_count(grid, unit, 0.6) == (38 if unit == 1 else 40)


def test_labels_with_mask_patches_write_the_masked_batch():
    from neurovit_amd import ops
    S, p = 16, 4
    x = index_volume(S)
    labels = ops.mim_labels(B, (4, 4, 4), 2, 11, 5)
    m = ops.mim_masked_count((4, 4, 4), 2, 0.5)
    jobs = torch.tensor([[b, 0, m] for b in range(B)], dtype=torch.int32, device="cuda")
    got = ops.mask_patches(x.cuda(), labels, jobs, p, -1.0).cpu()
    patches, masked = R.patches_of(got, (p,) * 3), labels.cpu() < m
    assert masked.sum(dim=1).tolist() == [m] * B
    assert (patches[masked] == -1.0).all() and torch.equal(patches[~masked], R.patches_of(x, (p,) * 3)[~masked])


# ------------------------------------------------------------------------------------------------ nv_recon_loss
@pytest.mark.parametrize("fmt", ["bf16", "fp16"])
@pytest.mark.parametrize("geom", list(GEOMS))
def test_recon_loss_and_dpred(geom, fmt):
    from neurovit_amd import _cabi, ops
    _cabi.set_operand_format(fmt)
    S, p = GEOMS[geom]
    G = S // p
    N, P = G ** 3, p ** 3
    P8 = (P + 7) // 8 * 8
    rows = B * (N + 1)
    x = index_volume(S, seed=1)
    labels = R.labels_ref(B, (G,) * 3, 1, 42, 9)
    m = R.masked_count((G,) * 3, 1, 0.6)
    gen = torch.Generator().manual_seed(5)
    for kind in ("l1", "l2"):
        for norm_pix in (True, False):
            for loss_scale in (1.0, 1024.0):
                # predictions of the targets' own size, so that every term of the loss matters
                tgt = R.targets_ref(x, (p,) * 3, norm_pix)
                scale = float(tgt.abs().max())
                ldp, ldd = P8 + 4, P8 + 8                    # wider than the patch: columns the kernel must not read as data / must zero
                pred = torch.randn(rows, ldp, generator=gen) * scale
                want_loss, want_d, masked, diff = R.recon_ref(pred, x, labels, m, (p,) * 3, kind, norm_pix, loss_scale)
                buf = torch.full((rows + 2, ldd), 7.0, dtype=DT16[fmt], device="cuda")      # two guard rows behind the buffer
                loss, dpred, partials = ops.recon_loss(pred.cuda(), x.cuda(), labels.cuda(), m, p, kind, norm_pix, loss_scale, dpred=buf[:rows])
                tag = f"recon {geom} {fmt} {kind} norm_pix={norm_pix} scale={loss_scale:g}"
                got = buf.cpu().double()
                assert (got[rows:] == 7.0).all(), tag + ": guard cells written"
                assert (got[:rows, P:] == 0).all() and (got[:rows][~masked] == 0).all(), tag + ": cells outside the masked patches must be exact zeros"
                got_d, want_m = got[:rows, :P][masked], want_d[masked]
                held = torch.ones_like(want_m, dtype=torch.bool)
                if kind == "l1":
                    pm = pred.double()[:, :P][masked]
                    tm = pm - diff[masked]
                    held = diff[masked].abs() > 2.0 ** -20 * torch.maximum(pm.abs(), tm.abs())
                    assert (~held).double().mean().item() <= 0.01, tag
                off = ((got_d - want_m).abs() / code_of(want_m, fmt))[held].max().item()
                e_loss = abs(loss.item() - want_loss.item()) / abs(want_loss.item())
                e_part = abs(partials.sum().item() - want_loss.item()) / abs(want_loss.item())
                report(f"{tag}: dpred worst {off:.3f} codes, loss rel {e_loss:.2e} (double partials {e_part:.2e})")
                print(f"{tag}: dpred worst {off:.3f} codes, loss rel {e_loss:.2e} (double partials {e_part:.2e})")
                assert off <= 1.0, (tag, off)
                assert e_loss <= 1e-6 and e_part <= 1e-12, (tag, e_loss, e_part)
                assert (partials.cpu()[~masked] == 0).all()


def test_recon_loss_is_deterministic_and_reads_no_pred_on_other_rows():
    """NaN in pred on every row that is not masked (and in the pad columns of the masked ones) must not reach the loss or dpred"""
    from neurovit_amd import _cabi, ops
    _cabi.set_operand_format("bf16")
    S, p = 12, 3
    G, P = S // p, p ** 3
    x = index_volume(S, seed=2).cuda()
    labels = ops.mim_labels(B, (G,) * 3, 1, 3, 1)
    m = ops.mim_masked_count((G,) * 3, 1, 0.6)
    pred = torch.randn(B * (G ** 3 + 1), 32, device="cuda")
    a = ops.recon_loss(pred, x, labels, m, p, "l2", True)
    masked = torch.zeros(B, G ** 3 + 1, dtype=torch.bool, device="cuda")
    masked[:, 1:] = labels < m
    poisoned = pred.clone()
    poisoned[~masked.reshape(-1)] = float("nan")
    poisoned[:, P:] = float("nan")
    b = ops.recon_loss(poisoned, x, labels, m, p, "l2", True)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and torch.equal(a[2], b[2]) and torch.isfinite(a[0]).all()


# ------------------------------------------------------------------------------------------------ nv_vit_backward_tokens
CFG16 = dict(image_size=16, image_patch_size=4, frames=16, frame_patch_size=4, num_classes=2, dim=64, depth=2, heads=1, dim_head=64,
             mlp_dim=128, channels=1)


def make_vit(cfgdict, seed, dropout=0.0):
    from neurovit_amd.vit_3d import ViT
    torch.manual_seed(seed)
    vit = ViT(**cfgdict, dropout=dropout, emb_dropout=dropout).cuda()
    vit.flat_parameters()
    vit._refresh_shadow()
    return vit


@pytest.mark.parametrize("drop", [0.0, 0.1])
def test_backward_tokens_equals_the_ordinary_backward_behind_its_head(drop):
    vit = make_vit(CFG16, 3)
    rt, arena, shadow = vit._rt, vit._arena, vit._shadow
    S = CFG16["image_size"]
    video = ref_cpu.fmri_to_video(W.make_volume((B, S, S, S), 4).cuda())
    n, d = 65, 64
    dropout = (drop, drop, 987654321) if drop else (0.0, 0.0, 0)
    rt.forward(video, arena, shadow, training=True, dropout=dropout, rows_form=1)
    dlogits = torch.randn(B, 2, generator=torch.Generator().manual_seed(1)).cuda()
    rt.backward(dlogits, arena, shadow, torch.zeros_like(arena), accumulate=False, stages=(0, 0))
    g = rt.tap("g", -1, (B * n, d), torch.float32).clone()
    assert g.reshape(B, n, d)[:, 1:].abs().max().item() == 0 and g.abs().max().item() > 0
    want, want_dv = torch.full_like(arena, float("nan")), torch.empty_like(video)
    rt.backward(dlogits, arena, shadow, want, accumulate=False, dvideo=want_dv)
    got, got_dv = torch.full_like(arena, float("nan")), torch.empty_like(video)
    rt.backward(None, arena, shadow, got, accumulate=False, dvideo=got_dv, dtokens=g.reshape(B, n, d))
    hb, he = rt.stage_range(0, 0)
    # the last layer's FC2 bias gradient is what the seeding launch itself writes (the column sums of dtokens, in its own order): held to
    # fp32 rounding; everything the later stages write is bit-equal
    i = [k for k, _ in vit.named_parameters()].index("transformer.layers.1.1.net.4.bias")
    b0, b1 = vit._offsets[i], vit._offsets[i] + vit._numels[i]
    assert rel_l2(got[b0:b1], want[b0:b1]) < 1e-6
    got[b0:b1] = want[b0:b1]
    assert he == arena.numel() and torch.equal(got[:hb], want[:hb]) and torch.isfinite(got).all()
    assert (got[hb:] == 0).all() and want[hb:].nan_to_num().abs().max().item() > 0, "the head's range is written as zeros"      # (NaN: the arena's padding)
    assert torch.equal(got_dv, want_dv) and got_dv.abs().max().item() > 0
    # accumulate = 1 adds everywhere else and leaves the head's range alone
    acc = torch.ones_like(arena)
    rt.backward(None, arena, shadow, acc, accumulate=True, dtokens=g)
    assert (acc[hb:] == 1).all() and rel_l2(acc[:hb] - 1, want[:hb]) < 1e-5
    # data-only: no arena, the same input gradient
    only_dv = torch.empty_like(video)
    rt.backward(None, arena, shadow, None, accumulate=False, dvideo=only_dv, weight_grads=False, dtokens=g)
    assert torch.equal(only_dv, want_dv)


def test_backward_tokens_refusals():
    vit = make_vit(CFG16, 3)
    rt, arena, shadow = vit._rt, vit._arena, vit._shadow
    video = ref_cpu.fmri_to_video(W.make_volume((B, 16, 16, 16), 4).cuda())
    g = torch.zeros(B, 65, 64, device="cuda")
    rt.forward(video, arena, shadow, training=True, rows_form=2)
    with pytest.raises(ValueError, match="rows_form=1"):
        rt.backward(None, arena, shadow, torch.zeros_like(arena), accumulate=False, dtokens=g)
    rt.forward(video, arena, shadow, training=True, rows_form=1)
    with pytest.raises(ValueError, match="not both"):
        rt.backward(torch.zeros(B, 2, device="cuda"), arena, shadow, torch.zeros_like(arena), accumulate=False, dtokens=g)
    with pytest.raises(ValueError, match="expected a device tensor"):
        rt.backward(None, arena, shadow, torch.zeros_like(arena), accumulate=False, dtokens=g[:, :64])


# ------------------------------------------------------------------------------------------------ whole models, three-way
SIZE = dict(TRAINING_VIT_DIM=64, TRAINING_VIT_DEPTH=2, TRAINING_VIT_HEADS=1, TRAINING_VIT_MLP_DIM=128)
ENC = "volume_encoder.vit3d."


def make_model(S, p, seed, **extra):
    import neurovit_amd.NeuroEncoder as ne
    torch.manual_seed(seed)
    model = ne.NeuroEncoder(W.neuro_config(S, p, DEVICE="cuda:0", **dict(SIZE, **extra)))
    model.train()
    return model


def gate(tag, name, hip, emu, f32, fails):
    e_h32, e_e32 = rel_l2(hip, f32), rel_l2(emu, f32)
    report(f"{tag} {name}: hip-fp32 {e_h32:.3e}  emu-fp32 {e_e32:.3e}")
    if not e_h32 <= RATIO * e_e32 + SLACK:
        fails.append((name, e_h32, e_e32))


@pytest.mark.parametrize("geom", list(GEOMS))
def test_forward_tokens_under_autograd_three_way(geom):
    """a torch MSE on the tokens differentiates the native encoder: tokens and every encoder gradient against the oracle's own blocks"""
    S, p = GEOMS[geom]
    model = make_model(S, p, 11)
    vit = model.volume_encoder.vit3d
    x = W.make_volume((B, S, S, S), 12)
    n, d = (S // p) ** 3 + 1, 64
    target = torch.randn(B, n, d, generator=torch.Generator().manual_seed(13))
    tokens = vit.forward_tokens(ref_cpu.fmri_to_video(x.cuda()))
    assert tokens.shape == (B, n, d) and tokens.dtype == torch.float32 and tokens.requires_grad
    torch.nn.functional.mse_loss(tokens, target.cuda()).backward()
    sd = {k[len(ENC):]: v.detach().cpu() for k, v in model.state_dict().items()}
    ocfg = ref_cpu.neuro_cfg(dict(model.config, DEVICE="cpu"))

    def oracle(emulate):
        leaves = {k: v.clone().requires_grad_(True) for k, v in sd.items()}
        taps = {}
        ref_cpu.vit_forward(leaves, ocfg, ref_cpu.fmri_to_video(x), emulate_bf16=emulate, taps=taps)
        tok = taps[f"block{ocfg.depth - 1}"]
        names = [k for k in leaves if not k.startswith("mlp_head.")]
        grads = torch.autograd.grad(torch.nn.functional.mse_loss(tok, target), [leaves[k] for k in names])
        return tok.detach(), dict(zip(names, grads))
    (tok_e, g_e), (tok_32, g_32) = oracle(True), oracle(False)
    fails = []
    gate(f"forward_tokens {geom}", "tokens", tokens.detach(), tok_e, tok_32, fails)
    for name, q in vit.named_parameters():
        if name.startswith("mlp_head."):
            assert q.grad is not None and q.grad.abs().max().item() == 0, name       # the head takes no part: zeros
        else:
            gate(f"forward_tokens {geom}", "grad " + name, q.grad, g_e[name], g_32[name], fails)
    assert not fails, fails


@pytest.mark.parametrize("geom,kind,norm_pix,unit", [("s16p4", "l1", True, 2), ("s12p3", "l2", True, 1), ("s12p3", "l1", False, 1)])
def test_one_pretraining_step_three_way(geom, kind, norm_pix, unit):
    """loss, the encoder's gradient and the decoder's gradients of one whole step (bf16 path) against the restatement: the masked copy by
    tests/test_perturbation_cpu.py's mask_ref, the oracle's blocks, LayerNorm + Linear, the loss of tests/mim_ref.py's independent form"""
    from neurovit_amd import MaskedPretrainStep
    from test_perturbation_cpu import mask_ref
    S, p = GEOMS[geom]
    G, P = S // p, p ** 3
    model = make_model(S, p, 21)
    vit = model.volume_encoder.vit3d
    step = MaskedPretrainStep(model, mask_ratio=0.6, mask_unit=unit, fill=0.25, loss=kind, norm_pix=norm_pix, lr=0.0, seed=31)      # lr 0: the gradients stay to be read
    x = W.make_volume((B, S, S, S), 22) * 2 + 0.5
    sd = {k[len(ENC):]: v.detach().cpu().clone() for k, v in model.state_dict().items()}
    hd = {k: v.detach().cpu().clone() for k, v in step.head.state_dict().items()}
    loss = step(x.cuda())
    m = step.masked_patches
    labels = R.labels_ref(B, (G,) * 3, unit, 31, 0)
    assert torch.equal(step.last_labels.cpu(), labels) and m == R.masked_count((G,) * 3, unit, 0.6)
    jobs = torch.tensor([[b, 0, m] for b in range(B)], dtype=torch.int32)
    masked = mask_ref(x, labels, jobs, p, 0.25)
    ocfg = ref_cpu.neuro_cfg(dict(model.config, DEVICE="cpu"))

    def oracle(emulate):
        leaves = {k: v.clone().requires_grad_(True) for k, v in sd.items()}
        head = {k: v.clone().requires_grad_(True) for k, v in hd.items()}
        taps = {}
        ref_cpu.vit_forward(leaves, ocfg, ref_cpu.fmri_to_video(masked), emulate_bf16=emulate, taps=taps)
        tok = taps[f"block{ocfg.depth - 1}"]
        xn = torch.nn.functional.layer_norm(tok, (64,), head["norm.weight"], head["norm.bias"], ref_cpu.LN_EPS)
        w = head["proj.weight"]
        pred = torch.nn.functional.linear(ref_cpu._r(xn) if emulate else xn, ref_cpu._r(w) if emulate else w) + head["proj.bias"]
        if emulate:       # the cast point of the decoder's backward: dpred exists in the operand format only, and the bias gradient is ITS column sum
            pred = ref_cpu._RoundGrad.apply(pred)
        value = R.recon_loss_autograd(pred.reshape(B * (G ** 3 + 1), P), x, labels, m, (p,) * 3, kind, norm_pix)
        names = [k for k in leaves if not k.startswith("mlp_head.")]
        grads = torch.autograd.grad(value, [leaves[k] for k in names] + list(head.values()))
        return value.item(), torch.cat([g.reshape(-1) for g in grads[:len(names)]]), dict(zip(head, grads[len(names):]))
    (l_e, enc_e, dec_e), (l_32, enc_32, dec_32) = oracle(True), oracle(False)
    tag = f"pretrain step {geom} {kind} norm_pix={norm_pix} unit={unit}"
    e_h, e_e = abs(loss.item() - l_32) / abs(l_32), abs(l_e - l_32) / abs(l_32)
    report(f"{tag} loss {loss.item():.6f}: hip-fp32 {e_h:.3e}  emu-fp32 {e_e:.3e}")
    fails = [] if e_h <= RATIO * e_e + SLACK else [("loss", e_h, e_e)]
    enc_hip = torch.cat([q.grad.reshape(-1) for k, q in vit.named_parameters() if not k.startswith("mlp_head.")])
    gate(tag, "encoder gradient", enc_hip, enc_e, enc_32, fails)
    for k, q in step.head.named_parameters():
        gate(tag, "decoder " + k, q.grad, dec_e[k], dec_32[k], fails)
    assert not fails, fails
    # lr = 0 moved nothing; the pad rows of the decoder got zero gradients
    assert all(torch.equal(v.cpu(), sd[k[len(ENC):]]) for k, v in model.state_dict().items())
    if P % 8:
        gW, gb = step.head._views(step.head.flat_gradients())[2:]
        assert gW[P:].abs().max().item() == 0 and gb[P:].abs().max().item() == 0


# ------------------------------------------------------------------------------------------------ the step as a training loop
def run_steps(model, step, xs):
    return [step(x).clone() for x in xs]


def volumes(S, count, seed):
    return [(W.make_volume((B, S, S, S), seed + i) * 1.5).cuda() for i in range(count)]


def test_mlp_head_stays_bit_unchanged_and_everything_else_moves():
    from neurovit_amd import MaskedPretrainStep
    model = make_model(12, 3, 41, TRAINING_DROPOUT=0.1)
    vit = model.volume_encoder.vit3d
    before = {k: v.detach().clone() for k, v in vit.state_dict().items()}
    step = MaskedPretrainStep(model, lr=1e-3, weight_decay=0.05, no_decay=True, layer_decay=0.75)
    head_before = {k: v.detach().clone() for k, v in step.head.state_dict().items()}
    losses = run_steps(model, step, volumes(12, 3, 42))
    assert all(torch.isfinite(l).item() for l in losses)
    for k, v in vit.state_dict().items():
        assert torch.equal(v, before[k]) == k.startswith("mlp_head."), k
    assert all(not torch.equal(v, head_before[k]) for k, v in step.head.state_dict().items())
    arena, shadow = vit.flat_parameters()
    assert torch.equal(shadow.float(), arena.to(shadow.dtype).float())                   # the 16-bit shadow follows the arena, mlp_head included
    W8 = step.head._views(step.head.flat_parameters()[0])[2]
    assert W8[27:].abs().max().item() == 0                                               # the decoder's pad rows stay zero


def test_two_runs_from_one_seed_are_bit_equal():
    from neurovit_amd import MaskedPretrainStep
    out = []
    for _ in range(2):
        model = make_model(16, 4, 51)
        step = MaskedPretrainStep(model, mask_unit=2, lr=1e-3, seed=5)
        losses = run_steps(model, step, volumes(16, 3, 52))
        out.append((torch.stack(losses), step.encoder_state_dict(), {k: v.clone() for k, v in step.head.state_dict().items()}))
    (la, ea, ha), (lb, eb, hb) = out
    assert torch.equal(la, lb) and all(torch.equal(ea[k], eb[k]) for k in ea) and all(torch.equal(ha[k], hb[k]) for k in ha)


def test_a_run_resumed_after_two_of_four_steps_equals_the_straight_run():
    from neurovit_amd import LRSchedule, MaskedPretrainStep
    xs = volumes(12, 4, 62)
    kw = dict(lr=2e-3, no_decay=True, loss="l2", seed=9)
    model = make_model(12, 3, 61)
    straight = MaskedPretrainStep(model, lr_schedule=LRSchedule(2e-3, 4, 1), **kw)
    want = run_steps(model, straight, xs)
    first = make_model(12, 3, 61)
    half = MaskedPretrainStep(first, lr_schedule=LRSchedule(2e-3, 4, 1), **kw)
    got = run_steps(first, half, xs[:2])
    encoder, state = half.encoder_state_dict(), half.state_dict()
    second = make_model(12, 3, 99)                                                       # another initialisation: everything must come from the two states
    second.load_state_dict(encoder, strict=True)
    rest = MaskedPretrainStep(second, lr_schedule=LRSchedule(2e-3, 4, 1), **kw)
    rest.load_state_dict(state)
    got += run_steps(second, rest, xs[2:])
    assert torch.equal(torch.stack(got), torch.stack(want))
    a, b = straight.encoder_state_dict(), rest.encoder_state_dict()
    assert all(torch.equal(a[k], b[k]) for k in a)
    assert all(torch.equal(v, rest.head.state_dict()[k]) for k, v in straight.head.state_dict().items())


def test_pretraining_learns_and_the_encoder_is_adopted():
    from neurovit_amd import MaskedPretrainStep
    from neurovit_amd.synthetic import cube_volumes
    import neurovit_amd.NeuroEncoder as ne
    S, p = 16, 4
    vols = cube_volumes(4 * B, S, 8, grid_noise=0.1, seed=1)[0]
    vols = (vols + 0.05 * torch.randn(vols.shape, generator=torch.Generator().manual_seed(2))).cuda()
    train, held_out = vols[:3 * B], vols[3 * B:]
    model = make_model(S, p, 71)
    head_before = {k: v.detach().clone() for k, v in model.volume_encoder.vit3d.mlp_head.state_dict().items()}
    step = MaskedPretrainStep(model, lr=1e-3, loss="l2", norm_pix=False, seed=3)
    trajectory, val = [], []
    for k in range(20):
        trajectory.append(step(train[(k % 3) * B:(k % 3 + 1) * B]).clone())
        if k in (0, 19):
            val.append(step.validation_loss(held_out).clone())
    assert torch.equal(step.validation_loss(held_out), val[1])                           # fixed masks, no dropout: the same number
    line = "pretraining on cube volumes, train loss per step: " + " ".join(f"{float(l):.4f}" for l in trajectory) + \
        f" | validation after step 1: {float(val[0]):.4f}, after step 20: {float(val[1]):.4f}"
    print(line)
    report(line)
    assert float(val[1]) < float(val[0])
    # adoption: the encoder loads strictly into a fresh NeuroEncoder, whose logits are the pretrained model's - under the untouched head
    fresh = ne.NeuroEncoder(dict(model.config))
    fresh.load_state_dict(step.encoder_state_dict(), strict=True)
    fresh.eval(), model.eval()
    with torch.no_grad():
        assert torch.equal(fresh(held_out), model(held_out))
    assert all(torch.equal(v, head_before[k]) for k, v in fresh.volume_encoder.vit3d.mlp_head.state_dict().items())


def test_fp16_operands_and_the_trainer_shell(tmp_path, monkeypatch):
    """the step on fp16 operands (static loss scale 1024 by default), and TRAINING_OBJECTIVE "mim" through Trainer.train / validate / run"""
    from neurovit_amd import MaskedPretrainStep
    from neurovit_amd.trainer import Trainer
    import neurovit_amd.NeuroEncoder as ne
    model = make_model(12, 3, 81, TRAINING_VIT_OPERANDS="fp16")
    step = MaskedPretrainStep(model, lr=1e-3)
    assert step.loss_scale == 1024.0 and step.head.operands == "fp16"
    before = step.encoder_state_dict()
    losses = run_steps(model, step, volumes(12, 2, 82))
    assert all(torch.isfinite(l).item() for l in losses)
    after = model.state_dict()
    assert all(torch.isfinite(v).all().item() for v in after.values()) and not torch.equal(after[ENC + "cls_token"], before[ENC + "cls_token"])
    assert all(torch.equal(after[k], before[k]) for k in after if ".mlp_head." in k)
    # the Trainer shell: labels are ignored, validation is the reconstruction loss under fixed masks, run() writes both checkpoints
    monkeypatch.chdir(tmp_path)
    vols = torch.cat([v.cpu() for v in volumes(12, 2, 83)])
    ds = torch.utils.data.TensorDataset(torch.zeros(len(vols), 1), torch.zeros(len(vols), 1), vols, torch.zeros(len(vols), dtype=torch.long))
    cfg = dict(W.neuro_config(12, 3, DEVICE="cuda:0", **SIZE), GLOBAL_OUTPUT_DIR=str(tmp_path / "out"), TRAINING_EPOCHS=2, TRAINING_BATCH_SIZE=3,
               TRAINING_NUM_WORKERS=0, TRAINING_OBJECTIVE="mim", PRETRAIN_MASK_RATIO=0.5, TRAINING_LEARNING_RATE=1e-3)
    torch.manual_seed(84)
    trainer = Trainer(cfg, ne.NeuroEncoder(cfg), ds, ds)
    first = trainer.validate(0)[0]
    assert trainer.validate(0)[0] == first                       # fixed masks
    trainer.run()
    assert trainer.step.optimizer.steps == 4 and math.isfinite(trainer.val_loss) and trainer.val_loss < first
    saved = sorted(q.name for q in (tmp_path / "out").rglob("*.pth"))
    assert saved == ["model-e0.pth", "model-e1.pth", "recon-head-e0.pth", "recon-head-e1.pth"]
    path = next((tmp_path / "out").rglob("model-e1.pth"))
    fresh = ne.NeuroEncoder(cfg)
    fresh.load_state_dict(torch.load(path, map_location="cpu", weights_only=True), strict=True)
    head = torch.load(path.with_name("recon-head-e1.pth"), map_location="cpu", weights_only=True)
    assert {k: tuple(v.shape) for k, v in head.items()} == {"norm.weight": (64,), "norm.bias": (64,), "proj.weight": (27, 64), "proj.bias": (27,)}
