"""CPU checks of masked-volume pretraining (no GPU): the restatement the GPU tests hold the kernels to (tests/mim_ref.py), the C-ABI pieces
the feature adds within revision 8, and everything MaskedPretrainStep and the Trainer decide before any device work.

  loss / dpred   mim_ref.recon_ref against torch autograd over torch's own l1_loss / mse_loss in float64, within 1e-12, L1 / L2 x norm_pix;
  labels         a permutation per sample, exactly m masked, mask units whole cubes, (step, sample, rank) change the mask, equal arguments
                 give equal masks; the masked copy (mask_ref of tests/test_perturbation_cpu.py) changes exactly the masked rows of
                 oracle.patchify;
  mask token     a constant patch under the patch LayerNorm is exactly beta;
  boundary       new symbols, revision 8 unchanged, argument checks of the entry points without a device;
  refusals       MaskedPretrainStep's, raised on a CPU-resident model; the Trainer's keys, "absent = unchanged" included.
"""
import ctypes

import pytest
import torch

import mim_ref as R
import weights as W
from oracle import ref_cpu
from test_perturbation_cpu import mask_ref

SIZE = dict(TRAINING_VIT_DIM=64, TRAINING_VIT_DEPTH=2, TRAINING_VIT_HEADS=1, TRAINING_VIT_MLP_DIM=128)
GEOMS = [(16, 4), (12, 3)]


def _cpu_model(S=16, p=4, **extra):
    import neurovit_amd.NeuroEncoder as ne
    return ne.NeuroEncoder(W.neuro_config(S, p, DEVICE="cpu", **dict(SIZE, **extra)))


# ------------------------------------------------------------------------------------------------ the restatement
@pytest.mark.parametrize("S,p", GEOMS)
@pytest.mark.parametrize("kind", ["l1", "l2"])
@pytest.mark.parametrize("norm_pix", [True, False])
def test_restated_loss_and_gradient_against_autograd(S, p, kind, norm_pix):
    B, G, P = 3, S // p, p ** 3
    gen = torch.Generator().manual_seed(S + p)
    x = torch.randn(B, S, S, S, generator=gen) * 3 + 1
    labels = R.labels_ref(B, (G,) * 3, 1, 7, 2)
    m = R.masked_count((G,) * 3, 1, 0.6)
    pred = torch.randn(B * (G ** 3 + 1), P + 5, generator=gen, dtype=torch.float64).requires_grad_(True)
    want = R.recon_loss_autograd(pred, x, labels, m, (p,) * 3, kind, norm_pix)
    (want_d,) = torch.autograd.grad(want, pred)
    loss, dpred, masked, _ = R.recon_ref(pred.detach(), x, labels, m, (p,) * 3, kind, norm_pix, loss_scale=8.0)
    assert abs(loss.item() - want.item()) <= 1e-12 * abs(want.item())
    assert (dpred / 8.0 - want_d[:, :P]).abs().max().item() <= 1e-12 * want_d.abs().max().item()
    assert want_d[:, P:].abs().max().item() == 0 and dpred[~masked].abs().max().item() == 0
    assert int(masked.sum()) == B * m and not masked.reshape(B, -1)[:, 0].any()


def test_norm_pix_targets_follow_maes_rule():
    x = torch.randn(2, 12, 12, 12, generator=torch.Generator().manual_seed(0)) * 5 - 2
    t = R.targets_ref(x, (3, 3, 3), True)
    assert t.mean(dim=-1).abs().max().item() < 1e-12
    raw = R.patches_of(x, (3, 3, 3)).double()
    assert torch.allclose(t.var(dim=-1, unbiased=True), raw.var(dim=-1, unbiased=True) / (raw.var(dim=-1, unbiased=True) + 1e-6), rtol=1e-12, atol=0)
    assert torch.equal(R.targets_ref(x, (3, 3, 3), False), raw)


# ------------------------------------------------------------------------------------------------ the masks
@pytest.mark.parametrize("unit", [1, 2])
def test_labels_are_permutations_with_m_masked_whole_cubes(unit):
    grid, B = (4, 4, 4), 4
    N, u3 = 64, unit ** 3
    for ratio in (0.01, 0.25, 0.6, 0.99):
        m = R.masked_count(grid, unit, ratio)
        U = N // u3
        assert m % u3 == 0 and u3 <= m <= N - u3 and m == min(max(int(ratio * U + 0.5), 1), U - 1) * u3
        labels = R.labels_ref(B, grid, unit, 5, 1)
        for b in range(B):
            assert sorted(labels[b].tolist()) == list(range(N))
            assert int((labels[b] < m).sum()) == m
            # a unit is masked as a whole: the patches of one cube carry one rank
            cube = labels[b].reshape(4, 4, 4) // u3                 # [g2, g0, g1] -> the unit's rank
            for g2 in range(4):
                for g0 in range(4):
                    for g1 in range(4):
                        assert cube[g2, g0, g1] == cube[g2 - g2 % unit, g0 - g0 % unit, g1 - g1 % unit]


def test_masks_differ_by_step_sample_rank_and_repeat():
    grid = (4, 4, 4)
    base = R.labels_ref(2, grid, 1, 9, 3, 0)
    assert torch.equal(base, R.labels_ref(2, grid, 1, 9, 3, 0))
    assert not torch.equal(base[0], base[1])
    for other in (R.labels_ref(2, grid, 1, 9, 4, 0), R.labels_ref(2, grid, 1, 9, 3, 1), R.labels_ref(2, grid, 1, 10, 3, 0)):
        assert not torch.equal(base, other)
    # sample b of a larger batch is the same sample: the draw does not depend on B
    assert torch.equal(R.labels_ref(3, grid, 1, 9, 3, 0)[:2], base)
    # no draw of the augmentation is reused: the domain differs
    import augment_ref as A
    assert R.unit_keys(9, 0, 3, 0, 4)[0] != A.draw(9, 0, 3, 0, 0) >> 40


@pytest.mark.parametrize("S,p", GEOMS)
def test_masked_copy_changes_exactly_the_masked_rows_of_patchify(S, p):
    B, G = 2, S // p
    x = torch.arange(B * S ** 3, dtype=torch.float32).reshape(B, S, S, S) + 1
    for unit in (1, 2):
        labels = R.labels_ref(B, (G,) * 3, unit, 1, 0)
        m = R.masked_count((G,) * 3, unit, 0.5)
        jobs = torch.tensor([[b, 0, m] for b in range(B)], dtype=torch.int32)
        masked = mask_ref(x, labels, jobs, p, -3.0)
        rows, orig, sel = R.patches_of(masked, (p,) * 3), R.patches_of(x, (p,) * 3), labels < m
        assert (rows[sel] == -3.0).all() and torch.equal(rows[~sel], orig[~sel]) and int(sel.sum()) == B * m


def test_a_constant_patch_under_the_patch_layernorm_is_beta():
    P = 27
    g = torch.Generator().manual_seed(1)
    gamma, beta = torch.randn(P, generator=g), torch.randn(P, generator=g)
    for value in (0.0, -1.5, 3e4):
        out = torch.nn.functional.layer_norm(torch.full((4, P), value), (P,), gamma, beta, 1e-5)
        assert torch.equal(out, beta.expand(4, P))


# ------------------------------------------------------------------------------------------------ the boundary
NEW = ("nv_mim_masked_count", "nv_mim_labels", "nv_recon_loss", "nv_token_grad_seed", "nv_token_grad_seed_rows", "nv_token_grad_seed_workspace_bytes",
       "nv_vit_backward_tokens")


def test_header_declares_and_library_exports_the_new_entry_points():
    from neurovit_amd import _cabi
    dll = ctypes.CDLL(_cabi.LIB_PATH)
    for name in NEW:
        assert name in _cabi.lib.protos, name
        assert getattr(dll, name) is not None, name
    assert _cabi.ABI_VERSION == 8 and _cabi.lib.nv_abi_version() == 8
    assert "#define NV_ABI_VERSION 8" in open(_cabi.HEADER).read()
    # nv_vit_backward_ex's argument list, a pointer in the place of a pointer
    assert _cabi.lib.protos["nv_vit_backward_tokens"] == _cabi.lib.protos["nv_vit_backward_ex"]


def test_entry_points_check_their_arguments_without_a_gpu():
    from neurovit_amd import _cabi, engine
    from neurovit_amd._cabi import lib

    def i3(*v):
        arr = (ctypes.c_int * 3)(*v)
        return arr, ctypes.cast(arr, ctypes.c_void_p)
    fake = 4096
    _a, g4 = i3(4, 4, 4)
    _b, g6 = i3(6, 4, 4)
    _c, g32 = i3(32, 32, 32)
    assert lib.nv_mim_masked_count(g4, 1, 0.6) == 38 and lib.nv_mim_masked_count(g4, 2, 0.6) == 40
    assert lib.nv_mim_masked_count(g4, 1, 0.001) == 1 and lib.nv_mim_masked_count(g4, 1, 0.999) == 63
    for grid, unit, ratio in ((g4, 3, 0.5), (g6, 4, 0.5), (g4, 4, 0.5), (g4, 0, 0.5), (g4, 1, 0.0), (g4, 1, 1.0), (g32, 1, 0.5)):
        assert lib.nv_mim_masked_count(grid, unit, ratio) == -1
    assert lib.nv_mim_labels(0, 0, 0, 2, g4, 3, fake, None) == -1 and "divide" in _cabi.last_error()
    assert lib.nv_mim_labels(0, 0, 0, 2, g4, 1, None, None) == -1 and lib.nv_mim_labels(0, 0, -1, 2, g4, 1, fake, None) == -1
    assert lib.nv_mim_labels(0, 0, 0, 0, g4, 1, fake, None) == -1
    _d, s16 = i3(16, 16, 16)
    _e, p4 = i3(4, 4, 4)
    _f, p5 = i3(4, 5, 4)
    ok = dict(pred=fake, ldp=64, x=fake, B=2, size=s16, patch=p4, labels=fake, m=38, kind=0, norm=1, scale=1.0, dpred=fake, ldd=64, part=fake, loss=fake)

    def recon(**kw):
        a = dict(ok, **kw)
        return lib.nv_recon_loss(a["pred"], a["ldp"], a["x"], a["B"], a["size"], a["patch"], a["labels"], a["m"], a["kind"], a["norm"], a["scale"], a["dpred"],
                                 a["ldd"], a["part"], a["loss"], None)
    for bad in (dict(pred=None), dict(x=None), dict(dpred=None), dict(part=None), dict(B=0), dict(patch=p5), dict(m=0), dict(m=65), dict(kind=2),
                dict(scale=0.0), dict(scale=float("inf")), dict(ldp=60), dict(ldp=66), dict(pred=fake + 4), dict(ldd=60), dict(ldd=68), dict(dpred=fake + 8)):
        assert recon(**bad) == -1, bad
    assert lib.nv_token_grad_seed(None, 4, 64, fake, fake, None, 0, 0, 0.0, None) == -1
    assert lib.nv_token_grad_seed(fake, 4, 62, fake, fake, None, 0, 0, 0.0, None) == -1
    assert lib.nv_token_grad_seed(fake, 4, 64, fake, fake, fake, 8, 0, 0.0, None) == -1 and "too small" in _cabi.last_error()
    assert lib.nv_token_grad_seed_rows(1000) == 256 and lib.nv_token_grad_seed_rows(7) == 7 and lib.nv_token_grad_seed_workspace_bytes(7, 64) == 7 * 64 * 4
    # nv_vit_backward_tokens: NULL / misaligned dtokens, and arguments that select the cls-rows form
    cfg = engine.make_config(image_size=16, image_patch_size=4, frames=16, frame_patch_size=4, num_classes=2, dim=64, depth=2, heads=1, dim_head=64,
                             mlp_dim=128, channels=1)
    strides = (ctypes.c_long * 5)(4096, 4096, 256, 16, 1)

    def tokens(dtokens, rows_form, B=2):
        return lib.nv_vit_backward_tokens(ctypes.byref(cfg), B, fake, strides, fake, fake, fake, 1 << 40, dtokens, fake, None, 0, 0, 3, 0.0, 0.0, 0, None,
                                          None, 1, rows_form, None)
    assert tokens(None, 1) == -1 and "dtokens" in _cabi.last_error()
    assert tokens(fake + 4, 1) == -1 and "dtokens" in _cabi.last_error()
    assert tokens(fake, 2) == -1 and "cls-rows" in _cabi.last_error()
    assert tokens(fake, 0) == -1 and "cls-rows" in _cabi.last_error()          # the process default is the cls-rows form


# ------------------------------------------------------------------------------------------------ the step, before any device work
def test_step_refusals():
    from neurovit_amd import LRSchedule, MaskedPretrainStep
    from neurovit_amd.optim import LossScaler
    model = _cpu_model()
    for kw, err in ((dict(mask_ratio=0.0), ValueError), (dict(mask_ratio=1.0), ValueError), (dict(mask_ratio="0.5"), ValueError),
                    (dict(mask_unit=3), ValueError), (dict(mask_unit=4), ValueError), (dict(mask_unit=0), ValueError), (dict(loss="huber"), ValueError),
                    (dict(norm_pix=1), TypeError), (dict(loss_scale="dynamic"), NotImplementedError), (dict(loss_scale=0.0), ValueError),
                    (dict(process_group=object()), NotImplementedError), (dict(lr_schedule="cosine"), TypeError), (dict(seed=-1), ValueError)):
        with pytest.raises(err):
            MaskedPretrainStep(model, **kw)
    four_d = _cpu_model()
    four_d.config = dict(four_d.config, TRAINING_DIM=4)
    with pytest.raises(NotImplementedError, match="3D"):
        MaskedPretrainStep(four_d)
    with pytest.raises(TypeError):
        MaskedPretrainStep(model.volume_encoder)
    from neurovit_amd.vit_3d import ViT
    rgb = _cpu_model()
    rgb.volume_encoder.vit3d = ViT(image_size=16, image_patch_size=4, frames=16, frame_patch_size=4, num_classes=2, dim=64, depth=1, heads=1, mlp_dim=64, channels=3)
    with pytest.raises(ValueError, match="channel"):
        MaskedPretrainStep(rgb)
    step = MaskedPretrainStep(model, mask_unit=2, lr_schedule=LRSchedule(1e-3, 10, 2))
    assert step.masked_patches == 40 == R.masked_count((4, 4, 4), 2, 0.6) and step.last_lr == 5e-4
    with pytest.raises(ValueError, match="cuda"):
        step(torch.zeros(2, 16, 16, 16))                                        # CPU tensors
    with pytest.raises(ValueError, match="expected volumes"):
        step(torch.zeros(2, 16, 16, 8))
    assert isinstance(LossScaler, type)


def test_step_groups_state_and_the_decoder_on_a_cpu_model():
    from neurovit_amd import MaskedPretrainStep, ReconstructionHead
    model = _cpu_model(12, 3)
    step = MaskedPretrainStep(model, lr=2e-3, weight_decay=0.05, no_decay=True, layer_decay=0.5)
    groups = step.optimizer.param_groups
    idle = groups[-1]
    assert idle["lr"] == 0.0 and idle["weight_decay"] == 0.0 and {id(p) for p in idle["params"]} == {id(p) for p in model.volume_encoder.vit3d.mlp_head.parameters()}
    seen = [id(p) for g in groups for p in g["params"]]
    assert len(seen) == len(set(seen)) == len(list(model.parameters())) + 4       # every parameter of the encoder and the decoder, once
    assert all(g["lr"] == 2e-3 * g["lr_scale"] for g in groups)
    # the decoder: P = 27 stored with 32 rows, state_dict exposes [27, 64]
    head = step.head
    assert isinstance(head, ReconstructionHead) and (head.patch_dim, head.padded_dim) == (27, 32)
    arena, _ = head.flat_parameters()
    assert arena.numel() == 2 * 64 + 32 * 64 + 32 and {k: tuple(v.shape) for k, v in head.state_dict().items()} == {
        "norm.weight": (64,), "norm.bias": (64,), "proj.weight": (27, 64), "proj.bias": (27,)}
    assert head.proj.weight.data_ptr() == arena.data_ptr() + 4 * 128 and head.proj.bias.data_ptr() == arena.data_ptr() + 4 * (128 + 32 * 64)
    assert arena[128 + 27 * 64:128 + 32 * 64].abs().max().item() == 0 and arena[-5:].abs().max().item() == 0      # the pad rows
    # encoder_state_dict: the model's keys and shapes; the state: step count, moments of both arenas, the decoder
    enc, ref = step.encoder_state_dict(), model.state_dict()
    assert list(enc) == list(ref) and all(enc[k].shape == ref[k].shape and enc[k].data_ptr() != ref[k].data_ptr() for k in ref)
    state = step.state_dict()
    assert state["steps"] == 0 and len(state["arenas"]) == 2 and set(state["head"]) == set(head.state_dict()) and len(state["groups"]) == len(groups)
    other = MaskedPretrainStep(_cpu_model(12, 3), lr=1e-3, no_decay=True, layer_decay=0.9)
    state["steps"] = 7
    other.load_state_dict(state)
    assert other.optimizer.steps == 7 and all(torch.equal(a, b) for a, b in zip(other.head.state_dict().values(), head.state_dict().values()))
    with pytest.raises(ValueError, match="version"):
        other.load_state_dict(dict(state, version=2))
    with pytest.raises(ValueError, match="parameter groups"):
        MaskedPretrainStep(_cpu_model(12, 3)).load_state_dict(state)


# ------------------------------------------------------------------------------------------------ the Trainer's keys
def test_trainer_keys():
    import neurovit_amd.NeuroEncoder as ne
    from neurovit_amd.pretrain import MaskedPretrainStep
    from neurovit_amd.trainer import Trainer, TrainStep
    read = Trainer.objective_from_config
    geo = dict(TRAINING_VIT_INPUT_SIZE=16, TRAINING_VIT_PATCH_SIZE=4)
    assert read({}) is None and read({"TRAINING_OBJECTIVE": None}) is None and read({"TRAINING_OBJECTIVE": "supervised"}) is None
    assert read(dict(geo, TRAINING_OBJECTIVE="mim")) == dict(mask_ratio=0.6, mask_unit=1, loss="l1", norm_pix=True)
    assert read(dict(geo, TRAINING_OBJECTIVE="mim", PRETRAIN_MASK_RATIO=0.75, PRETRAIN_MASK_UNIT=2, PRETRAIN_LOSS="l2", PRETRAIN_NORM_PIX=False)) == \
        dict(mask_ratio=0.75, mask_unit=2, loss="l2", norm_pix=False)
    for bad, err in ((dict(TRAINING_OBJECTIVE="mae"), ValueError), (dict(TRAINING_OBJECTIVE="mim", PRETRAIN_MASK_RATIO=1.5), ValueError),
                     (dict(TRAINING_OBJECTIVE="mim", PRETRAIN_MASK_UNIT=3), ValueError), (dict(TRAINING_OBJECTIVE="mim", PRETRAIN_LOSS="ce"), ValueError),
                     (dict(TRAINING_OBJECTIVE="mim", PRETRAIN_NORM_PIX="yes"), TypeError)):
        with pytest.raises(err):
            read(dict(geo, **bad))
    ds = torch.utils.data.TensorDataset(torch.zeros(2, 1), torch.zeros(2, 1), torch.zeros(2, 16, 16, 16), torch.zeros(2, dtype=torch.long))
    base = dict(W.neuro_config(16, 4, DEVICE="cpu", **SIZE), GLOBAL_OUTPUT_DIR="unused", TRAINING_EPOCHS=1, TRAINING_BATCH_SIZE=2, TRAINING_NUM_WORKERS=0)
    plain = Trainer(base, ne.NeuroEncoder(base), ds, ds)
    assert plain.pretrain is None and type(plain.step) is TrainStep                       # absent = unchanged
    assert type(Trainer(dict(base, PRETRAIN_MASK_RATIO=0.9), ne.NeuroEncoder(base), ds, ds).step) is TrainStep      # the other keys alone switch nothing on
    cfg = dict(base, TRAINING_OBJECTIVE="mim", PRETRAIN_MASK_UNIT=2, PRETRAIN_LOSS="l2", TRAINING_LR_SCHEDULE="cosine", TRAINING_NO_DECAY_NORM_BIAS=True)
    t = Trainer(cfg, ne.NeuroEncoder(cfg), ds, ds)
    assert isinstance(t.step, MaskedPretrainStep) and (t.step.mask_unit, t.step.loss, t.step.masked_patches) == (2, "l2", 40)
    assert t.step.lr_schedule is not None and t.optimizer is t.step.optimizer
    for clash in (dict(AUGMENT_MIXUP_ALPHA=0.2), dict(TRAINING_EMA_DECAY=0.99), dict(TRAINING_GRAD_CLIP=1.0), dict(TRAINING_LABEL_SMOOTHING=0.1)):
        with pytest.raises(ValueError, match="does not go with"):
            Trainer(dict(cfg, **clash), ne.NeuroEncoder(cfg), ds, ds)
