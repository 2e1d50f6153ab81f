"""CPU checks of Mixup / CutMix and the soft-target cross-entropy (no GPU): the C-ABI pieces added within revision 8 (nv_loss_opts,
nv_ce_loss_soft, nv_head_step_soft, nv_vit_train_step_ex, nv_mix_params, nv_augment_mix), the refusals of the Python layer, and the CPU
restatement (tests/mix_ref.py) that the GPU tests (tests/test_mix_gpu.py) hold the kernels to:

  loss           ce_soft_ref against torch in float64: without a mix F.cross_entropy(z, y, weight=w, label_smoothing=eps), without
                 weights F.cross_entropy(z, q, label_smoothing=eps), the gradient against autograd - to 1e-12; planted: denominator B
                 under weights;
  lambda         65 536 restated draws per alpha in {0.1, 0.4, 1.0}: the mean within 5 standard errors of 1/2 (sigma / sqrt(n) with
                 sigma^2 = 1 / (4 (2 alpha + 1))), the variance within 5 % of that value (the sample variance of n draws has a relative
                 standard error of sqrt((kurtosis - 1) / n) <= 1.1 / 256 = 0.43 % here, so 5 % is beyond 11 sigma);
  acceptance     for the exact (seed, rank, step, B) tuples of the GPU test no Joehnk try has |x + y - 1| < 1e-9;
  box            0 <= lo <= hi <= S, label lambda = 1 - cells / total, lambda = 1 gives an empty box; planted: box not clipped;
  mixing pass    mix_apply_ref against a cell-by-cell formulation in explicit numpy.float32 operations; planted: mu formed per cell in double;
  refusals       every NV_ERR_ARG of the new entry points and every argument error of VolumeMix, CrossEntropyLoss and TrainStep, without a device.
"""
import ctypes
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import augment_ref as R
import mix_ref as M

NAMES = ("nv_ce_loss_soft", "nv_head_step_soft", "nv_vit_train_step_ex", "nv_mix_params", "nv_augment_mix")


# ------------------------------------------------------------------ symbols and ABI
def test_header_declares_and_library_exports_the_new_entry_points():
    from neurovit_amd import _cabi
    from neurovit_amd.augment import MixConfig
    dll = ctypes.CDLL(_cabi.LIB_PATH)
    for name in NAMES:
        assert name in _cabi.lib.protos, name
        assert getattr(dll, name) is not None, name
    assert _cabi.ABI_VERSION == 8 and dll.nv_abi_version() == 8          # new symbols only
    header = open(_cabi.HEADER).read()
    assert "#define NV_ABI_VERSION 8" in header and "#define NV_MIX_COLS 12" in header
    assert ctypes.sizeof(_cabi.LossOpts) == 24 and ctypes.sizeof(MixConfig) == 48 and _cabi.MIX_COLS == M.COLS == 12
    # nv_vit_train_step_ex is nv_vit_train_step with one pointer more, in front of the dropout arguments
    old, new = _cabi.lib.protos["nv_vit_train_step"][1], _cabi.lib.protos["nv_vit_train_step_ex"][1]
    assert new == old[:18] + [ctypes.c_void_p] + old[18:]


def test_the_package_exports_volume_mix():
    import neurovit_amd
    from neurovit_amd.augment import VolumeMix
    assert neurovit_amd.VolumeMix is VolumeMix


# ------------------------------------------------------------------ the loss restatement against torch
def loss_case(B, C, seed, mixed):
    g = torch.Generator().manual_seed(seed)
    z = (3 * torch.randn(B, C, generator=g)).double()
    y = torch.randint(0, C, (B,), generator=g)
    w = torch.rand(C, generator=g).double() + 0.25
    mix = None
    if mixed:
        lam = torch.rand(B, generator=g).float()
        lam[0] = 1.0
        mix = np.zeros((B, M.COLS), dtype=np.int32)
        mix[:, 0] = np.arange(B)[::-1]
        mix[:, 3] = lam.numpy().view(np.int32)
    return z, y, w, mix


@pytest.mark.parametrize("eps", [0.0, 0.1])
@pytest.mark.parametrize("B,C", [(1, 2), (5, 3), (7, 300)])
def test_loss_restatement_equals_torch_in_float64(B, C, eps):
    z, y, w, mix = loss_case(B, C, 3, True)
    # index targets with weights: torch divides by sum w[y]
    zt = z.clone().requires_grad_(True)
    want = F.cross_entropy(zt, y, weight=w, label_smoothing=eps)
    want.backward()
    loss, grad = M.ce_soft_ref(z.numpy(), y.numpy(), eps, w.numpy())
    assert abs(loss - want.item()) < 1e-12 * max(1.0, abs(want.item())) and np.abs(grad - zt.grad.numpy()).max() < 1e-12
    # planted: the denominator B under weights is caught
    bad, _ = M.ce_soft_ref(z.numpy(), y.numpy(), eps, w.numpy(), defect="denominator_B")
    assert abs(bad - want.item()) > 1e-3 * abs(want.item())
    # probability targets without weights: torch divides by B
    q = torch.from_numpy(M.soft_targets(y.numpy(), C, mix))
    zt = z.clone().requires_grad_(True)
    want = F.cross_entropy(zt, q, label_smoothing=eps)
    want.backward()
    loss, grad = M.ce_soft_ref(z.numpy(), y.numpy(), eps, None, mix)
    assert abs(loss - want.item()) < 1e-12 * max(1.0, abs(want.item())) and np.abs(grad - zt.grad.numpy()).max() < 1e-12
    # both: the project's rule (D = the unsmoothed weight of the mixed target); the gradient is the derivative of the loss
    zt = z.clone().requires_grad_(True)
    qs = (1 - eps) * q + eps / C
    own = -(w * qs * F.log_softmax(zt, dim=1)).sum() / (w * q).sum()
    own.backward()
    loss, grad = M.ce_soft_ref(z.numpy(), y.numpy(), eps, w.numpy(), mix)
    assert abs(loss - own.item()) < 1e-12 * max(1.0, abs(own.item())) and np.abs(grad - zt.grad.numpy()).max() < 1e-12


# ------------------------------------------------------------------ lambda
@pytest.mark.parametrize("alpha", [0.1, 0.4, 1.0])
def test_joehnk_draws_have_the_moments_of_beta(alpha):
    n = 65536
    lam = np.array([float(M.joehnk(7, 0, b >> 8, b & 255, alpha)[0]) for b in range(n)])
    var = 1.0 / (4.0 * (2.0 * alpha + 1.0))
    assert abs(lam.mean() - 0.5) < 5.0 * math.sqrt(var / n), (lam.mean(), alpha)
    assert abs(lam.var() / var - 1.0) < 0.05, (lam.var(), var)
    assert lam.min() >= 0.0 and lam.max() <= 1.0


def test_no_try_of_the_gpu_tests_draws_sits_on_the_acceptance_edge():
    worst, most = float("inf"), 0
    for name, cfg in M.PARAM_CONFIGS.items():
        for seed, rank, step in M.PARAM_TRIPLES:
            for B in M.PARAM_BATCHES:
                rows, gap = M.mix_params_ref(B, step, M.PARAM_ROI, seed=seed, rank=rank, **cfg)
                worst, most = min(worst, gap), max(most, int(rows[:, 4].max()))
                assert (rows[:, 0] == np.arange(B)[::-1]).all()
                if name == "never" or B == 1:
                    assert (rows[:, 1] == 0).all()
                if B % 2:
                    assert rows[B // 2, 1] == 0                          # the middle sample pairs with itself
    assert worst >= 1e-9, worst
    assert 1 < most < 64


# ------------------------------------------------------------------ the box
def test_box_invariants_and_the_planted_unclipped_box():
    roi = (17, 20, 33)
    total = roi[0] * roi[1] * roi[2]
    outside = 0
    for b in range(512):
        lam = np.float32((b % 64) / 63.0) if b < 448 else M.joehnk(1, 0, 0, b, 0.4)[0]
        centres = [M.draw(9, 1, 3, b, 2 + a) for a in range(3)]
        edges, label = M.box(lam, centres, roi)
        cells = 1
        for a in range(3):
            lo, hi = edges[2 * a], edges[2 * a + 1]
            assert 0 <= lo <= hi <= roi[a], (b, edges)
            cells *= hi - lo
        assert label == np.float32(1.0 - cells / total)
        if lam == np.float32(1.0):
            assert cells == 0 and label == np.float32(1.0)
        bad, _ = M.box(lam, centres, roi, defect="unclipped")
        outside += any(bad[2 * a] < 0 or bad[2 * a + 1] > roi[a] for a in range(3))
    assert outside > 50                                                  # the planted defect leaves the window: the invariants above catch it
    # through the table: the same invariants on whole rows
    rows, _ = M.mix_params_ref(257, 4, roi, cutmix_alpha=1.0, seed=2)
    cut = rows[rows[:, 1] == 2]
    assert len(cut) == 256 and (cut[:, 5:11:2] >= 0).all() and (cut[:, 5:11:2] <= cut[:, 6:11:2]).all() and (cut[:, 6:11:2] <= np.array(roi)).all()
    bad, _ = M.mix_params_ref(257, 4, roi, cutmix_alpha=1.0, seed=2, defect="unclipped")
    assert ((bad[:, 5:11:2] < 0) | (bad[:, 6:11:2] > np.array(roi))).any()


# ------------------------------------------------------------------ the mixing pass
def small_case():
    g = torch.Generator().manual_seed(5)
    x = torch.randn(3, 7, 6, 5, 2, generator=g)
    x[0, 1, 2, 3, 0] = float("nan")
    x[1, 0, 0, 0, 1] = -0.0
    x[2, 3, 3, 3, 1] = float("inf")
    x.view(-1)[11] = torch.tensor([0x7fc01234], dtype=torch.int32).view(torch.float32)[0]
    scale, shift = torch.tensor([0.75, -0.3]).view(torch.int32).tolist()
    aug = torch.tensor([[1, 0, -1, 5, M.ONE_BITS, 0, 0, 0], [0, 2, 1, 2, scale, shift, 0, 0], [2, -1, 0, 0, M.ONE_BITS, 0, 0, 0]], dtype=torch.int32)
    lam = [0x3E99999B, M.f32_bits(0.5)]                          # 0.3 + 1 ulp: an odd multiple of 2^-25, so 1 - lambda does round in fp32
    mix = np.array([[2, 1, lam[0], lam[0], 1, 0, 0, 0, 0, 0, 0, 0], [1, 0, M.ONE_BITS, M.ONE_BITS, 0, 0, 0, 0, 0, 0, 0, 0],
                    [0, 2, lam[1], lam[1], 1, 1, 4, 0, 3, 2, 9, 0]], dtype=np.int32)
    return x, aug, mix, (5, 4, 4)


def test_mixing_restatement_against_a_cell_by_cell_formulation():
    x, aug, mix, roi = small_case()
    fill = -2.5
    got, moved = M.mix_apply_ref(x, aug, mix, roi, fill)
    A = R.apply_ref(x, aug, roi, fill).numpy()
    want = np.empty_like(A)
    f = np.float32
    with np.errstate(all="ignore"):
        for b in range(3):
            p, mode, lam = int(mix[b, 0]), int(mix[b, 1]), M.bits_f32(int(mix[b, 2]))
            mu = f(1.0) - lam
            for idx in np.ndindex(*A.shape[1:]):
                a_own, a_par = A[(b, *idx)], A[(p, *idx)]
                if mode == 1:
                    want[(b, *idx)] = f(f(lam * a_own) + f(mu * a_par))
                elif mode == 2 and mix[b, 5] <= idx[0] < mix[b, 6] and mix[b, 7] <= idx[1] < mix[b, 8] and mix[b, 9] <= idx[2] < mix[b, 10]:
                    want.view(np.uint32)[(b, *idx)] = A.view(np.uint32)[(p, *idx)]
                else:
                    want.view(np.uint32)[(b, *idx)] = A.view(np.uint32)[(b, *idx)]
    assert M.same_bits(got, torch.from_numpy(want), moved)
    assert np.array_equal(got.numpy().view(np.uint32)[1:], want.view(np.uint32)[1:])       # the unmixed and the cutmix sample: A_b / A_p verbatim
    assert moved[2].all()                                                                  # cutmix of two samples without an intensity change: bit moves
    assert not moved[0].any() and not moved[1].any()                                       # mixup is arithmetic; sample 1 has an intensity change
    # planted: mu formed per cell as 1 - lambda in double
    bad, _ = M.mix_apply_ref(x, aug, mix, roi, fill, defect="mu_double")
    assert not M.same_bits(bad, torch.from_numpy(want), moved)
    # a NULL augmentation table is the identity-row table; mode 0 everywhere is apply_ref
    same, _ = M.mix_apply_ref(x, None, mix, (7, 6, 5))
    rows, _ = M.mix_apply_ref(x, M.identity_rows(3), mix, (7, 6, 5))
    assert torch.equal(R.bits(same), R.bits(rows))
    none = mix.copy()
    none[:, 1] = 0
    assert torch.equal(R.bits(M.mix_apply_ref(x, aug, none, roi, fill)[0]), R.bits(R.apply_ref(x, aug, roi, fill)))


# ------------------------------------------------------------------ refusals of the entry points
def mix_config(**kw):
    from neurovit_amd.augment import MixConfig
    cfg = MixConfig(ctypes.sizeof(MixConfig), (ctypes.c_int * 3)(80, 80, 80), 0.4, 1.0, 1.0, 0.5)
    for k, v in kw.items():
        setattr(cfg, k, v)
    return cfg


def loss_opts(**kw):
    from neurovit_amd._cabi import LossOpts
    lo = LossOpts(ctypes.sizeof(LossOpts), 0.1, None, None)
    for k, v in kw.items():
        setattr(lo, k, v)
    return lo


def test_entry_points_check_their_arguments_without_a_gpu():
    from neurovit_amd import _cabi
    from neurovit_amd._cabi import lib
    fake = 4096                                            # a non-null, 16-byte aligned address nothing dereferences: the checks come first
    i3 = lambda *v: ctypes.cast((ctypes.c_int * 3)(*v), ctypes.c_void_p)
    st = ctypes.cast((ctypes.c_long * 5)(1, 1, 1, 1, 1), ctypes.c_void_p)

    def refused(rc, text):
        assert rc == -1 and text in _cabi.last_error(), (rc, _cabi.last_error())

    # nv_mix_params
    params = lambda cfg, B=4, rank=0, out=fake: lib.nv_mix_params(None if cfg is None else ctypes.byref(cfg), 0, 0, rank, B, out, None)
    refused(params(None), "bad arguments")
    refused(params(mix_config(), out=None), "bad arguments")
    refused(params(mix_config(), B=0), "bad arguments")
    refused(params(mix_config(), rank=-1), "bad arguments")
    refused(params(mix_config(struct_size=40)), "struct_size")
    refused(params(mix_config(roi=(ctypes.c_int * 3)(80, 0, 80))), "must be positive")
    for alpha in (0.04, 1.5, -0.4, float("nan")):
        refused(params(mix_config(mixup_alpha=alpha)), "outside [0.05, 1]")
        refused(params(mix_config(cutmix_alpha=alpha)), "outside [0.05, 1]")
    for p in (-0.1, 1.1, float("nan")):
        refused(params(mix_config(prob=p)), "outside [0, 1]")
        refused(params(mix_config(switch_prob=p)), "outside [0, 1]")
    # nv_augment_mix: as nv_augment_apply
    apply = lambda src=fake, B=2, in3=(20, 20, 20), T=1, aug=fake, mix=fake, roi=(16, 16, 16), out=fake: lib.nv_augment_mix(
        src, st, B, i3(*in3), T, aug, mix, i3(*roi), 0.0, out, None)
    refused(apply(src=None), "bad arguments")
    refused(apply(mix=None), "bad arguments")
    refused(apply(out=None), "bad arguments")
    refused(apply(B=0), "bad arguments")
    refused(apply(T=0), "bad arguments")
    refused(apply(roi=(16, 0, 16)), "must be positive")
    refused(apply(in3=(20, -1, 20)), "must be positive")
    refused(apply(roi=(16, 21, 16)), "larger than the input")
    refused(apply(out=fake + 4), "16-byte aligned")
    refused(apply(aug=fake + 2), "16-byte aligned")
    refused(apply(B=2 ** 27, in3=(32, 20, 20), roi=(32, 16, 16)), "beyond one launch")
    # nv_ce_loss_soft / nv_head_step_soft / nv_vit_train_step_ex: the option block is checked ahead of everything it guards
    ce = lambda lo, B=2, C=3, logits=fake, loss=fake: lib.nv_ce_loss_soft(logits, fake, B, C, 1.0, None, None if lo is None else ctypes.byref(lo), loss, fake, None)
    refused(ce(loss_opts(), B=0), "bad args")
    refused(ce(loss_opts(), C=0), "bad args")
    refused(ce(loss_opts(), logits=None), "bad args")
    refused(ce(loss_opts(), loss=None), "bad args")
    refused(ce(loss_opts(struct_size=16)), "struct_size")
    for eps in (-0.1, 1.0, 1.5, float("nan")):
        refused(ce(loss_opts(label_smoothing=eps)), "outside [0, 1)")
    refused(ce(loss_opts(class_weight=fake + 2)), "4-byte aligned")
    head = lambda lo, C=2, x=fake: lib.nv_head_step_soft(x, 8, 2, 8, fake, fake, 1e-5, fake, fake, C, fake, 1.0, None, ctypes.byref(lo), fake, fake, fake, fake, fake,
                                                        1, fake, 8, None, 8, fake, fake, fake, fake, None, 0, fake, 1 << 20, 0, 0.0, None)
    refused(head(loss_opts(struct_size=0)), "struct_size")
    refused(head(loss_opts(label_smoothing=1.0)), "outside [0, 1)")
    refused(head(loss_opts(), C=9), "nv_head_step_soft: B = 2, d = 8, C = 9")
    refused(head(loss_opts(), x=None), "null pointer")
    from neurovit_amd.engine import make_config
    cfg = make_config(image_size=16, image_patch_size=8, frames=16, frame_patch_size=8, num_classes=2, dim=64, depth=1, heads=2, mlp_dim=64, channels=1, dim_head=32)
    hp = _cabi.TrainHparams(ctypes.sizeof(_cabi.TrainHparams), 1, 1e-3, 0.9, 0.999, 1e-8, 1e-2, 1.0, 0, 1, 0, 0.0, None, None)
    step = lambda lo, hp=hp: lib.nv_vit_train_step_ex(ctypes.byref(cfg), 2, fake, st, st, None, fake, fake, fake, fake, fake, fake, 1 << 20, fake, fake, fake, fake,
                                                     ctypes.byref(hp), ctypes.byref(lo), 0.0, 0.0, 0, None, None)
    refused(step(loss_opts(struct_size=8)), "nv_loss_opts.struct_size")
    refused(step(loss_opts(label_smoothing=-1.0)), "outside [0, 1)")
    bad_hp = _cabi.TrainHparams(ctypes.sizeof(_cabi.TrainHparams), 1, 1e-3, 0.9, 0.999, 1e-8, 1e-2, 1.0, 0, 1, 7, 0.0, None, None)
    refused(step(loss_opts(), hp=bad_hp), "fuse_update = 7")


# ------------------------------------------------------------------ refusals of the Python layer
def test_volume_mix_validates_its_arguments():
    from neurovit_amd.augment import VolumeAugment, VolumeMix
    for kw, err in ((dict(mixup_alpha=1.5), ValueError), (dict(cutmix_alpha=0.01), ValueError), (dict(mixup_alpha="a"), TypeError), (dict(mixup_alpha=True), TypeError),
                    (dict(prob=1.5), ValueError), (dict(switch_prob=-0.5), ValueError), (dict(prob=None), TypeError), (dict(seed=-1), ValueError),
                    (dict(seed=1.5), TypeError), (dict(rank=2 ** 31), ValueError), (dict(rank="0"), TypeError)):
        with pytest.raises(err, match="VolumeMix"):
            VolumeMix(**kw)
    ident = VolumeMix()
    assert ident.is_identity() and not VolumeMix(mixup_alpha=0.4).is_identity() and not VolumeMix(cutmix_alpha=1).is_identity()
    mix = VolumeMix(mixup_alpha=0.4, cutmix_alpha=1.0)
    x = torch.zeros(2, 8, 8, 8)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        mix(x)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        mix.params(2, 0, (8, 8, 8), device="cpu")
    with pytest.raises(TypeError, match="float32"):
        mix(x.double())
    with pytest.raises(ValueError, match=r"expected \[B, X, Y, Z\]"):
        mix(x[0])
    with pytest.raises(ValueError, match="requires grad"):
        mix(x.clone().requires_grad_(True))
    with pytest.raises(ValueError, match="empty input"):
        mix(x[:0])
    with pytest.raises(TypeError, match="expected a tensor"):
        mix([1.0])
    with pytest.raises(TypeError, match="augment must be a VolumeAugment"):
        mix(x, augment="crop")
    with pytest.raises(TypeError, match="step must be an integer"):
        mix(x, step=1.5)
    with pytest.raises(ValueError, match="B must be a positive integer"):
        mix.params(0, 0, (8, 8, 8))
    with pytest.raises(ValueError, match="roi must be positive"):
        mix.params(2, 0, (8, 0, 8))
    with pytest.raises(ValueError, match="come together"):
        mix.apply(x, torch.zeros(2, 12, dtype=torch.int32), augment=VolumeAugment(8))
    with pytest.raises(TypeError, match="step must be an integer") as err:      # a shared check reports under the class the caller used
        VolumeMix(mixup_alpha=0.4)(x, step="0")
    assert "VolumeMix" in str(err.value) and "VolumeAugment" not in str(err.value)


def test_cross_entropy_loss_and_train_step_validate_their_arguments():
    from neurovit_amd import ops
    from neurovit_amd.nn import CrossEntropyLoss
    from neurovit_amd.trainer import Trainer, class_weights_from_counts
    for eps, err in ((1.0, ValueError), (-0.1, ValueError), ("0.1", TypeError), (True, TypeError), (float("nan"), ValueError)):
        with pytest.raises(err, match="label_smoothing"):
            CrossEntropyLoss(label_smoothing=eps)
        with pytest.raises(err, match="label_smoothing"):
            ops.loss_opts(eps)
    with pytest.raises(ValueError, match="weight must be"):
        CrossEntropyLoss(weight=torch.ones(2, 2))
    with pytest.raises(ValueError, match="weight must be"):
        CrossEntropyLoss(weight=torch.ones(2, dtype=torch.int64))
    crit = CrossEntropyLoss(weight=[1, 3], label_smoothing=0.1)
    assert crit.weight.dtype == torch.float32 and crit.weight.tolist() == [1.0, 3.0] and crit.label_smoothing == 0.1
    assert CrossEntropyLoss().weight is None and CrossEntropyLoss().label_smoothing == 0.0
    with pytest.raises(RuntimeError, match="MI355X only"):
        crit(torch.zeros(2, 2), torch.zeros(2, dtype=torch.long))
    assert ops.loss_opts() is None and ops.loss_opts(0.0, None, None, 4, 2) is None          # every option off: no option block at all
    with pytest.raises(ValueError, match="class_weight must be"):
        ops.loss_opts(0.0, torch.ones(2, dtype=torch.float64))
    with pytest.raises(ValueError, match="2 entries for 3 classes"):
        ops.loss_opts(0.0, torch.ones(2), None, 4, 3)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.loss_opts(0.0, torch.ones(2))
    with pytest.raises(ValueError, match="mix must be"):
        ops.loss_opts(0.0, None, torch.zeros(4, 8, dtype=torch.int32))
    with pytest.raises(ValueError, match="3 rows for a batch of 4"):
        ops.loss_opts(0.0, None, torch.zeros(3, 12, dtype=torch.int32), 4)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.loss_opts(0.0, None, torch.zeros(4, 12, dtype=torch.int32), 4)
    # Trainer's keys
    assert Trainer.mix_from_config({}) is None and Trainer.loss_options_from_config({}) == (0.0, None)
    mix = Trainer.mix_from_config(dict(AUGMENT_CUTMIX_ALPHA=1.0, AUGMENT_MIX_PROB=0.5, AUGMENT_SEED=3))
    assert (mix.mixup_alpha, mix.cutmix_alpha, mix.prob, mix.switch_prob, mix.seed) == (None, 1.0, 0.5, 0.5, 3)
    with pytest.raises(ValueError, match="VolumeMix"):
        Trainer.mix_from_config(dict(AUGMENT_MIXUP_ALPHA=2.0))
    eps, w = Trainer.loss_options_from_config(dict(TRAINING_LABEL_SMOOTHING=0.1, TRAINING_CLASS_WEIGHTS=[2, 0.5]))
    assert eps == 0.1 and w.dtype == torch.float32 and w.tolist() == [2.0, 0.5]
    with pytest.raises(ValueError, match="finite and non-negative"):
        Trainer.loss_options_from_config(dict(TRAINING_CLASS_WEIGHTS=[1, -1]))
    with pytest.raises(TypeError, match="list of numbers"):
        Trainer.loss_options_from_config(dict(TRAINING_CLASS_WEIGHTS=3))
    assert class_weights_from_counts([10, 30]) == [40 / 20, 40 / 60]
    assert class_weights_from_counts([5, 5, 5]) == [1.0, 1.0, 1.0]
    with pytest.raises(ValueError, match="positive and finite"):
        class_weights_from_counts([3, 0])
