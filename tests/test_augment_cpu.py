"""CPU checks of the on-device training augmentation (no GPU): the C-ABI pieces csrc/augment.hip adds within revision 8
(nv_augment_params, nv_augment_apply), the refusals of neurovit_amd.augment.VolumeAugment, and the CPU restatement
(tests/augment_ref.py) that the GPU tests (tests/test_augment_gpu.py) hold the kernels to:

  restatement    apply_ref against an independent formulation (torch.flip, F.pad(value=fill), slicing) on a 7 x 6 x 5 volume: every flip
                 combination, windows inside, partly outside on either side and wholly outside;
  crop only      a crop-only output is x[b, ox:ox+S, oy:oy+S, oz:oz+S] with every offset in range: the windows RandSpatialCrop produces;
  uniformity     4096 draws per axis at the reference's 90 -> 80 geometry: all 11 offsets occur, each 262 .. 483 times (binomial mean 372.4
                 +- 6 sigma, sigma 18.4); a flip at p = 0.5 lands 1856 .. 2240 times in 4096 draws (2048 +- 6 * 32);
  seeding        two ranks with one seed and step differ, the same rank reproduces;
  refusals       every argument error of VolumeAugment and of the two entry points is raised without a device.
"""
import ctypes
import itertools

import pytest
import torch
import torch.nn.functional as F

import augment_ref as R

NAMES = ("nv_augment_params", "nv_augment_apply")


# ------------------------------------------------------------------ symbols and ABI
def test_header_declares_and_library_exports_the_new_entry_points():
    from neurovit_amd import _cabi
    dll = ctypes.CDLL(_cabi.LIB_PATH)
    for name in NAMES:
        assert name in _cabi.lib.protos, name            # declared in the header
        assert getattr(dll, name) is not None, name      # exported by the library
    protos = _cabi.lib.protos
    assert protos["nv_augment_params"][1][1] is ctypes.c_ulong and protos["nv_augment_params"][1][2] is ctypes.c_ulong
    assert protos["nv_augment_apply"][1][7] is ctypes.c_float
    assert _cabi.ABI_VERSION == 8 and dll.nv_abi_version() == 8          # new symbols only
    assert "#define NV_ABI_VERSION 8" in open(_cabi.HEADER).read()


def test_the_package_exports_volume_augment():
    import neurovit_amd
    from neurovit_amd.augment import VolumeAugment
    assert neurovit_amd.VolumeAugment is VolumeAugment


def make_config(**kw):
    from neurovit_amd.augment import AugmentConfig
    cfg = AugmentConfig(ctypes.sizeof(AugmentConfig), (ctypes.c_int * 3)(90, 90, 90), (ctypes.c_int * 3)(80, 80, 80), (ctypes.c_int * 3)(0, 0, 0),
                        (ctypes.c_double * 3)(0, 0, 0), 1.0, 1.0, 0.0, 0.0)
    for k, v in kw.items():
        setattr(cfg, k, v)
    return cfg


def test_entry_points_check_their_arguments_without_a_gpu():
    from neurovit_amd import _cabi
    from neurovit_amd._cabi import lib
    from neurovit_amd.augment import AugmentConfig
    assert ctypes.sizeof(AugmentConfig) == 80
    fake = 4096                                            # a non-null, 16-byte aligned address nothing dereferences: the checks come first
    i3 = lambda *v: (ctypes.c_int * 3)(*v)
    params = lambda cfg, B=2, rank=0, out=fake: lib.nv_augment_params(ctypes.byref(cfg) if cfg is not None else None, 1, 0, rank, B, out, None)
    assert params(None) == -1
    assert params(make_config(), out=None) == -1
    assert params(make_config(), B=0) == -1
    assert params(make_config(), rank=-1) == -1
    assert params(make_config(struct_size=76)) == -1 and "struct_size" in _cabi.last_error()
    assert params(make_config(roi=i3(80, 91, 80))) == -1 and "larger" in _cabi.last_error()
    assert params(make_config(roi=i3(80, -1, 80))) == -1 and "positive" in _cabi.last_error()
    assert params(make_config(in_size=i3(-90, 90, 90))) == -1
    assert params(make_config(max_shift=i3(0, 0, -1))) == -1 and "max_shift" in _cabi.last_error()
    assert params(make_config(flip_prob=(ctypes.c_double * 3)(0, 1.5, 0))) == -1 and "probability" in _cabi.last_error()
    assert params(make_config(flip_prob=(ctypes.c_double * 3)(-0.1, 0, 0))) == -1
    assert params(make_config(flip_prob=(ctypes.c_double * 3)(float("nan"), 0, 0))) == -1
    assert params(make_config(scale_lo=1.5, scale_hi=0.5)) == -1 and "lo <= hi" in _cabi.last_error()
    assert params(make_config(shift_lo=0.5, shift_hi=-0.5)) == -1

    strides = (ctypes.c_long * 5)(8100, 90, 1, 0, 0)
    sp = ctypes.cast(strides, ctypes.c_void_p)
    p3 = lambda *v: ctypes.cast(i3(*v), ctypes.c_void_p)

    def apply(src=fake, st=sp, B=2, in3=(90, 90, 90), T=1, prm=fake, roi3=(80, 80, 80), out=fake):
        return lib.nv_augment_apply(src, st, B, p3(*in3), T, prm, p3(*roi3), 0.0, out, None)
    for kw in (dict(src=None), dict(st=None), dict(prm=None), dict(out=None), dict(B=0), dict(B=-3), dict(T=0)):
        assert apply(**kw) == -1, kw
    assert apply(roi3=(80, 80, 91)) == -1 and "larger" in _cabi.last_error()
    assert apply(roi3=(0, 80, 80)) == -1 and "positive" in _cabi.last_error()
    assert apply(in3=(90, -90, 90)) == -1 and "positive" in _cabi.last_error()
    assert apply(out=fake + 4) == -1 and "16-byte" in _cabi.last_error()
    assert apply(in3=(9000, 9000, 9000), roi3=(80, 8000, 8000), T=64) == -1 and "beyond one launch" in _cabi.last_error()


# ------------------------------------------------------------------ the restatement against an independent formulation
def apply_by_padding(x, params, roi, fill):
    """flip the window, not the index: pad every axis by P with `fill`, slice the window at o + P, flip the flagged axes"""
    P = 16
    out = []
    for b in range(x.shape[0]):
        ox, oy, oz, flips = params[b, :4].tolist()
        padded = F.pad(x[b], (P, P, P, P, P, P), value=fill)
        w = padded[ox + P:ox + P + roi[0], oy + P:oy + P + roi[1], oz + P:oz + P + roi[2]]
        out.append(torch.flip(w, [a for a in range(3) if (flips >> a) & 1]))
    return torch.stack(out)


def volume_765(B):
    g = torch.Generator().manual_seed(765)
    return torch.randn(B, 7, 6, 5, generator=g)


ONE, ZERO = 0x3F800000, 0


@pytest.mark.parametrize("roi", [(4, 3, 2), (7, 6, 5), (5, 5, 5)])
def test_restatement_equals_flip_pad_slice(roi):
    offsets = [(0, 0, 0), (7 - roi[0], 6 - roi[1], 5 - roi[2]), (1, 0, 0), (-2, 1, 0), (2, -3, 1), (0, 1, -4), (4, 0, 0), (0, 5, 0), (0, 0, 4),
               (-roi[0], 0, 0), (0, 6, 0), (1, 1, -roi[2]), (9, 9, 9), (-9, 2, 1)]                  # inside, partly outside on either side, wholly outside
    rows = [[*o, f, ONE, ZERO, 0, 0] for o in offsets for f in range(8)]
    params = torch.tensor(rows, dtype=torch.int32)
    x = volume_765(1).expand(len(rows), -1, -1, -1)
    for fill in (0.0, -7.5):
        got, want = R.apply_ref(x, params, roi, fill), apply_by_padding(x, params, roi, fill)
        assert torch.equal(R.bits(got), R.bits(want))
    whole = [r for r, o in enumerate(offsets) if o in ((-roi[0], 0, 0), (0, 6, 0), (1, 1, -roi[2]), (9, 9, 9), (-9, 2, 1))]
    got = R.apply_ref(x, params, roi, -7.5).view(len(offsets), 8, *roi)
    assert (got[whole] == -7.5).all()


def test_restatement_intensity_and_series():
    x = volume_765(2)
    half, quarter = torch.tensor([0.5, 0.25]).view(torch.int32).tolist()
    params = torch.tensor([[1, 0, -1, 5, half, quarter, 0, 0], [-1, 2, 1, 2, ONE, ZERO, 0, 0]], dtype=torch.int32)
    got = R.apply_ref(x, params, (4, 3, 2), fill=9.0)
    want = apply_by_padding(x, params, (4, 3, 2), float("nan"))
    want[0] = want[0] * 0.5 + 0.25                          # the fill is written verbatim, not scaled
    want = torch.where(want.isnan(), torch.tensor(9.0), want)
    assert torch.equal(R.bits(got), R.bits(want))
    # a series shares its sample's row: timepoint t of the result is the 3D result of timepoint t
    series = torch.stack([x, -x, 2 * x], dim=-1)
    got4 = R.apply_ref(series, params, (4, 3, 2), fill=9.0)
    assert got4.shape == (2, 4, 3, 2, 3)
    for t in range(3):
        assert torch.equal(R.bits(got4[..., t]), R.bits(R.apply_ref(series[..., t], params, (4, 3, 2), fill=9.0)))


def test_identity_intensity_is_a_bit_copy_in_the_restatement():
    patterns = torch.tensor([0x7FC00123, -0x7FFFFFFF - 1, 0x7F800000, -0x00800000, 0x7F800001, 1], dtype=torch.int32)   # NaN payloads, -0.0, +-inf, a denormal
    x = patterns.repeat(35)[:7 * 6 * 5].view(torch.float32).view(1, 7, 6, 5)
    params = torch.tensor([[1, 1, 1, 7, ONE, ZERO, 0, 0]], dtype=torch.int32)
    got = R.apply_ref(x, params, (5, 4, 3))
    want = torch.flip(R.bits(x)[:, 1:6, 1:5, 1:4], [1, 2, 3])
    assert torch.equal(R.bits(got), want)


def test_crop_only_outputs_are_the_windows_of_rand_spatial_crop():
    B, X, S = 64, (7, 6, 5), (4, 4, 3)
    x = volume_765(B)
    params = R.params_ref(B, 3, X, S, seed=11)
    assert (params[:, 3:] == torch.tensor([0, ONE, ZERO, 0, 0])).all()
    got = R.apply_ref(x, params, S)
    seen = set()
    for b in range(B):
        ox, oy, oz = params[b, :3].tolist()
        assert 0 <= ox <= X[0] - S[0] and 0 <= oy <= X[1] - S[1] and 0 <= oz <= X[2] - S[2]
        assert torch.equal(got[b], x[b, ox:ox + S[0], oy:oy + S[1], oz:oz + S[2]])
        seen.add((ox, oy, oz))
    assert len(seen) > 12                                   # 4 * 3 * 3 = 36 windows exist


# ------------------------------------------------------------------ distribution and seeding
def test_crop_offsets_are_uniform_at_the_reference_geometry():
    """90 -> 80: 11 offsets per axis, 4096 draws per axis: each count within binomial mean 372.4 +- 6 sigma (sigma 18.4) = 262 .. 483"""
    params = R.params_ref(4096, 0, (90, 90, 90), (80, 80, 80), seed=2024)
    for a in range(3):
        counts = torch.bincount(params[:, a].long(), minlength=11)
        print(f"axis {a}: counts {counts.tolist()}")
        assert counts.numel() == 11 and counts.min().item() >= 262 and counts.max().item() <= 483, (a, counts.tolist())
    assert (params[:, 3] == 0).all()


def test_flips_at_one_half_are_fair_and_certain_at_the_ends():
    """p = 0.5 over 4096 draws: 2048 +- 6 * 32 = 1856 .. 2240 per axis; p = 0 never, p = 1 always"""
    params = R.params_ref(4096, 7, (90, 90, 90), (80, 80, 80), flip_prob=(0.5, 0.5, 0.5), seed=5)
    for a in range(3):
        n = ((params[:, 3] >> a) & 1).sum().item()
        print(f"axis {a}: {n} flips of 4096")
        assert 1856 <= n <= 2240, (a, n)
    ends = R.params_ref(512, 7, (90, 90, 90), (80, 80, 80), flip_prob=(0.0, 1.0, 0.0), seed=5)
    assert (ends[:, 3] == 2).all()


def test_shifts_and_intensities_stay_in_their_ranges():
    params = R.params_ref(1024, 1, (90, 90, 90), (80, 80, 80), max_shift=(3, 0, 12), scale=(0.9, 1.1), shift=(-0.1, 0.2), seed=9)
    assert params[:, 0].min().item() >= -3 and params[:, 0].max().item() <= 13 and params[:, 0].min().item() < 0 and params[:, 0].max().item() > 10
    assert params[:, 1].min().item() >= 0 and params[:, 1].max().item() <= 10
    assert params[:, 2].min().item() >= -12 and params[:, 2].max().item() <= 22
    scale, shift = params[:, 4].contiguous().view(torch.float32), params[:, 5].contiguous().view(torch.float32)
    lo, hi = torch.tensor([0.9, 1.1])
    assert scale.min() >= lo and scale.max() <= hi + 2.0 ** -23 and scale.max() - scale.min() > 0.15
    assert shift.min() >= -0.1 and shift.max() <= 0.2 + 2.0 ** -24 and shift.max() - shift.min() > 0.2
    assert (params[:, 6:] == 0).all()


def test_ranks_differ_and_a_rank_reproduces():
    kw = dict(in_size=(90, 90, 90), roi=(80, 80, 80), flip_prob=(0.5, 0.5, 0.5), scale=(0.9, 1.1), seed=3)
    a = R.params_ref(16, 5, rank=0, **kw)
    assert torch.equal(a, R.params_ref(16, 5, rank=0, **kw))
    assert not torch.equal(a, R.params_ref(16, 5, rank=1, **kw))
    assert not torch.equal(a, R.params_ref(16, 6, rank=0, **kw))
    assert not torch.equal(a, R.params_ref(16, 5, rank=0, **dict(kw, seed=4)))
    assert not torch.equal(a[0], a[1])
    # a longer batch extends a shorter one: the counter is (step, sample), not the batch
    assert torch.equal(a[:4], R.params_ref(4, 5, rank=0, **kw))


# ------------------------------------------------------------------ refusals, without a device
def test_volume_augment_refuses_bad_configurations():
    from neurovit_amd.augment import VolumeAugment
    for kw in (dict(flip_prob=(0, 1.5, 0)), dict(flip_prob=(-0.1, 0, 0)), dict(max_shift=(0, -1, 0)), dict(scale=(1.2, 0.8)), dict(shift=(0.1, -0.1)),
               dict(flip_prob=(0.5, 0.5)), dict(scale=(float("nan"), 1.0)), dict(seed=-1), dict(rank=-1)):
        with pytest.raises(ValueError):
            VolumeAugment(8, **kw)
    for roi in (0, (8, 8), (8, -8, 8)):
        with pytest.raises(ValueError):
            VolumeAugment(roi)
    for kw in (dict(max_shift=(0.5, 0, 0)), dict(seed=1.5), dict(scale=1.0)):
        with pytest.raises(TypeError):
            VolumeAugment(8, **kw)
    aug = VolumeAugment(8, flip_prob=0.5, max_shift=2)
    assert aug.roi == (8, 8, 8) and aug.flip_prob == (0.5, 0.5, 0.5) and aug.max_shift == (2, 2, 2)


def test_volume_augment_refuses_bad_inputs_before_any_device_work():
    from neurovit_amd.augment import VolumeAugment
    aug = VolumeAugment(8, flip_prob=(0.5, 0, 0))
    x = torch.zeros(2, 10, 10, 10)
    params = torch.zeros(2, 8, dtype=torch.int32)
    for call in (lambda t: aug(t), lambda t: aug.apply(t, params)):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            call(x)
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            call(torch.zeros(2, 10, 10, 10, 3))
        with pytest.raises(ValueError, match="requires grad"):
            call(x.clone().requires_grad_())
        for dtype in (torch.float64, torch.float16, torch.bfloat16, torch.int16):
            with pytest.raises(TypeError, match="dtype"):
                call(x.to(dtype))
        with pytest.raises(ValueError, match="larger than the input"):
            call(torch.zeros(2, 10, 7, 10))
        with pytest.raises(ValueError, match="expected"):
            call(torch.zeros(10, 10, 10))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        VolumeAugment(10)(x)                                # the identity configuration has no CPU form either
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        aug.params(2, 0, device="cpu")
    with pytest.raises(ValueError, match="larger than the input"):
        aug.params(2, 0, in_size=(8, 7, 8))
    for step in (-1, 2 ** 64):
        with pytest.raises(ValueError, match="step"):
            aug.params(2, step)
    with pytest.raises(TypeError, match="step"):
        aug.params(2, 1.0)
    assert aug.step == 0 and aug.last_params is None


def test_trainer_reads_the_config_keys():
    from neurovit_amd.trainer import Trainer
    base = dict(TRAINING_VIT_INPUT_SIZE=32)
    assert Trainer.augment_from_config(base) is None and Trainer.augment_from_config(dict(base, DATASET_TRANSFORMS=False)) is None
    plain = Trainer.augment_from_config(dict(base, DATASET_TRANSFORMS=True))
    assert plain.roi == (32, 32, 32) and plain._transforms_off() and plain.rank == 0 and plain.seed == 0 and plain.fill == 0.0
    full = Trainer.augment_from_config(dict(base, DATASET_TRANSFORMS=True, AUGMENT_FLIP_PROB=(0.5, 0, 0), AUGMENT_MAX_SHIFT=2,
                                            AUGMENT_INTENSITY_SCALE=(0.9, 1.1), AUGMENT_INTENSITY_SHIFT=(-0.1, 0.1), AUGMENT_FILL=-1.0, AUGMENT_SEED=7))
    assert full.flip_prob == (0.5, 0.0, 0.0) and full.max_shift == (2, 2, 2) and full.fill == -1.0 and full.seed == 7
    assert abs(full.scale[0] - 0.9) < 1e-7 and abs(full.shift[1] - 0.1) < 1e-7
    with pytest.raises(ValueError):
        Trainer.augment_from_config(dict(base, DATASET_TRANSFORMS=True, AUGMENT_FLIP_PROB=(2, 0, 0)))


def test_center_window_is_a_view_at_the_middle_offset():
    from neurovit_amd.augment import center_window
    x = torch.arange(2 * 9 * 8 * 7, dtype=torch.float32).view(2, 9, 8, 7)
    w = center_window(x, (4, 4, 4))
    assert torch.equal(w, x[:, 2:6, 2:6, 1:5]) and w.data_ptr() == x[:, 2:, 2:, 1:].data_ptr()
    assert center_window(x, (9, 8, 7)) is x
    s = torch.zeros(2, 9, 8, 7, 3)
    assert center_window(s, (4, 4, 4)).shape == (2, 4, 4, 4, 3)
    with pytest.raises(ValueError):
        center_window(x, (10, 4, 4))
