"""On-device training augmentation on MI355X: the kernels of csrc/augment.hip (nv_augment_params, nv_augment_apply) against their CPU
restatement (tests/augment_ref.py, itself checked in tests/test_augment_cpu.py), VolumeAugment's call protocol, and the Trainer shell
with DATASET_TRANSFORMS.  Every comparison is torch.equal on int32 patterns unless a comment says otherwise."""
import itertools

import numpy as np
import pytest
import torch

import augment_ref as R
import weights as W
from augment_inputs import SPAN_SHAPES, layouts, sentinel_out, sentinels_intact, special_volume

pytestmark = pytest.mark.gpu

ONE, ZERO = 0x3F800000, 0
SCALE, SHIFT = torch.tensor([0.75, -0.3]).view(torch.int32).tolist()


@pytest.fixture(scope="module")
def VA():
    from neurovit_amd._cabi import require_gpu
    require_gpu()
    from neurovit_amd.augment import VolumeAugment
    return VolumeAugment


def same_bits_or_both_nan(got, want):
    """NaN-aware: where the restatement has a NaN the kernel has one (payloads need not agree behind arithmetic), every other cell bit for bit"""
    nan = want.isnan()
    return torch.equal(got.isnan(), nan) and torch.equal(R.bits(got)[~nan], R.bits(want)[~nan])


# ------------------------------------------------------------------ parameters
MODES = {"crop": dict(), "all": dict(flip_prob=(0.5, 0.25, 1.0), max_shift=(3, 0, 17), scale=(0.9, 1.1), shift=(-0.25, 0.125))}


@pytest.mark.parametrize("mode", sorted(MODES))
@pytest.mark.parametrize("B", [1, 3, 257])
def test_params_equal_the_restatement(VA, B, mode):
    in_size, roi = (90, 91, 109), (80, 80, 80)
    for seed, step, rank in itertools.product((0, 0xDEADBEEFCAFEF00D), (0, 2 ** 20 + 3), (0, 5)):
        aug = VA(roi, seed=seed, rank=rank, **MODES[mode])
        got = aug.params(B, step, in_size=in_size)
        assert got.dtype == torch.int32 and got.shape == (B, 8) and got.is_cuda
        want = R.params_ref(B, step, in_size, roi, seed=seed, rank=rank, **MODES[mode])
        assert torch.equal(got.cpu(), want), (seed, step, rank)
    if mode == "crop":
        assert (got[:, 3:].cpu() == torch.tensor([0, ONE, ZERO, 0, 0])).all()


# ------------------------------------------------------------------ apply, hand-written parameter tables
IN = (23, 21, 22)


def param_rows(roi):
    """offsets x flips: the eight corners under each of the eight flip combinations; windows pushed partly outside on each side of each
    axis, and wholly outside (all `fill`), cycling through the flips"""
    hi = [n - s for n, s in zip(IN, roi)]
    rows = [[*(h * c for h, c in zip(hi, corner)), f] for corner in itertools.product((0, 1), repeat=3) for f in range(8)]
    part = [(-3, 1, 1), (hi[0] + 2, 0, 2), (1, -5, 0), (2, hi[1] + 4, 1), (0, 1, -1), (1, 2, hi[2] + 6), (-2, hi[1] + 1, -7), (hi[0] + 1, -1, hi[2] + 1),
            (1, 1, -3), (1, 1, hi[2] + 3), (1, 1, -4), (1, 1, hi[2] + 4)]
    whole = [(-roi[0], 0, 0), (IN[0], 1, 1), (0, -roi[1] - 3, 0), (1, IN[1], 0), (0, 0, -roi[2]), (1, 1, IN[2] + 5), (-40, 50, -60)]
    rows += [[*o, (r + f) % 8] for r, o in enumerate(part) for f in (0, 4, 7)]
    rows += [[*o, r % 8] for r, o in enumerate(whole)]
    return rows, len(whole)


@pytest.fixture(scope="module")
def volumes():
    return layouts()


@pytest.mark.parametrize("layout", ["view", "dense", "moved"])
@pytest.mark.parametrize("S", [18, 17, 20])
def test_apply_hand_written_tables(VA, volumes, S, layout):
    host, on_device = volumes
    x = on_device[layout](lambda t: t.cuda())
    assert tuple(x.shape) == (3, *IN) and x.is_cuda
    roi = (S, S, S)
    rows, n_whole = param_rows(roi)
    fill = -2.5
    aug = VA(roi, fill=fill)
    rows += [rows[-1]] * (-len(rows) % 3)
    for intensity in ((ONE, ZERO), (SCALE, SHIFT)):
        table = torch.tensor([[*r, *intensity, 0, 0] for r in rows], dtype=torch.int32)
        for first in range(0, len(rows), 3):
            params = table[first:first + 3]
            got = aug.apply(x, params.cuda())
            assert got.shape == (3, *roi) and got.is_contiguous() and got.dtype == torch.float32
            want = R.apply_ref(host, params, roi, fill)
            if intensity == (ONE, ZERO):
                assert torch.equal(R.bits(got.cpu()), R.bits(want)), (first, params.tolist())     # a bit copy: payloads, -0.0
            else:
                assert same_bits_or_both_nan(got.cpu(), want), (first, params.tolist())
    tail = torch.tensor([[*r, SCALE, SHIFT, 0, 0] for r in rows[-3:]], dtype=torch.int32)          # wholly outside: the fill, verbatim
    assert n_whole >= 3 and (aug.apply(x, tail.cuda()) == fill).all()


@pytest.mark.parametrize("S", [17, 20])
def test_apply_writes_nothing_outside_out(VA, volumes, S):
    host, on_device = volumes
    x = on_device["view"](lambda t: t.cuda())
    roi, n = (S, S, S), 3 * S ** 3
    buf = torch.full((64 + n + 64,), 0x7FC0BEEF, dtype=torch.int32, device="cuda").view(torch.float32)      # 64 sentinel floats on both sides
    out = buf[64:64 + n].view(3, *roi)
    params = torch.tensor([[2, 1, 3, 5, ONE, ZERO, 0, 0], [-4, 2, 1, 2, SCALE, SHIFT, 0, 0], [30, 0, 0, 0, ONE, ZERO, 0, 0]], dtype=torch.int32)
    aug = VA(roi, fill=1.5)
    assert aug.apply(x, params.cuda(), out=out) is out
    edges = R.bits(torch.cat([buf[:64], buf[64 + n:]]).cpu())
    assert (edges == 0x7FC0BEEF).all()
    assert same_bits_or_both_nan(out.cpu(), R.apply_ref(host, params, roi, 1.5))
    for bad in (buf[63:63 + n].view(3, *roi), torch.empty(3, S, S, S + 1, device="cuda"), torch.empty(3, *roi, device="cuda", dtype=torch.float64),
                torch.empty(3, S, S, 2 * S, device="cuda")[..., ::2]):
        with pytest.raises(ValueError, match="out must be"):
            aug.apply(x, params.cuda(), out=bad)


# ------------------------------------------------------------------ 4D series
@pytest.mark.parametrize("T", [1, 4, 5])
def test_series_share_their_samples_parameters(VA, T):
    g = torch.Generator().manual_seed(40 + T)
    series = torch.randn(2, 13, 12, 11, T, generator=g)
    roi = (8, 8, 8)
    aug = VA(roi, fill=0.5)
    tables = [[[5, 4, 3, 0, ONE, ZERO, 0, 0], [0, 0, 0, 4, ONE, ZERO, 0, 0]],                       # runs of memory forwards, a flipped series
              [[2, -1, 1, 3, SCALE, SHIFT, 0, 0], [-3, 2, 6, 7, SCALE, SHIFT, 0, 0]],
              [[1, 1, -2, 2, ONE, ZERO, 0, 0], [0, 20, 0, 1, SCALE, SHIFT, 0, 0]]]
    x = series.cuda()
    strided = torch.zeros(2, 13, 12, 11, 2 * T).cuda()[..., ::2].copy_(x)                            # time is not dense: cell by cell
    for rows in tables:
        params = torch.tensor(rows, dtype=torch.int32)
        got = aug.apply(x, params.cuda())
        assert got.shape == (2, 8, 8, 8, T) and got.is_contiguous()
        assert torch.equal(R.bits(got.cpu()), R.bits(R.apply_ref(series, params, roi, 0.5))), rows
        assert torch.equal(R.bits(aug.apply(strided, params.cuda())), R.bits(got))
        for t in range(T):                                                                          # the 3D apply of each timepoint, same rows
            assert torch.equal(R.bits(aug.apply(x[..., t], params.cuda())), R.bits(got[..., t])), (rows, t)


# ------------------------------------------------------------------ a plane of more than one span
# (the planes of more than 4096 cells, one workgroup's span: SPAN_SHAPES in tests/augment_inputs.py)
def span_rows():
    """for both shapes (X - Sx, Y - Sy, Z - Sz) = (2, 3, 3): z flips, windows that leave the volume on the low and on the high side of
    every axis (one plane wholly outside), an intensity change on some samples"""
    return [[[1, 2, 1, 4, ONE, ZERO, 0, 0], [-1, -2, -3, 0, SCALE, SHIFT, 0, 0], [3, 5, 5, 7, ONE, ZERO, 0, 0]],
            [[0, 0, 0, 0, ONE, ZERO, 0, 0], [2, 3, 3, 4, SCALE, SHIFT, 0, 0], [1, -2, 6, 6, SCALE, SHIFT, 0, 0]]]


@pytest.mark.parametrize("case", sorted(SPAN_SHAPES))
def test_apply_reaches_a_second_span(VA, case):
    shape, roi = SPAN_SHAPES[case]
    host = special_volume(shape, 61)
    x = host.cuda()
    aug = VA(roi, fill=-2.5)
    buf, out = sentinel_out((3, *roi, *shape[4:]))
    assert int(np.prod(out.shape[2:])) > 4096
    for rows in span_rows():
        params = torch.tensor(rows, dtype=torch.int32)
        assert aug.apply(x, params.cuda(), out=out) is out
        assert sentinels_intact(buf), rows
        got, want = out.cpu(), R.apply_ref(host, params, roi, -2.5)
        for b, row in enumerate(rows):
            if row[4:6] == [ONE, ZERO]:
                assert torch.equal(R.bits(got[b]), R.bits(want[b])), (rows, b)                       # a bit copy: payloads, -0.0
            else:
                assert same_bits_or_both_nan(got[b], want[b]), (rows, b)


# ------------------------------------------------------------------ the call protocol
def test_call_draws_applies_and_counts(VA):
    g = torch.Generator().manual_seed(8)
    host = torch.randn(5, 14, 13, 12, generator=g)
    x = host.cuda()
    kw = dict(flip_prob=(0.5, 0.5, 0.5), max_shift=(2, 2, 2), scale=(0.8, 1.2), shift=(-0.1, 0.1), fill=-1.0, seed=77, rank=2)
    aug = VA((9, 10, 11), **kw)
    assert aug.step == 0 and aug.last_params is None
    outs = []
    for n in range(3):
        out = aug(x)
        assert aug.step == n + 1                                                                    # the counter advances by one per call
        assert torch.is_tensor(aug.last_params) and aug.last_params.is_cuda and aug.last_params.dtype == torch.int32
        params = aug.params(5, n, in_size=(14, 13, 12))
        assert torch.equal(aug.last_params, params)
        assert torch.equal(R.bits(out), R.bits(aug.apply(x, params)))
        assert torch.equal(params.cpu(), R.params_ref(5, n, (14, 13, 12), (9, 10, 11), **{k: v for k, v in kw.items() if k != "fill"}))
        assert torch.equal(R.bits(out.cpu()), R.bits(R.apply_ref(host, params.cpu(), (9, 10, 11), -1.0)))
        outs.append(out)
    assert not torch.equal(outs[0], outs[1])
    again = aug(x, step=1)                                                                          # a past batch, the counter stays
    assert aug.step == 3 and torch.equal(R.bits(again), R.bits(outs[1]))
    # 4D: the same rows for a series
    s = torch.stack([x, 2 * x], dim=-1)
    o4 = aug(s, step=0)
    assert o4.shape == (5, 9, 10, 11, 2) and torch.equal(R.bits(o4[..., 0]), R.bits(outs[0]))


def test_identity_configuration_returns_its_input(VA):
    x = torch.randn(2, 8, 8, 8, device="cuda")
    aug = VA(8)
    assert aug(x) is x and aug.last_params is None and aug.step == 1
    view = torch.randn(2, 9, 9, 9, device="cuda")[:, 1:, 1:, 1:]
    assert aug(view) is view
    s = torch.randn(2, 8, 8, 8, 3, device="cuda")
    assert aug(s) is s
    crop = aug(torch.randn(2, 9, 8, 8, device="cuda"))                                              # a larger input: the crop is on
    assert crop.shape == (2, 8, 8, 8) and aug.last_params is not None
    assert VA(8, flip_prob=(0, 0, 1.0))(x) is not x


# ------------------------------------------------------------------ the Trainer shell
class Volumes40(torch.utils.data.Dataset):
    """DatasetADNI's 7-tuples with UNCROPPED volumes: six 40^3 volumes for a 32^3 model"""

    def __init__(self):
        self.x = W.make_volume((6, 40, 40, 40), 4)
        self.y = torch.tensor([0, 1, 1, 0, 1, 0])

    def __len__(self):
        return 6

    def __getitem__(self, i):
        return f"s{i}", torch.tensor(0), self.x[i], torch.tensor(0), torch.tensor(1), torch.tensor(70), self.y[i]


def trainer_config(tmp_path, **extra):
    size = dict(TRAINING_VIT_DIM=128, TRAINING_VIT_DEPTH=2, TRAINING_VIT_HEADS=2, TRAINING_VIT_MLP_DIM=256)
    return W.neuro_config(32, 8, DEVICE="cuda", TRAINING_LEARNING_RATE=1e-3, TRAINING_WEIGHT_DECAY=1e-2, GLOBAL_OUTPUT_DIR=str(tmp_path / "runs"),
                          TRAINING_EPOCHS=1, TRAINING_BATCH_SIZE=2, TRAINING_NUM_WORKERS=0, **size, **extra)


def test_trainer_augments_training_batches_and_centres_validation(VA, tmp_path):
    from neurovit_amd.NeuroEncoder import NeuroEncoder
    from neurovit_amd.augment import center_window
    from neurovit_amd.trainer import Trainer
    flips = (0.5, 0.5, 0.5)
    cfg = trainer_config(tmp_path, DATASET_TRANSFORMS=True, AUGMENT_FLIP_PROB=flips, AUGMENT_SEED=13)
    torch.manual_seed(5)
    model = NeuroEncoder(cfg)
    data = Volumes40()
    tr = Trainer(cfg, model, data, data)
    assert isinstance(tr.augment, VA) and tr.augment.roi == (32, 32, 32) and tr.augment.rank == 0
    seen, losses = [], []
    real, run = tr.augment, tr.step._step

    class Spy:
        roi = real.roi

        def __call__(self, x, step=None):
            out = real(x, step=step)
            seen.append((step, tuple(x.shape), tuple(out.shape), real.last_params.clone()))
            return out

    def step_spy(fmri, labels):
        loss = run(fmri, labels)
        losses.append((tuple(fmri.shape), loss))
        return loss
    tr.augment, tr.step._step = Spy(), step_spy
    tr.train(0)
    assert [s[0] for s in seen] == [0, 1, 2] and tr.global_step == 3
    assert len(losses) == 3 and all(shape == (2, 32, 32, 32) and torch.isfinite(loss).item() for shape, loss in losses)
    for step, shape_in, shape_out, params in seen:
        assert shape_in == (2, 40, 40, 40) and shape_out == (2, 32, 32, 32) and params.is_cuda
        assert torch.equal(params.cpu(), R.params_ref(2, step, (40, 40, 40), (32, 32, 32), flip_prob=flips, seed=13)), step
    # validation: the centre window of every batch, in the loader's order
    outputs = []
    hook = model.register_forward_hook(lambda m, args, out: outputs.append((tuple(args[0].shape), out.detach().clone())))
    loss, acc = tr.validate(0)
    hook.remove()
    assert np.isfinite(loss) and len(outputs) == 3
    model.eval()
    with torch.no_grad(), model.precision(tr.validation_precision):
        for n, (shape, logits) in enumerate(outputs):
            batch = data.x[2 * n:2 * n + 2].cuda()
            window = center_window(batch, (32, 32, 32))
            assert shape == (2, 32, 32, 32) and torch.equal(window, batch[:, 4:36, 4:36, 4:36])
            assert torch.equal(logits, model(window.contiguous())), n                                 # the same values through the same kernels
    acc1, wrong = tr.evaluate_samples()
    assert 0.0 <= acc1 <= 100.0


def test_trainer_without_the_key_keeps_the_shape_error(VA, tmp_path):
    from neurovit_amd.NeuroEncoder import NeuroEncoder
    from neurovit_amd.trainer import Trainer
    for extra in ({}, {"DATASET_TRANSFORMS": False}):
        cfg = trainer_config(tmp_path, **extra)
        tr = Trainer(cfg, NeuroEncoder(cfg), Volumes40(), Volumes40())
        assert tr.augment is None
        with pytest.raises(ValueError, match="expected video"):
            tr.train(0)
