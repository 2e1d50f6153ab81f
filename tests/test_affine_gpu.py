"""Random affine augmentation on MI355X: the kernels of csrc/affine.hip (nv_affine_params, nv_affine_apply) against their CPU restatement
(tests/affine_ref.py, itself checked in tests/test_affine_cpu.py), VolumeAffine's call protocol, its composition with VolumeMix, and the
Trainer shell with the AUGMENT_ROTATE_DEG / _ZOOM / _TRANSLATE keys.  nv_affine_apply is held to the restatement BIT FOR BIT under the
same table (torch.equal on int32 patterns; the volumes hold normal values, so no NaN arises behind arithmetic) - tests/test_affine_cpu.py
shows that a fused lerp, another lerp order or an incremental coordinate would fail that gate on these inputs.  The tables of
nv_affine_params are formed in double with the device's sin / cos: their integer columns and unapplied rows are exact, a matrix entry
agrees within adjacent fp32 patterns, or within 2^-40 absolutely when it is below 2^-10 (the rotation products cancel there, and two
libraries' sin / cos agree to an absolute error, not a relative one)."""
import numpy as np
import pytest
import torch

import affine_ref as R
import augment_ref as A
import weights as W
from augment_inputs import SPAN_SHAPES, layouts, sentinel_out, sentinels_intact, special_volume

pytestmark = pytest.mark.gpu

ONE, ZERO = R.ONE, R.ZERO
SCALE, SHIFT = torch.tensor([0.75, -0.3]).view(torch.int32).tolist()
FILL = -2.5


@pytest.fixture(scope="module")
def VF():
    from neurovit_amd._cabi import require_gpu
    require_gpu()
    from neurovit_amd.augment import VolumeAffine
    return VolumeAffine


# ------------------------------------------------------------------ tables
KW = dict(rotate=(10, 5, 20), zoom=(0.9, 1.1), isotropic=False, translate=(4, 0.5, 2), prob=0.5, flip_prob=(0.5, 0.25, 1.0), scale=(0.9, 1.1),
          shift=(-0.25, 0.125))


def ordered(bits):
    """int32 patterns of fp32 -> integers in the order of the values (adjacent floats differ by one; +-0.0 coincide)"""
    b = bits.to(torch.int64)
    return torch.where(b < 0, -(b & 0x7FFFFFFF), b)


@pytest.mark.parametrize("isotropic", [False, True])
@pytest.mark.parametrize("B", [1, 3, 257])
def test_tables_equal_the_restatement(VF, B, isotropic):
    in_size, roi = (90, 91, 109), (80, 80, 80)
    kw = dict(KW, isotropic=isotropic)
    for seed, step, rank in ((0, 0, 0), (0xDEADBEEFCAFEF00D, 2 ** 20 + 3, 5)):
        got = VF(roi, seed=seed, rank=rank, **kw).params(B, step, in_size=in_size)
        assert got.dtype == torch.int32 and got.shape == (B, 16) and got.is_cuda
        got = got.cpu()
        want, _ = R.params_ref(B, step, in_size, roi, seed=seed, rank=rank, **kw)
        assert torch.equal(got[:, 12:], want[:, 12:]), (seed, step, rank)                            # intensity bits, flags, the zero
        unapplied = (want[:, 14] & 8) == 0
        assert torch.equal(got[unapplied], want[unapplied])                                         # integer maps: exact
        g, w = got[:, :12].view(torch.float32).double(), want[:, :12].view(torch.float32).double()
        close = (ordered(got[:, :12]) - ordered(want[:, :12])).abs() <= 1
        small = (w.abs() < 2.0 ** -10) & ((g - w).abs() <= 2.0 ** -40)
        worst = (ordered(got[:, :12]) - ordered(want[:, :12])).abs()[~small].max().item() if (~small).any() else 0
        print(f"B {B} seed {seed:#x}: {int((got[:, :12] != want[:, :12]).sum())} of {12 * B} entries differ, at most {worst} patterns apart")
        assert (close | small).all(), (seed, step, rank)
    if B == 257:
        assert 80 < int(unapplied.sum()) < 180                                                      # prob 0.5: 128.5 +- 6 sigma (sigma 8)


def test_prob_zero_draws_the_rows_of_an_index_copy(VF):
    got = VF((16, 17, 16), prob=0.0, rotate=30, zoom=(0.5, 2), translate=3, flip_prob=(0.5, 0.5, 0.5), seed=4).params(33, 9, in_size=R.IN).cpu()
    want, _ = R.params_ref(33, 9, R.IN, (16, 17, 16), rotate=(30,) * 3, zoom=(0.5, 2), translate=(3,) * 3, prob=0.0, flip_prob=(0.5,) * 3, seed=4)
    assert torch.equal(got, want) and ((got[:, 14] & 8) == 0).all()


# ------------------------------------------------------------------ apply, bit for bit
@pytest.fixture(scope="module")
def volumes():
    return {T: R.volume(T=T) for T in (None, 4, 5)}


@pytest.mark.parametrize("T", [1, 4, 5])
@pytest.mark.parametrize("roi", [(16, 16, 16), (17, 17, 17), (18, 17, 16)], ids=["16", "17", "18x17x16"])
def test_apply_equals_the_restatement_bit_for_bit(VF, volumes, roi, T):
    host = volumes[None if T == 1 else T]
    on_device = layouts(host)
    aff = VF(roi, fill=FILL)
    tables = {name: R.table_of(maps) for name, maps in R.hand_tables(roi).items()}
    drawn, _ = R.params_ref(6, 7, R.IN, roi, rotate=(10, 10, 10), zoom=(0.9, 1.1), translate=(2, 2, 2), prob=0.75, flip_prob=(0.5,) * 3, scale=(0.9, 1.1),
                            shift=(-0.1, 0.1), seed=21)
    tables["drawn"] = drawn
    tables["rotation, shaded"] = R.table_of(R.hand_tables(roi)["rotation"], (SCALE, SHIFT))
    for name, table in tables.items():
        assert len(table) % 3 == 0, name
        for first in range(0, len(table), 3):
            rows = table[first:first + 3]
            want = R.apply_ref(host, rows, roi, FILL)
            if name in ("outside", "non-finite"):
                assert (want == FILL).all(), name                                                   # the float-side range test: the fill, verbatim
            if name == "faces":
                assert all((want[b] == FILL).any() and (want[b] != FILL).any() for b in range(3)), first
            for layout, x in on_device.items():
                got = aff.apply(x, rows.cuda())
                assert got.shape == want.shape and got.is_contiguous() and got.dtype == torch.float32
                assert torch.equal(A.bits(got.cpu()), A.bits(want)), (name, first, layout)


# ------------------------------------------------------------------ a plane of more than one span, guard cells
# (the planes of more than 4096 cells, one workgroup's span: SPAN_SHAPES in tests/augment_inputs.py)
@pytest.mark.parametrize("case", sorted(SPAN_SHAPES))
def test_apply_reaches_a_second_span_and_keeps_inside_out(VF, case):
    shape, roi = SPAN_SHAPES[case]
    host = torch.randn(shape, generator=torch.Generator().manual_seed(61))
    x = host.cuda()
    aff = VF(roi, fill=FILL)
    buf, out = sentinel_out((3, *roi, *shape[4:]))
    assert int(np.prod(out.shape[2:])) > 4096
    turn = lambda deg, **kw: R.map_rows(roi, (1, 1, 2), kw.pop("flips", 0), [np.radians(d) for d in deg], **kw)
    tables = [R.table_of([turn((3, -2, 4)), turn((0, 0, 1.5), t=(0.5, -3.25, 4.0), flips=4), turn((-4, 3, 0), zoom=(1.1, 0.9, 1.0))]),
              R.table_of([R.integer_map(roi, (1, 2, 1), 4), R.integer_map(roi, (-1, -2, -3), 0), turn((2, 2, 2))], (SCALE, SHIFT))]
    for table in tables:
        assert aff.apply(x, table.cuda(), out=out) is out
        assert sentinels_intact(buf)
        assert torch.equal(A.bits(out.cpu()), A.bits(R.apply_ref(host, table, roi, FILL)))
    for bad in (buf[63:63 + out.numel()].view(out.shape), torch.empty(3, *roi, 2, device="cuda")[..., 0], torch.empty(out.shape, device="cuda", dtype=torch.float64)):
        with pytest.raises(ValueError, match="out must be"):
            aff.apply(x, tables[0].cuda(), out=bad)
    if case == "3d":                                                                                # an out that overlaps the source is refused by the library
        room = torch.zeros(x.numel() + out.numel(), device="cuda")
        src = room[:x.numel()].view(x.shape)
        inside = room[x.numel() - 64:x.numel() - 64 + out.numel()].view(out.shape)
        with pytest.raises(RuntimeError, match="aliases"):
            aff.apply(src, tables[0].cuda(), out=inside)


# ------------------------------------------------------------------ integer maps are what nv_augment_apply writes
@pytest.mark.parametrize("T", [1, 4, 5])
def test_integer_maps_equal_the_augmentation_pass_bit_for_bit(VF, T):
    from neurovit_amd.augment import VolumeAugment
    roi = (17, 16, 15)
    host = special_volume((3, *R.IN) if T == 1 else (3, *R.IN, T), 33)
    hi = [n - s for n, s in zip(R.IN, roi)]
    cases = [((0, 0, 0), 0), (tuple(hi), 7), ((1, 2, 1), 4), ((2, 1, 0), 3), ((-3, 1, 1), 5), ((1, -5, 2), 2), ((0, 1, hi[2] + 6), 4), ((1, 1, -3), 1),
             ((hi[0] + 2, 0, 2), 6), ((-40, 50, -60), 0), ((1, hi[1] + 4, 0), 7), ((0, 0, -1), 4)]
    aff, aug = VF(roi, fill=FILL), VolumeAugment(roi, fill=FILL)
    for layout, x in layouts(host).items():
        for intensity in ((ONE, ZERO), (SCALE, SHIFT)):
            for first in range(0, len(cases), 3):
                three = cases[first:first + 3]
                got = aff.apply(x, R.table_of([R.integer_map(roi, o, f) for o, f in three], intensity).cuda())
                want = aug.apply(x, R.augment_rows(three, intensity).cuda())
                assert torch.equal(A.bits(got), A.bits(want)), (layout, intensity, first)            # NaN payloads, -0.0, the fill verbatim
                if intensity == (ONE, ZERO):
                    assert torch.equal(A.bits(got.cpu()), A.bits(A.apply_ref(host, R.augment_rows(three), roi, FILL)))


# ------------------------------------------------------------------ 4D series
@pytest.mark.parametrize("T", [2, 4, 5, 8])
def test_a_series_is_its_volumes_one_by_one(VF, T):
    host = torch.randn(2, 13, 12, 11, T, generator=torch.Generator().manual_seed(40 + T))
    roi = (8, 9, 8)
    aff = VF(roi, fill=0.5)
    turn = lambda deg, **kw: R.map_rows(roi, (2, 1, 1), kw.pop("flips", 0), [np.radians(d) for d in deg], **kw)
    x = host.cuda()
    strided = torch.zeros(2, 13, 12, 11, 2 * T).cuda()[..., ::2].copy_(x)                            # time is not dense
    for table in (R.table_of([turn((9, -8, 10)), turn((0, 5, 0), t=(0.5, 4.5, -3.0), flips=6)], (SCALE, SHIFT)),
                  R.table_of([R.integer_map(roi, (5, 3, 3), 0), R.integer_map(roi, (-3, 2, 1), 7)]),
                  R.table_of([turn((0, 0, 0), zoom=(2.0, 0.5, 1.0)), R.integer_map(roi, (0, 20, 0), 1)])):
        got = aff.apply(x, table.cuda())
        assert got.shape == (2, *roi, T) and got.is_contiguous()
        assert torch.equal(A.bits(got.cpu()), A.bits(R.apply_ref(host, table, roi, 0.5)))
        assert torch.equal(A.bits(aff.apply(strided, table.cuda())), A.bits(got))
        for t in range(T):
            assert torch.equal(A.bits(aff.apply(x[..., t], table.cuda())), A.bits(got[..., t])), t


# ------------------------------------------------------------------ the call protocol
def test_call_draws_applies_and_counts(VF):
    host = torch.randn(5, 14, 13, 12, generator=torch.Generator().manual_seed(8))
    x = host.cuda()
    aff = VF((9, 10, 11), rotate=(10, 0, 5), zoom=(0.9, 1.1), translate=1.5, prob=0.8, flip_prob=(0.5, 0.5, 0.5), scale=(0.8, 1.2), shift=(-0.1, 0.1),
             fill=-1.0, seed=77, rank=2)
    assert aff.step == 0 and aff.last_params is None
    outs = []
    for n in range(3):
        out = aff(x)
        assert aff.step == n + 1                                                                    # the counter advances by one per call
        assert torch.is_tensor(aff.last_params) and aff.last_params.is_cuda and aff.last_params.dtype == torch.int32
        table = aff.params(5, n, in_size=(14, 13, 12))
        assert torch.equal(aff.last_params, table)
        assert torch.equal(A.bits(out), A.bits(aff.apply(x, table)))
        assert torch.equal(A.bits(out.cpu()), A.bits(R.apply_ref(host, table.cpu(), (9, 10, 11), -1.0)))
        outs.append(out)
    assert not torch.equal(outs[0], outs[1])
    again = aff(x, step=1)                                                                          # a past batch, the counter stays
    assert aff.step == 3 and torch.equal(A.bits(again), A.bits(outs[1]))
    s = torch.stack([x, 2 * x], dim=-1)                                                             # 4D: the same rows for a series
    o4 = aff(s, step=0)
    assert o4.shape == (5, 9, 10, 11, 2) and torch.equal(A.bits(o4[..., 0]), A.bits(outs[0]))


def test_identity_configuration_returns_its_input(VF):
    x = torch.randn(2, 8, 8, 8, device="cuda")
    aff = VF(8)
    assert aff(x) is x and aff.last_params is None and aff.step == 1
    assert VF(8, rotate=20, zoom=(0.5, 2), translate=3, prob=0.0)(x) is x
    s = torch.randn(2, 8, 8, 8, 3, device="cuda")
    assert aff(s) is s
    crop = aff(torch.randn(2, 9, 8, 8, device="cuda"))                                              # a larger input: the crop is on
    assert crop.shape == (2, 8, 8, 8) and aff.last_params is not None
    turned = VF(8, rotate=(0, 0, 10))(x)
    assert turned is not x and not torch.equal(turned, x)


def test_mix_behind_an_affine_is_the_two_passes(VF):
    from neurovit_amd.augment import VolumeMix
    x = torch.randn(6, 14, 13, 12, generator=torch.Generator().manual_seed(3)).cuda()
    roi = (9, 10, 11)
    aff = VF(roi, rotate=10, zoom=(0.9, 1.1), translate=2, flip_prob=(0.5, 0.5, 0.5), scale=(0.9, 1.1), fill=0.25, seed=5)
    for kw in (dict(mixup_alpha=0.8), dict(cutmix_alpha=1.0), dict(mixup_alpha=0.8, cutmix_alpha=1.0)):
        mix = VolumeMix(seed=5, **kw)
        got = mix(x, step=4, augment=aff)
        assert aff.step == 0 and mix.step == 0                                                      # `step=` given: no counter moves
        table, rows = aff.params(6, 4, in_size=(14, 13, 12)), mix.params(6, 4, roi)
        assert torch.equal(aff.last_params, table) and torch.equal(mix.last_mix, rows)
        window = aff.apply(x, table)
        assert torch.equal(A.bits(got), A.bits(mix.apply(window, rows))), kw
        assert torch.equal(A.bits(got), A.bits(mix.apply(x, rows, augment=aff, augment_params=table)))
        assert got.shape == (6, *roi) and not torch.equal(got, window)
    assert torch.equal(A.bits(VolumeMix()(x, step=4, augment=aff)), A.bits(aff(x, step=4)))         # no mix: the affine pass alone


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


def test_trainer_epoch_with_the_affine_keys_reproduces_from_global_step(VF, tmp_path):
    from neurovit_amd.NeuroEncoder import NeuroEncoder
    from neurovit_amd.trainer import Trainer
    size = dict(TRAINING_VIT_DIM=128, TRAINING_VIT_DEPTH=2, TRAINING_VIT_HEADS=2, TRAINING_VIT_MLP_DIM=256)
    cfg = W.neuro_config(32, 8, DEVICE="cuda", TRAINING_LEARNING_RATE=1e-3, TRAINING_WEIGHT_DECAY=1e-2, GLOBAL_OUTPUT_DIR=str(tmp_path / "runs"),
                         TRAINING_EPOCHS=1, TRAINING_BATCH_SIZE=2, TRAINING_NUM_WORKERS=0, DATASET_TRANSFORMS=True, AUGMENT_ROTATE_DEG=(10, 10, 5),
                         AUGMENT_ZOOM=(0.9, 1.1), AUGMENT_TRANSLATE=2, AUGMENT_AFFINE_PROB=0.75, AUGMENT_FLIP_PROB=(0.5, 0, 0), AUGMENT_SEED=13, **size)
    torch.manual_seed(5)
    data = Volumes40()
    tr = Trainer(cfg, NeuroEncoder(cfg), data, data)
    assert isinstance(tr.augment, VF) and tr.augment.roi == (32, 32, 32) and tr.augment.rank == 0 and tr.mix is None
    seen, fed = [], []
    real, run = tr.augment, tr.step._step

    class Spy:
        roi = real.roi

        def __call__(self, x, step=None):
            out = real(x, step=step)
            seen.append((step, x.clone(), out.clone(), real.last_params.clone()))
            return out

    def step_spy(fmri, labels):
        loss = run(fmri, labels)
        fed.append((fmri.clone(), loss))
        return loss
    tr.augment, tr.step._step = Spy(), step_spy
    tr.train(0)
    assert [s[0] for s in seen] == [0, 1, 2] and tr.global_step == 3 and len(fed) == 3
    fresh = Trainer.augment_from_config(cfg)                                                        # another instance, nothing but the config and the step index
    for (step, x, out, table), (fmri, loss) in zip(seen, fed):
        assert x.shape == (2, 40, 40, 40) and out.shape == (2, 32, 32, 32) and torch.isfinite(loss).item()
        assert torch.equal(A.bits(fmri), A.bits(out))
        assert torch.equal(A.bits(fresh(x, step=step)), A.bits(out)) and torch.equal(fresh.last_params, table), step
        want, _ = R.params_ref(2, step, (40, 40, 40), (32, 32, 32), rotate=(10, 10, 5), zoom=(0.9, 1.1), translate=(2, 2, 2), prob=0.75,
                               flip_prob=(0.5, 0, 0), seed=13)
        assert torch.equal(table[:, 12:].cpu(), want[:, 12:])                                       # the draws are AUGMENT_SEED's, at this step
        assert torch.equal(A.bits(out.cpu()), A.bits(R.apply_ref(x.cpu(), table.cpu(), (32, 32, 32), 0.0)))
    assert any(not torch.equal(seen[0][3], s[3]) for s in seen[1:])
    loss, acc = tr.validate(0)                                                                      # validation keeps the centre window
    assert np.isfinite(loss)
