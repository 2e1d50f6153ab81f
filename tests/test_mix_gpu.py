"""Mixup / CutMix and the soft-target cross-entropy on MI355X: the kernels of csrc/mix.hip and csrc/augment.hip (nv_mix_params, nv_augment_mix) and the soft
loss (nv_ce_loss_soft, nv_head_step_soft, nv_vit_train_step_ex) against their CPU restatement (tests/mix_ref.py, itself proved in
tests/test_mix_cpu.py), VolumeMix's call protocol, TrainStep with the options on every path, and the Trainer shell with the new keys.

Comparisons of the mixing pass are on int32 patterns: bit for bit wherever a cell is a move (mode 0, CutMix, the fill) or holds no NaN; a
NaN that arithmetic produced (an intensity change or the Mixup blend of a NaN voxel) must be a NaN, its payload is the hardware's - the
rule of tests/test_augment_gpu.py.  Loss and d(loss)/d(logits) are held to float64 within 1e-5 in conftest.rel_err, the project's gate
for fp32 kernel outputs; native and general train steps to each other bit for bit."""
import ctypes
import itertools

import numpy as np
import pytest
import torch

import augment_ref as R
import mix_ref as M
import weights as W
from conftest import rel_err
from augment_inputs import SPAN_SHAPES, layouts, sentinel_out, sentinels_intact, special_volume
from test_augment_gpu import span_rows

pytestmark = pytest.mark.gpu

ONE, ZERO = M.ONE_BITS, 0
SCALE, SHIFT = torch.tensor([0.75, -0.3]).view(torch.int32).tolist()
FP32_GATE = 1e-5


@pytest.fixture(scope="module")
def VM():
    from neurovit_amd._cabi import require_gpu
    require_gpu()
    from neurovit_amd.augment import VolumeMix
    return VolumeMix


def fbits(v):
    return M.f32_bits(v)


def mix_row(partner, mode=0, lam=1.0, label=None, box=(0, 0, 0, 0, 0, 0), tries=1):
    lam_bits = lam if isinstance(lam, int) else fbits(lam)
    return [partner, mode, lam_bits, lam_bits if label is None else fbits(label), tries, *box, 0]


# ------------------------------------------------------------------ parameters
@pytest.mark.parametrize("name", sorted(M.PARAM_CONFIGS))
@pytest.mark.parametrize("B", M.PARAM_BATCHES)
def test_params_equal_the_restatement(VM, B, name):
    cfg, roi = M.PARAM_CONFIGS[name], M.PARAM_ROI
    tables = {}
    for seed, rank, step in M.PARAM_TRIPLES:
        mix = VM(seed=seed, rank=rank, **cfg)
        got = mix.params(B, step, roi)
        assert got.dtype == torch.int32 and got.shape == (B, 12) and got.is_cuda
        got = got.cpu().numpy()
        tables[(seed, rank, step)] = got
        want, gap = M.mix_params_ref(B, step, roi, seed=seed, rank=rank, **cfg)
        assert gap >= 1e-9                                                   # (tests/test_mix_cpu.py: why `tries` can be demanded on every row)
        for col in (0, 1, 4, 11):                                            # partner, mode, tries, the spare 0: every row
            assert np.array_equal(got[:, col], want[:, col]), (name, seed, rank, step, col)
        # the pixel lambda: both sides round a double that agrees to ~1e-15 - 1 fp32 ulp (positive floats: adjacent patterns)
        assert (np.abs(got[:, 2].astype(np.int64) - want[:, 2].astype(np.int64)) <= 1).all()
        assert (np.abs(got[:, 3].astype(np.int64) - want[:, 3].astype(np.int64)) <= 1)[want[:, 1] != 2].all()
        # box and label lambda from the device's OWN pixel lambda: bit for bit
        again, _ = M.mix_params_ref(B, step, roi, seed=seed, rank=rank, pixel_bits=got[:, 2], **cfg)
        assert np.array_equal(got, again), (name, seed, rank, step)
        assert np.array_equal(mix.params(B, step, roi).cpu().numpy(), got)  # the same triple reproduces
    if B > 1 and name != "never":
        base = tables[M.PARAM_TRIPLES[0]]
        assert not np.array_equal(base, tables[M.PARAM_TRIPLES[2]]) and not np.array_equal(base, tables[M.PARAM_TRIPLES[3]])   # another rank, another step
    if name == "never" or B == 1:
        assert all((t[:, 1:5] == np.array([0, ONE, ONE, 0])).all() and (t[:, 5:] == 0).all() for t in tables.values())
    if name == "half" and B == 257:
        modes = np.bincount(tables[M.PARAM_TRIPLES[0]][:, 1], minlength=3)
        assert modes[0] > 64 and modes[1] > 32 and modes[2] > 8             # about 1/2, 3/8 and 1/8 of 256


# ------------------------------------------------------------------ the mixing pass, hand-written tables
IN = (23, 21, 22)


@pytest.fixture(scope="module")
def volumes():
    return layouts(subnormals=True)                          # (the recipe of tests/test_augment_gpu.py plus +-subnormals)


def aug_tables(S):
    """None (identity rows), and rows that differ between a sample and its partner: other offsets, other flips, windows partly outside the
    volume on either side, an intensity change on some"""
    hi = [n - S for n in IN]
    return [None,
            [[0, 0, 0, 0, ONE, ZERO, 0, 0], [hi[0], hi[1], hi[2], 7, ONE, ZERO, 0, 0], [1, 0, 2, 4, ONE, ZERO, 0, 0]],
            [[-3, 1, 1, 5, SCALE, SHIFT, 0, 0], [1, hi[1] + 4, 0, 2, ONE, ZERO, 0, 0], [2, 1, hi[2] + 3, 3, SCALE, SHIFT, 0, 0]],
            [[1, 2, -2, 0, ONE, ZERO, 0, 0], [hi[0] + 2, -1, 1, 6, SCALE, SHIFT, 0, 0], [0, 1, 1, 1, ONE, ZERO, 0, 0]]]


def mix_tables(S):
    tiny = fbits(2.0 ** -24)
    whole = (0, S, 0, S, 0, S)
    return [
        [mix_row(2, 1, 0.5), mix_row(1, 1, 0.5), mix_row(0, 1, 0x3E99999B)],                         # mixup; the middle sample with itself
        [mix_row(2, 1, 0.0), mix_row(0, 1, 1.0), mix_row(1, 1, tiny)],                               # lambda 0, 1 (the partner is not read), 2^-24
        [mix_row(1, 2, 0.5, box=whole), mix_row(2, 2, 0.5, box=(3, 3, 0, S, 0, S)), mix_row(0, 2, 0.5, box=(0, S, 4, 5, 0, S))],   # full, empty, one row wide
        [mix_row(2, 2, 0.25, box=(0, S, 0, S, 5, 6)), mix_row(0, 2, 0.25, box=(0, 3, 0, S, 0, S)), mix_row(1, 2, 0.25, box=(S - 3, S, 0, S, 0, S))],
        [mix_row(2, 2, 0.25, box=(0, S, 0, 2, 0, S)), mix_row(0, 2, 0.25, box=(0, S, S - 2, S, 0, S)), mix_row(1, 2, 0.25, box=(0, S, 0, S, 0, 3))],
        [mix_row(1, 2, 0.25, box=(1, S - 1, 2, S - 2, S - 3, S)), mix_row(2, 2, 0.25, box=(2, 9, 1, 8, 2, S - 1)), mix_row(0, 2, 0.25, box=(0, S, 1, S, 5, 11))],   # faces that cut 16-byte groups
        [mix_row(2, 2, 1.0, box=whole), mix_row(0, 2, 0.5, box=(-5, S + 7, -1, 4, 3, S + 9)), mix_row(7, 1, 0.5)],      # lambda 1; a box beyond the window; a partner outside the batch
        [mix_row(2), mix_row(1), mix_row(0)],                                                        # mode 0 everywhere
    ]


@pytest.mark.parametrize("layout", ["view", "dense", "moved"])
@pytest.mark.parametrize("S", [18, 17, 20])
def test_mix_hand_written_tables(VM, volumes, S, layout):
    from neurovit_amd.augment import VolumeAugment
    host, on_device = volumes
    x = on_device[layout](lambda t: t.cuda())
    assert tuple(x.shape) == (3, *IN) and x.is_cuda
    roi, fill = (S, S, S), -2.5
    aug, mixer = VolumeAugment(roi, fill=fill), VM(mixup_alpha=0.4)
    full = VolumeAugment(IN, fill=fill)
    for rows, table in itertools.product(aug_tables(S), mix_tables(S)):
        mix = torch.tensor(table, dtype=torch.int32)
        if rows is None:                                                     # a NULL table: the window is the whole volume
            got = mixer.apply(x, mix.cuda())
            want, moved = M.mix_apply_ref(host, None, mix, IN)
            assert got.shape == (3, *IN) and got.is_contiguous()
            ident = mixer.apply(x, mix.cuda(), augment=full, augment_params=M.identity_rows(3).cuda())
            assert torch.equal(R.bits(ident), R.bits(got)), table           # ... and equals the identity-row table
        else:
            params = torch.tensor(rows, dtype=torch.int32)
            got = mixer.apply(x, mix.cuda(), augment=aug, augment_params=params.cuda())
            want, moved = M.mix_apply_ref(host, params, mix, roi, fill)
            assert got.shape == (3, *roi) and got.is_contiguous() and got.dtype == torch.float32
            if all(r[1] == 0 for r in table):                                # mode 0 everywhere: nv_augment_apply, bit for bit
                assert torch.equal(R.bits(got), R.bits(aug.apply(x, params.cuda()))), rows
        assert M.same_bits(got.cpu(), want, moved), (rows, table)


@pytest.mark.parametrize("S", [17, 20])
def test_mix_writes_nothing_outside_out(VM, volumes, S):
    from neurovit_amd.augment import VolumeAugment
    host, on_device = volumes
    x = on_device["view"](lambda t: t.cuda())
    roi, n = (S, S, S), 3 * S ** 3
    buf = torch.full((64 + n + 64,), 0x7FC0BEEF, dtype=torch.int32, device="cuda").view(torch.float32)      # 64 sentinel floats on both sides
    out = buf[64:64 + n].view(3, *roi)
    params = torch.tensor(aug_tables(S)[2], dtype=torch.int32)
    mix = torch.tensor([mix_row(2, 1, 0.5), mix_row(1), mix_row(0, 2, 0.5, box=(1, S, 0, S - 1, 3, S))], dtype=torch.int32)
    aug, mixer = VolumeAugment(roi, fill=1.5), VM(cutmix_alpha=1.0)
    assert mixer.apply(x, mix.cuda(), augment=aug, augment_params=params.cuda(), out=out) is out
    edges = R.bits(torch.cat([buf[:64], buf[64 + n:]]).cpu())
    assert (edges == 0x7FC0BEEF).all()
    want, moved = M.mix_apply_ref(host, params, mix, roi, 1.5)
    assert M.same_bits(out.cpu(), want, moved)
    for bad in (buf[63:63 + n].view(3, *roi), torch.empty(3, S, S, S + 1, device="cuda"), torch.empty(3, *roi, device="cuda", dtype=torch.float64)):
        with pytest.raises(ValueError, match="out must be"):
            mixer.apply(x, mix.cuda(), augment=aug, augment_params=params.cuda(), out=bad)
    with pytest.raises(ValueError, match="mix must be int32"):
        mixer.apply(x, mix[:2].cuda(), augment=aug, augment_params=params.cuda())
    with pytest.raises(ValueError, match="augment_params must be int32"):
        mixer.apply(x, mix.cuda(), augment=aug, augment_params=params[:, :6].cuda())


@pytest.mark.parametrize("B", [1, 2, 3])
@pytest.mark.parametrize("T", [1, 4, 5])
def test_series_share_their_samples_rows(VM, T, B):
    from neurovit_amd.augment import VolumeAugment
    g = torch.Generator().manual_seed(40 + T)
    series = torch.randn(B, 13, 12, 11, T, generator=g)
    series.view(-1)[3::53] = float("nan")
    roi = (8, 7, 9)
    aug, mixer = VolumeAugment(roi, fill=0.5), VM(mixup_alpha=1.0)
    rows3 = [[[5, 4, 2, 0, ONE, ZERO, 0, 0], [0, 0, 0, 4, ONE, ZERO, 0, 0], [1, 2, 1, 3, ONE, ZERO, 0, 0]],     # runs of memory forwards, a flipped series
             [[2, -1, 1, 3, SCALE, SHIFT, 0, 0], [-3, 2, 6, 7, ONE, ZERO, 0, 0], [1, 1, -2, 2, SCALE, SHIFT, 0, 0]]]
    mixes3 = [[mix_row(B - 1, 1, 0.75), mix_row(B - 2, 2, 0.5, box=(1, 7, 0, 7, 2, 5)), mix_row(0, 2, 0.5, box=(0, 8, 3, 4, 0, 9))],
              [mix_row(B - 1, 2, 0.5, box=(2, 6, 1, 6, 1, 8)), mix_row(max(B - 2, 0), 1, 0.125), mix_row(0)]]
    x = series.cuda()
    strided = torch.zeros(B, 13, 12, 11, 2 * T).cuda()[..., ::2].copy_(x)                            # time is not dense: cell by cell
    for rows, table in itertools.product(rows3, mixes3):
        params, mix = torch.tensor(rows[:B], dtype=torch.int32), torch.tensor(table[:B], dtype=torch.int32)
        got = mixer.apply(x, mix.cuda(), augment=aug, augment_params=params.cuda())
        assert got.shape == (B, *roi, T) and got.is_contiguous()
        want, moved = M.mix_apply_ref(series, params, mix, roi, 0.5)
        assert M.same_bits(got.cpu(), want, moved), (rows, table)
        assert torch.equal(R.bits(mixer.apply(strided, mix.cuda(), augment=aug, augment_params=params.cuda())), R.bits(got))
        for t in range(T):                                                                          # the 3D pass of each timepoint, same rows
            assert torch.equal(R.bits(mixer.apply(x[..., t], mix.cuda(), augment=aug, augment_params=params.cuda())), R.bits(got[..., t])), (rows, t)


@pytest.mark.parametrize("case", sorted(SPAN_SHAPES))
def test_mix_reaches_a_second_span(VM, case):
    """tests/test_augment_gpu.py's planes of more than 4096 cells: one Mixup row, one mode-0 row and one CutMix row whose box crosses the
    span boundary in y (3D: the second span starts in output row 61; 4D: in row 8) and whose z faces cut 16-byte groups behind it"""
    from neurovit_amd.augment import VolumeAugment
    shape, roi = SPAN_SHAPES[case]
    box = (0, roi[0], 60, 64, 6, 59) if case == "3d" else (0, roi[0], 7, 9, 5, 9)
    host = special_volume(shape, 61, subnormals=True)
    x = host.cuda()
    aug, mixer = VolumeAugment(roi, fill=-2.5), VM(mixup_alpha=0.4, cutmix_alpha=1.0)
    buf, out = sentinel_out((3, *roi, *shape[4:]))
    tables = [[mix_row(2, 1, 0.3), mix_row(0, 2, 0.5, box=box), mix_row(0)],
              [mix_row(1, 2, 0.5, box=box), mix_row(1), mix_row(0, 1, 0.75)],
              [mix_row(2), mix_row(1), mix_row(0)]]                              # mode 0 everywhere
    for rows, table in itertools.product(span_rows(), tables):
        params, mix = torch.tensor(rows, dtype=torch.int32), torch.tensor(table, dtype=torch.int32)
        assert mixer.apply(x, mix.cuda(), augment=aug, augment_params=params.cuda(), out=out) is out
        assert sentinels_intact(buf), (rows, table)
        want, moved = M.mix_apply_ref(host, params, mix, roi, -2.5)
        assert M.same_bits(out.cpu(), want, moved), (rows, table)
        if all(r[1] == 0 for r in table):                                    # mode 0 everywhere: nv_augment_apply, bit for bit
            assert torch.equal(R.bits(out), R.bits(aug.apply(x, params.cuda()))), rows


def test_call_draws_applies_and_counts(VM):
    from neurovit_amd.augment import VolumeAugment
    g = torch.Generator().manual_seed(8)
    host = torch.randn(5, 14, 13, 12, generator=g)
    x = host.cuda()
    kw = dict(flip_prob=(0.5, 0.5, 0.5), max_shift=(2, 2, 2), scale=(0.8, 1.2), shift=(-0.1, 0.1), seed=77, rank=2)
    aug = VolumeAugment((9, 10, 11), fill=-1.0, **kw)
    mixer = VM(mixup_alpha=0.4, cutmix_alpha=1.0, seed=77, rank=2)
    outs = []
    for n in range(3):
        out = mixer(x, augment=aug)
        assert mixer.step == n + 1 and aug.step == 0                         # its own counter advances; the augmentation's is not touched
        mix, params = mixer.last_mix, aug.last_params
        assert torch.equal(mix, mixer.params(5, n, (9, 10, 11))) and torch.equal(params.cpu(), R.params_ref(5, n, (14, 13, 12), (9, 10, 11), **kw))
        want, moved = M.mix_apply_ref(host, params.cpu(), mix.cpu(), (9, 10, 11), -1.0)
        assert M.same_bits(out.cpu(), want, moved)
        outs.append(out)
    assert not torch.equal(outs[0], outs[1])
    again = mixer(x, step=1, augment=aug)                                    # a past batch, the counter stays
    assert mixer.step == 3 and torch.equal(R.bits(again), R.bits(outs[1]))
    plain = mixer(x, step=0)                                                 # without an augmentation: the whole volume
    assert plain.shape == x.shape and torch.equal(mixer.last_mix, mixer.params(5, 0, (14, 13, 12)))
    # both alphas None: the identity, nothing is launched
    ident = VM()
    assert ident(x) is x and ident.last_mix is None and ident.step == 1
    assert torch.equal(R.bits(ident(x, step=2, augment=aug)), R.bits(aug(x, step=2)))


# ------------------------------------------------------------------ the loss
def loss_inputs(B, C, seed):
    g = torch.Generator().manual_seed(seed)
    d = 8 if C <= 8 else 304
    x = torch.randn(B, 2, d, generator=g)
    gamma, beta = 1 + 0.1 * torch.randn(d, generator=g), 0.1 * torch.randn(d, generator=g)
    Wt, bias = torch.randn(C, d, generator=g) / d ** 0.5 * 3, torch.randn(C, generator=g)
    y = torch.randint(0, C, (B,), generator=g)
    w = torch.rand(C, generator=g) + 0.25
    w0 = w.clone()
    w0[(int(y[0]) + 1) % C] = 0.0                                            # one class of no weight (never the only one present: D > 0)
    lam = [0.0, 0.3, 1.0]
    mix = torch.tensor([mix_row(b if b % 5 == 3 else B - 1 - b, 1, lam[b % 3]) for b in range(B)], dtype=torch.int32)     # some rows pair with themselves
    return x, gamma, beta, Wt, bias, y, {"none": None, "given": w, "zero": w0}, mix


@pytest.mark.parametrize("eps", [0.0, 0.1])
@pytest.mark.parametrize("C", [2, 3, 300])
@pytest.mark.parametrize("B", [1, 3, 257])
def test_soft_loss_against_float64_and_between_its_entry_points(VM, B, C, eps):
    from neurovit_amd import ops
    x, gamma, beta, Wt, bias, y, weights, mix = loss_inputs(B, C, 100 * B + C)
    dev = lambda t: None if t is None else t.cuda()
    args = [dev(t) for t in (x, gamma, beta, Wt, bias, y)]
    plain = ops.head_step(*args)
    for (wname, w), mixed in itertools.product(weights.items(), (False, True)):
        m = mix if mixed else None
        out = ops.head_step_soft(*args, label_smoothing=eps, class_weight=dev(w), mix=dev(m))
        logits, loss, dl = out[0], out[3], out[4]
        assert torch.equal(logits, plain[0])
        loss2, dl2 = ops.ce_loss_soft(logits, args[5], eps, dev(w), dev(m))
        assert torch.equal(loss, loss2) and torch.equal(dl, dl2), (wname, mixed)             # one row body: the same bits
        if eps == 0.0 and w is None and m is None:                                         # every option off: the index-target kernels, bit for bit
            for a, b in zip(out, plain):
                assert torch.equal(R.bits(a.float()), R.bits(b.float()))
            l0, d0 = ops.ce_loss(logits, args[5])
            assert torch.equal(loss2, l0) and torch.equal(dl2, d0)
            continue
        want_loss, want_dl = M.ce_soft_ref(logits.cpu().double().numpy(), y.numpy(), eps, None if w is None else w.double().numpy(),
                                           None if m is None else m.numpy())
        e_loss, e_dl = abs(loss.item() - want_loss) / abs(want_loss), rel_err(dl, want_dl)
        print(f"soft loss B={B} C={C} eps={eps} w={wname} mix={mixed}: loss rel {e_loss:.2e}, dlogits rel {e_dl:.2e}")
        assert e_loss < FP32_GATE and e_dl < FP32_GATE, (wname, mixed, e_loss, e_dl)


def test_soft_loss_scale_state_bad_labels_and_zero_denominator(VM):
    from neurovit_amd import ops
    B, C = 3, 3
    x, gamma, beta, Wt, bias, y, weights, mix = loss_inputs(B, C, 7)
    args = [t.cuda() for t in (x, gamma, beta, Wt, bias, y)]
    w, m = weights["given"].cuda(), mix.cuda()
    logits = ops.head_step(*args)[0]
    loss, dl = ops.ce_loss_soft(logits, args[5], 0.1, w, m)
    state = torch.zeros(16, device="cuda")
    state[0] = 8.0
    loss_s, dl_s = ops.ce_loss_soft(logits, args[5], 0.1, w, m, scale_state=state)
    assert torch.equal(loss_s, loss) and torch.equal(dl_s, dl * 8.0)                        # dlogits carry state[0] (a power of two: exactly), the loss does not
    out = ops.head_step_soft(*args, label_smoothing=0.1, class_weight=w, mix=m, scale_state=state)
    assert torch.equal(out[3], loss) and torch.equal(out[4], dl_s)
    loss_g, dl_g = ops.ce_loss_soft(logits, args[5], 0.1, w, m, grad_scale=0.5)
    assert torch.equal(loss_g, loss) and torch.equal(dl_g, dl * 0.5)
    # a label outside [0, C): the row's own, or its partner's - NaN, and the call returns
    for row, value in ((0, C), (2, -1), (1, 2 ** 40)):
        bad = args[5].clone()
        bad[row] = value
        for mm in (None, m):
            l, d = ops.ce_loss_soft(logits, bad, 0.1, w, mm)
            assert torch.isnan(l).all() and d.shape == dl.shape
            assert torch.isnan(ops.head_step_soft(*args[:5], bad, label_smoothing=0.1, class_weight=w, mix=mm)[3]).all()
    only_partner = torch.tensor([mix_row(2, 1, 0.5), mix_row(1), mix_row(0)], dtype=torch.int32).cuda()      # rows 1 and 2 do not read row 2's label through a partner ...
    bad = args[5].clone()
    bad[2] = C
    assert torch.isnan(ops.ce_loss_soft(logits, bad, 0.0, None, only_partner)[0]).all()                      # ... row 0 does
    outside = torch.tensor([mix_row(5, 1, 0.5), mix_row(1), mix_row(-1, 1, 0.5)], dtype=torch.int32).cuda()   # a partner outside the batch
    assert torch.isnan(ops.ce_loss_soft(logits, args[5], 0.0, None, outside)[0]).all()
    # D == 0: NaN, not a fault
    assert torch.isnan(ops.ce_loss_soft(logits, args[5], 0.1, torch.zeros(C, device="cuda"))[0]).all()
    torch.cuda.synchronize()


def test_nn_cross_entropy_loss_with_options_is_differentiable(VM):
    from neurovit_amd.nn import CrossEntropyLoss
    B, C = 3, 3
    x, gamma, beta, Wt, bias, y, weights, mix = loss_inputs(B, C, 9)
    z = torch.randn(B, C, device="cuda", requires_grad=True)
    crit = CrossEntropyLoss(weight=weights["given"], label_smoothing=0.1).cuda()
    loss = crit(z, y.cuda(), mix.cuda())
    (2.0 * loss).backward()
    want_loss, want_dl = M.ce_soft_ref(z.detach().cpu().double().numpy(), y.numpy(), 0.1, weights["given"].double().numpy(), mix.numpy())
    assert abs(loss.item() - want_loss) < FP32_GATE * abs(want_loss) and rel_err(z.grad, 2.0 * want_dl) < FP32_GATE
    # defaults: nv_ce_loss, as before
    plain = CrossEntropyLoss()
    assert abs(plain(z, y.cuda()).item() - torch.nn.functional.cross_entropy(z, y.cuda()).item()) < 1e-6


# ------------------------------------------------------------------ the train step
SIZE = dict(TRAINING_VIT_DIM=128, TRAINING_VIT_DEPTH=2, TRAINING_VIT_HEADS=2, TRAINING_VIT_MLP_DIM=256)
STEP_WEIGHTS = [0.5, 2.0]


def micro_model(**extra):
    import neurovit_amd.NeuroEncoder as ne
    cfg = W.neuro_config(32, 8, DEVICE="cuda", TRAINING_LEARNING_RATE=1e-3, TRAINING_WEIGHT_DECAY=1e-2, **SIZE, **extra)
    model = ne.NeuroEncoder(cfg)
    model.load_state_dict(W.make_tensors(W.vit_param_spec(**W.MICRO), 1, prefix="volume_encoder.vit3d."), strict=True)
    model.train()
    return model


def step_batch():
    x = W.make_volume((3, 32, 32, 32), 2).cuda()
    y = torch.tensor([1, 0, 1], device="cuda")
    mix = torch.tensor([mix_row(2, 1, 0.3), mix_row(1), mix_row(0, 2, 0.5, label=0.7, box=(4, 20, 0, 32, 8, 30))], dtype=torch.int32).cuda()
    return x, y, mix


def run_steps(native, n, mix, model_kw=None, **step_kw):
    from neurovit_amd.trainer import TrainStep
    x, y, table = step_batch()
    model = micro_model(**(model_kw or {}))
    step = TrainStep(model, **step_kw)
    if not native:
        step._native = False
    torch.manual_seed(11)
    losses = [step(x, y, mix=table).clone() if mix else step(x, y).clone() for _ in range(n)]
    assert step._native == native and step.last_path == ("native" if native else "general")
    vit = model.volume_encoder.vit3d
    m, v = step.optimizer.arena_state(vit)
    return dict(losses=torch.stack(losses), logits=step.last_outputs.clone(), params=vit.flat_parameters()[0].clone(), shadow=vit.flat_parameters()[1].clone(),
                m=m.clone(), v=v.clone(), grads=vit.flat_gradients().clone(), step=step, vit=vit)


def assert_same_run(a, b, what):
    for name in ("losses", "logits", "params", "shadow", "m", "v"):
        assert torch.equal(a[name], b[name]), f"{what}: {name} differ"


def test_train_step_ex_with_every_option_off_is_the_plain_step(VM, monkeypatch):
    """nv_vit_train_step_ex with an option block that switches nothing on hands the loss to the index-target kernels: parameters, moments,
    loss and logits equal nv_vit_train_step's bit for bit.  (lo = NULL is nv_vit_train_step itself, which is now that very call.)"""
    from neurovit_amd._cabi import LossOpts, lib
    from neurovit_amd.trainer import TrainStep
    plain = run_steps(True, 2, False)
    calls = []
    real = lib.nv_vit_train_step_ex

    def spy(*a):
        calls.append(1)
        return real(*a)
    monkeypatch.setattr(lib.load(), "nv_vit_train_step_ex", spy, raising=False)
    monkeypatch.setattr(TrainStep, "_loss_opts", lambda self, labels, mix: LossOpts(ctypes.sizeof(LossOpts), 0.0, None, None))
    off = run_steps(True, 2, False)
    assert len(calls) == 2
    assert_same_run(plain, off, "every option off")
    assert torch.equal(plain["grads"], off["grads"])


@pytest.mark.parametrize("case", ["fuse0", "fuse3", "fuse0-three-calls", "fuse3-three-calls", "accumulate2"])
def test_native_step_with_the_options_equals_the_general_path_bitwise(VM, case):
    from neurovit_amd._cabi import lib
    kw = dict(label_smoothing=0.1, class_weight=STEP_WEIGHTS)
    acc = 2 if case == "accumulate2" else 1
    fuse = 3 if case.startswith("fuse3") else 0
    lib.nv_vit_set_head_step(0 if case.endswith("three-calls") else 1)
    try:
        a = run_steps(True, 2 * acc, True, accumulation_steps=acc, fuse_update=fuse, **kw)
        assert a["step"].last_fuse_update == (0 if acc > 1 else fuse)
        # the step's own d(loss)/d(logits) against the float64 formula on the step's own logits
        x, y, table = step_batch()
        want_loss, want_dl = M.ce_soft_ref(a["logits"].cpu().double().numpy(), y.cpu().numpy(), 0.1, STEP_WEIGHTS, table.cpu().numpy())
        dl = a["vit"]._rt.current.dlogits
        assert abs(a["losses"][-1].item() - want_loss) < FP32_GATE * abs(want_loss) and rel_err(dl, want_dl) < FP32_GATE
    finally:
        lib.nv_vit_set_head_step(1)
    b = run_steps(False, 2 * acc, True, accumulation_steps=acc, **kw)
    assert_same_run(a, b, case)
    plain = run_steps(True, 2 * acc, False, accumulation_steps=acc, fuse_update=fuse)
    assert not torch.equal(plain["params"], a["params"]) and not torch.equal(plain["losses"], a["losses"])       # the options do something


@pytest.mark.parametrize("case", ["fp16-dynamic-scale", "clipped", "static-scale"])
def test_scaled_and_clipped_steps_with_the_options_stay_bit_equal(VM, case):
    kw = dict(label_smoothing=0.1, class_weight=STEP_WEIGHTS)
    model_kw = {}
    if case == "fp16-dynamic-scale":
        model_kw = dict(TRAINING_VIT_OPERANDS="fp16")
    elif case == "clipped":
        kw["max_grad_norm"] = 0.05
    else:
        kw["loss_scale"] = 1024.0
    a = run_steps(True, 2, True, model_kw=model_kw, **kw)
    b = run_steps(False, 2, True, model_kw=model_kw, **kw)
    assert (a["step"].scaler is not None) == (case == "fp16-dynamic-scale")
    assert torch.isfinite(a["losses"]).all()
    assert_same_run(a, b, case)
    if case == "clipped":
        assert torch.equal(a["step"].last_grad_norm, b["step"].last_grad_norm) and a["step"].last_clip_coef.item() < 1.0


def test_graph_replay_is_not_taken_with_an_option_on(VM, monkeypatch):
    from neurovit_amd.trainer import TrainStep
    monkeypatch.setenv("NEUROVIT_GRAPH_STEP", "1")
    x, y, table = step_batch()
    step = TrainStep(micro_model(), label_smoothing=0.1)
    assert step._graphs_on
    for _ in range(6):
        step(x, y, mix=table)
    assert step._graphs == {} and step._graph_seen == {} and step.last_path == "native"
    for bad, err in ((table[:2], ValueError), (table.cpu(), RuntimeError), (table.float(), ValueError)):
        with pytest.raises(err, match="TrainStep: mix must"):
            step(x, y, mix=bad)


def test_neuro4d_trains_a_step_against_the_mixed_smoothed_target(VM, tmp_path):
    import neurovit_amd.NeuroEncoder as ne
    from neurovit_amd.trainer import TrainStep
    S, p, T = 16, 8, 8
    torch.manual_seed(11)
    m3 = ne.NeuroEncoder(W.neuro_config(S, p, DEVICE="cuda", **SIZE))
    torch.save(m3.state_dict(), str(tmp_path / "c.pth"))
    cfg4 = W.neuro_config(S, p, dim=4, DEVICE="cuda", GLOBAL_BASE_PATH=str(tmp_path), BEST_MODEL_PATH="c.pth", TRAINING_LEARNING_RATE=1e-2, **SIZE)
    torch.manual_seed(12)
    model = ne.NeuroEncoder(cfg4)
    model.train(); model.volume_encoder.eval()
    x = W.make_volume((4, S, S, S, T), 13).cuda()
    y = torch.tensor([0, 1, 1, 0], device="cuda")
    table = torch.tensor([mix_row(3, 1, 0.3), mix_row(2, 2, 0.5, label=0.6, box=(0, 8, 0, 16, 0, 12)), mix_row(1), mix_row(0, 1, 0.9)], dtype=torch.int32).cuda()
    step = TrainStep(model, label_smoothing=0.1)
    before = [q.detach().clone() for q in model.parameters() if q.requires_grad]
    loss = step(x, y, mix=table)
    assert step.last_path == "general"
    want, _ = M.ce_soft_ref(step.last_outputs.cpu().double().numpy(), y.cpu().numpy(), 0.1, None, table.cpu().numpy())
    assert abs(loss.item() - want) < FP32_GATE * abs(want)
    assert any(not torch.equal(a, b) for a, b in zip(before, [q for q in model.parameters() if q.requires_grad]))


def test_fp8_training_forward_takes_the_general_path_with_the_options(VM):
    """The fp8 training forward stays on the general path; with mix + smoothing + weights on it simply works: the loss is the restatement
    on the step's own logits, and parameters move."""
    from neurovit_amd.trainer import TrainStep
    x, y, table = step_batch()
    model = micro_model()
    vit = model.volume_encoder.vit3d
    vit.enable_fp8(x.permute(0, 3, 1, 2).unsqueeze(1), out_proj=False, training=True)
    assert vit.fp8_training
    step = TrainStep(model, label_smoothing=0.1, class_weight=STEP_WEIGHTS)
    before = vit.flat_parameters()[0].clone()
    loss = step(x, y, mix=table)
    assert step.last_path == "general"
    want, _ = M.ce_soft_ref(step.last_outputs.cpu().double().numpy(), y.cpu().numpy(), 0.1, STEP_WEIGHTS, table.cpu().numpy())
    assert abs(loss.item() - want) < FP32_GATE * abs(want) and not torch.equal(before, vit.flat_parameters()[0])


# ------------------------------------------------------------------ the Trainer shell
class Volumes40(torch.utils.data.Dataset):
    """DatasetADNI's 7-tuples with UNCROPPED volumes: six 40^3 volumes for a 32^3 model"""

    def __init__(self, size=40):
        self.x = W.make_volume((6, size, size, size), 4)
        self.y = torch.tensor([0, 1, 1, 0, 1, 0])

    def __len__(self):
        return 6

    def __getitem__(self, i):
        return f"s{i}", torch.tensor(0), self.x[i], torch.tensor(0), torch.tensor(1), torch.tensor(70), self.y[i]


def trainer_config(tmp_path, **extra):
    return W.neuro_config(32, 8, DEVICE="cuda", TRAINING_LEARNING_RATE=1e-3, TRAINING_WEIGHT_DECAY=1e-2, GLOBAL_OUTPUT_DIR=str(tmp_path / "runs"),
                          TRAINING_EPOCHS=1, TRAINING_BATCH_SIZE=2, TRAINING_NUM_WORKERS=0, **SIZE, **extra)


def test_trainer_mixes_training_batches_and_validates_plainly(VM, tmp_path, monkeypatch):
    from neurovit_amd.NeuroEncoder import NeuroEncoder
    from neurovit_amd.trainer import Trainer
    flips = (0.5, 0.5, 0.5)
    cfg = trainer_config(tmp_path, DATASET_TRANSFORMS=True, AUGMENT_FLIP_PROB=flips, AUGMENT_SEED=13, AUGMENT_MIXUP_ALPHA=0.4, AUGMENT_CUTMIX_ALPHA=1.0,
                         AUGMENT_MIX_PROB=1.0, AUGMENT_MIX_SWITCH_PROB=0.5, TRAINING_LABEL_SMOOTHING=0.1, TRAINING_CLASS_WEIGHTS=[0.5, 2.0])
    torch.manual_seed(5)
    model = NeuroEncoder(cfg)
    data = Volumes40()
    monkeypatch.setattr(torch.utils.data.DataLoader, "__init__", with_shuffle_off(torch.utils.data.DataLoader.__init__))
    tr = Trainer(cfg, model, data, data)
    assert isinstance(tr.mix, VM) and (tr.mix.mixup_alpha, tr.mix.cutmix_alpha, tr.mix.prob, tr.mix.switch_prob, tr.mix.seed) == (0.4, 1.0, 1.0, 0.5, 13)
    assert tr.step.criterion.label_smoothing == 0.1 and tr.step.criterion.weight.tolist() == [0.5, 2.0]
    assert tr.criterion.label_smoothing == 0.0 and tr.criterion.weight.tolist() == [0.5, 2.0]          # validation: unsmoothed, weighted
    seen = []
    run = tr.step._step

    def step_spy(fmri, labels, mix=None):
        loss = run(fmri, labels, mix)
        seen.append((fmri.clone(), labels.clone(), None if mix is None else mix.clone(), tr.mix.last_mix, tr.augment.last_params.clone(), loss,
                     tr.step.last_outputs.clone()))
        return loss
    tr.step._step = step_spy
    tr.train(0)
    assert len(seen) == 3 and tr.global_step == 3
    for n, (fmri, labels, mix, last, params, loss, logits) in enumerate(seen):
        assert mix is not None and mix is not last and torch.equal(mix, last)                         # last_mix is that step's table
        assert torch.equal(mix, tr.mix.params(2, n, (32, 32, 32))) and (mix[:, 1] != 0).all()
        assert torch.equal(params.cpu(), R.params_ref(2, n, (40, 40, 40), (32, 32, 32), flip_prob=flips, seed=13))
        batch = data.x[2 * n:2 * n + 2]
        want, moved = M.mix_apply_ref(batch, params.cpu(), mix.cpu(), (32, 32, 32), 0.0)
        assert fmri.shape == (2, 32, 32, 32) and M.same_bits(fmri.cpu(), want, moved), n               # the step saw the mixed batch
        assert torch.equal(labels.cpu(), data.y[2 * n:2 * n + 2])                                     # ... and the samples' own labels
        want_loss, _ = M.ce_soft_ref(logits.cpu().double().numpy(), labels.cpu().numpy(), 0.1, [0.5, 2.0], mix.cpu().numpy())
        assert abs(loss.item() - want_loss) < FP32_GATE * abs(want_loss)
    # validation: never mixed or smoothed, weighted
    outputs = []
    hook = model.register_forward_hook(lambda m, args, out: outputs.append((args[0].clone(), out.detach().clone())))
    val_loss, acc = tr.validate(0)
    hook.remove()
    assert len(outputs) == 3
    total = 0.0
    for n, (inp, logits) in enumerate(outputs):
        assert torch.equal(inp, data.x[2 * n:2 * n + 2, 4:36, 4:36, 4:36].cuda())
        total += torch.nn.functional.cross_entropy(logits.double(), data.y[2 * n:2 * n + 2].cuda(), weight=torch.tensor([0.5, 2.0], dtype=torch.float64, device="cuda")).item()
    assert abs(val_loss - round(total / 3, 5)) < 2e-5


def with_shuffle_off(init):
    def patched(self, *a, **kw):
        kw["shuffle"] = False
        return init(self, *a, **kw)
    return patched


def test_trainer_without_the_keys_is_the_plain_train_step_loop(VM, tmp_path, monkeypatch):
    from neurovit_amd.NeuroEncoder import NeuroEncoder
    from neurovit_amd.nn import CrossEntropyLoss
    from neurovit_amd.trainer import Trainer, TrainStep
    monkeypatch.setattr(torch.utils.data.DataLoader, "__init__", with_shuffle_off(torch.utils.data.DataLoader.__init__))
    data = Volumes40(32)
    cfg = trainer_config(tmp_path)
    sd = W.make_tensors(W.vit_param_spec(**W.MICRO), 1, prefix="volume_encoder.vit3d.")
    model = NeuroEncoder(cfg)
    model.load_state_dict(sd, strict=True)
    tr = Trainer(cfg, model, data, data)
    assert tr.mix is None and tr.augment is None and tr.criterion.weight is None and tr.criterion.label_smoothing == 0.0
    assert tr.step.criterion.weight is None and tr.step.criterion.label_smoothing == 0.0 and tr.step._loss_opts(data.y[:2].cuda(), None) is None
    calls = []
    run = tr.step._step

    def two_argument_spy(fmri, labels):                                      # the call Trainer made before: no third argument
        calls.append(1)
        return run(fmri, labels)
    tr.step._step = two_argument_spy
    tr.train(0)
    assert len(calls) == 3
    ref = NeuroEncoder(cfg)
    ref.load_state_dict(sd, strict=True)
    ref.train()
    step = TrainStep(ref)
    for n in range(3):
        step(data.x[2 * n:2 * n + 2].cuda(), data.y[2 * n:2 * n + 2].cuda())
    a, b = model.volume_encoder.vit3d, ref.volume_encoder.vit3d
    assert torch.equal(a.flat_parameters()[0], b.flat_parameters()[0]) and torch.equal(a.flat_parameters()[1], b.flat_parameters()[1])
