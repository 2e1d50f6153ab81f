"""The regression objective's restatement (tests/regression_ref.py) proven on the CPU: against float64 torch autograd over F.mse_loss /
F.l1_loss / F.huber_loss, the metrics against a direct computation, the planted defects each caught by the GPU gate on the GPU tests' own
inputs, the input conditions those gates rest on, and the Python-level refusals that need no device."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import regression_ref as R


def case(B, K):
    ins = R.head_inputs(B, K, 100 * B + K)
    return ins, R.head_logits_ref(*ins), R.mix_table(B)


def torch_loss(z, y, kind, delta, mean, std, w, mix):
    """the definition through torch autograd in double: F.*_loss over the valid cells, weighted, divided by the weight of the valid cells"""
    z = torch.tensor(z, dtype=torch.float64, requires_grad=True)
    yt = torch.tensor(np.asarray(y, dtype=np.float32)).double()
    B, K = z.shape
    valid = torch.isfinite(yt)
    t = torch.where(valid, yt, torch.zeros_like(yt))
    if mean is not None:
        t = (t - torch.tensor(mean).double()) / torch.tensor(std).double()
    if mix is not None:
        p = torch.tensor(mix[:, 0].astype(np.int64))
        lam = torch.tensor(mix[:, 3].astype(np.int32).view(np.float32).astype(np.float64))[:, None]
        t, valid = lam * t + (1.0 - lam) * t[p], valid & valid[p]
    wk = (torch.ones(K, dtype=torch.float64) if w is None else torch.tensor(w).double())[None, :].expand(B, K)
    fn = {"mse": F.mse_loss, "l1": F.l1_loss, "huber": lambda a, b, reduction: F.huber_loss(a, b, reduction=reduction, delta=delta)}[kind]
    cells = fn(z[valid], t[valid], reduction="none")
    loss = (wk[valid] * cells).sum() / wk[valid].sum()
    loss.backward()
    return loss.item(), z.grad.numpy()


@pytest.mark.parametrize("B,K", [(1, 1), (3, 3), (257, 3), (3, 300)])
def test_restatement_equals_float64_autograd(B, K):
    ins, z, mix = case(B, K)
    for kind, scaled, wname, with_nan, mixed in R.variants(K):
        m = mix if mixed else None
        mean, std = R.scale_of(scaled, K)
        y = R.targets_for(z, scaled, with_nan, m, seed=B + K)
        w = R.weights_of(K, B)[wname]
        got_loss, got_d = R.reg_loss_ref(z, y, kind, R.DELTA, mean, std, w, m)
        want_loss, want_d = torch_loss(z, y, kind, R.DELTA, mean, std, w, m)
        assert abs(got_loss - want_loss) <= 1e-12 * abs(want_loss), (kind, scaled, wname, with_nan, mixed)
        assert np.abs(got_d - want_d).max() <= 1e-12 * np.abs(want_d).max()
        assert (got_d[~np.isfinite(y)] == 0.0).all()
        half_loss, half_d = R.reg_loss_ref(z, y, kind, R.DELTA, mean, std, w, m, grad_scale=0.5)
        assert half_loss == got_loss and np.array_equal(half_d, 0.5 * got_d)


def test_l1_of_a_zero_residual_has_no_gradient_and_nothing_observed_is_zero():
    z = np.array([[0.5, -1.0]])
    loss, d = R.reg_loss_ref(z, np.array([[0.5, 0.0]], dtype=np.float32), "l1")
    assert d[0, 0] == 0.0 and d[0, 1] == -0.5 and loss == 0.5
    y = np.full((3, 2), np.nan, dtype=np.float32)
    loss, d = R.reg_loss_ref(np.ones((3, 2)), y, "mse")
    assert loss == 0.0 and not d.any()
    loss, d = R.reg_loss_ref(np.ones((3, 2)), np.zeros((3, 2), dtype=np.float32), "mse", mix=np.array([R.mix_row(3, 1, 0.5)] * 3, dtype=np.int32))
    assert np.isnan(loss)


@pytest.mark.parametrize("B,K", R.SHAPES)
def test_metrics_equal_a_direct_computation(B, K):
    batches = R.metric_batches(B, K, 5 * B + K)
    mean, std = R.scale_of(True, K)
    got = R.metrics_ref(batches, mean, std)
    z = np.concatenate([b[0] for b in batches])
    y = np.concatenate([b[1] for b in batches]).astype(np.float64)
    yh = ((z * np.float32(R.STD)).astype(np.float32) + np.float32(R.MEAN)).astype(np.float64)
    for k in range(K):
        ok = np.isfinite(y[:, k])
        e = yh[ok, k] - y[ok, k]
        want = [ok.sum(), np.mean(np.abs(e)), np.sqrt(np.mean(e ** 2)), np.mean(e), np.corrcoef(y[ok, k], yh[ok, k])[0, 1],
                1.0 - np.sum(e ** 2) / np.sum((y[ok, k] - y[ok, k].mean()) ** 2)]
        assert np.allclose(got[k], want, rtol=1e-12, atol=1e-12), (k, got[k], want)
    # what the GPU test's absolute gate on r / R^2 rests on: values an fp32 output resolves to 1e-6 (ulp(4) = 4.8e-7)
    assert (got[:, 0] >= R.METRIC_BATCHES - 1).all() and (np.abs(got[:, 4:]) < 4.0).all()


def test_metrics_undefined_cases_are_nan():
    one = [(np.zeros((1, 2), dtype=np.float32), np.array([[1.0, np.nan]], dtype=np.float32))]
    got = R.metrics_ref(one, None, None)
    assert got[0, 0] == 1 and got[0, 1] == 1.0 and np.isnan(got[0, 4:]).all()            # n = 1: errors defined, r / R^2 not
    assert got[1, 0] == 0 and np.isnan(got[1, 1:]).all()                                   # n = 0: nothing defined
    flat = [(np.arange(4, dtype=np.float32)[:, None], np.full((4, 1), 75.0, dtype=np.float32))]
    got = R.metrics_ref(flat, None, None)
    assert got[0, 0] == 4 and np.isfinite(got[0, 1:4]).all() and np.isnan(got[0, 4:]).all()   # zero variance of the targets


DEFECTS = {"denominator_BK": dict(with_nan=True), "mask_dropped": dict(with_nan=True), "huber_swapped": dict(kinds=("huber",)),
           "partner_validity": dict(with_nan=True, mixed=True)}


@pytest.mark.parametrize("defect", sorted(DEFECTS))
@pytest.mark.parametrize("B,K", R.SHAPES)
def test_planted_defects_move_the_result_by_more_than_the_gpu_gate(B, K, defect):
    """on the GPU tests' own inputs: every variant the defect can touch at this shape shows it above FP32_GATE"""
    ins, z, mix = case(B, K)
    need = DEFECTS[defect]
    touched = 0
    for kind, scaled, wname, with_nan, mixed in R.variants(K):
        if kind not in need.get("kinds", R.KINDS) or (need.get("with_nan") and not with_nan) or (need.get("mixed") and not mixed):
            continue
        m = mix if mixed else None
        mean, std = R.scale_of(scaled, K)
        y = R.targets_for(z, scaled, with_nan, m, seed=B + K)
        if need.get("with_nan") and not np.isnan(y).any():
            continue                                             # (a shape whose NaN pattern leaves no cell: nothing for a mask defect to do)
        if defect == "partner_validity" and not (np.isnan(y)[mix[:, 0]] & ~np.isnan(y)).any():
            continue
        w = R.weights_of(K, B)[wname]
        loss, d = R.reg_loss_ref(z, y, kind, R.DELTA, mean, std, w, m)
        bad_loss, bad_d = R.reg_loss_ref(z, y, kind, R.DELTA, mean, std, w, m, defect=defect)
        moved = max(abs(bad_loss - loss) / abs(loss), np.abs(bad_d - d).max() / np.abs(d).max())
        assert moved > 10 * R.FP32_GATE, (kind, scaled, wname, with_nan, mixed, moved)
        touched += 1
    if defect == "huber_swapped":
        assert touched > 0
    elif B > 1:
        assert touched > 0                                       # (B = 1 pairs with itself and keeps every cell: no NaN to mishandle)


@pytest.mark.parametrize("B,K", R.SHAPES)
def test_input_conditions_of_the_gpu_gates(B, K):
    ins, z, mix = case(B, K)
    for scaled, with_nan, mixed in [(s, n, m) for s in (False, True) for n in (False, True) for m in (False, True)]:
        m = mix if mixed else None
        mean, std = R.scale_of(scaled, K)
        y = R.targets_for(z, scaled, with_nan, m, seed=B + K)
        r, valid = R.residuals(z, y, mean, std, m)
        a = np.abs(r[valid])
        assert a.size and (a >= R.MARGIN).all() and (np.abs(a - R.DELTA) >= R.MARGIN).all()
        assert (a > R.DELTA).any() or a.size < 3                 # both huber branches are taken
        for w in R.weights_of(K, B).values():
            assert (valid * (1.0 if w is None else w[None, :])).sum() > 0                # D > 0 in every case that is not planted
        if with_nan and B > 1:
            assert np.isnan(y).any()


def test_planted_missing_batch_and_missing_column():
    z = R.head_logits_ref(*R.head_inputs(3, 3, 1))
    y = R.targets_for(z, True, False, None, seed=1)
    gone = np.full_like(y, np.nan)
    assert R.reg_loss_ref(z, gone, "huber", R.DELTA, *R.scale_of(True, 3))[0] == 0.0
    col = y.copy()
    col[:, 1] = np.nan
    loss, d = R.reg_loss_ref(z, col, "mse", 1.0, *R.scale_of(True, 3))
    assert loss > 0 and not d[:, 1].any() and d[:, 0].all() and d[:, 2].all()


def test_python_refusals_need_no_device():
    from neurovit_amd import ops
    from neurovit_amd.nn import RegressionLoss
    from neurovit_amd.trainer import target_stats
    with pytest.raises(ValueError):
        ops.reg_opts("quantile")
    with pytest.raises(ValueError):
        ops.reg_opts("huber", delta=0.0)
    with pytest.raises(TypeError):
        ops.reg_opts("huber", delta="1")
    with pytest.raises(RuntimeError):
        ops.reg_opts("mse", mean=torch.zeros(2))                  # a CPU tensor: there is no CPU fallback
    with pytest.raises(ValueError):
        RegressionLoss("huber", delta=-1.0)
    with pytest.raises(ValueError):
        RegressionLoss(target_std=[1.0, 0.0])
    with pytest.raises(ValueError):
        RegressionLoss(weight=[-1.0])
    with pytest.raises(RuntimeError):
        RegressionLoss()(torch.zeros(2, 1), torch.zeros(2))
    with pytest.raises(ValueError):
        ops.reg_targets(torch.zeros(3, 2), 3, 1)
    assert ops.reg_targets(torch.arange(3), 3, 1).dtype == torch.float32
    mean, std = target_stats([[60.0, 1.0], [80.0, float("nan")], [70.0, 3.0]])
    assert mean == [70.0, 2.0] and abs(std[0] - (200.0 / 3) ** 0.5) < 1e-12 and std[1] == 1.0
    with pytest.raises(ValueError):
        target_stats([float("nan")])


def test_regression_config_keys_build_the_head_and_refuse_the_4d_model():
    import weights as W
    from neurovit_amd.NeuroEncoder import NeuroEncoder
    size = dict(TRAINING_VIT_DIM=128, TRAINING_VIT_DEPTH=2, TRAINING_VIT_HEADS=2, TRAINING_VIT_MLP_DIM=256)
    cfg = W.neuro_config(32, 8, DEVICE="cpu", TRAINING_OBJECTIVE="regression", REGRESSION_TARGETS=3, REGRESSION_TARGET_MEAN=[70.0, 0.0, 1.0],
                         REGRESSION_TARGET_STD=[8.0, 1.0, 2.0], **size)
    model = NeuroEncoder(cfg)
    plain = NeuroEncoder(W.neuro_config(32, 8, DEVICE="cpu", **size))
    assert model.is_regression and not plain.is_regression
    assert model.volume_encoder.vit3d._cfg.num_classes == 3 and list(model.state_dict()) == list(plain.state_dict())     # the keys stay the reference's
    assert model.volume_encoder.target_std.tolist() == [8.0, 1.0, 2.0]
    with pytest.raises(RuntimeError):
        plain.predict(torch.zeros(1, 32, 32, 32))
    with pytest.raises(ValueError):
        NeuroEncoder(dict(cfg, REGRESSION_TARGET_STD=[8.0, 0.0, 2.0]))
    with pytest.raises(ValueError):
        NeuroEncoder(dict(cfg, REGRESSION_TARGETS=0))
    with pytest.raises(NotImplementedError):
        NeuroEncoder(dict(cfg, TRAINING_DIM=4))
