"""The regression objective on the MI355X: the loss kernels (nv_reg_loss, nv_head_step_reg) and the metrics held to the float64 restatement
(tests/regression_ref.py; what it is worth is proven in tests/test_regression_cpu.py), the train step on its three paths bit-equal to each
other, the model's raw-scale predictions and attribution on a regression model."""
import ctypes

import numpy as np
import pytest
import torch

import regression_ref as R
import weights as W
from conftest import rel_err

pytestmark = pytest.mark.gpu

FP32_GATE = R.FP32_GATE


@pytest.fixture(scope="module")
def ops():
    from neurovit_amd._cabi import require_gpu
    require_gpu()
    from neurovit_amd import ops
    return ops


def dev(t):
    if t is None:
        return None
    return (torch.from_numpy(np.ascontiguousarray(t)) if isinstance(t, np.ndarray) else t).cuda()


# ------------------------------------------------------------------ the loss kernels
@pytest.mark.parametrize("B,K", R.SHAPES)
def test_loss_against_float64_and_between_its_entry_points(ops, B, K):
    ins = R.head_inputs(B, K, 100 * B + K)
    z64, mix = R.head_logits_ref(*ins), R.mix_table(B)
    args = [dev(t) for t in ins]
    plain = ops.head_step(*args, torch.zeros(B, dtype=torch.int64, device="cuda"))
    logits = plain[0]
    assert rel_err(logits, z64) < FP32_GATE                                  # the inputs' margins were proven on these logits
    worst = [0.0, 0.0]
    for kind, scaled, wname, with_nan, mixed in R.variants(K):
        m = mix if mixed else None
        mean, std = R.scale_of(scaled, K)
        y = R.targets_for(z64, scaled, with_nan, m, seed=B + K)
        w = R.weights_of(K, B)[wname]
        keep = [dev(t) for t in (mean, std, w, m)]
        opts = ops.reg_opts(kind, R.DELTA, *keep, B=B, K=K)
        yd = dev(y)
        out = ops.head_step_reg(*args, yd, opts)
        loss, dl = out[3], out[4]
        assert torch.equal(out[0], logits)                                   # the head's forward is the classifier's, bit for bit
        loss2, dl2 = ops.reg_loss(logits, yd, opts)
        assert torch.equal(loss, loss2) and torch.equal(dl, dl2), (kind, scaled, wname, with_nan, mixed)      # one row body: the same bits
        want_loss, want_dl = R.reg_loss_ref(logits.cpu().double().numpy(), y, kind, R.DELTA, mean, std, w, m)
        e_loss, e_dl = abs(loss.item() - want_loss) / abs(want_loss), rel_err(dl, want_dl)
        worst = [max(worst[0], e_loss), max(worst[1], e_dl)]
        assert e_loss < FP32_GATE and e_dl < FP32_GATE, (kind, scaled, wname, with_nan, mixed, e_loss, e_dl)
        assert (dl.cpu().numpy()[~np.isfinite(y)] == 0.0).all() and not np.signbit(dl.cpu().numpy()[~np.isfinite(y)]).any()   # exactly 0.0f
        if mixed:
            _, valid, _ = R.mixed_targets(y, mean, std, m)
            assert (dl.cpu().numpy()[~valid] == 0.0).all()
        # the rest of the head step is the classifier's backward over these dlogits
        g, dW = out[5], out[9]
        want = ops.head_bwd(dl, args[3], args[0], out[2], out[1], args[1])
        assert torch.equal(g, want[0]) and torch.equal(dW, want[4])
    print(f"regression loss B={B} K={K}: worst loss rel {worst[0]:.2e}, worst dpred rel {worst[1]:.2e}")


def test_scales_planted_zeros_missing_data_bad_partners_and_refusals(ops):
    from neurovit_amd._cabi import RegOpts, lib
    B, K = 3, 3
    ins = R.head_inputs(B, K, 7)
    z64, mix = R.head_logits_ref(*ins), R.mix_table(B)
    args = [dev(t) for t in ins]
    mean, std = (dev(t) for t in R.scale_of(True, K))
    w, m = dev(R.weights_of(K, B)["given"]), dev(mix)
    y = dev(R.targets_for(z64, True, True, mix, seed=3))
    opts = ops.reg_opts("huber", R.DELTA, mean, std, w, m)
    out = ops.head_step_reg(*args, y, opts)
    logits, loss, dl = out[0], out[3], out[4]
    state = torch.zeros(16, device="cuda")
    state[0] = 8.0
    loss_s, dl_s = ops.reg_loss(logits, y, opts, scale_state=state)
    assert torch.equal(loss_s, loss) and torch.equal(dl_s, dl * 8.0)                       # dpred carries state[0] (a power of two: exactly), the loss does not
    out_s = ops.head_step_reg(*args, y, opts, scale_state=state, grad_scale=0.5)
    assert torch.equal(out_s[3], loss) and torch.equal(out_s[4], dl * 4.0)
    loss_g, dl_g = ops.reg_loss(logits, y, opts, grad_scale=0.5)
    assert torch.equal(loss_g, loss) and torch.equal(dl_g, dl * 0.5)
    # planted exact zeros: y == z (no mean / std), so t == z in fp32 and l'(0) = 0 exactly, in every kind
    for kind in R.KINDS:
        o = ops.reg_opts(kind, R.DELTA)
        y0 = logits.clone()
        y0[1, 2] += 1.0
        l0, d0 = ops.reg_loss(logits, y0, o)
        assert (d0.flatten()[[i for i in range(B * K) if i != 5]] == 0).all() and d0[1, 2] != 0 and l0.item() > 0
        assert torch.equal(ops.head_step_reg(*args, y0, o)[4], d0)
    # D == 0: a fully missing batch, and a batch whose only observed column has no weight - loss 0, gradient 0 (not the cross-entropy's NaN)
    gone = torch.full((B, K), float("nan"), device="cuda")
    only0 = gone.clone()
    only0[:, 0] = 70.0
    w0 = torch.tensor([0.0, 1.0, 1.0], device="cuda")
    for yy, oo in ((gone, opts), (only0, ops.reg_opts("mse", 1.0, mean, std, w0))):
        l, d = ops.reg_loss(logits, yy, oo)
        h = ops.head_step_reg(*args, yy, oo)
        for ll, dd in ((l, d), (h[3], h[4])):
            assert ll.item() == 0.0 and not dd.any() and not torch.isnan(dd).any()
        assert not h[5].any() and not h[9].any()                                           # nothing flows back
    # a fully missing column among observed ones: exactly zero there
    col = dev(R.targets_for(z64, True, False, None, seed=3))
    col[:, 1] = float("nan")
    d = ops.reg_loss(logits, col, ops.reg_opts("l1", 1.0, mean, std))[1]
    assert not d[:, 1].any() and d[:, 0].all()
    # a non-finite prediction in a valid cell propagates
    zbad = logits.clone()
    zbad[0, 0] = float("inf")
    for kind in R.KINDS:
        l, d = ops.reg_loss(zbad, only0, ops.reg_opts(kind, R.DELTA, mean, std))
        assert not torch.isfinite(l).any() and not torch.isfinite(d[0, 0]) and torch.isfinite(d[1:, 0]).all()
    # a partner outside the batch: NaN, and the call returns
    outside = dev(np.array([R.mix_row(5, 1, 0.5), R.mix_row(1), R.mix_row(-1, 1, 0.5)], dtype=np.int32))
    o = ops.reg_opts("mse", 1.0, mean, std, None, outside)
    assert torch.isnan(ops.reg_loss(logits, y, o)[0]).all() and torch.isnan(ops.head_step_reg(*args, y, o)[3]).all()
    torch.cuda.synchronize()
    # refusals, before any launch
    for bad in (RegOpts(ctypes.sizeof(RegOpts), 7, 1.0, None, None, None, None), RegOpts(ctypes.sizeof(RegOpts), 2, 0.0, None, None, None, None),
                RegOpts(ctypes.sizeof(RegOpts) - 4, 0, 1.0, None, None, None, None)):
        with pytest.raises(RuntimeError, match="nv_reg_loss"):
            ops.reg_loss(logits, y, bad)
        with pytest.raises(RuntimeError, match="nv_head_step_reg"):
            ops.head_step_reg(*args, y, bad)
    wide = R.head_inputs(2, 8, 1)
    x8, g8, b8 = wide[0][:, :, :8], wide[1], wide[2]
    with pytest.raises(RuntimeError, match="nv_head_step_reg"):                            # K > d on the fused route
        ops.head_step_reg(x8.cuda(), g8.cuda(), b8.cuda(), torch.zeros(9, 8).cuda(), torch.zeros(9).cuda(), torch.zeros(2, 9).cuda())
    assert lib.nv_reg_loss(None, None, 0, 0, 1.0, None, None, None, None, None) != 0
    torch.cuda.synchronize()


def test_nn_regression_loss_is_differentiable(ops):
    from neurovit_amd.nn import RegressionLoss
    B, K = 5, 3
    mix = R.mix_table(B)
    z = torch.randn(B, K, device="cuda", requires_grad=True)
    w = R.weights_of(K, 1)["zero"]
    y = R.targets_for(z.detach().cpu().double().numpy(), True, True, mix, seed=2)
    mean, std = R.scale_of(True, K)
    crit = RegressionLoss("huber", R.DELTA, target_mean=mean, target_std=std, weight=w)
    loss = crit(z, torch.from_numpy(y).double().cuda(), dev(mix))                          # any real dtype: cast to fp32
    (2.0 * loss).backward()
    want_loss, want_d = R.reg_loss_ref(z.detach().cpu().double().numpy(), y, "huber", R.DELTA, mean, std, w, mix)
    assert abs(loss.item() - want_loss) < FP32_GATE * abs(want_loss) and rel_err(z.grad, 2.0 * want_d) < FP32_GATE
    z1 = torch.randn(B, 1, device="cuda")
    y1 = torch.randn(B, device="cuda")
    assert abs(RegressionLoss()(z1, y1).item() - torch.nn.functional.mse_loss(z1[:, 0], y1).item()) < 1e-6
    assert abs(RegressionLoss("l1")(z1, y1).item() - torch.nn.functional.l1_loss(z1[:, 0], y1).item()) < 1e-6


# ------------------------------------------------------------------ metrics
@pytest.mark.parametrize("B,K", R.SHAPES)
def test_metrics_against_the_restatement_and_reproducible(ops, B, K):
    batches = R.metric_batches(B, K, 5 * B + K)
    mean, std = R.scale_of(True, K)
    runs = []
    for _ in range(2):
        met = ops.RegressionMetrics(K, mean, std, "cuda")
        for z, y in batches:
            met.update(dev(z), dev(y))
        runs.append(met.compute_device().clone())
    assert torch.equal(runs[0].view(torch.int32), runs[1].view(torch.int32))               # one fixed order: the same bits
    got, want = runs[0].cpu().double().numpy(), R.metrics_ref(batches, mean, std)
    assert np.array_equal(got[:, 0], want[:, 0])
    defined = np.isfinite(want)
    assert np.array_equal(np.isfinite(got), defined)
    rel = np.abs(got[:, 1:4] - want[:, 1:4])[defined[:, 1:4]] / np.abs(want[:, 1:4])[defined[:, 1:4]]
    ab = np.abs(got[:, 4:] - want[:, 4:])[defined[:, 4:]]
    print(f"regression metrics B={B} K={K}: MAE/RMSE/bias rel {rel.max() if rel.size else 0:.2e}, r/R2 abs {ab.max() if ab.size else 0:.2e}")
    assert (rel < 1e-6).all() and (ab < 1e-6).all()
    named = met.compute()
    assert sorted(named) == ["bias", "mae", "n", "r", "r2", "rmse"] and named["mae"].shape == (K,)
    met.reset()
    assert not met.state.any()


def test_metrics_undefined_cases_are_nan(ops):
    met = ops.RegressionMetrics(2, None, None, "cuda")
    met.update(torch.zeros(1, 2, device="cuda"), torch.tensor([[1.0, float("nan")]], device="cuda"))
    got = met.compute_device().cpu()
    assert got[0, 0] == 1 and got[0, 1] == 1.0 and got[0, 2] == 1.0 and got[0, 3] == -1.0 and torch.isnan(got[0, 4:]).all()     # n = 1
    assert got[1, 0] == 0 and torch.isnan(got[1, 1:]).all()                                                                   # n = 0
    flat = ops.RegressionMetrics(1, [70.0], [8.0], "cuda")
    flat.update(torch.arange(4.0, device="cuda")[:, None], torch.full((4,), 75.0, device="cuda"))                             # zero variance of the targets
    got = flat.compute_device().cpu()
    assert got[0, 0] == 4 and torch.isfinite(got[0, 1:4]).all() and torch.isnan(got[0, 4:]).all()
    same = ops.RegressionMetrics(1, None, None, "cuda")
    same.update(torch.full((4, 1), 0.5, device="cuda"), torch.arange(4.0, device="cuda"))                                     # ... of the predictions: r undefined, R^2 defined
    got = same.compute_device().cpu()
    assert torch.isnan(got[0, 4]) and torch.isfinite(got[0, 5])


# ------------------------------------------------------------------ the train step
SIZE = dict(TRAINING_VIT_DIM=128, TRAINING_VIT_DEPTH=2, TRAINING_VIT_HEADS=2, TRAINING_VIT_MLP_DIM=256)
SCALE = {1: ([70.0], [8.0]), 3: ([70.0, 0.0, 25.0], [8.0, 1.0, 4.0])}
TARGETS = {1: [[78.0], [61.5], [73.25]], 3: [[78.0, 0.5, 22.0], [61.5, float("nan"), 31.0], [73.25, -1.25, 27.5]]}
WEIGHT = {1: None, 3: [1.0, 0.5, 2.0]}


def micro_model(K, **extra):
    import neurovit_amd.NeuroEncoder as ne
    cfg = W.neuro_config(32, 8, DEVICE="cuda", TRAINING_LEARNING_RATE=1e-3, TRAINING_WEIGHT_DECAY=1e-2, TRAINING_OBJECTIVE="regression", REGRESSION_TARGETS=K,
                         REGRESSION_TARGET_MEAN=SCALE[K][0], REGRESSION_TARGET_STD=SCALE[K][1], **SIZE, **extra)
    model = ne.NeuroEncoder(cfg)
    model.load_state_dict(W.make_tensors(W.vit_param_spec(**dict(W.MICRO, num_classes=K)), 1, prefix="volume_encoder.vit3d."), strict=True)
    model.train()
    return model


def step_batch(K):
    x = W.make_volume((3, 32, 32, 32), 2).cuda()
    y = torch.tensor(TARGETS[K], device="cuda")
    mix = torch.tensor([R.mix_row(2, 1, 0.3), R.mix_row(1), R.mix_row(0, 2, 0.7)], dtype=torch.int32).cuda()
    return x, y, mix


def step_kw(K, kind="huber"):
    return dict(objective="regression", regression_loss=kind, huber_delta=R.DELTA, target_mean=SCALE[K][0], target_std=SCALE[K][1], target_weight=WEIGHT[K])


def run_steps(native, n, K, mix=True, model_kw=None, kind="huber", **kw):
    from neurovit_amd.trainer import TrainStep
    x, y, table = step_batch(K)
    model = micro_model(K, **(model_kw or {}))
    step = TrainStep(model, **step_kw(K, kind), **kw)
    if not native:
        step._native = False
    torch.manual_seed(11)
    losses = [step(x, y, mix=table).clone() if mix else step(x, y).clone() for _ in range(n)]
    assert step._native == native and step.last_path == ("native" if native else "general")
    vit = model.volume_encoder.vit3d
    m, v = step.optimizer.arena_state(vit)
    return dict(losses=torch.stack(losses), logits=step.last_outputs.clone(), params=vit.flat_parameters()[0].clone(), shadow=vit.flat_parameters()[1].clone(),
                m=m.clone(), v=v.clone(), step=step, vit=vit, model=model)


def assert_same_run(a, b, what):
    for name in ("losses", "logits", "params", "shadow", "m", "v"):
        assert torch.equal(a[name], b[name]), f"{what}: {name} differ"


@pytest.mark.parametrize("K", [1, 3])
@pytest.mark.parametrize("case", ["fuse0", "fuse3", "fuse0-three-calls", "fuse3-three-calls", "accumulate2"])
def test_native_regression_step_equals_the_general_path_bitwise(ops, case, K):
    from neurovit_amd._cabi import lib
    acc = 2 if case == "accumulate2" else 1
    fuse = 3 if case.startswith("fuse3") else 0
    kind = {"fuse0": "mse", "fuse3": "huber", "fuse0-three-calls": "l1", "fuse3-three-calls": "huber", "accumulate2": "mse"}[case]
    lib.nv_vit_set_head_step(0 if case.endswith("three-calls") else 1)
    try:
        a = run_steps(True, 2 * acc, K, accumulation_steps=acc, fuse_update=fuse, kind=kind)
        assert a["step"].last_fuse_update == (0 if acc > 1 else fuse)
        x, y, table = step_batch(K)
        want_loss, want_dl = R.reg_loss_ref(a["logits"].cpu().double().numpy(), y.cpu().numpy(), kind, R.DELTA, np.float32(SCALE[K][0]), np.float32(SCALE[K][1]),
                                            WEIGHT[K], table.cpu().numpy())
        dl = a["vit"]._rt.current.dlogits
        assert abs(a["losses"][-1].item() - want_loss) < FP32_GATE * abs(want_loss) and rel_err(dl, want_dl) < FP32_GATE
        assert torch.isfinite(a["losses"]).all()
    finally:
        lib.nv_vit_set_head_step(1)
    b = run_steps(False, 2 * acc, K, accumulation_steps=acc, kind=kind)
    assert_same_run(a, b, case)


@pytest.mark.parametrize("case", ["fp16-dynamic-scale", "clipped", "static-scale", "drop-path", "ema-groups"])
def test_scaled_clipped_and_dropped_regression_steps_stay_bit_equal(ops, case):
    kw, model_kw = {}, {}
    if case == "fp16-dynamic-scale":
        model_kw = dict(TRAINING_VIT_OPERANDS="fp16")
    elif case == "clipped":
        kw["max_grad_norm"] = 0.05
    elif case == "static-scale":
        kw["loss_scale"] = 1024.0
    elif case == "drop-path":
        model_kw = dict(TRAINING_DROP_PATH=0.1)
    else:
        kw.update(ema_decay=0.9, no_decay=True, layer_decay=0.75)
    a = run_steps(True, 2, 3, model_kw=model_kw, **kw)
    b = run_steps(False, 2, 3, model_kw=model_kw, **kw)
    assert (a["step"].scaler is not None) == (case == "fp16-dynamic-scale")
    assert torch.isfinite(a["losses"]).all()
    assert_same_run(a, b, case)
    if case == "ema-groups":
        for p, q in zip(a["step"].ema.module.parameters(), b["step"].ema.module.parameters()):
            assert torch.equal(p, q)


def test_regression_step_takes_no_graph_and_leaves_the_classifier_alone(ops, monkeypatch):
    from neurovit_amd.trainer import TrainStep
    monkeypatch.setenv("NEUROVIT_GRAPH_STEP", "1")
    x, y, _ = step_batch(1)
    step = TrainStep(micro_model(1), **step_kw(1))
    assert step._graphs_on
    for _ in range(6):
        step(x, y)
    assert not step._graphs and not step._graph_seen and step.last_path == "native"
    with pytest.raises(ValueError):
        TrainStep(micro_model(1), objective="regression", label_smoothing=0.1)
    with pytest.raises(ValueError):
        TrainStep(micro_model(1), objective="regression", class_weight=[1.0])
    with pytest.raises(ValueError):
        TrainStep(micro_model(1), objective="ordinal")
    with pytest.raises(ValueError):
        TrainStep(micro_model(3), objective="regression", target_mean=[1.0])


def test_native_dp_regression_step_on_a_one_rank_rccl_communicator_equals_the_single_process_step(ops):
    from neurovit_amd.trainer import TrainStep
    single = run_steps(True, 3, 3, fuse_update=0)
    x, y, table = step_batch(3)
    model = micro_model(3)
    step = TrainStep(model, n_buckets=3, native_dp=True, **step_kw(3))
    torch.manual_seed(11)
    losses = torch.stack([step(x, y, mix=table).clone() for _ in range(3)])
    torch.cuda.synchronize()
    assert step.last_path == "native-dp" and step.last_dp["messages"] == "fp32"
    assert torch.equal(losses, single["losses"]) and torch.equal(model.volume_encoder.vit3d.flat_parameters()[0], single["params"])


def test_state_dict_round_trip_resumes_bit_for_bit(ops):
    from neurovit_amd.trainer import TrainStep
    straight = run_steps(True, 4, 3, ema_decay=0.9)
    half = run_steps(True, 2, 3, ema_decay=0.9)
    state, weights = half["step"].state_dict(), {k: v.clone() for k, v in half["model"].state_dict().items()}
    assert state["objective"] == "regression" and state["kind"] == "huber" and state["delta"] == R.DELTA
    assert state["mean"].tolist() == SCALE[3][0] and state["std"].tolist() == SCALE[3][1]
    model = micro_model(3)
    model.load_state_dict(weights, strict=True)
    step = TrainStep(model, ema_decay=0.9, **step_kw(3))
    step.load_state_dict(state)
    x, y, table = step_batch(3)
    losses = [step(x, y, mix=table).clone() for _ in range(2)]
    vit = model.volume_encoder.vit3d
    assert torch.equal(torch.stack(losses), straight["losses"][2:]) and torch.equal(vit.flat_parameters()[0], straight["params"])
    m, v = step.optimizer.arena_state(vit)
    assert torch.equal(m, straight["m"]) and torch.equal(v, straight["v"])
    for p, q in zip(step.ema.module.parameters(), straight["step"].ema.module.parameters()):
        assert torch.equal(p, q)
    # a state of another objective, loss or scale is refused before anything is copied
    for other in (TrainStep(micro_model(3), ema_decay=0.9), TrainStep(micro_model(3), ema_decay=0.9, **step_kw(3, "mse")),
                  TrainStep(micro_model(3), ema_decay=0.9, **dict(step_kw(3), target_mean=[71.0, 0.0, 25.0]))):
        with pytest.raises(ValueError):
            other.load_state_dict(state)
    classifier = TrainStep(micro_model(3)).state_dict()
    assert "objective" not in classifier and "kind" not in classifier                     # a classifier's state is what it always was
    with pytest.raises(ValueError):
        step.load_state_dict(classifier)


# ------------------------------------------------------------------ the model's raw scale
def test_predict_returns_raw_scale_predictions(ops):
    model = micro_model(3).eval()
    x = step_batch(3)[0]
    with torch.no_grad():
        z = model(x).float()
    want = z * torch.tensor(SCALE[3][1], device="cuda") + torch.tensor(SCALE[3][0], device="cuda")
    got = model.predict(x)
    assert got.shape == (3, 3) and torch.equal(got, want) and not got.requires_grad


# ------------------------------------------------------------------ the Trainer shell
def planted_set(n, seed):
    """n volumes a_i * pattern + noise with the target 70 + 8 a_i (a known linear function of the planted intensity), as 7-tuples in the
    ADNI order: the volume is element 2, the target (`age`) element -2, a class label the last"""
    g = torch.Generator().manual_seed(seed)
    pattern = torch.randn(32, 32, 32, generator=torch.Generator().manual_seed(99))
    a = torch.rand(n, generator=g) * 2 - 1
    vol = a[:, None, None, None] * pattern + 0.3 * torch.randn(n, 32, 32, 32, generator=g)
    age = 70.0 + 8.0 * a
    ids = torch.arange(n)
    return torch.utils.data.TensorDataset(ids, ids.clone(), vol, ids.clone(), ids.clone(), age, (a > 0).long())


def trainer_config(**extra):
    return dict(W.neuro_config(32, 8, DEVICE="cuda", TRAINING_LEARNING_RATE=1e-3, TRAINING_WEIGHT_DECAY=1e-2, TRAINING_OBJECTIVE="regression",
                               REGRESSION_TARGET_MEAN=[70.0], REGRESSION_TARGET_STD=[8.0], **SIZE),
                GLOBAL_OUTPUT_DIR="unused", TRAINING_EPOCHS=2, TRAINING_BATCH_SIZE=4, TRAINING_NUM_WORKERS=0, **extra)


def test_trainer_learns_a_planted_target_and_reports_device_metrics(ops, monkeypatch, capsys):
    import neurovit_amd.NeuroEncoder as ne
    from neurovit_amd.trainer import Trainer, TrainStep
    torch.manual_seed(5)
    cfg = trainer_config(REGRESSION_LOSS="huber", REGRESSION_HUBER_DELTA=1.5, TRAINING_EMA_DECAY=0.5)
    model = ne.NeuroEncoder(cfg)
    train_set, val_set = planted_set(40, 1), planted_set(12, 2)
    t = Trainer(cfg, model, train_set, val_set)
    assert type(t.step) is TrainStep and t.step.objective == "regression" and t.step.criterion.kind == "huber" and t.step.criterion.delta == 1.5
    assert t._unpack([0, 1, 2, 3, 4, 5, 6]) == (2, 5)
    _, before = t.validate(-1)
    for epoch in range(2):
        t.train(epoch)
    assert t.step.last_path == "native" and "train_mae" in capsys.readouterr().out
    # one host read for the metrics of a validation pass: count what leaves the device
    reads = []
    for name in ("cpu", "item", "tolist", "numpy", "__float__", "__int__", "__bool__"):
        real = getattr(torch.Tensor, name)

        def spy(self, *a, _real=real, _name=name, **k):
            if self.is_cuda:
                reads.append(_name)
            return _real(self, *a, **k)
        monkeypatch.setattr(torch.Tensor, name, spy)
    t.validate_ema = False
    loss, after = t.validate(1)
    monkeypatch.undo()
    assert reads == ["cpu"], reads
    print(f"planted target: validation MAE {before[0]:.3f} -> {after[0]:.3f} over two epochs")
    assert after[0] < before[0]                                                           # validation MAE falls over two epochs
    # the logged metrics are RegressionMetrics over the same batches
    met = ops.RegressionMetrics(1, [70.0], [8.0], "cuda")
    model.eval()
    total = 0.0
    with torch.no_grad(), model.precision(t.validation_precision):
        for batch in t.val_dataloader:
            out = model(batch[2].cuda()).float()
            met.update(out, batch[-2].cuda())
            total += t.criterion(out, batch[-2].cuda()).item()
    want = met.compute()
    for key in ("mae", "rmse", "r", "r2"):
        assert t.val_metrics[key] == [round(float(want[key][0]), 5)], key
    assert t.val_metrics["n"] == [12.0] and abs(loss - round(total / len(t.val_dataloader), 5)) < 2e-5
    # the weight average is validated behind the model, and evaluate_samples reports per-sample predictions on the raw scale
    t.validate_ema = True
    t.validate(1)
    assert t.val_metrics_ema["n"] == [12.0] and "val_mae_ema" in capsys.readouterr().out
    mae, rows = t.evaluate_samples()
    assert len(rows) == 12 and abs(mae - t.val_metrics["mae"][0]) < 1e-3
    subject, prediction, actual = rows[3]
    with model.precision(t.validation_precision):
        want = float(model.predict(val_set[3][2][None].cuda())[0, 0])
    assert int(subject) == 3 and abs(actual - float(val_set[3][-2])) < 1e-6 and abs(prediction - want) < 1e-3


def test_trainer_mixes_targets_and_refuses_the_classifiers_loss_options(ops):
    import neurovit_amd.NeuroEncoder as ne
    from neurovit_amd.trainer import Trainer
    torch.manual_seed(6)
    cfg = trainer_config(AUGMENT_MIXUP_ALPHA=0.4, REGRESSION_TARGET_INDEX=5)
    model = ne.NeuroEncoder(cfg)
    data = planted_set(8, 3)
    t = Trainer(cfg, model, data, data)
    before = model.volume_encoder.vit3d.flat_parameters()[0].clone()
    t.train(0)
    assert t.mix.last_mix is not None and not torch.equal(before, model.volume_encoder.vit3d.flat_parameters()[0])
    assert torch.isfinite(model.volume_encoder.vit3d.flat_parameters()[0]).all()
    for bad in (dict(TRAINING_LABEL_SMOOTHING=0.1), dict(TRAINING_CLASS_WEIGHTS=[1.0, 2.0]), dict(REGRESSION_LOSS="quantile"),
                dict(REGRESSION_LOSS="huber", REGRESSION_HUBER_DELTA=0.0)):
        with pytest.raises(ValueError):
            Trainer(dict(trainer_config(), **bad), model, data, data)
    plain = dict(trainer_config())
    del plain["TRAINING_OBJECTIVE"]
    with pytest.raises(ValueError):                                                        # the key on the Trainer's side only: the model's head is a classifier's
        Trainer(trainer_config(), ne.NeuroEncoder(plain), data, data)


# ------------------------------------------------------------------ attribution on a regression model
def test_attribution_resolves_the_score_and_refuses_prob(ops):
    model = micro_model(3).eval()
    x = step_batch(3)[0][:2]
    maps, idx = model.occlusion_sensitivity(x)
    assert maps.shape == (2, 64) and idx.tolist() == [0, 0] and torch.isfinite(maps).all()       # target None: output 0, score "logit"
    want, _ = model.occlusion_sensitivity(x, target=0, score="logit")
    assert torch.equal(maps, want)
    other, idx2 = model.occlusion_sensitivity(x, target=2)
    assert idx2.tolist() == [2, 2] and not torch.equal(other, maps)
    ig = model.integrated_gradients(x, steps=8)
    assert ig["class_idx"].tolist() == [0, 0] and torch.isfinite(ig["token_maps"]).all()
    vols, cls = model.attribution_volumes(x, method="occlusion")
    assert vols.shape == (2, 32, 32, 32) and cls.tolist() == [0, 0]
    for call in (lambda: model.occlusion_sensitivity(x, score="prob"), lambda: model.integrated_gradients(x, score="prob"),
                 lambda: model.perturbation_curves(x, maps, score="prob"), lambda: model.shapley_values(x, score="prob")):
        with pytest.raises(ValueError, match="regression"):
            call()
    curves = model.perturbation_curves(x, maps, steps=4)
    assert all(torch.isfinite(v).all() for v in curves.values() if torch.is_tensor(v))
