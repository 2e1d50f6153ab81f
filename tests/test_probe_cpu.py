"""What tests/probe_ref.py (the restatement tests/test_probe_gpu.py holds the linear-probe kernels to) is worth, proven without a GPU: the
gradient against torch.autograd in float64, the regression fit against the closed-form ridge solution, the classification fit on a separable
set, the statistics against numpy; planted defects must fail; the inputs of the exact GPU case are exact.  Plus the header / binding side of
the new entry points and the host check under the host sanitizers."""
import ctypes
import math
import os
import subprocess

import numpy as np
import pytest
import torch

import probe_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def autograd_cost(case, H, C, mean, rstd, truth):
    """J = sum_h L_h + (l2_h / 2) |W_h|^2 written with torch in float64 -> (dW, db, loss [H])"""
    X = torch.from_numpy(case["X"]).double()
    if mean is not None:
        X = (X - torch.from_numpy(mean).double()) * torch.from_numpy(rstd).double()
    Wt = torch.from_numpy(case["W"]).double().requires_grad_(True)
    bt = torch.from_numpy(case["b"]).double().requires_grad_(True)
    logit = X @ Wt.T + bt
    losses = []
    for h in range(H):
        lg = logit[:, h * C:(h + 1) * C]
        if "labels" in truth:
            y = torch.from_numpy(truth["labels"]).long()
            ok = (y >= 0) & (y < C)
            cw = torch.from_numpy(truth["class_weight"]).double()
            nll = torch.nn.functional.cross_entropy(lg[ok], y[ok], weight=cw, reduction="sum")
            losses.append(nll / cw[y[ok]].sum())
        else:
            T = torch.from_numpy(truth["targets"]).double()
            seen = ~torch.isnan(T)
            per = [((lg[:, k] - T[:, k])[seen[:, k]] ** 2).sum() / seen[:, k].sum() for k in range(C) if seen[:, k].any()]
            losses.append(sum(per))
    l2 = torch.tensor(np.asarray(case["l2"], np.float32).astype(np.float64))
    J = sum(losses) + sum(0.5 * l2[h] * (Wt[h * C:(h + 1) * C] ** 2).sum() for h in range(H))
    J.backward()
    return Wt.grad.numpy(), bt.grad.numpy(), torch.stack(losses).detach().numpy()


@pytest.mark.parametrize("N,d,C,H", [(1, 4, 2, 1), (33, 72, 3, 5), (517, 72, 5, 3)], ids=lambda v: str(v))
def test_gradient_restatement_against_autograd_in_float64(N, d, C, H):
    for task in ("classification", "regression"):
        case = R.cls_case(N, d, C, H, seed=N + d) if task == "classification" else R.reg_case(N, d, C, H, seed=N + d)
        mean, rstd = R.stats_ref(case["X"])[:2] if N > 1 else (None, None)
        truth = dict(labels=case["labels"], class_weight=case["class_weight"]) if task == "classification" else dict(targets=case["targets"])
        got = R.grad_ref(case["X"], case["W"], case["b"], H, C, case["l2"], mean=mean, rstd=rstd, **truth)
        want = autograd_cost(case, H, C, mean, rstd, truth)
        assert all(R.rel(g, w) < 1e-12 for g, w in zip(got, want)), (task, [R.rel(g, w) for g, w in zip(got, want)])
        # the fp32 algorithm on the CPU sits far inside the gate the kernel is held to
        f32 = R.grad_ref(case["X"], case["W"], case["b"], H, C, case["l2"], mean=mean, rstd=rstd, dtype=np.float32, **truth)
        worst = max(R.rel(g, w) for g, w in zip(f32, got))
        print(f"fp32 restatement {task} {(N, d, C, H)}: {worst:.2e}")
        assert worst < R.LOSS_GATE / 4
        if task == "classification" and N > 1:
            assert (case["labels"] == -1).any() and (case["labels"] == C).any() and rstd[1] == 0


def test_statistics_restatement():
    X = R.features(517, 20, seed=1, const_col=3)
    mean, rstd, std, count = R.stats_ref(X)
    x64 = X.astype(np.float64)
    assert np.allclose(mean, x64.mean(0), rtol=1e-7) and np.allclose(std, x64.std(0), rtol=1e-6, atol=1e-12) and (count == 517).all()
    assert rstd[3] == 0 and std[3] == 0 and np.allclose(np.delete(rstd, 3), 1 / np.sqrt(np.delete(x64.var(0), 3) + 1e-12), rtol=1e-6)
    T = R.reg_case(300, 8, 3, 1, seed=2)["targets"]
    mean, rstd, std, count = R.stats_ref(T, skip_nan=True, eps=0.0)
    assert count[2] == 0 and mean[2] == 0 and rstd[2] == 0 and np.array_equal(count[:2], (~np.isnan(T[:, :2])).sum(0))
    assert np.allclose(mean[:2], np.nanmean(T[:, :2].astype(np.float64), 0), rtol=1e-7) and np.allclose(std[:2], np.nanstd(T[:, :2].astype(np.float64), 0), rtol=1e-6)
    labels = np.array([0, 1, -1, 2, 3, 1], np.int32)
    assert R.denom_ref(labels, 3)[0] == 4 and R.denom_ref(labels, 3, np.array([1, 0.5, 2], np.float32))[0] == 1 + 0.5 + 2 + 0.5


def test_the_exact_case_is_exact_in_fp32():
    for d in (4, 72, 768, 1024):
        case = R.int_case(d, seed=d)
        assert np.isnan(case["targets"]).any(1).sum() == 5 and len(case["X"]) == 517 and 517 - 5 == 512
        f64 = R.grad_ref(case["X"], case["W"], case["b"], R.INT_H, R.INT_K, case["l2"], targets=case["targets"])
        f32 = R.grad_ref(case["X"], case["W"], case["b"], R.INT_H, R.INT_K, case["l2"], targets=case["targets"], dtype=np.float32)
        assert all(np.array_equal(a.astype(np.float32), b) for a, b in zip(f64, f32))          # the fp32 algorithm rounds nowhere
        logit = R.logits_ref(case["X"], case["W"], case["b"])[0]
        assert np.abs(logit).max() <= d + 1 and (np.abs(logit).max() + 4) ** 2 < 2 ** 24


def test_regression_fit_reaches_the_ridge_solution():
    """N = 300, d = 72, a NaN target every 17th row, 500 steps at lr 0.01 (cosine) from zero: the float64 fit against the closed-form
    penalised optimum with unpenalised intercept, gated at 1e-6; 200 steps do not get there (so the gate is about the fit, not slack)."""
    N, d, l2 = 300, 72, [1e-3, 0.1]
    case = R.reg_case(N, d, 1, 2, seed=5)
    assert np.isnan(case["targets"][::17]).all() and np.isnan(case["targets"]).sum() == len(range(0, N, 17))
    mean, rstd = R.stats_ref(case["X"])[:2]
    tm, _, tsd, cnt = R.stats_ref(case["targets"], skip_nan=True, eps=0.0)
    Z = R.standardise(case["X"], mean, rstd, np.float64)
    t = ((case["targets"][:, 0] - tm[0]).astype(np.float32) / tsd[0]).astype(np.float64)
    kw = dict(targets=case["targets"], target_mean=tm, target_std=tsd, denom=cnt, mean=mean, rstd=rstd)
    W500, b500, hist = R.fit_ref(case["X"], 2, 1, l2, 500, **kw)
    W200, b200, _ = R.fit_ref(case["X"], 2, 1, l2, 200, **kw)
    Wdec, bdec, _ = R.fit_ref(case["X"], 2, 1, l2, 500, decoupled=True, **kw)
    W32, b32, _ = R.fit_ref(case["X"], 2, 1, l2, 500, dtype=np.float32, **kw)
    for h, lam in enumerate(l2):
        w, c = R.ridge_ref(Z, t, lam)
        want = np.append(w, c)
        e500, e200 = R.rel(np.append(W500[h], b500[h]), want), R.rel(np.append(W200[h], b200[h]), want)
        edec, e32 = R.rel(np.append(Wdec[h], bdec[h]), want), R.rel(np.append(W32[h], b32[h]), want)
        print(f"ridge l2={lam}: 500 steps {e500:.1e}, 200 steps {e200:.1e}, decoupled {edec:.1e}, fp32 restatement {e32:.1e}")
        assert e500 < 1e-6 < e200
        assert edec > 100 * e500                                      # planted defect: AdamW's decoupled decay does not land on the ridge optimum
        assert e32 < 1e-4
    assert hist[-1].max() < hist[0].min()
    # planted defect: a NaN target counted in the denominator moves the gradient
    good = R.grad_ref(case["X"], case["W"], case["b"], 2, 1, l2, targets=case["targets"], mean=mean, rstd=rstd)
    bad = R.grad_ref(case["X"], case["W"], case["b"], 2, 1, l2, targets=case["targets"], mean=mean, rstd=rstd, count_nan=True)
    assert R.rel(bad[0], good[0]) > 1e-3 and R.rel(bad[2], good[2]) > 1e-3


def test_classification_fit_separates_a_separable_set_and_planted_defects_fail():
    rng = np.random.default_rng(7)
    N, d, C, H = 300, 20, 3, 2
    centres = 4.0 * rng.standard_normal((C, d))
    labels = rng.integers(0, C, N).astype(np.int32)
    X = (centres[labels] + 0.3 * rng.standard_normal((N, d))).astype(np.float32)
    labels[::9] = -1
    mean, rstd = R.stats_ref(X)[:2]
    Wf, bf, hist = R.fit_ref(X, H, C, [1e-4, 1e-2], 200, labels=labels, mean=mean, rstd=rstd)
    assert (hist[-1] < 0.05 * hist[0]).all() and np.allclose(hist[0], math.log(C))             # from zero weights the loss starts at log C
    pred = R.logits_ref(X, Wf, bf, mean, rstd)[0].reshape(N, H, C).argmax(2)
    ok = labels >= 0
    assert (pred[ok] == labels[ok, None]).all()
    case = R.cls_case(300, 20, C, H, seed=9)
    kw = dict(labels=case["labels"], class_weight=case["class_weight"])
    good = R.grad_ref(case["X"], case["W"], case["b"], H, C, case["l2"], **kw)
    for defect in ("softmax_all", "count_unlabelled"):
        bad = R.grad_ref(case["X"], case["W"], case["b"], H, C, case["l2"], **kw, **{defect: True})
        assert R.rel(bad[0], good[0]) > 1e-3 and R.rel(bad[2], good[2]) > 1e-3, defect


def test_header_binding_and_wrapper_checks():
    from neurovit_amd import _cabi
    protos = _cabi.parse_header()
    for name in ("nv_probe_stats", "nv_probe_stats_workspace_bytes", "nv_probe_grad", "nv_probe_grad_workspace_bytes", "nv_probe_step", "nv_probe_predict"):
        assert name in protos, name
    assert protos["nv_probe_grad_workspace_bytes"][0] is ctypes.c_long and len(protos["nv_probe_grad"][1]) == 23
    src = open(_cabi.HEADER).read()
    for macro, value in (("NV_PROBE_CHUNK", _cabi.PROBE_CHUNK), ("NV_PROBE_MAX_M", _cabi.PROBE_MAX_M), ("NV_PROBE_MAX_D", _cabi.PROBE_MAX_D)):
        assert f"#define {macro} {value}" in src
    assert R.CHUNK == _cabi.PROBE_CHUNK and "#define NV_ABI_VERSION 8" in src                   # new symbols only: the revision stays
    assert ctypes.sizeof(_cabi.ProbeHeads) == 12 + 2 * 4 * _cabi.PROBE_MAX_M
    from neurovit_amd import ops
    from neurovit_amd.optim import LRSchedule
    with pytest.raises(ValueError, match="H \\* C"):
        ops.probe_heads(3, 11)
    with pytest.raises(ValueError, match="l2 must be >= 0"):
        ops.probe_heads(2, 3, l2=[0.1, -0.1])
    hd = ops.probe_heads(2, 3, l2=[0.5, 0.25], step=0.125)
    assert (hd.H, hd.C, hd.l2[1], hd.step[0], hd.step[1], hd.l2[2]) == (2, 3, 0.25, 0.125, 0.125, 0.0)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.probe_stats(torch.zeros(4, 8))
    sched = LRSchedule(0.01, 500, kind="cosine")
    assert all(sched.lr_at(k) == R.lr_at(k, 500, 0.01) for k in (1, 2, 250, 499, 500)) and sched.lr_at(500) == 0.0
    sizes, bc2s = ops.probe_adam_constants(3, [0.01, 0.02])
    assert sizes == [0.01 / (1 - 0.9 ** 3), 0.02 / (1 - 0.9 ** 3)] and bc2s == math.sqrt(1 - 0.999 ** 3)


def test_trainer_config_keys():
    from neurovit_amd.trainer import Trainer
    assert Trainer.linear_from_config({}) is None and Trainer.linear_from_config({"PRETRAIN_LINEAR_EVERY": 0}) is None
    got = Trainer.linear_from_config({"PRETRAIN_LINEAR_EVERY": 2})
    assert got == dict(every=2, steps=500, lr=0.01, l2=(1e-4, 1e-3, 1e-2, 1e-1), pool="patch_mean")
    got = Trainer.linear_from_config({"PRETRAIN_LINEAR_EVERY": 1, "PRETRAIN_LINEAR_L2": 0.5, "PRETRAIN_LINEAR_STEPS": 30, "PRETRAIN_LINEAR_LR": 0.1, "PRETRAIN_LINEAR_POOL": "cls"})
    assert got == dict(every=1, steps=30, lr=0.1, l2=(0.5,), pool="cls")
    for bad in ({"PRETRAIN_LINEAR_EVERY": -1}, {"PRETRAIN_LINEAR_EVERY": 1, "PRETRAIN_LINEAR_L2": [-1.0]}, {"PRETRAIN_LINEAR_EVERY": 1, "PRETRAIN_LINEAR_STEPS": 0},
                {"PRETRAIN_LINEAR_EVERY": 1, "PRETRAIN_LINEAR_LR": 0.0}, {"PRETRAIN_LINEAR_EVERY": 1, "PRETRAIN_LINEAR_POOL": "max"},
                {"PRETRAIN_LINEAR_EVERY": 1, "PRETRAIN_LINEAR_L2": [0.1, 0.1]}):
        with pytest.raises(ValueError, match="PRETRAIN_LINEAR"):
            Trainer.linear_from_config(bad)


def test_host_check_program_is_clean_under_the_host_sanitizers():
    """tools/probe_host_check.cpp: the host side of the probe's entry points (argument checks, workspace sizing) in a stand-alone program built
    with -Xarch_host -fsanitize=address,undefined; it makes bad-argument calls only, so nothing is launched.  Nothing loaded into Python is sanitised."""
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc on this machine")
    out = subprocess.run(["make", "-C", os.path.join(ROOT, "neurovit_amd", "csrc"), "probe-host-check"], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    assert "probe_host_check: ok" in out.stdout and "runtime error" not in out.stdout + out.stderr and "AddressSanitizer" not in out.stdout + out.stderr
