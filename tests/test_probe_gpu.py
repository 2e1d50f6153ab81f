"""The linear probe on the MI355X: nv_probe_stats, nv_probe_grad, nv_probe_step and nv_probe_predict held to the float64 restatement
(tests/probe_ref.py; what it is worth is proven in tests/test_probe_cpu.py), then features.LinearProbe / linear_evaluate and the Trainer's
linear validation.

Measured on one MI355X (gfx950): the integer regression case bit-equal at max_blocks 1, 3, automatic and on a repeat for d = 4, 72, 768, 1024;
random inputs against float64 (gate 1e-5): dW at most 6.1e-7, db 5.7e-7, loss 1.1e-7 over the five geometries and both tasks; fits against the
float64 fit: weights at most 7.8e-7, query logits 4.7e-7 (the reference's own fp32 fit: 7.4e-7 ... 1.2e-6, so gates of 1.2e-5 ... 1.9e-5); the
500-step regression fit 6.8e-7 (l2 1e-3) and 6.2e-7 (l2 0.1) from the closed-form ridge solution; the Adam step bit-equal to the torch fp32
expressions; prediction logits at 0.006 of the first-order fp32 bound."""
import numpy as np
import pytest
import torch

import knn_ref as KR
import ld_windows as L
import probe_ref as R
import weights as W
from conftest import report

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ops():
    from neurovit_amd._cabi import require_gpu
    require_gpu()
    from neurovit_amd import ops
    return ops


def dev(t, dtype=None):
    if t is None:
        return None
    t = torch.from_numpy(np.ascontiguousarray(t)) if isinstance(t, np.ndarray) else t
    return (t if dtype is None else t.to(dtype)).cuda()


def host(t):
    return t.detach().cpu().numpy()


def bits_equal(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def run_grad(ops, case, H, C, *, Xd=None, stats=None, max_blocks=0, denom=None, **over):
    """ops.probe_grad on a case dict -> numpy (dW, db, loss); the denominator comes from ops.probe_stats as in a fit"""
    c = dict(case, **over)
    Xd = dev(c["X"]) if Xd is None else Xd
    heads = ops.probe_heads(H, C, c["l2"])
    kw = dict(mean=dev(stats[0]), rstd=dev(stats[1])) if stats is not None else {}
    if c.get("labels") is not None:
        lab, cw = dev(c["labels"]), dev(c.get("class_weight"))
        denom = ops.probe_stats(labels=lab, num_classes=C, class_weight=cw)["denom"] if denom is None else denom
        out = ops.probe_grad(Xd, dev(c["W"]), dev(c["b"]), heads, denom, labels=lab, class_weight=cw, max_blocks=max_blocks, **kw)
    else:
        T = dev(c["targets"])
        denom = ops.probe_stats(T, skip_nan=True)["count"] if denom is None else denom
        out = ops.probe_grad(Xd, dev(c["W"]), dev(c["b"]), heads, denom, targets=T, target_mean=dev(c.get("target_mean")), target_std=dev(c.get("target_std")),
                             max_blocks=max_blocks, **kw)
    return tuple(host(t) for t in out)


# ------------------------------------------------------------------ 1. the exact case
@pytest.mark.parametrize("d", [4, 72, 768, 1024])
def test_integer_regression_gradient_is_bit_equal_at_every_grid(ops, d):
    """Integer features, weights and targets, D = 512 observed rows of 517 (the last chunk ragged), no standardisation: every product and sum
    is exact, so dW, db and the loss equal the float64 reference word for word, at 1, 3 and one workgroup per chunk and on a second run;
    the features sit in a padded leading dimension whose guard cells are NaN."""
    case = R.int_case(d, seed=d)
    H, K = R.INT_H, R.INT_K
    want = tuple(t.astype(np.float32) for t in R.grad_ref(case["X"], case["W"], case["b"], H, K, case["l2"], targets=case["targets"]))
    Xd = L.into_poisoned(torch.from_numpy(case["X"]), 4)
    assert Xd.stride(0) == d + 4
    count = ops.probe_stats(dev(case["targets"]), skip_nan=True)["count"]
    assert host(count).tolist() == [512.0, 512.0]
    for max_blocks in (1, 3, 0, 1):
        got = run_grad(ops, case, H, K, Xd=Xd, max_blocks=max_blocks, denom=count)
        for name, g, w in zip(("dW", "db", "loss"), got, want):
            assert bits_equal(g, w), (d, max_blocks, name, np.abs(g - w).max())


# ------------------------------------------------------------------ 2. random inputs
GRAD_CASES = [(1, 4, 2, 1), (33, 72, 3, 5), (517, 72, 5, 3), (300, 768, 2, 8), (517, 1024, 5, 6)]


@pytest.mark.parametrize("N,d,C,H", GRAD_CASES, ids=lambda v: str(v))
def test_gradient_and_loss_within_the_loss_gate_and_grid_independent(ops, N, d, C, H):
    """Loss and gradient against float64 at 1e-5 (relative, max-norm), classification (labels -1 and C, class weights, a zero-variance column,
    standardised features) and regression (NaN targets; for C >= 3 a column that is missing everywhere: gradient l2 W exactly); bits identical
    at max_blocks 1, 3, automatic and on a repeat; everything unlabelled: loss 0 and gradient l2 W exactly.
    Measured on MI355X, worst of (dW, db, loss) per geometry, classification / regression: (1, 4, 2, 1) 1.6e-7 / 5.8e-8; (33, 72, 3, 5) 1.6e-7 /
    1.9e-7; (517, 72, 5, 3) 2.2e-7 / 3.6e-7; (300, 768, 2, 8) 5.7e-7 / 5.2e-7; (517, 1024, 5, 6) 5.1e-7 / 6.1e-7 (the CPU fp32 restatement:
    1.6e-7 ... 3.2e-7 on the first three)."""
    worst = 0.0
    for task in ("classification", "regression"):
        case = R.cls_case(N, d, C, H, seed=N + d) if task == "classification" else R.reg_case(N, d, C, H, seed=N + d)
        stats = R.stats_ref(case["X"])[:2] if N > 1 else None
        truth = dict(labels=case["labels"], class_weight=case["class_weight"]) if task == "classification" else dict(targets=case["targets"])
        mean, rstd = stats if stats is not None else (None, None)
        want = R.grad_ref(case["X"], case["W"], case["b"], H, C, case["l2"], mean=mean, rstd=rstd, **truth)
        first = None
        for max_blocks in (1, 3, 0, 1):
            got = run_grad(ops, case, H, C, stats=stats, max_blocks=max_blocks)
            first = got if first is None else first
            assert all(bits_equal(g, f) for g, f in zip(got, first)), (task, max_blocks)
        errs = [R.rel(g, w) for g, w in zip(first, want)]
        print(f"probe_grad {task} N={N} d={d} C={C} H={H}: rel dW {errs[0]:.2e} db {errs[1]:.2e} loss {errs[2]:.2e}")
        report(f"probe_grad {task} N={N} d={d} C={C} H={H} vs float64: dW {errs[0]:.2e} db {errs[1]:.2e} loss {errs[2]:.2e} (gate {R.LOSS_GATE:.0e})")
        worst = max(worst, *errs)
        # fp32(0 + l2 W), the product in double: what is left when the data term is the zero of "nothing observed" (a -0 product becomes +0)
        l2w = (0.0 + np.repeat(np.asarray(case["l2"], np.float32).astype(np.float64), C)[:, None] * case["W"].astype(np.float64)).astype(np.float32)
        if task == "regression" and C >= 3:                     # the dead column of every head
            dead = np.arange(C - 1, H * C, C)
            assert bits_equal(first[0][dead], l2w[dead]) and (first[1][dead] == 0).all()
        if task == "classification":                            # nothing labelled at all
            none = run_grad(ops, case, H, C, stats=stats, labels=np.full(N, -1, np.int32))
            assert bits_equal(none[0], l2w) and (none[1] == 0).all() and (none[2] == 0).all()
    assert worst < R.LOSS_GATE


# ------------------------------------------------------------------ 3. statistics
def test_statistics_bit_equal_to_float64_rounded_once(ops):
    case = R.cls_case(517, 72, 5, 3, seed=3)
    mean, rstd, std, count = R.stats_ref(case["X"])
    got = ops.probe_stats(L.into_poisoned(torch.from_numpy(case["X"]), 4))
    assert bits_equal(host(got["mean"]), mean) and bits_equal(host(got["rstd"]), rstd) and bits_equal(host(got["std"]), std)
    assert rstd[1] == 0 and host(got["rstd"])[1] == 0 and (rstd[[0, 2, 3]] > 0).all()           # the constant column drops out
    assert (host(got["count"]) == 517).all()
    T = R.reg_case(517, 72, 3, 1, seed=4)["targets"]
    mean, rstd, std, count = R.stats_ref(T, skip_nan=True, eps=0.0)
    got = ops.probe_stats(dev(T), skip_nan=True, eps=0.0)
    assert np.array_equal(host(got["count"]), count) and count[2] == 0 and 0 < count[0] < 517
    assert bits_equal(host(got["mean"]), mean) and bits_equal(host(got["rstd"]), rstd) and bits_equal(host(got["std"]), std)
    assert mean[2] == 0 and rstd[2] == 0                                                      # nothing observed
    for cw in (None, case["class_weight"]):
        d = ops.probe_stats(labels=dev(case["labels"]), num_classes=5, class_weight=dev(cw))["denom"]
        assert np.array_equal(host(d), R.denom_ref(case["labels"], 5, cw))


# ------------------------------------------------------------------ 4. the Adam step
def test_step_is_bit_equal_to_the_torch_fp32_expressions(ops):
    """three consecutive steps over two heads with their own lr and l2: nv_probe_step against the same expressions on fp32 CPU tensors, every
    operation a torch op of its own (no fused multiply-add anywhere), the square root IEEE.
    Measured on MI355X: W, b and the four moments word for word after each of the three steps.  (What it caught: the toolchain's rounded
    intrinsics are inline functions compiled under the default contraction mode, so p - step * q had become one fused multiply-add.)"""
    N, d, C, H = 300, 72, 3, 2
    case = R.cls_case(N, d, C, H, seed=8)
    lrs, l2 = [0.01, 0.003], [1e-3, 0.1]
    Xd, lab = dev(case["X"]), dev(case["labels"])
    denom = ops.probe_stats(labels=lab, num_classes=C)["denom"]
    Wd, bd = dev(case["W"]), dev(case["b"])
    state = [torch.zeros_like(Wd), torch.zeros_like(Wd), torch.zeros_like(bd), torch.zeros_like(bd)]
    cW, cb = torch.from_numpy(case["W"]).clone(), torch.from_numpy(case["b"]).clone()
    cstate = [torch.zeros_like(cW), torch.zeros_like(cW), torch.zeros_like(cb), torch.zeros_like(cb)]
    f = lambda x: torch.tensor(np.float32(x))
    b1, b2 = R.BETAS
    for k in (1, 2, 3):
        sizes, bc2s = ops.probe_adam_constants(k, lrs, R.BETAS)
        heads = ops.probe_heads(H, C, l2, sizes)
        dW, db, _ = ops.probe_grad(Xd, Wd, bd, heads, denom, labels=lab)
        ops.probe_step(Wd, bd, dW, db, *state, heads, k, R.BETAS, R.ADAM_EPS)
        size_rows = torch.from_numpy(np.repeat(np.asarray(sizes, np.float32), C))
        for p, g, m, v, size in ((cW, dW.cpu(), cstate[0], cstate[1], size_rows[:, None]), (cb, db.cpu(), cstate[2], cstate[3], size_rows)):
            m.copy_(f(b1) * m + f(1.0 - b1) * g)
            v.copy_(f(b2) * v + (f(1.0 - b2) * g) * g)
            # the IEEE square root, as the kernel's: sqrt in double rounded to fp32 is the correctly rounded fp32 root (53 >= 2 * 24 + 2 bits),
            # which torch's vectorised fp32 sqrt on the CPU is not on every build (about 0.7 % of random inputs come out one ulp off)
            den = v.double().sqrt().float() / f(bc2s) + f(R.ADAM_EPS)
            p.copy_(p - size * (m / den))
        for got, want in zip([Wd, bd] + state, [cW, cb, cstate[0], cstate[1], cstate[2], cstate[3]]):
            assert bits_equal(host(got), want.numpy()), k
    assert not np.array_equal(host(Wd), case["W"])


# ------------------------------------------------------------------ 5. the fit, end to end
def _fit_refs(case, H, C, steps, truth, stats, queries):
    out = {}
    for dtype in (np.float64, np.float32):
        Wf, bf, hist = R.fit_ref(case["X"], H, C, case["l2"], steps, dtype=dtype, mean=stats[0], rstd=stats[1], **truth)
        out[dtype] = (Wf, bf, hist, R.logits_ref(queries, Wf, bf, stats[0], stats[1], dtype)[0])
    own = max(R.rel(out[np.float32][0], out[np.float64][0]), R.rel(out[np.float32][3], out[np.float64][3]))
    return out[np.float64], max(R.FIT_FACTOR * own, R.FIT_FLOOR), own


@pytest.mark.parametrize("steps", [30, 200])
@pytest.mark.parametrize("N,d,C", [(300, 72, 3), (517, 200, 2)])
def test_fit_tracks_the_float64_fit(ops, N, d, C, steps):
    """LinearProbe.fit against probe_ref's float64 fit: weights and query logits (max-norm, relative) within 16 x the deviation of the
    reference's OWN fp32 fit from its float64 fit on the same inputs (not below 1e-6) - the gate comes from the reference, never from the
    kernel.  Measured on MI355X (weights / logits; the reference's own fp32 fit; the gate): (300, 72, 3) 30 steps 7.8e-7 / 2.7e-7; 8.6e-7; 1.4e-5 - 200 steps
    7.4e-7 / 4.7e-7; 7.4e-7; 1.2e-5 - (517, 200, 2) 30 steps 5.9e-7 / 3.9e-7; 7.5e-7; 1.2e-5 - 200 steps 7.5e-7 / 4.7e-7; 1.2e-6; 1.9e-5.  Every arg-max of the query logits agrees."""
    from neurovit_amd import FeatureBank, LinearProbe
    H = 2
    case = R.cls_case(N, d, C, H, seed=N + d + 1)
    stats = R.stats_ref(case["X"])[:2]
    Q = R.features(40, d, seed=N + d + 9)
    truth = dict(labels=case["labels"], class_weight=case["class_weight"], denom=R.denom_ref(case["labels"], C, case["class_weight"]))
    (W64, b64, hist64, logit64), gate, own = _fit_refs(case, H, C, steps, truth, stats, Q)
    bank = FeatureBank.from_features(dev(case["X"]), labels=case["labels"])
    probe = LinearProbe(d, num_classes=C, l2=case["l2"]).fit(bank, steps=steps, lr=0.01, class_weight=case["class_weight"])
    got_logits, _ = probe.logits(dev(Q))
    eW, el, eh = R.rel(host(probe._W), W64), R.rel(host(got_logits), logit64), R.rel(host(probe.history), hist64)
    print(f"probe fit N={N} d={d} C={C} steps={steps}: weights {eW:.2e} logits {el:.2e} history {eh:.2e}; reference fp32 fit {own:.2e}, gate {gate:.2e}")
    report(f"probe fit N={N} d={d} C={C} steps={steps} vs float64 fit: weights {eW:.2e} logits {el:.2e} (reference's own fp32 fit {own:.2e}, gate {gate:.2e})")
    assert probe.history.shape == (steps, H) and probe.history.is_cuda
    assert eW < gate and el < gate
    assert np.array_equal(host(got_logits).reshape(40, H, C).argmax(2), logit64.reshape(40, H, C).argmax(2))
    assert hist64[-1].max() < hist64[0].min()                                                # the loss went down


def test_regression_fit_lands_on_the_ridge_solution(ops):
    """500 steps at lr 0.01, cosine: the fitted weights of both heads against the closed-form ridge solution on the standardised features and
    targets, within the gate of the fit test (16 x the reference's own fp32 deviation, not below 1e-6).  Measured on MI355X: 6.8e-7 (l2 1e-3) and
    6.2e-7 (l2 0.1) from the ridge solution; the float64 fit 1.4e-9 and 1.3e-9; the reference's own fp32 deviation 6.8e-7, gate 1.1e-5."""
    from neurovit_amd import FeatureBank, LinearProbe
    N, d, steps, l2 = 300, 72, 500, [1e-3, 0.1]
    case = R.reg_case(N, d, 1, 2, seed=5)
    stats = R.stats_ref(case["X"])[:2]
    tm, _, tsd, cnt = R.stats_ref(case["targets"], skip_nan=True, eps=0.0)
    truth = dict(targets=case["targets"], target_mean=tm, target_std=tsd, denom=cnt)
    Z = R.standardise(case["X"], stats[0], stats[1], np.float64)
    t = ((case["targets"][:, 0] - tm[0]).astype(np.float32) / tsd[0]).astype(np.float64)
    fits = {dt: R.fit_ref(case["X"], 2, 1, l2, steps, dtype=dt, mean=stats[0], rstd=stats[1], **truth) for dt in (np.float64, np.float32)}
    own = R.rel(fits[np.float32][0], fits[np.float64][0])
    gate = max(R.FIT_FACTOR * own, R.FIT_FLOOR)
    bank = FeatureBank.from_features(dev(case["X"]), targets=dev(case["targets"]))
    probe = LinearProbe(d, num_targets=1, l2=l2).fit(bank, steps=steps, lr=0.01)
    assert bits_equal(host(probe.target_mean), tm) and bits_equal(host(probe.target_std), tsd)
    for h, lam in enumerate(l2):
        w, c = R.ridge_ref(Z, t, lam)
        e64, e = R.rel(np.append(fits[np.float64][0][h], fits[np.float64][1][h]), np.append(w, c)), R.rel(np.append(host(probe._W)[h], host(probe._b)[h]), np.append(w, c))
        print(f"probe ridge l2={lam}: kernel fit {e:.2e}, float64 fit {e64:.2e}, reference's own fp32 deviation {own:.2e}, gate {gate:.2e}")
        report(f"probe 500-step regression fit vs closed-form ridge, l2={lam}: {e:.2e} (float64 fit {e64:.2e}, gate {gate:.2e})")
        assert e64 < 1e-6 and e < gate
    raw = probe.predict(dev(case["X"]))
    assert raw.shape == (2, N, 1) and 40 < raw.mean().item() < 60                              # the raw scale


# ------------------------------------------------------------------ 6. predict and evaluate
def test_predict_within_the_dot_product_bound_and_probabilities_within_the_gate(ops):
    d, C, H, Nq = 200, 5, 6, 67
    case = R.cls_case(Nq, d, C, H, seed=21)
    Q, Wt, b = case["X"], case["W"], case["b"]
    got, _ = ops.probe_predict(L.into_poisoned(torch.from_numpy(Q), 4), dev(Wt), dev(b), H, C)
    want = R.logits_ref(Q, Wt, b)[0]
    # d products and adds, the four-way meeting of the waves' partial sums and the bias: (d + 2) roundings to first order
    bound = (d + 2) * 2.0 ** -24 * (np.abs(Q.astype(np.float64)) @ np.abs(Wt.astype(np.float64)).T + np.abs(b.astype(np.float64)))
    err = np.abs(host(got).astype(np.float64) - want)
    print(f"probe_predict d={d}: worst |logit - f64| / bound = {(err / bound).max():.3f}")
    report(f"probe_predict d={d} M={H * C}: worst |logit - f64| / ((d + 2) 2^-24 (sum|q||w| + |b|)) = {(err / bound).max():.3f}")
    assert (err <= bound).all()
    mean, rstd = R.stats_ref(Q)[:2]
    logit, probs = ops.probe_predict(dev(Q), dev(Wt), dev(b), H, C, mean=dev(mean), rstd=dev(rstd), want_probs=True)
    want_p = R.softmax_heads(R.logits_ref(Q, Wt, b, mean, rstd)[0], H, C)
    ep = np.abs(host(probs).reshape(Nq, H, C) - want_p).max()
    report(f"probe_predict probabilities vs float64: {ep:.2e} (gate {KR.SOFTMAX_GATE:.0e})")
    assert ep < KR.SOFTMAX_GATE
    assert np.allclose(host(probs).reshape(Nq, H, C).sum(2), 1.0, atol=1e-6)


def test_evaluate_per_volume_and_per_subject_and_two_passes(ops):
    from neurovit_amd import FeatureBank, LinearProbe, linear_evaluate
    N, d, C, H = 300, 72, 5, 8                                 # 40 columns: two passes (6 heads, then 2)
    case = R.cls_case(N, d, C, H, seed=31)
    bank = FeatureBank.from_features(dev(case["X"]), labels=case["labels"])
    probe = LinearProbe(d, num_classes=C, l2=case["l2"]).fit(bank, steps=30)
    halves = [LinearProbe(d, num_classes=C, l2=case["l2"][lo:lo + 4]).fit(bank, steps=30) for lo in (0, 4)]
    assert bits_equal(host(probe._W), np.concatenate([host(p._W) for p in halves]))
    assert bits_equal(host(probe._b), np.concatenate([host(p._b) for p in halves]))
    assert bits_equal(host(probe.history), np.concatenate([host(p.history) for p in halves], axis=1))
    # 20 subjects of three volumes: the queries are noisy copies of bank rows
    rng = np.random.default_rng(32)
    rows = np.repeat(rng.permutation(N)[:20], 3)
    Q = (case["X"][rows] + 0.02 * rng.standard_normal((60, d)).astype(np.float32) / np.sqrt(d)).astype(np.float32)
    groups = np.repeat(np.arange(20), 3)
    y = np.where((case["labels"][rows] >= 0) & (case["labels"][rows] < C), case["labels"][rows], 0)
    out = linear_evaluate(probe, dev(Q), labels=y, query_groups=groups)
    pred, probs = probe.predict(dev(Q))
    assert pred.shape == (H, 60) and probs.shape == (H, 60, C) and pred.dtype == torch.int32
    p1, pr1 = probe.predict(dev(Q), head=3)
    assert torch.equal(p1, pred[3]) and torch.equal(pr1, probs[3])
    mean, rstd = host(probe.mean), host(probe.rstd)
    want_p = R.softmax_heads(R.logits_ref(Q, host(probe._W), host(probe._b), mean, rstd)[0], H, C)
    top = np.sort(want_p, axis=2)
    assert (top[:, :, -1] - top[:, :, -2]).min() > 2 * KR.SOFTMAX_GATE                        # no arg-max hangs on the last digits
    acc, sacc = R.evaluate_ref(want_p, y, groups)
    assert list(out["acc"]) == list(probe.l2) and list(out["subject_acc"]) == list(probe.l2)
    assert np.allclose([out["acc"][k] for k in probe.l2], acc, atol=1e-6) and np.allclose([out["subject_acc"][k] for k in probe.l2], sacc, atol=1e-6)
    # state_dict round trip
    other = LinearProbe(d, num_classes=C, l2=[0.0] * H).load_state_dict(probe.state_dict())
    assert torch.equal(other.predict(dev(Q))[1], probs) and other.l2 == probe.l2
    # regression: MAE per head, per volume and per subject
    reg = R.reg_case(N, d, 2, 2, seed=33, dead_column=False)
    rbank = FeatureBank.from_features(dev(reg["X"]), targets=dev(reg["targets"]))
    rp = LinearProbe(d, num_targets=2, l2=[1e-3, 0.1]).fit(rbank, steps=30)
    ro = linear_evaluate(rp, dev(reg["X"][rows]), targets=dev(reg["targets"][rows]), query_groups=groups)
    raw = host(rp.predict(dev(reg["X"][rows])))
    T = reg["targets"][rows].astype(np.float64)
    for h, lam in enumerate(rp.l2):
        want_mae = [np.nanmean(np.abs(raw[h][:, k] - T[:, k])) for k in range(2)]
        assert np.allclose(ro["mae"][lam], want_mae, rtol=1e-5) and len(ro["subject_mae"][lam]) == 2


def test_refusals_raise_what_the_docs_say(ops):
    from neurovit_amd import FeatureBank, LinearProbe
    X = torch.zeros(8, 8, device="cuda")
    for kw, msg in ((dict(dim=6, num_classes=2), "multiple of 4"), (dict(dim=1028, num_classes=2), "multiple of 4"), (dict(dim=8, num_classes=33), "C = 33"),
                    (dict(dim=8, num_classes=2, l2=[-1.0]), "l2"), (dict(dim=8), "one of the two"), (dict(dim=8, num_classes=2, num_targets=1), "one of the two")):
        with pytest.raises(ValueError, match=msg):
            LinearProbe(**kw)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        LinearProbe(8, num_classes=2, device="cpu")
    probe = LinearProbe(8, num_classes=2)
    with pytest.raises(ValueError, match="empty"):
        probe.fit(FeatureBank(8, 4))
    with pytest.raises(ValueError, match="labels"):
        probe.fit(FeatureBank.from_features(X))
    labelled = FeatureBank.from_features(X, labels=torch.zeros(8, dtype=torch.int32))
    with pytest.raises(ValueError, match="steps"):
        probe.fit(labelled, steps=0)
    with pytest.raises(ValueError, match="built for classification"):
        probe.fit(labelled, task="regression")
    with pytest.raises(ValueError, match="targets"):
        LinearProbe(8, num_targets=1).fit(labelled)
    with pytest.raises(ValueError, match="class_weight"):
        LinearProbe(8, num_targets=1).fit(FeatureBank.from_features(X, targets=torch.zeros(8, 1)), class_weight=[1.0])
    with pytest.raises(RuntimeError, match="nv_probe_grad"):
        from neurovit_amd._cabi import ProbeHeads
        bad = ProbeHeads(4, 1, 2)                                # a wrong struct_size reaches the C-ABI's own check
        ops.probe_grad(X, torch.zeros(2, 8, device="cuda"), torch.zeros(2, device="cuda"), bad, torch.ones(1, dtype=torch.float64, device="cuda"),
                       labels=torch.zeros(8, dtype=torch.int32, device="cuda"))


# ------------------------------------------------------------------ 7. the Trainer
SIZE = dict(TRAINING_VIT_DIM=64, TRAINING_VIT_DEPTH=2, TRAINING_VIT_HEADS=1, TRAINING_VIT_MLP_DIM=128)


def test_trainer_logs_the_linear_validation_only_when_asked_and_extracts_once(tmp_path, monkeypatch):
    import neurovit_amd.NeuroEncoder as ne
    from neurovit_amd.trainer import Trainer
    monkeypatch.chdir(tmp_path)
    vols = torch.cat([(W.make_volume((3, 12, 12, 12), 83 + i) * 1.5) for i in range(2)])
    names = torch.tensor([0, 0, 1, 1, 2, 2])
    labels = torch.tensor([0, 1, 0, 1, 0, 1])
    ds = torch.utils.data.TensorDataset(names, torch.zeros(6, 1), vols, labels)
    base = dict(W.neuro_config(12, 3, DEVICE="cuda:0", **SIZE), GLOBAL_OUTPUT_DIR=str(tmp_path / "out"), TRAINING_EPOCHS=1, TRAINING_BATCH_SIZE=3,
                TRAINING_NUM_WORKERS=0, TRAINING_OBJECTIVE="mim", PRETRAIN_MASK_RATIO=0.5, TRAINING_LEARNING_RATE=1e-3)

    def logged(cfg):
        torch.manual_seed(84)
        trainer = Trainer(cfg, ne.NeuroEncoder(cfg), ds, ds)
        seen, calls = [], []
        trainer._log = seen.append
        extract = trainer._knn_features
        trainer._knn_features = lambda *a, **k: (calls.append(1), extract(*a, **k))[1]
        trainer.train(0)
        trainer.validate(0)
        return trainer, seen, len(calls)

    plain_trainer, plain, n_plain = logged(base)
    assert plain_trainer.linear is None and n_plain == 0
    assert all(set(p) <= {"epoch", "batch", "recon_loss", "learning_rate", "duration", "val_recon_loss"} for p in plain)       # what it logged before
    lin = dict(PRETRAIN_LINEAR_EVERY=1, PRETRAIN_LINEAR_STEPS=20, PRETRAIN_LINEAR_L2=[1e-3, 0.1])
    trainer, with_lin, n_lin = logged(dict(base, **lin))
    drop_time = lambda ps: [{k: v for k, v in p.items() if k != "duration"} for p in ps]
    extra = [p for p in with_lin if "val_linear_acc" in p]
    assert drop_time([p for p in with_lin if "val_linear_acc" not in p]) == drop_time(plain)                                # the same training, the same records
    assert len(extra) == 1 and set(extra[0]) == {"epoch", "val_linear_acc", "val_linear_subject_acc", "val_linear_acc_l20.1", "val_linear_subject_acc_l20.1"}
    assert all(0.0 <= extra[0][k] <= 1.0 for k in extra[0] if k != "epoch") and n_lin == 2                                  # one extraction per set
    trainer.model.train()
    again = trainer.linear_validate()
    assert trainer.model.training and {k: v for k, v in extra[0].items() if k != "epoch"} == again                        # reproducible: the same bits
    assert trainer.linear_probe.history.shape == (20, 2)
    # both probes in one epoch, the same pooling: still one extraction per set; another pooling: two
    _, both, n_both = logged(dict(base, PRETRAIN_KNN_EVERY=1, PRETRAIN_KNN_K=1, **lin))
    assert n_both == 2 and any("val_knn_acc" in p for p in both) and [p for p in both if "val_linear_acc" in p] == extra
    _, _, n_two = logged(dict(base, PRETRAIN_KNN_EVERY=1, PRETRAIN_KNN_K=1, PRETRAIN_LINEAR_POOL="mean", **lin))
    assert n_two == 4
