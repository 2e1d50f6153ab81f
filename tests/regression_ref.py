"""Float64 numpy restatement of the regression objective (include/neurovit_hip.h, nv_reg_opts): the loss, its gradient with respect to the
head's outputs, and the validation metrics - and the builders of the inputs that tests/test_regression_cpu.py proves things about and
tests/test_regression_gpu.py holds the kernels to."""
import itertools

import numpy as np
import torch

KINDS = ("mse", "l1", "huber")
DELTA = 0.75                      # huber's threshold in the tests
MEAN, STD = 70.0, 8.0             # an age-like raw scale
MARGIN = 1e-3                     # no valid residual this close to 0 or to the huber threshold: the gradient's jumps stay away from rounding
SHAPES = [(B, K) for B in (1, 3, 257) for K in (1, 3, 300)]
FP32_GATE = 1e-5                  # tests/test_mix_gpu.py's gate for the same head with the cross-entropy


def f32_bits(v):
    return int(np.float32(v).view(np.int32))


def mix_row(partner, mode=0, lam=1.0):
    b = f32_bits(lam)
    return [partner, mode, b, b, 1, 0, 0, 0, 0, 0, 0, 0]


def partner_of(b, B):
    return b if b % 5 == 3 else B - 1 - b          # some rows pair with themselves (and the middle row of an odd batch)


def mix_table(B):
    lam = [0.0, 0.3, 1.0]
    return np.array([mix_row(partner_of(b, B), 1, lam[b % 3]) for b in range(B)], dtype=np.int32)


def head_inputs(B, K, seed):
    """the head's inputs, built like loss_inputs of tests/test_mix_gpu.py: x [B, 2, d], gamma, beta, W [K, d], bias (torch, fp32)"""
    g = torch.Generator().manual_seed(seed)
    d = 8 if K <= 8 else 304
    x = torch.randn(B, 2, d, generator=g)
    gamma, beta = 1 + 0.1 * torch.randn(d, generator=g), 0.1 * torch.randn(d, generator=g)
    Wt, bias = torch.randn(K, d, generator=g) / d ** 0.5 * 3, torch.randn(K, generator=g)
    return x, gamma, beta, Wt, bias


def head_logits_ref(x, gamma, beta, Wt, bias, eps=1e-5):
    """float64 LayerNorm of the cls rows and the Linear behind it: what the head kernels compute in fp32"""
    r = x[:, 0, :].double().numpy()
    mu = r.mean(axis=1, keepdims=True)
    var = ((r - mu) ** 2).mean(axis=1, keepdims=True)
    xh = (r - mu) / np.sqrt(var + eps) * gamma.double().numpy() + beta.double().numpy()
    return xh @ Wt.double().numpy().T + bias.double().numpy()


def weights_of(K, seed):
    """{"none": None, "given": w, "zero": w with one zero entry} - the zero variant only where another target keeps D > 0"""
    w = (np.random.default_rng(seed).random(K) + 0.25).astype(np.float32)
    out = {"none": None, "given": w}
    if K > 1:
        w0 = w.copy()
        w0[1] = 0.0
        out["zero"] = w0
    return out


def standardised(y, mean, std):
    y = np.asarray(y, dtype=np.float32).astype(np.float64)
    return (y - (0.0 if mean is None else np.asarray(mean, dtype=np.float64))) / (1.0 if std is None else np.asarray(std, dtype=np.float64))


def mixed_targets(y, mean, std, mix, defect=None):
    """(t [B, K] float64 with 0 in invalid cells, valid [B, K] bool, ok: every partner inside the batch)"""
    y = np.asarray(y, dtype=np.float32)
    B = y.shape[0]
    valid = np.isfinite(y)
    if defect == "mask_dropped":                   # NaN read as 0
        y, valid = np.nan_to_num(y, nan=0.0, posinf=0.0, neginf=0.0), np.ones_like(valid)
    t = np.where(valid, standardised(np.where(valid, y, 0.0), mean, std), 0.0)
    if mix is not None:
        p = mix[:, 0].astype(np.int64)
        if ((p < 0) | (p >= B)).any():
            return t, valid, False
        lam = mix[:, 3].astype(np.int32).view(np.float32).astype(np.float64)[:, None]
        t = lam * t + (1.0 - lam) * t[p]
        if defect != "partner_validity":
            valid = valid & valid[p]
    return np.where(valid, t, 0.0), valid, True


def reg_loss_ref(z, y, kind="mse", delta=1.0, mean=None, std=None, w=None, mix=None, grad_scale=1.0, defect=None):
    """(loss, dloss/dz [B, K]) in float64 by the header's definition.  defect: one of the planted mistakes of tests/test_regression_cpu.py."""
    z = np.asarray(z, dtype=np.float64)
    B, K = z.shape
    t, valid, ok = mixed_targets(y, mean, std, mix, defect)
    if not ok:
        return float("nan"), np.full((B, K), np.nan)
    r = np.where(valid, z - t, 0.0)
    a = np.abs(r)
    if kind == "mse":
        l, d = r * r, 2.0 * r
    elif kind == "l1":
        l, d = a, np.sign(r)
    elif kind == "huber":
        inner = (a > delta) if defect == "huber_swapped" else (a <= delta)
        l = np.where(inner, 0.5 * r * r, delta * (a - 0.5 * delta))
        d = np.where(inner, r, delta * np.sign(r))
    else:
        raise ValueError(kind)
    mw = valid * (np.ones(K) if w is None else np.asarray(w, dtype=np.float64))[None, :]
    D = float(B * K) if defect == "denominator_BK" else float(mw.sum())
    if D == 0.0:
        return 0.0, np.zeros((B, K))
    return float((mw * l).sum() / D), mw * d / D * grad_scale


def residuals(z, y, mean, std, mix):
    t, valid, _ = mixed_targets(y, mean, std, mix)
    return np.where(valid, np.asarray(z, dtype=np.float64) - t, np.nan), valid


def targets_for(z, scaled, with_nan, mix, seed, delta=DELTA):
    """Raw-scale targets fp32 [B, K] for the logits z (float64): about two residual units of spread, NaN in a fixed pattern of cells when
    with_nan (never in a row that pairs with itself, so D > 0), and no valid residual within MARGIN of 0 or of delta - a target that lands
    there is moved by 0.37 standardised units until none does."""
    B, K = z.shape
    rng = np.random.default_rng(seed)
    mean, std = (MEAN, STD) if scaled else (0.0, 1.0)
    y = ((z + rng.uniform(-2.0, 2.0, size=z.shape)) * std + mean).astype(np.float32)
    if with_nan:
        for b in range(B):
            if partner_of(b, B) != b:
                for k in range(K):
                    if (7 * b + 3 * k) % 5 == 0:
                        y[b, k] = np.nan
    for _ in range(64):
        r, valid = residuals(z, y, mean if scaled else None, std if scaled else None, mix)
        a = np.abs(np.where(valid, r, 1.0))
        close = valid & ((a < 2 * MARGIN) | (np.abs(a - delta) < 2 * MARGIN))
        if not close.any():
            return y
        y[close] += np.float32(0.37 * std)
        if mix is not None:                        # (a row of lambda 0 sees its partner's target alone)
            y[mix[:, 0]] = np.where(close & np.isfinite(y[mix[:, 0]]) & (mix[:, 0] != np.arange(B))[:, None], y[mix[:, 0]] + np.float32(0.23 * std), y[mix[:, 0]])
    raise AssertionError("targets_for: could not move every residual away from the gradient's jumps")


def variants(K):
    """(kind, scaled, weight name, with_nan, mixed)"""
    return itertools.product(KINDS, (False, True), sorted(weights_of(K, 0)), (False, True), (False, True))


def scale_of(scaled, K):
    """(mean, std) as fp32 vectors [K], or (None, None)"""
    if not scaled:
        return None, None
    return np.full(K, MEAN, dtype=np.float32), np.full(K, STD, dtype=np.float32)


# ------------------------------------------------------------------ metrics
def raw_predictions(z, mean, std):
    """yhat = (z * std) + mean with the fp32 product and the fp32 sum each rounded on their own"""
    z = np.asarray(z, dtype=np.float32)
    K = z.shape[1]
    s = np.ones(K, dtype=np.float32) if std is None else np.asarray(std, dtype=np.float32)
    m = np.zeros(K, dtype=np.float32) if mean is None else np.asarray(mean, dtype=np.float32)
    return (z * s[None, :]).astype(np.float32) + m[None, :]


def metrics_ref(batches, mean, std):
    """float64 [K, 6]: n, MAE, RMSE, bias, Pearson r, R^2 over the valid cells of every (z, y) batch; NaN where undefined"""
    zs = np.concatenate([np.asarray(z, dtype=np.float32) for z, _ in batches], axis=0)
    ys = np.concatenate([np.asarray(y, dtype=np.float32) for _, y in batches], axis=0)
    yh = raw_predictions(zs, mean, std).astype(np.float64)
    K = zs.shape[1]
    out = np.full((K, 6), np.nan)
    for k in range(K):
        ok = np.isfinite(ys[:, k])
        y, p = ys[ok, k].astype(np.float64), yh[ok, k]
        n = int(ok.sum())
        out[k, 0] = n
        if n == 0:
            continue
        e = p - y
        out[k, 1], out[k, 2], out[k, 3] = np.abs(e).sum() / n, np.sqrt((e * e).sum() / n), e.sum() / n
        if n < 2:
            continue
        yc, pc = y - y.mean(), p - p.mean()
        vy, vp = (yc * yc).sum(), (pc * pc).sum()
        if vy > 1e-12 * (y * y).sum():
            out[k, 5] = 1.0 - (e * e).sum() / vy
            if vp > 1e-12 * (p * p).sum():
                out[k, 4] = (yc * pc).sum() / np.sqrt(vy * vp)
    return out


METRIC_BATCHES = 5


def metric_batches(B, K, seed, scaled=True):
    """five (z, y) batches of B rows, NaN cells in the second batch.  The predictions of a column are spread over [-2, 2] by construction
    (a golden-ratio sequence over the rows of all batches, plus a little noise) and the targets follow them, so that even the four or five
    observed rows of B = 1 have a variance far above their errors: R^2 stays within (-4, 4), where an fp32 output still resolves the
    1e-6 the GPU test asks of it (tests/test_regression_cpu.py holds that)."""
    rng = np.random.default_rng(seed)
    mean, std = (MEAN, STD) if scaled else (0.0, 1.0)
    out = []
    for i in range(METRIC_BATCHES):
        rows = (i * B + np.arange(B))[:, None] + 0.37 * np.arange(K)[None, :]
        z = (((rows * 0.6180339887) % 1.0) * 4.0 - 2.0 + 0.1 * rng.normal(size=(B, K))).astype(np.float32)
        y = ((z + 0.2 * rng.normal(size=(B, K))) * std + mean + 0.1 * std).astype(np.float32)
        if i == 1:
            y[rng.random((B, K)) < 0.3] = np.nan
        out.append((z, y))
    return out
