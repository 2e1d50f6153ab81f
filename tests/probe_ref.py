"""numpy restatement of the linear-probe kernels (neurovit_amd/csrc/probe.hip): nv_probe_stats, nv_probe_grad (with its chunk-partial order),
nv_probe_step and a whole fit, in float64 - or, with dtype=np.float32, the fp32 algorithm on the CPU - and the inputs the GPU tests use.
What the restatement is worth is proven on the CPU in tests/test_probe_cpu.py (torch.autograd in float64, the closed-form ridge solution,
planted defects that must fail); tests/test_probe_gpu.py holds the kernels to it.  Where the order of a sum matters it is an explicit
ascending loop over the 256-row chunks, not np.sum over everything."""
import math

import numpy as np

CHUNK = 256                  # NV_PROBE_CHUNK
LOSS_GATE = 1e-5             # the project's gate for its loss kernels (knn_ref.SOFTMAX_GATE, test_regression_gpu.py)
FIT_FACTOR, FIT_FLOOR = 16.0, 1e-6      # the end-to-end gate: 16 x the deviation of the fp32 restatement from the float64 one, not below 1e-6
BETAS, ADAM_EPS = (0.9, 0.999), 1e-8


def chunks(N):
    return [(c, min(c + CHUNK, N)) for c in range(0, N, CHUNK)]


def rel(a, b):
    """max-norm relative deviation of a from b"""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-300))


# ------------------------------------------------------------------ statistics
def stats_ref(X, skip_nan=False, eps=1e-12):
    """-> (mean f32 [d], rstd f32 [d], std f32 [d], count f64 [d]): two passes in float64 over the chunks in ascending row order, the chunk
    partials added in ascending chunk order, every result rounded once.  Variance exactly 0 (or nothing observed): rstd 0."""
    X = np.asarray(X, np.float32)
    N, d = X.shape
    seen = ~np.isnan(X) if skip_nan else np.ones(X.shape, bool)
    x64 = np.where(seen, X, 0).astype(np.float64)

    def chunked(values):
        total = np.zeros(d, np.float64)
        for lo, hi in chunks(N):
            total = total + np.cumsum(values[lo:hi], axis=0)[-1]          # cumsum adds in sequence (np.sum would add pairwise)
        return total
    count = chunked(seen.astype(np.float64))
    with np.errstate(invalid="ignore", divide="ignore"):
        mean = np.where(count > 0, chunked(x64) / count, 0.0)
        dev = np.where(seen, X.astype(np.float64) - mean, 0.0)
        var = np.where(count > 0, chunked(dev * dev) / count, 0.0)
        rstd = np.where(var > 0, 1.0 / np.sqrt(var + np.float64(np.float32(eps))), 0.0)
    return mean.astype(np.float32), rstd.astype(np.float32), np.sqrt(var).astype(np.float32), count


def denom_ref(labels, C, class_weight=None, *, count_unlabelled=False):
    """the class-weighted count of the rows whose label lies in [0, C), float64, chunk partials in ascending order"""
    labels = np.asarray(labels)
    total = 0.0
    for lo, hi in chunks(len(labels)):
        part = 0.0
        for y in labels[lo:hi]:
            if 0 <= y < C:
                part += 1.0 if class_weight is None else float(np.float32(class_weight[y]))
            elif count_unlabelled:
                part += 1.0
        total += part
    return np.array([total], np.float64)


# ------------------------------------------------------------------ loss and gradient
def standardise(X, mean, rstd, dtype):
    X = np.asarray(X, np.float32).astype(dtype)
    if mean is None:
        return X
    return ((X - np.asarray(mean, np.float32).astype(dtype)).astype(dtype) * np.asarray(rstd, np.float32).astype(dtype)).astype(dtype)


def logits_ref(X, W, b, mean=None, rstd=None, dtype=np.float64):
    Z = standardise(X, mean, rstd, dtype)
    return (Z @ np.asarray(W, dtype).T + np.asarray(b, dtype)).astype(dtype), Z


def grad_ref(X, W, b, H, C, l2, *, labels=None, targets=None, mean=None, rstd=None, class_weight=None, target_mean=None, target_std=None, denom=None,
             dtype=np.float64, softmax_all=False, count_nan=False, count_unlabelled=False):
    """-> (dW [M, d], db [M], loss [H]) in `dtype` (the chunk sums and the final division always in float64, then cast).  Head h owns the
    columns [h C, (h + 1) C).  denom: as stats_ref / denom_ref give it (default: computed here).  Planted defects for the CPU test:
    softmax_all (one softmax over all M columns), count_nan (a missing target counts in the denominator), count_unlabelled (an unlabelled
    row counts in the denominator and pulls towards class 0)."""
    M = H * C
    W, b = np.asarray(W), np.asarray(b)          # fp32 as the kernel sees them, or the float64 parameters of a float64 fit
    N, d = np.asarray(X).shape
    logit, Z = logits_ref(X, W, b, mean, rstd, dtype)
    G = np.zeros((N, M), dtype)            # dlogits, not yet divided by the denominator
    Lc = np.zeros((N, M), dtype)           # loss cells: column h C of a head (classification) or every column (regression)
    if labels is not None:
        labels = np.asarray(labels)
        ok = (labels >= 0) & (labels < C)
        y = np.where(ok, labels, 0)
        if count_unlabelled:
            ok = np.ones(N, bool)
        cw = np.ones(N, dtype) if class_weight is None else np.asarray(class_weight, np.float32).astype(dtype)[y]
        D = denom_ref(labels, C, class_weight, count_unlabelled=count_unlabelled) if denom is None else np.asarray(denom, np.float64)
        Dm = np.full(M, D[0])
        groups = [np.arange(M)] if softmax_all else [np.arange(h * C, (h + 1) * C) for h in range(H)]
        for cols in groups:
            lg = logit[:, cols]
            mx = lg.max(1, keepdims=True)
            e = np.exp((lg - mx).astype(dtype)).astype(dtype)
            s = np.zeros((N, 1), dtype)
            for k in range(e.shape[1]):
                s = (s + e[:, k:k + 1]).astype(dtype)
            p = (e / s).astype(dtype)
            for h in range(H):
                own = np.arange(h * C, (h + 1) * C)
                if own[0] < cols[0] or own[-1] > cols[-1]:
                    continue
                at = own - cols[0]
                onehot = np.zeros((N, C), dtype)
                onehot[np.arange(N), y] = 1
                G[:, own] = np.where(ok[:, None], cw[:, None] * (p[:, at] - onehot), 0).astype(dtype)
                nll = (np.log(s[:, 0]).astype(dtype) - (lg[np.arange(N), at[y]] - mx[:, 0]).astype(dtype)).astype(dtype)
                Lc[:, own[0]] = np.where(ok, cw * nll, 0).astype(dtype)
    else:
        T = np.asarray(targets, np.float32).reshape(N, C)
        seen = ~np.isnan(T)
        tm = np.zeros(C, np.float32) if target_mean is None else np.asarray(target_mean, np.float32)
        ts = np.ones(C, np.float32) if target_std is None else np.asarray(target_std, np.float32)
        # the standardised target is formed in fp32, each operation rounded, as the kernel (and nv_reg_loss) forms it
        t = ((np.where(seen, T, 0).astype(np.float32) - tm).astype(np.float32) / ts).astype(np.float32).astype(dtype)
        D = (np.full(C, float(N)) if count_nan else seen.sum(0).astype(np.float64)) if denom is None else np.asarray(denom, np.float64)
        Dm = np.tile(D, H)
        r = (logit - np.tile(t, (1, H))).astype(dtype)
        seenM = np.tile(seen, (1, H))
        G = np.where(seenM, 2 * r, 0).astype(dtype)
        Lc = np.where(seenM, r * r, 0).astype(dtype)
    SW, Sb, SL = np.zeros((M, d), np.float64), np.zeros(M, np.float64), np.zeros(M, np.float64)
    for lo, hi in chunks(N):
        SW = SW + (G[lo:hi].T @ Z[lo:hi]).astype(dtype).astype(np.float64)          # the chunk's partial lives in `dtype`
        # bias and loss cells: row by row in float64 (cumsum adds in sequence, np.sum would add pairwise)
        Sb = Sb + np.cumsum(G[lo:hi].astype(np.float64), axis=0)[-1]
        SL = SL + np.cumsum(Lc[lo:hi].astype(np.float64), axis=0)[-1]
    with np.errstate(invalid="ignore", divide="ignore"):
        live = Dm > 0
        l2m = np.repeat(np.asarray(l2, np.float32).astype(np.float64), C)
        dW = np.where(live[:, None], SW / Dm[:, None], 0.0) + l2m[:, None] * W.astype(np.float64)
        db = np.where(live, Sb / Dm, 0.0)
        cell = np.where(live, SL / Dm, 0.0)
    loss = np.zeros(H, np.float64)
    for h in range(H):
        for k in range(C):
            loss[h] = loss[h] + cell[h * C + k]
    return dW.astype(dtype), db.astype(dtype), loss.astype(dtype)


# ------------------------------------------------------------------ Adam and the fit
def lr_at(k, steps, lr, schedule="cosine"):
    """neurovit_amd.optim.LRSchedule(lr, steps, kind=schedule).lr_at(k) without warm-up: cosine to 0, exactly 0 at k = steps"""
    if schedule == "constant":
        return lr
    q = min(1.0, k / max(1, steps))
    if q >= 1.0:
        return 0.0
    return lr * 0.5 * (1.0 + math.cos(math.pi * q)) if schedule == "cosine" else lr + (0.0 - lr) * q


def adam_ref(p, g, m, v, step_size, bc2_sqrt, dtype=np.float64, betas=BETAS, eps=ADAM_EPS):
    """one Adam update; in float32 every operation is rounded on its own, in the kernel's order.  step_size broadcasts over p's rows."""
    f = dtype
    b1, b2, omb1, omb2 = f(betas[0]), f(betas[1]), f(1.0 - betas[0]), f(1.0 - betas[1])
    p, g, m, v = (np.asarray(t, f) for t in (p, g, m, v))
    m = ((b1 * m).astype(f) + (omb1 * g).astype(f)).astype(f)
    v = ((b2 * v).astype(f) + ((omb2 * g).astype(f) * g).astype(f)).astype(f)
    den = ((np.sqrt(v).astype(f) / f(bc2_sqrt)).astype(f) + f(eps)).astype(f)
    p = (p - (np.asarray(step_size, f) * (m / den).astype(f)).astype(f)).astype(f)
    return p, m, v


def fit_ref(X, H, C, l2, steps, lr=0.01, schedule="cosine", *, dtype=np.float64, decoupled=False, W0=None, b0=None, **kw):
    """Full-batch Adam from zeros (or W0 / b0): -> (W [M, d], b [M], loss history [steps, H]).  kw: what grad_ref takes.  decoupled: the planted
    defect - the L2 term leaves the gradient and becomes AdamW's decay p -= lr l2 p."""
    M, d = H * C, np.asarray(X).shape[1]
    f = dtype
    W = np.zeros((M, d), f) if W0 is None else np.asarray(W0, f).copy()
    b = np.zeros(M, f) if b0 is None else np.asarray(b0, f).copy()
    mW, vW, mb, vb = np.zeros_like(W), np.zeros_like(W), np.zeros_like(b), np.zeros_like(b)
    hist = np.zeros((steps, H), f)
    l2m = np.repeat(np.asarray(l2, np.float64), C)
    for k in range(1, steps + 1):
        dW, db, hist[k - 1] = grad_ref(X, W, b, H, C, np.zeros(H) if decoupled else l2, dtype=f, **kw)
        lrk = lr_at(k, steps, lr, schedule)
        size = np.float32(lrk / (1.0 - BETAS[0] ** k)) if f == np.float32 else lrk / (1.0 - BETAS[0] ** k)
        bc2 = math.sqrt(1.0 - BETAS[1] ** k)
        if decoupled:
            W = W * (1.0 - lrk * l2m)[:, None]
        W, mW, vW = adam_ref(W, dW, mW, vW, size, bc2, f)
        b, mb, vb = adam_ref(b, db, mb, vb, size, bc2, f)
    return W, b, hist


def ridge_ref(Z, t, lam):
    """The stationary point of (1 / D) sum (w z + c - t)^2 + (lam / 2) |w|^2 over the observed rows (t not NaN), the intercept c unpenalised:
    (2 Z^T Z / D + lam I) w + (2 Z^T 1 / D) c = 2 Z^T t / D,  (2 1^T Z / D) w + 2 c = 2 1^T t / D.  float64 -> (w [d], c)."""
    Z, t = np.asarray(Z, np.float64), np.asarray(t, np.float64)
    seen = ~np.isnan(t)
    Z, t = Z[seen], t[seen]
    D, d = len(t), Z.shape[1]
    A = np.zeros((d + 1, d + 1))
    A[:d, :d] = 2.0 * Z.T @ Z / D + lam * np.eye(d)
    A[:d, d] = A[d, :d] = 2.0 * Z.sum(0) / D
    A[d, d] = 2.0
    sol = np.linalg.solve(A, np.concatenate([2.0 * Z.T @ t / D, [2.0 * t.sum() / D]]))
    return sol[:d], sol[d]


# ------------------------------------------------------------------ prediction and evaluation
def softmax_heads(logit, H, C):
    logit = np.asarray(logit, np.float64).reshape(len(logit), H, C)
    e = np.exp(logit - logit.max(2, keepdims=True))
    return e / e.sum(2, keepdims=True)


def evaluate_ref(probs, labels, groups=None):
    """probs float64 [Nq, H, C] -> (acc [H], subject_acc [H] or None): arg-max with ties to the lower class; per subject the mean of its volumes'
    probabilities, arg-max, against the label of its first volume"""
    labels = np.asarray(labels)
    acc = (probs.argmax(2) == labels[:, None]).mean(0)
    if groups is None:
        return acc, None
    groups = np.asarray(groups)
    ids = [g for g in range(groups.max() + 1) if (groups == g).any()]
    hit = np.zeros(probs.shape[1])
    for g in ids:
        rows = np.nonzero(groups == g)[0]
        hit += probs[rows].mean(0).argmax(1) == labels[rows[0]]
    return acc, hit / len(ids)


# ------------------------------------------------------------------ inputs
L2_GRID = (1e-4, 1e-3, 1e-2, 1e-1, 0.0, 1.0, 3e-3, 3e-2)


def features(N, d, seed, const_col=None):
    """unit-norm rows plus a DC offset of 0.3 / sqrt(d) (what a pooled, L2-normalised embedding looks like); const_col: a zero-variance column"""
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((N, d))
    X /= np.linalg.norm(X, axis=1, keepdims=True)
    X += 0.3 / math.sqrt(d)
    X = X.astype(np.float32)
    if const_col is not None:
        X[:, const_col] = np.float32(0.25)
    return X


def cls_case(N, d, C, H, seed):
    """-> dict(X, labels, class_weight, W, b, l2): about a seventh of the labels -1, one label C (out of range on the other side), labels that
    depend on the features (so a fit has something to find), a zero-variance column (d > 4), random weights of the size a short fit reaches"""
    rng = np.random.default_rng(seed + 1)
    X = features(N, d, seed, const_col=1 if d > 4 else None)
    proj = rng.standard_normal((d, C))
    labels = ((X - X.mean(0)) @ proj).argmax(1).astype(np.int32)
    if N > 1:
        labels[rng.random(N) < 1.0 / 7.0] = -1
        labels[N // 2] = C
        labels[0] = 0
    M = H * C
    return dict(X=X, labels=labels, class_weight=rng.uniform(0.5, 2.0, C).astype(np.float32), W=(0.5 * rng.standard_normal((M, d))).astype(np.float32),
                b=(0.1 * rng.standard_normal(M)).astype(np.float32), l2=[L2_GRID[h % len(L2_GRID)] for h in range(H)])


def reg_case(N, d, K, H, seed, dead_column=True):
    """-> dict(X, targets, W, b, l2): linear targets plus noise on a raw scale (mean 50, spread 10), a NaN every 17th row (the column rotates);
    dead_column (K >= 3): the last column is missing everywhere, so its denominator is 0"""
    rng = np.random.default_rng(seed + 2)
    X = features(N, d, seed)
    T = 50.0 + 10.0 * ((X - X.mean(0)) @ rng.standard_normal((d, K)) * math.sqrt(d) + 0.1 * rng.standard_normal((N, K)))
    T = T.astype(np.float32)
    for r in range(0, N, 17):
        T[r, (r // 17) % K] = np.nan
    if dead_column and K >= 3:
        T[:, K - 1] = np.nan
    M = H * K
    return dict(X=X, targets=T, W=(0.5 * rng.standard_normal((M, d))).astype(np.float32), b=(0.1 * rng.standard_normal(M)).astype(np.float32),
                l2=[L2_GRID[h % len(L2_GRID)] for h in range(H)])


INT_MISSING = (100, 255, 256, 400, 516)          # the rows without a target: 517 - 5 = 512 = 2^9 observed, the last chunk (rows 512 ..) is ragged
INT_H, INT_K, INT_L2 = 3, 2, (0.0, 0.5, 2.0)


def int_case(d, seed):
    """The exact case: features, weights, biases in {-1, 0, 1}, targets in -4 .. 4, l2 in {0, 1/2, 2}, D = 512: every logit (|.| <= d + 1), residual,
    square (< 2^21), chunk partial of dW (256 rows: < 2^20) is an integer below 2^24, the division by 512 and the product with l2 are exact in
    double - the result does not depend on the order of any sum."""
    rng = np.random.default_rng(seed)
    N, M = 517, INT_H * INT_K
    X = rng.integers(-1, 2, size=(N, d)).astype(np.float32)
    T = rng.integers(-4, 5, size=(N, INT_K)).astype(np.float32)
    T[list(INT_MISSING)] = np.nan
    return dict(X=X, targets=T, W=rng.integers(-1, 2, size=(M, d)).astype(np.float32), b=rng.integers(-1, 2, size=M).astype(np.float32), l2=list(INT_L2))
