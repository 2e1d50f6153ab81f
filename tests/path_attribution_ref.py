"""CPU restatements of the path-attribution kernels (csrc/path_attr.hip) and of the whole integrated-gradients method: plain torch on the
CPU, every fp32 sum and product a separate tensor operation (one rounding each, no FMA), in the order the header states.

  path_points_ref        out[j] = bl + alphas[k] * (x[b] - bl)                                  (nv_path_points)
  class_score_grads_ref  one-hot, or p_c (delta_ci - p_i) of the max-subtracted fp32 softmax    (nv_class_score_grads)
  path_accumulate_ref    acc[b] = acc[b] + weights[k] * g[j], job after job                     (nv_path_accumulate)
  path_finish_ref        (x - bl) * acc                                                         (nv_path_finish)
  token_sums_ref         float64 [B, N, 2]: sum and sum of |.| of every patch's voxels          (nv_attr_token_sums, before its fp32 store)
  integrated_gradients_ref   the method of ViT.integrated_gradients on any differentiable forward
"""
import torch


def _baseline_rows(baseline, B, V):
    """[B, V] fp32 rows of a baseline that is a float, or a [B, V] / [1, V] tensor"""
    if torch.is_tensor(baseline):
        return baseline.reshape(baseline.shape[0], V).expand(B, V)
    return torch.full((B, V), float(baseline), dtype=torch.float32)


def path_points_ref(x, jobs, alphas, baseline=0.0, out=None):
    """x [B, V] fp32, jobs [J, 2] int of (b, k), alphas [K] fp32 -> [J, V]; `out`: the pre-filled result (a job with b or k out of range
    leaves its row as it is)"""
    B, V = x.shape
    bl = _baseline_rows(baseline, B, V)
    out = torch.zeros((jobs.shape[0], V)) if out is None else out.clone()
    for j, (b, k) in enumerate(jobs.tolist()):
        if not (0 <= b < B and 0 <= k < alphas.shape[0]):
            continue
        d = x[b] - bl[b]
        t = alphas[k] * d
        out[j] = bl[b] + t
    return out


def class_score_grads_ref(logits, jobs, cls, kind, out=None):
    """logits [J, C] fp32, jobs [J, 2], cls [B] int64 -> [J, C] fp32"""
    J, C = logits.shape
    out = torch.zeros((J, C)) if out is None else out.clone()
    for j, (b, _) in enumerate(jobs.tolist()):
        if not 0 <= b < cls.shape[0]:
            continue
        c = int(cls[b])
        if not 0 <= c < C:
            out[j] = float("nan")
            continue
        onehot = torch.zeros(C)
        onehot[c] = 1.0
        if kind == "logit":
            out[j] = onehot
        else:
            e = torch.exp(logits[j] - logits[j].max())
            p = e / e.sum()
            out[j] = p[c] * (onehot - p)
    return out


def path_accumulate_ref(g, jobs, weights, acc):
    """g [J, V], jobs [J, 2], weights [K], acc [B, V] -> the new acc"""
    acc = acc.clone()
    for j, (b, k) in enumerate(jobs.tolist()):
        if not (0 <= b < acc.shape[0] and 0 <= k < weights.shape[0]):
            continue
        t = weights[k] * g[j]
        acc[b] = acc[b] + t
    return acc


def path_finish_ref(acc, x, baseline=0.0):
    B, V = x.shape
    d = x - _baseline_rows(baseline, B, V)
    return d * acc


def token_sums_ref(attr, patch):
    """attr [B, S0, S1, S2] -> float64 [B, N, 2]; token t = (i2 / p2) G0 G1 + (i0 / p0) G1 + i1 / p1, its voxels in the order
    (d0 p1 + d1) p2 + d2 - the rows of oracle.ref_cpu.patchify on the [B, 1, D, H, W] view"""
    p0, p1, p2 = (patch,) * 3 if isinstance(patch, int) else tuple(patch)
    B, S0, S1, S2 = attr.shape
    G0, G1, G2 = S0 // p0, S1 // p1, S2 // p2
    rows = attr.double().reshape(B, G0, p0, G1, p1, G2, p2).permute(0, 5, 1, 3, 2, 4, 6).reshape(B, G2 * G0 * G1, p0 * p1 * p2)
    return torch.stack([rows.sum(-1), rows.abs().sum(-1)], dim=-1)


def integrated_gradients_ref(forward, x, cls, alphas, weights, baseline=0.0, score="logit", chunk=None):
    """forward: [J, ...] -> logits [J, C] (differentiable); x [B, ...] fp32; cls [B] int64; alphas / weights [K] fp32.  Jobs are volume-major
    (b, 0 .. K - 1), taken in slices of `chunk` (None: all at once).  Returns (attributions of x's shape, delta float64 [B], score_input,
    score_baseline)."""
    B, K = x.shape[0], alphas.shape[0]
    V = x[0].numel()
    flat = x.reshape(B, V)
    base = baseline.reshape(baseline.shape[0], V) if torch.is_tensor(baseline) else baseline
    jobs = torch.stack([torch.arange(B).repeat_interleave(K), torch.arange(K).repeat(B)], 1)
    chunk = B * K if chunk is None else chunk

    def scores(logits, rows):
        if score == "logit":
            return logits.gather(1, cls[rows][:, None])[:, 0]
        e = torch.exp(logits - logits.max(dim=1, keepdim=True).values)
        return (e / e.sum(dim=1, keepdim=True)).gather(1, cls[rows][:, None])[:, 0]

    acc = torch.zeros(B, V)
    for first in range(0, B * K, chunk):
        part = jobs[first:first + chunk]
        points = path_points_ref(flat, part, alphas, base).reshape((part.shape[0],) + tuple(x.shape[1:])).requires_grad_(True)
        (g,) = torch.autograd.grad(scores(forward(points), part[:, 0]).sum(), points)
        acc = path_accumulate_ref(g.reshape(part.shape[0], V), part, weights, acc)
    attr = path_finish_ref(acc, flat, base)
    with torch.no_grad():
        ends = torch.cat([flat, _baseline_rows(base, B, V)]).reshape((2 * B,) + tuple(x.shape[1:]))
        s = scores(forward(ends), torch.arange(B).repeat(2))
    delta = attr.double().sum(1) - (s[:B].double() - s[B:].double())
    return attr.reshape(x.shape), delta, s[:B], s[B:]
