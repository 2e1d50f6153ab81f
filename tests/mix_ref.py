"""CPU restatement of the Mixup / CutMix kernels (csrc/mix.hip) and of the soft-target cross-entropy (ce_row_term_soft, csrc/common.h):

  * the draw rule of nv_mix_params in Python integers and float64 (Joehnk's Beta sampler) and numpy.float32 (the CutMix box);
  * the mixing pass of nv_augment_mix in numpy.float32, built on tests/augment_ref.py (each sample and its partner under their own rows);
  * loss and d(loss)/d(logits) in float64 by the formulas of include/neurovit_hip.h.

tests/test_mix_cpu.py proves the restatements (against torch, against independent formulations, and by planting a defect in each: the
`defect=` arguments exist for that alone); tests/test_mix_gpu.py holds the kernels to them."""
import numpy as np
import torch

import augment_ref as R

COLS = 12
M64 = R.M64
ONE_BITS = 0x3F800000
F32 = np.float32


def draw(seed, rank, step, b, d):
    """draw d of sample b at step `step` for `rank`, in the mix domain"""
    seed_m = R.hash64(R.hash64(seed, rank), 0x4D4958)
    return R.hash64(seed_m, ((((step << 32) + b) & M64) * 256 + d) & M64)


def unit_open(h):
    """((h >> 12) + 0.5) 2^-52: exact in float64, never 0"""
    return (float(h >> 12) + 0.5) * 2.0 ** -52


def f32_bits(v):
    return int(np.array([v], dtype=F32).view(np.int32)[0])


def bits_f32(w):
    return np.array([w], dtype=np.int32).view(F32)[0]


def joehnk(seed, rank, step, b, alpha):
    """(lambda as numpy.float32, tries, [x + y of every try]): Beta(alpha, alpha) by Joehnk's rule in float64"""
    sums = []
    x = y = 0.0
    tries = 64
    for t in range(64):
        x = unit_open(draw(seed, rank, step, b, 16 + 2 * t)) ** (1.0 / alpha)
        y = unit_open(draw(seed, rank, step, b, 17 + 2 * t)) ** (1.0 / alpha)
        sums.append(x + y)
        if x + y <= 1.0:
            tries = t + 1
            break
    return F32(x / (x + y)), tries, sums


def box(lam, centres, roi, defect=None):
    """the CutMix box of a pixel lambda (numpy.float32) and the three centre draws: ([x0, x1, y0, y1, z0, z1], label lambda as numpy.float32).
    defect="unclipped": lo / hi are not clipped to the window (planted, for tests/test_mix_cpu.py)"""
    r = np.sqrt(F32(1.0) - F32(lam))                           # fp32 subtraction, correctly rounded fp32 square root
    out, cells = [], 1
    for a in range(3):
        S = roi[a]
        e = int(F32(S) * r)                                     # fp32 product, truncated
        c = R.below(centres[a], S)
        lo, hi = c - e // 2, c + e // 2
        if defect != "unclipped":
            lo, hi = max(lo, 0), min(hi, S)
        out += [lo, hi]
        cells *= hi - lo
    return out, F32(1.0 - cells / float(roi[0] * roi[1] * roi[2]))


def mix_params_ref(B, step, roi, mixup_alpha=None, cutmix_alpha=None, prob=1.0, switch_prob=0.5, seed=0, rank=0, pixel_bits=None, defect=None):
    """(int32 [B, 12] rows, the smallest |x + y - 1| over every Joehnk try).  pixel_bits: per row, the bits of a pixel lambda to use
    in place of the restated one (the GPU test hands in the device's own, so that box and label lambda can be held bit for bit)."""
    rows = np.zeros((B, COLS), dtype=np.int32)
    gap = float("inf")
    for b in range(B):
        h = lambda d: draw(seed, rank, step, b, d)
        partner = B - 1 - b
        rows[b, :4] = [partner, 0, ONE_BITS, ONE_BITS]
        mode = 0
        if partner != b and (h(0) >> 48) < int(float(prob) * 65536.0):
            if mixup_alpha and cutmix_alpha:
                mode = 2 if (h(1) >> 48) < int(float(switch_prob) * 65536.0) else 1
            else:
                mode = 2 if cutmix_alpha else (1 if mixup_alpha else 0)
        if not mode:
            continue
        lam, tries, sums = joehnk(seed, rank, step, b, cutmix_alpha if mode == 2 else mixup_alpha)
        gap = min(gap, min(abs(s - 1.0) for s in sums))
        if pixel_bits is not None:
            lam = bits_f32(int(pixel_bits[b]))
        rows[b, 1], rows[b, 2], rows[b, 3], rows[b, 4] = mode, f32_bits(lam), f32_bits(lam), tries
        if mode == 2:
            edges, label = box(lam, [h(2), h(3), h(4)], roi, defect)
            rows[b, 5:11] = edges
            rows[b, 3] = f32_bits(label)
    return rows, gap


# ------------------------------------------------------------------ the mixing pass
def identity_rows(B):
    rows = torch.zeros(B, 8, dtype=torch.int32)
    rows[:, 4] = ONE_BITS
    return rows


def mix_apply_ref(x, aug, mix, roi, fill=0.0, defect=None):
    """x fp32 [B, X, Y, Z(, T)] (CPU torch), aug int32 [B, 8] or None (identity rows), mix int32 [B, 12] (torch or numpy) ->
    (out [B, Sx, Sy, Sz(, T)] as torch fp32, moved: a bool array, True where the cell is a bit move of a source voxel or the fill - there
    NaN payloads and -0.0 must survive; elsewhere arithmetic stands between source and output).
    defect="mu_double": mu is formed per cell as 1 - lambda in float64 (planted, for tests/test_mix_cpu.py)"""
    B = x.shape[0]
    aug = identity_rows(B) if aug is None else aug
    A = R.apply_ref(x, aug, roi, fill).numpy()                 # A_s for every sample under its own row
    Au = A.view(np.uint32)
    mix = np.asarray(mix)
    out = np.empty_like(Au)
    moved = np.empty(A.shape, dtype=bool)
    plain = [(int(aug[s, 4]) == ONE_BITS and int(aug[s, 5]) == 0) for s in range(B)]
    for b in range(B):
        p, mode = int(mix[b, 0]), int(mix[b, 1])
        lam = bits_f32(int(mix[b, 2]))
        if mode not in (1, 2) or lam == F32(1.0) or not (0 <= p < B):
            out[b], moved[b] = Au[b], plain[b]
        elif mode == 1:
            with np.errstate(all="ignore"):
                left = lam * A[b]                                # fp32 product
                if defect == "mu_double":
                    right = ((1.0 - np.float64(lam)) * A[p].astype(np.float64)).astype(F32)
                else:
                    mu = F32(1.0) - lam                          # rounded once per sample
                    right = mu * A[p]                            # fp32 product
                out[b] = (left + right).view(np.uint32)          # fp32 sum
            moved[b] = False
        else:
            x0, x1, y0, y1, z0, z1 = (int(v) for v in mix[b, 5:11])
            inside = np.zeros(A.shape[1:], dtype=bool)
            inside[max(x0, 0):max(x1, 0), max(y0, 0):max(y1, 0), max(z0, 0):max(z1, 0)] = True
            out[b] = np.where(inside, Au[p], Au[b])
            moved[b] = np.where(inside, plain[p], plain[b])
    return torch.from_numpy(out.view(F32)), moved


def same_bits(got, want, moved):
    """the kernel's output against the restatement: bit for bit wherever the cell is a move or the restatement holds no NaN; a NaN that
    arithmetic produced must be a NaN (its payload is the hardware's business, as in tests/test_augment_gpu.py)"""
    g, w = R.bits(got).numpy(), R.bits(want).numpy()
    nan = np.isnan(want.numpy())
    exact = moved | ~nan
    return bool(np.array_equal(g[exact], w[exact]) and np.isnan(got.numpy()[~exact]).all())


# ------------------------------------------------------------------ the loss
def soft_targets(y, C, mix=None):
    """q [B, C] float64 = lam onehot(y) + (1 - lam) onehot(y[partner]); lam is the fp32 label lambda of the row, taken to float64"""
    y = np.asarray(y)
    B = len(y)
    q = np.zeros((B, C))
    for b in range(B):
        lam, p = 1.0, b
        if mix is not None:
            p, lam = int(mix[b][0]), float(bits_f32(int(mix[b][3])))
        q[b, y[b]] += lam
        q[b, y[p]] += 1.0 - lam
    return q


def ce_soft_ref(z, y, eps=0.0, w=None, mix=None, defect=None):
    """(loss, d(loss)/d(logits)) in float64:
        q' = (1 - eps) q + eps / C;  loss = sum_bc w_c q'_bc (-log p_bc) / D;  D = sum_bc w_c q_bc;  dloss/dz_bc = (p_bc S_b - w_c q'_bc) / D
    defect="denominator_B": D = B whatever the weights (planted, for tests/test_mix_cpu.py)"""
    z = np.asarray(z, dtype=np.float64)
    B, C = z.shape
    w = np.ones(C) if w is None else np.asarray(w, dtype=np.float64)
    q = soft_targets(y, C, mix)
    qs = (1.0 - eps) * q + eps / C
    zs = z - z.max(axis=1, keepdims=True)
    logp = zs - np.log(np.exp(zs).sum(axis=1, keepdims=True))
    D = float(B) if defect == "denominator_B" else (w * q).sum()
    wq = w * qs
    loss = -(wq * logp).sum() / D
    grad = (np.exp(logp) * wq.sum(axis=1, keepdims=True) - wq) / D
    return loss, grad


# ------------------------------------------------------------------ the draws the GPU test takes (shared with tests/test_mix_cpu.py, which
# proves that no Joehnk try of theirs lands within 1e-9 of the acceptance edge x + y = 1: the device's pow may differ from the host's in
# the last bits of a double, ~1e-16, so accept / reject - and with it `tries` - is the same on both sides on EVERY row)
PARAM_ROI = (80, 81, 79)
PARAM_CONFIGS = {
    "mixup": dict(mixup_alpha=0.4),
    "cutmix": dict(cutmix_alpha=1.0),
    "both": dict(mixup_alpha=0.2, cutmix_alpha=0.8),
    "half": dict(mixup_alpha=0.1, cutmix_alpha=1.0, prob=0.5, switch_prob=0.25),
    "never": dict(mixup_alpha=0.4, cutmix_alpha=0.4, prob=0.0),
}
PARAM_TRIPLES = ((0, 0, 0), (0xDEADBEEFCAFEF00D, 5, 2 ** 20 + 3), (0, 5, 0), (0, 0, 1))      # (seed, rank, step)
PARAM_BATCHES = (1, 2, 3, 257)
