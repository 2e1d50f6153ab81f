"""CPU restatement of the masked-pretraining kernels (csrc/pretrain.hip): the draw rule and label tables of nv_mim_labels in pure integer
Python, and the target, loss and d loss / d pred of nv_recon_loss in float64 on top of the oracle's patchify.  The GPU tests
(tests/test_pretrain_gpu.py) hold the kernels to these; tests/test_pretrain_cpu.py checks the restatement itself (torch autograd, the
oracle's patch order, the mask properties)."""
import math

import torch

from augment_ref import M64, hash64
from oracle import ref_cpu

MIM_DOMAIN, MIM_STRIDE = 0x4D494D, 4096


def masked_count(grid, unit, ratio):
    """m = clamp(floor(ratio U + 0.5), 1, U - 1) u^3"""
    U = (grid[0] // unit) * (grid[1] // unit) * (grid[2] // unit)
    mu = min(max(int(math.floor(ratio * U + 0.5)), 1), U - 1)
    return mu * unit ** 3


def unit_keys(seed, rank, step, b, U):
    """the fp32 keys of sample b's U mask units, as the integers (h >> 40): key = that integer times 2^-24, exact, so the order is the same"""
    seed_p = hash64(hash64(seed, rank), MIM_DOMAIN)
    base = (((step << 32) + b) & M64) * MIM_STRIDE
    return [hash64(seed_p, (base + q) & M64) >> 40 for q in range(U)]


def labels_ref(B, grid, unit, seed, step, rank=0):
    """int32 [B, N]: labels[b, t] = rank(unit of t) u^3 + index of t inside its unit; patches and units indexed by nv_mask_patches' token
    rule (axis 2 slowest, then axis 0, then axis 1); ranks descending in the key, ties to the lower unit index"""
    G0, G1, G2 = grid
    u = unit
    U0, U1, U2 = G0 // u, G1 // u, G2 // u
    U, N = U0 * U1 * U2, G0 * G1 * G2
    out = torch.empty(B, N, dtype=torch.int32)
    for b in range(B):
        keys = unit_keys(seed, rank, step, b, U)
        order = sorted(range(U), key=lambda q: (-keys[q], q))
        rank_of = [0] * U
        for r, q in enumerate(order):
            rank_of[q] = r
        for t in range(N):
            g2, rem = divmod(t, G0 * G1)
            g0, g1 = divmod(rem, G1)
            q = ((g2 // u) * U0 + g0 // u) * U1 + g1 // u
            inside = ((g2 % u) * u + g0 % u) * u + g1 % u
            out[b, t] = rank_of[q] * u ** 3 + inside
    return out


def patches_of(x, patch):
    """x [B, S0, S1, S2] -> [B, N, P]: the oracle's patchify of the [B, 1, D, H, W] view (token and element order of the engine)"""
    p0, p1, p2 = patch
    return ref_cpu.patchify(ref_cpu.fmri_to_video(x), p0, p1, p2)


def targets_ref(x, patch, norm_pix):
    """float64 [B, N, P] reconstruction targets: the patches, standardised by the patch mean and the unbiased variance when norm_pix (MAE)"""
    t = patches_of(x, patch).double()
    if norm_pix:
        mean = t.mean(dim=-1, keepdim=True)
        var = t.var(dim=-1, unbiased=True, keepdim=True)
        t = (t - mean) / (var + 1e-6).sqrt()
    return t


def recon_ref(pred, x, labels, m, patch, kind="l1", norm_pix=True, loss_scale=1.0):
    """pred [B (N + 1), >= P] (any float dtype; the cls row first in every volume) -> (loss float64 scalar, dpred float64 [B (N + 1), P],
    masked bool [B (N + 1)], diff float64 [B (N + 1), P]): the loss over the masked patches and loss_scale d loss / d pred, written out"""
    B = x.shape[0]
    tgt = targets_ref(x, patch, norm_pix)
    N, P = tgt.shape[1], tgt.shape[2]
    rows = pred.double().reshape(B, N + 1, -1)[:, :, :P]
    masked = torch.zeros(B, N + 1, dtype=torch.bool)
    masked[:, 1:] = labels.long() < m
    diff = torch.zeros(B, N + 1, P, dtype=torch.float64)
    diff[:, 1:] = rows[:, 1:] - tgt
    diff = diff * masked[:, :, None]
    count = float(B * m * P)
    if kind == "l1":
        loss = diff.abs().sum() / count
        dpred = torch.sign(diff) * (loss_scale / count)
    else:
        loss = (diff * diff).sum() / count
        dpred = diff * (2.0 * loss_scale / count)
    return loss, dpred.reshape(B * (N + 1), P), masked.reshape(-1), diff.reshape(B * (N + 1), P)


def recon_loss_autograd(pred, x, labels, m, patch, kind="l1", norm_pix=True):
    """an independent formulation for the CPU test: torch's own l1_loss / mse_loss over the gathered masked rows, differentiated by autograd"""
    B = x.shape[0]
    tgt = targets_ref(x, patch, norm_pix)
    N, P = tgt.shape[1], tgt.shape[2]
    p = pred.double().reshape(B, N + 1, -1)[:, 1:, :P]
    sel = labels.long() < m
    fn = torch.nn.functional.l1_loss if kind == "l1" else torch.nn.functional.mse_loss
    return fn(p[sel], tgt[sel], reduction="mean")
