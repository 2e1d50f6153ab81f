"""CPU restatements of the Shapley kernels (csrc/shapley.hip, nv_mask_patches_rows of csrc/perturb.hip): the draw in pure integer Python on
the hash the augmentation and MIM restatements state, ranked by ranks_ref of tests/test_perturbation_cpu.py; the label rows; mask_ref with
a label row per job; the accumulator in numpy float64, operation by operation in the kernel's order; the token maps; the exact Shapley
values of a game from its 2^F coalition values; and first-order rounding bounds for the accumulator's outputs.  The GPU tests
(tests/test_shapley_gpu.py) hold the kernels to these; tests/test_shapley_cpu.py checks the restatement itself.

Rounding bounds (u = 2^-53, M = the largest |score| of the volume; first order in u).  In exact arithmetic the marginals of one permutation
telescope, sum_f m_f = s_F - s_0, so delta is rounding only:
  marginal  m = fl(double(a) - double(b)): |error| <= u |a - b| <= 2 M u;  |m| <= 2 M;
  unit      R = 2: fl(m_0 + m_1) adds u |m_0 + m_1| <= 4 M u to the inherited 4 M u, and halving is exact: <= 4 M u (R = 1: 2 M u); |v| <= 2 M;
  sum_f     U additions whose partial sums are <= 2 M U: <= 2 M U^2 u, plus the inherited 4 M U u;
  value     sum / U: (2 M U^2 u + 4 M U u) / U + u |sum / U| <= M u (2 U + 6), then one fp32 rounding 2^-25 |value| <= 2^-24 M;
  total     F additions of the sums, partial sums <= 2 M U F: <= 2 M U F^2 u, plus the inherited F (2 M U^2 u + 4 M U u);
  delta     total / U: the above / U plus u |total / U| <= 2 M F u;  fl(s_F - s_0): 2 M u;  the last subtraction u (2 M F + 2 M):
            |delta| <= M u (2 F^2 + 2 F U + 8 F + 4), and the fp32 rounding of that double scales it by (1 + 2^-24).
"""
from fractions import Fraction
from itertools import permutations as all_orders
from math import factorial

import numpy as np
import torch

from augment_ref import M64, hash64
from test_perturbation_cpu import mask_ref, ranks_ref

SHAPLEY_DOMAIN, SHAPLEY_STRIDE = 0x53484150, 4096
U64 = 2.0 ** -53


def player_keys(seed, unit, b, F):
    """the keys of the F players of (unit, sample b) as the integers (h >> 40): key = that integer times 2^-24, exact in fp32"""
    seed_s = hash64(seed, SHAPLEY_DOMAIN)
    base = ((((unit << 32) + b) & M64) * SHAPLEY_STRIDE) & M64
    return [hash64(seed_s, (base + f) & M64) >> 40 for f in range(F)]


def draw_ref(seed, first_unit, U, R, B, F):
    """int32 [U R, B, F]: row u R of unit u the rank of every player (descending key, ties to the lower index), row u R + 1 (R = 2) F - 1 - rank"""
    out = torch.empty(U * R, B, F, dtype=torch.int32)
    for u in range(U):
        keys = torch.tensor([player_keys(seed, first_unit + u, b, F) for b in range(B)], dtype=torch.float32) * 2.0 ** -24
        rank = ranks_ref(keys)
        out[u * R] = rank
        if R == 2:
            out[u * R + 1] = F - 1 - rank
    return out


def labels_ref(ranks, features):
    """ranks int [Rows, F] (or [Q, B, F]), features int [B, N] -> int32 [Rows, N]: row q takes the features of volume q mod B; an id outside
    [0, F) gives F"""
    F = ranks.shape[-1]
    rows = ranks.reshape(-1, F).long()
    B = features.shape[0]
    feats = features.long()[torch.arange(rows.shape[0]) % B]
    player = (feats >= 0) & (feats < F)
    got = rows.gather(1, feats.clamp(0, F - 1))
    return torch.where(player, got, torch.full_like(got, F)).to(torch.int32)


def mask_rows_ref(x, labels, jobs, patch, baseline=0.0, out=None):
    """mask_ref with labels [Rows, N] and jobs [J, 4] = (b, row, lo, hi); a job with b or row out of range leaves its slot of `out`"""
    B, Rows = x.shape[0], labels.shape[0]
    out = torch.zeros((jobs.shape[0],) + tuple(x.shape[1:])) if out is None else out.clone()
    for j, (b, row, lo, hi) in enumerate(jobs.tolist()):
        if not (0 <= b < B and 0 <= row < Rows):
            continue
        base = baseline
        if torch.is_tensor(baseline):
            base = baseline[b:b + 1] if baseline.shape[0] == B and B > 1 else baseline[0:1]
        out[j] = mask_ref(x[b:b + 1], labels[row:row + 1], torch.tensor([[0, lo, hi]]), patch, base)[0]
    return out


def accumulate_ref(interior, ends, ranks, R=1):
    """interior fp32 [U R, B, F - 1], ends fp32 [B, 2], ranks int [U R, B, F] (torch, CPU) -> (values f32 [B, F], stderr f32 [B, F], delta f32
    [B], sums f64 [B, F, 2]) as numpy arrays: float64 operations one by one in the order of shapley_accumulate_kernel"""
    rk = ranks.numpy().astype(np.int64)
    Q, B, F = rk.shape
    U = Q // R
    e = ends.numpy().astype(np.float64)
    s = np.concatenate([np.broadcast_to(e[None, :, 0:1], (Q, B, 1)), interior.numpy().astype(np.float64).reshape(Q, B, F - 1),
                        np.broadcast_to(e[None, :, 1:2], (Q, B, 1))], axis=2)                     # [Q, B, F + 1]: s_0 .. s_F
    m = (np.take_along_axis(s, rk + 1, 2) - np.take_along_axis(s, rk, 2)).reshape(U, R, B, F)
    unit = m[:, 0] if R == 1 else (m[:, 0] + m[:, 1]) / 2.0
    total, totalsq = np.zeros((B, F)), np.zeros((B, F))
    for u in range(U):
        total = total + unit[u]
        totalsq = totalsq + unit[u] * unit[u]
    n = np.float64(U)
    values = (total / n).astype(np.float32)
    with np.errstate(invalid="ignore", divide="ignore"):
        var = (totalsq - total * total / n) / (n - 1.0)
        stderr = np.sqrt(np.maximum(var, 0.0) / n).astype(np.float32)
    if U == 1:
        stderr = np.full((B, F), np.nan, dtype=np.float32)
    over_players = np.zeros(B)
    for f in range(F):
        over_players = over_players + total[:, f]
    delta = (over_players / n - (e[:, 1] - e[:, 0])).astype(np.float32)
    return values, stderr, delta, np.stack([total, totalsq], axis=2)


def token_maps_ref(values, features):
    """values f32 [B, F], features int [B, N] -> f32 [B, N]: values[b, f] / (patches of f in volume b) as one fp32 division; 0 for no player"""
    B, F = values.shape
    out = torch.zeros(features.shape, dtype=torch.float32)
    for b in range(B):
        feats = features[b].long()
        player = (feats >= 0) & (feats < F)
        count = torch.bincount(feats[player], minlength=F).to(torch.float32)
        idx = feats.clamp(0, F - 1)
        out[b] = torch.where(player, values[b][idx] / count[idx].clamp_min(1.0), torch.zeros(()))
    return out


def exact_shapley(coalition_values):
    """float64 [F] from the 2^F values v[mask] (bit f of mask set = player f present), by the subset formula
    phi_f = sum_{S without f} |S|! (F - |S| - 1)! / F! (v[S + f] - v[S]) in rational arithmetic, rounded once"""
    v = [Fraction(float(c)) for c in coalition_values]
    F = len(v).bit_length() - 1
    assert len(v) == 1 << F
    phi = []
    for f in range(F):
        acc = Fraction(0)
        for mask in range(1 << F):
            if not mask >> f & 1:
                size = bin(mask).count("1")
                acc += Fraction(factorial(size) * factorial(F - size - 1), factorial(F)) * (v[mask | 1 << f] - v[mask])
        phi.append(float(acc))
    return np.array(phi, dtype=np.float64)


def game_scores(coalition_values, ranks):
    """the score rows the accumulator reads for a game on ONE volume: ranks int [Q, F] -> (interior f32 [Q, 1, F - 1], ends f32 [1, 2]);
    s_k of a permutation is the value of the coalition of its k first-ranked players"""
    v = torch.as_tensor(coalition_values, dtype=torch.float32)
    Q, F = ranks.shape
    interior = torch.empty(Q, 1, F - 1)
    for q in range(Q):
        for k in range(1, F):
            mask = sum(1 << f for f in range(F) if int(ranks[q, f]) < k)
            interior[q, 0, k - 1] = v[mask]
    return interior, torch.stack([v[0], v[(1 << F) - 1]]).view(1, 2)


def all_rank_rows(F):
    """int32 [F!, F]: every permutation as a rank row, in itertools' order"""
    return torch.tensor(list(all_orders(range(F))), dtype=torch.int32)


def delta_bound(M, F, U):
    """|delta| of a volume whose scores are within [-M, M] (the derivation is in the module docstring)"""
    return float(M) * U64 * (2 * F * F + 2 * F * U + 8 * F + 4) * (1 + 2.0 ** -24)


def value_bound(M, U):
    """|values - the exact mean of the marginals| per player: M u (2 U + 6) from the double arithmetic and 2^-24 M from the fp32 store"""
    return float(M) * (U64 * (2 * U + 6) + 2.0 ** -24)
