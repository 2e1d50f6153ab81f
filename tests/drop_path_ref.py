"""CPU restatement of stochastic depth (csrc/drop_path.hip and the path-aware residual sites), imported by tests/test_drop_path_cpu.py and
tests/test_drop_path_gpu.py.

  schedule / draw_table   the schedule and the draw of nv_drop_path_draw, in numpy uint64 like oracle.ref_cpu.drop_mask_at
  vit_forward_sd          ref_cpu.vit_forward's loop with x <- x + f[l, c, b] * branch(x), composed from the oracle's own blocks; runs under
                          autograd, so it yields gradients
"""
import numpy as np
import torch
import torch.nn.functional as F

from oracle import ref_cpu

LINEAR, CONSTANT = "linear", "constant"
DOMAIN = 0x50415448
_M64 = (1 << 64) - 1


def schedule(rate: float, depth: int, kind: str = LINEAR) -> np.ndarray:
    """q_l, float64 [depth].  The kernel receives `rate` as a float: its value is the fp32 one."""
    r = np.float64(np.float32(rate))
    if kind == CONSTANT:
        return np.full(depth, r, dtype=np.float64)
    if depth == 1:
        return np.zeros(1, dtype=np.float64)
    return r * np.arange(depth, dtype=np.float64) / np.float64(depth - 1)


def _hash64(seed, grp):
    """csrc/common.h::nv_hash64 on numpy uint64 (scalars or arrays)"""
    with np.errstate(over="ignore"):
        x = ((np.asarray(grp, dtype=np.uint64) + np.uint64(0x9E3779B97F4A7C15)) * np.uint64(0xBF58476D1CE4E5B9)) ^ np.uint64(seed)
        x = x ^ (x >> np.uint64(30)); x = x * np.uint64(0xBF58476D1CE4E5B9)
        x = x ^ (x >> np.uint64(27)); x = x * np.uint64(0x94D049BB133111EB)
        return x ^ (x >> np.uint64(31))


def draw_table(seed: int, B: int, depth: int, rate: float, kind: str = LINEAR) -> torch.Tensor:
    """fp32 [depth, 2, B]: 0 or 1 / (1 - q_l), bit for bit what nv_drop_path_draw writes."""
    q = schedule(rate, depth, kind)
    seed_p = _hash64(seed & _M64, np.uint64(DOMAIN))
    out = np.ones((depth, 2, B), dtype=np.float32)
    b = np.arange(B, dtype=np.uint64)
    for l in range(depth):
        thresh = int(q[l] * 65536.0)
        if thresh == 0:
            continue
        kept_factor = np.float32(1.0) / (np.float32(1.0) - np.float32(q[l]))
        for c in range(2):
            h = _hash64(seed_p, (np.uint64(2 * l + c) << np.uint64(32)) + b)
            out[l, c] = np.where((h >> np.uint64(48)) >= np.uint64(thresh), kept_factor, np.float32(0))
    return torch.from_numpy(out)


def vit_forward_sd(sd, cfg, video, table, emulate_bf16=False, dropout=None, taps=None):
    """ref_cpu.vit_forward with x <- x + f[l, c, b] * branch(x): table fp32 [depth, 2, B].  The oracle's blocks apply the element-dropout
    factor e inside themselves, so their output is multiplied by f: (v e) f where the kernels form v (e f) - the same bits for f in {0, 1}
    (both products are exact), one rounding apart otherwise, which the callers' tolerances hold."""
    dp = dropout if dropout and (dropout[0] > 0 or dropout[1] > 0) else None
    x = ref_cpu.patch_embed(sd, cfg, video, emulate_bf16, taps, (dp[1], ref_cpu.site_seed(dp[2], 4 * cfg.depth)) if dp and dp[1] > 0 else None)
    for i in range(cfg.depth):
        pa, pf = f"transformer.layers.{i}.0.", f"transformer.layers.{i}.1."
        da = (dp[0], ref_cpu.site_seed(dp[2], 4 * i + 0), ref_cpu.site_seed(dp[2], 4 * i + 1)) if dp and dp[0] > 0 else None
        df = (dp[0], ref_cpu.site_seed(dp[2], 4 * i + 2), ref_cpu.site_seed(dp[2], 4 * i + 3)) if dp and dp[0] > 0 else None
        x = ref_cpu.attention(sd, pa, x, cfg.heads, cfg.dim_head, emulate_bf16, taps, da) * table[i, 0][:, None, None] + x
        x = ref_cpu.feed_forward(sd, pf, x, emulate_bf16, df) * table[i, 1][:, None, None] + x
        if taps is not None:
            taps[f"block{i}"] = x
    x = x.mean(dim=1) if cfg.pool == "mean" else x[:, 0]
    x = F.layer_norm(x, (cfg.dim,), sd["mlp_head.0.weight"], sd["mlp_head.0.bias"], ref_cpu.LN_EPS)
    return F.linear(x, sd["mlp_head.1.weight"], sd["mlp_head.1.bias"])
