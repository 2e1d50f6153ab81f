"""CPU restatement of the augmentation kernels (csrc/augment.hip): the draw rule of nv_augment_params in pure integer Python (fp32 only
where the header says fp32: torch scalars on the CPU) and the apply rule of nv_augment_apply as a gather in plain torch.  The GPU tests
(tests/test_augment_gpu.py) hold the kernels to these bit for bit; tests/test_augment_cpu.py checks the restatement itself against an
independent formulation (torch.flip / F.pad / slicing)."""
import torch

M64 = (1 << 64) - 1


def hash64(seed, counter):
    """nv_hash64 of csrc/common.h (the splitmix64 finaliser over a seed / counter mix), mod 2^64"""
    x = (((counter + 0x9E3779B97F4A7C15) & M64) * 0xBF58476D1CE4E5B9 & M64) ^ seed
    x ^= x >> 30
    x = x * 0xBF58476D1CE4E5B9 & M64
    x ^= x >> 27
    x = x * 0x94D049BB133111EB & M64
    x ^= x >> 31
    return x


def draw(seed, rank, step, b, d):
    """draw d of sample b at step `step` for `rank`"""
    return hash64(hash64(seed, rank), ((((step << 32) + b) & M64) * 16 + d) & M64)


def below(h, n):
    """an integer on [0, n)"""
    return ((h >> 32) * n) >> 32


def between(h, lo, hi):
    """lo + (hi - lo) u with u = (h >> 40) 2^-24: every operation rounded to fp32 on its own"""
    f = lambda v: torch.tensor(v, dtype=torch.float32)
    u = f(float(h >> 40)) * f(2.0 ** -24)               # both exact
    return f(lo) + (f(hi) - f(lo)) * u                  # three tensor operations: three roundings, no FMA


def params_ref(B, step, in_size, roi, flip_prob=(0, 0, 0), max_shift=(0, 0, 0), scale=(1, 1), shift=(0, 0), seed=0, rank=0):
    """int32 [B, 8]: {ox, oy, oz, flip bits, bits of scale, bits of shift, 0, 0}"""
    rows = torch.zeros(B, 8, dtype=torch.int32)
    for b in range(B):
        h = lambda d: draw(seed, rank, step, b, d)
        flips = 0
        for a in range(3):
            m = max_shift[a]
            rows[b, a] = below(h(a), in_size[a] - roi[a] + 1) + below(h(3 + a), 2 * m + 1) - m
            if (h(6 + a) >> 48) < int(float(flip_prob[a]) * 65536.0):
                flips |= 1 << a
        rows[b, 3] = flips
        rows[b, 4] = between(h(9), *scale).view(torch.int32)
        rows[b, 5] = between(h(10), *shift).view(torch.int32)
    return rows


def apply_ref(x, params, roi, fill=0.0):
    """x fp32 [B, X, Y, Z] or [B, X, Y, Z, T] (CPU), params int32 [B, 8] -> [B, Sx, Sy, Sz(, T)]: a gather, cell by cell in index arithmetic.
    Identity intensity moves int32 patterns (a bit copy); otherwise (x * scale) + shift as two tensor operations."""
    four_d = x.dim() == 5
    v = x if four_d else x.unsqueeze(-1)
    B, T = v.shape[0], v.shape[-1]
    out = torch.empty(B, *roi, T, dtype=torch.float32)
    fill_t = torch.tensor(fill, dtype=torch.float32)
    for b in range(B):
        row = params[b].tolist()
        src, inside = [], []
        for a in range(3):
            i = torch.arange(roi[a])
            s = row[a] + (roi[a] - 1 - i if (row[3] >> a) & 1 else i)
            inside.append((s >= 0) & (s < v.shape[1 + a]))
            src.append(s.clamp(0, v.shape[1 + a] - 1))
        got = v[b][src[0][:, None, None], src[1][None, :, None], src[2][None, None, :]]            # [Sx, Sy, Sz, T]
        scale, shift = (torch.tensor(w, dtype=torch.int32).view(torch.float32) for w in row[4:6])
        if not (scale.item() == 1.0 and shift.item() == 0.0):
            got = (got * scale) + shift
        ok = (inside[0][:, None, None] & inside[1][None, :, None] & inside[2][None, None, :])[..., None].expand_as(got)
        out[b].view(torch.int32).copy_(torch.where(ok, got.contiguous().view(torch.int32), fill_t.view(torch.int32)))
    return out if four_d else out.squeeze(-1)


def bits(t):
    """the int32 patterns of an fp32 tensor (dense copy)"""
    return t.contiguous().view(torch.int32)
