"""CPU restatement of the affine augmentation kernels (csrc/affine.hip): the draw rule of nv_affine_params in integer Python and Python
floats (doubles; fp32 only where the header says fp32) and the apply rule of nv_affine_apply as a gather in plain torch, every fp32
operation a tensor operation of its own (no FMA on the CPU path).  The same apply function takes dtype=torch.float64: the geometry it
states is checked against F.grid_sample there, and its fp32 rounding against itself (tests/test_affine_cpu.py).  The GPU tests
(tests/test_affine_gpu.py) hold the kernels to the fp32 form bit for bit.  It also builds the hand-written tables and the volumes both
test files use, so that what the CPU tests prove about these inputs holds for what the GPU tests run."""
import itertools
import math

import torch

import augment_ref as A

COLS = 16
ONE, ZERO = 0x3F800000, 0


def f32_bits(v):
    """the int32 pattern of the fp32 nearest to the Python float v (a zero is +0.0)"""
    return int(torch.tensor(v + 0.0, dtype=torch.float64).to(torch.float32).view(torch.int32))


def draw(seed, rank, step, b, d):
    """draw d of sample b at step `step` for `rank`, in the affine domain"""
    seed_f = A.hash64(A.hash64(seed, rank), 0x414646)
    return A.hash64(seed_f, ((((step << 32) + b) & A.M64) * 32 + d) & A.M64)


def real(h):
    return (h >> 11) * 2.0 ** -53


def mat3(a, b):
    return [[(a[r][0] * b[0][q] + a[r][1] * b[1][q]) + a[r][2] * b[2][q] for q in range(3)] for r in range(3)]


def map_rows(roi, o, flips, theta=(0.0, 0.0, 0.0), zoom=(1.0, 1.0, 1.0), t=(0.0, 0.0, 0.0), applied=True):
    """the twelve doubles of the map: M = Rz (Ry Rx) diag(f / z), m_a3 = ((o + t) + c) - M c"""
    R = [[1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0]]
    if applied:
        cx, sx, cy, sy, cz, sz = (fn(theta[a]) for a in range(3) for fn in (math.cos, math.sin))
        Rx = [[1.0, 0.0, 0.0], [0.0, cx, -sx], [0.0, sx, cx]]
        Ry = [[cy, 0.0, sy], [0.0, 1.0, 0.0], [-sy, 0.0, cy]]
        Rz = [[cz, -sz, 0.0], [sz, cz, 0.0], [0.0, 0.0, 1.0]]
        R = mat3(Rz, mat3(Ry, Rx))
    half = [(s - 1) / 2.0 for s in roi]
    f = [-1.0 if (flips >> a) & 1 else 1.0 for a in range(3)]
    out = []
    for a in range(3):
        M = [R[a][q] * (f[q] / zoom[q]) for q in range(3)]
        through = (M[0] * half[0] + M[1] * half[1]) + M[2] * half[2]
        out += [*M, ((o[a] + t[a]) + half[a]) - through]
    return out


def params_ref(B, step, in_size, roi, rotate=(0, 0, 0), zoom=(1, 1), isotropic=True, translate=(0, 0, 0), prob=1.0, flip_prob=(0, 0, 0),
               scale=(1, 1), shift=(0, 0), seed=0, rank=0):
    """int32 [B, 16] and, beside it, the twelve doubles of every row before their rounding to fp32 (float64 [B, 12])"""
    rows, exact = torch.zeros(B, COLS, dtype=torch.int32), torch.zeros(B, 12, dtype=torch.float64)
    for b in range(B):
        h = lambda d: draw(seed, rank, step, b, d)
        o = [A.below(h(a), in_size[a] - roi[a] + 1) for a in range(3)]
        flips = sum(1 << a for a in range(3) if (h(3 + a) >> 48) < int(float(flip_prob[a]) * 65536.0))
        applied = (h(6) >> 48) < int(float(prob) * 65536.0)
        theta, z, t = (0.0,) * 3, (1.0,) * 3, (0.0,) * 3
        if applied:
            theta = [(2.0 * real(h(7 + a)) - 1.0) * float(rotate[a]) * (math.pi / 180.0) for a in range(3)]
            z = [float(zoom[0]) + (float(zoom[1]) - float(zoom[0])) * real(h(10 if isotropic else 10 + a)) for a in range(3)]
            t = [(2.0 * real(h(13 + a)) - 1.0) * float(translate[a]) for a in range(3)]
        m = map_rows(roi, o, flips, theta, z, t, applied)
        exact[b] = torch.tensor(m, dtype=torch.float64)
        rows[b, :12] = torch.tensor([f32_bits(v) for v in m], dtype=torch.int32)
        rows[b, 12] = A.between(h(16), *scale).view(torch.int32)
        rows[b, 13] = A.between(h(17), *shift).view(torch.int32)
        rows[b, 14] = flips | (8 if applied else 0)
    return rows, exact


def table_of(maps, intensity=(ONE, ZERO)):
    """hand-written rows: `maps` a list of twelve Python floats each -> int32 [len, 16]"""
    return torch.tensor([[*(f32_bits(v) for v in m), *intensity, 0, 0] for m in maps], dtype=torch.int32)


def integer_map(roi, offset, flips):
    """the map of nv_augment_apply's row {ox, oy, oz, flips}: s_a = o_a + (flip ? S_a - 1 - i_a : i_a)"""
    m = []
    for a in range(3):
        f = (flips >> a) & 1
        m += [(-1.0 if f else 1.0) if q == a else 0.0 for q in range(3)] + [float(offset[a] + (roi[a] - 1 if f else 0))]
    return m


def augment_rows(maps_offsets_flips, intensity=(ONE, ZERO)):
    """the [n, 8] rows of nv_augment_apply for (offset, flips) pairs"""
    return torch.tensor([[*o, f, *intensity, 0, 0] for o, f in maps_offsets_flips], dtype=torch.int32)


def _sel(cond, a, b):
    """where(cond, a, b) that moves fp32 values as int32 patterns (NaN payloads, -0.0)"""
    if a.dtype == torch.float32:
        return torch.where(cond, a.contiguous().view(torch.int32), b.contiguous().view(torch.int32)).view(torch.float32)
    return torch.where(cond, a, b)


def apply_ref(x, table, roi, fill=0.0, dtype=torch.float32, lerp_fused=False, order="zyx", incremental=False):
    """x fp32 [B, X, Y, Z] or [B, X, Y, Z, T] (CPU), table int32 [B, 16] -> [B, Sx, Sy, Sz(, T)] of `dtype`, in the order the header spells
    out.  dtype=torch.float64: the same statements in double (the fp32 table entries and voxels widened).
    The last three arguments are WRONG on purpose, one at a time, for the tests that show the bit gate has teeth: a lerp whose product
    and sum are fused, a lerp order other than z, y, x, and a coordinate advanced along k by adding M_a2 instead of being formed from k."""
    four_d = x.dim() == 5
    v = (x if four_d else x.unsqueeze(-1)).to(dtype)
    B, T = v.shape[0], v.shape[-1]
    size = v.shape[1:4]
    out = torch.empty(B, *roi, T, dtype=dtype)
    fill_t = torch.tensor(fill, dtype=torch.float32).to(dtype)
    i, j, k = (torch.arange(roi[a], dtype=dtype).view([-1 if q == a else 1 for q in range(3)]) for a in range(3))
    for b in range(B):
        m = table[b, :12].view(torch.float32).to(dtype).tolist()
        mt = [torch.tensor(c, dtype=dtype) for c in m]                               # 0-dim tensors: every product and sum is rounded to dtype
        axes = []
        for a in range(3):
            M0, M1, M2, m3 = mt[4 * a:4 * a + 4]
            if incremental:
                steps = torch.cumsum(torch.cat([torch.zeros(1, dtype=dtype), M2.expand(roi[2] - 1)]), 0).view(1, 1, -1)      # 0, M2, M2 + M2, ...
                s = ((M0 * i + M1 * j) + m3) + steps
            else:
                s = ((M0 * i + M1 * j) + M2 * k) + m3
            s = s.expand(*roi).contiguous()
            fl = torch.floor(s)
            w = s - fl
            ok = (s >= -1.0) & (s < float(size[a]))
            lo = torch.where(ok, fl, torch.full_like(fl, -1.0)).to(torch.int64)
            axes.append(dict(w=w, use_hi=w != 0.0, lo=lo, in_lo=ok & (lo >= 0), in_hi=ok & (lo + 1 < size[a]), n=size[a]))
        any_in = torch.ones(roi, dtype=torch.bool)
        for ax in axes:
            any_in &= ax["in_lo"] | (ax["use_hi"] & ax["in_hi"])
        corners = {}
        for d in itertools.product((0, 1), repeat=3):
            inside = torch.ones(roi, dtype=torch.bool)
            idx = []
            for ax, up in zip(axes, d):
                inside &= ax["in_hi"] if up else ax["in_lo"]
                idx.append((ax["lo"] + up).clamp(0, ax["n"] - 1))
            got = v[b][idx[0], idx[1], idx[2]]                                           # [Sx, Sy, Sz, T]
            corners[d] = _sel(inside[..., None].expand_as(got), got, fill_t.expand_as(got))

        def lerp(lo_v, hi_v, ax):
            w = ax["w"][..., None]
            if lerp_fused:                                                           # (b - a) rounded, then ONE rounding of a + d w
                both = (lo_v.double() + (hi_v - lo_v).double() * w.double()).to(dtype)
            else:
                both = lo_v + ((hi_v - lo_v) * w)
            return _sel(ax["use_hi"][..., None].expand_as(lo_v), both, lo_v)
        level = corners
        for name in order:                                                           # "zyx": along z first, then y, then x
            a = "xyz".index(name)
            keys = sorted({tuple(None if q == a else c for q, c in enumerate(d)) for d in level})
            level = {key: lerp(level[tuple(0 if q == a else c for q, c in enumerate(key))], level[tuple(1 if q == a else c for q, c in enumerate(key))],
                               axes[a]) for key in keys}
        (value,) = level.values()
        scale, shift = (torch.tensor(wd, dtype=torch.int32).view(torch.float32).to(dtype) for wd in table[b, 12:14].tolist())
        if not (scale.item() == 1.0 and shift.item() == 0.0):
            value = (value * scale) + shift
        out[b] = _sel(any_in[..., None].expand_as(value), value, fill_t.expand_as(value))
    return out if four_d else out.squeeze(-1)


def bound(x, table, roi, fill):
    """The first-order bound on |fp32 restatement - float64 restatement| per cell, float64 [B, Sx, Sy, Sz]: 2^-24 (4 R A + 8 V) with
    A = sum_a (|M_a0| i + |M_a1| j + |M_a2| k + |m_a3|), R the range and V the largest magnitude of the volume with `fill`.  Each
    coordinate carries at most four roundings of numbers no larger than A_a, the value moves by at most R per voxel of coordinate error
    along each axis, and the three lerps and the fraction add at most eight roundings of numbers no larger than V."""
    vals = torch.cat([x.flatten().double(), torch.tensor([fill], dtype=torch.float64)])
    R, V = (vals.max() - vals.min()).item(), vals.abs().max().item()
    i, j, k = (torch.arange(roi[a], dtype=torch.float64).view([-1 if q == a else 1 for q in range(3)]) for a in range(3))
    out = []
    for b in range(table.shape[0]):
        m = table[b, :12].view(torch.float32).double().abs().tolist()
        Acc = sum(m[4 * a] * i + m[4 * a + 1] * j + m[4 * a + 2] * k + m[4 * a + 3] for a in range(3))
        out.append(2.0 ** -24 * (4.0 * R * Acc + 8.0 * V))
    return torch.stack(out)


# ---------------------------------------------------------------------- the inputs the GPU bit gate runs (and the CPU teeth tests with it)
IN = (20, 19, 18)


def volume(B=3, T=None, seed=3):
    """[B, 20, 19, 18(, T)] of normal values"""
    g = torch.Generator().manual_seed(seed)
    return torch.randn((B, *IN) if T is None else (B, *IN, T), generator=g)


def rotation_map(roi, degrees, zoom=(1.0, 1.0, 1.0), t=(0.0, 0.0, 0.0), offset=None, flips=0):
    offset = [(n - s) // 2 for n, s in zip(IN, roi)] if offset is None else offset
    return map_rows(roi, offset, flips, [math.radians(d) for d in degrees], zoom, t)


def hand_tables(roi):
    """{name: list of maps (twelve floats each)}, every list a multiple of three rows long (B = 3)"""
    hi = [n - s for n, s in zip(IN, roi)]
    ident = integer_map(roi, (0, 0, 0), 0)
    centre = [h // 2 for h in hi]
    half = [v + (0.5 if q % 4 == 3 else 0.0) for q, v in enumerate(integer_map(roi, centre, 0))]
    quarter = []
    for a, b in ((1, 2), (0, 2), (0, 1)):                    # a quarter turn in the plane of axes (a, b) about the window's centre, by hand
        for sign in (1.0, -1.0):
            m = [0.0] * 12
            c = [(s - 1) / 2.0 for s in roi]
            rot = [[1.0 if r == q else 0.0 for q in range(3)] for r in range(3)]
            rot[a][a], rot[b][b], rot[a][b], rot[b][a] = 0.0, 0.0, -sign, sign
            for r in range(3):
                m[4 * r:4 * r + 3] = rot[r]
                m[4 * r + 3] = float(math.floor(centre[r] + c[r] - sum(rot[r][q] * c[q] for q in range(3))))     # (floor: an integer map for a window that is no cube, too)
            quarter.append(m)
    faces = [integer_map(roi, o, f) for o, f in (((-3, 1, 1), 0), ((hi[0] + 2, 0, 2), 4), ((1, -5, 0), 7), ((2, hi[1] + 4, 1), 1), ((0, 1, -1), 2),
                                                 ((1, 2, hi[2] + 6), 4))]
    faces += [rotation_map(roi, (4, -3, 5), offset=o) for o in ((-4, 1, 1), (hi[0] + 4, 0, 1), (1, -4, 0), (1, hi[1] + 4, 0), (0, 1, -4), (1, 0, hi[2] + 4))]
    outside = [integer_map(roi, (-roi[0], 0, 0), 0), integer_map(roi, (1, IN[1], 0), 3), rotation_map(roi, (10, 10, 10), offset=(0, 0, IN[2] + 12))]
    bad = []
    for q, value in ((0, math.nan), (3, math.inf), (5, -math.inf), (11, 1e30), (7, -1e30), (10, math.nan)):
        m = list(rotation_map(roi, (3, 3, 3)))
        m[q] = value
        bad.append(m)
    return {
        "identity": [ident, integer_map(roi, hi, 7), integer_map(roi, centre, 5)],
        "half voxel": [half, [v + (0.5 if q == 11 else 0.0) for q, v in enumerate(integer_map(roi, centre, 0))], half],
        "rotation": [rotation_map(roi, (10, -9, 11)), rotation_map(roi, (-10, 10, 10), t=(0.3, -1.7, 2.2)), rotation_map(roi, (8, 11, -10), flips=5)],
        "zoom": [rotation_map(roi, (0, 0, 0), zoom=(0.5,) * 3), rotation_map(roi, (0, 0, 0), zoom=(2.0,) * 3), rotation_map(roi, (5, 0, 0), zoom=(0.5, 2.0, 1.25))],
        "faces": faces,
        "outside": outside,
        "quarter turns": quarter,
        "non-finite": bad,
    }
