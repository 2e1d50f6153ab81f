"""The inputs and guard buffers that tests/test_augment_gpu.py, tests/test_affine_gpu.py and tests/test_mix_gpu.py share: volumes with special
values, the three memory layouts of a source, the plane shapes that reach a second span, and an `out` between sentinels."""
import numpy as np
import torch

from augment_ref import bits


def special_volume(shape, seed, subnormals=False):
    """tests/test_perturbation_gpu.py's recipe: NaN (one with a payload), +-inf, -0.0 among normal values; subnormals: +-subnormals too"""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(shape, generator=g)
    flat = x.view(shape[0], -1)
    flat[:, 0::17] = float("nan")
    flat[:, 1::19] = float("inf")
    flat[:, 2::23] = float("-inf")
    flat[:, 3::29] = -0.0
    flat[:, 5::31] = torch.tensor([0x7fc01234], dtype=torch.int32).view(torch.float32)[0]       # NaNs with a payload
    if subnormals:
        flat[:, 7::37] = torch.tensor([0x00000123], dtype=torch.int32).view(torch.float32)[0]       # a subnormal
        flat[:, 9::41] = torch.tensor([-0x7FFFFFFF - 1 + 0x00400001], dtype=torch.int32).view(torch.float32)[0]     # a negative subnormal (0x80400001)
    return x


def layouts(host=None, subnormals=False):
    """The three layouts of a source.  Without `host`: (the dense host volume [3, 23, 21, 22] of special values, {name: d -> the same values
    in that layout, moved to the device by d}) - a sliced view, the dense copy, and x innermost.  With host [B, X, Y, Z(, T)]: {name: the
    same values on the device in that layout} - dense, a sliced view, and the base moved by one element."""
    if host is None:
        big = special_volume((3, 25, 24, 27), 23, subnormals)
        view = big[:, 1:24, 2:23, 3:25]                          # a sliced, non-contiguous view: rows of 22 floats at every alignment
        dense = view.contiguous()
        moved = view.permute(0, 3, 2, 1).contiguous().permute(0, 3, 2, 1)       # the same values with x innermost: no row is a run of memory
        assert not view.is_contiguous() and not moved.is_contiguous() and torch.equal(bits(moved), bits(dense))
        return dense, {"view": lambda d: d(big)[:, 1:24, 2:23, 3:25], "dense": lambda d: d(dense), "moved": lambda d: d(moved.permute(0, 3, 2, 1)).permute(0, 3, 2, 1)}
    pad = [(1, 2), (2, 1), (3, 4)]
    big = torch.zeros(host.shape[0], *(n + lo + hi for n, (lo, hi) in zip(host.shape[1:4], pad)), *host.shape[4:]).cuda()
    view = big[:, 1:1 + host.shape[1], 2:2 + host.shape[2], 3:3 + host.shape[3]]
    view.copy_(host)
    flat = torch.zeros(host.numel() + 1).cuda()
    moved = flat[1:].view(host.shape)                        # the base moved by one element: no source row starts a 16-byte group
    moved.copy_(host)
    assert not view.is_contiguous() and moved.data_ptr() % 16 == 4
    return {"dense": host.cuda(), "view": view, "moved": moved}


# A workgroup owns 4096 cells of an output plane.  The smallest planes that reach a second one: 65 x 67 = 4355 cells (4355 mod 4 = 3, so
# consecutive planes start at every 16-byte alignment; the second span is 259 cells from output row 61, column 9) and, for a series,
# 9 x 10 x 47 = 4230 cells (rows of 470; the second span is 134 cells from row 8, k = 7).
SPAN_SHAPES = {"3d": ((3, 5, 68, 70), (3, 65, 67)), "4d": ((3, 4, 12, 13, 47), (2, 9, 10))}


def sentinel_out(shape):
    """a dense `out` of that shape with 64 sentinel floats on both sides"""
    n = int(np.prod(shape))
    buf = torch.full((64 + n + 64,), 0x7FC0BEEF, dtype=torch.int32, device="cuda").view(torch.float32)
    return buf, buf[64:64 + n].view(shape)


def sentinels_intact(buf):
    return bool((bits(torch.cat([buf[:64], buf[-64:]]).cpu()) == 0x7FC0BEEF).all())
