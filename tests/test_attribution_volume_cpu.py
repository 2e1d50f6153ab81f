"""CPU checks of the batched attribution volumes (no GPU): the C-ABI pieces the feature adds within revision 8
(nv_gradcam_reduce_per_volume, nv_token_map_to_volume and their workspace queries), and the CPU restatement that the GPU tests
(tests/test_attribution_volume_gpu.py) measure the kernels against, pinned to the shipped single-volume code:

  restatement   per volume: the cut by the quantile rule of the header (order statistics, double arithmetic, rounded to fp32), cells >= cut
                kept, F.interpolate(trilinear, align_corners=False) - must EQUAL NeuroEncoder._token_map_to_volume (torch.quantile) exactly,
                for G in {4, 5, 8, 10, 16}, keep in {5, 20, 37.5, 100}, on ReLU-shaped maps (about half exact zeros);
  index rule    the header's per-axis source index / lambda arithmetic in fp32, applied as three separable passes, against F.interpolate:
                <= 2e-6 absolute (the gate of the GPU tests; values are convex combinations of numbers in [0, 1]).
"""
import ctypes
import types

import numpy as np
import pytest
import torch
import torch.nn.functional as F

GRID_TO_SIZE = {4: 32, 5: 45, 8: 128, 10: 90, 16: 128}
KEEPS = (5, 20, 37.5, 100)
VOLUME_TOL = 2e-6


def relu_maps(B, N, seed):
    """[B, N] fp32: the ReLU of a normal draw - about half the cells are exact zeros, as a Grad-CAM map's"""
    g = torch.Generator().manual_seed(seed)
    return torch.relu(torch.randn(B, N, generator=g, dtype=torch.float32))


def minmax_division(t):
    """the single-volume methods' normalisation (NeuroEncoder.get_attention_rollout): a true division, over the whole tensor"""
    return (t - t.min()) / (t.max() - t.min() + 1e-8)


def minmax_reciprocal(t):
    """the kernels' normalisation, per volume [B, N]: (v - min) * (1 / (max - min + 1e-8)) in fp32"""
    lo, hi = t.amin(dim=1, keepdim=True), t.amax(dim=1, keepdim=True)
    return (t - lo) * (1.0 / (hi - lo + 1e-8))


def quantile_cut(cells, keep_percent):
    """torch.quantile(cells.double(), 1 - keep / 100, interpolation='linear') restated on the order statistics; fp32 scalar tensor"""
    s = torch.sort(cells.flatten().double()).values
    N = s.numel()
    q = 1.0 - keep_percent / 100.0
    pos = q * (N - 1)
    lo = int(np.floor(pos))
    hi = min(lo + 1, N - 1)
    w = pos - lo
    a, e = s[lo], s[hi]
    cut = a + w * (e - a) if w < 0.5 else e - (e - a) * (1.0 - w)
    return cut.to(torch.float32)


def restate(norm_maps, grid, size, keep_percent):
    """CPU restatement of nv_token_map_to_volume behind its normalisation: norm_maps [B, N] fp32 -> (cuts [B], thresholded maps [B, N],
    volumes [B, S0, S1, S2]), every volume on its own"""
    cuts, sparse, vols = [], [], []
    for m in norm_maps:
        cut = quantile_cut(m, keep_percent)
        sp = torch.where(m >= cut, m, torch.zeros_like(m))
        cuts.append(cut)
        sparse.append(sp)
        vols.append(F.interpolate(sp.reshape(1, 1, *grid), size=tuple(size), mode='trilinear', align_corners=False)[0, 0])
    return torch.stack(cuts), torch.stack(sparse), torch.stack(vols)


def test_header_declares_and_library_exports_the_new_entry_points():
    from neurovit_amd import _cabi
    names = ("nv_gradcam_reduce_per_volume", "nv_gradcam_per_volume_workspace_bytes", "nv_token_map_to_volume",
             "nv_token_map_to_volume_workspace_bytes")
    dll = ctypes.CDLL(_cabi.LIB_PATH)
    for name in names:
        assert name in _cabi.lib.protos, name            # declared in the header
        assert getattr(dll, name) is not None, name      # exported by the library
    # new symbols only: the revision stays, the existing reduction keeps its argument list (the per-volume form takes the same one)
    assert _cabi.ABI_VERSION == 8 and _cabi.lib.nv_abi_version() == 8
    assert _cabi.lib.protos["nv_gradcam_reduce_per_volume"] == _cabi.lib.protos["nv_gradcam_reduce"]
    assert len(_cabi.lib.protos["nv_gradcam_reduce"][1]) == 10
    assert _cabi.lib.protos["nv_token_map_to_volume"][1][5] is ctypes.c_double


def test_argument_checks_without_a_gpu():
    from neurovit_amd import _cabi
    from neurovit_amd._cabi import lib

    def i3(*v):
        arr = (ctypes.c_int * 3)(*v)
        return arr, ctypes.cast(arr, ctypes.c_void_p)
    fake = 4096                                            # a non-null, 16-byte aligned address nothing dereferences: the checks come first
    _g, g8 = i3(8, 8, 8)
    _s, s128 = i3(128, 128, 128)
    assert lib.nv_token_map_to_volume_workspace_bytes(3, g8) == (2 * 3 * 512 + 3) * 4
    assert lib.nv_token_map_to_volume_workspace_bytes(0, g8) < 0
    assert lib.nv_gradcam_per_volume_workspace_bytes(0, 513) < 0 and lib.nv_gradcam_per_volume_workspace_bytes(3, 513) >= 16 + 3 * 8
    big = 1 << 30
    assert lib.nv_token_map_to_volume(None, 1, g8, s128, 1, 5.0, fake, fake, big, None) == -1
    assert lib.nv_token_map_to_volume(fake, 1, g8, s128, 1, 5.0, fake, fake, 8, None) == -1
    assert "workspace" in _cabi.last_error()
    assert lib.nv_token_map_to_volume(fake, 1, g8, s128, 1, 101.0, fake, fake, big, None) == -1
    assert "keep_percent" in _cabi.last_error()
    _l, large = i3(17, 16, 16)                             # one plane more than ViT3D-large's grid
    assert lib.nv_token_map_to_volume(fake, 1, large, s128, 1, 5.0, fake, fake, big, None) == -1
    assert "4096" in _cabi.last_error() and "17 x 16 x 16" in _cabi.last_error()
    assert lib.nv_gradcam_reduce_per_volume(fake, fake, 2, 513, 100, fake, None, fake, big, None) == -1     # d % 8
    assert lib.nv_gradcam_reduce_per_volume(fake, fake, 2, 513, 768, fake, None, fake, 8, None) == -1       # workspace too small


@pytest.mark.parametrize("keep", KEEPS)
@pytest.mark.parametrize("G", sorted(GRID_TO_SIZE))
def test_restatement_equals_the_single_volume_method(G, keep):
    from neurovit_amd.NeuroEncoder import NeuroEncoder
    S = GRID_TO_SIZE[G]
    stub = types.SimpleNamespace(config=dict(TRAINING_VIT_INPUT_SIZE=S, TRAINING_VIT_PATCH_SIZE=S // G, GRADCAM_THRESHOLD=keep))
    for seed in (1, 2):
        token_map = minmax_division(relu_maps(1, G ** 3, 100 * G + seed))
        assert 0.3 < float((token_map == 0).float().mean()) < 0.7
        want = NeuroEncoder._token_map_to_volume(stub, token_map)
        cuts, sparse, vols = restate(token_map, (G, G, G), (S, S, S), keep)
        shipped_cut = torch.quantile(token_map.double().flatten(), 1.0 - keep / 100.0).to(torch.float32)
        assert torch.equal(cuts[0], shipped_cut), (G, keep, float(cuts[0]), float(shipped_cut))
        assert want.shape == (S, S, S) and torch.equal(vols[0], want)
        if keep == 100:
            assert torch.equal(sparse[0], token_map[0])


def axis_matrix(G, S):
    """[S, G] fp32 taps of one axis by the header's rule: src = max((dst + 0.5) (G / S) - 0.5, 0), every step rounded to fp32"""
    f = np.float32
    scale = f(G) / f(S)
    W = np.zeros((S, G), dtype=np.float32)
    for dst in range(S):
        src = max(f(f(scale * f(f(dst) + f(0.5))) - f(0.5)), f(0))
        i0 = min(int(src), G - 1)
        i1 = min(i0 + 1, G - 1)
        l1 = f(src - f(i0))
        W[dst, i0] += f(1) - l1
        W[dst, i1] += l1
    return torch.from_numpy(W)


@pytest.mark.parametrize("grid,size", [((4,) * 3, (32,) * 3), ((10,) * 3, (90,) * 3), ((8,) * 3, (128,) * 3), ((16,) * 3, (128,) * 3),
                                       ((3,) * 3, (27,) * 3), ((4, 6, 5), (20, 36, 45))])
def test_index_rule_against_aten(grid, size):
    cells = minmax_division(relu_maps(1, grid[0] * grid[1] * grid[2], 7)).reshape(grid)
    want = F.interpolate(cells[None, None], size=size, mode='trilinear', align_corners=False)[0, 0]
    Wx, Wy, Wz = (axis_matrix(g, s) for g, s in zip(grid, size))
    got = torch.einsum("xa,abc->xbc", Wx, cells)
    got = torch.einsum("zc,xbc->xbz", Wz, got)
    got = torch.einsum("yb,xbz->xyz", Wy, got)
    err = float((got - want).abs().max())
    print(f"index rule {grid} -> {size}: max |err| {err:.2e}")
    assert err <= VOLUME_TOL
