"""CPU checks of the perturbation attribution (no GPU): the C-ABI pieces the feature adds within revision 8 (nv_token_ranks, nv_mask_patches,
nv_class_scores, nv_curve_auc, nv_occlusion_gather), and the CPU restatements that the GPU tests (tests/test_perturbation_gpu.py) compare
the kernels with bit for bit, pinned to the oracle:

  ranks_ref     the inverse of torch.sort(descending=True, stable=True).indices; equal to the counting rule of the header, evaluated directly;
  mask_ref      the select of nv_mask_patches with the token of every voxel formed by the header's rule; for EVERY single token t, masking t in a
                random volume changes exactly row t of oracle.ref_cpu.patchify(fmri_to_video(x)) - every element of it - and no other row,
                at (27, 9), (32, 8) and the rectangular (8, 12, 16) / (4, 6, 8); cubic token indices also equal oracle.ref_cpu.patch_index_map;
  step rule     perturbation_step_bounds: m_0 = 0, m_steps = N, never decreasing;
  refusals      every argument error of perturbation_curves / occlusion_sensitivity is raised without a device.
"""
import ctypes

import numpy as np
import pytest
import torch

import weights as W
from oracle import ref_cpu

GEOMETRIES = [((27,) * 3, (9,) * 3), ((32,) * 3, (8,) * 3), ((8, 12, 16), (4, 6, 8))]
MICRO_SIZE = dict(TRAINING_VIT_DIM=128, TRAINING_VIT_DEPTH=2, TRAINING_VIT_HEADS=2, TRAINING_VIT_MLP_DIM=256)


def ranks_ref(maps):
    """[B, N] fp32 -> int32 [B, N]: position of every token in the stable descending sort of its volume's map"""
    order = torch.sort(maps, dim=1, descending=True, stable=True).indices
    ranks = torch.empty_like(order)
    ranks.scatter_(1, order, torch.arange(maps.shape[1]).expand_as(order))
    return ranks.to(torch.int32)


def ranks_by_counting(maps):
    """the header's rule, evaluated directly: #{ j : m_j > m_t or (m_j == m_t and j < t) }"""
    m_j, m_t = maps[:, :, None], maps[:, None, :]
    idx = torch.arange(maps.shape[1])
    before = idx[:, None] < idx[None, :]
    return ((m_j > m_t) | ((m_j == m_t) & before)).sum(dim=1).to(torch.int32)


def token_of_voxel(size, patch):
    """int64 [S0, S1, S2]: t = (i2 / p2) G0 G1 + (i0 / p0) G1 + i1 / p1"""
    G0, G1 = size[0] // patch[0], size[1] // patch[1]
    i0, i1, i2 = torch.meshgrid(*(torch.arange(s) for s in size), indexing="ij")
    return (i2 // patch[2]) * G0 * G1 + (i0 // patch[0]) * G1 + i1 // patch[1]


def mask_ref(x, labels, jobs, patch, baseline=0.0, out=None):
    """CPU restatement of nv_mask_patches: x [B, S0, S1, S2] fp32, labels [B, N] int, jobs [J, 3] int -> [J, S0, S1, S2]; moves bit patterns.
    `out`: the pre-filled result (a job with b outside [0, B) leaves its slot as it is)"""
    B, size = x.shape[0], tuple(x.shape[1:])
    patch = (patch,) * 3 if isinstance(patch, int) else tuple(patch)
    token = token_of_voxel(size, patch)
    out = torch.zeros((jobs.shape[0],) + size) if out is None else out.clone()
    for j, (b, lo, hi) in enumerate(jobs.tolist()):
        if not 0 <= b < B:
            continue
        if torch.is_tensor(baseline):
            base = baseline[b if baseline.shape[0] == B else 0]
        else:
            base = torch.full(size, float(baseline))
        lab = labels[b].long()[token]
        out[j] = torch.where((lab >= lo) & (lab < hi), base.view(torch.int32), x[b].view(torch.int32)).view(torch.float32)
    return out


def test_header_declares_and_library_exports_the_new_entry_points():
    from neurovit_amd import _cabi
    names = ("nv_token_ranks", "nv_mask_patches", "nv_mask_patches_set_group", "nv_class_scores", "nv_curve_auc", "nv_occlusion_gather")
    dll = ctypes.CDLL(_cabi.LIB_PATH)
    for name in names:
        assert name in _cabi.lib.protos, name            # declared in the header
        assert getattr(dll, name) is not None, name      # exported by the library
    assert _cabi.ABI_VERSION == 8 and _cabi.lib.nv_abi_version() == 8          # new symbols only: the revision stays
    assert _cabi.lib.protos["nv_mask_patches"][1][7] is ctypes.c_float and _cabi.lib.protos["nv_mask_patches"][1][9] is ctypes.c_long
    header = open(_cabi.HEADER).read()
    assert "NV_SCORE_PROB 0" in header and "NV_SCORE_LOGIT 1" in header


def test_entry_points_check_their_arguments_without_a_gpu():
    from neurovit_amd import _cabi
    from neurovit_amd._cabi import lib

    def i3(*v):
        arr = (ctypes.c_int * 3)(*v)
        return arr, ctypes.cast(arr, ctypes.c_void_p)
    fake = 4096                                            # a non-null, 16-byte aligned address nothing dereferences: the checks come first
    _a, s32 = i3(32, 32, 32)
    _b, p8 = i3(8, 8, 8)
    _c, p5 = i3(8, 5, 8)
    _d, p1 = i3(1, 1, 1)
    assert lib.nv_token_ranks(None, 1, 8, fake, None) == -1
    assert lib.nv_token_ranks(fake, 1, 4097, fake, None) == -1 and "4096" in _cabi.last_error()
    assert lib.nv_token_ranks(fake, 0, 8, fake, None) == -1
    assert lib.nv_mask_patches(fake, 1, s32, p8, fake, fake, 1, 0.0, None, 0, None, None) == -1
    assert lib.nv_mask_patches(fake, 1, s32, p5, fake, fake, 1, 0.0, None, 0, fake, None) == -1 and "whole number" in _cabi.last_error()
    assert lib.nv_mask_patches(fake, 1, s32, p1, fake, fake, 1, 0.0, None, 0, fake, None) == -1 and "4096" in _cabi.last_error()
    assert lib.nv_mask_patches(fake, 1, s32, p8, fake, fake, 0, 0.0, None, 0, fake, None) == -1
    assert lib.nv_mask_patches(fake, 1, s32, p8, fake, fake, 1, 0.0, None, 0, fake + 4, None) == -1 and "16-byte" in _cabi.last_error()
    assert lib.nv_mask_patches(fake, 2, s32, p8, fake, fake, 1, 0.0, fake, 5, fake, None) == -1 and "stride" in _cabi.last_error()
    assert lib.nv_mask_patches_set_group(0) == -1 and lib.nv_mask_patches_set_group(17) == -1 and lib.nv_mask_patches_set_group(4) == 0
    assert lib.nv_class_scores(fake, 4, 2, fake, fake, 2, 2, fake, None) == -1 and "kind" in _cabi.last_error()
    assert lib.nv_class_scores(fake, 4, 0, fake, fake, 2, 0, fake, None) == -1
    assert lib.nv_curve_auc(fake, 2, 1, 1, fake, None) == -1
    assert lib.nv_curve_auc(fake, 2, 6, 5, fake, None) == -1
    assert lib.nv_occlusion_gather(fake, fake, None, 2, 8, 8, fake, None) == -1


def rank_maps(B, N, seed):
    """the maps of the GPU test: {name: [B, N] fp32}"""
    g = torch.Generator().manual_seed(seed)
    relu = torch.relu(torch.randn(B, N, generator=g))
    zeros = torch.zeros(B, N)
    zeros[:, ::2] = -0.0
    zeros[:, ::3] = torch.randn(B, (N + 2) // 3, generator=g).clamp_min(0.0)
    ramp = torch.arange(N, dtype=torch.float32).expand(B, N) * 0.37 - 3.0
    dense = torch.rand(B, N, generator=g)
    cut = torch.quantile(dense.double(), 0.95, dim=1, keepdim=True).float()
    return {"relu": relu, "equal": torch.full((B, N), 0.25), "signed zeros": zeros, "ascending": ramp.contiguous(), "descending": (-ramp).contiguous(),
            "cut at 5 %": torch.where(dense >= cut, dense, torch.zeros_like(dense))}


@pytest.mark.parametrize("N", [8, 27, 125, 1000])
def test_ranks_ref_is_the_counting_rule(N):
    for name, maps in rank_maps(2, N, 3 + N).items():
        got = ranks_ref(maps)
        assert torch.equal(got, ranks_by_counting(maps)), (name, N)
        assert torch.equal(torch.sort(got.long(), dim=1).values, torch.arange(N).expand(2, N)), name          # a permutation
    signed = rank_maps(2, N, 3 + N)["signed zeros"]
    assert bool((signed.view(torch.int32) == -2 ** 31).any())                                             # -0.0 is really there


@pytest.mark.parametrize("size,patch", GEOMETRIES, ids=["27p9", "32p8", "rect"])
def test_mask_ref_changes_exactly_one_row_of_the_oracle_patchify(size, patch):
    g = torch.Generator().manual_seed(sum(size))
    x = torch.randn((2,) + size, generator=g)
    assert not bool((x == 0).any())
    N = (size[0] // patch[0]) * (size[1] // patch[1]) * (size[2] // patch[2])
    labels = torch.arange(N, dtype=torch.int32).expand(2, N)
    jobs = torch.tensor([[1, t, t + 1] for t in range(N)], dtype=torch.int32)
    masked = mask_ref(x, labels, jobs, patch, baseline=0.0)                       # [N, S0, S1, S2]: volume 1 with token t zeroed
    rows = ref_cpu.patchify(ref_cpu.fmri_to_video(x[1:2]), patch[0], patch[1], patch[2])[0]          # (p1, p2, pf) = patch edges along (H, W, D)
    assert rows.shape[0] == N
    got = ref_cpu.patchify(ref_cpu.fmri_to_video(masked), patch[0], patch[1], patch[2])
    for t in range(N):
        changed = got[t] != rows
        assert bool(changed[t].all()) and int(changed.sum()) == rows.shape[1], (size, t)
        assert float(got[t, t].abs().max()) == 0.0
    if len(set(size)) == 1:                                                        # the integer restatement of the same contract
        idx = torch.from_numpy(ref_cpu.patch_index_map(size[0], patch[0]))
        token = token_of_voxel(size, patch).flatten()
        for t in range(N):
            assert bool((token[idx[t]] == t).all())


@pytest.mark.parametrize("N", [8, 27, 125, 1000, 4096])
def test_step_rule(N):
    from neurovit_amd.NeuroEncoder import perturbation_step_bounds
    for steps in (1, 7, 20, N, 2 * N):
        m = perturbation_step_bounds(N, steps)
        assert m.dtype == torch.int64 and m.shape == (steps + 1,)
        assert int(m[0]) == 0 and int(m[-1]) == N and bool((m[1:] >= m[:-1]).all()), (N, steps)
        want = np.floor(np.arange(steps + 1, dtype=np.float64) * N / steps + 0.5).astype(np.int64)     # k N / steps rounded half up (exact in double)
        assert np.array_equal(m.numpy(), want), (N, steps)
        if steps == N:
            assert torch.equal(m, torch.arange(N + 1))


def test_argument_errors_without_a_device(tmp_path):
    from neurovit_amd.NeuroEncoder import NeuroEncoder
    S = 16
    model = NeuroEncoder(W.neuro_config(S, 8, **MICRO_SIZE))
    x, maps = torch.zeros(2, S, S, S), torch.zeros(2, 8)
    with pytest.raises(ValueError, match="mode"):
        model.perturbation_curves(x, maps, mode="removal")
    with pytest.raises(ValueError, match="score"):
        model.perturbation_curves(x, maps, score="margin")
    with pytest.raises(ValueError, match="score"):
        model.occlusion_sensitivity(x, score="margin")
    for steps in (0, -3, 2.5):
        with pytest.raises(ValueError, match="steps"):
            model.perturbation_curves(x, maps, steps=steps)
    for window in (0, -1, 1.5):
        with pytest.raises(ValueError, match="window"):
            model.occlusion_sensitivity(x, window=window)
    for wrong in (torch.zeros(2, 9), torch.zeros(3, 8), torch.zeros(2, 2, 2, 2)):
        with pytest.raises(ValueError, match="token_maps"):
            model.perturbation_curves(x, wrong)
    for wrong in (torch.zeros(3, S, S, S), torch.zeros(S, S, S), torch.zeros(1, S, S, 8)):
        with pytest.raises(ValueError, match="baseline"):
            model.perturbation_curves(x, maps, baseline=wrong)
        with pytest.raises(ValueError, match="baseline"):
            model.occlusion_sensitivity(x, baseline=wrong)
    with pytest.raises(ValueError, match="chunk"):
        model.perturbation_curves(x, maps, chunk=0)
    with pytest.raises(ValueError, match="x must be"):
        model.occlusion_sensitivity(torch.zeros(2, S, S, 8))
    with pytest.raises(ValueError, match="method"):
        model.attribution_volumes(x, method="lime")
    torch.save(model.state_dict(), tmp_path / "c.pth")
    four_d = NeuroEncoder(W.neuro_config(S, 8, dim=4, GLOBAL_BASE_PATH=str(tmp_path), BEST_MODEL_PATH="c.pth", **MICRO_SIZE))
    with pytest.raises(NotImplementedError, match="3D model only"):
        four_d.perturbation_curves(x, maps)
    with pytest.raises(NotImplementedError, match="3D model only"):
        four_d.occlusion_sensitivity(x)
