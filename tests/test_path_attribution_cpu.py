"""CPU checks of the path attribution (no GPU): the C-ABI pieces the feature adds within revision 8 (nv_path_points, nv_class_score_grads,
nv_path_accumulate, nv_path_finish, nv_attr_token_sums), the quadrature tables, and the CPU restatements (tests/path_attribution_ref.py)
that the GPU tests (tests/test_path_attribution_gpu.py) compare the kernels and the method with:

  tables         every rule's float64 weights sum to 1 within 1e-12; the Gauss-Legendre nodes are leggauss mapped to [0, 1];
  polynomial     the restated method on f(x) = sum_i c_i x_i^3 (attributions c_i x_i^3 for a zero baseline): the midpoint rule misses by
                 1 / (4 m^2), Gauss-Legendre with m >= 2 is exact (the integrand has degree 2 <= 2 m - 1) within fp32 rounding;
  token sums     the restated pooling equals oracle.ref_cpu.patchify(...).sum(-1) on the [B, 1, D, H, W] view, bit for bit in float64;
  completeness   the restated method on the fp32 oracle: |delta| of Gauss-Legendre at 8 / 16 / 32 steps (the yardstick of the GPU gate);
  refusals       every argument error of path_quadrature / integrated_gradients is raised without a device.
"""
import ctypes

import numpy as np
import pytest
import torch

import path_attribution_ref as R
import weights as W
from conftest import rel_err
from oracle import ref_cpu

MICRO_SIZE = dict(TRAINING_VIT_DIM=128, TRAINING_VIT_DEPTH=2, TRAINING_VIT_HEADS=2, TRAINING_VIT_MLP_DIM=256)
NAMES = ("nv_path_points", "nv_class_score_grads", "nv_path_accumulate", "nv_path_finish", "nv_attr_token_sums")


def test_header_declares_and_library_exports_the_new_entry_points():
    from neurovit_amd import _cabi
    dll = ctypes.CDLL(_cabi.LIB_PATH)
    for name in NAMES:
        assert name in _cabi.lib.protos, name            # declared in the header
        assert getattr(dll, name) is not None, name      # exported by the library
    protos = _cabi.lib.protos
    assert protos["nv_path_points"][1][2] is ctypes.c_long and protos["nv_path_points"][1][7] is ctypes.c_float
    assert protos["nv_path_accumulate"][1][7] is ctypes.c_long and protos["nv_path_finish"][1][4] is ctypes.c_float


def test_entry_points_check_their_arguments_without_a_gpu():
    from neurovit_amd import _cabi
    from neurovit_amd._cabi import lib

    def i3(*v):
        arr = (ctypes.c_int * 3)(*v)
        return arr, ctypes.cast(arr, ctypes.c_void_p)
    fake = 4096                                            # a non-null, 16-byte aligned address nothing dereferences: the checks come first
    _a, s27 = i3(27, 27, 27)
    _b, p9 = i3(9, 9, 9)
    _c, p8 = i3(8, 8, 8)
    assert lib.nv_path_points(None, 1, 64, fake, 1, fake, 1, 0.0, None, 0, fake, None) == -1
    assert lib.nv_path_points(fake, 1, 0, fake, 1, fake, 1, 0.0, None, 0, fake, None) == -1
    assert lib.nv_path_points(fake, 1, 64, fake, 1, fake, 1, 0.0, None, 0, fake + 4, None) == -1 and "16-byte" in _cabi.last_error()
    assert lib.nv_path_points(fake, 2, 64, fake, 1, fake, 1, 0.0, fake, 5, fake, None) == -1 and "stride" in _cabi.last_error()
    assert lib.nv_path_points(fake, 2, 64, fake, 65535 * 8 + 1, fake, 1, 0.0, None, 0, fake, None) == -1 and "jobs" in _cabi.last_error()
    assert lib.nv_class_score_grads(fake, 4, 2, fake, fake, 2, 2, fake, None) == -1 and "kind" in _cabi.last_error()
    assert lib.nv_class_score_grads(fake, 4, 0, fake, fake, 2, 0, fake, None) == -1
    assert lib.nv_path_accumulate(fake, fake, 1025, fake, 4, fake, 2, 64, None) == -1 and "1024" in _cabi.last_error()
    assert lib.nv_path_accumulate(fake, fake, 4, fake, 4, fake + 8, 2, 64, None) == -1 and "16-byte" in _cabi.last_error()
    assert lib.nv_path_finish(fake, None, 2, 64, 0.0, None, 0, fake, None) == -1
    assert lib.nv_path_finish(fake, fake, 2, 64, 0.0, fake, 63, fake, None) == -1 and "stride" in _cabi.last_error()
    assert lib.nv_attr_token_sums(fake, 1, s27, p8, fake, None) == -1 and "whole number" in _cabi.last_error()
    assert lib.nv_attr_token_sums(fake, 0, s27, p9, fake, None) == -1


# ------------------------------------------------------------------ quadrature tables
def tables64(method, m):
    """the rules of path_quadrature's docstring, evaluated independently in float64"""
    if method == "riemann_middle":
        return (np.arange(m) + 0.5) / m, np.full(m, 1.0 / m)
    if method == "riemann_trapezoid":
        w = np.full(m, 1.0 / (m - 1))
        w[[0, -1]] /= 2
        return np.arange(m) / (m - 1), w
    nodes, w = np.polynomial.legendre.leggauss(m)
    return (nodes + 1) / 2, w / 2


@pytest.mark.parametrize("method", ["riemann_middle", "riemann_trapezoid", "gausslegendre"])
@pytest.mark.parametrize("m", [2, 7, 50])
def test_quadrature_tables(method, m):
    from neurovit_amd.NeuroEncoder import path_quadrature
    a64, w64 = tables64(method, m)
    assert abs(w64.sum() - 1.0) <= 1e-12
    alphas, weights = path_quadrature(method, m)
    assert alphas.dtype == weights.dtype == torch.float32 and alphas.shape == weights.shape == (m,)
    assert torch.equal(alphas, torch.from_numpy(a64).float()) and torch.equal(weights, torch.from_numpy(w64).float())
    assert abs(weights.double().sum().item() - 1.0) <= m * 2.0 ** -24          # every fp32 weight is within half an ulp of its float64 value
    assert (alphas >= 0).all() and (alphas <= 1).all() and (alphas[1:] > alphas[:-1]).all()
    if method == "gausslegendre":
        nodes, _ = np.polynomial.legendre.leggauss(m)
        assert torch.equal(alphas, torch.from_numpy(0.5 * (nodes + 1.0)).float())


def test_quadrature_refusals():
    from neurovit_amd.NeuroEncoder import path_quadrature
    for method, steps in (("simpson", 8), ("riemann_middle", 0), ("gausslegendre", -3), ("gausslegendre", 2.5), ("riemann_trapezoid", 1)):
        with pytest.raises(ValueError):
            path_quadrature(method, steps)
    assert path_quadrature("riemann_middle", 1)[0].tolist() == [0.5]


def polynomial_attributions(method, m):
    from neurovit_amd.NeuroEncoder import path_quadrature
    g = torch.Generator().manual_seed(3)
    x = torch.randn(2, 4, 5, generator=g)
    c = torch.randn(4, 5, generator=g)
    alphas, weights = path_quadrature(method, m)
    attr, delta, s_in, s_bl = R.integrated_gradients_ref(lambda v: (c * v ** 3).sum(dim=(1, 2))[:, None], x, torch.zeros(2, dtype=torch.long), alphas,
                                                         weights)
    return attr, c * x ** 3, delta, s_in, s_bl


def test_restated_method_on_a_closed_form_polynomial():
    # zero baseline: attr_i = x_i * sum_k w_k 3 c_i (alpha_k x_i)^2 = c_i x_i^3 * 3 sum_k w_k alpha_k^2; the midpoint rule gives
    # 3 sum_k w_k alpha_k^2 = 1 - 1 / (4 m^2) exactly, Gauss-Legendre with m >= 2 gives 1
    errs = {}
    for m in (4, 8):
        attr, exact, delta, s_in, s_bl = polynomial_attributions("riemann_middle", m)
        errs[m] = rel_err(attr, exact)
        assert abs(errs[m] - 1.0 / (4 * m * m)) <= 1e-6, (m, errs[m])
        assert torch.equal(s_bl, torch.zeros(2)) and rel_err(s_in, exact.sum(dim=(1, 2))) <= 1e-6
        assert rel_err(delta, -exact.double().sum(dim=(1, 2)) / (4 * m * m)) <= 1e-4        # the residual IS the quadrature error
    assert abs(errs[4] / errs[8] - 4.0) <= 1e-3                                             # O(1 / m^2)
    for m in (2, 3, 16):
        attr, exact, delta, _, _ = polynomial_attributions("gausslegendre", m)
        assert rel_err(attr, exact) <= 1e-6, m
    attr, exact, _, _, _ = polynomial_attributions("gausslegendre", 1)                     # one point: the midpoint rule, 1 - 1/4
    assert abs(rel_err(attr, exact) - 0.25) <= 1e-6


# ------------------------------------------------------------------ token sums
@pytest.mark.parametrize("S,p", [(16, 8), (27, 9)])
def test_token_sums_restatement_is_the_oracles_patchify(S, p):
    g = torch.Generator().manual_seed(S)
    attr = torch.randn(3, S, S, S, generator=g)
    rows = ref_cpu.patchify(ref_cpu.fmri_to_video(attr.double()), p, p, p)
    got = R.token_sums_ref(attr, p)
    assert got.dtype == torch.float64 and got.shape == (3, (S // p) ** 3, 2)
    assert torch.equal(got[..., 0], rows.sum(-1)) and torch.equal(got[..., 1], rows.abs().sum(-1))
    # and the header's rule, voxel by voxel: scatter every voxel into its token
    G = S // p
    i0, i1, i2 = torch.meshgrid(*(torch.arange(S),) * 3, indexing="ij")
    token = ((i2 // p) * G * G + (i0 // p) * G + i1 // p).reshape(-1)
    direct = torch.zeros(3, G ** 3, dtype=torch.float64).index_add_(1, token, attr.double().reshape(3, -1))
    assert (direct - got[..., 0]).abs().max().item() <= p ** 3 * 2.0 ** -53 * got[..., 1].max().item()


# ------------------------------------------------------------------ completeness on the fp32 oracle
def oracle_cfg(cfgdict):
    return ref_cpu.ViTCfg(**cfgdict)


def test_restated_method_completeness_on_the_fp32_oracle():
    """|delta| of the restated method on the fp32 oracle (W.MICRO, weights seed 51, input seed 52, class 1, zero baseline, Gauss-Legendre):
        8 steps 8.630e-01,  16 steps 7.062e-01,  32 steps 5.538e-02   (float64 sums of fp32 attributions; the logit difference is 8.772e-01)
    The residual is quadrature error and falls slowly: the patch LayerNorm makes the logits of alpha x nearly independent of alpha except
    close to alpha = 0, so the integrand is a narrow peak at the baseline end that few points resolve.  The GPU completeness gate
    (tests/test_path_attribution_gpu.py) holds the native |delta| against RATIO x the oracle's |delta| at the same rule + SLACK."""
    from neurovit_amd.NeuroEncoder import path_quadrature
    sd = W.make_tensors(W.vit_param_spec(**W.MICRO), 51)
    cfg = oracle_cfg(W.MICRO)
    video = ref_cpu.fmri_to_video(W.make_volume((1, 32, 32, 32), 52)).contiguous()
    cls = torch.tensor([1])
    deltas = {}
    for m in (8, 16, 32):
        alphas, weights = path_quadrature("gausslegendre", m)
        _, delta, s_in, s_bl = R.integrated_gradients_ref(lambda v: ref_cpu.vit_forward(sd, cfg, v), video, cls, alphas, weights)
        deltas[m] = abs(delta.item())
        print(f"fp32 oracle, gausslegendre {m} steps: |delta| {deltas[m]:.3e}  (score_input - score_baseline {(s_in - s_bl).item():.3e})")
    assert deltas[32] <= deltas[8], deltas


# ------------------------------------------------------------------ refusals, without a device
def test_integrated_gradients_refuses_bad_arguments_before_any_device_work(tmp_path):
    from neurovit_amd.NeuroEncoder import NeuroEncoder
    model = NeuroEncoder(W.neuro_config(32, 8, **MICRO_SIZE))
    x = torch.zeros(2, 32, 32, 32)
    for kwargs in (dict(method="simpson"), dict(steps=0), dict(steps=2.5), dict(chunk=0), dict(chunk=1.5), dict(score="margin"),
                   dict(baseline=torch.zeros(3, 32, 32, 32)), dict(method="riemann_trapezoid", steps=1)):
        with pytest.raises(ValueError):
            model.integrated_gradients(x, **kwargs)
    with pytest.raises(ValueError):
        model.integrated_gradients(torch.zeros(2, 16, 16, 16))
    with pytest.raises(ValueError, match="integrated_gradients"):
        model.attribution_volumes(x, method="saliency")
    torch.save(model.state_dict(), tmp_path / "c.pth")
    four_d = NeuroEncoder(W.neuro_config(32, 8, dim=4, GLOBAL_BASE_PATH=str(tmp_path), BEST_MODEL_PATH="c.pth", **MICRO_SIZE))
    with pytest.raises(NotImplementedError, match="3D model only"):
        four_d.integrated_gradients(x)
