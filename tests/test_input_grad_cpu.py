"""Gradient w.r.t. the input volume, host side (no GPU needed).

* the fp32 oracle's autograd reproduces the imported reference's input gradients (tests/golden/input_grad.npz, written by
  tests/golden/make_input_grad_golden.py) to 1e-5 - which makes the oracle the yardstick of the GPU tests in test_input_grad_gpu.py;
* the ctypes mirror of struct nv_vit_backward_opts has the header's fields and layout;
* nv_vit_backward_ex refuses malformed options before it queues anything.
"""
import ctypes
import re

import pytest
import torch

import weights as W
from conftest import rel_err
from oracle import ref_cpu

TOL = 1e-5
P729 = dict(W.MICRO, image_size=27, image_patch_size=9, frames=27, frame_patch_size=9)
CASES = {"micro": W.MICRO, "p729": P729, "rect": W.RECT}


def oracle_cfg(cfgdict):
    """ref_cpu.ViTCfg of a ViT constructor dict ((height, width) pairs as the reference takes them, vit_3d.py:80-81)"""
    v = dict(cfgdict)
    (H, Wd), (p1, p2) = (x if isinstance(x, tuple) else (x, x) for x in (v.pop("image_size"), v.pop("image_patch_size")))
    return ref_cpu.ViTCfg(image_size=H, image_patch_size=p1, image_width=Wd, patch_width=p2, **v)


@pytest.mark.parametrize("tag", sorted(CASES))
def test_oracle_input_grad_matches_reference(golden, tag):
    g = golden("input_grad.npz")
    cfgdict = CASES[tag]
    seed_w, seed_x = (int(v) for v in g[f"{tag}.seeds"])
    sd = W.make_tensors(W.vit_param_spec(**cfgdict), seed_w)
    video = W.make_volume(tuple(int(v) for v in g[f"{tag}.shape"]), seed_x).requires_grad_(True)
    logits = ref_cpu.vit_forward(sd, oracle_cfg(cfgdict), video)
    logits[:, 0].sum().backward()
    assert rel_err(logits, g[f"{tag}.logits"]) < TOL
    assert rel_err(video.grad, g[f"{tag}.grad"]) < TOL


def test_oracle_neuro3d_input_grad_matches_reference(golden):
    g = golden("input_grad.npz")
    B, S = int(g["neuro3d.shape"][0]), int(g["neuro3d.shape"][1])
    seed_w, seed_x = (int(v) for v in g["neuro3d.seeds"])
    config = W.neuro_config(S, 8)
    vc = dict(image_size=S, image_patch_size=8, frames=S, frame_patch_size=8, num_classes=2, dim=1024, depth=6, heads=8,
              mlp_dim=2048, channels=1, dim_head=64)
    sd = W.make_tensors(W.vit_param_spec(**vc), seed_w, prefix="volume_encoder.vit3d.")
    x = W.make_volume((B, S, S, S), seed_x).requires_grad_(True)      # [B, H, W, D]: the permute view's backward is autograd's
    logits = ref_cpu.neuro_forward(sd, config, x)
    logits[:, 0].sum().backward()
    assert rel_err(logits, g["neuro3d.logits"]) < TOL
    assert rel_err(x.grad, g["neuro3d.grad"]) < TOL


def test_backward_opts_struct_matches_header():
    from neurovit_amd import _cabi
    src = re.sub(r"/\*.*?\*/", " ", open(_cabi.HEADER).read(), flags=re.S)
    body = re.search(r"typedef struct nv_vit_backward_opts\s*\{(.*?)\}\s*nv_vit_backward_opts;", src, flags=re.S).group(1)
    decls = [d.strip() for d in body.split(";") if d.strip()]
    names = [re.search(r"(\w+)$", d).group(1) for d in decls]
    assert names == [f[0] for f in _cabi.BackwardOpts._fields_]
    # C types of the header's fields -> the ctypes a C compiler lays out the same way
    ctype = [ctypes.c_void_p if "*" in d else {"int": ctypes.c_int, "long": ctypes.c_long}[d.split()[0]] for d in decls]
    assert ctype == [f[1] for f in _cabi.BackwardOpts._fields_]
    assert ctypes.sizeof(_cabi.BackwardOpts) == 32
    assert [getattr(_cabi.BackwardOpts, n).offset for n in names] == [0, 8, 16, 24]


def test_backward_ex_rejects_bad_options_on_the_host():
    from neurovit_amd import engine
    from neurovit_amd._cabi import BackwardOpts, last_error, lib
    cfg = engine.make_config(**W.MICRO)
    B = 2
    dummy = ctypes.c_void_p(256)       # never dereferenced: every call below fails its argument checks first
    strides = (ctypes.c_long * 5)(32 ** 3, 32 ** 3, 1, 32 * 32, 32)
    ws_bytes = lib.nv_vit_workspace_bytes(ctypes.byref(cfg), B, 1)

    def call(opts, grads):
        return lib.nv_vit_backward_ex(ctypes.byref(cfg), B, dummy, strides, dummy, dummy, dummy, ws_bytes, dummy, grads, None, 0, 0,
                                      cfg.depth + 1, 0.0, 0.0, 0, None, None, 1, 0, ctypes.byref(opts))

    bad_size = BackwardOpts(ctypes.sizeof(BackwardOpts) - 4, None, None, 1)
    assert call(bad_size, dummy) != 0 and "struct_size" in last_error()
    no_strides = BackwardOpts(ctypes.sizeof(BackwardOpts), dummy.value, None, 1)
    assert call(no_strides, dummy) != 0 and "dvideo_strides5" in last_error()
    data_only_with_arena = BackwardOpts(ctypes.sizeof(BackwardOpts), None, None, 0)
    assert call(data_only_with_arena, dummy) != 0 and "data-only" in last_error()


def test_patch_ln_dx_rejects_bad_arguments_on_the_host():
    from neurovit_amd._cabi import last_error, lib
    dummy = ctypes.c_void_p(256)
    s = (ctypes.c_long * 5)(27 ** 3, 27 ** 3, 27 * 27, 27, 1)
    assert lib.nv_patch_ln_dx(dummy, s, 1, 1, 27, 27, 27, 9, 9, 9, dummy, 728, dummy, dummy, dummy, dummy, s, None) != 0
    assert "ldd" in last_error()
    assert lib.nv_patch_ln_dx(dummy, s, 1, 1, 27, 27, 27, 9, 9, 9, dummy, 736, dummy, dummy, dummy, None, s, None) != 0
    assert "null" in last_error()
    assert lib.nv_patch_ln_dx(dummy, s, 1, 1, 27, 27, 26, 9, 9, 9, dummy, 736, dummy, dummy, dummy, dummy, s, None) != 0
    assert "divisible" in last_error()


def test_oracle_input_grad_is_what_a_patch_layernorm_backward_gives():
    """The kernel's formula, dx = rstd (g - mean(g) - xhat mean(g xhat)) with g = dy gamma, scattered through the patch map, equals
    float64 autograd of F.layer_norm(patchify(video)) - the restatement test_input_grad_gpu.py holds nv_patch_ln_dx to."""
    torch.manual_seed(0)
    video = torch.randn(2, 2, 12, 16, 24, dtype=torch.float64)
    p1, p2, pf = 8, 4, 4
    P = 2 * p1 * p2 * pf
    gamma = 1 + 0.1 * torch.randn(P, dtype=torch.float64)
    dy = torch.randn(2, (12 // pf) * (16 // p1) * (24 // p2), P, dtype=torch.float64)
    v = video.clone().requires_grad_(True)
    y = torch.nn.functional.layer_norm(ref_cpu.patchify(v, p1, p2, pf), (P,), gamma, None, 1e-5)
    (want,) = torch.autograd.grad(y, v, dy)
    x = ref_cpu.patchify(video, p1, p2, pf)
    mean = x.mean(-1, keepdim=True)
    rstd = 1 / torch.sqrt(((x - mean) ** 2).mean(-1, keepdim=True) + 1e-5)
    xh, g = (x - mean) * rstd, dy * gamma
    dx = rstd * (g - g.mean(-1, keepdim=True) - xh * (g * xh).mean(-1, keepdim=True))
    got = torch.zeros_like(video)
    idx = ref_cpu.patchify(torch.arange(video.numel(), dtype=torch.float64).reshape(video.shape), p1, p2, pf).long()
    got.view(-1)[idx.reshape(-1)] = dx.reshape(-1)
    assert rel_err(got, want) < 1e-12
