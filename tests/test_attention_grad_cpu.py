"""CPU checks of the attention-gradient export (no GPU): the reference-made fixture tests/golden/attention_grad.npz against the oracle
identity the GPU tests rest on (dP_l = dOut_l V^T), the relevance rule in its two forms, and the C-ABI pieces the feature adds within
revision 8 (nv_vit_attn_grad_export, nv_attn_grad, nv_attn_relevance, nv_vit_backward_attn)."""
import ctypes
import subprocess

import numpy as np
import pytest
import torch

import weights as W
from conftest import rel_l2
from oracle import ref_cpu

P729 = dict(W.MICRO, image_size=27, image_patch_size=9, frames=27, frame_patch_size=9)
VIT_CASES = [("micro", W.MICRO), ("p729", P729), ("rect", W.RECT), ("noproj", W.NOPROJ), ("mean", dict(W.MICRO, pool="mean"))]
NEURO = dict(image_size=24, image_patch_size=8, frames=24, frame_patch_size=8, num_classes=2, dim=1024, depth=6, heads=8, mlp_dim=2048,
             channels=1, dim_head=64, pool="cls")
ALL_CASES = VIT_CASES + [("neuro3d", NEURO)]


def oracle_cfg(cfgdict):
    v = dict(cfgdict)
    (H, Wd), (p1, p2) = (x if isinstance(x, tuple) else (x, x) for x in (v.pop("image_size"), v.pop("image_patch_size")))
    return ref_cpu.ViTCfg(image_size=H, image_patch_size=p1, image_width=Wd, patch_width=p2, **v)


def oracle_attention_grads(cfgdict, sd, video, target=None, emulate=False):
    """(logits, target, [dP_l]) of the oracle: dP_l = dOut_l V^T, dOut_l = the gradient of the target logits w.r.t. the block's attention
    output ('b n (h d) -> b h n d'; rounded to the operand format when emulating, as the kernel reads it), V the block's `v` tap."""
    taps = {}
    v = video.clone().requires_grad_(True)                 # so that every tap carries a graph
    logits = ref_cpu.vit_forward(sd, oracle_cfg(cfgdict), v, emulate_bf16=emulate, taps=taps)
    if target is None:
        target = logits.argmax(dim=1)
    outs = [taps[f"transformer.layers.{l}.0.attn.out"] for l in range(cfgdict["depth"])]
    grads = torch.autograd.grad(logits.gather(1, target[:, None]).sum(), outs)
    B, n, h, dh = video.shape[0], outs[0].shape[1], cfgdict["heads"], cfgdict["dim_head"]
    dP = []
    for l, g in enumerate(grads):
        dO = (ref_cpu._r(g) if emulate else g).reshape(B, n, h, dh).permute(0, 2, 1, 3)
        dP.append(dO @ taps[f"transformer.layers.{l}.0.v"].detach().transpose(-1, -2))
    return logits.detach(), target, dP


def relevance_rows(A, pool):
    """u <- u + u A_l from the last layer down (float64), every token"""
    B, n = A[0].shape[0], A[0].shape[-1]
    u = np.full((B, n), 1.0 / n) if pool == "mean" else np.tile(np.eye(n)[0], (B, 1))
    for a in A[::-1]:
        u = u + np.einsum("bi,bij->bj", u, a)
    return u


def layer_terms(g, tag, depth):
    return [np.maximum(g[f"{tag}.dP{l}"].astype(np.float64) * g[f"{tag}.P{l}"].astype(np.float64), 0.0).mean(axis=1) for l in range(depth)]


@pytest.mark.parametrize("tag,cfg", ALL_CASES, ids=[c[0] for c in ALL_CASES])
def test_fixture_equals_dout_vt_of_the_oracle(golden, tag, cfg):
    g = golden("attention_grad.npz")
    sw, sx = (int(v) for v in g[f"{tag}.seeds"])
    sd = W.make_tensors(W.vit_param_spec(**cfg), sw)
    video = W.make_volume(tuple(int(v) for v in g[f"{tag}.shape"]), sx)
    if tag == "neuro3d":
        video = ref_cpu.fmri_to_video(video)
    logits, target, dP = oracle_attention_grads(cfg, sd, video)
    assert np.abs(logits.numpy() - g[f"{tag}.logits"]).max() <= 1e-5
    assert np.array_equal(target.numpy(), g[f"{tag}.target"])
    for l in range(cfg["depth"]):
        want = g[f"{tag}.dP{l}"]
        assert want.dtype == np.float32 and want.shape == tuple(dP[l].shape)
        err = rel_l2(dP[l], want)
        print(f"{tag} layer {l}: oracle dOut V^T vs fixture rel L2 {err:.2e}")
        assert err <= 1e-5, (tag, l, err)
    if cfg.get("pool", "cls") == "cls":               # only the cls row of the last block reaches the head
        last = g[f"{tag}.dP{cfg['depth'] - 1}"]
        assert np.all(last[:, :, 1:] == 0) and np.abs(last[:, :, 0]).max() > 0


@pytest.mark.parametrize("tag,cfg", ALL_CASES, ids=[c[0] for c in ALL_CASES])
def test_relevance_row_vector_form_equals_the_matrix_form(golden, tag, cfg):
    """u <- u + u A_l (last layer first) is the row of R <- R + A_l R (R = I, first layer first) of the token the head reads"""
    g = golden("attention_grad.npz")
    A = layer_terms(g, tag, cfg["depth"])
    pool = cfg.get("pool", "cls")
    u = relevance_rows(A, pool)
    B, n = u.shape
    R = np.tile(np.eye(n), (B, 1, 1))
    for a in A:
        R = R + a @ R
    want = R.mean(axis=1) if pool == "mean" else R[:, 0]
    err = np.abs(u - want).max() / np.abs(want).max()
    assert err <= 1e-12, err
    assert np.abs(u[:, 1:] - g[f"{tag}.relevance"]).max() <= 1e-12
    assert (g[f"{tag}.relevance"] >= 0).all()


def test_attn_grad_struct_matches_the_header_and_the_revision_stays_8(tmp_path):
    from neurovit_amd import _cabi
    from neurovit_amd._cabi import HEADER, AttnGradExport
    lines = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{HEADER}"', 'int main(void) {',
             '  printf("size %zu\\n", sizeof(nv_vit_attn_grad_export));']
    for fname, _ in AttnGradExport._fields_:
        lines.append(f'  printf("{fname} %zu\\n", offsetof(nv_vit_attn_grad_export, {fname}));')
    lines += ['  printf("consts %d\\n", NV_ATTN_GRAD_PER_HEAD);', '  printf("consts2 %d\\n", NV_ATTN_GRAD_RELEVANCE);',
              '  printf("abi %d\\n", NV_ABI_VERSION);', '  return 0;', '}']
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-o", str(exe), str(src)], check=True)
    got = dict(l.split() for l in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split("\n") if l.strip())
    assert int(got["size"]) == ctypes.sizeof(AttnGradExport)
    for fname, _ in AttnGradExport._fields_:
        assert int(got[fname]) == getattr(AttnGradExport, fname).offset, fname
    assert [int(got["consts"]), int(got["consts2"])] == [_cabi.ATTN_GRAD_FORMS["per_head"], _cabi.ATTN_GRAD_FORMS["relevance"]]
    assert int(got["abi"]) == 8 and _cabi.ABI_VERSION == 8 and _cabi.lib.nv_abi_version() == 8
    dll = ctypes.CDLL(_cabi.LIB_PATH)
    for name in ("nv_attn_grad", "nv_attn_relevance", "nv_attn_relevance_workspace_bytes", "nv_vit_backward_attn"):
        assert name in _cabi.lib.protos, name            # declared in the header
        assert getattr(dll, name) is not None, name      # exported by the library
    # the new entry point takes nv_vit_backward_ex's arguments plus the export; the existing symbols keep their argument lists
    assert _cabi.lib.protos["nv_vit_backward_attn"][1][:-1] == _cabi.lib.protos["nv_vit_backward_ex"][1]
    assert len(_cabi.lib.protos["nv_attn_rollout"][1]) == 9


def test_argument_checks_without_a_gpu():
    from neurovit_amd import _cabi, engine
    from neurovit_amd._cabi import AttnGradExport, BackwardOpts, lib
    assert lib.nv_attn_relevance_workspace_bytes(4, 513) == 2 * 4 * 513 * 4
    assert lib.nv_attn_relevance_workspace_bytes(0, 513) < 0
    fake = 4096                                            # a non-null, 16-byte aligned address nothing dereferences: the checks come first
    assert lib.nv_attn_grad(None, 192, fake, 64, 1, 9, 1, 64, 0.125, 0, fake, None) == -1
    assert lib.nv_attn_grad(fake, 192, None, 64, 1, 9, 1, 64, 0.125, 0, fake, None) == -1
    assert lib.nv_attn_grad(fake, 192, fake, 64, 1, 9, 1, 64, 0.125, 0, None, None) == -1
    assert lib.nv_attn_grad(fake, 192, fake, 64, 1, 9, 1, 64, 0.125, 2, fake, None) == -1          # form out of range
    assert "form" in _cabi.last_error()
    assert lib.nv_attn_grad(fake, 192, fake, 64, 1, 9, 1, 60, 0.125, 0, fake, None) == -1          # dim_head not a multiple of 8
    assert lib.nv_attn_grad(fake, 128, fake, 64, 1, 9, 1, 64, 0.125, 0, fake, None) == -1          # ld_qkv does not cover q, k, v
    assert lib.nv_attn_relevance(None, 2, 1, 9, 0, fake, fake, 1 << 20, None) == -1
    ptrs = (ctypes.c_void_p * 2)(fake, None)
    assert lib.nv_attn_relevance(ctypes.cast(ptrs, ctypes.c_void_p), 2, 1, 9, 0, fake, fake, 1 << 20, None) == -1     # a NULL layer
    ptrs = (ctypes.c_void_p * 2)(fake, fake)
    assert lib.nv_attn_relevance(ctypes.cast(ptrs, ctypes.c_void_p), 2, 1, 9, 0, fake, fake, 8, None) == -1           # workspace too small

    cfg = engine.make_config(**W.MICRO)
    strides = (ctypes.c_long * 5)(1, 1, 1, 1, 1)
    maps = (ctypes.c_void_p * cfg.depth)(*([fake] * cfg.depth))
    opts = BackwardOpts(ctypes.sizeof(BackwardOpts), None, None, 0)

    def call(export, drop_p=0.0, video=fake):
        return lib.nv_vit_backward_attn(ctypes.byref(cfg), 1, video, strides, fake, fake, fake, 1 << 40, fake, None, None, 0, 0, cfg.depth + 1,
                                        drop_p, 0.0, 0, None, None, 1, 0, ctypes.byref(opts), None if export is None else ctypes.byref(export))
    good = AttnGradExport(ctypes.sizeof(AttnGradExport), ctypes.cast(maps, ctypes.c_void_p), 0)
    assert call(AttnGradExport(ctypes.sizeof(AttnGradExport) + 8, ctypes.cast(maps, ctypes.c_void_p), 0)) == -1
    assert "struct_size" in _cabi.last_error()
    assert call(AttnGradExport(ctypes.sizeof(AttnGradExport), None, 0)) == -1
    assert call(AttnGradExport(ctypes.sizeof(AttnGradExport), ctypes.cast(maps, ctypes.c_void_p), 2)) == -1
    assert call(good, drop_p=0.1) == -1
    assert "drop_p" in _cabi.last_error()
    assert call(good, video=None) == -1                    # the null-pointer check of the backward itself
    assert call(None, video=None) == -1
