"""CPU checks of the attention-probability export (no GPU): the reference-made fixture tests/golden/attention.npz against the oracle,
its rollout against a numpy restatement of the rule, and the C-ABI pieces the export adds (nv_vit_attn_export, revision 8)."""
import ctypes
import subprocess

import numpy as np
import pytest
import torch

import weights as W
from oracle import ref_cpu

P729 = dict(W.MICRO, image_size=27, image_patch_size=9, frames=27, frame_patch_size=9)
VIT_CASES = [("micro", W.MICRO), ("p729", P729), ("rect", W.RECT), ("noproj", W.NOPROJ), ("mean", dict(W.MICRO, pool="mean"))]
NEURO = dict(image_size=24, image_patch_size=8, frames=24, frame_patch_size=8, num_classes=2, dim=1024, depth=6, heads=8, mlp_dim=2048,
             channels=1, dim_head=64, pool="cls")


def oracle_cfg(cfgdict):
    v = dict(cfgdict)
    (H, Wd), (p1, p2) = (x if isinstance(x, tuple) else (x, x) for x in (v.pop("image_size"), v.pop("image_patch_size")))
    return ref_cpu.ViTCfg(image_size=H, image_patch_size=p1, image_width=Wd, patch_width=p2, **v)


def oracle_probs(cfgdict, sd, video):
    taps = {}
    with torch.no_grad():
        ref_cpu.vit_forward(sd, oracle_cfg(cfgdict), video, taps=taps)
    out = []
    for l in range(cfgdict["depth"]):
        q, k = taps[f"transformer.layers.{l}.0.q"].double(), taps[f"transformer.layers.{l}.0.k"].double()
        out.append(torch.softmax(q @ k.transpose(-1, -2) * cfgdict["dim_head"] ** -0.5, dim=-1).numpy())
    return out


def rollout(P, pool):
    B, n = P[0].shape[0], P[0].shape[-1]
    u = np.full((B, n), 1.0 / n) if pool == "mean" else np.tile(np.eye(n)[0], (B, 1))
    for p in P[::-1]:
        A = p.astype(np.float64).mean(axis=1)
        u = np.stack([u[b] @ ((A[b] + np.eye(n)) / (A[b].sum(axis=1, keepdims=True) + 1.0)) for b in range(B)])
    return u[:, 1:]


@pytest.mark.parametrize("tag,cfg", VIT_CASES + [("neuro3d", NEURO)], ids=[c[0] for c in VIT_CASES] + ["neuro3d"])
def test_fixture_against_the_oracle_and_its_rollout(golden, tag, cfg):
    g = golden("attention.npz")
    sw, sx = (int(v) for v in g[f"{tag}.seeds"])
    shape = tuple(int(v) for v in g[f"{tag}.shape"])
    sd = W.make_tensors(W.vit_param_spec(**cfg), sw)
    video = W.make_volume(shape, sx)
    if tag == "neuro3d":
        video = ref_cpu.fmri_to_video(video)              # [B, H, W, D] -> [B, 1, D, H, W], as ViT3DEncoder feeds it
    P = oracle_probs(cfg, sd, video)
    stored = [g[f"{tag}.P{l}"] for l in range(cfg["depth"])]
    for l in range(cfg["depth"]):
        assert stored[l].dtype == np.float32 and stored[l].shape == P[l].shape
        assert np.abs(stored[l] - P[l]).max() <= 1e-6, (tag, l)
    assert np.abs(rollout(stored, cfg.get("pool", "cls")) - g[f"{tag}.rollout"]).max() <= 1e-12


def test_rollout_rule_is_the_normalised_identity_augmented_head_mean(golden):
    """(A + I) / (rowsum(A) + 1) is the (A + I) / 2, row-renormalised rule of the widely used recipe when the rows of A sum to 1"""
    g = golden("attention.npz")
    P = [g[f"micro.P{l}"].astype(np.float64) for l in range(W.MICRO["depth"])]
    n = P[0].shape[-1]
    u = np.tile(np.eye(n)[0], (P[0].shape[0], 1))
    for p in P[::-1]:
        A = (p.mean(axis=1) + np.eye(n)) / 2
        A = A / A.sum(axis=-1, keepdims=True)
        u = np.einsum("bi,bij->bj", u, A)
    assert np.abs(u[:, 1:] - g["micro.rollout"]).max() <= 1e-6


def test_attn_export_struct_matches_the_header_and_revision_8(tmp_path):
    from neurovit_amd import _cabi
    from neurovit_amd._cabi import HEADER, AttnExport, VitInput
    structs = {"nv_vit_attn_export": AttnExport, "nv_vit_input": VitInput}
    lines = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{HEADER}"', 'int main(void) {']
    for cname, cls in structs.items():
        lines.append(f'  printf("{cname} size %zu\\n", sizeof({cname}));')
        for fname, _ in cls._fields_:
            lines.append(f'  printf("{cname} {fname} %zu\\n", offsetof({cname}, {fname}));')
    lines.append('  printf("consts %d %d %d %d %d %d\\n", NV_ATTN_PER_HEAD, NV_ATTN_FUSE_MEAN, NV_ATTN_FUSE_MAX, NV_ATTN_FUSE_MIN, '
                 'NV_ATTN_ROWS_ALL, NV_ATTN_ROWS_CLS);')
    lines += ['  return 0;', '}']
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-o", str(exe), str(src)], check=True)
    out = [l.split() for l in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split("\n") if l.strip()]
    got = {(l[0], l[1]): int(l[2]) for l in out if l[0] != "consts"}
    for cname, cls in structs.items():
        assert got[(cname, "size")] == ctypes.sizeof(cls), cname
        for fname, _ in cls._fields_:
            assert got[(cname, fname)] == getattr(cls, fname).offset, (cname, fname)
    consts = [int(v) for l in out if l[0] == "consts" for v in l[1:]]
    assert consts == [_cabi.ATTN_FUSIONS[k] for k in (None, "mean", "max", "min")] + [_cabi.ATTN_ROWS["all"], _cabi.ATTN_ROWS["cls"]]
    assert _cabi.ABI_VERSION == 8 and _cabi.lib.nv_abi_version() == 8
    for name in ("nv_attn_probs", "nv_attn_rollout", "nv_attn_rollout_workspace_bytes"):
        assert name in _cabi.lib.protos


def test_rollout_workspace_and_argument_checks_without_a_gpu():
    from neurovit_amd._cabi import lib
    assert lib.nv_attn_rollout_workspace_bytes(4, 513) == 2 * 4 * 513 * 4
    assert lib.nv_attn_rollout_workspace_bytes(0, 513) < 0
    # rejected before anything is launched
    assert lib.nv_attn_probs(0, None, 192, 1, 9, 1, 64, 0.125, 0, 0, None, None) == -1
    assert lib.nv_attn_probs(0, 16, 192, 1, 9, 1, 64, 0.125, 4, 0, 16, None) == -1            # fusion out of range
