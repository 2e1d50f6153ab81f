#!/usr/bin/env python3
"""Volumes/s of forward + backward for the gradient w.r.t. the input volume (saliency, integrated gradients, captum), through the
native ViT3D: a TRAINABLE model (parameter gradients are produced as well, the full backward + nv_patch_ln_dx) against a FROZEN one
(requires_grad_(False): the data-only backward, no gradient arena).  For reference, the plain training forward + backward of the same
batch without an input gradient.

    python tools/input_grad_bench.py --preset base --batch 4
    python tools/input_grad_bench.py --preset reference --batch 128      # the reference's shipped config: 90^3, patch 9

Prints one JSON line.  Timing: CUDA events around `--steps` iterations after `--warmup`, the median of `--repeats` such windows.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

PRESETS = {
    "base": dict(image_size=128, image_patch_size=16, frames=128, frame_patch_size=16, num_classes=2, dim=768, depth=12, heads=12,
                 mlp_dim=3072, channels=1, dim_head=64),
    "reference": dict(image_size=90, image_patch_size=9, frames=90, frame_patch_size=9, num_classes=2, dim=1024, depth=6, heads=8,
                      mlp_dim=2048, channels=1, dim_head=64),
}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--preset", default="base", choices=sorted(PRESETS))
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--operands", default="bf16", choices=["bf16", "fp16"])
    args = ap.parse_args()

    from neurovit_amd._cabi import require_gpu
    from neurovit_amd.vit_3d import ViT
    require_gpu()
    cfg = PRESETS[args.preset]
    torch.manual_seed(0)
    model = ViT(**cfg).cuda().train().set_operands(args.operands)
    S = cfg["image_size"]
    fmri = torch.randn(args.batch, S, S, S, device="cuda")

    def step_input(x):
        logits = model(x.permute(0, 3, 1, 2).unsqueeze(1))
        (g,) = torch.autograd.grad(logits[:, 0].sum(), x)
        return g

    def step_params():
        model(fmri.permute(0, 3, 1, 2).unsqueeze(1))[:, 0].sum().backward()

    def timed(fn):
        for _ in range(args.warmup):
            fn()
        torch.cuda.synchronize()
        times = []
        for _ in range(args.repeats):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(args.steps):
                fn()
            b.record()
            torch.cuda.synchronize()
            times.append(a.elapsed_time(b) / args.steps)
        ms = sorted(times)[len(times) // 2]
        return {"ms": round(ms, 4), "volumes_per_s": round(args.batch / ms * 1e3, 1)}

    x = fmri.clone().requires_grad_(True)
    out = {"preset": args.preset, "batch": args.batch, "operands": args.operands, "steps": args.steps, "repeats": args.repeats}
    model.requires_grad_(True)
    out["train_fwd_bwd_no_input_grad"] = timed(step_params)
    out["trainable_fwd_input_grad"] = timed(lambda: step_input(x))
    model.zero_grad(set_to_none=True)
    model.requires_grad_(False)
    out["frozen_fwd_input_grad"] = timed(lambda: step_input(x))
    out["frozen_over_trainable"] = round(out["frozen_fwd_input_grad"]["volumes_per_s"] / out["trainable_fwd_input_grad"]["volumes_per_s"], 3)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
