#!/usr/bin/env python3
"""Cost of the attention-probability export and of attention rollout through the native ViT3D (nv_attn_probs behind every attention
launch, nv_attn_rollout): eval-mode no-grad forwards, timed with device events, without an export against

    per_head   every layer exported per head, all rows ([B, heads, n, n] fp32 each: what hooks on `attend` receive)
    mean       every layer exported head-fused (mean, [B, n, n])
    rollout    ViT.attention_rollout (mean-fused export + nv_attn_rollout)

    python tools/attention_maps_bench.py --preset base --batch 4
    python tools/attention_maps_bench.py --preset reference --batch 32      # the reference's shipped config: 90^3, patch 9

Prints one JSON line: ms per forward of each form, the added ms, the bytes the export writes and the write bandwidth that added time
implies (a lower bound on what the kernels achieve: the added time also holds their read of qkv and their launch gaps).
--trace: only a few iterations of each form, for `rocprofv3 --kernel-trace --stats -- python tools/attention_maps_bench.py --trace`;
--stats CSV [--steps N]: reads that run's kernel_stats.csv and reports the export kernels' own time against their written bytes.
"""
import argparse
import csv
import json
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PRESETS = {
    "base": dict(image_size=128, image_patch_size=16, frames=128, frame_patch_size=16, num_classes=2, dim=768, depth=12, heads=12,
                 mlp_dim=3072, channels=1, dim_head=64),
    "reference": dict(image_size=90, image_patch_size=9, frames=90, frame_patch_size=9, num_classes=2, dim=1024, depth=6, heads=8,
                      mlp_dim=2048, channels=1, dim_head=64),
}
HBM_TBS = 6.3          # achievable HBM bandwidth of the MI355X (TB/s)


def tokens(cfg):
    return (cfg["image_size"] // cfg["image_patch_size"]) ** 2 * (cfg["frames"] // cfg["frame_patch_size"]) + 1


def export_bytes(cfg, B):
    n = tokens(cfg)
    per_head = 4.0 * B * cfg["heads"] * n * n * cfg["depth"]
    return {"per_head": per_head, "mean": per_head / cfg["heads"], "rollout": per_head / cfg["heads"]}


def stats(path, cfg, B, steps):
    """export kernels' time per form from a rocprofv3 kernel_stats.csv of a --trace run (steps forwards of each form)"""
    rows = list(csv.DictReader(open(path)))
    byts = export_bytes(cfg, B)
    out = {}
    for key, tag in (("attn_probs16_kernel", "export"), ("rollout_", "rollout_kernels")):
        sel = [r for r in rows if key in r["Name"]]
        out[tag] = [{"kernel": r["Name"][:90], "calls": int(r["Calls"]), "avg_us": round(float(r["AverageNs"]) / 1e3, 2),
                     "total_us_per_step": round(float(r["TotalDurationNs"]) / 1e3 / steps, 1)} for r in sel]
    # per_head (FUSE = 0) and fused-mean (FUSE = 1) instantiations: the last template argument of the kernel's name
    for form, fuse in (("per_head", 0), ("mean", 1)):
        last = re.compile(rf"(Li{fuse}EEEv|, {fuse}>\()")                 # mangled or demangled name
        ns = sum(float(r["TotalDurationNs"]) for r in rows if "attn_probs16_kernel" in r["Name"] and last.search(r["Name"]))
        if ns:
            steps_form = 2 * steps if form == "mean" else steps        # the rollout form runs the mean export as well
            t = ns / steps_form
            out[f"{form}_kernel_us"] = round(t / 1e3, 1)
            out[f"{form}_write_TBps"] = round(byts[form] / t / 1e3, 2)
            out[f"{form}_of_hbm"] = round(byts[form] / t / 1e3 / HBM_TBS, 3)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--preset", default="base", choices=sorted(PRESETS))
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--trace", action="store_true", help="a few iterations of each form, nothing timed (run under rocprofv3)")
    ap.add_argument("--stats", help="kernel_stats.csv of a --trace run: report the export kernels' time and bandwidth")
    args = ap.parse_args()
    cfg = PRESETS[args.preset]
    if args.stats:
        print(json.dumps({"preset": args.preset, "batch": args.batch, **stats(args.stats, cfg, args.batch, args.steps)}))
        return

    import torch
    from neurovit_amd._cabi import require_gpu
    from neurovit_amd.vit_3d import ViT
    require_gpu()
    torch.manual_seed(0)
    model = ViT(**cfg).cuda().eval()
    S = cfg["image_size"]
    video = torch.randn(args.batch, S, S, S, device="cuda").permute(0, 3, 1, 2).unsqueeze(1)
    forms = {
        "plain": lambda: model(video),
        "per_head": lambda: model.attention_maps(video),
        "mean": lambda: model.attention_maps(video, head_fusion="mean"),
        "rollout": lambda: model.attention_rollout(video),
    }
    if args.trace:
        with torch.no_grad():
            for fn in forms.values():
                for _ in range(args.steps):
                    fn()
            torch.cuda.synchronize()
        print(json.dumps({"trace": True, "steps_per_form": args.steps}))
        return

    def timed(fn):
        with torch.no_grad():
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
        return sorted(times)[len(times) // 2]

    out = {"preset": args.preset, "batch": args.batch, "tokens": tokens(cfg), "steps": args.steps, "repeats": args.repeats}
    base = timed(forms["plain"])
    out["plain_ms"] = round(base, 4)
    byts = export_bytes(cfg, args.batch)
    for form in ("per_head", "mean", "rollout"):
        ms = timed(forms[form])
        out[f"{form}_ms"] = round(ms, 4)
        out[f"{form}_added_ms"] = round(ms - base, 4)
        out[f"{form}_export_MB"] = round(byts[form] / 1e6, 1)
        if form != "rollout" and ms > base:
            out[f"{form}_implied_write_TBps"] = round(byts[form] / ((ms - base) * 1e-3) / 1e12, 2)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
