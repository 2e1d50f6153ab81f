#!/usr/bin/env python3
"""Cost of the attention-gradient export and of the class-specific attention relevance through the native ViT3D (nv_attn_grad behind every
layer's attention backward, nv_attn_relevance): eval-mode forward (training layout) + data-only backward of a one-hot, timed with
device events, without an export against

    per_head    every layer's dP = dO V^T exported per head ([B, heads, n, n] fp32 each: what backward hooks on `attend` receive)
    relevance   every layer exported in the relevance form (mean_h relu(dP * P), [B, n, n])
    attention_relevance   ViT.attention_relevance (relevance-form export + nv_attn_relevance)

    python tools/attention_grad_bench.py --preset base --batch 4
    python tools/attention_grad_bench.py --preset reference --batch 32      # the reference's shipped config: 90^3, patch 9

Prints one JSON line: ms per forward + backward of each form, the added ms, the bytes the export writes and the MFMA work of the
relevance form (computed from the shapes below).
--trace: only a few iterations of each form, for `rocprofv3 --kernel-trace --stats -- python tools/attention_grad_bench.py --trace`;
--stats CSV [--steps N]: reads that run's kernel_stats.csv and reports the kernels' own time per layer against the per-head form's
byte floor (B heads n^2 4 bytes per layer at the achievable HBM rate) and the relevance form's MFMA floor.
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
MFMA_TFS = 2500.0      # dense bf16 / fp16 MFMA peak of the MI355X (TFLOP/s)


def tokens(cfg):
    return (cfg["image_size"] // cfg["image_patch_size"]) ** 2 * (cfg["frames"] // cfg["frame_patch_size"]) + 1


def layer_bytes(cfg, B):
    """bytes one layer's export writes"""
    n = tokens(cfg)
    per_head = 4.0 * B * cfg["heads"] * n * n
    return {"per_head": per_head, "relevance": per_head / cfg["heads"]}


def relevance_layer_flops(cfg, B):
    """MFMA work of one layer in the relevance form: Q K^T and dO V^T over all heads in the store pass (the statistics sweep repeats
    Q K^T once more per key split; not counted - the floor is the work the result needs)"""
    n = tokens(cfg)
    return 2 * 2.0 * B * cfg["heads"] * n * n * cfg["dim_head"]


def stats(path, cfg, B, steps):
    """the export kernels' time per form from a rocprofv3 kernel_stats.csv of a --trace run (steps iterations of each form)"""
    rows = list(csv.DictReader(open(path)))
    byts, L = layer_bytes(cfg, B), cfg["depth"]
    out = {"kernels": [{"kernel": r["Name"][:100], "calls": int(r["Calls"]), "avg_us": round(float(r["AverageNs"]) / 1e3, 2)}
                       for r in rows if "attn_grad16_kernel" in r["Name"] or "relevance_gemv" in r["Name"] or "attn_bwd" in r["Name"].lower()]}
    # the per-head instantiation (FORM = 0) by the last template argument of its name, mangled or demangled; the other is the relevance form
    per_head = re.compile(r"(Li0EEEv|, 0>\()")
    for form in ("per_head", "relevance"):
        sel = [r for r in rows if "attn_grad16_kernel" in r["Name"] and bool(per_head.search(r["Name"])) == (form == "per_head")]
        ns, calls = sum(float(r["TotalDurationNs"]) for r in sel), sum(int(r["Calls"]) for r in sel)
        if calls:
            t = ns / calls                                               # per layer
            out[f"{form}_layer_us"] = round(t / 1e3, 1)
            out[f"{form}_write_TBps"] = round(byts[form] / t / 1e3, 2)
            out[f"{form}_byte_floor_us"] = round(byts[form] / (HBM_TBS * 1e12) * 1e6, 1)
            if form == "relevance":
                fl = relevance_layer_flops(cfg, B)
                out["relevance_mfma_TFps"] = round(fl / t / 1e3, 1)
                out["relevance_mfma_floor_us"] = round(fl / (MFMA_TFS * 1e12) * 1e6, 1)
    sel = [r for r in rows if "relevance_gemv" in r["Name"]]
    if sel:
        out["relevance_gemv_layer_us"] = round(sum(float(r["TotalDurationNs"]) for r in sel) / sum(int(r["Calls"]) for r in sel) / 1e3, 1)
    out["layers"] = L
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--preset", default="base", choices=sorted(PRESETS))
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--trace", action="store_true", help="a few iterations of each form, nothing timed (run under rocprofv3)")
    ap.add_argument("--stats", help="kernel_stats.csv of a --trace run: report the export kernels' time, bandwidth and MFMA rate")
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
    model = ViT(**cfg).cuda().eval().requires_grad_(False)
    S, depth = cfg["image_size"], cfg["depth"]
    video = torch.randn(args.batch, S, S, S, device="cuda").permute(0, 3, 1, 2).unsqueeze(1)
    model.check_video(video)
    rt = model._rt

    def plain():
        """what attention_gradients runs, without the export: training-layout forward + data-only backward of the layers"""
        logits = model._run_forward(video, True)
        dlogits = torch.nn.functional.one_hot(logits.argmax(dim=1), cfg["num_classes"]).float()
        rt.backward(dlogits, model._arena, model._shadow, None, accumulate=False, stages=(0, depth), weight_grads=False, final=True)

    forms = {
        "plain": plain,
        "per_head": lambda: model.attention_gradients(video),
        "relevance": lambda: model.attention_gradients(video, form="relevance"),
        "attention_relevance": lambda: model.attention_relevance(video),
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

    out = {"preset": args.preset, "batch": args.batch, "tokens": tokens(cfg), "layers": depth, "steps": args.steps, "repeats": args.repeats}
    base = timed(forms["plain"])
    out["plain_ms"] = round(base, 4)
    byts = layer_bytes(cfg, args.batch)
    for form in ("per_head", "relevance", "attention_relevance"):
        ms = timed(forms[form])
        out[f"{form}_ms"] = round(ms, 4)
        out[f"{form}_added_ms"] = round(ms - base, 4)
        out[f"{form}_added_us_per_layer"] = round((ms - base) * 1e3 / depth, 1)
    out["per_head_export_MB"] = round(byts["per_head"] * depth / 1e6, 1)
    out["relevance_export_MB"] = round(byts["relevance"] * depth / 1e6, 1)
    out["per_head_byte_floor_us_per_layer"] = round(byts["per_head"] / (HBM_TBS * 1e12) * 1e6, 1)
    out["relevance_mfma_floor_us_per_layer"] = round(relevance_layer_flops(cfg, args.batch) / (MFMA_TFS * 1e12) * 1e6, 1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
